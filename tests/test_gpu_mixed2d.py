"""Mixed-width fused 2-D kernels (kernel_stream2d with `mixed`; kernel.generate's
`mixed_widths`) on a real MI355X, all through the C ABI from `<app>.mw.hsaco`: the reference's
fixtures array for array, shapes taken from each entry's own constants - the output's box
against the oracle, the whole array against the per-stage run -, the sweep's memory contract
in guarded arenas, full-width operands, the run-time compile with the switch and the
generated `<app>_test`.  Every comparison is of bytes (tests/switch_form_gpu.py).

mask2d, two inputs of one width and different types, runs its fused kernel from the DEFAULT
blob: the reference's fixtures and the oracle on a ragged shape.

The shared harness's guarded runs and full-width run place and type every array by input 0's
element (test_gpu_memory_contract.skews_for, switch_form_gpu.full_width_operands); the
arrays of these programs differ in width, so held() and the full-width test here place each
array by its OWN element size: the pool placement puts array i at (its size + 16 i) bytes
into a 64-byte piece - a uint8 array at 1, 17, 33 bytes, aligned to its element only."""
import functools
import json
import os

import numpy as np
import pytest

from soda_hip.codegen import kernel, switches
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
import switch_form_gpu as harness
from test_gpu_memory_contract import box_of

pytestmark = pytest.mark.gpu

APPS = ('edge8f', 'tone16', 'quant2d', 'dsum2d')
# the programs that cast a float to an integer, and the range of the cast's target
CASTS_TO = {'tone16': (0, 255), 'quant2d': (0, 65535)}

FORM = harness.Form(
    keyword='mixed_widths', family='mixed2d', fixtures=lambda app: 6,
    kernels=lambda spec: [('%s_fused_k1' % spec['app_name'], 1)],
    limit=lambda spec: 0, margins=harness.lowered_hull_margins)



def _shapes_taken(app):
  """The lane shapes of kernel.mixed_shapes the register estimate takes, narrowest first."""
  spec = gpu_util.load_spec(app)
  return [c for c in sorted(kernel.mixed_shapes(spec))
          if kernel.generate(spec, mixed_widths=True, cols=c)[1][-1]['kind'] == 'fused']


def _shipped(app):
  return kernel.generate(gpu_util.load_spec(app), mixed_widths=True)[1][-1]['cols']


# every lane shape besides the one the prebuilt blob has: edge8f at 8 and 16 columns and
# dsum2d at 4 store a lane's row in two to four 16-byte pieces, which no shipped shape does
OTHER_SHAPES = [(app, c) for app in APPS for c in _shapes_taken(app) if c != _shipped(app)]
assert OTHER_SHAPES == [('edge8f', 8), ('edge8f', 16), ('quant2d', 8), ('dsum2d', 4)]

opened = functools.partial(harness.opened, FORM)
check_shape = functools.partial(harness.check_shape, FORM)
fused_of = functools.partial(harness.fused_of, FORM)
shapes_of = functools.partial(harness.shapes_of, FORM)


def skews_of(mode, dtypes):
  """Start offsets within a 64-byte piece, per array by its own element size."""
  if mode == 'pool':
    return [(dt.itemsize + 16 * i) % gpu_util.ARENA_PIECE for i, dt in enumerate(dtypes)]
  assert mode == 'sixteen'
  return [(16 * (i + 1)) % gpu_util.ARENA_PIECE for i in range(len(dtypes))]


def shifted(a, dx, dy):
  """a(dx, dy) of the DSL as an array: cell (y, x) holds a[y + dy, x + dx]; what wraps round
  lies outside every box."""
  return np.roll(a, (-dy, -dx), axis=(0, 1))


def cast_argument(app, inputs):
  """The float value a sample clamps before it casts it to an integer, evaluated from the
  inputs in the sample's own order and precision (float32, no contraction)."""
  f = np.float32
  with np.errstate(all='ignore'):
    if app == 'tone16':
      (img,) = [a.astype(f) for a in inputs]
      bx = f(0.25) * shifted(img, -1, 0) + f(0.5) * img + f(0.25) * shifted(img, 1, 0)
      by = f(0.25) * shifted(bx, 0, -1) + f(0.5) * bx + f(0.25) * shifted(bx, 0, 1)
      return (by + shifted(by, 1, 0)) * f(0.001953125)
    assert app == 'quant2d'
    img, gain = inputs[0], inputs[1].astype(f)
    return (img + f(0.5) * (shifted(img, -1, 0) + shifted(img, 1, 1))) * \
        shifted(gain, 0, -1) * f(100.0)


def check_cast_is_defined(app, inputs, want, sl):
  """On the box: the clamped value - fmax drops a NaN, fmin caps - lies within the target's
  range, and truncated it IS the oracle's output, so this is the value the oracle cast."""
  lo, hi = CASTS_TO[app]
  assert (np.iinfo(want.dtype).min, np.iinfo(want.dtype).max) == (lo, hi)
  arg = cast_argument(app, inputs).astype(np.float64)[sl]
  clamped = np.fmin(np.fmax(arg, 0.0), float(hi))
  assert not np.isnan(clamped).any() and clamped.min() >= lo and clamped.max() <= hi
  assert np.array_equal(np.trunc(clamped).astype(want.dtype), want[sl])
  return arg


def held(prog, orc, k, shape, mode, inputs=None):
  """One guarded run of one iteration in the default schedule: the launch is `k`, the box
  equals the oracle byte for byte, guards intact, inputs unchanged."""
  spec = prog.spec
  dims = tuple(reversed(shape))
  if inputs is None:
    inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
  assert [e['name'] for e, _ in prog.schedule(dims, 1)] == [k['name']]
  skews = skews_of(mode, list(prog.in_dtypes) + list(prog.out_dtypes))
  if mode == 'pool':
    assert all(s % 16 for s in skews)
  outs, bad, timing = gpu_util.run_guarded(prog, inputs, 1, skews=skews)
  assert timing['max_depth'] == 1
  want = orc.run(inputs, iterate=1)
  (name,) = spec['outputs']
  lo, hi = box_of(spec, name, dims, 1)
  sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
  g, w = np.ascontiguousarray(outs[0][sl]), np.ascontiguousarray(want[name][sl])
  assert g.size > 0
  differ = np.argwhere(g.view(np.uint8) != w.view(np.uint8))
  assert differ.size == 0, ('%d bytes of the box differ, first at %s' % (len(differ), differ[0]),
                            spec['app_name'], shape, mode)
  assert bad == [], (bad, spec['app_name'], shape, mode)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  harness.fixtures(FORM, app)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """The kernel on every shape of shapes_of: a one-cell box, one strip plus one column, two
  shortest chunks less a row, two workgroup tiles plus 37 columns by 60 rows."""
  prog, orc = opened(app)
  (k,) = fused_of(prog)
  for shape in shapes_of(k, prog.spec, 1):
    assert shape[0] * shape[1] <= 10000 * 70
    check_shape(prog, orc, shape, 1)


@pytest.mark.parametrize('app', APPS)
def test_memory_contract(app):
  """The ragged shape from the pool allocator's placement - every array aligned to its own
  element only - and from multiples of 16 bytes."""
  prog, orc = opened(app)
  (k,) = fused_of(prog)
  shape = shapes_of(k, prog.spec, 1)[-1]
  for mode in ('pool', 'sixteen'):
    held(prog, orc, k, shape, mode)


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """Every bit of every input's element, mixed signs and exponents (gpu_util.wide_inputs).
  The oracle's values on the box are finite, and where the program casts a float to an
  integer the value cast is within the target's range: the clamped argument is evaluated
  from the inputs and held to the range and to the oracle's output (check_cast_is_defined)
  before bytes are compared."""
  prog, orc = opened(app)
  spec = prog.spec
  (k,) = fused_of(prog)
  shape = harness.wide_shape_of(FORM, k, spec, 1)
  inputs = gpu_util.wide_inputs(spec, shape)
  want = orc.run(inputs, iterate=1)
  (name,) = spec['outputs']
  _, _, sl = harness.slices_of(spec, name, shape, 1)
  assert want[name][sl].size > 0 and np.isfinite(want[name][sl]).all()
  if app in CASTS_TO:
    check_cast_is_defined(app, inputs, want[name], sl)
  held(prog, orc, k, shape, 'pool', inputs)


@pytest.mark.parametrize('app,cols', OTHER_SHAPES)
def test_every_other_lane_shape(app, cols):
  """The lane shapes the prebuilt blob does not have, compiled at run time with `cols`: the
  shapes of shapes_of against the oracle and the per-stage run, the ragged shape in guarded
  arenas from both placements, and full-width operands - the same byte comparisons as the
  shipped shape's."""
  spec = gpu_util.load_spec(app)
  text, table = kernel.generate(spec, mixed_widths=True, cols=cols)
  orc = gpu_util.make_oracle(spec)
  prog = host.open_program(source=text, spec=spec)
  try:
    assert prog.kernels == table
    (k,) = fused_of(prog)
    assert k['cols'] == cols
    shapes = shapes_of(k, spec, 1)
    for shape in shapes:
      assert shape[0] * shape[1] <= 10000 * 70
      check_shape(prog, orc, shape, 1)
    for mode in ('pool', 'sixteen'):
      held(prog, orc, k, shapes[-1], mode)
    shape = harness.wide_shape_of(FORM, k, spec, 1)
    inputs = gpu_util.wide_inputs(spec, shape)
    if app in CASTS_TO:
      (name,) = spec['outputs']
      _, _, sl = harness.slices_of(spec, name, shape, 1)
      check_cast_is_defined(app, inputs, orc.run(inputs, iterate=1)[name], sl)
    held(prog, orc, k, shape, 'pool', inputs)
  finally:
    prog.close()
    prog.blob.unload()


def test_run_time_compile_with_the_switch():
  harness.run_time_compile(FORM, 'edge8f', 1, ['stage', 'stage'])


@pytest.mark.parametrize('app', APPS)
def test_the_generated_test_passes_with_the_switch(app):
  prog, _ = opened(app)
  assert switches.depth_limit_of(prog.spec, dict(mixed_widths=True)) == (0, [])
  blob = os.path.join(gpu_util.BLOBS, app + '.mw.hsaco')
  assert host.app_test(prog.spec, blob, [301, 53, 0, 0], iterate=1, mixed_widths=True) == 0


# ---- two inputs of one width and different types: the default blob -------------------------------

def test_mask2d_from_the_default_blob():
  """float and int32 inputs: the fused kernel of the default schedule against the
  reference's fixtures, and against the oracle and the per-stage run on a ragged shape."""
  prog = gpu_util.open_prebuilt('mask2d')
  spec = prog.spec
  try:
    (k,) = [e for e in prog.kernels if e['kind'] == 'fused']
    assert k['name'] == 'mask2d_fused_k1'
    with open(os.path.join(harness.GOLDEN, 'mixed2d_manifest.json')) as f:
      manifest = json.load(f)
    n = 0
    for fx, meta in sorted(manifest.items()):
      if not meta['key'].startswith('mask2d.'):
        continue
      data = np.load(os.path.join(harness.GOLDEN, 'mixed2d', fx))
      inputs = [data['in_' + t['name']] for t in spec['inputs']]
      dims = tuple(reversed(inputs[0].shape))
      assert [e['name'] for e, _ in prog.schedule(dims, 1)] == [k['name']]
      (got,) = prog.run_numpy(inputs, iterate=1)
      assert np.array_equal(got.view(np.uint8), data['out_out'].view(np.uint8)), fx
      n += 1
    assert n == 6
    orc = gpu_util.make_oracle(spec)
    mx, my = harness.box_margins(spec, 1)
    shape = (my + 60, 2 * k['tile'][0] + 37 + mx)
    inputs = gpu_util.wide_inputs(spec, shape)
    want = orc.run(inputs, iterate=1)['out']
    _, _, sl = harness.slices_of(spec, 'out', shape, 1)
    assert np.isfinite(want[sl]).all()
    assert [e['name'] for e, _ in prog.schedule(tuple(reversed(shape)), 1)] == [k['name']]
    (got,) = prog.run_numpy(inputs, iterate=1)
    assert np.array_equal(np.ascontiguousarray(got[sl]).view(np.uint8),
                          np.ascontiguousarray(want[sl]).view(np.uint8))
    prog.set_max_depth(-1)
    assert all(e['kind'] == 'stage' for e, _ in prog.schedule(tuple(reversed(shape)), 1))
    (staged,) = prog.run_numpy(inputs, iterate=1)
    assert np.array_equal(got.view(np.uint8), staged.view(np.uint8))
  finally:
    prog.set_max_depth(0)
    prog.close()
