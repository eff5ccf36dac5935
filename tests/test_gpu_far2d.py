"""Far-lane 2-D kernels (kernel_stream2d / kernel_fields2d with `hops`; kernel.generate's
`far_lanes`) on a real MI355X, all through the C ABI from `<app>.far.hsaco`: the reference's
fixtures array for array, shapes taken from each entry's own constants - every output on its
own box against the oracle, the whole arrays against the per-stage run -, the sweep's memory
contract in guarded arenas, full-width operands, and the run-time compile with the switch.
Every comparison is of bytes.

star2d, dstar2d and skewfar2d run their fused kernels in the default schedule.  acoustic2d's
are kernels over several fields, which the launcher admits only under a positive depth limit
(csrc/schedule.cpp, plans_fused - as for wave2d and every other multi-field program): every
entry point generated with the switch sets that limit (switches.depth_limit_of), and the
fused runs here are those under the same limit, from the same function."""
import json
import os

import numpy as np
import pytest

from soda_hip.codegen import kernel, switches
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
from test_gpu_memory_contract import box_of, hold

pytestmark = pytest.mark.gpu

APPS = ('star2d', 'dstar2d', 'skewfar2d', 'acoustic2d')
DEPTHS = {'star2d': [1, 2], 'dstar2d': [1, 2, 4], 'skewfar2d': [1, 2], 'acoustic2d': [1, 2]}
CHUNK_ROWS_MIN = 8
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'far2d_manifest.json')) as _f:
  MANIFEST = json.load(_f)

_CACHE = {}


def opened(app):
  """(program from the prebuilt code object generated with far_lanes=True, oracle)"""
  if app not in _CACHE:
    spec = gpu_util.load_spec(app)
    path = os.path.join(gpu_util.BLOBS, app + '.far.hsaco')
    assert os.path.exists(path), '%s missing: run __graft_entry__.build()' % path
    prog = host.open_program(blob=path, spec=spec)
    _CACHE[app] = (prog, gpu_util.make_oracle(spec))
  return _CACHE[app]


def fused_of(prog):
  fused = [k for k in prog.kernels if k['kind'] == 'fused']
  app = prog.spec['app_name']
  assert [k['name'] for k in fused] == ['%s_fused_k%d' % (app, d) for d in DEPTHS[app]]
  assert max(k['halo'][0] for k in fused) > fused[0]['cols']     # a halo wider than one lane
  return fused


def limit_of(prog):
  """The depth limit of a fused run, as the entry points of a `--hip-far-lanes` product set
  it: none (the default schedule) for the single-array programs, the deepest kernel's for
  the one over fields."""
  limit, _ = switches.depth_limit_of(prog.spec, dict(far_lanes=True))
  assert limit == (max(DEPTHS['acoustic2d']) if len(prog.spec['outputs']) > 1 else 0)
  return limit


def margins(spec, iterate):
  lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), iterate)[-1]
  return [a + b for a, b in zip(lo, hi)]


def fused_and_staged(prog, inputs, iterate, depth=None):
  """The arrays of the fused schedule - every launch one of the far-lane kernels; `depth`:
  the split fixed to launches of that depth - and the per-stage run's."""
  dims = tuple(reversed(inputs[0].shape))
  stages = [k['name'] for k in prog.kernels if k['kind'] == 'stage']
  try:
    prog.set_max_depth(limit_of(prog))
    if depth is not None:
      assert iterate % depth == 0
      prog.set_split(dims, iterate, [depth] * (iterate // depth))
    launched = [k for k, _ in prog.schedule(dims, iterate)]
    assert all(k['kind'] == 'fused' for k in launched), [k['name'] for k in launched]
    assert sum(k['depth'] for k in launched) == iterate
    if depth is not None:
      assert [k['depth'] for k in launched] == [depth] * (iterate // depth)
    got = prog.run_numpy(inputs, iterate=iterate)
    if depth is not None:
      prog.set_split(dims, iterate, [])
    prog.set_max_depth(-1)
    assert [k['name'] for k, _ in prog.schedule(dims, iterate)] == stages * iterate
    staged = prog.run_numpy(inputs, iterate=iterate)
  finally:
    prog.set_max_depth(0)
  return got, staged


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  """The whole arrays equal the reference's: each output on its box, zero outside; the same
  arrays per stage."""
  prog, _ = opened(app)
  spec = prog.spec
  fused_of(prog)
  n = 0
  for fx, meta in sorted(MANIFEST.items()):
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'far2d', fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    got, staged = fused_and_staged(prog, inputs, meta['iterate'])
    for name, g, s in zip(spec['outputs'], got, staged):
      want = data['out_' + name]
      assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (fx, name)
      assert np.array_equal(s.view(np.uint8), want.view(np.uint8)), (fx, name, 'per stage')
    n += 1
  assert n == 4 * (2 if app == 'skewfar2d' else 3)


def shapes_of(k, spec, iterate):
  """(y, x) from the entry's own constants: an intersection box of one cell; one strip plus
  one column with fewer rows than fill_rows + 1; two of the shortest chunks less one row, a
  few cells wide; two workgroup tiles plus 37 columns by 60 rows - strips whose halo lanes,
  more than one per side, hang over both ends of the rows, chunks whose fill rows are
  clamped at the top and at the bottom."""
  mx, my = margins(spec, iterate)
  assert k['fill_rows'] >= 2 and k['tile'][0] == 4 * k['w_out']
  return [(my + 1, mx + 1),
          (my + k['fill_rows'] - 1, k['w_out'] + 1 + mx),
          (my + 2 * CHUNK_ROWS_MIN - 1, mx + 5),
          (my + 60, 2 * k['tile'][0] + 37 + mx)]


def check_shape(prog, orc, shape, iterate, depth):
  spec = prog.spec
  dims = tuple(reversed(shape))
  inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
  want = orc.run(inputs, iterate=iterate)
  got, staged = fused_and_staged(prog, inputs, iterate, depth)
  for name, g, s in zip(spec['outputs'], got, staged):
    lo, hi = box_of(spec, name, dims, iterate)
    if name == 'pc' and iterate == 1:      # handed on: the whole array
      assert lo == [0, 0] and hi == list(dims)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert g[sl].size > 0, (name, shape, iterate)
    assert np.array_equal(np.ascontiguousarray(g[sl]).view(np.uint8),
                          np.ascontiguousarray(want[name][sl]).view(np.uint8)), \
        (name, shape, iterate, depth)
    assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (name, shape, iterate, depth)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every kernel of the table on every shape of shapes_of, as many iterations as it fuses."""
  prog, orc = opened(app)
  for k in fused_of(prog):
    for shape in shapes_of(k, prog.spec, k['depth']):
      assert shape[0] * shape[1] <= 2100 * 130
      check_shape(prog, orc, shape, k['depth'], k['depth'])


@pytest.mark.parametrize('app', APPS)
def test_the_schedule_mixes_depths(app):
  """One iteration more than the deepest kernel fuses: the sweep ends in a shallower kernel,
  on the ragged shape."""
  prog, orc = opened(app)
  deep = fused_of(prog)[-1]
  iterate = deep['depth'] + 1
  check_shape(prog, orc, shapes_of(deep, prog.spec, iterate)[-1], iterate, None)


@pytest.mark.parametrize('app', APPS)
def test_memory_contract(app):
  """gpu_util.run_guarded on the ragged shape with the deepest kernel, from the pool
  allocator's placement and from multiples of 16 bytes: every output's box equals the
  oracle, guards intact, inputs unchanged."""
  prog, orc = opened(app)
  deep = fused_of(prog)[-1]
  shape = shapes_of(deep, prog.spec, deep['depth'])[-1]
  prog.set_max_depth(limit_of(prog))
  try:
    for mode in ('pool', 'sixteen'):
      launched = hold(prog, orc, shape, deep['depth'], mode, 'stream', deep['depth'],
                      split=[deep['depth']])
      assert [k['name'] for k in launched] == [deep['name']]
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """Mixed signs and exponents over the element's whole mantissa (gpu_util.wide_inputs at
  the default span), in float (star2d, skewfar2d) and in double (dstar2d, acoustic2d), two
  iterations in the depth-2 kernel.  The oracle's values on every output's box are finite:
  no NaN payload enters the byte comparison."""
  prog, orc = opened(app)
  spec = prog.spec
  assert spec['inputs'][0]['c_type'] == ('double' if app in ('dstar2d', 'acoustic2d')
                                         else 'float')
  k = fused_of(prog)[1]
  assert k['depth'] == 2
  mx, my = margins(spec, 2)
  shape = (my + 23, k['tile'][0] + 35 + mx)
  inputs = gpu_util.wide_inputs(spec, shape)
  want = orc.run(inputs, iterate=2)
  for name in spec['outputs']:
    lo, hi = box_of(spec, name, tuple(reversed(shape)), 2)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert want[name][sl].size > 0 and np.isfinite(want[name][sl]).all(), name
  prog.set_max_depth(limit_of(prog))
  try:
    launched = hold(prog, orc, shape, 2, 'pool', 'stream', 2, split=[2], inputs=inputs)
    assert [k['name'] for k in launched] == [k['name']]
  finally:
    prog.set_max_depth(0)


def test_the_products_limit_admits_the_kernels_over_fields():
  """What a `--hip-far-lanes` product of acoustic2d runs: under the limit its entry points
  set, every launch is one of the far-lane kernels - without it the launcher keeps a program
  over several fields per stage -, and the generated `<app>_test` passes with the switch."""
  prog, _ = opened('acoustic2d')
  spec = prog.spec
  limit, flags = switches.depth_limit_of(spec, dict(far_lanes=True))
  assert (limit, flags) == (2, ['--hip-far-lanes'])
  dims = (301, 53)
  try:
    prog.set_max_depth(limit)
    assert [k['name'] for k, _ in prog.schedule(dims, 3)] == [
        'acoustic2d_fused_k2', 'acoustic2d_fused_k1']
    prog.set_max_depth(0)
    assert all(k['kind'] == 'stage' for k, _ in prog.schedule(dims, 3))
  finally:
    prog.set_max_depth(0)
  blob = os.path.join(gpu_util.BLOBS, 'acoustic2d.far.hsaco')
  assert host.app_test(spec, blob, [301, 53, 0, 0], iterate=3, far_lanes=True) == 0


def test_run_time_compile_with_the_switch():
  """host.open_program(spec=..., far_lanes=True): the offline build's table, the blob's bytes
  on the ragged shape; without the switch the per-stage kernels only."""
  spec = gpu_util.load_spec('skewfar2d')
  blob_prog, orc = opened('skewfar2d')
  prog = host.open_program(spec=spec, far_lanes=True)
  try:
    assert prog.kernels == kernel.generate(spec, far_lanes=True)[1]
    assert prog.kernels == blob_prog.kernels
    shape = shapes_of(fused_of(prog)[-1], spec, 2)[-1]
    check_shape(prog, orc, shape, 2, 2)
    inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
    got, _ = fused_and_staged(prog, inputs, 2)
    same, _ = fused_and_staged(blob_prog, inputs, 2)
    for g, s in zip(got, same):
      assert np.array_equal(g.view(np.uint8), s.view(np.uint8))
  finally:
    prog.close()
    prog.blob.unload()
  plain = host.open_program(spec=spec)
  try:
    assert [k['kind'] for k in plain.kernels] == ['stage', 'stage']
  finally:
    plain.close()
    plain.blob.unload()
