"""LDS plane-ring kernels (soda_hip/codegen/kernel_stream3d_lds.py with ring=True) on a real
MI355X, all through the C ABI from `<app>.ldsr.hsaco` under a depth limit of 1: the
reference's fixtures array for array, shapes taken from the entry's own constants - every
output on its own box against the oracle, the whole arrays against the per-stage run -, box
depths at which the plane loop leaves at every unrolled step, two iterations, the sweep's
memory contract in guarded arenas, full-width operands, and the run-time compile with the
switch.  Every comparison is of bytes."""
import json
import os

import numpy as np
import pytest

from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
from test_gpu_lds3d import SHORTEST_CHUNK
from test_gpu_memory_contract import box_of, hold

pytestmark = pytest.mark.gpu

APPS = ('cross3d', 'skewcross3d', 'coupled3d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'lds3d_ring_manifest.json')) as _f:
  MANIFEST = json.load(_f)

_CACHE = {}


def name_of(spec):
  return '%s_fused_k1r%s' % (spec['app_name'], 'f' if len(spec['outputs']) > 1 else '')


def opened(app):
  """(program from the prebuilt code object generated with lds_ring=True, oracle)"""
  if app not in _CACHE:
    spec = gpu_util.load_spec(app)
    path = os.path.join(gpu_util.BLOBS, app + '.ldsr.hsaco')
    assert os.path.exists(path), '%s missing: run __graft_entry__.build()' % path
    prog = host.open_program(blob=path, spec=spec)
    _CACHE[app] = (prog, gpu_util.make_oracle(spec))
  return _CACHE[app]


def entry_of(prog):
  (k,) = [k for k in prog.kernels if k['kind'] == 'fused']
  assert k['name'] == name_of(prog.spec) and k['depth'] == 1
  assert len(k['lds_ring']) == k['lds_planes'] and all(k['period'] % s == 0
                                                       for s in k['lds_ring'])
  assert k.get('fields') == (len(prog.spec['outputs']) if len(prog.spec['outputs']) > 1
                             else None)
  return k


def margins(spec, iterate):
  """Cells the intersection of the outputs' boxes after `iterate` iterations is shorter than
  the array: the hull's lo + hi margin, (x, y, z)."""
  lo, hi = specmod.iteration_margins(spec, iterate)[-1]
  return [a + b for a, b in zip(lo, hi)]


def shapes_of(prog, iterate):
  """(z, y, x) from the entry's own constants: an intersection box of one cell each way; one
  tile plus one column and one row with fewer planes than fill_rows + 1; two of the shortest
  chunks less one plane, a few cells wide, so the ring restarts at a chunk seam; a ragged
  grid of 2 x 3 tiles plus odd remainders, 29 planes: clamped loads on all six sides."""
  k = entry_of(prog)
  mx, my, mz = margins(prog.spec, iterate)
  tx, ty = k['tile'][:2]
  assert k['fill_rows'] >= 2
  return [(mz + 1, my + 1, mx + 1),
          (mz + k['fill_rows'] - 1, ty + 1 + my, tx + 1 + mx),
          (mz + 2 * SHORTEST_CHUNK - 1, my + 3, mx + 5),
          (mz + 29, 3 * ty + 5 + my, 2 * tx + 37 + mx)]


def fused_and_staged(prog, inputs, iterate):
  """The arrays of the schedule under depth limit 1 (every launch the plane-ring kernel) and
  the per-stage run's."""
  dims = tuple(reversed(inputs[0].shape))
  stages = [k['name'] for k in prog.kernels if k['kind'] == 'stage']
  try:
    prog.set_max_depth(1)
    assert [k['name'] for k, _ in prog.schedule(dims, iterate)] == [name_of(prog.spec)] * iterate
    got = prog.run_numpy(inputs, iterate=iterate)
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
  n = 0
  for fx, meta in sorted(MANIFEST.items()):
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'lds3d_ring', fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    got, staged = fused_and_staged(prog, inputs, meta['iterate'])
    for name, g, s in zip(spec['outputs'], got, staged):
      want = data['out_' + name]
      assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (fx, name)
      assert np.array_equal(s.view(np.uint8), want.view(np.uint8)), (fx, name, 'per stage')
    n += 1
  assert n == 8


def check_shape(prog, orc, shape, iterate):
  spec = prog.spec
  dims = tuple(reversed(shape))
  inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
  want = orc.run(inputs, iterate=iterate)
  got, staged = fused_and_staged(prog, inputs, iterate)
  for name, g, s in zip(spec['outputs'], got, staged):
    lo, hi = box_of(spec, name, dims, iterate)
    if name == 'velc':      # handed on: its box never shrinks, the whole array is compared
      assert lo == [0, 0, 0] and hi == list(dims)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert g[sl].size > 0, (name, shape, iterate)
    assert np.array_equal(np.ascontiguousarray(g[sl]).view(np.uint8),
                          np.ascontiguousarray(want[name][sl]).view(np.uint8)), \
        (name, shape, iterate)
    assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (name, shape, iterate)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every shape of shapes_of at one iteration."""
  prog, orc = opened(app)
  for shape in shapes_of(prog, 1):
    check_shape(prog, orc, shape, 1)


@pytest.mark.parametrize('app', APPS)
def test_the_plane_loop_leaves_at_every_unrolled_step(app):
  """What the ring adds: one tile, box depths of 1 to `period` planes.  A chunk of `depth`
  planes walks fill_rows + depth steps (the shortest chunk is 8 planes: the deepest boxes
  may be cut in two, which leave at other steps still), so the plane loop leaves at every
  unrolled step and every LDS slot is the last one filled."""
  prog, orc = opened(app)
  k = entry_of(prog)
  mx, my, mz = margins(prog.spec, 1)
  left_at = set()
  for depth in range(1, k['period'] + 1):
    left_at.add((k['fill_rows'] + depth) % k['period'])
    check_shape(prog, orc, (mz + depth, my + 3, mx + 5), 1)
  assert left_at == set(range(k['period']))


@pytest.mark.parametrize('app', APPS)
def test_iterated(app):
  """Two iterations: the ping-pong of every field, extras that grow and boxes that shrink,
  on the smallest and on the ragged shape.  coupled3d's velc is compared on the whole array
  (check_shape)."""
  prog, orc = opened(app)
  shapes = shapes_of(prog, 2)
  for shape in (shapes[0], shapes[-1]):
    check_shape(prog, orc, shape, 2)


@pytest.mark.parametrize('app', APPS)
def test_memory_contract(app):
  """gpu_util.run_guarded on the ragged shape, from the pool allocator's placement and from
  multiples of 16 bytes: every output's box equals the oracle, guards intact, inputs
  unchanged."""
  prog, orc = opened(app)
  shape = shapes_of(prog, 2)[-1]
  prog.set_max_depth(1)
  try:
    for mode in ('pool', 'sixteen'):
      launched = hold(prog, orc, shape, 2, mode, 'stream', 1)
      assert [k['name'] for k in launched] == [name_of(prog.spec)] * 2
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """Mixed signs and exponents over the element's whole mantissa (gpu_util.wide_inputs at
  the default span), in float (cross3d, coupled3d) and in double (skewcross3d).  The
  oracle's values on every output's box are finite: no NaN payload enters the byte
  comparison."""
  prog, orc = opened(app)
  spec = prog.spec
  assert spec['inputs'][0]['c_type'] == ('double' if app == 'skewcross3d' else 'float')
  k = entry_of(prog)
  mx, my, mz = margins(spec, 2)
  shape = (mz + 11, k['tile'][1] + 9 + my, k['tile'][0] + 35 + mx)
  inputs = gpu_util.wide_inputs(spec, shape)
  want = orc.run(inputs, iterate=2)
  for name in spec['outputs']:
    lo, hi = box_of(spec, name, tuple(reversed(shape)), 2)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert want[name][sl].size > 0 and np.isfinite(want[name][sl]).all(), name
  prog.set_max_depth(1)
  try:
    launched = hold(prog, orc, shape, 2, 'pool', 'stream', 1, inputs=inputs)
    assert [k['name'] for k in launched] == [name_of(spec)] * 2
  finally:
    prog.set_max_depth(0)


def test_run_time_compile_with_the_switch():
  """host.open_program(spec=..., lds_ring=True): the offline build's table, the blob's bytes
  on the ragged shape; without the switch the per-stage kernel only."""
  spec = gpu_util.load_spec('cross3d')
  blob_prog, orc = opened('cross3d')
  prog = host.open_program(spec=spec, lds_ring=True)
  try:
    assert prog.kernels == kernel.generate(spec, lds_ring=True)[1]
    assert prog.kernels == blob_prog.kernels
    shape = shapes_of(prog, 2)[-1]
    check_shape(prog, orc, shape, 2)
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
    assert [k['kind'] for k in plain.kernels] == ['stage']
  finally:
    plain.close()
    plain.blob.unload()
