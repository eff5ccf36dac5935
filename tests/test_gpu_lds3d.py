"""LDS-plane kernels for high-order 3-D stencils (soda_hip/codegen/kernel_stream3d_lds.py) on
a real MI355X, all through the C ABI from `<app>.lds.hsaco`: the reference's fixtures array
for array, shapes taken from the entry's own constants against the oracle and against the
per-stage run, the sweep's memory contract in guarded arenas, full-width operands, and the
run-time compile with the switch.  Every comparison is of bytes."""
import json
import os

import numpy as np
import pytest

from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
from test_gpu_memory_contract import box_of, hold

pytestmark = pytest.mark.gpu

APPS = ('star3d', 'iso3dfd', 'skewstar3d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'lds3d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
SHORTEST_CHUNK = 8            # csrc/schedule.cpp: chunk_rows_min

_CACHE = {}


def opened(app):
  """(program from the prebuilt code object generated with lds_planes=True, oracle)"""
  if app not in _CACHE:
    spec = gpu_util.load_spec(app)
    path = os.path.join(gpu_util.BLOBS, app + '.lds.hsaco')
    assert os.path.exists(path), '%s missing: run __graft_entry__.build()' % path
    prog = host.open_program(blob=path, spec=spec)
    _CACHE[app] = (prog, gpu_util.make_oracle(spec))
  return _CACHE[app]


def entry_of(prog):
  (k,) = [k for k in prog.kernels if k['kind'] == 'fused']
  assert k['name'] == prog.spec['app_name'] + '_fused_k1l' and k['depth'] == 1
  return k


def margins(spec, iterate):
  """Cells the box of `iterate` iterations is shorter than the array, (x, y, z)."""
  lo, hi = specmod.iteration_boxes(spec, iterate)[-1][spec['outputs'][0]]
  return [b - a for a, b in zip(lo, hi)]


def shapes_of(prog, iterate):
  """(z, y, x) from the entry's own constants: a box of one cell each way; one tile plus
  one column and one row with fewer planes than fill_rows + 1; two of the shortest chunks
  less one plane; a ragged grid of several tiles each way."""
  k = entry_of(prog)
  mx, my, mz = margins(prog.spec, iterate)
  tx, ty = k['tile'][:2]
  assert k['fill_rows'] >= 2
  return [(mz + 1, my + 1, mx + 1),
          (mz + k['fill_rows'] - 1, ty + 1 + my, tx + 1 + mx),
          (mz + 2 * SHORTEST_CHUNK - 1, my + 3, mx + 5),
          (mz + 29, 3 * ty + 5 + my, 2 * tx + 37 + mx)]


def fused_and_staged(prog, inputs, iterate):
  """The default schedule's arrays (all launches the LDS-plane kernel) and the per-stage
  run's."""
  dims = tuple(reversed(inputs[0].shape))
  name = prog.spec['app_name'] + '_fused_k1l'
  assert [k['name'] for k, _ in prog.schedule(dims, iterate)] == [name] * iterate
  got = prog.run_numpy(inputs, iterate=iterate)
  prog.set_max_depth(-1)
  try:
    launched = [k for k, _ in prog.schedule(dims, iterate)]
    assert len(launched) == iterate and all(k['kind'] == 'stage' for k in launched)
    staged = prog.run_numpy(inputs, iterate=iterate)
  finally:
    prog.set_max_depth(0)
  return got, staged


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  """The whole array equals the reference's: the output on its box, zero outside; the same
  arrays per stage."""
  prog, _ = opened(app)
  spec = prog.spec
  n = 0
  for fx, meta in sorted(MANIFEST.items()):
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'lds3d', fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    got, staged = fused_and_staged(prog, inputs, meta['iterate'])
    for name, g, s in zip(spec['outputs'], got, staged):
      want = data['out_' + name]
      assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (fx, name)
      assert np.array_equal(s.view(np.uint8), want.view(np.uint8)), (fx, name, 'per stage')
    n += 1
  assert n == (4 if app == 'iso3dfd' else 8)


def check_shape(prog, orc, shape, iterate):
  spec = prog.spec
  dims = tuple(reversed(shape))
  inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
  want = orc.run(inputs, iterate=iterate)
  got, staged = fused_and_staged(prog, inputs, iterate)
  for name, g, s in zip(spec['outputs'], got, staged):
    lo, hi = box_of(spec, name, dims, iterate)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert g[sl].size > 0
    assert np.array_equal(np.ascontiguousarray(g[sl]).view(np.uint8),
                          np.ascontiguousarray(want[name][sl]).view(np.uint8)), (shape, iterate)
    assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (shape, iterate)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every shape of shapes_of at the program's first iteration: the box against the oracle,
  the whole array against the per-stage run."""
  prog, orc = opened(app)
  for shape in shapes_of(prog, 1):
    check_shape(prog, orc, shape, 1)


@pytest.mark.parametrize('iterate', (2, 3, 4))
def test_star3d_iterated(iterate):
  """The shrinking boxes and the ping-pong: the smallest and the ragged shape."""
  prog, orc = opened('star3d')
  shapes = shapes_of(prog, iterate)
  for shape in (shapes[0], shapes[-1]):
    check_shape(prog, orc, shape, iterate)


def test_skewstar3d_iterated():
  prog, orc = opened('skewstar3d')
  check_shape(prog, orc, shapes_of(prog, 3)[-1], 3)


@pytest.mark.parametrize('app,iterate', [('star3d', 1), ('star3d', 3), ('iso3dfd', 1),
                                         ('skewstar3d', 2)])
def test_memory_contract(app, iterate):
  """gpu_util.run_guarded on the smallest and on the ragged shape, from the pool
  allocator's placement and from multiples of 64 and 16 bytes: the box equals the oracle,
  guards intact, inputs unchanged."""
  prog, orc = opened(app)
  shapes = shapes_of(prog, iterate)
  for shape, modes in ((shapes[0], ('pool', 'aligned')), (shapes[-1], ('pool', 'sixteen'))):
    for mode in modes:
      launched = hold(prog, orc, shape, iterate, mode, 'stream', 1)
      assert [k['name'] for k in launched] == [app + '_fused_k1l'] * iterate


@pytest.mark.parametrize('app,iterate', [('star3d', 2), ('iso3dfd', 1), ('skewstar3d', 2)])
def test_full_width_operands(app, iterate):
  """Mixed signs and exponents over the element's whole mantissa (gpu_util.wide_inputs), in
  float and in double."""
  prog, orc = opened(app)
  k = entry_of(prog)
  mx, my, mz = margins(prog.spec, iterate)
  shape = (mz + 11, k['tile'][1] + 9 + my, k['tile'][0] + 35 + mx)
  inputs = gpu_util.wide_inputs_of(app, prog.spec, shape)
  hold(prog, orc, shape, iterate, 'pool', 'stream', 1, inputs=inputs)


def test_run_time_compile_with_the_switch():
  """host.open_program(spec=..., lds_planes=True): the offline build's table, bit-exact on
  a ragged shape; without the switch the per-stage kernels only."""
  spec = gpu_util.load_spec('skewstar3d')
  prog = host.open_program(spec=spec, lds_planes=True)
  try:
    assert prog.kernels == kernel.generate(spec, lds_planes=True)[1]
    assert prog.kernels == opened('skewstar3d')[0].kernels
    check_shape(prog, opened('skewstar3d')[1], shapes_of(prog, 2)[-1], 2)
  finally:
    prog.close()
    prog.blob.unload()
  plain = host.open_program(spec=spec)
  try:
    assert [k['kind'] for k in plain.kernels] == ['stage']
  finally:
    plain.close()
    plain.blob.unload()
