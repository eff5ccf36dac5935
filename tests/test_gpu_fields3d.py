"""Fused 3-D multi-field kernels (soda_hip/codegen/kernel_fields3d.py) on a real MI355X, all
through the C ABI: the reference's fixtures array for array, every schedule the depth
limit allows against the oracle and against the per-stage run, the sweep's memory
contract in guarded arenas, full-width operands, and the generated entry point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from soda_hip.codegen import spec as specmod

import gpu_util
from conftest import ROOT
from test_gpu_memory_contract import box_of, hold, modes_of

pytestmark = pytest.mark.gpu

APPS = ('wave3d', 'maxwell3d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'fields3d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
FUSED_DEPTHS = (2, 1)             # what the samples' tables hold

_CACHE = {}


def opened(app):
  """(program from the prebuilt code object, oracle)"""
  if app not in _CACHE:
    prog = gpu_util.open_prebuilt(app)
    _CACHE[app] = (prog, gpu_util.make_oracle(prog.spec))
  return _CACHE[app]


def split_of(iterate, limit):
  """`iterate` as fused depths <= limit, deepest first."""
  out = []
  for d in FUSED_DEPTHS:
    while d <= limit and sum(out) + d <= iterate:
      out.append(d)
  return out


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  """The whole array equals the reference's: each output on its own box, zero outside."""
  prog, _ = opened(app)
  spec = prog.spec
  assert {k['depth'] for k in prog.kernels if k['kind'] == 'fused'} == set(FUSED_DEPTHS)
  n = 0
  prog.set_max_depth(2)   # admits the fused kernels: by default these programs run per stage
  try:
    for fx, meta in sorted(MANIFEST.items()):
      if not fx.endswith('.npz') or not meta['key'].startswith(app + '.'):
        continue
      data = np.load(os.path.join(GOLDEN, 'fields3d', fx))
      inputs = [data['in_' + t['name']] for t in spec['inputs']]
      launched = [k for k, _ in prog.schedule(meta['dims'], meta['iterate'])]
      assert launched and all(k['kind'] == 'fused' for k in launched), fx
      assert sum(k['depth'] for k in launched) == meta['iterate'], fx
      got = prog.run_numpy(inputs, iterate=meta['iterate'])
      for name, g in zip(spec['outputs'], got):
        want = data['out_' + name]
        assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (fx, name)
      n += 1
  finally:
    prog.set_max_depth(0)
  assert n == 12


@pytest.mark.parametrize('app', APPS)
def test_schedules(app):
  """iterate x depth limit on a ragged shape: every output bit-exact with the oracle on
  its own box, the whole array identical to the per-stage run, and the launches are the
  fused depths the limit leaves."""
  prog, orc = opened(app)
  spec = prog.spec
  n_stages = len(specmod.inline_pointwise(spec)['stages'])
  shape = (203, 45, 37)
  dims = tuple(reversed(shape))
  inputs = gpu_util.random_inputs(spec, shape)
  try:
    for iterate in (1, 2, 3, 5, 8):
      want = orc.run(inputs, iterate=iterate)
      prog.set_max_depth(-1)
      staged_launches = [k for k, _ in prog.schedule(dims, iterate)]
      assert all(k['kind'] == 'stage' for k in staged_launches)
      assert len(staged_launches) == iterate * n_stages
      staged = prog.run_numpy(inputs, iterate=iterate)
      for limit in (0, 1, 2):
        prog.set_max_depth(limit)
        # the scheduler's own choice.  No limit: per stage, until the fused kernels have
        # been measured (profiles/r07_fields3d.txt).  A limit admits them: fused all the
        # way, no deeper than the limit
        own = [k for k, _ in prog.schedule(dims, iterate)]
        if not limit:
          assert [k['name'] for k in own] == [k['name'] for k in staged_launches], (app, iterate)
        else:
          assert all(k['kind'] == 'fused' for k in own), (app, iterate, limit)
          assert sum(k['depth'] for k in own) == iterate, (app, iterate, limit)
          assert max(k['depth'] for k in own) <= limit, (app, iterate, limit)
        split = split_of(iterate, limit or 2)
        prog.set_split(dims, iterate, split)
        try:
          launched = [k for k, _ in prog.schedule(dims, iterate)]
          got, timing = prog.run_numpy(inputs, iterate=iterate, timed=True)
        finally:
          prog.set_split(dims, iterate, [])
        what = (app, iterate, limit, [k['name'] for k in launched])
        assert all(k['kind'] == 'fused' and k['fields'] == len(spec['outputs'])
                   for k in launched), what
        assert [k['depth'] for k in launched] == split and sum(split) == iterate, what
        assert timing['max_depth'] == max(split), (timing, what)
        for name, g, s in zip(spec['outputs'], got, staged):
          lo, hi = box_of(spec, name, dims, iterate)
          sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
          assert g[sl].size > 0
          assert np.array_equal(np.ascontiguousarray(g[sl]).view(np.uint8),
                                np.ascontiguousarray(want[name][sl]).view(np.uint8)), (name, what)
          assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (name, what)
  finally:
    prog.set_max_depth(0)


def contract_shapes(prog, iterate, depth):
  """(z, y, x) around the kernel's own constants: boxes one cell from empty in each
  dimension and in all, a width below one tile with r_out + margin + 1 rows and fewer
  planes than the pipeline fill, one tile plus one column, two chunks less one plane (of
  the shortest chunk the launcher takes, 8, and of the entry's own), several tiles each
  way."""
  spec = prog.spec
  k = next(k for k in prog.kernels if k['kind'] == 'fused' and k['depth'] == depth)
  boxes = specmod.iteration_boxes(spec, iterate)[-1]
  # cells the SMALLEST box is shorter than the array, per dimension
  mx, my, mz = [max(boxes[o][1][d] - boxes[o][0][d] for o in spec['outputs'])
                for d in (0, 1, 2)]
  w_out, r_out, fill, chunk = k['w_out'], k['r_out'], k['fill_rows'], k['tile'][2]
  assert fill >= 2 and w_out // 2 > mx and chunk == 64
  return [(mz + 1, 30, 70), (20, my + 1, 70), (20, 30, mx + 1), (mz + 2, my + 2, mx + 2),
          (fill - 1 + mz, r_out + my + 1, w_out // 2), (2 * 8 - 1 + mz, my + 3, w_out + mx + 1),
          (2 * chunk - 1 + mz, my + 5, w_out + mx), (mz + 9, 3 * r_out + my + 2, 4 * w_out + 17)]


@pytest.mark.parametrize('app,iterate,split', [
    ('wave3d', 3, [2, 1]), ('wave3d', 2, [1, 1]), ('maxwell3d', 3, [2, 1]),
    ('maxwell3d', 5, [2, 2, 1]), ('maxwell3d', 1, [1])])
def test_memory_contract(app, iterate, split):
  """gpu_util.run_guarded from the pool allocator's placement, multiples of 64 and 16
  bytes: boxes equal the oracle, guards intact, inputs unchanged."""
  prog, orc = opened(app)
  shapes = contract_shapes(prog, iterate, split[0])
  for i, shape in enumerate(shapes):
    for mode in modes_of(i):
      hold(prog, orc, shape, iterate, mode, 'stream', split[0], split=split)


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """Mixed signs and exponents in every field (gpu_util.wide_inputs)."""
  prog, orc = opened(app)
  shape, iterate, split = (41, 37, 131), 3, [2, 1]
  inputs = gpu_util.wide_inputs_of(app, prog.spec, shape)
  hold(prog, orc, shape, iterate, 'pool', 'stream', split[0], split=split, inputs=inputs)


def test_generated_entry_point(tmp_path):
  """`sodac --hip` on wave3d: the generated wave3d_test says PASS."""
  pkg = os.path.join(ROOT, 'soda-compiler_amd')
  out = tmp_path / 'out'
  subprocess.check_call([sys.executable, os.path.join(pkg, 'sodac'),
                         gpu_util.sample_path('wave3d'), '--hip', str(out)])
  env = dict(os.environ, PYTHONPATH=os.pathsep.join(
      [pkg] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
  r = subprocess.run([sys.executable, str(out / 'wave3d.py'), str(out / 'wave3d.hsaco'),
                      '70', '45', '40'], capture_output=True, text=True, env=env, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  assert 'INFO: PASS!' in r.stderr
