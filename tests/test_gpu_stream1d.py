"""Fused kernels of iterated 1-D programs (soda_hip/codegen/kernel_stream1d.py) on a real
MI355X, all through the C ABI: the reference's fixtures array for array, every schedule
the depth limits and explicit splits give against the oracle and against the per-stage
run, the sweep's memory contract in guarded arenas (with the box on the array's first and
last element), other element types on full-width operands, resumed sweeps, and that a run
without a limit still goes per stage."""
import json
import os

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
import test_gpu_memory_contract as contract
from test_gpu_memory_contract import box_of, hold, margins_of

pytestmark = pytest.mark.gpu

APPS = ('smooth1d', 'fir1d')
ITERATES = (1, 2, 3, 5, 8, 13, 21)
LIMITS = (1, 2, 4, 8, 12)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'stream1d_manifest.json')) as _f:
  MANIFEST = json.load(_f)

_CACHE = {}


def opened(app, dsl_type='float', wrap=False):
  """(program JIT-compiled from freshly generated text, oracle), once per session.
  smooth1d and fir1d are the sample files; head1d / tail1d are the texts of the
  memory-contract tests, generated with an iteration count that admits every depth.
  `dsl_type` re-types every tensor of the program."""
  key = (app, dsl_type)
  if key not in _CACHE:
    if app in APPS:
      with open(os.path.join(ROOT, 'tests', 'samples', 'extra', app + '.soda')) as f:
        text = f.read()
    else:
      text = contract.TEXT[app] % (app, 13)
    assert 'float:' in text
    spec = specmod.spec_from_stencil(frontend.loads(text.replace('float:', dsl_type + ':')))
    source, _ = kernel.generate(spec)
    prog = host.open_program(source=source, spec=spec)
    want = np.dtype(specmod.NUMPY_NAME[specmod.native_type(dsl_type)])
    assert prog.in_dtypes[0] == want and prog.out_dtypes[0] == want, (prog.in_dtypes, want)
    make = gpu_util.make_wrap_oracle if wrap else gpu_util.make_oracle
    _CACHE[key] = (prog, make(spec))
  return _CACHE[key]


def depths_of(prog):
  return sorted((k['depth'] for k in prog.kernels if k['kind'] == 'fused'), reverse=True)


def split_of(prog, iterate, limit):
  """`iterate` as the table's fused depths <= limit, deepest first."""
  out = []
  for d in depths_of(prog):
    while d <= limit and sum(out) + d <= iterate:
      out.append(d)
  return out


def lengths(prog, iterate, depth):
  """Array lengths from the entry's own constants, m = cells the box of `iterate`
  iterations is shorter than the array: a box of one cell, half a segment, one segment
  and one cell more, one workgroup less and more than a cell, three workgroups and an odd
  rest, and 100003.  (A length of m or less has no box: nothing runs, nothing to hold.)"""
  k = contract.entry(prog, 'stream', depth)
  m = margins_of(prog.spec, iterate)[0]
  w_out, tile = k['w_out'], k['tile'][0]
  ns = [m + 1, w_out // 2, w_out + m, w_out + m + 1, tile - 1 + m, tile + 1 + m,
        3 * tile + 17, 100003]
  return [n for n in ns if n > m]


def test_tables_are_the_fused_1d_family():
  for app, want in (('smooth1d', [12, 8, 4, 2, 1]), ('fir1d', [8, 4, 2, 1])):
    prog, _ = opened(app)
    assert depths_of(prog) == want
    for k in prog.kernels:
      assert k['kind'] != 'fused' or (contract.FAMILY['stream'](k) and k['fill_rows'] == 0)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  """The whole array equals the reference's - the output on its box, zero outside - per
  stage, under a depth limit and, where the table has the depth, as ONE fused launch."""
  prog, _ = opened(app)
  spec = prog.spec
  name = spec['outputs'][0]
  n = 0
  try:
    for fx, meta in sorted(MANIFEST.items()):
      if not fx.endswith('.npz') or not meta['key'].startswith(app + '.'):
        continue
      data = np.load(os.path.join(GOLDEN, 'stream1d', fx))
      inputs = [data['in_' + spec['inputs'][0]['name']]]
      want = data['out_' + name]
      dims, iterate = tuple(meta['dims']), meta['iterate']
      splits = [None, split_of(prog, iterate, 2)]
      if iterate in depths_of(prog):
        splits.append([iterate])
      for split in splits:
        prog.set_max_depth(4 if split is None else 0)
        if split:
          prog.set_split(dims, iterate, split)
        try:
          launched = [k for k, _ in prog.schedule(dims, iterate)]
          got = prog.run_numpy(inputs, iterate=iterate)[0]
        finally:
          if split:
            prog.set_split(dims, iterate, [])
        assert launched and all(k['kind'] == 'fused' for k in launched), (fx, split)
        assert split is None or [k['depth'] for k in launched] == split, (fx, split)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (fx, split)
      prog.set_max_depth(-1)
      got = prog.run_numpy(inputs, iterate=iterate)[0]
      assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (fx, 'per stage')
      n += 1
  finally:
    prog.set_max_depth(0)
  assert n == 16


@pytest.mark.parametrize('iterate', ITERATES)
@pytest.mark.parametrize('app', APPS)
def test_schedules(app, iterate):
  """Depth limits and explicit splits on lengths around the kernels' constants: the box
  bit-exact with the oracle, the whole array identical to the per-stage run, the launches
  the depths asked for."""
  prog, orc = opened(app)
  spec = prog.spec
  name = spec['outputs'][0]
  splits = []
  for limit in LIMITS:
    s = split_of(prog, iterate, limit)
    for split in (s, s[::-1]):        # deepest first and shallowest first
      if split not in splits:
        splits.append(split)
  ns = sorted({n for split in splits for n in lengths(prog, iterate, split[0])})
  try:
    for n in ns:
      dims = (n,)
      inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
      want = orc.run(inputs, iterate=iterate)[name]
      lo, hi = box_of(spec, name, dims, iterate)
      sl = slice(lo[0], hi[0])
      assert want[sl].size > 0
      prog.set_max_depth(-1)
      staged_launches = [k for k, _ in prog.schedule(dims, iterate)]
      assert all(k['kind'] == 'stage' for k in staged_launches)
      assert len(staged_launches) == iterate * len(spec['stages'])
      staged = prog.run_numpy(inputs, iterate=iterate)[0]
      assert np.array_equal(staged[sl].view(np.uint8), want[sl].view(np.uint8)), (app, n)

      def check(got, timing, launched, asked):
        what = (app, n, iterate, asked, [k['name'] for k in launched])
        assert all(contract.FAMILY['stream'](k) for k in launched), what
        assert sum(k['depth'] for k in launched) == iterate, what
        assert timing['max_depth'] == max(k['depth'] for k in launched), (timing, what)
        assert np.array_equal(got[sl].view(np.uint8), want[sl].view(np.uint8)), what
        assert np.array_equal(got.view(np.uint8), staged.view(np.uint8)), what

      for limit in LIMITS:
        prog.set_max_depth(limit)
        launched = [k for k, _ in prog.schedule(dims, iterate)]
        got, timing = prog.run_numpy(inputs, iterate=iterate, timed=True)
        assert max(k['depth'] for k in launched) <= limit, (app, n, iterate, limit)
        check(got[0], timing, launched, limit)
      prog.set_max_depth(0)
      for split in splits:
        prog.set_split(dims, iterate, split)
        try:
          launched = [k for k, _ in prog.schedule(dims, iterate)]
          got, timing = prog.run_numpy(inputs, iterate=iterate, timed=True)
        finally:
          prog.set_split(dims, iterate, [])
        assert [k['depth'] for k in launched] == split, (app, n, iterate, split)
        check(got[0], timing, launched, split)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('depth', [1, 4, 12])
@pytest.mark.parametrize('app', ['smooth1d', 'head1d', 'tail1d'])
def test_memory_contract(app, depth):
  """gpu_util.run_guarded from the pool allocator's placement, multiples of 64 and of 16
  bytes: the box equals the oracle (for head1d / tail1d it starts on the array's first /
  ends on its last element), guards intact, the input unchanged."""
  prog, orc = opened(app)
  iterate = depth + 1
  for n in lengths(prog, iterate, depth):
    for mode in contract.SKEWS:
      hold(prog, orc, (n,), iterate, mode, 'stream', depth, split=[depth, 1],
           edge=contract.edge_of(app))


@pytest.mark.parametrize('dsl_type', ['double', 'int32', 'uint16'])
def test_types_and_full_width_operands(dsl_type):
  """smooth1d on 8-, 4- and 2-byte elements (2, 4 and 8 cells per lane), every bit of the
  element in use (gpu_util.wide_inputs); the integers against the -fwrapv oracle."""
  prog, orc = opened('smooth1d', dsl_type, wrap=dsl_type != 'double')
  elem = {'double': 8, 'int32': 4, 'uint16': 2}[dsl_type]
  assert prog.in_dtypes[0].itemsize == elem
  assert all(k['cols'] == 16 // elem for k in prog.kernels if k['kind'] == 'fused')
  for depth in (1, 4, 12):
    iterate = depth + 1
    k = contract.entry(prog, 'stream', depth)
    m = margins_of(prog.spec, iterate)[0]
    for i, n in enumerate((k['w_out'] + m + 1, 3 * k['tile'][0] + 17)):
      inputs = gpu_util.wide_inputs(prog.spec, (n,), seed=gpu_util.SEED + n)
      hold(prog, orc, (n,), iterate, contract.SKEWS[(i + depth) % 3], 'stream', depth,
           split=[depth, 1], inputs=inputs)


@pytest.mark.parametrize('app', APPS)
def test_resumed_sweeps(app):
  """t1 iterations, then t2 more from the margins the first run returned: the same bits
  as t1 + t2 in one call, under a depth limit of 4."""
  prog, _ = opened(app)
  spec = prog.spec
  name = spec['outputs'][0]
  k = contract.entry(prog, 'stream', 4)
  prog.set_max_depth(4)
  try:
    for n in (k['tile'][0] + 37, 100003):
      dims = (n,)
      (a,) = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
      for t1 in range(1, 5):
        lo, hi = prog.margins(t1)
        level = np.random.default_rng(11).integers(0, 2 ** 32, size=(n,), dtype=np.uint32).view(
            np.float32).copy()
        level[lo[0]:n - hi[0]] = prog.run_numpy([a], iterate=t1)[0][lo[0]:n - hi[0]]
        for t2 in range(1, 6 - t1):
          whole = prog.run_numpy([a], iterate=t1 + t2)[0]
          launched = [e for e, _ in prog.schedule(dims, t2, valid_lo=lo, valid_hi=hi)]
          assert all(contract.FAMILY['stream'](e) for e in launched), (app, n, t1, t2)
          assert sum(e['depth'] for e in launched) == t2
          outs, bad, _ = gpu_util.run_guarded(prog, [level], t2, valid_lo=lo, valid_hi=hi,
                                              skews=gpu_util.pool_skews(2, 4))
          flo, fhi = box_of(spec, name, dims, t1 + t2)
          sl = slice(flo[0], fhi[0])
          assert whole[sl].size > 0 and whole[sl].std() > 0
          assert np.array_equal(outs[0][sl].view(np.uint8), whole[sl].view(np.uint8)), (
              app, n, t1, t2)
          assert bad == [], (bad, app, n, t1, t2)
  finally:
    prog.set_max_depth(0)


def test_the_default_schedule_stays_per_stage():
  prog, _ = opened('smooth1d')
  prog.set_max_depth(0)
  for n, iterate in ((100003, 12), (1 << 24, 100), (300, 3)):
    launched = [k for k, _ in prog.schedule((n,), iterate)]
    assert len(launched) == iterate and all(k['kind'] == 'stage' for k in launched), (n, iterate)
