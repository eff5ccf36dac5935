"""Fused kernels of iterated 1-D programs over several fields (soda_hip/codegen/
kernel_fields1d.py) on a real MI355X, all through the C ABI: the reference's fixtures array
for array, every schedule the depth limits and explicit splits give against the oracle and
against the per-stage run, the sweep's memory contract in guarded arenas (with the boxes on
the array's first and last element), other element types on full-width operands, sweeps
resumed from per-field valid regions, that a run without a limit still goes per stage, and
the generated entry point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
import test_gpu_memory_contract as contract
from test_gpu_memory_contract import box_of, hold

pytestmark = pytest.mark.gpu

APPS = ('wave1d', 'skewpair1d', 'fdtd1d', 'mixpair1d')
ITERATES = (1, 2, 3, 5, 8, 13)
LIMITS = (1, 2, 4, 8)
CAP = 13          # `iterate` the programs are generated with: admits every depth
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'fields1d_manifest.json')) as _f:
  MANIFEST = json.load(_f)

_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: %d\n'
TEXT = {
    # reads at offsets >= 0 only: cell 0 of both arrays is a valid cell
    'headpair1d': _HEAD + 'input float: f\ninput float: g(*)\n'
                  'output float: fn(0) = (f(0) + g(1)) * 0.5f\n'
                  'output float: gn(0) = (g(0) + f(2)) * 0.5f\n',
    # reads at offsets <= 0 only: the LAST element of both arrays is a valid cell
    'tailpair1d': _HEAD + 'input float: f\ninput float: g(*)\n'
                  'output float: fn(0) = (f(0) + g(-1)) * 0.5f\n'
                  'output float: gn(0) = (g(0) + f(-2)) * 0.5f\n'}


def text_of(app):
  if app in TEXT:
    return TEXT[app] % (app, CAP)
  with open(os.path.join(ROOT, 'tests', 'samples', 'extra', app + '.soda')) as f:
    return f.read()


# Checked on the CPU, at import: the boxes of headpair1d start on element 0 whatever the
# iteration count, those of tailpair1d end on the last element.
for _app in TEXT:
  _spec = specmod.spec_from_stencil(frontend.loads(text_of(_app)))
  for _it in (1, 3, 13):
    for _name in _spec['outputs']:
      _lo, _hi = box_of(_spec, _name, [1000], _it)
      assert (_lo == [0]) == (_app[:4] == 'head') and (_hi == [1000]) == (_app[:4] == 'tail')
      assert _hi[0] > _lo[0]

_CACHE = {}


def opened(app, dsl_type=None, wrap=False):
  """(program JIT-compiled from freshly generated text, oracle), once per session, generated
  with an iteration count that admits every depth.  `dsl_type` re-types every tensor of a
  float program."""
  key = (app, dsl_type)
  if key not in _CACHE:
    text = text_of(app)
    if dsl_type:
      assert 'float:' in text
      text = text.replace('float:', dsl_type + ':')
      if dsl_type == 'int32':
        # integer coefficients with the integer tensors: a float expression stored to an
        # int32 is undefined in C++ once it leaves the type's range, which full-width
        # operands make it do - the oracle has no answer there, with -fwrapv or without
        assert '2.0f' in text and '0.1f' in text
        text = text.replace('2.0f', '2').replace('0.1f', '3')
        assert '.' not in text.split('output', 1)[1].replace('(*)', '')
    spec = specmod.spec_from_stencil(frontend.loads(text, iterate=CAP))
    source, _ = kernel.generate(spec)
    prog = host.open_program(source=source, spec=spec)
    if dsl_type:
      want = np.dtype(specmod.NUMPY_NAME[specmod.native_type(dsl_type)])
      assert all(dt == want for dt in prog.in_dtypes + prog.out_dtypes), prog.in_dtypes
    make = gpu_util.make_wrap_oracle if wrap else gpu_util.make_oracle
    _CACHE[key] = (prog, make(spec))
  return _CACHE[key]


def fields1d(k):
  return contract.FAMILY['stream'](k) and k.get('fields', 0) >= 2 and k['fill_rows'] == 0


def depths_of(prog):
  return sorted((k['depth'] for k in prog.kernels if k['kind'] == 'fused'), reverse=True)


def split_of(prog, iterate, limit):
  """`iterate` as the table's fused depths <= limit, deepest first."""
  out = []
  for d in depths_of(prog):
    while d <= limit and sum(out) + d <= iterate:
      out.append(d)
  return out


def hull_margin(spec, iterate):
  """Cells the intersection of the outputs' boxes is shorter than the array."""
  lo, hi = specmod.iteration_margins(spec, iterate)[-1]
  return lo[0] + hi[0]


def lengths(prog, iterate, depth):
  """Array lengths from the entry's own constants, m = the hull margin of `iterate`
  iterations: a box of one cell, half a segment, one segment and one cell more, one
  workgroup less and more than a cell, three workgroups and an odd rest, and 100003."""
  k = contract.entry(prog, 'stream', depth)
  m = hull_margin(prog.spec, iterate)
  w_out, tile = k['w_out'], k['tile'][0]
  ns = [m + 1, w_out // 2, w_out + m, w_out + m + 1, tile - 1 + m, tile + 1 + m,
        3 * tile + 17, 100003]
  return [n for n in ns if n > m]


def test_tables_are_the_fused_fields1d_family():
  for app in APPS + tuple(TEXT):
    prog, _ = opened(app)
    assert depths_of(prog) == [12, 8, 4, 2, 1]
    for k in prog.kernels:
      assert k['kind'] != 'fused' or (fields1d(k) and k['fields'] == 2)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  """The whole array of every output equals the reference's - the output on its own box,
  zero outside - per stage, under a depth limit and, where the table has the depth, as ONE
  fused launch."""
  prog, _ = opened(app)
  spec = prog.spec
  n = 0
  try:
    for fx, meta in sorted(MANIFEST.items()):
      if not fx.endswith('.npz') or not meta['key'].startswith(app + '.'):
        continue
      data = np.load(os.path.join(GOLDEN, 'fields1d', fx))
      inputs = [data['in_' + t['name']] for t in spec['inputs']]
      want = [data['out_' + name] for name in spec['outputs']]
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
          got = prog.run_numpy(inputs, iterate=iterate)
        finally:
          if split:
            prog.set_split(dims, iterate, [])
        assert launched and all(fields1d(k) for k in launched), (fx, split)
        assert split is None or [k['depth'] for k in launched] == split, (fx, split)
        for name, g, w in zip(spec['outputs'], got, want):
          assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (fx, split, name)
      prog.set_max_depth(-1)
      got = prog.run_numpy(inputs, iterate=iterate)
      for name, g, w in zip(spec['outputs'], got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (fx, 'per stage', name)
      n += 1
  finally:
    prog.set_max_depth(0)
  assert n == 16


@pytest.mark.parametrize('iterate', ITERATES)
@pytest.mark.parametrize('app', APPS)
def test_schedules(app, iterate):
  """Depth limits and explicit splits on lengths around the kernels' constants: every
  output's box bit-exact with the oracle, the whole arrays identical to the per-stage run,
  the launches the depths asked for."""
  prog, orc = opened(app, wrap=(app == 'mixpair1d'))
  spec = prog.spec
  splits = []
  for limit in LIMITS:
    s = split_of(prog, iterate, limit)
    for split in (s, s[::-1]):        # deepest first and shallowest first
      if split not in splits:
        splits.append(split)
  ns = sorted({n for split in splits for n in lengths(prog, iterate, max(split))})
  try:
    for n in ns:
      dims = (n,)
      inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
      want = orc.run(inputs, iterate=iterate)
      boxes = []
      for name in spec['outputs']:
        lo, hi = box_of(spec, name, dims, iterate)
        boxes.append(slice(lo[0], hi[0]))
        assert want[name][boxes[-1]].size > 0
      prog.set_max_depth(-1)
      staged_launches = [k for k, _ in prog.schedule(dims, iterate)]
      assert all(k['kind'] == 'stage' for k in staged_launches)
      assert len(staged_launches) == iterate * len(spec['stages'])
      staged = prog.run_numpy(inputs, iterate=iterate)
      for name, sl, s in zip(spec['outputs'], boxes, staged):
        assert np.array_equal(s[sl].view(np.uint8), want[name][sl].view(np.uint8)), (app, n, name)

      def check(got, timing, launched, asked):
        what = (app, n, iterate, asked, [k['name'] for k in launched])
        assert all(fields1d(k) for k in launched), what
        assert sum(k['depth'] for k in launched) == iterate, what
        assert timing['max_depth'] == max(k['depth'] for k in launched), (timing, what)
        for name, sl, g, s in zip(spec['outputs'], boxes, got, staged):
          assert np.array_equal(g[sl].view(np.uint8), want[name][sl].view(np.uint8)), (name, what)
          assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (name, what)

      for limit in LIMITS:
        prog.set_max_depth(limit)
        launched = [k for k, _ in prog.schedule(dims, iterate)]
        got, timing = prog.run_numpy(inputs, iterate=iterate, timed=True)
        assert max(k['depth'] for k in launched) <= limit, (app, n, iterate, limit)
        check(got, timing, launched, limit)
      prog.set_max_depth(0)
      for split in splits:
        prog.set_split(dims, iterate, split)
        try:
          launched = [k for k, _ in prog.schedule(dims, iterate)]
          got, timing = prog.run_numpy(inputs, iterate=iterate, timed=True)
        finally:
          prog.set_split(dims, iterate, [])
        assert [k['depth'] for k in launched] == split, (app, n, iterate, split)
        check(got, timing, launched, split)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('depth', [1, 4, 8])
@pytest.mark.parametrize('app', ['wave1d', 'skewpair1d', 'fdtd1d', 'headpair1d', 'tailpair1d'])
def test_memory_contract(app, depth):
  """gpu_util.run_guarded from the pool allocator's placement, multiples of 64 and of 16
  bytes: every output's box equals the oracle (for headpair1d / tailpair1d it starts on the
  array's first / ends on its last element), guards intact, the inputs unchanged."""
  prog, orc = opened(app)
  iterate = depth + 1
  for n in lengths(prog, iterate, depth):
    for mode in contract.SKEWS:
      hold(prog, orc, (n,), iterate, mode, 'stream', depth, split=[depth, 1],
           edge=contract.edge_of(app))


@pytest.mark.parametrize('app,dsl_type', [('wave1d', 'double'), ('wave1d', 'int32'),
                                          ('mixpair1d', None)])
def test_types_and_full_width_operands(app, dsl_type):
  """8-, 4- and 2-byte elements (2, 4 and 8 cells per lane), every bit of the element in use
  (gpu_util.wide_inputs); the integers against the -fwrapv oracle."""
  prog, orc = opened(app, dsl_type, wrap=dsl_type != 'double')
  elem = prog.in_dtypes[0].itemsize
  assert elem == {'double': 8, 'int32': 4, None: 2}[dsl_type]
  assert all(k['cols'] == 16 // elem for k in prog.kernels if k['kind'] == 'fused')
  for depth in (1, 4, 8):
    iterate = depth + 1
    k = contract.entry(prog, 'stream', depth)
    m = hull_margin(prog.spec, iterate)
    for i, n in enumerate((k['w_out'] + m + 1, 3 * k['tile'][0] + 17)):
      inputs = gpu_util.wide_inputs(prog.spec, (n,), seed=gpu_util.SEED + n)
      hold(prog, orc, (n,), iterate, contract.SKEWS[(i + depth) % 3], 'stream', depth,
           split=[depth, 1], inputs=inputs)


@pytest.mark.parametrize('app', ['wave1d', 'skewpair1d', 'fdtd1d'])
def test_resumed_sweeps(app):
  """t1 iterations, then t2 more from the raw result - unspecified cells and all - with the
  per-field margins the first run returned: the same bits as t1 + t2 in one call on every
  output's box, under a depth limit of 4, in guarded arenas."""
  prog, _ = opened(app)
  spec = prog.spec
  k = contract.entry(prog, 'stream', 4)
  prog.set_max_depth(4)
  try:
    for n in (k['tile'][0] + 37, 100003):
      dims = (n,)
      inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
      for t1, t2 in ((1, 1), (1, 4), (2, 3), (3, 5), (4, 2), (5, 8)):
        whole = prog.run_numpy(inputs, iterate=t1 + t2)
        level, bad, _ = gpu_util.run_guarded(prog, inputs, t1)
        assert bad == [], bad
        margins = prog.field_margins(t1)
        assert margins == specmod.iteration_field_margins(spec, t1)[-1]
        valid = dict(valid_lo=[lo for lo, _ in margins], valid_hi=[hi for _, hi in margins])
        launched = [e['kernel'] for e in prog.schedule_fields(dims, t2, **valid)]
        assert all(fields1d(e) for e in launched), (app, n, t1, t2)
        assert sum(e['depth'] for e in launched) == t2
        outs, bad, _ = gpu_util.run_guarded(prog, level, t2, seed=gpu_util.SEED + 1,
                                            skews=gpu_util.pool_skews(4, 4), **valid)
        assert bad == [], (bad, app, n, t1, t2)
        for name, g, w in zip(spec['outputs'], outs, whole):
          lo, hi = box_of(spec, name, dims, t1 + t2)
          sl = slice(lo[0], hi[0])
          assert w[sl].size > 0 and w[sl].std() > 0
          assert np.array_equal(g[sl].view(np.uint8), w[sl].view(np.uint8)), (app, n, t1, t2, name)
  finally:
    prog.set_max_depth(0)


def test_the_default_schedule_stays_per_stage():
  for app in ('wave1d', 'fdtd1d'):
    prog, _ = opened(app)
    prog.set_max_depth(0)
    for n, iterate in ((100003, 12), (1 << 24, 100), (300, 3)):
      launched = [k for k, _ in prog.schedule((n,), iterate)]
      assert len(launched) == iterate * len(prog.spec['stages']), (app, n, iterate)
      assert all(k['kind'] == 'stage' for k in launched), (app, n, iterate)


def test_generated_entry_point(tmp_path):
  """`sodac --hip` on wave1d: the generated wave1d_test says PASS."""
  pkg = os.path.join(ROOT, 'soda-compiler_amd')
  out = tmp_path / 'out'
  subprocess.check_call([sys.executable, os.path.join(pkg, 'sodac'),
                         gpu_util.sample_path('wave1d'), '--hip', str(out)])
  env = dict(os.environ, PYTHONPATH=os.pathsep.join(
      [pkg] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
  r = subprocess.run([sys.executable, str(out / 'wave1d.py'), str(out / 'wave1d.hsaco'),
                      '100003'], capture_output=True, text=True, env=env, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  assert 'INFO: PASS!' in r.stderr
