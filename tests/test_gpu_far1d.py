"""Far-tap 1-D kernels (kernel_stream1d / kernel_fields1d with `hops`; kernel.generate's
`far_taps`) on a real MI355X, all through the C ABI from `<app>.taps.hsaco`: the reference's
fixtures array for array, lengths taken from each entry's own constants at every depth and
split - every output on its own box against the oracle, the whole arrays against the
per-stage run -, the sweep's memory contract in guarded arenas (with the box on the array's
first and last element), full-width operands, a sweep resumed from per-field valid regions,
and the run-time compile with the switch.  Every comparison is of bytes
(tests/switch_form_gpu.py, what fits a 1-D program; the rest is here).

No fused 1-D kernel is in the default schedule (csrc/schedule.cpp, plans_fused): every entry
point generated with the switch sets the depth limit of the program's deepest kernel
(switches.depth_limit_of), and the fused runs here are those under the same limit, from the
same function."""
import os

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel, switches
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
import switch_form_gpu as harness
import test_gpu_memory_contract as contract
from test_gpu_memory_contract import box_of

pytestmark = pytest.mark.gpu

APPS = ('lowpass1d', 'dfir1d', 'skewfir1d', 'acoustic1d')
DEPTHS = {'lowpass1d': [1, 2, 4], 'dfir1d': [1, 2, 4], 'skewfir1d': [1, 2],
          'acoustic1d': [1, 2, 4]}
ITERATIONS = {'lowpass1d': 4, 'dfir1d': 3, 'skewfir1d': 2, 'acoustic1d': 3}    # fixture sets

_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: 4\ninput float: a(*)\n'
TEXT = {
    # reads at offsets >= 0 only, four lanes above: cell 0 of the array is a valid cell
    'headfar1d': _HEAD + 'output float: b(0) = 0.5f * a(0) + 0.25f * a(6) + 0.125f * a(13)\n',
    # reads at offsets <= 0 only, five lanes below: the LAST element is a valid cell
    'tailfar1d': _HEAD + 'output float: b(0) = 0.5f * a(0) - 0.25f * a(-9) + 0.125f * a(-17)\n'}

# Checked on the CPU, at import: the box of headfar1d starts on element 0 whatever the
# iteration count, that of tailfar1d ends on the last element; both are in the switch's class.
for _app in TEXT:
  _spec = specmod.spec_from_stencil(frontend.loads(TEXT[_app] % _app))
  for _it in (1, 3, 5):
    _lo, _hi = box_of(_spec, 'b', [1000], _it)
    assert (_lo == [0]) == (_app[:4] == 'head') and (_hi == [1000]) == (_app[:4] == 'tail')
    assert _hi[0] > _lo[0]
  assert [k['depth'] for k in kernel.generate(_spec, far_taps=True)[1]
          if k['kind'] == 'fused'] == [1, 2, 4]
  assert all(k['kind'] == 'stage' for k in kernel.generate(_spec)[1])


def _check(fused, spec):
  assert min(k['halo'][0] + k['halo'][1] for k in fused) > 2 * fused[0]['cols']   # > a lane a side
  assert all(k['fill_rows'] == 0 and contract.FAMILY['stream'](k) for k in fused)
  assert all(k.get('fields') == (3 if len(spec['outputs']) == 3 else None) for k in fused)


def _depths(spec):
  return DEPTHS.get(spec['app_name'], [1, 2, 4])


# the depth limit: the deepest kernel's, for programs over one array too.  acoustic1d's velc
# is handed on at every iteration, its uc at the first
FORM = harness.Form(
    keyword='far_taps', family='far1d',
    fixtures=lambda app: 4 * ITERATIONS[app],
    kernels=lambda spec: [('%s_fused_k%d' % (spec['app_name'], d), d) for d in _depths(spec)],
    limit=lambda spec: max(_depths(spec)),
    margins=harness.lowered_hull_margins, check=_check,
    whole=lambda name, iterate: name == 'velc' or (name == 'uc' and iterate == 1))

_JIT = {}


def opened(app):
  """The sample from its prebuilt code object; headfar1d / tailfar1d compiled at run time
  with the switch."""
  if app in APPS:
    return harness.opened(FORM, app)
  if app not in _JIT:
    spec = specmod.spec_from_stencil(frontend.loads(TEXT[app] % app))
    _JIT[app] = (host.open_program(spec=spec, far_taps=True), gpu_util.make_oracle(spec))
  return _JIT[app]


def lengths(k, spec, iterate):
  """harness.line_lengths, m = cells the launch's box of `iterate` iterations is shorter than
  the array."""
  (m,) = FORM.margins(spec, iterate)
  return harness.line_lengths(k, m)


splits_of = harness.splits_of


def check_length(prog, orc, n, iterate, splits):
  """Random inputs of `n` cells: per split, every output's box against the oracle and the
  whole arrays against the per-stage run; every launch a fused kernel of the depth asked."""
  spec = prog.spec
  dims = (n,)
  inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
  want = orc.run(inputs, iterate=iterate)
  boxes = []
  for name in spec['outputs']:
    lo, hi, sl = harness.slices_of(spec, name, (n,), iterate)
    if FORM.whole(name, iterate):
      assert (lo, hi) == ([0], [n])
    assert want[name][sl].size > 0, (name, n, iterate)
    boxes.append(sl)
  try:
    prog.set_max_depth(-1)
    launched = [k for k, _ in prog.schedule(dims, iterate)]
    assert [k['kind'] for k in launched] == ['stage'] * (iterate * len(spec['stages']))
    staged = prog.run_numpy(inputs, iterate=iterate)
    prog.set_max_depth(harness.limit_of(FORM, prog))
    for split in splits:
      what = (spec['app_name'], n, iterate, split)
      prog.set_split(dims, iterate, split)
      try:
        launched = [k for k, _ in prog.schedule(dims, iterate)]
        got = prog.run_numpy(inputs, iterate=iterate)
      finally:
        prog.set_split(dims, iterate, [])
      assert [k['name'] for k in launched] == [
          '%s_fused_k%d' % (spec['app_name'], d) for d in split], what
      for name, sl, g, s in zip(spec['outputs'], boxes, got, staged):
        assert np.array_equal(g[sl].view(np.uint8), want[name][sl].view(np.uint8)), (name, what)
        assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (name, what)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  harness.fixtures(FORM, app)


@pytest.mark.parametrize('app', APPS)
def test_lengths_at_every_depth_and_split(app):
  """Every kernel alone on the lengths of its own constants, as many iterations as it fuses;
  then one iteration more than the deepest fuses, in every split the limits give, on the
  lengths of every kernel in the split."""
  prog, orc = opened(app)
  spec = prog.spec
  fused = harness.fused_of(FORM, prog)
  by_depth = {k['depth']: k for k in fused}
  for k in fused:
    for n in lengths(k, spec, k['depth']):
      assert n <= 3 * 3584 + 17
      check_length(prog, orc, n, k['depth'], [[k['depth']]])
  iterate = max(by_depth) + 1
  splits = splits_of(sorted(by_depth), iterate)
  assert [iterate - 1, 1] in splits and [1] * iterate in splits
  for n in sorted({n for d in by_depth for n in lengths(by_depth[d], spec, iterate)}):
    check_length(prog, orc, n, iterate, [s for s in splits])


@pytest.mark.parametrize('app', APPS + tuple(TEXT))
def test_memory_contract(app):
  """gpu_util.run_guarded from the pool allocator's placement, multiples of 64 and of 16
  bytes, the deepest kernel and one iteration more: every output's box equals the oracle
  (for headfar1d / tailfar1d it starts on the array's first / ends on its last element),
  guards intact, the inputs unchanged."""
  prog, orc = opened(app)
  deep = harness.fused_of(FORM, prog)[-1]
  iterate = deep['depth'] + 1
  prog.set_max_depth(harness.limit_of(FORM, prog))
  try:
    for n in lengths(deep, prog.spec, iterate):
      for mode in contract.SKEWS:
        launched = contract.hold(prog, orc, (n,), iterate, mode, 'stream', deep['depth'],
                                 split=[deep['depth'], 1], edge=contract.edge_of(app))
        assert [k['depth'] for k in launched] == [deep['depth'], 1]
        assert all(k['kind'] == 'fused' for k in launched)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('app,c_type', [('lowpass1d', 'float'), ('dfir1d', 'double'),
                                        ('acoustic1d', 'double')])
def test_full_width_operands(app, c_type):
  """Mixed signs and exponents over the element's whole mantissa (gpu_util.wide_inputs), at
  every depth alone, in guarded arenas.  The oracle's values on every output's box are
  finite: no NaN payload enters the byte comparison."""
  prog, orc = opened(app)
  spec = prog.spec
  assert spec['inputs'][0]['c_type'] == c_type
  for i, k in enumerate(harness.fused_of(FORM, prog)):
    iterate = k['depth']
    (m,) = FORM.margins(spec, iterate)
    for j, n in enumerate((k['w_out'] + m + 1, k['tile'][0] + 35 + m)):
      inputs = gpu_util.wide_inputs(spec, (n,), seed=gpu_util.SEED + n)
      want = orc.run(inputs, iterate=iterate)
      for name in spec['outputs']:
        _, _, sl = harness.slices_of(spec, name, (n,), iterate)
        assert want[name][sl].size > 0 and np.isfinite(want[name][sl]).all(), name
      harness.held(FORM, prog, orc, k, [iterate], (n,), iterate, contract.SKEWS[(i + j) % 3],
                   inputs)


def test_resumed_sweep_with_per_field_valid_regions():
  """acoustic1d: t1 iterations, then t2 more from the raw result - unspecified cells and all -
  with the per-field margins the first run returned (velc's stay 0): the same bits as
  t1 + t2 in one call on every output's box, under the product's limit, in guarded arenas."""
  prog, _ = opened('acoustic1d')
  spec = prog.spec
  deep = harness.fused_of(FORM, prog)[-1]
  prog.set_max_depth(harness.limit_of(FORM, prog))
  try:
    n = deep['tile'][0] + 37 + FORM.margins(spec, 7)[0]
    dims = (n,)
    inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
    for t1, t2 in ((1, 1), (1, 4), (2, 3), (3, 4)):
      whole = prog.run_numpy(inputs, iterate=t1 + t2)
      level, bad, _ = gpu_util.run_guarded(prog, inputs, t1)
      assert bad == [], bad
      margins = prog.field_margins(t1)
      assert margins == specmod.iteration_field_margins(spec, t1)[-1]
      assert [list(v) for v in margins[2]] == [[0], [0]]
      assert [list(v) for v in margins[0]] == [[8 * t1], [8 * t1]]
      valid = dict(valid_lo=[lo for lo, _ in margins], valid_hi=[hi for _, hi in margins])
      launched = [e['kernel'] for e in prog.schedule_fields(dims, t2, **valid)]
      assert all(e['kind'] == 'fused' and e['fields'] == 3 for e in launched), (t1, t2)
      assert sum(e['depth'] for e in launched) == t2
      outs, bad, _ = gpu_util.run_guarded(prog, level, t2, seed=gpu_util.SEED + 1,
                                          skews=gpu_util.pool_skews(6, 8), **valid)
      assert bad == [], (bad, t1, t2)
      for name, g, w in zip(spec['outputs'], outs, whole):
        lo, hi = box_of(spec, name, dims, t1 + t2)
        sl = slice(lo[0], hi[0])
        assert w[sl].size > 0 and w[sl].std() > 0
        assert np.array_equal(g[sl].view(np.uint8), w[sl].view(np.uint8)), (t1, t2, name)
  finally:
    prog.set_max_depth(0)


def test_the_products_limit_admits_the_fused_kernels():
  """What a `--hip-far-taps` product runs: under the limit its entry points set every launch
  is one of the far-tap kernels - without it the launcher keeps a 1-D program per stage -,
  and the generated `<app>_test` passes with the switch."""
  for app, want in (('skewfir1d', [2, 1]), ('acoustic1d', [2, 1]), ('lowpass1d', [4, 1])):
    prog, _ = opened(app)
    spec = prog.spec
    limit, flags = switches.depth_limit_of(spec, dict(far_taps=True))
    assert (limit, flags) == (max(DEPTHS[app]), ['--hip-far-taps'])
    iterate = sum(want)
    try:
      prog.set_max_depth(min(limit, want[0]))
      launched = [k for k, _ in prog.schedule((3001,), iterate)]
      assert all(k['name'] == '%s_fused_k%d' % (app, k['depth']) for k in launched), app
      assert sum(k['depth'] for k in launched) == iterate
      assert max(k['depth'] for k in launched) <= want[0]
      prog.set_max_depth(0)
      assert all(k['kind'] == 'stage' for k, _ in prog.schedule((3001,), iterate))
    finally:
      prog.set_max_depth(0)
  for app in ('skewfir1d', 'acoustic1d'):
    blob = os.path.join(gpu_util.BLOBS, app + '.taps.hsaco')
    assert host.app_test(gpu_util.load_spec(app), blob, [3001, 0, 0, 0], iterate=3,
                         far_taps=True) == 0


def test_run_time_compile_with_the_switch():
  """host.open_program(spec=..., far_taps=True): the offline build's table, bit-exact on the
  ragged length and the blob's bytes there; without the switch the per-stage kernels only."""
  spec = gpu_util.load_spec('skewfir1d')
  blob_prog, orc = opened('skewfir1d')
  prog = host.open_program(spec=spec, far_taps=True)
  try:
    assert prog.kernels == kernel.generate(spec, far_taps=True)[1]
    assert prog.kernels == blob_prog.kernels
    deep = harness.fused_of(FORM, prog)[-1]
    n = lengths(deep, spec, 2)[-1]
    check_length(prog, orc, n, 2, [[2], [1, 1]])
    inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
    got, _ = harness.fused_and_staged(FORM, prog, inputs, 2)
    same, _ = harness.fused_and_staged(FORM, blob_prog, inputs, 2)
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
