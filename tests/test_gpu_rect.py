"""Fused one-pass kernels over several outputs (kernel.generate's `fuse_outputs`;
kernel_fields2d / kernel_fields3d at depth 1) on a real MI355X, all through the C ABI and
from the code objects __graft_entry__.build() made with the switch (<app>.fused.hsaco):
the reference's fixtures array for array under fused and under per-stage launches, grids
sized by the kernel's own tile against the oracle on full-width operands in guarded
arenas, the cells outside an output's box, resumed sweeps with a valid region per input,
and outchain, whose first output also feeds the second."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
from test_gpu_memory_contract import box_of, hold, skews_for
from test_rect_codegen import composed

pytestmark = pytest.mark.gpu

APPS = ('grad2d', 'blend2d', 'grad3d', 'mix3d')
ALL = APPS + ('outchain',)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rect')
with open(os.path.join(GOLDEN, 'manifest.json')) as _f:
  MANIFEST = json.load(_f)
CHUNK = 7          # rows (planes) per chunk of the grids below; the kernels' own is 256 (64)

_CACHE = {}
_ORACLES = {}


def fused_blob(app):
  path = os.path.join(gpu_util.BLOBS, app + '.fused.hsaco')
  assert os.path.exists(path), '%s missing: run __graft_entry__.build()' % path
  return path


def oracle_of(app):
  """blend2d's integers are held to the -fwrapv oracle like every integer program on
  full-range operands."""
  if app not in _ORACLES:
    make = gpu_util.make_wrap_oracle if app == 'blend2d' else gpu_util.make_oracle
    _ORACLES[app] = make(gpu_util.load_spec(app))
  return _ORACLES[app]


def opened(app):
  """(program with the fused kernel, oracle), one per module; never called under
  small_chunks, so the cached plan runs the kernel's own chunk length."""
  assert 'SODA_HIP_CHUNK_ROWS' not in os.environ
  if app not in _CACHE:
    _CACHE[app] = host.open_program(blob=fused_blob(app), spec=gpu_util.load_spec(app))
  return _CACHE[app], oracle_of(app)


def fused_entry(prog):
  k = prog.kernels[-1]
  assert (k['kind'], k['depth'], k['fields']) == ('fused', 1, len(prog.spec['outputs']))
  assert all(e['kind'] == 'stage' for e in prog.kernels[:-1])
  return k


def kinds(prog, dims):
  return [k['kind'] for k, _ in prog.schedule(dims, 1)]


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  """The whole array equals the reference's - each output on its own box, zero outside -
  launched fused (depth limit 1) and per stage (no limit, and limit -1)."""
  prog, _ = opened(app)
  spec = prog.spec
  fused_entry(prog)
  n = 0
  try:
    for fx, meta in sorted(MANIFEST.items()):
      if not fx.endswith('.npz') or not meta['key'].startswith(app + '.'):
        continue
      data = np.load(os.path.join(GOLDEN, fx))
      inputs = [data['in_' + t['name']] for t in spec['inputs']]
      for limit, want_kinds in ((1, ['fused']), (0, ['stage'] * len(prog.lowered['stages'])),
                                (-1, ['stage'] * len(prog.lowered['stages']))):
        prog.set_max_depth(limit)
        assert kinds(prog, meta['dims']) == want_kinds, (fx, limit)
        got, timing = prog.run_numpy(inputs, iterate=1, timed=True)
        assert timing['max_depth'] == 1
        for name, g in zip(spec['outputs'], got):
          want = data['out_' + name]
          assert g.dtype == want.dtype
          assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (fx, name, limit)
      n += 1
  finally:
    prog.set_max_depth(0)
  assert n == 4


def reaching_shape(prog, k):
  """A grid the small fixtures cannot reach, from the kernel's own figures: a workgroup's
  four strips (2-D) or tiles (3-D), one more and a ragged one along x, two tiles and a
  ragged one along y (3-D), two chunks of CHUNK and a remainder; the boxes lie one window
  from the array's edge on every side, where loads are clamped."""
  spec = prog.spec
  lo, hi = specmod.iteration_margins(spec, 1)[-1]
  w = k['tile'][0] + k['w_out'] + 37 + lo[0] + hi[0]
  outer = 2 * CHUNK + 3 + lo[-1] + hi[-1]
  if spec['dim'] == 2:
    return (outer, w)
  return (outer, 2 * k['r_out'] + 3 + lo[1] + hi[1], w)


@pytest.fixture
def small_chunks(monkeypatch):
  """Programs opened inside plan with chunks of CHUNK rows (the library reads the two
  variables when a plan is created)."""
  monkeypatch.setenv('SODA_HIP_TUNING', '1')
  monkeypatch.setenv('SODA_HIP_CHUNK_ROWS', str(CHUNK))
  made = []

  def open_(app):
    prog = host.open_program(blob=fused_blob(app), spec=gpu_util.load_spec(app))
    made.append(prog)
    return prog
  yield open_
  for prog in made:
    prog.close()


def arena_before(prog, inputs, skews):
  """The bytes gpu_util.run_guarded uploaded (same layout, same seed): what every output
  cell held before the sweep."""
  spec, shape = prog.spec, inputs[0].shape
  names_in = ['in:' + t['name'] for t in spec['inputs']]
  names_out = ['out:' + o for o in spec['outputs']]
  arena = gpu_util.Arena([(n, 'in', shape, dt) for n, dt in zip(names_in, prog.in_dtypes)] +
                         [(n, 'out', shape, dt) for n, dt in zip(names_out, prog.out_dtypes)],
                         skews=skews)
  img = arena.image(dict(zip(names_in, inputs)))
  return [arena.view(img, n) for n in names_out]


@pytest.mark.parametrize('app', ALL)
def test_grids_the_fixtures_cannot_reach(app, small_chunks):
  """Full-width mixed-sign operands in guarded arenas, pool placement and 64-byte aligned:
  every output bit-exact with the oracle on its box, guards intact, inputs unchanged
  (hold), ONE fused launch - and the cells outside output j's box are left as found."""
  orc = oracle_of(app)
  prog = small_chunks(app)
  spec = prog.spec
  k = fused_entry(prog)
  shape = reaching_shape(prog, k)
  dims = tuple(reversed(shape))
  inputs = gpu_util.wide_inputs_of(app, spec, shape)
  prog.set_max_depth(1)
  plan = prog.schedule_fields(dims, 1)
  assert [l['kernel']['name'] for l in plan] == [k['name']]
  assert plan[0]['param'][0] == CHUNK
  for mode in ('pool', 'aligned'):
    launched = hold(prog, orc, shape, 1, mode, 'stream', 1, inputs=inputs)
    assert [e['name'] for e in launched] == [k['name']]
  # the same run once more, for the raw arrays: outside its box an output is untouched
  n = len(spec['inputs']) + len(spec['outputs'])
  skews = skews_for('pool', n, inputs[0].dtype.itemsize)
  outs, bad, timing = gpu_util.run_guarded(prog, inputs, 1, skews=skews)
  assert bad == [] and timing['max_depth'] == 1
  for name, got, before in zip(spec['outputs'], outs, arena_before(prog, inputs, skews)):
    lo, hi = box_of(spec, name, dims, 1)
    outside = np.ones(shape, bool)
    outside[tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))] = False
    assert outside.any() and not outside.all()
    assert np.array_equal(got[outside].view(np.uint8), before[outside].view(np.uint8)), name
    assert not np.array_equal(got[~outside].view(np.uint8), before[~outside].view(np.uint8))


@pytest.mark.parametrize('app', APPS)
def test_host_buffer_entry_leaves_the_rest_as_found(app):
  """soda_hip_run_buffers on pre-filled outputs, launched fused: each output's own box
  equals the oracle, every other cell keeps what it held."""
  prog, orc = opened(app)
  spec = prog.spec
  shape = (23, 300) if spec['dim'] == 2 else (9, 21, 140)
  dims = tuple(reversed(shape))
  inputs = gpu_util.wide_inputs_of(app, spec, shape)
  want = orc.run(inputs, iterate=1)
  fill = [np.full(shape, 77, dtype=dt) for dt in prog.out_dtypes]
  outs = [f.copy() for f in fill]
  prog.set_max_depth(1)
  try:
    assert kinds(prog, dims) == ['fused']
    prog.run_buffers(inputs, outs, 1)
  finally:
    prog.set_max_depth(0)
  for name, got, f in zip(spec['outputs'], outs, fill):
    lo, hi = box_of(spec, name, dims, 1)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert np.array_equal(np.ascontiguousarray(got[sl]).view(np.uint8),
                          np.ascontiguousarray(want[name][sl]).view(np.uint8)), name
    rest = np.ones(shape, bool)
    rest[sl] = False
    assert np.array_equal(got[rest], f[rest]), name


@pytest.mark.parametrize('app', ALL)
def test_resumed_sweep_with_a_region_per_input(app):
  """Every input valid on a region of its own, the cells outside it poisoned: each
  output, on the box the regions leave it, equals the run on the arrays cropped to the
  region all inputs share (launched fused, in guarded arenas) and the oracle's."""
  prog, orc = opened(app)
  spec = prog.lowered
  dim, n_in = spec['dim'], len(spec['inputs'])
  shape = (41, 290) if dim == 2 else (13, 25, 150)
  dims = tuple(reversed(shape))
  v_lo = [tuple((j + d) % 3 + 1 for d in range(dim)) for j in range(n_in)]
  v_hi = [tuple((2 * j + d) % 4 for d in range(dim)) for j in range(n_in)]
  if n_in == 1:
    v_lo, v_hi = [(2, 1, 3)[:dim]], [(1, 3, 2)[:dim]]
  clean = gpu_util.wide_inputs_of(app, prog.spec, shape)
  rng = np.random.default_rng(9)
  poisoned = []
  for a, lo, hi in zip(clean, v_lo, v_hi):
    p = gpu_util.wide_array(a.dtype, shape, rng)
    if p.dtype.kind == 'f':
      p[...] = np.nan
    sl = tuple(slice(lo[d], dims[d] - hi[d]) for d in reversed(range(dim)))
    p[sl] = a[sl]
    poisoned.append(p)
  c_lo = [min(v[d] for v in v_lo) for d in range(dim)]
  c_hi = [min(v[d] for v in v_hi) for d in range(dim)]
  crop = tuple(slice(c_lo[d], dims[d] - c_hi[d]) for d in reversed(range(dim)))
  cropped = [np.ascontiguousarray(a[crop]) for a in clean]
  start = [([-(v[d] - c_lo[d]) for d in range(dim)], [w[d] - c_hi[d] for d in range(dim)])
           for v, w in zip(v_lo, v_hi)]
  boxes = composed(spec, start)
  prog.set_max_depth(1)
  try:
    plan = prog.schedule_fields(dims, 1, valid_lo=v_lo, valid_hi=v_hi)
    assert [l['kernel']['kind'] for l in plan] == ['fused']
    outs, bad, _ = gpu_util.run_guarded(prog, poisoned, 1, valid_lo=v_lo, valid_hi=v_hi)
    assert kinds(prog, tuple(reversed(cropped[0].shape))) == ['fused']
    fresh = prog.run_numpy(cropped, iterate=1)
  finally:
    prog.set_max_depth(0)
  assert bad == []
  want = orc.run(cropped, iterate=1)
  for name, got, f in zip(spec['outputs'], outs, fresh):
    blo, bhi = boxes[name]
    # the box in the cropped arrays' coordinates, x first
    lo = [-blo[d] for d in range(dim)]
    hi = [dims[d] - c_lo[d] - c_hi[d] - bhi[d] for d in range(dim)]
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    g = np.ascontiguousarray(got[crop][sl])
    assert g.size > 0
    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(want[name][sl]).view(np.uint8)), name
    # a fresh run's box (the cropped arrays are valid everywhere) contains the resumed one
    flo, fhi = box_of(spec, name, tuple(reversed(cropped[0].shape)), 1)
    assert all(a >= b for a, b in zip(lo, flo)) and all(a <= b for a, b in zip(hi, fhi))
    assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(f[sl]).view(np.uint8)), name


def test_outchain_is_fused():
  """`first` is stored from its window and also feeds `second`: both equal numpy and the
  oracle on their boxes (as tests/test_gpu_parity.py holds the per-stage run), in ONE
  launch; the prebuilt default code object still holds per-stage kernels only."""
  prog, orc = opened('outchain')
  fused_entry(prog)
  plain = gpu_util.open_prebuilt('outchain')
  assert all(k['kind'] == 'stage' for k in plain.kernels)
  a = np.random.default_rng(5).random((90, 150), dtype=np.float32)
  f32 = np.float32
  m = (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1]) * f32(0.25)     # rows 0..H-2, cols 0..W-2
  first = m[:, 1:] - m[:, :-1] * f32(0.5)                      # rows 0..H-2, cols 1..W-2
  second = (first[:-2, :-1] + first[2:, 1:]) + a[1:-2, 1:-2] * f32(2.0)
  prog.set_max_depth(1)
  try:
    assert kinds(prog, (150, 90)) == ['fused']
    (got1, got2), timing = prog.run_numpy([a], iterate=1, timed=True)
    o1 = np.full_like(a, -1.0)
    o2 = np.full_like(a, -1.0)
    prog.run_buffers([a], [o1, o2], 1)
  finally:
    prog.set_max_depth(0)
  assert timing['max_depth'] == 1
  want = orc.run([a], iterate=1)
  for got_first, got_second in ((got1, got2), (o1, o2)):
    assert np.array_equal(got_first[:-1, 1:-1], first)
    assert np.array_equal(got_second[1:-2, 1:-2], second)
    assert np.array_equal(got_first[:-1, 1:-1], want['first'][:-1, 1:-1])
    assert np.array_equal(got_second[1:-2, 1:-2], want['second'][1:-2, 1:-2])
  for o, inner in ((o1, (slice(0, -1), slice(1, -1))), (o2, (slice(1, -2), slice(1, -2)))):
    rest = np.ones(a.shape, bool)
    rest[inner] = False
    assert (o[rest] == -1).all()
  p1, p2 = plain.run_numpy([a], iterate=1)
  assert np.array_equal(p1, got1) and np.array_equal(p2, got2)
  plain.close()


@pytest.mark.parametrize('app', ('blend2d', 'mix3d'))
def test_compiled_at_run_time(app):
  """host.open_program(spec=..., fuse_outputs=True): the kernels generated with the switch
  and compiled by hiprtc - the same table as the offline build, ONE fused launch under the
  depth limit, bit-exact with the oracle on every output's box."""
  spec = gpu_util.load_spec(app)
  orc = oracle_of(app)
  prog = host.open_program(spec=spec, fuse_outputs=True)
  try:
    k = fused_entry(prog)
    assert prog.kernels == kernel.generate(spec, fuse_outputs=True)[1]
    shape = (19, 300) if spec['dim'] == 2 else (9, 17, 140)
    dims = tuple(reversed(shape))
    inputs = gpu_util.wide_inputs_of(app, spec, shape)
    assert kinds(prog, dims) == ['stage'] * len(prog.lowered['stages'])
    prog.set_max_depth(1)
    launched = hold(prog, orc, shape, 1, 'pool', 'stream', 1, inputs=inputs)
    assert [e['name'] for e in launched] == [k['name']]
  finally:
    prog.close()
    prog.blob.unload()
  # without the switch the same entry compiles the per-stage kernels only
  plain = host.open_program(spec=spec)
  try:
    assert all(e['kind'] == 'stage' for e in plain.kernels)
  finally:
    plain.close()
    plain.blob.unload()


def test_app_test_compiled_with_the_switch(capfd):
  """host.app_test(fuse_outputs=True) without a blob: run-time compile, the depth limit
  set, the generated self-check's verdict."""
  spec = gpu_util.load_spec('grad3d')
  assert host.app_test(spec, None, [140, 21, 9], fuse_outputs=True) == 0
  assert 'INFO: PASS!' in capfd.readouterr().err


def test_generated_entry_points(tmp_path):
  """`sodac --hip-fuse-outputs --hip` on grad2d: the generated grad2d_test says PASS, and
  the generated `grad2d` entry - which sets the depth limit itself - writes each output's
  box bit-exact with the oracle; its code object launches fused under that limit."""
  pkg = os.path.join(ROOT, 'soda-compiler_amd')
  out = tmp_path / 'out'
  subprocess.check_call([sys.executable, os.path.join(pkg, 'sodac'),
                         gpu_util.sample_path('grad2d'), '--hip-fuse-outputs', '--hip', str(out)])
  env = dict(os.environ, PYTHONPATH=os.pathsep.join(
      [pkg] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
  r = subprocess.run([sys.executable, str(out / 'grad2d.py'), str(out / 'grad2d.hsaco'),
                      '500', '300'], capture_output=True, text=True, env=env, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  assert 'INFO: PASS!' in r.stderr
  spec = gpu_util.load_spec('grad2d')
  prog = host.open_program(blob=str(out / 'grad2d.hsaco'), spec=spec)
  try:
    prog.set_max_depth(1)
    assert kinds(prog, (500, 300)) == ['fused']
  finally:
    prog.close()
    prog.blob.unload()
  shim = {}
  exec(compile((out / 'grad2d.py').read_text(), 'grad2d.py', 'exec'), shim)
  shape = (37, 301)
  img, = gpu_util.wide_inputs_of('grad2d', spec, shape)
  gx, gy = np.full(shape, 5, np.float32), np.full(shape, 5, np.float32)
  assert shim['grad2d'](img, gx, gy, str(out / 'grad2d.hsaco')) == 0
  want = oracle_of('grad2d').run([img], iterate=1)
  for name, got in (('gx', gx), ('gy', gy)):
    lo, hi = box_of(spec, name, tuple(reversed(shape)), 1)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert np.array_equal(np.ascontiguousarray(got[sl]).view(np.uint8),
                          np.ascontiguousarray(want[name][sl]).view(np.uint8)), name
    rest = np.ones(shape, bool)
    rest[sl] = False
    assert (got[rest] == 5).all()
