"""Fused kernels for iterated 1-D programs (soda_hip/codegen/kernel_stream1d.py), without a
GPU: what the kernel tables hold, what the generator refuses and why, that every kernel
compiles for gfx950 within 128 VGPRs and without scratch, that the launcher's grid and the
kernel's segment origins store every cell of a box exactly once, how the planner schedules
and prices these kernels, that the checker agrees with the reference's fixtures, and that
the tables of 2-D and 3-D programs are what they were without this family."""
import hashlib
import json
import os
import shutil

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel, kernel_stream1d
from soda_hip.codegen import spec as specmod

from codegen_util import HIPCC, READELF, resource_figures, spec_of, spec_of_text
from conftest import ROOT, SAMPLES
import test_schedule as ts
from test_schedule import probe      # noqa: F401 - the planner probe, built once per module

APPS = ('smooth1d', 'fir1d')
DEPTHS = {'smooth1d': {1, 2, 4, 8, 12}, 'fir1d': {1, 2, 4, 8}}
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'stream1d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
LANES = 64


def sample_text(app):
  with open(os.path.join(SAMPLES, 'extra', app + '.soda')) as f:
    return f.read()


def retyped(app, dsl_type):
  """The sample with every tensor of another type (float literals stay: C++ promotes)."""
  return spec_of_text(sample_text(app).replace('float:', dsl_type + ':'))


def fused_of(table):
  return {k['depth']: k for k in table if k['kind'] == 'fused'}


# ---- tables -------------------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_tables_hold_the_fused_depths(app):
  spec = spec_of(app)
  assert spec['dim'] == 1
  text, table = kernel.generate(spec)
  fused = fused_of(table)
  # (a depth that profiles/r10_stream1d.txt shows not to ship leaves STREAM1D_DEPTHS)
  assert set(fused) == {d for d in DEPTHS[app] if d in kernel.STREAM1D_DEPTHS}
  assert set(fused) == DEPTHS[app]
  for depth, k in fused.items():
    assert depth <= spec['iterate']
    assert k['fill_rows'] == 0 and k['step_bytes'] > 0 and k['step_valu'] > 0
    assert k['stage'] == -1 and k['block'] == [256, 1, 1]
    assert k['tile'] == [4 * k['segs'] * k['w_out'], 1, 1, 1]
    assert k['cols'] == 4 and k['segs'] == kernel_stream1d.DEFAULT_SEGS
    assert k['origin_align'] == k['cols']
    assert k['w_out'] + sum(k['halo']) == LANES * k['cols']
    assert 'groups' not in k and 'stack' not in k
    # the halo is the composed window, padded to whole vectors
    lo, hi = specmod.iteration_margins(spec, depth)[-1]
    assert [-(-lo[0] // 4) * 4, -(-hi[0] // 4) * 4] == k['halo']
  # the per-stage kernels stay: the default schedule and max_depth < 0 use them
  assert sum(k['kind'] == 'stage' for k in table) == len(spec['stages'])
  assert 'not fused' not in text


def test_iterate_caps_the_depths_and_segs_is_an_option():
  _, table = kernel.generate(spec_of('smooth1d', iterate=5))
  assert set(fused_of(table)) == {1, 2, 4}
  _, table = kernel.generate(spec_of('smooth1d'), segs=2)
  for k in fused_of(table).values():
    assert k['segs'] == 2 and k['tile'][0] == 8 * k['w_out']
  # 8-byte lanes: two cells of a float per lane
  _, table = kernel.generate(spec_of('smooth1d'), cols=2)
  assert all(k['cols'] == 2 and k['w_out'] + sum(k['halo']) == 128
             for k in fused_of(table).values())


# ---- refusals -----------------------------------------------------------------------------

_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: 4\n'
FAR = _HEAD % 'far' + 'input float: a(*)\noutput float: b(0) = a(5) + a(0)\n'
TWO_IN = _HEAD.replace('iterate: 4', 'iterate: 1') % 'two_in' + \
    'input float: f\ninput float: u(*)\noutput float: o(0) = u(0) + u(1) * f(-1)\n'
WIDEN = _HEAD.replace('iterate: 4', 'iterate: 1') % 'widen' + \
    'input float: a(*)\noutput double: b(0) = a(-1) + a(1)\n'


@pytest.mark.parametrize('text,reason', [
    (FAR, 'x offset 5 exceeds the 4 columns a lane holds'),
    (TWO_IN, 'one input feeding one output (2 input(s), 1 output(s))'),
    (WIDEN, "the output (double) is not of the input's type (float)")])
def test_refused_programs_keep_a_stage_only_table_and_say_why(text, reason):
  spec = spec_of_text(text)
  assert spec['dim'] == 1
  source, table = kernel.generate(spec)
  assert table and all(k['kind'] == 'stage' for k in table)
  assert '// depth 1 not fused: ' in source and reason in source
  with pytest.raises(kernel_stream1d.NotFusable):
    kernel_stream1d.emit(specmod.inline_pointwise(spec), 1)


def test_the_far_read_fits_a_wider_lane():
  """The same program as uint16 holds 8 cells per lane: offset 5 is a neighbour's cell."""
  _, table = kernel.generate(spec_of_text(FAR.replace('float:', 'uint16:')))
  assert set(fused_of(table)) == {1, 2, 4} and fused_of(table)[1]['cols'] == 8


# ---- compile ------------------------------------------------------------------------------

PROGRAMS = {
    'smooth1d': lambda: spec_of('smooth1d'), 'fir1d': lambda: spec_of('fir1d'),
    'smooth1d_double': lambda: retyped('smooth1d', 'double'),
    'smooth1d_uint16': lambda: retyped('smooth1d', 'uint16')}


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('which', sorted(PROGRAMS))
def test_kernels_compile_for_gfx950_within_128_registers(which, tmp_path):
  """Every fused entry: no private segment (scratch), no spilled VGPR or SGPR, at most 128
  VGPRs (four wavefronts per SIMD)."""
  spec = PROGRAMS[which]()
  text, table = kernel.generate(spec)
  fused = [k['name'] for k in table if k['kind'] == 'fused']
  assert len(fused) == (4 if which == 'fir1d' else 5)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  assert all(k['cols'] == 16 // elem for k in table if k['kind'] == 'fused')
  found = resource_figures(text, fused, str(tmp_path / (which + '.hsaco')))
  for kname, figures in found.items():
    assert figures['private_segment_fixed_size'] == 0, (kname, figures)
    assert figures['vgpr_spill_count'] == 0, (kname, figures)
    assert figures['sgpr_spill_count'] == 0, (kname, figures)
    assert 0 < figures['vgpr_count'] <= 128, (kname, figures)


# ---- planner ------------------------------------------------------------------------------

def one_case(dims, iterate, max_depth=0, split=(), valid_lo=(0,), valid_hi=(0,), final_only=0):
  return dict(ts.case(dims, iterate, max_depth, split), final_only=final_only,
              valid_lo=tuple(valid_lo), valid_hi=tuple(valid_hi))


def stored_cells(k, launch, n):
  """How often every cell of an array of n cells is stored by the launch: the kernel's own
  rule (kernel_stream1d.emit) on the launcher's grid."""
  lo, hi = launch['lo'][0], launch['hi'][0]
  assert launch['grid'][1:] == [1, 1]
  count = np.zeros(n, dtype=np.int32)
  origin = lo - lo % k['origin_align']
  segs, w_out = k['segs'], k['w_out']
  for block in range(launch['grid'][0]):
    for wave in range(4):
      xs0 = origin + (block * 4 * segs + wave) * w_out
      if xs0 >= hi:       # the wavefront leaves
        continue
      interior = xs0 - k['halo'][0] >= 0 and \
          xs0 + (segs - 1) * 4 * w_out - k['halo'][0] + LANES * k['cols'] <= n
      for s in range(segs):
        xs = xs0 + 4 * s * w_out
        first = xs - k['halo'][0]
        # whole-vector loads stay inside the array
        assert not interior or (first >= 0 and first + LANES * k['cols'] <= n)
        a, b = max(xs, lo), min(xs + w_out, hi)
        if a < b:
          assert a >= 0 and b <= n
          count[a:b] += 1
  return count


@pytest.mark.parametrize('app', APPS)
def test_grid_and_segments_store_every_cell_of_the_box_once(probe, tmp_path, app):  # noqa: F811
  spec, table = ts.program(app, 8)
  for depth, k in sorted(fused_of(table).items()):
    tile, align = k['tile'][0], k['origin_align']
    mlo, mhi = specmod.iteration_margins(spec, depth)[-1]
    # what a stored cell reads lies inside its segment
    assert k['halo'][0] >= mlo[0] and k['halo'][1] >= mhi[0]
    widths = [1, k['w_out'] - 1, k['w_out'], k['w_out'] + 1, tile - 1, tile, tile + 1,
              2 * tile - 1, 2 * tile, 2 * tile + 1]
    cases = [one_case((start + w + mlo[0] + mhi[0],), depth, depth, valid_lo=(start,))
             for start in range(align + 1) for w in widths]
    for c, r in ts.plan(probe, tmp_path, app, 8, cases, 2, 0):
      assert r['rc'] == 0, (c, r['error'])
      (launch,) = r['launches']
      assert table[launch['kernel']] is k
      lo, hi = launch['lo'][0], launch['hi'][0]
      assert lo == c['valid_lo'][0] + mlo[0] and hi == c['dims'][0] - mhi[0]
      assert launch['grid'][0] == ts.ceil_div(hi - lo + lo % align, tile)
      count = stored_cells(k, launch, c['dims'][0])
      assert (count[lo:hi] == 1).all(), (c, depth)
      assert count[:lo].sum() == 0 and count[hi:].sum() == 0, (c, depth)


@pytest.mark.parametrize('app', APPS)
def test_schedules_limits_splits_and_prices(probe, tmp_path, app):  # noqa: F811
  gen_iterate = 100
  spec, table = ts.program(app, gen_iterate)
  depths = sorted(fused_of(table))
  assert depths == [1, 2, 4, 8, 12]
  splits = {5: (4, 1), 13: (12, 1), 21: (8, 8, 4, 1), 3: (1, 1, 1), 8: (2, 2, 2, 2)}
  cases = [ts.case((n,), iterate, limit) for n in (100003, 1 << 20)
           for iterate in (1, 2, 3, 5, 8, 13, 21) for limit in (0, -1, 1, 2, 4, 8, 12)]
  cases += [ts.case((100003,), iterate, 0, split) for iterate, split in splits.items()]
  cases += [ts.case((1 << 28,), 100, limit) for limit in (0, 12)]      # full size
  for facts in ((1, 0), (8, 0)):
    for c, r in ts.plan(probe, tmp_path, app, gen_iterate, ts.variants(cases), *facts):
      assert r['rc'] == 0, (c, r['error'])
      ts.check_depths_and_boxes(spec, table, c, r)
      ts.check_routing(spec, table, c, r)
      kinds = {table[l['kernel']]['kind'] for l in r['launches']}
      ran = [table[l['kernel']]['depth'] for l in r['launches']]
      if c['max_depth'] <= 0 and not c['split']:
        # not in the default schedule (profiles/r10_stream1d.txt)
        assert kinds == {'stage'}
        assert all(l['est_us'] == 0 for l in r['launches'])
        continue
      assert kinds == {'fused'}
      assert sum(ran) == c['iterate']
      if c['split']:
        assert ran == list(c['split'])
      else:
        assert max(ran) <= c['max_depth']
      for l in r['launches']:
        k = table[l['kernel']]
        lo, hi = l['lo'][0], l['hi'][0]
        assert l['grid'] == [ts.ceil_div(hi - lo + lo % k['origin_align'], k['tile'][0]), 1, 1]
        assert l['est_us'] > 0 and l['lds'] == 0 and l['param'] == [0, 0, 0, 0]


def test_the_price_grows_with_the_extent_and_the_planner_goes_deep(probe, tmp_path):  # noqa: F811
  spec, table = ts.program('smooth1d', 100)
  cases = [one_case((n,), 12, 12, split=(12,)) for n in (1 << 16, 1 << 22, 1 << 25, 1 << 28)]
  cases.append(one_case((1 << 28,), 100, 12))
  planned = ts.plan(probe, tmp_path, 'smooth1d', 100, cases, 8, 0)
  prices = []
  for c, r in planned[:4]:
    (launch,) = r['launches']
    assert table[launch['kernel']]['depth'] == 12
    prices.append(launch['est_us'])
  assert prices[0] > 0 and prices == sorted(prices) and prices[3] > 4 * prices[1]
  # HBM bounds these kernels in the model: 2^28 floats in and out at 4.6 TB/s, plus halo
  assert 2 * 4 * 2 ** 28 / 4.6e12 * 1e6 < prices[3] < 1.25 * 2 * 4 * 2 ** 28 / 4.6e12 * 1e6
  # with prices the split is the model's: 100 = 8 x 12 + 4, never 100 launches of depth 1
  c, r = planned[4]
  ran = [table[l['kernel']]['depth'] for l in r['launches']]
  assert sum(ran) == 100 and len(ran) <= 10 and max(ran) == 12, ran


# ---- fixtures from the reference's own CPU loops ------------------------------------------

FIXTURES = sorted(k for k in MANIFEST if k.endswith('.npz'))


def test_fixture_set_is_what_the_script_writes():
  assert len(FIXTURES) == 2 * 4 * 2 * 2 and len(MANIFEST) == len(FIXTURES)
  for app in APPS:
    for it in (1, 2, 3, 4):
      for n in (37, 300):
        for kind in ('ramp', 'random'):
          assert '%s.iter%d.%d.%s.npz' % (app, it, n, kind) in MANIFEST


@pytest.mark.skipif(shutil.which('g++') is None, reason='the oracle needs g++')
@pytest.mark.parametrize('app', APPS)
def test_oracle_equals_the_reference_fixtures(app):
  """Array for array: the oracle's values on the output's box, the reference's zeros
  outside it (the oracle's ping-pong arrays keep earlier levels there)."""
  from oracle import soda_oracle
  spec = spec_of(app)
  orc = soda_oracle.Oracle(spec)
  name = spec['outputs'][0]
  seen = 0
  for fx in FIXTURES:
    meta = MANIFEST[fx]
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'stream1d', fx))
    want = data['out_' + name]
    assert hashlib.sha256(want.tobytes()).hexdigest() == meta['sha256'][name]
    got = orc.run([data['in_' + spec['inputs'][0]['name']]], iterate=meta['iterate'])[name]
    assert got.dtype == want.dtype
    lo, hi = specmod.iteration_boxes(spec, meta['iterate'])[-1][name]
    sl = slice(-lo[0], meta['dims'][0] - hi[0])
    clean = np.zeros_like(got)
    clean[sl] = got[sl]
    assert clean[sl].size > 0 and clean[sl].std() > 0
    assert np.array_equal(clean.view(np.uint8), want.view(np.uint8)), fx
    seen += 1
  assert seen == 16


# ---- the other families' tables -----------------------------------------------------------

def digest(spec, **options):
  text, table = kernel.generate(spec, **options)
  return (hashlib.sha256(text.encode()).hexdigest(),
          hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest())


@pytest.mark.parametrize('app', ['jacobi2d', 'blur', 'jacobi3d', 'wave2d'])
def test_tables_of_other_dimensions_are_unchanged(app, monkeypatch):
  """generate() with and without the 1-D family in the family list: the same text and the
  same table, byte for byte (the family returns before anything for dim != 1)."""
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  load = lambda **kw: specmod.spec_from_stencil(frontend.load(path, **kw))     # noqa: E731
  assert kernel.stream1d_kernels in kernel.FAMILIES
  cases = [(load(), {}), (load(iterate=4), dict(max_depth=4)), (load(iterate=8), dict(segs=2))]
  with_family = [digest(spec, **o) for spec, o in cases]
  monkeypatch.setattr(kernel, 'FAMILIES', tuple(
      f for f in kernel.FAMILIES if f is not kernel.stream1d_kernels))
  assert with_family == [digest(spec, **o) for spec, o in cases]
  # ... and it is that family, and nothing else, that makes the 1-D tables
  _, table = kernel.generate(spec_of('smooth1d'))
  assert all(k['kind'] == 'stage' for k in table)
