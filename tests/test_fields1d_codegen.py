"""Fused kernels for iterated 1-D programs over several fields (soda_hip/codegen/
kernel_fields1d.py), without a GPU: what the kernel tables hold, what the generator refuses
and why, that the single-array 1-D family and every other family print what they printed
before, the per-output extras and their packing, the planner's launch lists (fresh and
resumed from per-field valid regions) with every output's store ranges recomputed from the
kernel's own rule, the checker against the reference's fixtures, and that every kernel
compiles for gfx950 within 128 VGPRs and without scratch."""
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from soda_hip.codegen import kernel, kernel_fields1d, kernel_stream1d
from soda_hip.codegen import spec as specmod

from codegen_util import HIPCC, READELF, resource_figures, spec_of, spec_of_text
from conftest import ROOT, SAMPLES
import test_schedule as ts
import test_schedule_fields as tsf
import test_stream1d_codegen as s1d
from test_schedule import probe            # noqa: F401 - the planner probes, built once
from test_schedule_fields import probes    # noqa: F401   per module

APPS = ('wave1d', 'skewpair1d', 'fdtd1d', 'mixpair1d')
# STREAM1D_DEPTHS capped by the sample's own `iterate` (8, 6, 8, 5)
DEPTHS = {'wave1d': [1, 2, 4, 8], 'skewpair1d': [1, 2, 4], 'fdtd1d': [1, 2, 4, 8],
          'mixpair1d': [1, 2, 4]}
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'fields1d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
LANES = 64


def sample_path(app):
  path = os.path.join(SAMPLES, app + '.soda')
  return path if os.path.exists(path) else os.path.join(SAMPLES, 'extra', app + '.soda')


def retyped(app, dsl_type, was='float'):
  with open(sample_path(app)) as f:
    return spec_of_text(f.read().replace(was + ':', dsl_type + ':'))


def fused_of(table):
  return {k['depth']: k for k in table if k['kind'] == 'fused'}


# ---- tables -------------------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_tables_hold_the_fused_depths(app):
  """(Stage-only tables before this family existed.)"""
  spec = spec_of(app)
  assert spec['dim'] == 1 and len(spec['inputs']) == len(spec['outputs']) == 2
  text, table = kernel.generate(spec)
  lowered = specmod.inline_pointwise(spec)
  fused = fused_of(table)
  assert sorted(fused) == DEPTHS[app]
  assert sorted(fused) == [d for d in kernel.STREAM1D_DEPTHS if d <= spec['iterate']]
  for depth, k in fused.items():
    assert k['fields'] == 2 and k['fill_rows'] == 0
    assert k['segs'] == kernel_fields1d.default_segs(2) == 4
    assert k['tile'] == [4 * k['segs'] * k['w_out'], 1, 1, 1]
    assert k['stage'] == -1 and k['block'] == [256, 1, 1]
    assert k['origin_align'] == k['cols']
    assert k['step_bytes'] > 0 and k['step_valu'] > 0
    assert 'groups' not in k and 'stack' not in k
    # the halo is the hull of the composed window over all fields, in whole vectors
    lo, hi = specmod.iteration_margins(lowered, depth)[-1]
    C = k['cols']
    assert [-(-lo[0] // C) * C, -(-hi[0] // C) * C] == k['halo']
    # per workgroup and launch: every field's loaded vectors in, every output's tile out
    elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
    assert k['step_bytes'] == 2 * (4 * LANES * k['segs'] * C + k['tile'][0]) * elem
  assert sum(k['kind'] == 'stage' for k in table) == len(lowered['stages'])
  assert [k['kind'] for k in table] == ['stage'] * len(lowered['stages']) + ['fused'] * len(fused)
  assert 'not fused' not in text


def test_iterate_caps_the_depths_and_segs_is_an_option():
  _, table = kernel.generate(spec_of('wave1d', iterate=5))
  assert sorted(fused_of(table)) == [1, 2, 4]
  _, table = kernel.generate(spec_of('wave1d', iterate=13))
  assert sorted(fused_of(table)) == [1, 2, 4, 8, 12]
  _, table = kernel.generate(spec_of('wave1d', iterate=13), max_depth=4)
  assert sorted(fused_of(table)) == [1, 2, 4]
  _, table = kernel.generate(spec_of('wave1d'), depths=[3])
  assert sorted(fused_of(table)) == [1, 3]
  _, table = kernel.generate(spec_of('fdtd1d'), segs=2)
  for k in fused_of(table).values():
    assert k['segs'] == 2 and k['tile'][0] == 8 * k['w_out']
  # segs defaults to at most 8 vector loads in flight per lane
  assert [kernel_fields1d.default_segs(n) for n in (2, 3, 4, 5, 6)] == [4, 2, 2, 1, 1]
  assert kernel.form_options('fields1d', dict(segs=2, rows=4, align='none')) == dict(segs=2)


@pytest.mark.parametrize('which,cols', [('float', 4), ('uint16', 8), ('double', 2)])
def test_geometry(which, cols):
  spec = spec_of('mixpair1d') if which == 'uint16' else retyped('wave1d', which)
  _, table = kernel.generate(spec)
  fused = fused_of(table)
  assert fused
  for k in fused.values():
    assert k['cols'] == cols and k['w_out'] + sum(k['halo']) == LANES * cols
    assert k['halo'][0] % cols == 0 and k['halo'][1] % cols == 0 and k['w_out'] >= cols


# ---- refusals -----------------------------------------------------------------------------

_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: 4\n'
SEVEN = _HEAD % 'seven' + ''.join(
    'input float: a%d%s\n' % (j, '(*)' if j == 6 else '') for j in range(7)) + ''.join(
        'output float: b%d(0) = a%d(0) + a%d(1)\n' % (j, j, (j + 1) % 7) for j in range(7))
WIDTHS = _HEAD % 'widths' + 'input float: f\ninput double: g(*)\n' \
    'output float: fn(0) = f(0) + f(1)\noutput double: gn(0) = g(0) + g(-1)\n'
FAR = _HEAD % 'farpair' + 'input float: f\ninput float: g(*)\n' \
    'output float: fn(0) = f(0) + g(5)\noutput float: gn(0) = g(0) + f(-1)\n'


@pytest.mark.parametrize('text,reason', [
    (SEVEN, '7 outputs: the launch arguments carry the boxes of 6'),
    (WIDTHS, 'fields of different widths'),
    (FAR, 'x offset 5 exceeds the 4 columns a lane holds')])
def test_refused_programs_keep_a_stage_only_table_and_say_why(text, reason):
  spec = spec_of_text(text)
  assert spec['dim'] == 1 and kernel_fields1d.multi_field(spec)
  source, table = kernel.generate(spec)
  assert table and all(k['kind'] == 'stage' for k in table)
  notes = [line for line in source.splitlines() if 'not fused' in line]
  # one note, this family's: the single-array family says nothing about such programs
  assert notes == ['// depth 1 not fused: ' + reason]
  with pytest.raises(kernel_fields1d.NotFusable):
    kernel_fields1d.emit(specmod.inline_pointwise(spec), 1)


def test_six_fields_are_taken_and_types_may_differ_at_equal_width():
  six = SEVEN.replace('input float: a6(*)\n', '').replace('input float: a5\n',
                                                           'input float: a5(*)\n')
  six = '\n'.join(l for l in six.splitlines() if not l.startswith('output float: b6')) + '\n'
  six = six.replace('a5(0) + a6(1)', 'a5(0) + a0(1)')
  _, table = kernel.generate(spec_of_text(six))
  fused = fused_of(table)
  assert sorted(fused) == [1, 2, 4] and all(k['fields'] == 6 and k['segs'] == 1
                                            for k in fused.values())
  mixed = WIDTHS.replace('double', 'int32')
  source, table = kernel.generate(spec_of_text(mixed))
  assert sorted(fused_of(table)) == [1, 2, 4]
  assert 'vec_widths_fused_k1_float' in source and 'vec_widths_fused_k1_int32_t' in source


@pytest.mark.parametrize('text,reason', [
    (s1d.FAR, 'x offset 5 exceeds the 4 columns a lane holds'),
    (s1d.TWO_IN, 'stream1d handles one input feeding one output (2 input(s), 1 output(s))'),
    (s1d.WIDEN, "the output (double) is not of the input's type (float)")])
def test_the_single_array_refusals_are_what_they_were(text, reason):
  source, table = kernel.generate(spec_of_text(text))
  assert all(k['kind'] == 'stage' for k in table)
  assert [line for line in source.splitlines() if 'not fused' in line] == \
      ['// depth 1 not fused: ' + reason]


# ---- the other families' output -----------------------------------------------------------

# sha256 of kernel_stream1d.emit's text before kernel_fields1d shared its load helper
STREAM1D_TEXT = {
    'smooth1d/1': 'c0ef0b3386dc2522f9689852cb5824a12ea2fe8c882aad37a3fe8f4b96810cf2',
    'smooth1d/2': '339e90bac77dc2263074d4e30c94fdcb0ed00b44350988423f2a8f42179a44f9',
    'smooth1d/4': '4677e2f4b950d0a371c309ad88649ca3cbd20c946785782adb70010d68c0c1ac',
    'smooth1d/8': 'a0d4f092a6a45f3cb29914650889f87928937de57c3f8e7d0aa09acf433af18e',
    'smooth1d/12': 'd715cdbf48ba129e1ce8ed3dfde1043735eaf3a5cfb2f233568f1b0903c1bfbb',
    'fir1d/1': 'ad49ebfb6027042cfc95bfab2df962b818cc1a46f5fd1455918e780f7e163037',
    'fir1d/2': '6f50fa2ac45f5efe13397012e51bc6c15d88b2c1b4f28c684bd2409a01507311',
    'fir1d/4': '51b7da0115f405b5f044e4a84cdd72039303d9d4afe8971b5f587633ca5b4654',
    'fir1d/8': 'b7ce5311effd0eb9c50bb8347ad570d05b0bc0d9b915e8fd8b7741068e669887',
    'fir1d/12': '2c6b45f07b66cb66ada746227cd0103ea94636774914c9da563d42741fd68765'}


def test_stream1d_prints_the_text_it_printed_before():
  for key, want in STREAM1D_TEXT.items():
    app, depth = key.split('/')
    text, _ = kernel_stream1d.emit(specmod.inline_pointwise(spec_of(app)), int(depth))
    assert hashlib.sha256(text.encode()).hexdigest() == want, key


def digest(spec, **options):
  text, table = kernel.generate(spec, **options)
  return (hashlib.sha256(text.encode()).hexdigest(),
          hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest())


def test_texts_and_tables_outside_the_new_class_are_unchanged(monkeypatch):
  """generate() with and without the family in the family list: the same text and the same
  table, byte for byte."""
  assert kernel.FAMILIES.index(kernel.fields1d_kernels) + 1 == \
      kernel.FAMILIES.index(kernel.stream1d_kernels)
  cases = [(spec_of(app), {}) for app in ('smooth1d', 'fir1d', 'jacobi2d', 'wave2d', 'jacobi3d',
                                          'wave3d')]
  cases += [(spec_of(app), dict(max_depth=4)) for app in ('smooth1d', 'fir1d')]
  with_family = [digest(spec, **o) for spec, o in cases]
  monkeypatch.setattr(kernel, 'FAMILIES', tuple(
      f for f in kernel.FAMILIES if f is not kernel.fields1d_kernels))
  assert with_family == [digest(spec, **o) for spec, o in cases]
  # ... and it is that family, and nothing else, that makes the new tables
  _, table = kernel.generate(spec_of('wave1d'))
  assert all(k['kind'] == 'stage' for k in table)


# ---- extras -------------------------------------------------------------------------------

def test_output_extras_are_the_differences_of_the_boxes():
  spec = specmod.inline_pointwise(spec_of('skewpair1d'))
  seen = set()
  for done in range(7):
    for depth in (1, 2, 4):
      boxes = specmod.iteration_boxes(spec, done + depth)[-1]
      lo = max(-boxes[o][0][0] for o in spec['outputs'])      # the intersection's margins
      hi = max(boxes[o][1][0] for o in spec['outputs'])
      want = [(lo + boxes[o][0][0], hi - boxes[o][1][0]) for o in spec['outputs']]
      got = kernel_fields1d.output_extras(spec, done, depth)
      assert got == want and all(v >= 0 for ex in got for v in ex)
      assert min(ex[0] for ex in got) == 0 and min(ex[1] for ex in got) == 0
      seen.add(tuple(got))
  assert len(seen) > 1                                  # they change along a sweep
  assert any(ex[0] != ex[1] for ex in seen)             # ... differ between the outputs
  assert any(a != b for ex in seen for a, b in ex)      # ... and between the sides


def test_pack_extras_round_trips():
  rng = np.random.default_rng(5)
  for n in range(1, kernel_fields1d.MAX_OUTPUTS + 1):
    extras = [tuple(int(v) for v in rng.integers(0, 256, size=2)) for _ in range(n)]
    words = kernel_fields1d.pack_extras(extras)
    assert len(words) == 3 and all(0 <= w < 2 ** 64 for w in words) and words[2] == 0
    assert kernel_fields1d.unpack_extras(words, n) == extras
    for j, (lo, hi) in enumerate(extras):     # include/soda_hip.h, soda_hip_args.param
      assert (words[j // 4] >> (16 * (j % 4))) & 0xffff == lo | hi << 8
  assert kernel_fields1d.pack_extras([(255, 0), (0, 255)]) == [255 | 255 << 24, 0, 0]
  with pytest.raises(AssertionError):
    kernel_fields1d.pack_extras([(256, 0)])


# ---- launch lists against the planner -----------------------------------------------------

PLANNED = ('skewpair1d', 'fdtd1d')
TOTAL = tsf.TOTAL


def parse(text, n_cases):
  results = []
  for line in text.splitlines():
    f = line.split()
    if f[0] == 'case':
      results.append(dict(rc=int(f[3]), depth=int(f[7]), error='', launches=[]))
    elif f[0] == 'error':
      results[-1]['error'] = line[6:]
    else:
      assert f[0] == 'L'
      results[-1]['launches'].append(dict(
          kernel=int(f[1]), lo=[int(v) for v in f[3:7]], hi=[int(v) for v in f[8:12]],
          grid=[int(v) for v in f[13:16]], param=[int(v) & (2 ** 64 - 1) for v in f[17:21]]))
  assert len(results) == n_cases
  return results


def plan_fields(probes, tmp_path, app, cases):      # noqa: F811
  """tests/schedule_fields_probe.cpp, as test_schedule_fields.plan_fields, grids included."""
  spec, table = tsf.program(app)
  req = tsf.header(spec, table) + struct.pack('=i', len(cases))
  for c in cases:
    req += struct.pack('=4i4q', c['max_depth'], 0, c['iterate'], 0, *tsf.pad4(c['dims'], 1))
    for side in ('lo', 'hi'):
      for v in c[side]:
        req += struct.pack('=4i', *tsf.pad4(v, 0))
  path = tmp_path / (app + '.fields1d.req')
  path.write_bytes(req)
  out = subprocess.check_output([probes['schedule_fields_probe'], str(path)], text=True)
  return parse(out, len(cases))


def stored_cells(k, launch, n, boxes):
  """How often every cell of every output's array of n cells is stored by the launch: the
  kernel's own rule (kernel_fields1d.emit) on the launcher's grid.  boxes: per output, its
  own (lo, hi)."""
  assert launch['grid'][1:] == [1, 1]
  counts = [np.zeros(n, dtype=np.int32) for _ in boxes]
  lo, hi = min(b[0] for b in boxes), max(b[1] for b in boxes)       # the union
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
        for count, (blo, bhi) in zip(counts, boxes):
          a, b = max(xs, blo), min(xs + w_out, bhi)
          if a < b:
            assert a >= 0 and b <= n
            count[a:b] += 1
  return counts


def check_fused_launches(spec, table, n, launches, k1):
  """Every launch of a sweep that starts at level k1: its extras, its grid, and that the
  segments store every output's box once and nothing else."""
  levels = specmod.iteration_boxes(spec, TOTAL)
  done = k1
  for l in launches:
    k = table[l['kernel']]
    assert k['kind'] == 'fused' and k['fields'] == len(spec['outputs'])
    extras = kernel_fields1d.output_extras(spec, done, k['depth'])
    assert l['param'][1:] == kernel_fields1d.pack_extras(extras) and l['param'][0] == 0
    done += k['depth']
    boxes = [(l['lo'][0] - ex[0], l['hi'][0] + ex[1]) for ex in extras]
    for o, box in zip(spec['outputs'], boxes):
      olo, ohi = levels[done - 1][o]
      assert box == (-olo[0], n - ohi[0]) and 0 <= box[0] < box[1] <= n
    assert l['lo'][0] == max(b[0] for b in boxes) and l['hi'][0] == min(b[1] for b in boxes)
    # the margins of the hull lie inside the segment's halo
    mlo, mhi = specmod.iteration_margins(spec, k['depth'])[-1]
    assert k['halo'][0] >= mlo[0] and k['halo'][1] >= mhi[0]
    ulo, uhi = min(b[0] for b in boxes), max(b[1] for b in boxes)
    assert l['grid'] == [ts.ceil_div(uhi - ulo + ulo % k['origin_align'], k['tile'][0]), 1, 1]
    for count, (blo, bhi) in zip(stored_cells(k, l, n, boxes), boxes):
      assert (count[blo:bhi] == 1).all() and count[:blo].sum() == 0 and count[bhi:].sum() == 0
  return done


@pytest.mark.parametrize('app', PLANNED)
def test_launch_lists_fresh_and_resumed(probes, tmp_path, app):      # noqa: F811
  spec, table = tsf.program(app)
  fused = fused_of(table)
  assert sorted(fused) == [1, 2, 4]
  n_stages = len(spec['stages'])
  seen = set()
  for n in (37, 300, 3 * fused[1]['tile'][0] + 17):
    cases = []
    for k1 in range(TOTAL):
      m = tsf.margins_after(spec, k1)
      for k2 in range(1, TOTAL - k1 + 1):
        for max_depth in (1, 2, 4, 0):
          cases.append(dict(dims=(n,), iterate=k2, max_depth=max_depth, k1=k1,
                            lo=[lo for lo, _ in m], hi=[hi for _, hi in m]))
    assert any(len(set(c['lo'])) > 1 or len(set(c['hi'])) > 1 for c in cases)
    for c, r in zip(cases, plan_fields(probes, tmp_path, app, cases)):
      assert r['rc'] == 0, (c, r['error'])
      launches = r['launches']
      if c['max_depth'] == 0:
        # no limit, no split: not in the default schedule
        assert len(launches) == c['iterate'] * n_stages
        assert all(table[l['kernel']]['kind'] == 'stage' for l in launches), c
        continue
      depths = [table[l['kernel']]['depth'] for l in launches]
      assert sum(depths) == c['iterate'] and max(depths) == r['depth'] <= c['max_depth'], (
          c, depths)
      seen.update((c['k1'] > 0, d) for d in depths)
      assert check_fused_launches(spec, table, n, launches, c['k1']) == c['k1'] + c['iterate']
  # every depth ran, fresh and resumed
  assert seen == {(resumed, d) for resumed in (False, True) for d in (1, 2, 4)}


@pytest.mark.parametrize('app', PLANNED)
def test_an_explicit_split_is_launched_as_given(probe, tmp_path, app):      # noqa: F811
  spec, table = ts.program(app, TOTAL)
  n = 3 * fused_of(table)[1]['tile'][0] + 17
  cases = [dict(ts.case((n,), 5, 0, split), final_only=0, valid_lo=(0,), valid_hi=(0,))
           for split in ((1, 4), (2, 1, 2))]
  for c, r in ts.plan(probe, tmp_path, app, TOTAL, cases, 2, 0):
    assert r['rc'] == 0, (c, r['error'])
    assert [table[l['kernel']]['depth'] for l in r['launches']] == list(c['split'])
    ts.check_routing(spec, table, c, r)
    for l in r['launches']:
      l['param'] = [v & (2 ** 64 - 1) for v in l['param']]
    assert check_fused_launches(spec, table, n, r['launches'], 0) == 5


# ---- fixtures from the reference's own CPU loops ------------------------------------------

FIXTURES = sorted(k for k in MANIFEST if k.endswith('.npz'))


def test_fixture_set_is_what_the_script_writes():
  assert len(FIXTURES) == 4 * 4 * 2 * 2 and len(MANIFEST) == len(FIXTURES)
  for app in APPS:
    for it in (1, 2, 3, 4):
      for n in (37, 300):
        for kind in ('ramp', 'random'):
          assert '%s.iter%d.%d.%s.npz' % (app, it, n, kind) in MANIFEST
  assert sorted(os.listdir(os.path.join(GOLDEN, 'fields1d'))) == FIXTURES


@pytest.mark.skipif(shutil.which('g++') is None, reason='the oracle needs g++')
@pytest.mark.parametrize('app', APPS)
def test_oracle_equals_the_reference_fixtures(app):
  """Array for array: the oracle's values on each output's own box, the reference's zeros
  outside it (the oracle's ping-pong arrays keep earlier levels there)."""
  from oracle import soda_oracle
  spec = spec_of(app)
  orc = soda_oracle.Oracle(spec)
  seen = 0
  for fx in FIXTURES:
    meta = MANIFEST[fx]
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'fields1d', fx))
    got = orc.run([data['in_' + t['name']] for t in spec['inputs']], iterate=meta['iterate'])
    boxes = specmod.iteration_boxes(spec, meta['iterate'])[-1]
    for name in spec['outputs']:
      want = data['out_' + name]
      assert hashlib.sha256(want.tobytes()).hexdigest() == meta['sha256'][name]
      assert got[name].dtype == want.dtype
      lo, hi = boxes[name]
      sl = slice(-lo[0], meta['dims'][0] - hi[0])
      clean = np.zeros_like(got[name])
      clean[sl] = got[name][sl]
      assert clean[sl].size > 0 and clean[sl].std() > 0
      assert np.array_equal(clean.view(np.uint8), want.view(np.uint8)), (fx, name)
    seen += 1
  assert seen == 16


# ---- compile ------------------------------------------------------------------------------

PROGRAMS = dict({app: (lambda app=app: spec_of(app)) for app in APPS},
                wave1d_double=lambda: retyped('wave1d', 'double'),
                wave1d_int32=lambda: retyped('wave1d', 'int32'))


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('which', sorted(PROGRAMS))
def test_kernels_compile_for_gfx950_within_128_registers(which, tmp_path):
  """Every fused entry at default options: no private segment (scratch), no spilled VGPR or
  SGPR, at most 128 VGPRs (four wavefronts per SIMD)."""
  spec = PROGRAMS[which]()
  text, table = kernel.generate(spec)
  fused = [k['name'] for k in table if k['kind'] == 'fused']
  assert len(fused) == len(DEPTHS[which.split('_')[0]])
  found = resource_figures(text, fused, str(tmp_path / (which + '.hsaco')))
  for kname, figures in found.items():
    print(kname, figures)
    assert figures['private_segment_fixed_size'] == 0, (kname, figures)
    assert figures['vgpr_spill_count'] == 0, (kname, figures)
    assert figures['sgpr_spill_count'] == 0, (kname, figures)
    assert 0 < figures['vgpr_count'] <= 128, (kname, figures)
