"""LDS-plane kernels over several outputs (soda_hip/codegen/kernel_stream3d_lds.py with
fields=True; kernel.generate's `lds_fields`), without a GPU: the switch is opt-in, the three
samples get exactly one `<app>_fused_k1lf` whose register windows are the hulls over their
stages, it compiles for gfx950 without scratch or spills, programs outside the form keep
their stage kernels and a note in the metadata that names the reason, every other program
keeps table and text, the checker agrees with the reference's fixtures, the launch planner
packs the growing extras of acoustic3d up to the byte's limit, and sodac carries the switch
into every product."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from soda_hip.codegen import (kernel, kernel_common, kernel_fields3d, kernel_stream2d,
                              kernel_stream3d_lds)
from soda_hip.codegen import spec as specmod

import test_schedule_fields as tsf
from conftest import ROOT, SAMPLES
from codegen_util import (HIPCC, READELF, SODAC, notes_of, resource_figures, spec_of,
                          spec_of_text, without_meta)
from test_lds3d_codegen import RANDOM, RANDOM_3D, lds_note
from test_schedule_fields import probes      # noqa: F401  (the planner probes, built once)

APPS = ('acoustic3d', 'skewwave3d', 'deriv3d')
SAMPLES_3D = ('jacobi3d', 'heat3d', 'denoise3d', 'wave3d', 'maxwell3d', 'grad3d', 'mix3d',
              'star3d', 'iso3dfd', 'skewstar3d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'lds3d_fields_manifest.json')) as _f:
  MANIFEST = json.load(_f)


def switches(app):
  """deriv3d is one pass over one input: in a fused form's class only with fuse_outputs"""
  return dict(lds_fields=True, fuse_outputs=app == 'deriv3d')


def fields_note(text):
  return kernel_common.read_meta_from_source(text).get('lds_fields')


# ---- the tables ------------------------------------------------------------------------------

OLD_NOTES = {
    'acoustic3d': ['// depth 1 not fused: depth 1 leaves no output cells in a 64x8 tile'],
    'skewwave3d': ['// depth 1 not fused: x offset -3 exceeds the 1 columns a lane holds'],
    'deriv3d': ['// depth 1 not fused: stream3d handles single-output programs'],
}


@pytest.mark.parametrize('app', APPS)
def test_without_the_switch_stage_kernels_only(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  assert [k['kind'] for k in table] == ['stage'] * len(spec['outputs'])
  assert '_fused_k' not in text and notes_of(text) == OLD_NOTES[app]
  assert fields_note(text) is None and lds_note(text) is None
  assert kernel.generate(spec, lds_fields=False) == (text, table)


@pytest.mark.parametrize('app', APPS)
def test_with_the_switch_one_fused_kernel(app):
  spec = spec_of(app)
  n_out = len(spec['outputs'])
  plain = kernel.generate(spec, fuse_outputs=app == 'deriv3d')[1]
  text, table = kernel.generate(spec, **switches(app))
  assert table[:-1] == plain and [k['kind'] for k in table] == ['stage'] * n_out + ['fused']
  k = table[-1]
  assert k['name'] == app + '_fused_k1lf' and k['depth'] == 1 and k['stage'] == -1
  assert k['fields'] == n_out and k['lds_planes'] == 1
  assert 0 < k['lds_bytes'] <= 65536 and k['est_vgprs'] <= 250
  # the entry against geometry(): tile, halo and LDS of the shape it names
  lowered = specmod.inline_pointwise(spec)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  C = 16 // elem
  lanes_x = k['tile'][0] // C
  _, fields = kernel_stream3d_lds.analyse_fields(lowered)
  geo = kernel_stream3d_lds.geometry(fields, elem, k['waves'], k['rows'], lanes_x)
  assert k['tile'] == [geo['TX'], geo['TY'], 64, 1] and k['block'] == [geo['threads'], 1, 1]
  assert k['halo'] == [geo['HXL'], geo['HXH'], geo['HYL'], geo['HYH']]
  assert k['lds_bytes'] == geo['lds_bytes'] == 2 * geo['PITCH'] * geo['ROWS'] * elem
  assert k['cols'] == C == k['origin_align'] and k['tile'][:2] == [k['w_out'], k['r_out']]
  # the halo covers the hull of the windows, in whole vectors along x
  lo, hi = spec['radius']['lo'], spec['radius']['hi']
  assert k['halo'] == [-(-lo[0] // C) * C, -(-hi[0] // C) * C, lo[1], hi[1]]
  assert k['fill_rows'] == lo[2] + hi[2] + 1
  # bytes per plane: the LDS plane with its halo, the other inputs and every output tile for
  # tile; arithmetic: every stage's operators
  cells = k['tile'][0] * k['tile'][1]
  assert k['loaded_cells'] == geo['PITCH'] * geo['ROWS'] + (len(fields) - 1) * cells
  assert k['step_bytes'] == (k['loaded_cells'] + n_out * cells) * elem
  assert k['step_valu'] == k['waves'] * kernel.arithmetic_weight(spec) * k['rows'] * C * 2
  # the old notes stay, and the metadata names the kernel; the other switch says nothing
  # (deriv3d under fuse_outputs: kernel_fields3d's refusal instead of kernel_stream3d's)
  assert notes_of(text) == (OLD_NOTES[app] if app != 'deriv3d' else OLD_NOTES['acoustic3d'])
  assert fields_note(text) == k['name'] and lds_note(text) is None
  assert text.count('void %s(soda_hip_args a)' % k['name']) == 1
  assert kernel_common.read_meta_from_source(text)['kernels'] == table
  # both LDS switches together: the same table, and the one-output form's refusal
  both_text, both = kernel.generate(spec, lds_planes=True, **switches(app))
  assert both == table and without_meta(both_text) == without_meta(text)
  assert lds_note(both_text) == 'not fused: %d outputs: the LDS-plane form stores one' % n_out
  # a named shape is taken as it is
  _, forced = kernel.generate(spec, lds_shape=(4, 1, 16), **switches(app))
  assert forced[-1]['block'] == [256, 1, 1] and forced[-1]['rows'] == 1
  assert forced[-1]['tile'][:2] == [16 * C, 16] and forced[-1]['fields'] == n_out


def test_a_one_pass_program_needs_fuse_outputs_as_well():
  spec = spec_of('deriv3d')
  text, table = kernel.generate(spec)
  out, got = kernel.generate(spec, lds_fields=True)
  assert got == table and without_meta(out) == without_meta(text)
  assert fields_note(out) == ('not fused: a one-pass program with several outputs is fused '
                              'only with fuse_outputs')


def test_register_windows_are_the_hulls_over_the_stages():
  def by_name(app):
    stages, fields = kernel_stream3d_lds.analyse_fields(specmod.inline_pointwise(spec_of(app)))
    return stages, {f.name: f for f in fields}
  stages, f = by_name('acoustic3d')
  assert [(f[n].lds, f[n].keep) for n in ('u', 'up', 'vel')] == [(True, 10), (False, 2),
                                                                 (False, 2)]
  assert (f['u'].zlo, f['u'].zhi, f['u'].zc, f['u'].hx, f['u'].hy) == (-4, 4, 0, (4, 4), (4, 4))
  spec = specmod.inline_pointwise(spec_of('acoustic3d'))
  assert [kernel_stream3d_lds.passed_through(spec, s) for s in stages] == [None, 'u', 'vel']
  # skewwave3d: en reads e in-plane one plane up, hn reads it along z only - one window
  stages, f = by_name('skewwave3d')
  e, h = f['e'], f['h']
  assert (e.zlo, e.zhi, e.zc, e.hx, e.hy, e.keep) == (-1, 2, 1, (3, 5), (2, 3), 5)
  assert (h.lds, h.zlo, h.zhi, h.keep) == (False, 0, 0, 2)
  hn = stages[1]
  assert hn['name'] == 'hn' and all(tuple(rel[:2]) == (0, 0) for _, rel in hn['loads'])
  assert sorted(tuple(rel) for n, rel in hn['loads'] if n == 'e') == [(0, 0, -1), (0, 0, 0)]
  spec = specmod.inline_pointwise(spec_of('skewwave3d'))
  assert [kernel_stream3d_lds.passed_through(spec, s) for s in stages] == [None, None]
  # deriv3d: the only in-plane reads are at plane 0, and dz reads none
  stages, f = by_name('deriv3d')
  (g,) = f.values()
  assert (g.zlo, g.zhi, g.zc, g.hx, g.hy) == (-4, 4, 0, (4, 4), (4, 4))
  assert {rel[2] for rel in g.rels if rel[:2] != (0, 0)} == {0}
  dz = stages[2]
  assert dz['name'] == 'dz' and all(tuple(rel[:2]) == (0, 0) for _, rel in dz['loads'])
  # the estimate counts the cells of the outputs that are computed, not of those handed on
  for app, computed in (('acoustic3d', 1), ('skewwave3d', 2), ('deriv3d', 3)):
    spec = specmod.inline_pointwise(spec_of(app))
    elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
    _, fields = kernel_stream3d_lds.analyse_fields(spec)
    geo = kernel_stream3d_lds.geometry(fields, elem, 8, 2, 16)
    one = kernel_stream3d_lds.estimate_vgprs(fields, elem, geo, 2)
    entry = kernel_stream3d_lds.emit(spec, 1, 8, 2, 16, fields=True)[1]
    assert entry['est_vgprs'] == one + (computed - 1) * 2 * (16 // elem) * (elem // 4)


# ---- the compiler ----------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', APPS)
def test_kernels_compile_for_gfx950_without_scratch_or_spills(app, tmp_path):
  """From the compiler's resource report: no private segment, no spilled VGPRs, no SGPRs
  parked in VGPR lanes, the static LDS of the entry; array subscripts in bounds at compile
  time."""
  text, table = kernel.generate(spec_of(app), **switches(app))
  kname = table[-1]['name']
  figures = resource_figures(text, [kname], str(tmp_path / (app + '.hsaco')),
                             extra_flags=['-Werror=array-bounds'])[kname]
  assert figures['private_segment_fixed_size'] == 0, (kname, figures)
  assert figures['vgpr_spill_count'] == 0, (kname, figures)
  assert figures['sgpr_spill_count'] == 0, (kname, figures)
  assert 0 < figures['vgpr_count'] <= 256, (kname, figures)
  assert figures['group_segment_fixed_size'] == table[-1]['lds_bytes'], (kname, figures)


# ---- refusals --------------------------------------------------------------------------------

_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: 2\n'
STAGE_READS_STAGE = _HEAD % 'chained' + '''input float: a
input float: b(32, 32, *)
output float: c(0, 0, 0) = a(3, 0, 0) + a(-3, 0, 0) + b(0, 0, 0)
output float: d(0, 0, 0) = c(0, 3, 0) + a(0, 0, 0)
'''
FOUR_OUTPUTS = _HEAD % 'fourouts' + ''.join(
    'input float: a%d%s\n' % (j, '(32, 32, *)' if j == 3 else '') for j in range(4)) + ''.join(
    'output float: b%d(0, 0, 0) = a%d(3, 0, 0) + a%d(0, -3, 0)\n' % (j, j, (j + 1) % 4)
    for j in range(4))
MIXED_WIDTHS = _HEAD % 'mixed' + '''input float: a
input double: b(32, 32, *)
output float: c(0, 0, 0) = a(3, 0, 0) + a(-3, 0, 0)
output double: d(0, 0, 0) = b(0, 3, 0) + b(0, 0, -1)
'''
TWO_BYTES = _HEAD % 'shorts' + '''input uint16: a
input uint16: b(32, 32, *)
output uint16: c(0, 0, 0) = a(9, 0, 0) + a(-9, 0, 0) + b(0, 0, 0)
output uint16: d(0, 0, 0) = b(0, 3, 0) * 3
'''
TWO_PLANES = _HEAD % 'twoplanes' + '''input float: a
input float: b(32, 32, *)
output float: c(0, 0, 0) = a(3, 0, 0) + b(0, 0, 0)
output float: d(0, 0, 0) = a(0, 3, 1) + b(0, 0, 0)
'''


@pytest.mark.parametrize('text,reason', [
    (STAGE_READS_STAGE, 'stage d reads stage c: the LDS-plane form over fields takes stages '
                        'that read inputs only'),
    (FOUR_OUTPUTS, '4 outputs: the LDS-plane form over fields stores 2 to 3'),
    (MIXED_WIDTHS, 'mixed element widths'),
    (TWO_BYTES, '2-byte elements: the LDS-plane form handles 4- and 8-byte ones'),
    (TWO_PLANES, 'input a is read off the z axis at plane offsets 0 and 1: one plane of an '
                 'input lies in LDS')])
def test_programs_outside_the_form_keep_their_stage_kernels_and_get_a_note(text, reason):
  """The note is the entry `lds_fields` of the metadata: everything before the metadata is
  the text without the switch."""
  spec = spec_of_text(text)
  plain_text, plain = kernel.generate(spec)
  assert all(k['kind'] == 'stage' for k in plain) and fields_note(plain_text) is None
  out, table = kernel.generate(spec, lds_fields=True)
  assert table == plain and len(table) == len(specmod.inline_pointwise(spec)['stages'])
  assert fields_note(out) == 'not fused: ' + reason
  assert without_meta(out) == without_meta(plain_text)
  with pytest.raises(kernel_stream2d.NotFusable) as e:
    kernel_stream3d_lds.emit(specmod.inline_pointwise(spec), fields=True)
  assert str(e.value) == reason


@pytest.mark.parametrize('app,note', [
    ('grad2d', 'not fused: the LDS-plane form handles 3-D programs'),
    ('star3d', 'not concerned: one output'),
    ('jacobi2d', 'not concerned: one output')])
def test_two_dimensional_and_single_output_programs(app, note):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  out, got = kernel.generate(spec, lds_fields=True)
  assert got == table and without_meta(out) == without_meta(text)
  assert fields_note(out) == note
  if app == 'star3d':
    assert all(k['kind'] == 'stage' for k in table)
    with pytest.raises(kernel_stream2d.NotFusable, match='1 outputs: the LDS-plane form over '
                                                         'fields stores 2 to 3'):
      kernel_stream3d_lds.emit(specmod.inline_pointwise(spec), fields=True)


def test_what_no_shape_fits_is_refused_with_the_figures():
  lowered = specmod.inline_pointwise(spec_of('acoustic3d'))
  with pytest.raises(kernel_stream2d.NotFusable, match='would need about 3[0-9][0-9] VGPRs'):
    kernel_stream3d_lds.emit(lowered, 1, 4, 4, 32, fields=True)
  with pytest.raises(kernel_stream2d.NotFusable, match=r'84480 bytes of LDS \(cap 65536\)'):
    kernel_stream3d_lds.emit(lowered, 1, 8, 4, 64, fields=True)
  with pytest.raises(kernel_stream2d.NotFusable, match='depth 1'):
    kernel_stream3d_lds.emit(lowered, 2, fields=True)


# ---- every other program keeps its table -----------------------------------------------------

def test_random_programs_keep_table_and_text():
  assert len(RANDOM_3D) == 33
  for key in RANDOM_3D:
    spec = spec_of_text(RANDOM[key]['text'])
    text, table = kernel.generate(spec)
    out, got = kernel.generate(spec, lds_fields=True)
    assert got == table, key
    assert without_meta(out) == without_meta(text), key
    note = fields_note(out)
    if len(spec['outputs']) < 2:
      assert note == 'not concerned: one output', key
    elif any(k['kind'] == 'fused' and k['depth'] == 1 for k in table):
      assert note.startswith('not wanted: %s_fused_k1' % spec['app_name']), key
    else:
      assert note.startswith('not fused: '), key


@pytest.mark.parametrize('app', SAMPLES_3D)
def test_existing_samples_keep_table_and_text(app):
  spec = spec_of(app)
  for fuse in (False, True):
    text, table = kernel.generate(spec, fuse_outputs=fuse)
    out, got = kernel.generate(spec, fuse_outputs=fuse, lds_fields=True)
    assert got == table and without_meta(out) == without_meta(text)
    assert '_fused_k1lf' not in out


@pytest.mark.parametrize('app', APPS)
def test_the_one_output_switch_still_refuses_the_new_samples(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  out, got = kernel.generate(spec, lds_planes=True)
  assert got == table and without_meta(out) == without_meta(text)
  assert lds_note(out) == 'not fused: %d outputs: the LDS-plane form stores one' % len(
      spec['outputs'])
  assert fields_note(out) is None


# ---- fixtures --------------------------------------------------------------------------------

FIXTURES = sorted(k for k in MANIFEST if k.endswith('.npz'))
CASES = ('41x19x18', '23x27x21')
ITERATIONS = (('acoustic3d', (1, 2)), ('skewwave3d', (1, 2)), ('deriv3d', (1,)))


def test_fixture_set_is_what_the_script_writes():
  assert len(FIXTURES) == 20 == len(MANIFEST)
  assert sorted(FIXTURES) == sorted(os.listdir(os.path.join(GOLDEN, 'lds3d_fields')))
  for app, iterations in ITERATIONS:
    for it in iterations:
      for dims in CASES:
        for kind in ('ramp', 'random'):
          fx = '%s.iter%d.%s.%s.npz' % (app, it, dims, kind)
          assert fx in MANIFEST
          assert os.path.getsize(os.path.join(GOLDEN, 'lds3d_fields', fx)) < 1 << 20


@pytest.mark.skipif(shutil.which('g++') is None, reason='the oracle needs g++')
@pytest.mark.parametrize('app', APPS)
def test_oracle_equals_the_reference_fixtures(app):
  """Array for array: the oracle's values on each output's box, the reference's zeros outside
  it, and the bytes the manifest pins."""
  from oracle import soda_oracle
  spec = spec_of(app)
  orc = soda_oracle.Oracle(spec)
  n = 0
  for fx in FIXTURES:
    meta = MANIFEST[fx]
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'lds3d_fields', fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    assert all(a.shape == tuple(reversed(meta['dims'])) for a in inputs)
    got = orc.run(inputs, iterate=meta['iterate'])
    boxes = specmod.iteration_boxes(spec, meta['iterate'])[-1]
    for name in spec['outputs']:
      want = data['out_' + name]
      assert hashlib.sha256(want.tobytes()).hexdigest() == meta['sha256'][name], (fx, name)
      lo, hi = boxes[name]
      sl = tuple(slice(-lo[d], max(-lo[d], meta['dims'][d] - hi[d])) for d in (2, 1, 0))
      clean = np.zeros_like(got[name])
      clean[sl] = got[name][sl]
      assert clean[sl].size > 0
      assert np.array_equal(clean.view(np.uint8), want.view(np.uint8)), (fx, name)
    n += 1
  assert n == (4 if app == 'deriv3d' else 8)


# ---- the launch planner ----------------------------------------------------------------------

def planned(probes, tmp_path, monkeypatch, app, cap, cases):      # noqa: F811
  """test_schedule_fields.plan_fields on the table generated with the switch."""
  source = spec_of(app, iterate=cap)
  table = kernel.generate(source, **switches(app))[1]
  spec = specmod.inline_pointwise(source)
  monkeypatch.setattr(tsf, 'program', lambda name: (spec, table))
  return spec, table, tsf.plan_fields(probes, tmp_path, app, cases)


def ceil_div(a, b):
  return -(-a // b)


def grid_of(result, i):
  f = result['lines'][i].split()
  assert f[12] == 'grid'
  return [int(v) for v in f[13:16]]


def test_planner_packs_the_growing_extras_of_acoustic3d(probes, tmp_path, monkeypatch):  # noqa: F811
  """600^3 under depth limit 1.  iterate 4: four launches of acoustic3d_fused_k1lf, their
  extras those of kernel_fields3d.output_extras, the grid over the union of the boxes (velc
  keeps the whole array).  The velocity output's extra grows by 4 per iteration: 63
  iterations plan (252), 64 are the documented error (256 > 255), and plan per stage."""
  dims = (600, 600, 600)
  zero = [(0, 0, 0)] * 3
  cases = [dict(dims=dims, iterate=it, max_depth=md, lo=zero, hi=zero)
           for it, md in ((4, 1), (63, 1), (64, 1), (64, -1))]
  spec, table, (four, most, beyond, staged) = planned(probes, tmp_path, monkeypatch,
                                                      'acoustic3d', 64, cases)
  k = table[-1]
  assert four['rc'] == 0, four['error']
  assert [table[l['kernel']]['name'] for l in four['launches']] == ['acoustic3d_fused_k1lf'] * 4
  for i, l in enumerate(four['launches']):
    m = 4 * (i + 1)
    assert l['lo'][:3] == [m] * 3 and l['hi'][:3] == [600 - m] * 3
    extras = kernel_fields3d.output_extras(spec, i, 1)
    assert [tuple(tsf.extras_of(3, l, j)) for j in range(3)] == extras
    assert extras == [(0,) * 6, (4,) * 6, (m,) * 6]
    assert l['param'][1:] == kernel_fields3d.pack_extras(extras)
    # the union is the whole array: tiles from column 0, row 0, plane 0
    chunk = l['param'][0]
    assert chunk >= 8
    assert grid_of(four, i) == [ceil_div(600, k['tile'][0]), ceil_div(600, k['tile'][1]),
                                ceil_div(600, chunk)]
  assert most['rc'] == 0 and len(most['launches']) == 63
  assert {table[l['kernel']]['name'] for l in most['launches']} == {'acoustic3d_fused_k1lf'}
  assert max(tsf.extras_of(3, most['launches'][-1], 2)) == 252
  assert beyond['rc'] == -22 and 'limit 255' in beyond['error'], beyond
  assert staged['rc'] == 0 and len(staged['launches']) == 64 * 3
  assert all(table[l['kernel']]['kind'] == 'stage' for l in staged['launches'])


def test_planner_resumes_skewwave3d_with_per_field_regions(probes, tmp_path, monkeypatch):  # noqa: F811
  """k2 iterations from the per-field margins of k1: every launch's unpacked boxes are those
  of ONE run of k1 + k2 iterations, the launch's box their intersection, the grid their
  union."""
  dims = (70, 40, 33)
  source = spec_of('skewwave3d', iterate=3)
  lowered = specmod.inline_pointwise(source)
  cases = []
  for k1, k2 in ((0, 3), (1, 1), (1, 2), (2, 1)):
    m = tsf.margins_after(lowered, k1)
    cases.append(dict(dims=dims, iterate=k2, max_depth=1, k1=k1,
                      lo=[lo for lo, _ in m], hi=[hi for _, hi in m]))
  spec, table, results = planned(probes, tmp_path, monkeypatch, 'skewwave3d', 3, cases)
  k = table[-1]
  levels = specmod.iteration_boxes(spec, 3)
  for c, r in zip(cases, results):
    assert r['rc'] == 0, (c, r['error'])
    assert [table[l['kernel']]['name'] for l in r['launches']] == \
        ['skewwave3d_fused_k1lf'] * c['iterate']
    for i, l in enumerate(r['launches']):
      done = c['k1'] + i + 1
      own = []
      for j, o in enumerate(spec['outputs']):
        ex = tsf.extras_of(3, l, j)
        olo, ohi = levels[done - 1][o]
        box = [(l['lo'][d] - ex[d], l['hi'][d] + ex[3 + d]) for d in range(3)]
        assert box == [(-olo[d], dims[d] - ohi[d]) for d in range(3)], (c, j, done)
        own.append(box)
      union = [(min(b[d][0] for b in own), max(b[d][1] for b in own)) for d in range(3)]
      for d in range(3):
        assert l['lo'][d] == max(b[d][0] for b in own)
        assert l['hi'][d] == min(b[d][1] for b in own)
      x0 = union[0][0] - union[0][0] % k['origin_align']
      assert grid_of(r, i) == [ceil_div(union[0][1] - x0, k['tile'][0]),
                               ceil_div(union[1][1] - union[1][0], k['tile'][1]),
                               ceil_div(union[2][1] - union[2][0], l['param'][0])]


# ---- sodac -----------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'acoustic3d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-lds-fields', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['acoustic3d.h', 'acoustic3d.hsaco', 'acoustic3d.py',
                                     'acoustic3d_host.cpp', 'acoustic3d_kernel.hip']
  text = (out / 'acoustic3d_kernel.hip').read_text()
  assert text == kernel.generate(spec_of('acoustic3d'), lds_fields=True)[0]
  assert (out / 'acoustic3d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'acoustic3d.py').read_text()
  compile(shim, 'acoustic3d.py', 'exec')
  assert 'lds_fields=True' in shim and 'program.set_max_depth(1)' in shim
  host_cpp = (out / 'acoustic3d_host.cpp').read_text()
  assert '"acoustic3d_fused_k1lf"' in host_cpp
  assert 'soda_hip_plan_set_max_depth(plan, 1)' in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'acoustic3d_host.cpp')])
  # --hip-lds-planes alone on the same program: only the metadata says so
  plain, planes = tmp_path / 'plain', tmp_path / 'planes'
  for base, flags in ((plain, []), (planes, ['--hip-lds-planes'])):
    r = subprocess.run([sys.executable, SODAC, sample] + flags + [
        '--hip-kernel', str(base) + '.hip', '--hip-host', str(base) + '.py',
        '--hip-host-cpp', str(base) + '.cpp'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for suffix in ('.hip', '.py', '.cpp'):
      got = open(str(base) + suffix).read()
      assert 'fused_k1l' not in got and 'lds_fields' not in got and 'set_max_depth' not in got
  assert without_meta(open(str(planes) + '.hip').read()) == \
      without_meta(open(str(plain) + '.hip').read())
  assert lds_note(open(str(planes) + '.hip').read()) == \
      'not fused: 3 outputs: the LDS-plane form stores one'
  assert open(str(planes) + '.cpp').read() == open(str(plain) + '.cpp').read()


def test_the_measurement_tool_prints_its_usage():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'lds3d', 'lds3d_bench.py'),
                      '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert '--fields' in r.stdout and 'lds_fields' in r.stdout
