"""Far-tap 1-D kernels (kernel_stream1d / kernel_fields1d with `hops`; kernel.generate's
`far_taps`), without a GPU: the four samples get the usual fused kernels at the family's
depths with hop chains exactly as long as their reads need, nothing changes without the
switch or for any other program, the shipped units compile for gfx950 without scratch or
spilled registers and inside their register estimate, the refusals of the neighbour-lane forms
are what they were, and sodac, the shim and build() carry the switch."""
import hashlib
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from soda_hip.codegen import (host_shim, kernel, kernel_common, kernel_fields1d,
                              kernel_stream1d, kernel_stream2d, switches)
from soda_hip.codegen import spec as specmod

from conftest import ROOT, SAMPLES
from codegen_util import HIPCC, SODAC, resource_figures, spec_of, spec_of_text, without_meta

APPS = ('lowpass1d', 'dfir1d', 'skewfir1d', 'acoustic1d')
# per sample, per fused depth: (halo lo, halo hi, cells of a segment that are stored).  Halos
# are whole lanes (4 floats, 2 doubles) over the window composed over the depth: lowpass1d's
# radius 16 per iteration; dfir1d's and acoustic1d's radius 8; skewfir1d's two stages compose
# to 31 below and 7 above per iteration, 62 / 14 over two.
TABLE = {
    'lowpass1d': {1: (16, 16, 224), 2: (32, 32, 192), 4: (64, 64, 128)},
    'dfir1d': {1: (8, 8, 112), 2: (16, 16, 96), 4: (32, 32, 64)},
    'skewfir1d': {1: (32, 8, 216), 2: (64, 16, 176)},
    'acoustic1d': {1: (8, 8, 112), 2: (16, 16, 96), 4: (32, 32, 64)},
}
# segments a wavefront takes: four, and two where three fields share the loads in flight
SEGS = {'lowpass1d': 4, 'dfir1d': 4, 'skewfir1d': 4, 'acoustic1d': 2}
# lanes the lowered program reads away: (below, above) over all its stages
HOPS = {'lowpass1d': (4, 4), 'dfir1d': (4, 4), 'skewfir1d': (8, 2), 'acoustic1d': (4, 4)}
# the first read beyond the neighbour lane, in the order of the stages' loads
FIRST_FAR = {'lowpass1d': 5, 'dfir1d': 3, 'skewfir1d': -29, 'acoustic1d': 3}
DEEPEST = {app: max(TABLE[app]) for app in APPS}
NOT_1D = 'not fused: the far-tap form handles 1-D programs'
NOT_CONCERNED = 'not concerned: every read within the neighbour lanes'
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'far1d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
ITERATIONS = {'lowpass1d': (1, 2, 3, 4), 'dfir1d': (1, 2, 4), 'skewfir1d': (1, 2),
              'acoustic1d': (1, 2, 3)}


def taps_note(text):
  return kernel_common.read_meta_from_source(text).get('far_taps')


def chains(text, side):
  """Lengths of the maximal chains of from_lane_<side>( in the text."""
  return [len(m.group(0)) // len('from_lane_%s(' % side)
          for m in re.finditer(r'(?:from_lane_%s\()+' % side, text)]


_GENERATED = {}


def generated(app):
  if app not in _GENERATED:
    _GENERATED[app] = kernel.generate(spec_of(app), far_taps=True)
  return _GENERATED[app]


def fused_text(text, name):
  """The text of one fused kernel's segment function: every level and the stores."""
  start = text.index('DEV void %s_segment' % name)
  return text[start:text.index('GLOBAL', start)]


# ---- the tables and the text ------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_without_the_switch_stage_kernels_and_todays_notes(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  lowered = specmod.inline_pointwise(spec)
  assert [k['kind'] for k in table] == ['stage'] * len(lowered['stages'])
  assert '_fused_k' not in text and taps_note(text) is None
  cols = kernel.default_cols(spec)
  first = [rel[0] for s in lowered['stages'] for _, rel in s['loads'] if abs(rel[0]) > cols][0]
  assert first == FIRST_FAR[app]
  notes = [l for l in text.splitlines() if l.startswith('// depth')]
  assert notes == ['// depth 1 not fused: x offset %d exceeds the %d columns a lane holds' % (
      first, cols)]
  assert kernel.generate(spec, far_taps=False) == (text, table)


@pytest.mark.parametrize('app', APPS)
def test_with_the_switch_the_usual_kernels_at_the_usual_depths(app):
  spec = spec_of(app)
  plain_text, plain = kernel.generate(spec)
  text, table = generated(app)
  fused = [k for k in table if k['kind'] == 'fused']
  assert table[:len(plain)] == plain and table[len(plain):] == fused
  assert [k['depth'] for k in fused] == sorted(TABLE[app])
  fields = app == 'acoustic1d'
  for k in fused:
    d = k['depth']
    assert k['name'] == '%s_fused_k%d' % (app, d)
    assert (k['halo'][0], k['halo'][1], k['w_out']) == TABLE[app][d], (app, d)
    assert k['segs'] == SEGS[app] and k['cols'] == kernel.default_cols(spec)
    assert k['tile'] == [4 * SEGS[app] * k['w_out'], 1, 1, 1]
    assert k['halo'][0] + k['halo'][1] + k['w_out'] == 64 * k['cols']
    assert k['fill_rows'] == 0 and k['origin_align'] == k['cols']
    assert k.get('fields') == (3 if fields else None)
    lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), d)[-1]
    assert 0 <= k['halo'][0] - lo[0] < k['cols'] and 0 <= k['halo'][1] - hi[0] < k['cols']
  assert taps_note(text) == app + '_fused_k1'
  assert not [l for l in text.splitlines() if l.startswith('// depth')]


def test_a_depth_whose_segment_keeps_no_cells_leaves_the_usual_note():
  """lowpass1d's window over 8 iterations is 128 cells a side: all of a 256-cell segment."""
  text, table = kernel.generate(spec_of('lowpass1d', iterate=8), far_taps=True)
  assert [k['depth'] for k in table if k['kind'] == 'fused'] == [1, 2, 4]
  assert [l for l in text.splitlines() if l.startswith('// depth')] == [
      '// depth 8 not fused: depth 8 leaves no output cells in a segment']
  assert table[:4] == generated('lowpass1d')[1]
  # the deepest kernel made is the limit, not the deepest asked for
  assert switches.depth_limit_of(spec_of('lowpass1d', iterate=8), dict(far_taps=True))[0] == 4


@pytest.mark.parametrize('app', APPS)
def test_no_hop_chain_is_longer_than_the_program_needs(app):
  text, table = generated(app)
  below, above = HOPS[app]
  for k in table:
    if k['kind'] != 'fused':
      continue
    body = fused_text(text, k['name'])
    assert max(chains(body, 'below')) == below, k['name']
    assert max(chains(body, 'above')) == above, k['name']
    if app != 'skewfir1d':      # a full window: every length up to the reach
      assert set(chains(body, 'below')) == set(range(1, below + 1))
      assert set(chains(body, 'above')) == set(range(1, above + 1))
  # a(-29) is eight lanes below for cell 0 and seven for the others, a(-13) four and three,
  # a(6) one above for cells 0 and 1 and two for 2 and 3; m(-2) and m(1) stay next door
  if app == 'skewfir1d':
    body = fused_text(text, 'skewfir1d_fused_k1')
    assert sorted(chains(body, 'below')) == [1, 1, 3, 3, 3, 4, 7, 7, 7, 8]
    assert sorted(chains(body, 'above')) == [1, 1, 1, 2, 2]
  # the chains are made of the prelude's two shifts: no helper of their own
  assert not re.search(r'from_lane_(?:below|above)\w+\(', text.replace('_or(', '('))


def test_lowpass1d_text_reads_every_tap_from_the_right_lane():
  """Every read of lowpass1d's depth-1 kernel, cell for cell: the chain and the element."""
  text, table = generated('lowpass1d')
  body = fused_text(text, 'lowpass1d_fused_k1')
  for c in range(4):
    for dx in range(-16, 17):
      j = c + dx
      inner = r'in_a\[0\]\[%d\]' % (j % 4)
      h = abs(j // 4)
      side = 'below' if j < 0 else 'above'
      pattern = (r'from_lane_%s\(' % side) * h + inner + r'\)' * h
      assert re.search(r'(?<!below\()(?<!above\()' + pattern, body), (c, dx)


def test_one_hop_prints_the_text_of_today():
  """`hops=1` is the default and changes no text; more hops than a near program needs do not
  either (the chains follow the reads)."""
  for app, form in (('smooth1d', kernel_stream1d), ('fir1d', kernel_stream1d),
                    ('wave1d', kernel_fields1d), ('fdtd1d', kernel_fields1d)):
    spec = specmod.inline_pointwise(spec_of(app))
    for depth in (1, 4):
      plain = form.emit(spec, depth)
      assert form.emit(spec, depth, hops=1) == plain
      assert form.emit(spec, depth, hops=kernel_stream1d.MAX_HOPS_1D) == plain


# ---- the register estimate ----------------------------------------------------------------------

def test_the_estimate_without_far_reads_is_unchanged():
  for app, fields in (('smooth1d', 0), ('fir1d', 0), ('wave1d', 2), ('fdtd1d', 2)):
    spec = specmod.inline_pointwise(spec_of(app))
    build = kernel_fields1d.build_levels if fields else kernel_stream1d.build_levels
    levels = build(spec, 2)
    assert kernel_stream1d.far_vgprs(levels[0] if fields else levels, 4) == 0
    for k in kernel.generate(spec_of(app), far_taps=True)[1]:
      if k['kind'] == 'fused':      # float, four segments (two fields: four as well)
        assert k['est_vgprs'] == (70 if fields else 34)


def test_the_estimate_counts_what_far_reads_keep_alive():
  """Per side and column, one link per lane beyond the first that a cell reads, and one level
  of sums: lowpass1d 2 x 4 x 3 + 4, dfir1d (2 x 2 x 3) x 2 words + 2 x 2; skewfir1d's far stage
  reads ten chain ends, a(-29), a(-13) on four cells and a(6) on two, + 4."""
  for app, far, base in (('lowpass1d', 28, 34), ('dfir1d', 28, 34), ('skewfir1d', 14, 34),
                         ('acoustic1d', 28, 76)):
    spec = specmod.inline_pointwise(spec_of(app))
    for k in generated(app)[1]:
      if k['kind'] != 'fused':
        continue
      build = kernel_fields1d.build_levels if app == 'acoustic1d' else kernel_stream1d.build_levels
      levels = build(spec, k['depth'])
      levels = levels[0] if app == 'acoustic1d' else levels
      assert kernel_stream1d.far_vgprs(levels, k['cols']) == far, (app, k['depth'])
      assert k['est_vgprs'] == base + far, (app, k['depth'])


# ---- compile and resources --------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
@pytest.mark.parametrize('app', APPS)
def test_the_shipped_unit_compiles_inside_its_estimate(app, tmp_path):
  """The unit build() ships, with -Werror=array-bounds: every fused kernel without scratch
  and without a spilled VGPR or SGPR, in no more VGPRs than its entry estimates.  Where a new
  compiler allots more, re-fit kernel_stream1d.far_vgprs to the counts this test prints."""
  spec = spec_of(app, iterate=entry.BLOB_ITERATE.get(app))
  text, table = kernel.generate(spec, far_taps=True)
  assert (text, table) == generated(app)
  fused = [k for k in table if k['kind'] == 'fused']
  assert fused
  found = resource_figures(text, [k['name'] for k in fused], str(tmp_path / (app + '.hsaco')),
                           extra_flags=['-Werror=array-bounds'])
  for k in fused:
    figures = found[k['name']]
    print(k['name'], figures, 'estimate', k['est_vgprs'])
    assert figures['private_segment_fixed_size'] == 0, (k['name'], figures)
    assert figures['vgpr_spill_count'] == 0, (k['name'], figures)
    assert figures['sgpr_spill_count'] == 0, (k['name'], figures)
    assert 0 < figures['vgpr_count'] <= k['est_vgprs'], (
        k['name'], figures, k['est_vgprs'], 're-fit kernel_stream1d.far_vgprs')


# ---- refusals -----------------------------------------------------------------------------------

def test_one_hop_refusals_are_unchanged():
  for app, form, cols in (('lowpass1d', kernel_stream1d, 4), ('dfir1d', kernel_stream1d, 2),
                          ('skewfir1d', kernel_stream1d, 4), ('acoustic1d', kernel_fields1d, 2)):
    spec = specmod.inline_pointwise(spec_of(app))
    for kw in ({}, dict(hops=1)):
      with pytest.raises(kernel_stream2d.NotFusable) as e:
        form.emit(spec, 1, **kw)
      assert str(e.value) == 'x offset %d exceeds the %d columns a lane holds' % (
          FIRST_FAR[app], cols)
  # one lane short of what the program needs: still refused, by the first read out of reach
  with pytest.raises(kernel_stream2d.NotFusable) as e:
    kernel_stream1d.emit(specmod.inline_pointwise(spec_of('skewfir1d')), 1, hops=7)
  assert str(e.value) == 'x offset -29 exceeds the 4 columns a lane holds'


def test_hops_outside_the_range_are_a_value_error():
  assert kernel_stream1d.MAX_HOPS_1D == 8
  for app, form in (('lowpass1d', kernel_stream1d), ('smooth1d', kernel_stream1d),
                    ('acoustic1d', kernel_fields1d), ('wave1d', kernel_fields1d)):
    spec = specmod.inline_pointwise(spec_of(app))
    for hops in (0, 9, -1):
      with pytest.raises(ValueError, match='hops'):
        form.emit(spec, 1, hops=hops)
    form.emit(spec, 1, hops=8)


def test_reads_beyond_max_hops_are_refused():
  wide = 'kernel: reach\nburst width: 512\nunroll factor: 1\niterate: 2\ninput float: a(*)\n' \
         'output float: b(0) = a(0) + 0.5f * (a(%d) + a(-%d))\n'
  text, table = kernel.generate(spec_of_text(wide % (33, 33)), far_taps=True)
  assert [k['kind'] for k in table] == ['stage']
  assert taps_note(text) == 'not fused: x offset 33 exceeds the 4 columns a lane holds'
  assert '// depth 1 not fused: x offset 33 exceeds the 4 columns a lane holds' in text
  assert switches.depth_limit_of(spec_of_text(wide % (33, 33)), dict(far_taps=True)) == (0, [])
  # 32 cells away is eight lanes: taken, and at depth 2 half a segment is left
  text, table = kernel.generate(spec_of_text(wide % (32, 32)), far_taps=True)
  assert taps_note(text) == 'reach_fused_k1'
  fused = [k for k in table if k['kind'] == 'fused']
  assert [(k['depth'], k['w_out']) for k in fused] == [(1, 192), (2, 128)]
  assert max(chains(text, 'below')) == 8 and max(chains(text, 'above')) == 8


def test_a_program_of_several_outputs_that_do_not_feed_back_is_refused_as_ever():
  spec = spec_of_text('kernel: onepass\nburst width: 512\nunroll factor: 1\niterate: 1\n'
                      'input float: a(*)\n'
                      'output float: b(0) = a(7) + a(-6)\n'
                      'output float: c(0) = a(3) - a(0)\n')
  plain_text, plain = kernel.generate(spec)
  text, table = kernel.generate(spec, far_taps=True)
  assert table == plain and [k['kind'] for k in table] == ['stage', 'stage']
  assert taps_note(text).startswith('not fused: stream1d handles one input feeding one output')
  assert switches.depth_limit_of(spec, dict(far_taps=True)) == (0, [])


# ---- the switch is inert elsewhere ------------------------------------------------------------

def all_samples():
  return sorted(f[:-5] for d in (SAMPLES, os.path.join(SAMPLES, 'extra'))
                for f in os.listdir(d) if f.endswith('.soda'))


def test_every_other_sample_keeps_table_and_text_and_every_note_is_right():
  apps = [a for a in all_samples() if a not in APPS]
  assert len(apps) > 40
  one_d = []
  for app in apps:
    spec = spec_of(app)
    for fuse in (False, True):
      text, table = kernel.generate(spec, fuse_outputs=fuse)
      out, got = kernel.generate(spec, fuse_outputs=fuse, far_taps=True)
      assert got == table and without_meta(out) == without_meta(text), app
      assert taps_note(text) is None
      assert taps_note(out) == (NOT_1D if spec['dim'] != 1 else NOT_CONCERNED), (app, taps_note(out))
    if spec['dim'] == 1:
      one_d.append(app)
  assert one_d == ['fdtd1d', 'fir1d', 'mixpair1d', 'skewpair1d', 'smooth1d', 'wave1d']
  for app in APPS:
    assert taps_note(generated(app)[0]) == app + '_fused_k1'


def test_the_other_switches_leave_the_new_samples_alone():
  others = dict(far_lanes=True, lds_planes=True, lds_fields=True, lds_ring=True)
  for app in APPS:
    spec = spec_of(app)
    text, table = kernel.generate(spec)
    for on in [{name: True} for name in others] + [others]:
      out, got = kernel.generate(spec, **on)
      assert got == table and without_meta(out) == without_meta(text), (app, on)
      assert taps_note(out) is None
    assert kernel_common.read_meta_from_source(kernel.generate(spec, far_lanes=True)[0])[
        'far_lanes'] == 'not fused: the far-lane form handles 2-D programs'
    both, got = kernel.generate(spec, far_taps=True, **others)
    assert got == generated(app)[1] and without_meta(both) == without_meta(generated(app)[0])


# ---- fixtures, output and build ---------------------------------------------------------------

def test_fixture_set_is_what_the_script_writes():
  fixtures = sorted(k for k in MANIFEST if k.endswith('.npz'))
  assert len(fixtures) == 48 == len(MANIFEST)
  assert fixtures == sorted(os.listdir(os.path.join(GOLDEN, 'far1d')))
  for app in APPS:
    spec = spec_of(app)
    for it in ITERATIONS[app]:
      for n in (701, 157):
        for kind in ('ramp', 'random'):
          fx = '%s.iter%d.%d.%s.npz' % (app, it, n, kind)
          assert fx in MANIFEST and MANIFEST[fx]['iterate'] == it
          assert MANIFEST[fx]['dims'] == [n]
          path = os.path.join(GOLDEN, 'far1d', fx)
          assert os.path.getsize(path) < 1 << 16
          data = np.load(path)
          for name in spec['outputs']:
            assert data['out_' + name].shape == (n,)
            assert hashlib.sha256(data['out_' + name].tobytes()).hexdigest() == \
                MANIFEST[fx]['sha256'][name], (fx, name)
      # every box keeps cells on both lengths; the long one is wider than any segment stores
      lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), it)[-1]
      assert 157 - lo[0] - hi[0] >= 29, (app, it)
    assert all(701 - k['halo'][0] - k['halo'][1] > k['w_out']
               for k in generated(app)[1] if k['kind'] == 'fused')
  lo, hi = specmod.iteration_margins(spec_of('lowpass1d'), 4)[-1]
  assert 157 - lo[0] - hi[0] == 29


def test_the_switch_table_row_and_what_follows_from_it():
  row = switches.BY_KEYWORD['far_taps']
  assert (row.flag, row.dest, row.suffix, row.depth_limit, row.note) == (
      '--hip-far-taps', 'hip_far_taps', '.taps', False, 'far_taps')
  names = [s.keyword for s in switches.SWITCHES]
  assert names.index('far_taps') == names.index('far_lanes') - 1 and len(names) == 6
  assert entry.blob_path('x', far_taps=True).endswith('x.taps.hsaco')
  assert entry.FAR_TAPS_APPS == APPS
  assert set(APPS) <= set(entry.ALL_APPS) and ('far_taps', APPS) in entry.SWITCH_BLOBS
  assert not switches.depth_limit(dict(far_taps=True))
  # no fused 1-D kernel is in the default schedule: a program the switch gave kernels, over
  # one array or several, runs under the depth of the deepest; every other as without it
  for app in APPS:
    assert switches.depth_limit_of(spec_of(app), dict(far_taps=True)) == (
        DEEPEST[app], ['--hip-far-taps']), app
    assert switches.depth_limit_of(spec_of(app), {}) == (0, [])
    assert switches.depth_limit_of(spec_of(app), dict(far_lanes=True)) == (0, [])
    assert os.path.exists(entry.sample_path(app))
    assert switches.for_program(spec_of(app), far_taps=True) == dict(far_taps=True)
  assert DEEPEST == {'lowpass1d': 4, 'dfir1d': 4, 'skewfir1d': 2, 'acoustic1d': 4}
  for app in ('jacobi2d', 'smooth1d', 'wave1d', 'acoustic2d', 'wave3d'):
    assert switches.depth_limit_of(spec_of(app), dict(far_taps=True)) == (0, [])
  # the two far switches concern disjoint programs; a row with `depth_limit` goes first
  assert switches.depth_limit_of(spec_of('acoustic2d'), dict(far_lanes=True, far_taps=True)) == (
      2, ['--hip-far-lanes'])
  assert switches.depth_limit_of(spec_of('acoustic1d'), dict(far_lanes=True, far_taps=True)) == (
      4, ['--hip-far-taps'])
  assert switches.depth_limit_of(spec_of('acoustic1d'), dict(far_taps=True, lds_ring=True)) == (
      1, ['--hip-lds-ring'])
  assert switches.keyword_text(dict(far_taps=True)) == ', far_taps=True'
  for app in ('lowpass1d', 'acoustic1d'):
    out = io.StringIO()
    host_shim.print_code(spec_of(app), out, far_taps=True)
    (line,) = [l for l in out.getvalue().splitlines() if 'program.set_max_depth(' in l]
    assert line.strip() == 'program.set_max_depth(4)    # generated with --hip-far-taps'
    assert ', far_taps=True' in out.getvalue()
  out = io.StringIO()
  host_shim.print_code(spec_of('smooth1d'), out, far_taps=True)
  assert 'program.set_max_depth(' not in out.getvalue()
  with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
    assert '`--hip-far-taps`' in f.read()
  # the forms take `hops`; nobody passes it but the switch: as a form option it is dropped
  # like every name the 1-D forms are not listed for
  assert 'hops' not in kernel.STREAM1D_OPTIONS + kernel.FIELDS1D_OPTIONS
  assert kernel.generate(spec_of('lowpass1d'), hops=4) == kernel.generate(spec_of('lowpass1d'))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'skewfir1d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-far-taps', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['skewfir1d.h', 'skewfir1d.hsaco', 'skewfir1d.py',
                                     'skewfir1d_host.cpp', 'skewfir1d_kernel.hip']
  text = (out / 'skewfir1d_kernel.hip').read_text()
  assert text == generated('skewfir1d')[0]
  assert (out / 'skewfir1d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'skewfir1d.py').read_text()
  compile(shim, 'skewfir1d.py', 'exec')
  assert 'far_taps=True' in shim
  assert 'program.set_max_depth(2)    # generated with --hip-far-taps' in shim
  host_cpp = (out / 'skewfir1d_host.cpp').read_text()
  assert '"skewfir1d_fused_k1"' in host_cpp and '"skewfir1d_fused_k2"' in host_cpp
  assert 'soda_hip_plan_set_max_depth(plan, 2)' in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'skewfir1d_host.cpp')])
  # without the flag: per-stage kernels, no limit
  plain = tmp_path / 'plain'
  subprocess.check_call([sys.executable, SODAC, sample, '--hip', str(plain)])
  assert '_fused_k' not in (plain / 'skewfir1d_kernel.hip').read_text()
  assert 'set_max_depth(' not in (plain / 'skewfir1d.py').read_text()


def test_the_measurement_tool_prints_its_usage():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'far', 'far_bench.py'),
                      '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert 'far_taps' in r.stdout and '--apps' in r.stdout and '--cols' in r.stdout
