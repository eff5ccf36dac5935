"""LDS plane-ring kernels (soda_hip/codegen/kernel_stream3d_lds.py with ring=True;
kernel.generate's `lds_ring`), without a GPU: the three samples get exactly one
`<app>_fused_k1r` / `_k1rf` whose LDS slot indices are literals below the ring's length, the
slot of every read is the one a small model of the ring holds its plane in, the kernels
compile for gfx950 without scratch or spills, the switch is inert for every other program,
the three LDS switches together give each of the nine LDS samples its own form, and sodac,
the shim and build() carry the switch."""
import io
import json
import os
import re
import subprocess
import sys

import pytest

import __graft_entry__ as entry
from soda_hip.codegen import (host_shim, kernel, kernel_common, kernel_stage,
                              kernel_stream2d, kernel_stream3d_lds, switches)
from soda_hip.codegen import spec as specmod

from conftest import ROOT, SAMPLES
from codegen_util import (HIPCC, READELF, SODAC, notes_of, resource_figures, spec_of,
                          without_meta)
from test_lds3d_codegen import lds_note
from test_lds3d_fields_codegen import fields_note

APPS = ('cross3d', 'skewcross3d', 'coupled3d')
# the ring's slots per shared input.  cross3d reads the planes -1 to 1 and skewcross3d -1 to
# 2: 4 and 5 slots at least.  Their register windows hold 10 and 7 planes; the period is a
# common multiple, and the fewest registers are kept by period 10 with 5 LDS slots and period
# 7 with 7 (ring_rotation pads LDS slots before register slots).  coupled3d: 8 register
# slots, period 8, 4 LDS slots for each of ea and eb.
RING = {'cross3d': [5], 'skewcross3d': [7], 'coupled3d': [4, 4]}
LEAST = {'cross3d': [4], 'skewcross3d': [5], 'coupled3d': [4, 4]}
PERIOD = {'cross3d': 10, 'skewcross3d': 7, 'coupled3d': 8}
ONE_PLANE = ('star3d', 'iso3dfd', 'skewstar3d', 'acoustic3d', 'skewwave3d', 'deriv3d')
NOT_CONCERNED = 'not concerned: one plane per input, lds_planes / lds_fields take it'
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'lds3d_ring_manifest.json')) as _f:
  MANIFEST = json.load(_f)


def ring_note(text):
  return kernel_common.read_meta_from_source(text).get('lds_ring')


def name_of(spec):
  return '%s_fused_k1r%s' % (spec['app_name'], 'f' if len(spec['outputs']) > 1 else '')


def fields_of(spec):
  lowered = specmod.inline_pointwise(spec)
  return kernel_stream3d_lds.analyse(lowered, len(spec['outputs']) > 1, ring=True)[1]


_GENERATED = {}


def generated(app):
  if app not in _GENERATED:
    _GENERATED[app] = kernel.generate(spec_of(app), lds_ring=True)
  return _GENERATED[app]


# ---- the tables ------------------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_without_the_switch_stage_kernels_only(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  assert [k['kind'] for k in table] == ['stage'] * len(spec['outputs'])
  assert '_fused_k' not in text and ring_note(text) is None
  assert kernel.generate(spec, lds_ring=False) == (text, table)


@pytest.mark.parametrize('app', APPS)
def test_with_the_switch_one_fused_kernel(app):
  spec = spec_of(app)
  n_out = len(spec['outputs'])
  plain_text, plain = kernel.generate(spec)
  text, table = generated(app)
  assert table[:-1] == plain and [k['kind'] for k in table] == ['stage'] * n_out + ['fused']
  k = table[-1]
  assert k['name'] == name_of(spec) and k['depth'] == 1 and k['stage'] == -1
  assert k.get('fields') == (n_out if n_out > 1 else None)
  fields = fields_of(spec)
  shared = [f for f in fields if f.lds]
  assert [f.lds_slots for f in shared] == LEAST[app]
  assert k['lds_ring'] == RING[app] and k['lds_planes'] == len(shared)
  assert k['period'] == PERIOD[app]
  for s, f in zip(k['lds_ring'], shared):
    assert s >= f.lds_slots == f.phi - f.plo + 2 and k['period'] % s == 0
  for f in fields:
    assert any(d >= f.keep and k['period'] % d == 0 for d in range(1, k['period'] + 1))
  # the entry against geometry(): tile, halo and LDS of the shape it names
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  C = 16 // elem
  lanes_x = k['tile'][0] // C
  geo = kernel_stream3d_lds.geometry(fields, elem, k['waves'], k['rows'], lanes_x,
                                     lds_slots=dict(zip([f.name for f in shared],
                                                        k['lds_ring'])))
  assert k['tile'] == [geo['TX'], geo['TY'], 64, 1] and k['block'] == [geo['threads'], 1, 1]
  assert k['halo'] == [geo['HXL'], geo['HXH'], geo['HYL'], geo['HYH']]
  assert k['lds_bytes'] == geo['lds_bytes'] == \
      sum(k['lds_ring']) * geo['PITCH'] * geo['ROWS'] * elem
  assert 0 < k['lds_bytes'] <= kernel_stream3d_lds.RING_LDS_CAP and k['est_vgprs'] <= 250
  lo, hi = spec['radius']['lo'], spec['radius']['hi']
  assert k['fill_rows'] == lo[2] + hi[2] + 1
  # every plane is loaded once with its halo: loaded_cells as in the single-plane forms
  cells = k['tile'][0] * k['tile'][1]
  assert k['loaded_cells'] == len(shared) * geo['PITCH'] * geo['ROWS'] + \
      (len(fields) - len(shared)) * cells
  assert k['step_bytes'] == (k['loaded_cells'] + n_out * cells) * elem
  # the first shape, by loaded over stored cells, that fits the budget and the cap
  lowered = specmod.inline_pointwise(spec)
  for shape in kernel_stream3d_lds.shapes_by_loaded_cells(lowered, fields=n_out > 1, ring=True):
    if shape == (k['waves'], k['rows'], lanes_x):
      break
    with pytest.raises(kernel_stream2d.NotFusable, match='would need'):
      kernel_stream3d_lds.emit(lowered, 1, *shape, fields=n_out > 1, ring=True)
  else:
    raise AssertionError('the shape of the entry is none of SHAPES')
  # the per-stage text stays, the metadata names the kernel, the other switches say nothing
  assert kernel_stage.emit(lowered)[0] in text and notes_of(text) == notes_of(plain_text)
  assert ring_note(text) == k['name'] and lds_note(text) is None and fields_note(text) is None
  assert text.count('void %s(soda_hip_args a)' % k['name']) == 1
  assert kernel_common.read_meta_from_source(text)['kernels'] == table
  # a named shape is taken as it is
  _, forced = kernel.generate(spec, lds_ring=True, lds_shape=(4, 1, 16))
  assert forced[-1]['block'] == [256, 1, 1] and forced[-1]['rows'] == 1
  assert forced[-1]['tile'][:2] == [16 * C, 16] and forced[-1]['name'] == k['name']


def test_fields_record_the_planes():
  (a,) = fields_of(spec_of('cross3d'))
  assert (a.planes, a.plo, a.phi, a.zlo, a.zhi, a.hx, a.hy) == ([-1, 0, 1], -1, 1, -4, 4,
                                                                (4, 4), (4, 4))
  (a,) = fields_of(spec_of('skewcross3d'))       # planes 0 and 1 are gaps: in the ring still
  assert (a.planes, a.plo, a.phi, a.zlo, a.zhi, a.hx, a.hy) == ([-1, 2], -1, 2, -2, 3,
                                                                (3, 2), (2, 3))
  by = {f.name: f for f in fields_of(spec_of('coupled3d'))}
  assert [(by[n].lds, by[n].planes, by[n].keep) for n in ('ea', 'eb', 'vel')] == [
      (True, [-1, 0, 1], 8), (True, [-1, 0, 1], 8), (False, [], 2)]
  # hulls over all planes: ea is read along x and y in plane 0, along y alone in planes -1, 1
  assert (by['ea'].hx, by['ea'].hy, by['eb'].hx, by['eb'].hy) == ((3, 3),) * 4
  # the single-plane form is the ring of two slots
  (u,) = [f for f in kernel_stream3d_lds.analyse(spec_of('star3d'))[1]]
  assert (u.planes, u.plo, u.phi, u.lds_slots) == ([0], 0, 0, 2)


def test_the_estimate_counts_the_vectors_of_all_planes():
  fields = fields_of(spec_of('cross3d'))
  vectors = kernel_stream3d_lds.lds_vectors(fields, 4, 2, ring=True)
  assert len(vectors) == len(set(vectors)) == 28
  assert sorted({v[1] for v in vectors}) == [-1, 0, 1]
  # none of them lies in the lane's own cells, in any plane
  assert not [v for v in vectors if v[3] == 0 and 0 <= v[2] < 2]
  geo = kernel_stream3d_lds.geometry(fields, 4, 8, 2, 16)
  flat = kernel_stream3d_lds.estimate_vgprs(fields, 4, geo, 2)
  ring = kernel_stream3d_lds.estimate_vgprs(fields, 4, geo, 2, ring=True)
  one_plane = kernel_stream3d_lds.lds_vectors(fields, 4, 2)
  assert ring - flat == 4 * (len(vectors) - len(one_plane)) + 4 * 2 * 4


def test_what_no_shape_fits_is_refused_with_the_figures():
  lowered = specmod.inline_pointwise(spec_of('coupled3d'))
  with pytest.raises(kernel_stream2d.NotFusable, match=r'bytes of LDS \(cap 163840\)'):
    kernel_stream3d_lds.emit(lowered, 1, 8, 4, 64, fields=True, ring=True)
  with pytest.raises(kernel_stream2d.NotFusable, match='would need about [0-9]+ VGPRs'):
    kernel_stream3d_lds.emit(lowered, 1, 8, 2, 16, fields=True, ring=True)
  with pytest.raises(kernel_stream2d.NotFusable, match='depth 1'):
    kernel_stream3d_lds.emit(lowered, 2, fields=True, ring=True)
  # the two single-plane forms keep their cap
  with pytest.raises(kernel_stream2d.NotFusable, match=r'84480 bytes of LDS \(cap 65536\)'):
    kernel_stream3d_lds.emit(specmod.inline_pointwise(spec_of('star3d')), 1, 8, 4, 64)


# ---- the text: slots, reads, fills ------------------------------------------------------------

READ = re.compile(r'const \w+ (l_\w+) = \*\(const \w+\*\)&lds_(\w+)\[(\d+)\]'
                  r'\[(\d+) \+ ly \+ (-?\d+)\]\[(\d+) \+ lx \* (\d+) \+ (-?\d+)\];')
FILL_OWN = re.compile(r'\*\(\w+\*\)&lds_(\w+)\[(\d+)\]\[\d+ \+ ly \+ \d+\]\[\d+ \+ lx \* \d+\] = v;')
FILL_HALO = re.compile(r'\*\(\w+\*\)\(&lds_(\w+)\[(\d+)\]\[0\]\[0\] \+ h_lds\[\d+\]\) = halo_')
ANY_SLOT = re.compile(r'lds_(\w+)\[([^\]]+)\]\[')


def steps_of(text, name):
  body = text[text.index('DEV void %s_tile(' % name):text.index('GLOBAL WG_SIZE', text.index(
      'DEV void %s_tile(' % name))]
  return body.split('// unrolled step ')[1:]


@pytest.mark.parametrize('app', APPS)
def test_every_lds_slot_index_is_a_literal_below_the_ring_length(app):
  text, table = generated(app)
  k = table[-1]
  slots = dict(zip([f.name for f in fields_of(spec_of(app)) if f.lds], k['lds_ring']))
  steps = steps_of(text, k['name'])
  assert len(steps) == k['period']
  seen = {n: set() for n in slots}
  for step in steps:
    for fname, index in ANY_SLOT.findall(step):
      assert index.isdigit() and int(index) < slots[fname], (fname, index)
      seen[fname].add(int(index))
  assert seen == {n: set(range(s)) for n, s in slots.items()}
  for fname, s in slots.items():
    assert re.search(r'lds_%s\[%d\]\[\d+\]\[\d+\];' % (fname, s), text)       # the declaration
  assert text.count('soda_block_barrier();') - plain_barriers(app) == k['period']


def plain_barriers(app):
  return kernel.generate(spec_of(app))[0].count('soda_block_barrier();')


@pytest.mark.parametrize('app', APPS)
def test_reads_and_fills_against_a_model_of_the_ring(app):
  """A model of the ring, two full periods long: at step t (output plane t, unrolled step
  t % period) the fill writes plane t + phi + 1.  Every read of the text at that step must
  find the plane it names, t + dz, in the slot it names, filled at an EARLIER step (a barrier
  lies between); the slot a step fills holds a plane below t + plo that this step does not
  read - other wavefronts may still be reading while one fills.  Rows and vectors of the reads
  are those of the loads (dx, dy, dz) of the program."""
  spec = spec_of(app)
  text, table = generated(app)
  k = table[-1]
  fields = fields_of(spec)
  by = {f.name: f for f in fields}
  C, RW = k['cols'], k['rows']
  hxl, _, hyl, _ = k['halo']
  steps = steps_of(text, k['name'])
  wanted = kernel_stream3d_lds.lds_vectors(fields, C, RW, ring=True)
  # what the program's loads need, restated: per load and cell of the lane a row and a vector
  needed = set()
  for f in fields:
    for dx, dy, dz in f.rels:
      for r in range(RW):
        for c in range(C):
          row, vi = r + dy, (c + dx) // C
          if (dx, dy) != (0, 0) and not (vi == 0 and 0 <= row < RW):
            needed.add((f.name, dz, row, vi))
  assert needed == set(wanted) and len(wanted) == len(set(wanted))
  held = {f.name: {} for f in fields if f.lds}           # slot -> (plane, step it was filled)
  for t in range(2 * k['period']):
    step = steps[t % k['period']]
    reads = READ.findall(step)
    assert len(reads) == len(wanted)                     # each vector once per lane and step
    read_slots = {n: set() for n in held}
    for (vname, fname, slot, row0, row, col0, width, col), key in zip(reads, wanted):
      f = by[fname]
      assert key[0] == fname and vname == kernel_stream3d_lds.lds_vector(fname, key[2], key[3],
                                                                         key[1])
      assert (int(row0), int(row), int(col0), int(width), int(col)) == (
          hyl, key[2], hxl, C, key[3] * C), (vname, step[:20])
      assert int(col) % C == 0                           # a whole aligned vector
      read_slots[fname].add(int(slot))
      if t >= f.phi - f.plo + 1:                         # the planes t + plo .. are all filled
        plane, filled_at = held[fname][int(slot)]
        assert plane == t + key[1] and filled_at < t, (vname, t, held[fname])
    fills = set(FILL_OWN.findall(step)) | set(FILL_HALO.findall(step))
    assert {n for n, _ in fills} == set(held) and len(fills) == len(held)
    assert set(FILL_OWN.findall(step)) == set(FILL_HALO.findall(step))
    for fname, slot in fills:
      f = by[fname]
      assert int(slot) not in read_slots[fname], (fname, slot, t)
      if int(slot) in held[fname]:
        assert held[fname][int(slot)][0] <= t + f.plo - 1
      held[fname][int(slot)] = (t + f.phi + 1, t)
    # the fill comes after the step's reads and before its one barrier
    assert step.count('soda_block_barrier();') == 1
    last_read = max(m.end() for m in READ.finditer(step))
    first_fill = min(m.start() for m in FILL_OWN.finditer(step))
    assert last_read < first_fill < step.index('soda_block_barrier();')
    assert 'a barrier lies between' in step[:first_fill]       # the comment at the fill


@pytest.mark.parametrize('app', APPS)
def test_loads_in_the_lanes_own_cells_come_from_the_window(app):
  """No LDS vector is declared for what a lane holds itself, in any plane: such loads are
  window registers (w_<input>[slot][row][column])."""
  spec = specmod.inline_pointwise(spec_of(app))
  text, table = generated(app)
  k = table[-1]
  step = steps_of(text, k['name'])[0]
  for vname, fname, slot, row0, row, col0, width, col in READ.findall(step):
    assert not (int(col) == 0 and 0 <= int(row) < k['rows']), vname
  assert re.search(r'w_\w+\[\d+\]\[\d+\]\[\d+\]', step)


# ---- the compiler ----------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', APPS)
def test_kernels_compile_for_gfx950_without_scratch_or_spills(app, tmp_path):
  """From the compiler's resource report: no private segment, no spilled VGPRs, no SGPRs
  parked in VGPR lanes, the static LDS of the entry; array subscripts in bounds at compile
  time."""
  text, table = generated(app)
  kname = table[-1]['name']
  figures = resource_figures(text, [kname], str(tmp_path / (app + '.hsaco')),
                             extra_flags=['-Werror=array-bounds'])[kname]
  assert figures['private_segment_fixed_size'] == 0, (kname, figures)
  assert figures['vgpr_spill_count'] == 0, (kname, figures)
  assert figures['sgpr_spill_count'] == 0, (kname, figures)
  assert 0 < figures['vgpr_count'] <= 256, (kname, figures)
  assert figures['group_segment_fixed_size'] == table[-1]['lds_bytes'], (kname, figures)


# ---- the switch is inert elsewhere ------------------------------------------------------------

def all_samples():
  return sorted(f[:-5] for d in (SAMPLES, os.path.join(SAMPLES, 'extra'))
                for f in os.listdir(d) if f.endswith('.soda'))


def test_every_other_sample_keeps_table_and_text():
  apps = [a for a in all_samples() if a not in APPS]
  assert len(apps) > 30 and set(ONE_PLANE) <= set(apps)
  for app in apps:
    spec = spec_of(app)
    for fuse in (False, True):
      text, table = kernel.generate(spec, fuse_outputs=fuse)
      out, got = kernel.generate(spec, fuse_outputs=fuse, lds_ring=True)
      assert got == table and without_meta(out) == without_meta(text), app
      assert '_fused_k1r' not in out and ring_note(out) is not None, app
    note = ring_note(kernel.generate(spec, lds_ring=True)[0])
    if spec['dim'] != 3:
      assert note == 'not fused: the LDS-plane form handles 3-D programs', app
    elif app in ONE_PLANE:
      assert note == NOT_CONCERNED, app
    elif any(k['kind'] == 'fused' and k['depth'] == 1 for k in kernel.generate(spec)[1]):
      assert note == 'not wanted: %s_fused_k1' % app, app
    else:
      assert note.startswith(('not concerned: ', 'not fused: ')), (app, note)


@pytest.mark.parametrize('app', APPS)
def test_the_single_plane_switches_still_refuse_the_new_samples(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  shared = [f for f in fields_of(spec) if f.lds]
  refusal = 'not fused: input %s is read off the z axis at plane offsets %s: one plane of ' \
      'an input lies in LDS' % (shared[0].name, ' and '.join(map(str, shared[0].planes)))
  for on in (dict(lds_planes=True), dict(lds_fields=True)):
    out, got = kernel.generate(spec, **on)
    assert got == table and without_meta(out) == without_meta(text)
    assert ring_note(out) is None
  if len(spec['outputs']) == 1:
    assert lds_note(kernel.generate(spec, lds_planes=True)[0]) == refusal
    assert fields_note(kernel.generate(spec, lds_fields=True)[0]) == 'not concerned: one output'
  else:
    assert fields_note(kernel.generate(spec, lds_fields=True)[0]) == refusal
    assert lds_note(kernel.generate(spec, lds_planes=True)[0]) == \
        'not fused: 3 outputs: the LDS-plane form stores one'


def test_all_three_switches_give_each_lds_sample_its_own_form():
  own = dict([(a, ('lds_planes', '_fused_k1l')) for a in ('star3d', 'iso3dfd', 'skewstar3d')] +
             [(a, ('lds_fields', '_fused_k1lf')) for a in ('acoustic3d', 'skewwave3d',
                                                           'deriv3d')] +
             [(a, ('lds_ring', name_of(spec_of(a))[len(a):])) for a in APPS])
  assert len(own) == 9
  for app, (switch, suffix) in own.items():
    spec = spec_of(app)
    on = switches.for_program(spec, lds_fields=True) if app == 'deriv3d' else {switch: True}
    alone_text, alone = kernel.generate(spec, **on)
    text, table = kernel.generate(spec, **dict(on, lds_planes=True, lds_fields=True,
                                               lds_ring=True))
    assert table == alone and without_meta(text) == without_meta(alone_text), app
    fused = [k['name'] for k in table if k['kind'] == 'fused']
    assert fused == [app + suffix], app
    meta = kernel_common.read_meta_from_source(text)
    assert meta[switch] == app + suffix
    assert [n for n in ('lds_planes', 'lds_fields', 'lds_ring') if meta[n] == app + suffix] == \
        [switch]


def test_a_one_pass_program_with_mixed_planes_needs_fuse_outputs():
  text = ('kernel: onepass\nburst width: 512\nunroll factor: 1\niterate: 1\n'
          'input float: a(32, 32, *)\n'
          'output float: b(0, 0, 0) = a(3, 0, 1) + a(-3, 0, -1)\n'
          'output float: c(0, 0, 0) = a(0, 3, 0) + a(0, 0, -1)\n')
  from test_lds3d_codegen import spec_of_text
  spec = spec_of_text(text)
  assert kernel_stream2d.rectangular(spec)
  assert switches.for_program(spec, lds_ring=True) == dict(lds_ring=True)
  plain_text, plain = kernel.generate(spec)
  out, got = kernel.generate(spec, lds_ring=True)
  assert got == plain and without_meta(out) == without_meta(plain_text)
  assert ring_note(out) == ('not fused: a one-pass program with several outputs is fused only '
                            'with fuse_outputs')
  _, table = kernel.generate(spec, lds_ring=True, fuse_outputs=True)
  assert table[-1]['name'] == 'onepass_fused_k1rf' and table[-1]['lds_ring'] == [4]


# ---- fixtures, output and build ---------------------------------------------------------------

def test_fixture_set_is_what_the_script_writes():
  fixtures = sorted(k for k in MANIFEST if k.endswith('.npz'))
  assert len(fixtures) == 24 == len(MANIFEST)
  assert fixtures == sorted(os.listdir(os.path.join(GOLDEN, 'lds3d_ring')))
  for app in APPS:
    for it in (1, 2):
      for dims in ('41x19x18', '23x27x21'):
        for kind in ('ramp', 'random'):
          fx = '%s.iter%d.%s.%s.npz' % (app, it, dims, kind)
          assert fx in MANIFEST and MANIFEST[fx]['iterate'] == it
          assert os.path.getsize(os.path.join(GOLDEN, 'lds3d_ring', fx)) < 1 << 20


def test_the_switch_table_row_and_what_follows_from_it():
  row = switches.BY_KEYWORD['lds_ring']
  assert (row.flag, row.dest, row.suffix, row.depth_limit, row.note) == (
      '--hip-lds-ring', 'hip_lds_ring', '.ldsr', True, 'lds_ring')
  assert switches.SWITCHES[-1] is row
  assert entry.blob_path('x', lds_ring=True).endswith('x.ldsr.hsaco')
  assert entry.LDS_RING_APPS == APPS
  for app in APPS:
    assert os.path.exists(entry.sample_path(app))
  out = io.StringIO()
  host_shim.print_code(spec_of('cross3d'), out, lds_ring=True)
  (line,) = [l for l in out.getvalue().splitlines() if 'program.set_max_depth(1)' in l]
  assert [w for w in line.split('#', 1)[1].split() if w.startswith('--')] == ['--hip-lds-ring']
  assert ', lds_ring=True' in out.getvalue()
  # generate() hands `lds_shape` to the form and to nobody else
  assert kernel.form_options('stream3d_lds', dict(lds_shape=(4, 1, 16), rows=8)) == dict(
      lds_shape=(4, 1, 16))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'coupled3d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-lds-ring', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['coupled3d.h', 'coupled3d.hsaco', 'coupled3d.py',
                                     'coupled3d_host.cpp', 'coupled3d_kernel.hip']
  text = (out / 'coupled3d_kernel.hip').read_text()
  assert text == generated('coupled3d')[0]
  assert (out / 'coupled3d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'coupled3d.py').read_text()
  compile(shim, 'coupled3d.py', 'exec')
  assert 'lds_ring=True' in shim and 'program.set_max_depth(1)' in shim
  host_cpp = (out / 'coupled3d_host.cpp').read_text()
  assert '"coupled3d_fused_k1rf"' in host_cpp
  assert 'soda_hip_plan_set_max_depth(plan, 1)' in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'coupled3d_host.cpp')])


def test_the_measurement_tool_prints_its_usage():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'lds3d', 'lds3d_bench.py'),
                      '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert '--ring' in r.stdout and 'lds_ring' in r.stdout
