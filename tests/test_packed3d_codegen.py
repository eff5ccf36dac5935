"""Packed-cell 3-D kernels (kernel_stream3d_pk; kernel.generate's `packed_cells`), without a
GPU: the four samples over 8- and 16-bit volumes get the usual fused kernels with their
windows declared as dwords, one wave shift per neighbour register and row, nothing changes
without the switch or for any other program, the shipped units compile for gfx950 without
scratch at two waves per SIMD and inside their register estimate, the refusals say why, sodac,
the shim and build() carry the switch, and the measuring tool pairs every schedule with the
per-stage one."""
import argparse
import hashlib
import importlib.util
import inspect
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from soda_hip.codegen import (backend, host_shim, kernel, kernel_common, kernel_stream2d,
                              kernel_stream3d_pk, switches)
from soda_hip.codegen import spec as specmod

from conftest import ROOT, SAMPLES
from codegen_util import (HIPCC, READELF, SODAC, resource_figures, spec_of, spec_of_text,
                          without_meta)

APPS = ('smooth3d', 'skewvol3d', 'sdiff3d', 'castvol3d')
DEPTHS = {'smooth3d': [1, 2], 'skewvol3d': [1], 'sdiff3d': [1], 'castvol3d': [1]}
ITERATIONS = {'smooth3d': (1, 2, 3), 'skewvol3d': (1,), 'sdiff3d': (1,), 'castvol3d': (1,)}
NOT_CONCERNED = 'not concerned: 4- or 8-byte elements'
NOT_3D = 'not fused: the packed-cell form handles 3-D programs'
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 2\niterate: 1\n'


def packed_note(text):
  return kernel_common.read_meta_from_source(text).get('packed_cells')


_GENERATED = {}


def generated(app):
  if app not in _GENERATED:
    _GENERATED[app] = kernel.generate(spec_of(app), packed_cells=True)
  return _GENERATED[app]


def waves_of(text, name):
  """Waves per SIMD the kernel is compiled for: its amdgpu_waves_per_eu attribute."""
  m = re.search(r'amdgpu_waves_per_eu\((\d), (\d)\)\)\) void %s\(' % name, text)
  assert m and m.group(1) == m.group(2)
  return int(m.group(1))


def tile_text(text, name):
  start = text.index('DEV void %s_tile' % name)
  return text[start:text.index('GLOBAL', start)]


# ---- the tables and the text ------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_with_the_switch_the_usual_kernels(app):
  spec = spec_of(app)
  plain_text, plain = kernel.generate(spec)
  text, table = generated(app)
  fused = [k for k in table if k['kind'] == 'fused']
  assert table[:len(plain)] == plain and table[len(plain):] == fused
  assert [(k['name'], k['depth']) for k in fused] == [
      ('%s_fused_k%d' % (app, d), d) for d in DEPTHS[app]]
  assert packed_note(text) == app + '_fused_k1'
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  lowered = specmod.inline_pointwise(spec)
  for k in fused:
    # the fields of kernel_stream3d's entries, with their meaning
    assert set(k) >= {'tile', 'fill_rows', 'cols', 'rows', 'period', 'w_out', 'r_out',
                      'est_vgprs', 'nt', 'step_valu', 'step_bytes'}
    assert 'origin_align' not in k and 'min_extent' not in k
    assert k['cols'] * elem in (8, 16)                       # lane loads of 8 or 16 bytes
    lo, hi = specmod.iteration_margins(lowered, k['depth'])[-1]
    halo = [-(-m // k['cols']) * k['cols'] for m in (lo[0], hi[0])]
    assert k['w_out'] == 64 * k['cols'] - sum(halo) and k['r_out'] == k['rows'] - lo[1] - hi[1]
    assert k['tile'] == [4 * k['w_out'] - k['cols'], k['r_out'], 64, 1]
    assert k['block'] == [256, 1, 1] and k['nt'] == 4
    # the occupancy the shape was taken at, said to the compiler, and its register budget
    assert k['est_vgprs'] <= dict(kernel_stream3d_pk.OCCUPANCY_LEVELS)[waves_of(text, k['name'])]
    body = tile_text(text, k['name'])
    assert '__shared__' not in body and 'barrier' not in body


@pytest.mark.parametrize('app', APPS)
def test_without_the_switch_nothing_changes(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  assert kernel.generate(spec, packed_cells=False) == (text, table)
  lowered = specmod.inline_pointwise(spec)
  assert [k['kind'] for k in table] == ['stage'] * len(lowered['stages'])
  assert '_fused_k' not in text and packed_note(text) is None
  assert 'depth 1 not fused:' in text       # today's refusal of the 4- and 8-byte forms


def all_samples():
  return sorted(f[:-5] for d in (SAMPLES, os.path.join(SAMPLES, 'extra'))
                for f in os.listdir(d) if f.endswith('.soda'))


def test_every_other_sample_keeps_table_and_text_and_every_note_is_right():
  apps = [a for a in all_samples() if a not in APPS]
  assert len(apps) > 40
  seen = set()
  for app in apps:
    spec = spec_of(app)
    types = specmod.tensor_c_types(spec)
    ends = [t['c_type'] for t in spec['inputs']] + [types[o] for o in spec['outputs']]
    wide = all(specmod.ELEM_SIZE[t] >= 4 for t in ends)
    assert wide or spec['dim'] != 3, app      # no narrow 3-D sample before these four
    for fuse in (False, True):
      text, table = kernel.generate(spec, fuse_outputs=fuse)
      out, got = kernel.generate(spec, fuse_outputs=fuse, packed_cells=True)
      assert got == table and without_meta(out) == without_meta(text), app
      assert packed_note(text) is None
      assert packed_note(out) == (NOT_CONCERNED if wide else NOT_3D), (app, packed_note(out))
      seen.add(packed_note(out))
  assert seen == {NOT_CONCERNED, NOT_3D}      # blur and casts are narrow and 2-D


def test_the_other_switches_leave_the_new_samples_alone():
  others = {s.keyword: True for s in switches.ALL if s.keyword != 'packed_cells'}
  for app in APPS:
    spec = spec_of(app)
    text, table = kernel.generate(spec)
    for keyword in others:
      out, got = kernel.generate(spec, **{keyword: True})
      assert [k for k in got if k['kind'] == 'fused'] == [], (app, keyword)
      assert got == table, (app, keyword)


# ---- refusals -----------------------------------------------------------------------------------

def test_half_and_far_reads_are_refused_with_a_reason():
  half = spec_of_text(HEAD % 'h3' + 'input half: a(32, 32, *)\n'
                      'output half: b(0, 0, 0) = a(0, 0, 0) + a(1, 0, 0) + a(0, 0, 1)\n')
  text, table = kernel.generate(half, packed_cells=True)
  plain_text, plain = kernel.generate(half)
  assert table == plain and without_meta(text) == without_meta(plain_text)
  assert packed_note(text) == 'not fused: half is outside the packed-cell form'
  far = spec_of_text(HEAD % 'far3' + 'input uint16: a(32, 32, *)\n'
                     'output uint16: b(0, 0, 0) = a(0, 0, 0) + a(9, 0, 0) + a(0, 0, 1)\n')
  text, table = kernel.generate(far, packed_cells=True)
  plain_text, plain = kernel.generate(far)
  assert table == plain and without_meta(text) == without_meta(plain_text)
  assert re.fullmatch(r'not fused: x offset 9 exceeds the [48] columns a lane holds',
                      packed_note(text))
  # eight columns away is the neighbour lane of an 8-column lane: taken
  near = spec_of_text(HEAD % 'near3' + 'input uint16: a(32, 32, *)\n'
                      'output uint16: b(0, 0, 0) = a(0, 0, 0) + a(8, 0, 0) + a(0, 0, 1)\n')
  text, table = kernel.generate(near, packed_cells=True)
  assert packed_note(text) == 'near3_fused_k1' and table[-1]['cols'] == 8
  for body, why in (
      ('input uint8: a(32, 32, *)\noutput uint16: b(0, 0, 0) = a(0, 0, 0) + a(1, 0, 0)\n',
       'inputs and output of different widths'),
      ('input uint16: a(32, 32, *)\nlocal double: t(0, 0, 0) = a(0, 0, 0) * 0.5\n'
       'output uint16: b(0, 0, 0) = uint16(t(0, 0, 0) + t(1, 0, 0))\n',
       'local t has 8-byte elements'),
      ('input uint16: a(32, 32, *)\noutput uint16: b(0, 0, 0) = a(0, 0, 0) + a(1, 0, 0)\n'
       'output uint16: c(0, 0, 0) = a(0, 0, 0) - a(0, 1, 0)\n',
       'the packed-cell form handles single-output programs')):
    text, table = kernel.generate(spec_of_text(HEAD % 'odd3' + body), packed_cells=True)
    assert all(k['kind'] == 'stage' for k in table)
    assert packed_note(text) == 'not fused: ' + why
  # depths beyond 2 are nobody's
  with pytest.raises(kernel_stream2d.NotFusable, match='2 iterations deep'):
    kernel_stream3d_pk.emit(specmod.inline_pointwise(spec_of('smooth3d', iterate=4)), 4)
  _, table = kernel.generate(spec_of('smooth3d', iterate=8), packed_cells=True)
  assert [k['depth'] for k in table if k['kind'] == 'fused'] == [1, 2]
  _, table = kernel.generate(spec_of('smooth3d', iterate=1), packed_cells=True)
  assert [k['depth'] for k in table if k['kind'] == 'fused'] == [1]


def test_tile_shapes_and_overrides():
  """Most waves per SIMD first, then most of the tile kept: the first shape that fits the
  level's budget."""
  assert kernel_stream3d_pk.OCCUPANCY_LEVELS == ((4, 128), (3, 168), (2, 240))
  assert all(budget <= 512 // waves for waves, budget in kernel_stream3d_pk.OCCUPANCY_LEVELS)
  spec = spec_of('smooth3d')
  lowered = specmod.inline_pointwise(spec)
  shapes = kernel_stream3d_pk.shapes_by_kept_fraction(lowered, 1)
  assert sorted(shapes) == sorted(kernel_stream3d_pk.TILE_SHAPES[2])
  assert {c for _, c in shapes} == {4, 8}
  kept = [kernel_stream3d_pk.tile_geometry(lowered, 1, r, c)['kept'] for r, c in shapes]
  assert kept == sorted(kept, reverse=True) and shapes[0] == (8, 8)
  assert {c for _, c in kernel_stream3d_pk.TILE_SHAPES[1]} == {8, 16}
  # 8 x 8 keeps more of the tile but needs 132 registers: four waves per SIMD take 8 x 4
  text, table = generated('smooth3d')
  with pytest.raises(kernel_stream2d.NotFusable, match='about 132 VGPRs in 8 x 8 tiles'):
    kernel_stream3d_pk.emit(lowered, 1, rows=8, cols=8)
  assert [(k['rows'], k['cols'], waves_of(text, k['name'])) for k in table[-2:]] == [
      (8, 4, 4), (8, 4, 4)]
  # the float local costs castvol3d a level
  text, table = generated('castvol3d')
  assert (table[-1]['rows'], table[-1]['cols'], waves_of(text, table[-1]['name'])) == (8, 4, 3)
  # a shape asked for is taken at the first level it fits, an occupancy asked for is the level
  text, forced = kernel.generate(spec, packed_cells=True, cols=4, rows=16)
  assert [(k['rows'], k['cols'], waves_of(text, k['name'])) for k in forced[-2:]] == [
      (16, 4, 3), (16, 4, 2)]
  text, forced = kernel.generate(spec, packed_cells=True, waves_per_eu=2)
  assert [(k['rows'], k['cols'], waves_of(text, k['name'])) for k in forced[-2:]] == [
      (8, 8, 2), (8, 8, 2)]
  with pytest.raises(kernel_stream2d.NotFusable, match='lane loads are 8 or 16 bytes'):
    kernel_stream3d_pk.emit(lowered, 1, cols=2)


# ---- the text: dwords, crossings, extraction ----------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_windows_are_dwords_and_a_four_byte_local_is_a_register_per_cell(app):
  spec = specmod.inline_pointwise(spec_of(app))
  types = specmod.tensor_c_types(spec)
  text, table = generated(app)
  for k in (e for e in table if e['kind'] == 'fused'):
    body = tile_text(text, k['name'])
    declared = re.findall(r'^  (unsigned|float|int) (\w+)\[(\d+)\]\[(\d+)\]\[(\d+)\];$', body, re.M)
    assert declared
    total = 0
    for ctype, ident, keep, rows, regs in declared:
      tensor = ident.split('_', 1)[1]
      elem = specmod.ELEM_SIZE[types[tensor]]
      assert int(rows) == k['rows']
      if elem < 4:
        assert ctype == 'unsigned' and int(regs) == k['cols'] * elem // 4, ident
      else:
        assert ctype == kernel_common.builtin_type(types[tensor]) and int(regs) == k['cols']
      total += int(keep) * int(rows) * int(regs)
    # est_vgprs counts dwords
    dwords = k['cols'] * specmod.ELEM_SIZE[spec['inputs'][0]['c_type']] // 4
    assert k['est_vgprs'] == total + kernel_stream3d_pk.overhead_vgprs(k['rows'], k['cols'], dwords)
    # nothing is unpacked at load time: an interior row is one vector load into its dwords
    assert re.search(r'const vec_%s v = \*\(const vec_%s\*\)' % (k['name'], k['name']), body)
  if app == 'castvol3d':
    assert re.search(r'^  float k0_f\[\d+\]\[8\]\[4\];$', tile_text(text, 'castvol3d_fused_k1'),
                     re.M)
  if app == 'smooth3d':       # the issue's arithmetic: a uint16 row of 4 cells is 2 registers
    assert '  unsigned in_v[3][8][2];' in tile_text(text, 'smooth3d_fused_k1')


def rows_of(body, ident):
  """{(unrolled step, row): text} of the rows of one instance."""
  out = {}
  step = -1
  for block in re.split(r'(?=    \{  // unrolled step )', body):
    m = re.match(r'    \{  // unrolled step (\d+)', block)
    if not m:
      continue
    step = int(m.group(1))
    for piece in re.split(r'(?=      \{  // row \d+ of )', block):
      r = re.match(r'      \{  // row (\d+) of (\w+)\n', piece)
      if r and r.group(2) == ident:
        out[step, int(r.group(1))] = piece
  return out


def test_one_wave_shift_per_neighbour_register_and_row():
  """skewvol3d, four cells per dword, 8 per lane: w reads t two columns to the left (cells 6
  and 7 of the lane below: its second dword) and one to the right (cell 0 of the lane above);
  t reads v two to the right (cells 0 and 1 of the lane above: one dword)."""
  text, table = generated('skewvol3d')
  assert table[-1]['cols'] == 8
  body = tile_text(text, 'skewvol3d_fused_k1')
  readers = rows_of(body, 'k0_w')
  assert len(readers) == table[-1]['period'] * table[-1]['r_out']
  for (step, r), piece in readers.items():
    assert len(re.findall(r'from_lane_', piece)) == 2, (step, r)
    (below,) = re.findall(r'const auto (\w+) = from_lane_below\(k0_t\[\d\]\[%d\]\[1\]\);' % r, piece)
    (above,) = re.findall(r'const auto (\w+) = from_lane_above\(k0_t\[\d\]\[%d\]\[0\]\);' % (r + 1),
                          piece)
    # the lane below's cells 6 and 7 feed cells 0 and 1, the lane above's cell 0 feeds cell 7
    assert '((unsigned char)(%s >> 16))' % below in re.search(r'cell\[0\] = .*', piece).group(0)
    assert '((unsigned char)(%s >> 24))' % below in re.search(r'cell\[1\] = .*', piece).group(0)
    assert '((unsigned char)(%s))' % above in re.search(r'cell\[7\] = .*', piece).group(0)
    assert piece.count(below) == 3 and piece.count(above) == 2
  for (step, r), piece in rows_of(body, 'k0_t').items():
    assert len(re.findall(r'from_lane_', piece)) == 1
    assert re.search(r'from_lane_above\(in_v\[\d\]\[%d\]\[0\]\)' % r, piece)
  # no operand crosses lanes cell by cell
  assert not re.search(r'cell\[\d+\] = .*from_lane_', body)


def test_cells_are_typed_as_the_reference_types_them():
  text, _ = generated('sdiff3d')
  body = tile_text(text, 'sdiff3d_fused_k1')
  assert '((short)(in_a[' in body and ' >> 16))' in body       # sign-extending extraction
  assert '(unsigned short)' not in body.split('unrolled step 0')[1].split('cell[0] =')[1].split('\n')[0]
  assert '(unsigned)(unsigned short)cell[0] | ((unsigned)(unsigned short)cell[1] << 16)' in body
  text, _ = generated('smooth3d')
  body = tile_text(text, 'smooth3d_fused_k2')
  assert '((unsigned short)(k0_s[' in body and '((unsigned short)(in_v[' in body
  # the expression text is cell_assignment's: the reference's operators on extracted cells
  assert re.search(r'cell\[0\] = \(\(+unsigned short\)\(in_v\[\d\]\[\d+\]\[0\]\)\) \* 3\)', body)
  assert ') / 9);' in body and 'v_pk' not in body and '__builtin_amdgcn_perm' not in body
  text, _ = generated('castvol3d')
  body = tile_text(text, 'castvol3d_fused_k1')
  assert re.search(r'k0_f\[\d\]\[\d+\]\[0\] = \(static_cast<float >\(\(\(unsigned short\)\(in_img', body)
  # the float local is read as it is, a register per cell, across lanes as well
  assert re.search(r'const auto (\w+) = from_lane_below\(k0_f\[\d\]\[\d+\]\[3\]\);', body)
  assert re.search(r'cell\[0\] = \(static_cast<unsigned short >\(0.25f \* \(k0_f\[', body)


def extract(dword, elem, sub, signed):
  """The model of `(T)(dword >> shift)`: the cell, as C converts it to int."""
  bits = 8 * elem
  cell = (dword >> (bits * sub)) & ((1 << bits) - 1)
  return cell - (1 << bits) if signed and cell >> (bits - 1) else cell


def pack(cells, elem):
  """The model of `(unsigned)(U)cell | (unsigned)(U)cell << ...`: truncation to U first."""
  bits = 8 * elem
  return sum((c & ((1 << bits) - 1)) << (bits * i) for i, c in enumerate(cells))


def test_extract_sign_extend_and_repack_round_trip():
  """Every int16 and every int8 value in every position of a dword, beside all-ones and
  all-zeros neighbours: extraction sign-extends, packing truncates, the dword comes back."""
  for elem, lo, hi in ((2, -32768, 32768), (1, -128, 128)):
    per = 4 // elem
    mask = (1 << 8 * elem) - 1
    for value in range(lo, hi):
      for sub in range(per):
        for fill in (0, -1):
          cells = [fill] * per
          cells[sub] = value
          dword = pack(cells, elem)
          assert 0 <= dword < 1 << 32
          assert [extract(dword, elem, i, True) for i in range(per)] == cells
          assert [extract(dword, elem, i, False) for i in range(per)] == [c & mask for c in cells]
          assert pack([extract(dword, elem, i, True) for i in range(per)], elem) == dword
          # a result outside the type is truncated on packing, as a narrow store truncates
          wrapped = list(cells)
          wrapped[sub] = value + (1 << 8 * elem) * 3
          assert pack(wrapped, elem) == dword
  # the model is the generator's text
  assert kernel_stream3d_pk.extract('w', 'int16_t', 1) == '((short)(w >> 16))'
  assert kernel_stream3d_pk.extract('w', 'uint8_t', 0) == '((unsigned char)(w))'
  assert kernel_stream3d_pk.extract('w', 'int8_t', 3) == '((signed char)(w >> 24))'
  assert kernel_stream3d_pk.pack(lambda c: 'c%d' % c, 'int16_t', 2) == \
      '(unsigned)(unsigned short)c2 | ((unsigned)(unsigned short)c3 << 16)'
  assert kernel_stream3d_pk.pack(lambda c: 'c%d' % c, 'uint8_t', 4).count('(unsigned char)') == 4


# ---- compile and resources --------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', APPS)
def test_the_shipped_unit_compiles_at_two_waves_per_simd(app, tmp_path):
  """The unit build() ships, with -Werror=array-bounds, from the compiler's resource report:
  no scratch, no spilled VGPR, at most 256 VGPRs - two waves per SIMD of gfx950's 512 -, no
  more than the occupancy the kernel was selected for allows, and within 1.25 x the entry's
  estimate."""
  spec = spec_of(app, iterate=entry.BLOB_ITERATE.get(app))
  text, table = kernel.generate(spec, packed_cells=True)
  assert (text, table) == generated(app)
  fused = [k for k in table if k['kind'] == 'fused']
  found = resource_figures(text, [k['name'] for k in fused], str(tmp_path / (app + '.hsaco')),
                           extra_flags=['-Werror=array-bounds'])
  for k in fused:
    figures = found[k['name']]
    print(k['name'], figures, 'estimate', k['est_vgprs'])
    assert figures['private_segment_fixed_size'] == 0, (k['name'], figures)
    assert figures['vgpr_spill_count'] == 0, (k['name'], figures)
    assert 0 < figures['vgpr_count'] <= 256, (k['name'], figures)
    assert 512 // figures['vgpr_count'] >= waves_of(text, k['name']) >= 2
    assert figures['vgpr_count'] <= 1.25 * k['est_vgprs'], (k['name'], figures, k['est_vgprs'])
    assert figures['group_segment_fixed_size'] == 0       # no LDS


# ---- fixtures, the switch's row, output and build ----------------------------------------------

def test_fixture_set_is_what_the_script_writes():
  with open(os.path.join(GOLDEN, 'packed3d_manifest.json')) as f:
    manifest = json.load(f)
  fixtures = sorted(k for k in manifest if k.endswith('.npz'))
  assert len(fixtures) == 24 == len(manifest)
  assert fixtures == sorted(os.listdir(os.path.join(GOLDEN, 'packed3d')))
  for app in APPS:
    spec = spec_of(app)
    for it in ITERATIONS[app]:
      for dims in ((600, 11, 7), (37, 13, 9)):
        for kind in ('ramp', 'random'):
          fx = '%s.iter%d.%s.%s.npz' % (app, it, 'x'.join(map(str, dims)), kind)
          assert manifest[fx]['iterate'] == it and manifest[fx]['dims'] == list(dims)
          path = os.path.join(GOLDEN, 'packed3d', fx)
          assert os.path.getsize(path) < 200 << 10
          data = np.load(path)
          for t in spec['inputs']:
            assert data['in_' + t['name']].dtype == np.dtype(specmod.NUMPY_NAME[t['c_type']])
            assert data['in_' + t['name']].shape == tuple(reversed(dims))
          for name in spec['outputs']:
            assert hashlib.sha256(data['out_' + name].tobytes()).hexdigest() == \
                manifest[fx]['sha256'][name], (fx, name)
        # every output box keeps a cell, and the wide grid a tile seam inside it
        lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), it)[-1]
        assert all(n - a - b >= 1 for n, a, b in zip(dims, lo, hi)), (app, it, dims)
    for k in (e for e in generated(app)[1] if e['kind'] == 'fused'):
      assert k['w_out'] + 16 < 600


def test_the_switch_table_row_and_what_follows_from_it():
  row = switches.BY_KEYWORD['packed_cells']
  assert (row.flag, row.dest, row.suffix, row.depth_limit, row.note) == (
      '--hip-packed-cells', 'hip_packed_cells', '.pk', False, 'packed_cells')
  # the forms by element width have a table of their own; every reader takes both
  assert switches.ELEMENT_SWITCHES == (row,) and row not in switches.SWITCHES
  assert switches.ALL == switches.SWITCHES + switches.ELEMENT_SWITCHES
  parser = argparse.ArgumentParser()
  backend.add_arguments(parser)
  assert switches.from_args(parser.parse_args(['--hip-packed-cells']), switches.ALL) == {
      s.keyword: s is row for s in switches.ALL}
  assert 'packed_cells' not in switches.from_args(parser.parse_args(['--hip-packed-cells']))
  assert inspect.signature(kernel.generate).parameters['packed_cells'].default is False
  assert switches.blob_suffix(dict(packed_cells=True)) == '.pk'
  assert entry.blob_path('x', packed_cells=True).endswith('x.pk.hsaco')
  assert entry.PACKED_CELLS_APPS == APPS and set(APPS) <= set(entry.ALL_APPS)
  assert ('packed_cells', APPS) in entry.SWITCH_BLOBS
  names = [f.func.__name__ if hasattr(f, 'func') else f.__name__ for f in kernel.FAMILIES]
  assert names.index('packed3d_kernels') == names.index('deep3d_kernels') + 1
  for app in APPS + ('jacobi3d', 'blur', 'wave3d'):
    assert switches.depth_limit_of(spec_of(app), dict(packed_cells=True)) == (0, [])
  assert switches.keyword_text(dict(packed_cells=True)) == ', packed_cells=True'
  for app in APPS:
    assert os.path.exists(entry.sample_path(app))
    assert switches.for_program(spec_of(app), packed_cells=True) == dict(packed_cells=True)
    out = io.StringIO()
    host_shim.print_code(spec_of(app), out, packed_cells=True)
    assert ', packed_cells=True' in out.getvalue()
    assert 'program.set_max_depth(' not in out.getvalue()
  with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
    assert '`--hip-packed-cells`' in f.read()
  with pytest.raises(TypeError):
    kernel.generate(spec_of('smooth3d'), packed=True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'castvol3d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-packed-cells', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['castvol3d.h', 'castvol3d.hsaco', 'castvol3d.py',
                                     'castvol3d_host.cpp', 'castvol3d_kernel.hip']
  text = (out / 'castvol3d_kernel.hip').read_text()
  assert text == generated('castvol3d')[0]
  assert (out / 'castvol3d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'castvol3d.py').read_text()
  compile(shim, 'castvol3d.py', 'exec')
  assert 'packed_cells=True' in shim and 'program.set_max_depth(' not in shim
  host_cpp = (out / 'castvol3d_host.cpp').read_text()
  assert '"castvol3d_fused_k1"' in host_cpp and 'soda_hip_plan_set_max_depth' not in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'castvol3d_host.cpp')])


# ---- the measuring tool -----------------------------------------------------------------------

def bench_module():
  spec = importlib.util.spec_from_file_location(
      'packed3d_bench', os.path.join(ROOT, 'tools', 'packed3d', 'packed3d_bench.py'))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  return module


def test_the_measuring_tool_pairs_every_schedule_with_the_per_stage_one():
  bench = bench_module()
  args = bench.parse_args([])
  assert (args.sizes, args.iterate, args.sweeps, args.warmup, args.repeats, args.apps) == (
      [512, 256], 4, 7, 2, 3, None)
  assert bench.parse_args(['--sizes', '128', '--apps', 'sdiff3d']).sizes == [128]
  with pytest.raises(SystemExit):
    bench.parse_args(['--sweeps', '2'])
  _, table = generated('smooth3d')
  rows = bench.schedules_of(table, 4)
  assert [r[0] for r in rows] == ['default', 'depth 1', 'depth 2', 'per-stage']
  assert [r[1] for r in rows] == [0, 0, 0, -1]          # the same blob under set_max_depth(-1)
  assert [r[2] for r in rows] == [None, [1, 1, 1, 1], [2, 2], None]
  assert [r[3] and r[3]['name'] for r in rows] == [None, 'smooth3d_fused_k1',
                                                   'smooth3d_fused_k2', None]
  with pytest.raises(ValueError, match='no multiple of depth 2'):
    bench.schedules_of(table, 3)
  with pytest.raises(ValueError, match='no fused kernel'):
    bench.schedules_of(kernel.generate(spec_of('smooth3d'))[1], 4)
  # the report: judge()'s rule, one line per schedule, the per-stage line without a verdict
  times = {'default': [6.0, 7.0, 8.0], 'depth 1': [11.0, 12.5, 12.0], 'per-stage': [13.0, 11.0, 12.0]}
  launches = {'default': ['k2', 'k2'], 'depth 1': ['k1'] * 4, 'per-stage': ['s'] * 4}
  judged = bench.judge(times)
  assert judged['default']['verdict'] == 'FASTER'
  assert judged['depth 1']['verdict'] == 'NO DIFFERENCE beyond the spread'
  lines = bench.report_lines('smooth3d', (64, 64, 64), 4, judged, launches, 1000000, 4)
  assert lines[0].startswith('smooth3d 64 x 64 x 64 x 4;')
  assert len(lines) == 2 + len(times)
  assert 'FASTER (spread 2.000 ms)' in lines[2] and lines[2].split()[0] == 'default'
  assert 'NO DIFFERENCE' in lines[3]
  assert lines[4].split()[0] == 'per-stage' and 'spread' not in lines[4]
  assert '%13.1f' % (7.0 * 1e3 / 2) in lines[2]          # us per launch from the median


def test_the_measurement_tool_prints_its_usage():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'packed3d', 'packed3d_bench.py'),
                      '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert 'packed_cells' in r.stdout and '--sizes' in r.stdout
