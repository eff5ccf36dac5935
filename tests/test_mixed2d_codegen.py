"""Mixed-width fused 2-D kernels (kernel_stream2d with `mixed`; kernel.generate's
`mixed_widths`), without a GPU: the four samples get `<app>_fused_k1` with every input loaded
through a vector of its own type and the store in the output's width, nothing changes without
the switch or for any other program, what is outside the class is refused with a reason, the
lane shapes are the list kernel.mixed_shapes says and `cols=` overrides it, step_bytes is
summed per tensor, the shipped units compile for gfx950 without scratch or spilled registers
and inside their register estimate, and sodac, the shim and build() carry the switch.

mask2d - two inputs of ONE width and different types, fused in the default path - is held to
the same rule about its loads: before per-input vector types its int32 rows were read through
the float vector in every interior strip."""
import argparse
import hashlib
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from soda_hip.codegen import backend, kernel, kernel_common, kernel_stream2d, switches
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import selfcheck

from conftest import ROOT, SAMPLES
from codegen_util import HIPCC, SODAC, resource_figures, spec_of, spec_of_text, without_meta

APPS = ('edge8f', 'tone16', 'quant2d', 'dsum2d')
TODAY = '// depth 1 not fused: inputs and output of different widths'
NOT_CONCERNED = 'not concerned: inputs and output of one width'
NOT_2D = 'not fused: the mixed-width form handles 2-D programs'
# per sample: (element sizes of inputs and output, the lane shapes the register estimate
# takes, the shipped one: columns per lane).  The list runs from 16 / widest to 16 / narrowest;
# tone16 and quant2d at 16 columns are over the budget of 244 VGPRs.
TABLE = {
    'edge8f': ([1, 4], [4, 8, 16], 4),
    'tone16': ([2, 1], [8], 8),
    'quant2d': ([4, 1, 2], [4, 8], 4),
    'dsum2d': ([4, 8], [2, 4], 2),
}
BUILTIN = {'uint8_t': 'unsigned char', 'uint16_t': 'unsigned short', 'int32_t': 'int',
           'float': 'float', 'double': 'double'}
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'mixed2d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
GRIDS = ('301x53', '71x57', '1100x11')


def note(text):
  return kernel_common.read_meta_from_source(text).get('mixed_widths')


_GENERATED = {}


def generated(app):
  if app not in _GENERATED:
    _GENERATED[app] = kernel.generate(spec_of(app), mixed_widths=True)
  return _GENERATED[app]


def fused_entry(table):
  (k,) = [e for e in table if e['kind'] == 'fused']
  return k


# ---- the tables and the text ------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_without_the_switch_stage_kernels_and_todays_note(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  assert [k['kind'] for k in table] == ['stage'] * len(specmod.inline_pointwise(spec)['stages'])
  assert '_fused_k' not in text and note(text) is None
  assert [l for l in text.splitlines() if l.startswith('// depth')] == [TODAY]
  assert kernel.generate(spec, mixed_widths=False) == (text, table)
  assert kernel.mixed_end_sizes(spec) == TABLE[app][0]


@pytest.mark.parametrize('app', APPS)
def test_with_the_switch_one_fused_kernel_and_the_note(app):
  spec = spec_of(app)
  _, plain = kernel.generate(spec)
  text, table = generated(app)
  k = fused_entry(table)
  assert table == plain + [k]
  assert (k['name'], k['depth'], k['cols']) == (app + '_fused_k1', 1, TABLE[app][2])
  assert k['fill_rows'] >= 2 and k['period'] <= 12 and k['est_vgprs'] <= 244
  assert k['halo'][0] + k['halo'][1] + k['w_out'] == 64 * k['cols']
  assert note(text) == app + '_fused_k1'
  assert TODAY not in text
  # every read lies within the neighbour lane at the shipped shape
  lowered = specmod.inline_pointwise(spec)
  assert max(abs(rel[0]) for s in lowered['stages'] for _, rel in s['loads']) <= k['cols']


@pytest.mark.parametrize('app', APPS + ('mask2d',))
def test_every_input_is_loaded_through_a_vector_of_its_own_type(app):
  """Per input: a typedef of the input's own element type, `cols` elements, aligned to the
  element; the interior load of its rows goes through that typedef and no other."""
  spec = spec_of(app)
  text, table = kernel.generate(spec, mixed_widths=app != 'mask2d')
  k = fused_entry(table)
  if app == 'mask2d':      # the default path: no switch, and the switch does not concern it
    assert kernel.generate(spec, mixed_widths=True)[1] == table
  typedefs = {m.group(2): (m.group(1), int(m.group(3)), int(m.group(4))) for m in re.finditer(
      r'typedef ([\w ]+?) (vec_\w+) __attribute__\(\(ext_vector_type\((\d+)\), aligned\((\d+)\)\)\);',
      text)}
  for t in spec['inputs']:
    loads = re.findall(
        r'// load row head\+\d+ of %s\n(?:.*\n){2}        if \(INTERIOR\) \{\n'
        r'          const (\w+) v = \*\(const (\w+)\*\)p;' % t['name'], text)
    assert loads and len(set(loads)) == 1, (app, t['name'])
    vec, cast = loads[0]
    assert vec == cast
    assert typedefs[vec] == (BUILTIN[t['c_type']], k['cols'], specmod.ELEM_SIZE[t['c_type']]), (
        app, t['name'], typedefs[vec])
  out_type = specmod.tensor_c_types(spec)[spec['outputs'][0]]
  assert typedefs['vec_%s_out' % k['name']] == (
      BUILTIN[out_type], k['cols'], specmod.ELEM_SIZE[out_type])


@pytest.mark.parametrize('app', APPS)
def test_stores_use_the_outputs_size(app):
  text, table = generated(app)
  k = fused_entry(table)
  spec = spec_of(app)
  size = specmod.ELEM_SIZE[specmod.tensor_c_types(spec)[spec['outputs'][0]]]
  row = k['cols'] * size
  assert 'st_voff = st_full ? (unsigned)(x * %d) :' % size in text
  assert '(int)(W * %d), 0x27000)' % size in text
  assert 'a.dims[0] * %d >= 0x7ffffff0ll' % size in text
  stores = re.findall(r'raw_buffer_store_(b\d+)\(', text)
  assert set(stores) == {'b%d' % (8 * min(row, 16))}


def test_a_row_of_more_than_16_bytes_leaves_in_pieces():
  spec = spec_of('edge8f')
  text, table = kernel.generate(spec, mixed_widths=True, cols=16)
  k = fused_entry(table)
  assert k['cols'] == 16
  calm = text[text.index('if (!RAGGED) {'):]
  calm = calm[:calm.index('} else if')]
  assert re.findall(r'st_voff \+ (\d+),', calm) == ['0', '16', '32', '48']
  assert calm.count('make_buffer_rsrc') == 1
  # the lanes that store nothing: a lane offset no piece's offset wraps round
  assert 'st_voff = st_full ? (unsigned)(x * 4) : 0x80000000u;' in text
  assert 'typedef float vec_edge8f_fused_k1_piece __attribute__((ext_vector_type(4)));' in text


# ---- lane shapes ------------------------------------------------------------------------------

@pytest.mark.parametrize('app', APPS)
def test_the_shape_list_and_the_cols_override(app):
  spec = spec_of(app)
  sizes, taken, shipped = TABLE[app]
  shapes = kernel.mixed_shapes(spec)
  assert sorted(shapes) == [c for c in (1, 2, 4, 8, 16)
                            if 16 // max(sizes) <= c <= 16 // min(sizes)]
  assert shapes == (sorted(shapes) if kernel.MIXED_WIDEST_FIRST else sorted(shapes)[::-1])
  assert kernel.mixed_shapes(spec, 8) == [8]
  made = []
  for cols in sorted(shapes):
    text, table = kernel.generate(spec, mixed_widths=True, cols=cols)
    fused = [k for k in table if k['kind'] == 'fused']
    if fused:
      assert fused[0]['cols'] == cols and note(text) == app + '_fused_k1'
      made.append(cols)
    else:     # over the register budget: skipped, not emitted
      assert re.match(r'not fused: depth 1 would need about \d+ VGPRs \(budget 244\)',
                      note(text)), note(text)
  assert made == taken
  # the shipped shape is the first of the list the estimate takes
  assert shipped == [c for c in shapes if c in taken][0]


def test_a_shape_over_the_budget_is_skipped_for_the_next():
  """A budget only the narrowest shape fits: the list goes on to it."""
  spec = spec_of('edge8f')
  order = kernel.mixed_shapes(spec)
  budget = {c: fused_entry(kernel.generate(spec, mixed_widths=True, cols=c)[1])['est_vgprs']
            for c in order}
  tight = min(budget.values())
  _, table = kernel.generate(spec, mixed_widths=True, vgpr_budget=tight)
  assert fused_entry(table)['cols'] == min(budget, key=budget.get)


def test_the_estimate_counts_a_retained_row_by_its_own_type():
  spec = specmod.inline_pointwise(spec_of('edge8f'))
  insts, _ = kernel_stream2d.build_pipeline(spec, 1, 3)
  kernel_stream2d.rotation_period(insts, 12)
  for inst in insts:
    inst.edges = dict(lo=0, hi=0)
  img, g, out = insts
  assert (img.c_type, g.c_type) == ('uint8_t', 'float')
  for cols in (4, 8, 16):
    # a loaded uint8 row: cols bytes in whole registers; a float row: cols registers
    assert kernel_stream2d.estimated_vgprs(insts, cols, mixed=True) == \
        img.keep * cols // 4 + g.keep * cols + 9 * cols + 16
  # a double row counts twice
  spec = specmod.inline_pointwise(spec_of('dsum2d'))
  insts, _ = kernel_stream2d.build_pipeline(spec, 1, 3)
  kernel_stream2d.rotation_period(insts, 12)
  for inst in insts:
    inst.edges = dict(lo=0, hi=0)
  assert kernel_stream2d.estimated_vgprs(insts, 2, mixed=True) == \
      insts[0].keep * 2 + 9 * 2 * 2 + 16


@pytest.mark.parametrize('app', APPS)
def test_geometry_aligns_strips_on_lines_of_every_tensor(app):
  """An aligned origin lies on a 128-byte line of the narrowest tensor, hence of every one;
  a lane shape too narrow for that falls back to unaligned strips."""
  spec = spec_of(app)
  for cols in TABLE[app][1]:
    k = fused_entry(kernel.generate(spec, mixed_widths=True, cols=cols)[1])
    line = 128 // min(TABLE[app][0])
    if k['origin_align'] > cols:
      assert k['origin_align'] % line == 0 and k['w_out'] % line == 0, (app, cols, k)
      assert all(k['origin_align'] * s % 128 == 0 for s in TABLE[app][0])
    else:
      assert 'exact' not in k and 64 * cols < 2 * line + line
  assert fused_entry(generated('edge8f')[1])['origin_align'] == 4     # 256 uint8: two lines
  with pytest.raises(kernel_stream2d.NotFusable):
    kernel_stream2d.geometry(specmod.inline_pointwise(spec_of('edge8f')), 1, 4, 256, 'full', 1)


@pytest.mark.parametrize('app', APPS)
def test_step_bytes_is_summed_per_tensor(app):
  spec = spec_of(app)
  k = fused_entry(generated(app)[1])
  sizes = TABLE[app][0]
  assert k['step_bytes'] == 4 * 64 * k['cols'] * sum(sizes[:-1]) + k['tile'][0] * sizes[-1]
  # a program of one width: as ever
  blur = [e for e in kernel.generate(spec_of('blur'))[1] if e['name'] == 'blur_fused_k1'][0]
  assert blur['step_bytes'] == (4 * 64 * blur['cols'] + blur['tile'][0]) * 2


# ---- compile and resources --------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
@pytest.mark.parametrize('app', APPS + ('mask2d',))
def test_the_shipped_unit_compiles_inside_its_estimate(app, tmp_path):
  """The unit build() ships, with -Werror=array-bounds: the fused kernel without scratch and
  without a spilled VGPR or SGPR, the mixed-width ones in no more VGPRs than their entry
  estimates (the estimate's factor is fitted to one compiler, kernel_stream2d.estimated_vgprs:
  where a new one allots more, re-fit it to the counts this test prints).  mask2d's kernel is
  one of the default path, whose estimate only ranks shapes: it is held to the first two."""
  spec = spec_of(app)
  text, table = kernel.generate(spec, mixed_widths=app != 'mask2d')
  k = fused_entry(table)
  figures = resource_figures(text, [k['name']], str(tmp_path / (app + '.hsaco')),
                             extra_flags=['-Werror=array-bounds'])[k['name']]
  print(k['name'], figures, 'estimate', k['est_vgprs'])
  assert figures['private_segment_fixed_size'] == 0, figures
  assert figures['vgpr_spill_count'] == 0 and figures['sgpr_spill_count'] == 0, figures
  if app != 'mask2d':
    assert 0 < figures['vgpr_count'] <= k['est_vgprs'], (figures, k['est_vgprs'])


# ---- refusals -----------------------------------------------------------------------------------

HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 4\niterate: 1\n'


def stays_per_stage(spec, why, **more):
  plain_text, plain = kernel.generate(spec, **more)
  text, table = kernel.generate(spec, mixed_widths=True, **more)
  assert table == plain and all(k['kind'] == 'stage' for k in table)
  assert without_meta(text) == without_meta(plain_text)
  assert note(text) == why, note(text)


def test_3d_and_1d_programs_are_refused():
  stays_per_stage(spec_of_text(HEAD % 'vol' + 'input uint8: a(32, 32, *)\n'
                               'output float: b(0, 0, 0) = float(a(0, 0, 0)) + float(a(1, 0, 1))\n'),
                  NOT_2D)
  stays_per_stage(spec_of_text(HEAD % 'line' + 'input uint8: a(*)\n'
                               'output float: b(0) = float(a(0)) + float(a(1))\n'), NOT_2D)


def test_several_outputs_are_refused():
  spec = spec_of_text(HEAD % 'two' + 'input uint8: a(32, *)\n'
                      'output float: b(0, 0) = float(a(0, 0)) + float(a(1, 1))\n'
                      'output float: c(0, 0) = float(a(0, 0)) - float(a(-1, 0))\n')
  why = 'not fused: the mixed-width form handles programs with one output'
  stays_per_stage(spec, why)
  # ... and the form over several outputs keeps its own refusal of mixed widths
  text, table = kernel.generate(spec, mixed_widths=True, fuse_outputs=True)
  assert note(text) == why
  assert kernel.generate(spec, fuse_outputs=True)[1] == table


def test_half_is_refused():
  spec = spec_of_text(HEAD % 'halves' + 'input half: a(32, *)\n'
                      'output float: b(0, 0) = float(a(0, 0)) + float(a(1, 1))\n')
  stays_per_stage(spec, 'not fused: the mixed-width form does not take half elements')
  with pytest.raises(kernel_stream2d.NotFusable) as e:
    kernel_stream2d.emit(spec, 1, mixed=True)
  assert str(e.value) == 'mixed widths: half elements'


def test_a_read_beyond_the_neighbour_lane_stays_per_stage_with_far_lanes_too():
  spec = spec_of_text(HEAD % 'reach' + 'input uint8: a(32, *)\n'
                      'output float: b(0, 0) = float(a(0, 0)) + float(a(-9, 1))\n')
  # 4 columns per lane: 9 columns away is three lanes
  text, table = kernel.generate(spec, mixed_widths=True, cols=4)
  assert all(k['kind'] == 'stage' for k in table)
  assert note(text) == 'not fused: x offset -9 exceeds the 4 columns a lane holds'
  text, table = kernel.generate(spec, mixed_widths=True, far_lanes=True, cols=4)
  assert all(k['kind'] == 'stage' for k in table)
  assert note(text) == 'not fused: mixed widths: a read beyond the neighbour lane'
  with pytest.raises(kernel_stream2d.NotFusable):
    kernel_stream2d.emit(spec, 1, mixed=True, cols=4, hops=3)
  # with the lane shape left to the list, 16 columns hold the read in the neighbour lane
  text, table = kernel.generate(spec, mixed_widths=True)
  assert fused_entry(table)['cols'] == 16 and note(text) == 'reach_fused_k1'
  # a program no shape takes: the note is the FIRST shape's refusal, not the last one tried
  far = spec_of_text(HEAD % 'reach' + 'input uint8: a(32, *)\n'
                     'output float: b(0, 0) = float(a(0, 0)) + float(a(-19, 1))\n')
  text, table = kernel.generate(far, mixed_widths=True)
  assert all(k['kind'] == 'stage' for k in table)
  assert note(text) == 'not fused: x offset -19 exceeds the 4 columns a lane holds'


def test_emit_without_mixed_refuses_as_ever_and_depth_2_is_refused():
  spec = specmod.inline_pointwise(spec_of('edge8f'))
  with pytest.raises(kernel_stream2d.NotFusable) as e:
    kernel_stream2d.emit(spec, 1)
  assert str(e.value) == 'inputs and output of different widths'
  with pytest.raises(kernel_stream2d.NotFusable) as e:
    kernel_stream2d.emit(spec, 2, mixed=True)
  assert str(e.value) == 'mixed widths: depth 1 only'


# ---- the switch is inert elsewhere ------------------------------------------------------------

def all_samples():
  return sorted(f[:-5] for d in (SAMPLES, os.path.join(SAMPLES, 'extra'))
                for f in os.listdir(d) if f.endswith('.soda'))


def test_every_other_sample_keeps_table_and_text_and_every_note_is_right():
  apps = [a for a in all_samples() if a not in APPS]
  assert len(apps) > 40 and 'mask2d' in apps
  for app in apps:
    spec = spec_of(app)
    text, table = kernel.generate(spec)
    out, got = kernel.generate(spec, mixed_widths=True)
    assert got == table and without_meta(out) == without_meta(text), app
    assert note(text) is None
    sizes = kernel.mixed_end_sizes(spec)
    if len(set(sizes)) == 1:
      assert note(out) == NOT_CONCERNED, (app, note(out))
    else:     # several widths outside the class: 3-D, or several outputs
      assert note(out).startswith('not fused: the mixed-width form handles'), (app, note(out))


def test_the_other_switches_leave_the_new_samples_alone():
  others = {s.keyword: True for s in switches.ALL}
  for app in APPS:
    spec = spec_of(app)
    text, table = kernel.generate(spec)
    out, got = kernel.generate(spec, **others)
    assert got == table and without_meta(out) == without_meta(text)
    both, got = kernel.generate(spec, mixed_widths=True, **others)
    assert got == generated(app)[1] and without_meta(both) == without_meta(generated(app)[0])


# ---- fixtures, output and build ---------------------------------------------------------------

def test_fixture_set_is_what_the_script_writes():
  fixtures = sorted(k for k in MANIFEST if k.endswith('.npz'))
  assert len(fixtures) == 30 == len(MANIFEST)
  assert fixtures == sorted(os.listdir(os.path.join(GOLDEN, 'mixed2d')))
  for app in APPS + ('mask2d',):
    spec = spec_of(app)
    types = specmod.tensor_c_types(spec)
    assert not {'p', 'q', 'r', 's'} & set(types)      # the reference's loop variables
    for dims in GRIDS:
      for kind in ('ramp', 'random'):
        fx = '%s.iter1.%s.%s.npz' % (app, dims, kind)
        assert fx in MANIFEST and MANIFEST[fx]['iterate'] == 1
        path = os.path.join(GOLDEN, 'mixed2d', fx)
        assert os.path.getsize(path) < 1 << 20
        data = np.load(path)
        for t in spec['inputs']:
          assert data['in_' + t['name']].dtype == np.dtype(specmod.NUMPY_NAME[t['c_type']])
        for name in spec['outputs']:
          assert data['out_' + name].dtype == np.dtype(specmod.NUMPY_NAME[types[name]])
          assert hashlib.sha256(data['out_' + name].tobytes()).hexdigest() == \
              MANIFEST[fx]['sha256'][name], (fx, name)
    # every output box keeps at least 8 cells each way on every grid
    lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), 1)[-1]
    for w, h in ((301, 53), (71, 57), (1100, 11)):
      assert w - lo[0] - hi[0] >= 8 and h - lo[1] - hi[1] >= 8, app
  # a strip seam lies inside the widest grid's box at every lane shape
  for app in APPS:
    for cols in TABLE[app][1]:
      k = fused_entry(kernel.generate(spec_of(app), mixed_widths=True, cols=cols)[1])
      assert k['w_out'] + 8 < 1100


def test_the_switch_table_row_and_what_follows_from_it():
  row = switches.BY_KEYWORD['mixed_widths']
  assert (row.flag, row.dest, row.suffix, row.depth_limit, row.note) == (
      '--hip-mixed-widths', 'hip_mixed_widths', '.mw', False, 'mixed_widths')
  # the tables of the earlier forms are held to their rows by those forms' tests: the row has
  # a table of its own, and every reader takes all three
  assert switches.MIXED_SWITCHES == (row,) and row not in switches.ALL
  assert switches.EVERY == switches.ALL + switches.MIXED_SWITCHES
  parser = argparse.ArgumentParser()
  backend.add_arguments(parser)
  assert switches.from_args(parser.parse_args(['--hip-mixed-widths']), switches.EVERY) == {
      s.keyword: s is row for s in switches.EVERY}
  assert inspect.signature(kernel.generate).parameters['mixed_widths'].default is False
  assert switches.blob_suffix(dict(mixed_widths=True)) == '.mw'
  assert entry.blob_path('x', mixed_widths=True).endswith('x.mw.hsaco')
  assert entry.MIXED_WIDTHS_APPS == APPS
  assert ('mixed_widths', APPS) in entry.SWITCH_BLOBS
  assert set(APPS + ('mask2d',)) <= set(entry.ALL_APPS)
  assert not switches.depth_limit(dict(mixed_widths=True))
  assert switches.keyword_text(dict(mixed_widths=True)) == ', mixed_widths=True'
  for app in APPS:
    assert os.path.exists(entry.sample_path(app))
    spec = spec_of(app)
    assert spec['iterate'] == 1
    assert switches.depth_limit_of(spec, dict(mixed_widths=True)) == (0, [])
    assert switches.for_program(spec, mixed_widths=True) == dict(mixed_widths=True)
  with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
    assert '--hip-mixed-widths' in f.read()
  # the form takes `mixed`; nobody passes it but the switch
  assert kernel.generate(spec_of('edge8f'), mixed=True) == kernel.generate(spec_of('edge8f'))
  with pytest.raises(TypeError):
    kernel.generate(spec_of('edge8f'), mixed_width=True)


@pytest.mark.parametrize('app', APPS)
def test_the_self_check_of_an_output_of_another_type_compiles(app):
  """`<app>_test`'s CPU half: an output of another type than its input feeds nothing back."""
  text = selfcheck.generate_cpp(spec_of(app))
  assert 'it == 0 ?' not in text and '(const %s*)inputs[0];' % spec_of(app)['inputs'][0]['c_type'] in text
  r = subprocess.run(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-x', 'c++', '-'],
                     input=text, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'quant2d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-mixed-widths', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['quant2d.h', 'quant2d.hsaco', 'quant2d.py',
                                     'quant2d_host.cpp', 'quant2d_kernel.hip']
  assert (out / 'quant2d_kernel.hip').read_text() == generated('quant2d')[0]
  assert (out / 'quant2d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'quant2d.py').read_text()
  compile(shim, 'quant2d.py', 'exec')
  assert 'mixed_widths=True' in shim and 'program.set_max_depth(' not in shim
  host_cpp = (out / 'quant2d_host.cpp').read_text()
  assert '"quant2d_fused_k1"' in host_cpp and 'soda_hip_plan_set_max_depth' not in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'quant2d_host.cpp')])
  # without the flag: the per-stage kernels only
  plain = tmp_path / 'plain'
  r = subprocess.run([sys.executable, SODAC, sample, '--hip', str(plain)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert '_fused_k' not in (plain / 'quant2d_kernel.hip').read_text()


def test_the_measurement_tool_prints_its_usage():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'mixed2d', 'mixed2d_bench.py'),
                      '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert 'mixed_widths' in r.stdout and '--apps' in r.stdout and '--build-only' in r.stdout
