"""LDS-plane kernels for high-order 3-D stencils (soda_hip/codegen/kernel_stream3d_lds.py;
kernel.generate's `lds_planes`), without a GPU: the switch is opt-in and leaves every table
that has a fused kernel alone, the samples get exactly one `<app>_fused_k1l`, it compiles
for gfx950 without scratch or spills and with the LDS its entry names, programs outside
the form keep their stage kernels and a note that names the reason, the checker agrees
with the reference's fixtures, and the launch planner walks star3d's shrinking boxes."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from soda_hip.codegen import (kernel, kernel_common, kernel_stage, kernel_stream2d,
                              kernel_stream3d_lds)
from soda_hip.codegen import spec as specmod

import test_schedule as ts
from codegen_util import (HIPCC, READELF, SODAC, notes_of, resource_figures, spec_of,
                          spec_of_text, without_meta)
from conftest import ROOT, SAMPLES
from test_schedule import probe      # noqa: F401  (the planner probe, built once)

APPS = ('star3d', 'iso3dfd', 'skewstar3d')
UNTOUCHED = ('jacobi3d', 'heat3d', 'denoise3d', 'wave3d', 'maxwell3d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'lds3d_manifest.json')) as _f:
  MANIFEST = json.load(_f)
with open(os.path.join(GOLDEN, 'random_programs.json')) as _f:
  RANDOM = json.load(_f)

def lds_note(text):
  return kernel_common.read_meta_from_source(text).get('lds_planes')


# ---- the tables ------------------------------------------------------------------------------

OLD_NOTES = {
    'star3d': ['// depth 1 not fused: x offset 3 exceeds the 2 columns a lane holds',
               '// depth 2 not fused: depth 2 leaves no output cells in a 128x12 tile'],
    'iso3dfd': ['// depth 1 not fused: x offset 2 exceeds the 1 columns a lane holds'],
    'skewstar3d': ['// depth 1 not fused: x offset -3 exceeds the 2 columns a lane holds',
                   '// depth 2 not fused: depth 2 leaves no output cells in a 128x12 tile'],
}


@pytest.mark.parametrize('app', APPS)
def test_without_the_switch_stage_kernels_only(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  stage_text, stage_table = kernel_stage.emit(specmod.inline_pointwise(spec))
  assert [k['kind'] for k in table] == ['stage'] and table[0]['name'] == stage_table[0]['name']
  assert stage_text in text and '_fused_k' not in text
  assert notes_of(text) == OLD_NOTES[app]
  assert lds_note(text) is None
  assert kernel.generate(spec, lds_planes=False) == (text, table)


@pytest.mark.parametrize('app', APPS)
def test_with_the_switch_one_fused_kernel(app):
  spec = spec_of(app)
  plain_text, plain = kernel.generate(spec)
  text, table = kernel.generate(spec, lds_planes=True)
  assert table[:-1] == plain and [k['kind'] for k in table] == ['stage', 'fused']
  k = table[-1]
  assert k['name'] == app + '_fused_k1l' and k['depth'] == 1 and k['stage'] == -1
  assert 0 < k['lds_bytes'] <= 65536 and k['est_vgprs'] <= 250
  assert k['fill_rows'] > 0 and k['step_valu'] > 0 and k['step_bytes'] > 0
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  C = 16 // elem
  lanes_x = k['tile'][0] // C
  assert k['cols'] == C == k['origin_align'] and k['block'] == [64 * k['waves'], 1, 1]
  assert k['tile'] == [lanes_x * C, k['waves'] * (64 // lanes_x) * k['rows'], 64, 1]
  assert k['tile'][:2] == [k['w_out'], k['r_out']]
  # the halo covers the window, in whole vectors along x; the LDS is two slots of it
  lo, hi = spec['radius']['lo'], spec['radius']['hi']
  hxl, hxh, hyl, hyh = k['halo']
  assert (hxl, hxh) == (-(-lo[0] // C) * C, -(-hi[0] // C) * C) and (hyl, hyh) == (lo[1], hi[1])
  assert k['lds_bytes'] == 2 * (k['tile'][0] + hxl + hxh) * (k['tile'][1] + hyl + hyh) * elem
  assert k['fill_rows'] == lo[2] + hi[2] + 1
  # bytes: the LDS plane with its halo, the centre-only inputs and the output tile for tile
  cells = k['tile'][0] * k['tile'][1]
  assert k['step_bytes'] == (k['lds_bytes'] // (2 * elem) + len(spec['inputs']) * cells) * elem
  assert k['step_valu'] == k['waves'] * kernel.arithmetic_weight(spec) * k['rows'] * C * 2
  # the first shape, by loaded over stored cells, that fits the budget and the LDS cap
  lowered = specmod.inline_pointwise(spec)
  ratios = []
  for shape in kernel_stream3d_lds.shapes_by_loaded_cells(lowered):
    _, fields = kernel_stream3d_lds.analyse(lowered)
    ratios.append(kernel_stream3d_lds.geometry(fields, elem, *shape)['loaded'])
    if shape == (k['waves'], k['rows'], lanes_x):
      break
    with pytest.raises(kernel_stream2d.NotFusable, match='would need'):
      kernel_stream3d_lds.emit(lowered, 1, *shape)
  assert ratios == sorted(ratios) and len(ratios) < len(kernel_stream3d_lds.SHAPES)
  # the old notes stay, nothing is said twice, and the metadata names the kernel
  assert notes_of(text) == OLD_NOTES[app] and lds_note(text) == k['name']
  assert text.count('void %s(soda_hip_args a)' % k['name']) == 1
  assert kernel_common.read_meta_from_source(text)['kernels'] == table
  # a named shape is taken as it is
  _, forced = kernel.generate(spec, lds_planes=True, lds_shape=(4, 1, 16))
  assert forced[-1]['block'] == [256, 1, 1] and forced[-1]['rows'] == 1
  assert forced[-1]['tile'][:2] == [16 * C, 16]


def test_register_windows_are_the_z_windows():
  _, fields = kernel_stream3d_lds.analyse(spec_of('iso3dfd'))
  by = {f.name: f for f in fields}
  assert [(by[n].lds, by[n].keep) for n in ('up', 'vel', 'u')] == [(False, 2), (False, 2),
                                                                   (True, 10)]
  assert (by['u'].zlo, by['u'].zhi, by['u'].zc) == (-4, 4, 0)
  _, (a,) = kernel_stream3d_lds.analyse(spec_of('skewstar3d'))
  assert (a.zlo, a.zhi, a.zc, a.hx, a.hy) == (-1, 3, 0, (3, 5), (3, 3))
  # an even period of which every field's slot count is a divisor
  period, slots = kernel_stream3d_lds.rotation(fields, 16)
  assert period == 10 and slots == dict(up=2, vel=2, u=10)


# ---- the compiler ----------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', APPS)
def test_kernels_compile_for_gfx950_without_scratch_or_spills(app, tmp_path):
  """From the compiler's resource report: no private segment, no spilled VGPRs, no SGPRs
  parked in VGPR lanes, the static LDS of the entry; array subscripts in bounds at compile
  time."""
  text, table = kernel.generate(spec_of(app), lds_planes=True)
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
TWO_PLANES = _HEAD % 'twoplanes' + '''input float: a(32, 32, *)
output float: b(0, 0, 0) = a(3, 0, 0) + a(1, 0, 1) + a(0, 0, 0)
'''
TWO_STAGES = _HEAD % 'twostages' + '''input float: a(32, 32, *)
local float: t(0, 0, 0) = a(3, 0, 0) + a(-3, 0, 0) + a(0, 3, 0)
output float: b(0, 0, 0) = t(0, -3, 0) + t(0, 0, 3) + t(0, 0, -3)
'''
TWO_OUTPUTS = (_HEAD % 'twoouts').replace('iterate: 2', 'iterate: 1') + '''input float: a(32, 32, *)
output float: b(0, 0, 0) = a(3, 0, 0) + a(-3, 0, 0)
output float: c(0, 0, 0) = a(0, 3, 0) + a(0, 0, -3)
'''
TWO_BYTES = _HEAD % 'shorts' + '''input uint16: a(32, 32, *)
output uint16: b(0, 0, 0) = a(9, 0, 0) + a(-9, 0, 0) + a(0, 3, 0) * 3
'''


@pytest.mark.parametrize('text,reason', [
    (TWO_PLANES, 'input a is read off the z axis at plane offsets 0 and 1: one plane of an '
                 'input lies in LDS'),
    (TWO_STAGES, '2 stages: the LDS-plane form takes one stage, the output'),
    (TWO_OUTPUTS, '2 outputs: the LDS-plane form stores one'),
    (TWO_BYTES, '2-byte elements: the LDS-plane form handles 4- and 8-byte ones')])
def test_programs_outside_the_form_keep_their_stage_kernels_and_get_a_note(text, reason):
  """The note is the entry `lds_planes` of the metadata in the kernel text: everything
  before the metadata is the text without the switch."""
  spec = spec_of_text(text)
  plain_text, plain = kernel.generate(spec)
  assert all(k['kind'] == 'stage' for k in plain) and lds_note(plain_text) is None
  out, table = kernel.generate(spec, lds_planes=True)
  assert table == plain and len(table) == len(specmod.inline_pointwise(spec)['stages'])
  assert lds_note(out) == 'not fused: ' + reason
  assert without_meta(out) == without_meta(plain_text)
  with pytest.raises(kernel_stream2d.NotFusable) as e:
    kernel_stream3d_lds.emit(specmod.inline_pointwise(spec))
  assert str(e.value) == reason


def test_what_no_shape_fits_is_refused_with_the_figures():
  lowered = specmod.inline_pointwise(spec_of('star3d'))
  with pytest.raises(kernel_stream2d.NotFusable, match='would need about 282 VGPRs'):
    kernel_stream3d_lds.emit(lowered, 1, 4, 4, 32)
  with pytest.raises(kernel_stream2d.NotFusable, match=r'84480 bytes of LDS \(cap 65536\)'):
    kernel_stream3d_lds.emit(lowered, 1, 8, 4, 64)
  with pytest.raises(kernel_stream2d.NotFusable, match='depth 1'):
    kernel_stream3d_lds.emit(lowered, 2)
  # reads along z only: the register forms take that
  axis = spec_of_text(_HEAD % 'axis' + 'input float: a(32, 32, *)\n'
                      'output float: b(0, 0, 0) = a(0, 0, 3) + a(0, 0, -3)\n')
  with pytest.raises(kernel_stream2d.NotFusable, match='no read off the z axis'):
    kernel_stream3d_lds.emit(axis)


# ---- every other program keeps its table -----------------------------------------------------

RANDOM_3D = sorted(k for k, p in RANDOM.items() if p['dim'] == 3)
# the 3-D programs without a fused depth-1 kernel today: each is multi-stage, has several
# outputs or elements that are not 4 or 8 bytes wide - outside the LDS-plane form as well
RANDOM_UNFUSED = ['ops5', 'plain22', 'plain30', 'plain5', 'plain7', 'plain8', 'struct10',
                  'struct11', 'struct13', 'struct15', 'struct2', 'struct3']


def test_random_programs_keep_table_and_text():
  assert len(RANDOM_3D) == 33
  unfused = []
  for key in RANDOM_3D:
    spec = spec_of_text(RANDOM[key]['text'])
    text, table = kernel.generate(spec)
    lds_text, lds_table = kernel.generate(spec, lds_planes=True)
    assert lds_table == table, key
    assert without_meta(lds_text) == without_meta(text), key
    if any(k['kind'] == 'fused' and k['depth'] == 1 for k in table):
      assert lds_note(lds_text).startswith('not wanted: %s_fused_k1' % spec['app_name']), key
    else:
      unfused.append(key)
      lowered = specmod.inline_pointwise(spec)
      widths = {specmod.ELEM_SIZE[t] for t in specmod.tensor_c_types(lowered).values()}
      assert len(lowered['stages']) > 1 or len(spec['outputs']) > 1 or \
          not widths <= {4, 8}, key
      assert lds_note(lds_text).startswith('not fused: '), key
  assert unfused == RANDOM_UNFUSED


def test_samples_without_a_fused_kernel_are_outside_the_form():
  for app in ('grad3d', 'mix3d'):
    spec = spec_of(app)
    text, table = kernel.generate(spec)
    assert all(k['kind'] == 'stage' for k in table)
    lds_text, lds_table = kernel.generate(spec, lds_planes=True)
    assert lds_table == table and without_meta(lds_text) == without_meta(text)
    assert lds_note(lds_text) == 'not fused: %d outputs: the LDS-plane form stores one' % len(
        spec['outputs'])


@pytest.mark.parametrize('app', UNTOUCHED)
def test_samples_with_a_fused_kernel_keep_table_and_text(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec)
  assert any(k['kind'] == 'fused' and k['depth'] == 1 for k in table)
  lds_text, lds_table = kernel.generate(spec, lds_planes=True)
  assert lds_table == table and without_meta(lds_text) == without_meta(text)
  assert lds_note(lds_text) == 'not wanted: %s_fused_k1' % app


def test_two_dimensional_programs_are_not_concerned():
  spec = spec_of('jacobi2d')
  text, table = kernel.generate(spec)
  lds_text, lds_table = kernel.generate(spec, lds_planes=True)
  assert lds_table == table and without_meta(lds_text) == without_meta(text)


# ---- fixtures --------------------------------------------------------------------------------

FIXTURES = sorted(k for k in MANIFEST if k.endswith('.npz'))
CASES = ('41x19x18', '23x27x21')


def test_fixture_set_is_what_the_script_writes():
  assert len(FIXTURES) == 20 == len(MANIFEST)
  assert sorted(FIXTURES) == sorted(os.listdir(os.path.join(GOLDEN, 'lds3d')))
  for app, iterations in (('star3d', (1, 2)), ('iso3dfd', (1,)), ('skewstar3d', (1, 2))):
    for it in iterations:
      for dims in CASES:
        for kind in ('ramp', 'random'):
          fx = '%s.iter%d.%s.%s.npz' % (app, it, dims, kind)
          assert fx in MANIFEST
          assert os.path.getsize(os.path.join(GOLDEN, 'lds3d', fx)) < 1 << 20


@pytest.mark.skipif(shutil.which('g++') is None, reason='the oracle needs g++')
@pytest.mark.parametrize('app', APPS)
def test_oracle_equals_the_reference_fixtures(app):
  """Array for array: the oracle's values on the output's box, the reference's zeros outside
  it, and the bytes the manifest pins."""
  from oracle import soda_oracle
  spec = spec_of(app)
  orc = soda_oracle.Oracle(spec)
  n = 0
  for fx in FIXTURES:
    meta = MANIFEST[fx]
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'lds3d', fx))
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
  assert n == (4 if app == 'iso3dfd' else 8)


# ---- the launch planner ----------------------------------------------------------------------

def test_planner_walks_star3d_at_512_cubed(probe, tmp_path, monkeypatch):      # noqa: F811
  """512^3 x 4 with the `.lds` table, default schedule: four launches of star3d_fused_k1l,
  boxes 4 cells shorter per side and launch, the grid of tiles and chunks covers each box
  exactly once; under set_max_depth(-1) four launches of the stage kernel."""
  source = spec_of('star3d')
  table = kernel.generate(source, lds_planes=True)[1]
  spec = specmod.inline_pointwise(source)
  monkeypatch.setattr(ts, 'program', lambda app, iterate: (spec, table))
  dims = (512, 512, 512)
  cases = [dict(ts.case(dims, 4, md), final_only=fo, valid_lo=(0, 0, 0), valid_hi=(0, 0, 0))
           for md in (0, 1, -1) for fo in (0, 1)]
  k = table[-1]
  for w, static in ((1, k['lds_bytes']), (2, k['lds_bytes'])):
    for c, r in ts.plan(probe, tmp_path, 'star3d', 4, cases, w, static):
      assert r['rc'] == 0, (c, r['error'])
      ts.check_depths_and_boxes(spec, table, c, r)
      ts.check_routing(spec, table, c, r)
      ts.check_grids(spec, table, c, r, w, static)
      names = [table[l['kernel']]['name'] for l in r['launches']]
      if c['max_depth'] < 0:
        assert names == ['star3d_stage_b'] * 4
        continue
      assert names == ['star3d_fused_k1l'] * 4
      for i, l in enumerate(r['launches']):
        m = 4 * (i + 1)
        assert l['lo'][:3] == [m] * 3 and l['hi'][:3] == [512 - m] * 3
        # tiles start at the box's first column rounded down to a vector, at its first row
        # and plane: every cell of the box in exactly one tile and one chunk
        x0 = m - m % k['origin_align']
        chunk = l['param'][0]
        assert chunk >= 8 and l['param'][1:] == [0, 0, 0]
        assert l['grid'] == [ts.ceil_div(512 - m - x0, k['tile'][0]),
                             ts.ceil_div(512 - 2 * m, k['tile'][1]),
                             ts.ceil_div(512 - 2 * m, chunk)]
        for d, (first, size) in enumerate(((x0, k['tile'][0]), (m, k['tile'][1]), (m, chunk))):
          n = l['grid'][d]
          assert first <= l['lo'][d] < first + size                    # the first tile is not empty
          assert first + (n - 1) * size < l['hi'][d] <= first + n * size   # nor is the last
        assert l['lds'] == 0 and l['est_us'] > 0


# ---- sodac -----------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'skewstar3d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-lds-planes', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['skewstar3d.h', 'skewstar3d.hsaco', 'skewstar3d.py',
                                     'skewstar3d_host.cpp', 'skewstar3d_kernel.hip']
  text = (out / 'skewstar3d_kernel.hip').read_text()
  assert text == kernel.generate(spec_of('skewstar3d'), lds_planes=True)[0]
  assert (out / 'skewstar3d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'skewstar3d.py').read_text()
  compile(shim, 'skewstar3d.py', 'exec')
  assert 'lds_planes=True' in shim and 'set_max_depth' not in shim
  host_cpp = (out / 'skewstar3d_host.cpp').read_text()
  assert '"skewstar3d_fused_k1l"' in host_cpp and 'set_max_depth' not in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'skewstar3d_host.cpp')])
  plain = tmp_path / 'plain'
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-kernel', str(plain) + '.hip',
                      '--hip-host', str(plain) + '.py', '--hip-host-cpp', str(plain) + '.cpp'],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  for suffix in ('.hip', '.py', '.cpp'):
    got = open(str(plain) + suffix).read()
    assert 'fused_k1l' not in got and 'lds_planes' not in got


def test_the_measurement_tool_prints_its_usage():
  """tools/lds3d/lds3d_bench.py lies below tools/ (tests/test_tools.py starts the scripts of
  tools/ itself): `--help` prints the usage and exits 0 without touching a GPU."""
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'lds3d', 'lds3d_bench.py'),
                      '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert 'lds_planes' in r.stdout and '--build-candidates' in r.stdout
