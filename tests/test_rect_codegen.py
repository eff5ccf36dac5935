"""Fused one-pass kernels for 2-D / 3-D programs with several outputs that do not feed the
inputs pairwise ("rectangular": kernel_stream2d.rectangular; kernel.generate's
`fuse_outputs`), without a GPU: the switch is opt-in and leaves every other table alone,
every refusal is written into the kernel text, the extras a launch carries are the boxes'
own differences - planned fresh and resumed with a valid region per input -, the kernels
compile for gfx950 without scratch memory or spilled registers, and `sodac
--hip-fuse-outputs` writes every product."""
import json
import os
import struct
import subprocess
import sys

import pytest

from soda_hip import frontend
from soda_hip.codegen import (kernel, kernel_fields2d, kernel_fields3d, kernel_stage,
                              kernel_stream2d)
from soda_hip.codegen import spec as specmod

from codegen_util import (HIPCC, READELF, SODAC, notes_of, resource_figures, spec_of,
                          spec_of_text)
from conftest import ROOT, SAMPLES
from test_schedule_fields import extras_of, header, pad4, parse, probes  # noqa: F401

APPS = ('grad2d', 'blend2d', 'grad3d', 'mix3d')
ALL = APPS + ('outchain',)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rect')

@pytest.mark.parametrize('app', ALL)
def test_a_plain_generate_has_stage_kernels_only(app):
  """Without the switch: the per-stage kernels, their text as kernel_stage prints it, and
  the single-output forms' own refusal in the notes - what the table held before the
  switch existed (tools/kernel_text_digests.py compares the whole text with a parent)."""
  spec = spec_of(app)
  assert kernel_stream2d.rectangular(spec) and not kernel_stream2d.multi_field(spec)
  text, table = kernel.generate(spec)
  stage_text, stage_table = kernel_stage.emit(specmod.inline_pointwise(spec))
  assert [k['kind'] for k in table] == ['stage'] * len(spec['stages'])
  assert [k['name'] for k in table] == [k['name'] for k in stage_table]
  assert stage_text in text and '_fused_k' not in text
  assert notes_of(text) == ['// depth 1 not fused: stream%dd handles single-output programs'
                            % spec['dim']]
  assert kernel.generate(spec, fuse_outputs=False)[0] == text


@pytest.mark.parametrize('app', ALL)
def test_the_switch_adds_one_fused_depth_1_kernel(app):
  spec = spec_of(app)
  text, table = kernel.generate(spec, fuse_outputs=True)
  stage_text, stage_table = kernel_stage.emit(specmod.inline_pointwise(spec))
  assert stage_text in text and notes_of(text) == []
  assert [k['name'] for k in table[:-1]] == [k['name'] for k in stage_table]
  last = table[-1]
  assert (last['kind'], last['depth'], last['name']) == ('fused', 1, app + '_fused_k1')
  assert last['fields'] == len(spec['outputs'])
  assert last['fill_rows'] >= 0 and last['step_bytes'] > 0 and last['step_valu'] > 0
  # the halo is the hull of the composed windows over all outputs
  lo, hi = specmod.iteration_margins(spec, 1)[-1]
  cols = last['cols']
  assert last['halo'] == [-(-lo[0] // cols) * cols, -(-hi[0] // cols) * cols]
  assert last['w_out'] == 64 * cols - sum(last['halo'])
  if spec['dim'] == 3:
    assert last['r_out'] == last['rows'] - lo[1] - hi[1]
  # depths, a depth limit and a chain of requests change nothing: one pass is one deep
  assert kernel.generate(spec, fuse_outputs=True, depths=[2, 4], max_depth=8)[1] == table


def test_outchain_keeps_the_output_another_stage_reads_in_its_window():
  text, table = kernel.generate(spec_of('outchain'), fuse_outputs=True)
  rows = {l.split()[1]: l.split() for l in text.splitlines() if l.startswith('//   k0_')}
  # `first` feeds `second` at rows -1 and +1: three rows kept (rounded up to a divisor of
  # the rotation period), AND stored; `second` leaves from a row of temporaries
  assert int(rows['k0_first'][3]) >= 3 and rows['k0_first'][-2:] == ['->', 'HBM']
  assert int(rows['k0_second'][3]) == 0 and rows['k0_second'][-2:] == ['->', 'HBM']
  assert 'g_out0' in text and 'g_out1' in text


def test_an_output_of_a_type_no_input_has_gets_its_vector_type():
  text, _ = kernel.generate(spec_of('blend2d'), fuse_outputs=True)
  for c_type in ('float', 'int32_t', 'uint32_t'):
    assert 'vec_blend2d_fused_k1_%s ' % c_type in text


_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: %d\n'


def test_too_many_outputs_are_refused_with_the_reason():
  for dim, limit, tile in ((2, kernel_fields2d.MAX_OUTPUTS, '(32, *)'),
                           (3, kernel_fields3d.MAX_OUTPUTS, '(32, 32, *)')):
    zero = ', '.join('0' * dim)
    for n in (limit, limit + 1):
      text = _HEAD % ('many', 1) + 'input float: a%s\n' % tile + ''.join(
          'output float: o%d(%s) = a(%s) * %d.0f\n' % (j, zero, zero, j + 2) for j in range(n))
      out, table = kernel.generate(spec_of_text(text), fuse_outputs=True)
      if n == limit:
        assert table[-1]['kind'] == 'fused' and table[-1]['fields'] == n
      else:
        assert all(k['kind'] == 'stage' for k in table)
        assert notes_of(out) == ['// depth 1 not fused: %d outputs: the launch arguments '
                                 'carry the boxes of %d' % (n, limit)]


def test_mixed_widths_are_refused_with_the_reason():
  # an output, and a local, of another width than the input
  for dim, tile, zero in ((2, '(32, *)', '0, 0'), (3, '(32, 32, *)', '0, 0, 0')):
    wide_out = _HEAD % ('widths', 1) + 'input float: a%s\n' % tile + \
        'output float: o(%s) = a(%s) * 2.0f\noutput double: p(%s) = a(%s) * 0.5\n' % (
            (zero,) * 4)
    one = zero.replace('0', '1', 1)
    wide_local = _HEAD % ('widths', 1) + 'input float: a%s\n' % tile + \
        'local double: m(%s) = a(%s) * 0.5\n' % (zero, zero) + \
        'output float: o(%s) = float(m(%s)) + a(%s)\n' % (zero, one, zero) + \
        'output float: p(%s) = float(m(%s)) - a(%s)\n' % (zero, zero, one)
    for text in (wide_out, wide_local):
      out, table = kernel.generate(spec_of_text(text), fuse_outputs=True)
      assert all(k['kind'] == 'stage' for k in table)
      note, = notes_of(out)
      assert 'widths' in note, note


def test_an_x_offset_beyond_the_lane_is_refused_with_the_reason():
  far2 = _HEAD % ('far', 1) + 'input float: a(32, *)\n' \
      'output float: o(0, 0) = a(0, 0) + a(5, 0)\noutput float: p(0, 0) = a(0, 1)\n'
  out, table = kernel.generate(spec_of_text(far2), fuse_outputs=True)
  assert all(k['kind'] == 'stage' for k in table)
  assert notes_of(out) == ['// depth 1 not fused: x offset 5 exceeds the 4 columns a lane holds']
  # four columns away is the neighbouring lane's: taken
  _, table = kernel.generate(spec_of_text(far2.replace('a(5, 0)', 'a(4, 0)')), fuse_outputs=True)
  assert table[-1]['kind'] == 'fused'
  far3 = _HEAD % ('far', 1) + 'input float: a(32, 32, *)\n' \
      'output float: o(0, 0, 0) = a(0, 0, 0) + a(-3, 0, 0)\noutput float: p(0, 0, 0) = a(0, 1, 0)\n'
  out, table = kernel.generate(spec_of_text(far3), fuse_outputs=True)
  assert all(k['kind'] == 'stage' for k in table)
  note, = notes_of(out)
  assert 'x offset -3 exceeds the' in note and 'columns a lane holds' in note


def test_a_3d_program_takes_at_most_four_inputs():
  """Tile rows x inputs are capped (kernel.RECT3D_INPUT_ROWS) and the smallest tile has 8
  rows: four inputs get 8-row tiles, five the reason in the kernel text; 2-D has no cap."""
  def text(n, dim):
    zero = ', '.join('0' * dim)
    tile = '(32, *)' if dim == 2 else '(32, 32, *)'
    lines = ['input float: f%d%s' % (j, tile if j == n - 1 else '') for j in range(n)]
    total = ' + '.join('f%d(%s)' % (j, zero) for j in range(n))
    lines += ['output float: o(%s) = %s' % (zero, total),
              'output float: p(%s) = f0(%s) * 2.0f' % (zero, zero.replace('0', '1', 1))]
    return _HEAD % ('wide', 1) + '\n'.join(lines) + '\n'
  assert 8 * 4 <= kernel.RECT3D_INPUT_ROWS < 8 * 5
  _, table = kernel.generate(spec_of_text(text(4, 3)), fuse_outputs=True)
  assert table[-1]['kind'] == 'fused' and table[-1]['rows'] == 8
  out, table = kernel.generate(spec_of_text(text(5, 3)), fuse_outputs=True)
  assert all(k['kind'] == 'stage' for k in table)
  assert notes_of(out) == ['// depth 1 not fused: 5 inputs, 3-D tiles take %d rows x inputs'
                           % kernel.RECT3D_INPUT_ROWS]
  _, table = kernel.generate(spec_of_text(text(7, 2)), fuse_outputs=True)
  assert table[-1]['kind'] == 'fused'


@pytest.mark.parametrize('app', APPS)
def test_an_iterated_program_with_unequal_counts_is_refused_with_the_reason(app):
  """The DSL refuses such a text; a spec that says so anyway (another front end) keeps its
  per-stage kernels and the reason."""
  with pytest.raises(Exception, match='iterate > 1'):
    frontend.load(os.path.join(SAMPLES, 'extra', app + '.soda'), iterate=2)
  spec = dict(spec_of(app), iterate=2)
  assert not kernel_stream2d.rectangular(spec)
  text, table = kernel.generate(spec, fuse_outputs=True)
  assert all(k['kind'] == 'stage' for k in table)
  assert ('// outputs not fused: iterate 2 over %d input(s) and %d output(s) that do not '
          'feed each other pairwise' % (len(spec['inputs']), len(spec['outputs']))) in text
  with pytest.raises(kernel_stream2d.NotFusable, match='pairwise'):
    (kernel_fields2d if spec['dim'] == 2 else kernel_fields3d).emit(spec, 1)


@pytest.mark.parametrize('app', ('wave2d', 'maxwell3d', 'jacobi2d', 'denoise3d'))
def test_other_programs_are_unaffected_by_the_switch(app):
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  spec = specmod.spec_from_stencil(frontend.load(path))
  assert not kernel_stream2d.rectangular(spec)
  assert kernel.generate(spec, fuse_outputs=True) == kernel.generate(spec)


# ---- the planner ---------------------------------------------------------------------------

CUS = 256
GRIDS = {2: [(64, 48), (37, 29), (300, 61)], 3: [(20, 18, 16), (33, 9, 12), (70, 20, 24)]}


def composed(spec, start):
  """{tensor: (lo, hi)} of one pass whose input j starts from the box start[j] - what
  csrc/schedule.cpp (grow_boxes) composes for a resumed sweep.  An independent restatement
  from the program's stage windows, on purpose: the planner's boxes are checked against
  it here and the resumed GPU run in tests/test_gpu_rect.py takes its boxes from it."""
  boxes = {t['name']: b for t, b in zip(spec['inputs'], start)}
  for stage, wins in specmod.stage_windows(spec).items():
    los = [[p + w for p, w in zip(boxes[parent][0], wlo)] for parent, (wlo, _) in wins.items()]
    his = [[p + w for p, w in zip(boxes[parent][1], whi)] for parent, (_, whi) in wins.items()]
    boxes[stage] = ([min(0, *v) for v in zip(*los)], [max(0, *v) for v in zip(*his)])
  return boxes


def plan(probes, tmp_path, spec, table, cases):
  req = header(spec, table) + struct.pack('=i', len(cases))
  for c in cases:
    req += struct.pack('=4i4q', c['max_depth'], 0, 1, 0, *pad4(c['dims'], 1))
    for side in ('lo', 'hi'):
      for v in c[side]:
        req += struct.pack('=4i', *pad4(v, 0))
  path = tmp_path / (spec['app_name'] + '.req')
  path.write_bytes(req)
  out = subprocess.check_output([probes['schedule_fields_probe'], str(path)], text=True)
  return parse(out, len(cases))


@pytest.mark.parametrize('app', ALL)
def test_planned_extras_are_the_python_extras(probes, tmp_path, app):
  """Fresh runs, runs resumed from one margin for all inputs and from a margin per input:
  under a depth limit of 1 ONE fused launch whose box is the intersection of the outputs'
  boxes and whose extras unpack to each output's own box; per stage otherwise (the default
  included).  Fresh and uniformly resumed, the extras are output_extras()."""
  source = spec_of(app)
  table = kernel.generate(source, fuse_outputs=True)[1]
  spec = specmod.inline_pointwise(source)
  dim, n_in, n_out = spec['dim'], len(spec['inputs']), len(spec['outputs'])
  fields = kernel_fields2d if dim == 2 else kernel_fields3d
  python_extras = fields.output_extras(spec, 0, 1)
  assert any(any(ex) for ex in python_extras)
  zero = (0,) * dim
  regions = [([zero] * n_in, [zero] * n_in),
             ([tuple(1 + d for d in range(dim))] * n_in, [tuple(2 - d % 2 for d in range(dim))] * n_in),
             ([tuple((j + d) % 3 for d in range(dim)) for j in range(n_in)],
              [tuple((2 * j + d + 1) % 4 for d in range(dim)) for j in range(n_in)])]
  cases = [dict(dims=dims, max_depth=md, lo=lo, hi=hi)
           for dims in GRIDS[dim] for lo, hi in regions for md in (1, 0, -1)]
  results = plan(probes, tmp_path, spec, table, cases)
  for c, r in zip(cases, results):
    assert r['rc'] == 0, (c, r['error'])
    launches = r['launches']
    if c['max_depth'] != 1:
      assert [table[l['kernel']]['kind'] for l in launches] == ['stage'] * len(spec['stages']), c
      continue
    assert len(launches) == 1 and table[launches[0]['kernel']]['name'] == app + '_fused_k1', c
    l, = launches
    # inputs from the caller's arrays, every output to its own: no ping-pong partner, no local
    assert r['lines'][0].split(' buf ')[1].split() == \
        ['i%d' % j for j in range(n_in)] + \
        ['o%d' % spec['outputs'].index(s['name']) if s['name'] in spec['outputs'] else '-0'
         for s in spec['stages']], r['lines']
    vlo = [min(v[d] for v in c['lo']) for d in range(dim)]
    vhi = [min(v[d] for v in c['hi']) for d in range(dim)]
    start = [([-(v[d] - vlo[d]) for d in range(dim)], [w[d] - vhi[d] for d in range(dim)])
             for v, w in zip(c['lo'], c['hi'])]
    boxes = composed(spec, start)
    own = []
    for j, o in enumerate(spec['outputs']):
      ex = extras_of(dim, l, j)
      olo, ohi = boxes[o]
      box = [(l['lo'][d] - ex[d], l['hi'][d] + ex[dim + d]) for d in range(dim)]
      assert box == [(vlo[d] - olo[d], c['dims'][d] - vhi[d] - ohi[d]) for d in range(dim)], (c, o)
      assert all(0 <= a < b <= c['dims'][d] for d, (a, b) in enumerate(box)), (c, o)
      own.append(box)
      if all(s == start[0] for s in start):
        assert tuple(ex) == python_extras[j], (c, o)
        words = fields.pack_extras(python_extras)
        assert [p & (2 ** 64 - 1) for p in l['param'][1:4]] == words
    for d in range(dim):
      assert l['lo'][d] == max(b[d][0] for b in own) and l['hi'][d] == min(b[d][1] for b in own)


# ---- the compiler --------------------------------------------------------------------------

@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', ALL)
def test_kernels_compile_for_gfx950_without_scratch_or_spills(app, tmp_path):
  """From the compiler's resource report: no private segment, no spilled VGPRs, no SGPRs
  parked in VGPR lanes; array subscripts in bounds at compile time."""
  text, table = kernel.generate(spec_of(app), fuse_outputs=True)
  kname = table[-1]['name']
  figures = resource_figures(text, [kname], str(tmp_path / (app + '.hsaco')),
                             extra_flags=['-Werror=array-bounds'])[kname]
  assert figures['private_segment_fixed_size'] == 0, (kname, figures)
  assert figures['vgpr_spill_count'] == 0, (kname, figures)
  assert figures['sgpr_spill_count'] == 0, (kname, figures)
  assert 0 < figures['vgpr_count'] <= 256, (kname, figures)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_sodac_writes_all_products_with_the_switch(tmp_path):
  out = tmp_path / 'out'
  sample = os.path.join(SAMPLES, 'extra', 'grad2d.soda')
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-fuse-outputs', '--hip', str(out)],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  assert sorted(os.listdir(out)) == ['grad2d.h', 'grad2d.hsaco', 'grad2d.py', 'grad2d_host.cpp',
                                     'grad2d_kernel.hip']
  text = (out / 'grad2d_kernel.hip').read_text()
  assert text == kernel.generate(spec_of('grad2d'), fuse_outputs=True)[0]
  assert (out / 'grad2d.hsaco').read_bytes()[:4] == b'\x7fELF'
  shim = (out / 'grad2d.py').read_text()
  compile(shim, 'grad2d.py', 'exec')
  assert 'program.set_max_depth(1)' in shim and 'fuse_outputs=True' in shim
  host_cpp = (out / 'grad2d_host.cpp').read_text()
  assert '"grad2d_fused_k1"' in host_cpp and 'soda_hip_plan_set_max_depth(plan, 1)' in host_cpp
  subprocess.check_call(['g++', '-std=c++11', '-fopenmp', '-fsyntax-only', '-Wall', '-Werror',
                         '-I', os.path.join(ROOT, 'include'), str(out / 'grad2d_host.cpp')])
  # without the switch: no product names the fused kernel or the depth limit
  plain = tmp_path / 'plain'
  r = subprocess.run([sys.executable, SODAC, sample, '--hip-kernel', str(plain) + '.hip',
                      '--hip-host', str(plain) + '.py', '--hip-host-cpp', str(plain) + '.cpp'],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  for suffix in ('.hip', '.py', '.cpp'):
    got = open(str(plain) + suffix).read()
    assert 'fused_k1' not in got.replace('not fused', '') and 'set_max_depth' not in got


def test_fixture_set_is_what_the_script_writes():
  with open(os.path.join(GOLDEN, 'manifest.json')) as f:
    manifest = json.load(f)
  names = sorted(k for k in manifest if k.endswith('.npz'))
  assert sorted(names + ['manifest.json']) == sorted(os.listdir(GOLDEN)) and len(names) == 16
  for app in APPS:
    for dims in (('37x29', '64x48') if app.endswith('2d') else ('20x18x16', '33x9x12')):
      for kind in ('ramp', 'random'):
        assert '%s.iter1.%s.%s.npz' % (app, dims, kind) in manifest
