"""Fused 3-D kernels for iterated programs over several fields (soda_hip/codegen/
kernel_fields3d.py), without a GPU: what the kernel tables hold, that every kernel compiles
for gfx950 without scratch memory or spills, that programs outside the form keep their
stage kernels with a note, that the checker agrees with the reference's fixtures, and that
the launch planner packs each output's own box into the launch arguments."""
import json
import os
import shutil

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel, kernel_fields3d, kernel_stream2d, kernel_stream3d
from soda_hip.codegen import spec as specmod

import test_schedule as ts
from codegen_util import HIPCC, READELF, resource_figures, spec_of, spec_of_text
from conftest import ROOT, SAMPLES
from test_schedule import probe      # noqa: F401  (the planner probe, built once)

APPS = ('wave3d', 'maxwell3d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'fields3d_manifest.json')) as _f:
  MANIFEST = json.load(_f)


@pytest.mark.parametrize('app', APPS)
def test_tables_hold_fused_kernels(app):
  spec = spec_of(app)
  assert spec['dim'] == 3 and kernel_stream2d.multi_field(spec)
  text, table = kernel.generate(spec)
  names = [k['name'] for k in table]
  assert '%s_fused_k1' % app in names and '%s_fused_k2' % app in names, names
  fused = {k['depth']: k for k in table if k['kind'] == 'fused'}
  assert set(fused) == {1, 2}
  for depth, k in fused.items():
    assert k['fields'] == len(spec['outputs']) and k['est_vgprs'] <= 250
    geo = kernel_fields3d.tile_geometry(spec, depth, k['rows'], k['cols'])
    assert (k['w_out'], k['r_out']) == (geo['w_out'], geo['r_out'])
    assert k['tile'][:2] == [4 * k['w_out'], k['r_out']] and k['origin_align'] == k['cols']
    assert k['fill_rows'] > 0 and k['step_bytes'] > 0 and k['step_valu'] > 0
    # the first shape, by how much of the tile survives the halo, that fits the budget
    lowered = specmod.inline_pointwise(spec)
    for rows, cols in kernel_fields3d.shapes_by_kept_fraction(lowered, depth):
      if (rows, cols) == (k['rows'], k['cols']):
        break
      with pytest.raises(kernel_stream2d.NotFusable, match='would need about'):
        kernel_fields3d.emit(lowered, depth, rows=rows, cols=cols)
  assert 'not fused' not in text
  # the per-stage kernels stay: they are the default schedule and what max_depth < 0 runs
  assert sum(k['kind'] == 'stage' for k in table) == len(
      specmod.inline_pointwise(spec)['stages'])
  # no kernel deeper than the program iterates
  _, table = kernel.generate(spec_of(app, iterate=1))
  assert [k['depth'] for k in table if k['kind'] == 'fused'] == [1]


def test_planes_kept_are_those_of_the_windows():
  """prefetch 0: wave3d keeps 5 planes at depth 1 and 11 at depth 2, maxwell3d 7 and 14."""
  for app, planes in (('wave3d', (5, 11)), ('maxwell3d', (7, 14))):
    spec = specmod.inline_pointwise(spec_of(app))
    for depth, want in zip((1, 2), planes):
      insts, _ = kernel_stream3d.pipeline(spec, depth, 0, fields=True)
      kernel_stream2d.rotation_period(insts, 12)
      assert sum(i.keep for i in insts) == want, (app, depth)
      assert sorted(i.tensor for i in insts if i.final) == sorted(spec['outputs'])
  # (16, 2) fits wave3d at depth 1 at about 216 registers; depth 2 does not
  _, k = kernel_fields3d.emit(specmod.inline_pointwise(spec_of('wave3d')), 1, rows=16, cols=2)
  assert k['est_vgprs'] == 6 * 32 + 24
  with pytest.raises(kernel_stream2d.NotFusable, match='would need about 408 VGPRs'):
    kernel_fields3d.emit(specmod.inline_pointwise(spec_of('wave3d')), 2, rows=16, cols=2)


def test_single_output_pipeline_is_untouched_by_the_fields_switch():
  spec = specmod.spec_from_stencil(frontend.load(os.path.join(SAMPLES, 'jacobi3d.soda')))
  insts, final = kernel_stream3d.pipeline(spec, 2, 0)
  assert [i.final for i in insts].count(True) == 1 and final.final
  with pytest.raises(kernel_stream2d.NotFusable):
    kernel_stream3d.pipeline(spec_of('wave3d'), 2, 0)


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', APPS)
def test_kernels_compile_for_gfx950_without_scratch(app, tmp_path):
  """Every fused entry: no private segment (scratch) and no spill counts, neither of
  VGPRs nor of SGPRs."""
  text, table = kernel.generate(spec_of(app))
  fused = [k['name'] for k in table if k['kind'] == 'fused']
  assert len(fused) == 2
  found = resource_figures(text, fused, str(tmp_path / (app + '.hsaco')))
  for kname, figures in found.items():
    assert figures['private_segment_fixed_size'] == 0, (kname, figures)
    assert figures['vgpr_spill_count'] == 0, (kname, figures)
    assert figures['sgpr_spill_count'] == 0, (kname, figures)
    assert 0 < figures['vgpr_count'] <= 256, (kname, figures)


_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: 4\n'
FOUR_OUT = _HEAD % 'four' + ''.join(
    'input float: f%d%s\n' % (j, '(32, 32, *)' if j == 3 else '') for j in range(4)) + ''.join(
        'output float: o%d(0, 0, 0) = f%d(0, 0, 0) + f%d(1, 0, 0)\n' % (j, j, (j + 1) % 4)
        for j in range(4))
MIXED_WIDTHS = _HEAD % 'mixedw' + '''input float: a
input double: b(32, 32, *)
output float: an(0, 0, 0) = a(0, 0, 0) + a(0, 1, 0)
output double: bn(0, 0, 0) = b(0, 0, 0) + b(0, 0, 1)
'''
TWO_BYTES = _HEAD % 'shorts' + '''input uint16: a
input uint16: b(32, 32, *)
output uint16: an(0, 0, 0) = a(0, 0, 0) * 3 + b(-1, 0, 0)
output uint16: bn(0, 0, 0) = b(0, 0, 0) * 5 - a(0, 0, 1)
'''
DOUBLES = _HEAD % 'doubles' + '''input double: a
input double: b(32, 32, *)
output double: an(0, 0, 0) = a(0, 0, 0) + 0.5 * b(0, 1, 0)
output double: bn(0, 0, 0) = b(0, 0, 0) - 0.5 * a(0, 0, -1)
'''


@pytest.mark.parametrize('text,note', [
    (FOUR_OUT, '4 outputs: the launch arguments carry the boxes of 3'),
    (MIXED_WIDTHS, 'fields of different widths'),
    (TWO_BYTES, 'fields3d handles 4- and 8-byte elements')])
def test_programs_outside_the_form_get_a_note_and_stage_kernels(text, note):
  spec = spec_of_text(text)
  assert kernel_stream2d.multi_field(spec)
  out, table = kernel.generate(spec)
  assert [k['kind'] for k in table] == ['stage'] * len(spec['stages'])
  assert '// depth 1 not fused: %s' % note in out


def test_eight_byte_fields_are_inside_the_form():
  _, table = kernel.generate(spec_of_text(DOUBLES))
  assert [k['depth'] for k in table if k['kind'] == 'fused'] == [1, 2]


def test_a_shape_nothing_fits_is_refused_with_the_register_figure():
  text, table = kernel.generate(spec_of('maxwell3d'), vgpr_budget=64)
  assert all(k['kind'] == 'stage' for k in table)
  assert '// depth 1 not fused: depth 1 would need about' in text


def test_extras_are_the_boxes_own_differences():
  spec = spec_of('maxwell3d')
  seen = set()
  for done in range(5):
    for depth in (1, 2):
      boxes = specmod.iteration_boxes(spec, done + depth)[-1]
      hull_lo, hull_hi = ts.hull(spec, boxes)
      extras = kernel_fields3d.output_extras(spec, done, depth)
      assert len(extras) == 3
      for name, ex in zip(spec['outputs'], extras):
        lo, hi = boxes[name]
        assert [hull_lo[d] - ex[d] for d in range(3)] == [-v for v in lo]
        assert [hull_hi[d] - ex[3 + d] for d in range(3)] == list(hi)
        seen.add(ex)
      words = kernel_fields3d.pack_extras(extras)
      for j, ex in enumerate(extras):
        assert tuple((words[j] >> (8 * i)) & 255 for i in range(6)) == ex
  # the boxes differ in every dimension, z included
  for d in range(3):
    assert any(ex[d] or ex[3 + d] for ex in seen), d


FIXTURES = sorted(k for k in MANIFEST if k.endswith('.npz'))


def test_fixture_set_is_what_the_script_writes():
  assert len(FIXTURES) == 2 * 3 * 2 * 2
  for app in APPS:
    for it in (1, 2, 3):
      for dims in ('20x18x16', '33x9x12'):
        for kind in ('ramp', 'random'):
          fx = '%s.iter%d.%s.%s.npz' % (app, it, dims, kind)
          assert fx in MANIFEST
          assert os.path.getsize(os.path.join(GOLDEN, 'fields3d', fx)) < 1 << 20


@pytest.mark.skipif(shutil.which('g++') is None, reason='the oracle needs g++')
@pytest.mark.parametrize('app', APPS)
def test_oracle_equals_the_reference_fixtures(app):
  """Array for array: the oracle's values on each output's own box, and the reference's
  zeros outside it."""
  from oracle import soda_oracle
  spec = spec_of(app)
  orc = soda_oracle.Oracle(spec)
  for fx in FIXTURES:
    meta = MANIFEST[fx]
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'fields3d', fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    got = orc.run(inputs, iterate=meta['iterate'])
    boxes = specmod.iteration_boxes(spec, meta['iterate'])[-1]
    for name in spec['outputs']:
      want = data['out_' + name]
      lo, hi = boxes[name]
      sl = tuple(slice(-lo[d], max(-lo[d], meta['dims'][d] - hi[d])) for d in (2, 1, 0))
      clean = np.zeros_like(got[name])
      clean[sl] = got[name][sl]
      assert clean[sl].size > 0
      assert np.array_equal(clean.view(np.uint8), want.view(np.uint8)), (fx, name)


# ---- the launch planner (csrc/schedule.cpp) on these programs ------------------------------

def extras3d_of(launch, j):
  word = launch['param'][1 + j] & (2 ** 64 - 1)
  return [(word >> (8 * i)) & 0xff for i in range(6)]


@pytest.mark.parametrize('app', APPS)
def test_planner_packs_every_outputs_box(probe, tmp_path, app):      # noqa: F811
  """64^3 and a ragged grid, iterate 1, 2, 3 and 5: under a depth limit every launch is
  fused and its unpacked extras reproduce each output's box of spec.iteration_boxes; the
  widened box lies inside the array and the grid covers it; without a limit the plan is
  per stage."""
  cases = [ts.case(dims, iterate, max_depth)
           for dims in ((64, 64, 64), (37, 45, 203)) for iterate in (1, 2, 3, 5)
           for max_depth in (0, 1, 2)]
  cases += [ts.case((64, 64, 64), 3, 0, (1, 2)), ts.case((64, 64, 64), 5, 0, (2, 2, 1))]
  n_fused = 0
  for iterate in (1, 2, 3, 5):
    spec, table = ts.program(app, iterate)
    group = [c for c in ts.variants(cases) if c['iterate'] == iterate]
    for w, static in ((1, 0), (2, 64 * 1024)):
      for c, r in ts.plan(probe, tmp_path, app, iterate, group, w, static):
        assert r['rc'] == 0, (c, r['error'])
        ts.check_depths_and_boxes(spec, table, c, r)
        ts.check_routing(spec, table, c, r)
        kinds = {table[l['kernel']]['kind'] for l in r['launches']}
        if c['max_depth'] == 0 and not c['split']:
          assert kinds == {'stage'}        # not in the default schedule until measured
          continue
        assert kinds == {'fused'}
        if c['split']:
          assert [table[l['kernel']]['depth'] for l in r['launches']] == list(c['split'])
        levels = specmod.iteration_boxes(spec, iterate)
        done = 0
        for l in r['launches']:
          k = table[l['kernel']]
          done += k['depth']
          n_fused += 1
          lo, hi = list(l['lo']), list(l['hi'])
          extras = [extras3d_of(l, j) for j in range(len(spec['outputs']))]
          for o, ex in zip(spec['outputs'], extras):
            olo, ohi = levels[done - 1][o]
            for d in range(3):    # unpacked, the output's own box: inside the array too
              assert l['lo'][d] - ex[d] == c['valid_lo'][d] - olo[d] >= 0
              assert l['hi'][d] + ex[3 + d] == c['dims'][d] - c['valid_hi'][d] - ohi[d] \
                  <= c['dims'][d]
          for j in range(len(spec['outputs']), 3):
            assert l['param'][1 + j] == 0
          for d in range(3):      # the grid covers the union of the outputs' boxes
            lo[d] -= max(e[d] for e in extras)
            hi[d] += max(e[3 + d] for e in extras)
            assert 0 <= lo[d] < hi[d] <= c['dims'][d]
          ext = [hi[d] - lo[d] for d in range(3)]
          assert l['grid'][0] == ts.ceil_div(ext[0] + lo[0] % k['origin_align'], k['tile'][0])
          assert l['grid'][1] == ts.ceil_div(ext[1], k['tile'][1])
          chunk, chunks = l['param'][0], l['grid'][2]
          assert chunk >= 1 and chunk * chunks >= ext[2] > chunk * (chunks - 1)
          assert l['lds'] == 0 and l['est_us'] > 0
  assert n_fused > 100
