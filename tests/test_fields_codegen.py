"""Fused kernels for iterated programs over several fields (soda_hip/codegen/
kernel_fields2d.py), without a GPU: what the kernel tables hold, that every kernel
compiles for gfx950 without scratch memory, that the checker agrees with the reference's
fixtures on the four samples, that programs outside the class keep today's tables, and
that the per-output extras a launch carries are the boxes' own differences."""
import json
import os
import shutil

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel, kernel_fields2d, kernel_stream2d
from soda_hip.codegen import spec as specmod

from codegen_util import HIPCC, READELF, resource_figures, spec_of, spec_of_text
from conftest import ROOT, SAMPLES

APPS = ('wave2d', 'fdtd2d', 'skewpair2d', 'mixpair2d')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'fields_manifest.json')) as _f:
  MANIFEST = json.load(_f)


@pytest.mark.parametrize('app', APPS)
def test_tables_hold_fused_kernels_deeper_than_one(app):
  spec = spec_of(app)
  assert kernel_stream2d.multi_field(spec)
  text, table = kernel.generate(spec)
  fused = {k['depth']: k for k in table if k['kind'] == 'fused'}
  assert {1, 2, 4} <= set(fused), sorted(fused)
  assert set(fused) <= {1, 2, 4, 8}
  for depth, k in fused.items():
    assert depth <= spec['iterate'] and k['fields'] == len(spec['outputs'])
    assert k['fill_rows'] > 0 and k['step_bytes'] > 0 and k['step_valu'] > 0
  # the per-stage kernels stay: max_depth < 0 and arrays the fused ones refuse use them
  assert sum(k['kind'] == 'stage' for k in table) == len(spec['stages'])
  assert kernel.fused_depths(spec, kernel.DEFAULT_MAX_DEPTH) == [
      d for d in (1, 2, 4, 8) if d <= spec['iterate']]


def test_a_depth_over_the_register_budget_lands_in_the_notes():
  text, table = kernel.generate(spec_of('wave2d'))
  assert 8 not in [k['depth'] for k in table if k['kind'] == 'fused']
  assert '// depth 8 not fused: depth 8 would need about' in text


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('app', APPS)
def test_kernels_compile_for_gfx950_without_scratch(app, tmp_path):
  """Every fused entry: no private segment (scratch) and no spill counts, neither of
  VGPRs nor of SGPRs (the allocator parks those in VGPR lanes, inside the row loop)."""
  text, table = kernel.generate(spec_of(app))
  fused = [k['name'] for k in table if k['kind'] == 'fused']
  assert fused
  found = resource_figures(text, fused, str(tmp_path / (app + '.hsaco')))
  for kname, figures in found.items():
    assert figures['private_segment_fixed_size'] == 0, (kname, figures)
    assert figures['vgpr_spill_count'] == 0, (kname, figures)
    assert figures['sgpr_spill_count'] == 0, (kname, figures)
    assert 0 < figures['vgpr_count'] <= 256, (kname, figures)


FIXTURES = sorted(k for k in MANIFEST if k.endswith('.npz'))


def test_fixture_set_is_what_the_script_writes():
  assert len(FIXTURES) == 4 * 4 * 2 * 2
  for app in APPS:
    for it in (1, 2, 3, 4):
      for dims in ('37x29', '64x48'):
        for kind in ('ramp', 'random'):
          assert '%s.iter%d.%s.%s.npz' % (app, it, dims, kind) in MANIFEST


@pytest.mark.skipif(shutil.which('g++') is None, reason='the oracle needs g++')
@pytest.mark.parametrize('app', APPS)
def test_oracle_equals_the_reference_fixtures(app):
  """Array for array: the oracle's values on each output's own box, and the reference's
  zeros outside it (the oracle's ping-pong arrays keep earlier levels there)."""
  from oracle import soda_oracle
  spec = spec_of(app)
  orc = soda_oracle.Oracle(spec)
  for fx in FIXTURES:
    meta = MANIFEST[fx]
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, 'fields', fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    got = orc.run(inputs, iterate=meta['iterate'])
    boxes = specmod.iteration_boxes(spec, meta['iterate'])[-1]
    for name in spec['outputs']:
      want = data['out_' + name]
      assert got[name].dtype == want.dtype
      lo, hi = boxes[name]
      sl = tuple(slice(-lo[d], max(-lo[d], meta['dims'][d] - hi[d])) for d in (1, 0))
      clean = np.zeros_like(got[name])
      clean[sl] = got[name][sl]
      assert clean[sl].size > 0
      assert np.array_equal(clean.view(np.uint8), want.view(np.uint8)), (fx, name)


TWO_OUT = '''
kernel: two_out
burst width: 512
unroll factor: 1
iterate: 1
input float: a(64, *)
output float: sx(0, 0) = a(0, 0) + a(1, 0)
output float: sy(0, 0) = a(0, 0) - a(0, 3)
'''
TWO_IN = '''
kernel: two_in
burst width: 512
unroll factor: 1
iterate: 1
input float: f
input float: u(32, *)
output float: o(0, 0) = u(0, 0) + u(1, 0) * f(0, -1)
'''
MIXED_TYPES = '''
kernel: mixed
burst width: 512
unroll factor: 1
iterate: 1
input float: f
input int32: u(32, *)
output int32: fo(0, 0) = u(0, 0) + u(1, 0)
output float: uo(0, 0) = f(0, 0) * 0.5f
'''


def test_programs_outside_the_class_keep_their_tables():
  _, table = kernel.generate(spec_of_text(TWO_OUT))
  assert [k['kind'] for k in table] == ['stage', 'stage']
  _, table = kernel.generate(spec_of_text(TWO_IN))
  assert [(k['kind'], k['depth']) for k in table] == [('stage', 0), ('fused', 1)]
  assert 'fields' not in table[-1]
  # as many outputs as inputs, but output j is not of input j's type: not iterable
  spec = spec_of_text(MIXED_TYPES)
  assert not kernel_stream2d.multi_field(spec)
  _, table = kernel.generate(spec)
  assert all(k['kind'] == 'stage' for k in table)
  assert kernel.fused_depths(spec, 12) == [1]


def test_more_outputs_than_the_launch_arguments_carry_stay_per_stage():
  n = kernel_fields2d.MAX_OUTPUTS + 1
  lines = ['kernel: seven', 'burst width: 512', 'unroll factor: 1', 'iterate: 4']
  lines += ['input float: f%d%s' % (j, '(32, *)' if j == n - 1 else '') for j in range(n)]
  lines += ['output float: o%d(0, 0) = f%d(0, 0) + f%d(1, 0)' % (j, j, (j + 1) % n)
            for j in range(n)]
  spec = spec_of_text('\n'.join(lines) + '\n')
  assert kernel_stream2d.multi_field(spec)
  _, table = kernel.generate(spec)
  assert all(k['kind'] == 'stage' for k in table)
  assert kernel.fused_depths(spec, 12) == [1]


def test_extras_of_skewpair2d_are_the_boxes_own_differences():
  spec = spec_of('skewpair2d')
  seen = set()
  for done in range(7):
    for depth in (1, 2, 4):
      boxes = specmod.iteration_boxes(spec, done + depth)[-1]
      hull_lo = [max(-boxes[o][0][d] for o in spec['outputs']) for d in range(2)]
      hull_hi = [max(boxes[o][1][d] for o in spec['outputs']) for d in range(2)]
      extras = kernel_fields2d.output_extras(spec, done, depth)
      assert len(extras) == 2
      for name, ex in zip(spec['outputs'], extras):
        lo, hi = boxes[name]
        # the launch's box widened by the extras IS the output's own box
        assert [hull_lo[d] - ex[d] for d in range(2)] == [-v for v in lo]
        assert [hull_hi[d] - ex[2 + d] for d in range(2)] == list(hi)
        assert all(0 <= v <= kernel_fields2d.MAX_EXTRA for v in ex)
        seen.add(ex)
      words = kernel_fields2d.pack_extras(extras)
      for j, ex in enumerate(extras):
        word = words[j // 2] >> (32 * (j % 2))
        assert tuple((word >> (8 * i)) & 255 for i in range(4)) == ex
  # they change along a sweep and differ between the low and the high side
  assert len(seen) > 2 and any(ex[0] != ex[2] or ex[1] != ex[3] for ex in seen)


def test_single_field_pipeline_is_untouched_by_the_fields_switch():
  spec = specmod.spec_from_stencil(frontend.load(os.path.join(SAMPLES, 'jacobi2d.soda')))
  insts, final = kernel_stream2d.build_pipeline(spec, 2, 3)
  assert [i.final for i in insts].count(True) == 1 and final.final
  with pytest.raises(kernel_stream2d.NotFusable):
    kernel_stream2d.build_pipeline(spec_of('wave2d'), 2, 3)
  insts, _ = kernel_stream2d.build_pipeline(spec_of('wave2d'), 2, 3, fields=True)
  assert sorted(i.tensor for i in insts if i.final) == ['uc', 'un']
