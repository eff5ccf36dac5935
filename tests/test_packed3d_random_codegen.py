"""The random programs of the packed-cell 3-D kernels (tests/random_programs.py:
narrow_volume_program; tests/test_gpu_packed3d_random.py runs them), without a GPU: what the
committed set covers, counted from each program's lowered spec and from the table generate()
gives it under the keywords the GPU test uses (tests/packed3d_random.py) - so the set cannot
drift into the corner the four samples already sit in (8-byte lanes, unsigned or 16-bit, one
input, + - * / only); every unit compiles for gfx950 without scratch inside the occupancy it
declares; and the fixtures are what tests/golden/make_packed3d_random_golden.py writes."""
import concurrent.futures
import hashlib
import os
import re

import numpy as np
import pytest

from soda_hip.codegen import kernel, kernel_common, kernel_stream3d, kernel_stream3d_pk
from soda_hip.codegen import spec as specmod

from codegen_util import HIPCC, READELF, resource_figures
from codegen_util import spec_of as sample
from conftest import GOLDEN, _cpu_quota
from packed3d_random import (FAMILY, FIXTURES, KEYS, MANIFEST, PROGRAMS, SEAM_MARGIN, fused_of,
                             generated, keywords_of, lane_bytes, spec_of)
from test_packed3d_codegen import waves_of

OPERATOR_GROUPS = {
    '%': r'%',
    'comparison': r'[<>]=?|==|!=',
    '&& or ||': r'&&|\|\|',
    'unary -': r'-(?! )',
    '~': r'~',
    '!': r'!(?!=)',
    '&': r'(?<!&)&(?!&)',
    '|': r'(?<!\|)\|(?!\|)',
    '^': r'\^',
    '/ of a difference': r'\(x - x\) / \d',
    '/ of a product beyond 16 bits': r'\(x \* (?:300|1000|257)\) / \d',
}


def expression_texts(lowered):
  """The stages' expressions with every load as `x` and every cast of a load as `x`."""
  for stage in lowered['stages']:
    for text in [stage['expr']] + [l['expr'] for l in stage['lets']]:
      plain = specmod.LOAD_RE.sub('x', text)
      yield 'static_cast<' in plain, re.sub(r'static_cast<\w+ >\(x\)', 'x', plain)


def features_of(key):
  """What program `key` covers, from its lowered spec and its table - nothing from names."""
  spec = spec_of(key)
  lowered = specmod.inline_pointwise(spec)
  types = specmod.tensor_c_types(lowered)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  text, table = generated(key)
  found = set()
  for end in [t['c_type'] for t in spec['inputs']] + [types[o] for o in spec['outputs']]:
    found.add(('end', end))
  if len(spec['inputs']) == 2:
    found.add('two inputs')
  local_types = [s['c_type'] for s in lowered['stages'] if s['name'] not in spec['outputs']]
  for c_type in local_types:
    if specmod.ELEM_SIZE[c_type] < 4 and specmod.ELEM_SIZE[c_type] != elem:
      found.add('narrow local of another width')
    if c_type in ('int32_t', 'float'):
      found.add('%s local' % c_type)
  for k in fused_of(table):
    found.add(('lane', elem, k['cols'], 'depth %d' % k['depth']))
    if lane_bytes(spec, k) == 16 and k['depth'] == 2:
      found.add('16-byte lanes at depth 2')
    geo = kernel_stream3d_pk.tile_geometry(lowered, k['depth'], k['rows'], k['cols'])
    assert (geo['w_out'], geo['r_out']) == (k['w_out'], k['r_out'])
    for side in ('halo_lo', 'halo_hi'):
      if geo[side] == 0:
        found.add('%s == 0' % side)
    found.add('fill_rows %s' % ('>= 2' if k['fill_rows'] >= 2 else k['fill_rows']))
    if k['depth'] == 2 and local_types:
      found.add('depth 2 over a local')
    insts, _ = kernel_stream3d.pipeline(lowered, k['depth'], k['prefetch'])
    for inst in insts:
      for src, rel, _ in inst.reads:
        assert abs(rel[0]) <= k['cols']
        if abs(rel[0]) == k['cols']:
          found.add('x offset %sC' % '+-'[rel[0] < 0])
        if rel[0] < 0 and specmod.ELEM_SIZE[src.c_type] == 2:
          found.add('16-bit read across lanes from the left')
  for cast, plain in expression_texts(lowered):
    if cast:
      found.add(('operator', 'cast'))
    for group, pattern in OPERATOR_GROUPS.items():
      if re.search(pattern, plain):
        found.add(('operator', group))
  return found


WANTED = (
    [('end', t) for t in ('uint8_t', 'int8_t', 'uint16_t', 'int16_t')] +
    # both lane widths of each element size, each at both depths
    [('lane', elem, cols, 'depth %d' % d)
     for elem, cols in ((1, 8), (1, 16), (2, 4), (2, 8)) for d in (1, 2)] +
    ['16-byte lanes at depth 2', 'two inputs', 'narrow local of another width', 'int32_t local',
     'float local', 'x offset +C', 'x offset -C', '16-bit read across lanes from the left',
     'halo_lo == 0', 'halo_hi == 0', 'fill_rows 0', 'fill_rows 1', 'fill_rows >= 2',
     'depth 2 over a local', ('operator', 'cast')] +
    [('operator', group) for group in OPERATOR_GROUPS])


def test_the_set_is_the_generators_and_about_two_dozen():
  assert 20 <= len(KEYS) <= 28
  for key in KEYS:
    entry = PROGRAMS[key]
    assert set(entry) == {'text', 'dim', 'iterate', 'generate', 'grid'} and entry['dim'] == 3
    assert set(entry['generate']) <= {'cols', 'rows', 'waves_per_eu'}
    spec = spec_of(key)
    assert spec['iterate'] == entry['iterate'] and len(spec['outputs']) == 1
    types = specmod.tensor_c_types(spec)
    ends = [t['c_type'] for t in spec['inputs']] + [types[spec['outputs'][0]]]
    assert len({specmod.ELEM_SIZE[t] for t in ends}) == 1 and len(spec['inputs']) in (1, 2)
    assert specmod.ELEM_SIZE[ends[0]] in (1, 2)
    chain = len(ends) == 2 and ends[0] == ends[1]
    assert 1 <= entry['iterate'] <= (3 if chain else 1)


@pytest.mark.parametrize('key', KEYS)
def test_every_program_is_taken(key):
  """The switch's note is the depth-1 kernel's name - not a refusal -, the table holds that
  kernel and, for an iteration chain whose depth-2 kernel fits two waves per SIMD, that one,
  and both carry the form's marks."""
  spec = spec_of(key)
  text, table = generated(key)
  assert kernel_common.read_meta_from_source(text)['packed_cells'] == '%s_fused_k1' % spec['app_name']
  fused = fused_of(table)
  types = specmod.tensor_c_types(spec)
  chain = len(spec['inputs']) == 1 and spec['inputs'][0]['c_type'] == types[spec['outputs'][0]]
  names = [(k['name'], k['depth']) for k in fused]
  assert names[0] == ('%s_fused_k1' % spec['app_name'], 1)
  assert names[1:] in ([], [('%s_fused_k2' % spec['app_name'], 2)][:chain and spec['iterate'] >= 2])
  assert 'depth 1 not fused: depth 1' not in text        # (the form's refusals name the depth)
  for k in fused:
    assert lane_bytes(spec, k) in (8, 16)
    assert 'typedef unsigned vec_%s __attribute__((ext_vector_type(%d)' % (
        k['name'], lane_bytes(spec, k) // 4) in text
    if 'cols' in keywords_of(key):
      assert k['cols'] == keywords_of(key)['cols']


def test_the_set_covers_what_the_samples_do_not():
  have = {}
  for key in KEYS:
    for f in features_of(key):
      have.setdefault(f, []).append(key)
  missing = [f for f in WANTED if f not in have]
  assert not missing, missing
  for f in WANTED:
    print(f, have[f])


def test_registers_that_cross_lanes_count_in_the_estimate():
  """nv19 - two int16 inputs, a uint8 local, 16-byte lanes -: the local's rows read 8
  registers of the neighbour lane where the lane has 4 dwords, the estimate carries 16 for
  the 4 beyond (two per cell at most), and the kernel is taken at three waves per SIMD, not at
  four, where it spilled (the compile test below holds it to that occupancy).  The four
  samples cross no more than their dwords: their estimates are what they were."""
  key = 'nv19'
  lowered = specmod.inline_pointwise(spec_of(key))
  text, table = generated(key)
  (k,) = fused_of(table)
  assert (k['cols'], lane_bytes(spec_of(key), k)) == (8, 16)
  insts, _ = kernel_stream3d.pipeline(lowered, 1, k['prefetch'])
  assert kernel_stream3d_pk.row_crossings(insts, 8) == 8
  windows = sum(i.keep * 8 * kernel_stream3d_pk.regs_per_row(i.c_type, 8) for i in insts)
  assert kernel_stream3d_pk.overhead_vgprs(8, 8, 4, 8) == kernel_stream3d_pk.overhead_vgprs(8, 8, 4) + 16
  assert k['est_vgprs'] == windows + kernel_stream3d_pk.overhead_vgprs(8, 8, 4, 8) == 132
  assert waves_of(text, k['name']) == 3
  assert kernel_stream3d_pk.overhead_vgprs(8, 4, 2, 15) == kernel_stream3d_pk.overhead_vgprs(8, 4, 2) + 8
  for app, depths in (('smooth3d', (1, 2)), ('skewvol3d', (1,)), ('sdiff3d', (1,)), ('castvol3d', (1,))):
    low = specmod.inline_pointwise(sample(app))
    for depth in depths:
      entry = [e for e in kernel.generate(sample(app), packed_cells=True)[1]
               if e['kind'] == 'fused' and e['depth'] == depth][0]
      insts, _ = kernel_stream3d.pipeline(low, depth, entry['prefetch'])
      dwords = lane_bytes(sample(app), entry) // 4
      assert kernel_stream3d_pk.row_crossings(insts, entry['cols']) <= dwords, (app, depth)


def contains_the_store_point(spec):
  """Every stage's window composed back to the inputs - the hull of its offsets, NOT widened
  to the origin as specmod.iteration_boxes widens it - holds offset 0 on every axis: the
  condition under which the reference's CPU loops stay inside the arrays.  (The first
  iteration decides: sums of hulls that hold 0 hold 0.)"""
  zero = ([0] * spec['dim'], [0] * spec['dim'])
  boxes = {t['name']: zero for t in spec['inputs']}
  for stage in spec['stages']:
    los, his = [], []
    for parent, (wlo, whi) in specmod.stage_windows(spec)[stage['name']].items():
      los.append([a + b for a, b in zip(boxes[parent][0], wlo)])
      his.append([a + b for a, b in zip(boxes[parent][1], whi)])
    boxes[stage['name']] = ([min(v) for v in zip(*los)], [max(v) for v in zip(*his)])
    if any(a > 0 or b < 0 for a, b in zip(*boxes[stage['name']])):
      return False
  return True


def test_fixture_set_is_what_the_script_writes():
  """One fixture per program whose windows all contain the store point - at least five in
  six -, a manifest row that says why for each of the others; names, types, shapes and
  digests as recorded, every file under 200 KB; the grid 40 columns wider than one tile
  stores, with a tile seam and at least one cell inside the output's box."""
  assert len(MANIFEST) == len(KEYS)
  assert sorted(FIXTURES.values()) == sorted(os.listdir(os.path.join(GOLDEN, FAMILY)))
  with_answer = [key for key in KEYS if contains_the_store_point(spec_of(key))]
  assert sorted(FIXTURES) == sorted(with_answer) and 6 * len(with_answer) >= 5 * len(KEYS)
  for key in KEYS:
    if key not in FIXTURES:
      assert MANIFEST['%s.%s' % (FAMILY, key)] == dict(
          key=key, reference_cpu_path='one-sided window: loops leave the arrays')
      continue
    spec = spec_of(key)
    entry, meta = PROGRAMS[key], MANIFEST[FIXTURES[key]]
    dims = entry['grid']
    assert FIXTURES[key] == key + '.npz'
    assert meta['dims'] == dims and meta['iterate'] == entry['iterate'] and meta['key'] == key
    path = os.path.join(GOLDEN, FAMILY, FIXTURES[key])
    assert os.path.getsize(path) < 200 << 10
    data = np.load(path)
    assert sorted(data.files) == sorted(['in_' + t['name'] for t in spec['inputs']] +
                                        ['out_' + n for n in spec['outputs']])
    for t in spec['inputs']:
      a = data['in_' + t['name']]
      assert a.dtype == np.dtype(specmod.NUMPY_NAME[t['c_type']])
      assert a.shape == tuple(reversed(dims))
      # uniform over the whole range of the type: the smallest and the largest of some ten
      # thousand draws lie within a hundredth of the range of its ends, top bits set
      info = np.iinfo(a.dtype)
      assert int(a.min()) - info.min <= (info.max - info.min) // 100 >= info.max - int(a.max())
    types = specmod.tensor_c_types(spec)
    for name in spec['outputs']:
      out = data['out_' + name]
      assert out.dtype == np.dtype(specmod.NUMPY_NAME[types[name]])
      assert hashlib.sha256(out.tobytes()).hexdigest() == meta['sha256'][name], (key, name)
    lowered = specmod.inline_pointwise(spec)
    lo, hi = specmod.iteration_margins(lowered, entry['iterate'])[-1]
    assert all(n - a - b >= 1 for n, a, b in zip(dims, lo, hi)), (key, dims, lo, hi)
    fused = fused_of(generated(key)[1])
    assert dims[0] == max(k['w_out'] for k in fused) + SEAM_MARGIN
    for k in fused:      # the first tile's last stored column lies inside the box
      first_lo = specmod.iteration_margins(lowered, k['depth'])[-1][0][0]
      assert first_lo - first_lo % k['cols'] + k['w_out'] < dims[0] - hi[0], (key, k['name'])


@pytest.fixture(scope='module')
def figures(tmp_path_factory):
  """{program: {kernel: resource figures}}: every unit compiled once, side by side."""
  out = tmp_path_factory.mktemp(FAMILY)

  def compiled(key):
    text, table = generated(key)
    return key, resource_figures(text, [k['name'] for k in fused_of(table)],
                                 str(out / (key + '.hsaco')),
                                 extra_flags=['-Werror=array-bounds'])
  with concurrent.futures.ThreadPoolExecutor(max(1, min(8, _cpu_quota()))) as pool:
    return dict(pool.map(compiled, KEYS))


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(READELF)),
                    reason='needs hipcc and llvm-readelf')
@pytest.mark.parametrize('key', KEYS)
def test_the_unit_compiles_without_scratch_at_its_occupancy(key, figures):
  """With -Werror=array-bounds, from the compiler's resource report: no scratch, no spilled
  VGPR, and no more registers than the waves per SIMD the kernel declares leave each of them
  (512 per SIMD on gfx950) - else overhead_vgprs would have selected it a level too high."""
  text, table = generated(key)
  for k in fused_of(table):
    found = figures[key][k['name']]
    waves = waves_of(text, k['name'])
    print(key, k['name'], 'cols', k['cols'], 'waves', waves, found, 'estimate', k['est_vgprs'])
    assert found['private_segment_fixed_size'] == 0, (k['name'], found)
    assert found['vgpr_spill_count'] == 0, (k['name'], found)
    assert 0 < found['vgpr_count'] <= 512 // waves, (k['name'], found, waves)
    assert found['group_segment_fixed_size'] == 0       # no LDS
