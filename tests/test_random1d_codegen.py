"""The random programs of the fused 1-D kernels (tests/random_programs.py: line_program;
tests/test_gpu_random1d.py runs them), without a GPU: the committed set is the generator's;
every program is taken by kernel_stream1d under the keywords the GPU test uses
(tests/random1d.py); what the set covers is counted from each program's spec and table - so it
cannot drift back into the corner the samples sit in (one stage, `+ - *` on floats, 16-byte
lanes, far reads of the input only); the fixtures are what
tests/golden/make_random1d_golden.py writes; the operands of the GPU test's full-width runs
are admissible - finite, and the same bytes from the oracle at -O0 and at -O2; and every unit
compiles for gfx950 without scratch."""
import concurrent.futures
import hashlib
import os
import re

import numpy as np
import pytest

from soda_hip.codegen import kernel, kernel_common, kernel_stream1d, kernel_stream2d
from soda_hip.codegen import spec as specmod

import gpu_util
import random_programs
import test_gpu_memory_contract as contract
from codegen_util import HIPCC, READELF, resource_figures, without_meta
from conftest import GOLDEN, _cpu_quota
from random1d import (FAMILY, FIXTURES, KEYS, MANIFEST, MAX_CELLS, PROGRAMS, SEAM_MARGIN,
                      edge_of, fused_of, generated, hops_of, keywords_of, lane_class, lengths,
                      margin_of, reads_far_local, refused_depths, spec_of, wide_lengths,
                      wide_seed)
from test_packed3d_random_codegen import (OPERATOR_GROUPS, contains_the_store_point,
                                          expression_texts)

FLOATS = ('float', 'double')


def is_far(key):
  return bool(keywords_of(key).get('far_taps'))


def local_types(spec):
  return [s['c_type'] for s in spec['stages'] if s['name'] not in spec['outputs']]


def test_the_set_is_the_generators():
  """The JSON is what line_set() writes - texts, iteration counts, keywords, and the length
  from the table -, some 32 programs of the class the issue of this set names."""
  assert random_programs.LINE_MAX_HOPS == kernel_stream1d.MAX_HOPS_1D
  written = {key: dict(text=text, dim=dim, iterate=iterate, generate=keywords)
             for key, text, dim, iterate, keywords in random_programs.line_set()}
  assert sorted(written) == sorted(PROGRAMS) and 28 <= len(KEYS) <= 40
  deep, near, far_local = [], [], []
  for i, key in enumerate(KEYS):
    entry = dict(PROGRAMS[key])
    (length,) = entry.pop('grid')
    assert entry == written[key], key
    assert set(entry['generate']) <= {'far_taps', 'segs'} and entry['dim'] == 1
    spec = spec_of(key)
    seed = int(key[2:])
    types = specmod.tensor_c_types(spec)
    (source,), (out,) = spec['inputs'], spec['outputs']
    assert source['c_type'] == types[out] == specmod.native_type(
        random_programs.LINE_ENDS[seed % 7])
    assert spec['iterate'] == entry['iterate'] and len(local_types(spec)) <= 2
    assert len({specmod.ELEM_SIZE[t] for t in types.values()}) == 1
    fused = fused_of(generated(key)[1])
    assert length == max(k['w_out'] for k in fused) + margin_of(spec, entry['iterate']) + \
        SEAM_MARGIN
    offsets = [rel[0] for stage in spec['stages'] for _, rel in stage['loads']]
    if seed % 8 == 7:
      assert max(offsets) < 0, key
    else:       # every stage reads the store point of a parent
      assert all(any(rel[0] == 0 for _, rel in stage['loads']) for stage in spec['stages']), key
    assert 1 <= entry['iterate'] <= 13
    if entry['iterate'] >= 8:
      deep.append(key)
    else:
      assert entry['iterate'] <= 5
    assert is_far(key) == (max(hops_of(key)) >= 2), key
    assert max(hops_of(key)) <= kernel_stream1d.MAX_HOPS_1D
    if not is_far(key):
      near.append(key)
    elif reads_far_local(key):
      far_local.append(key)
  assert 3 <= len(deep) <= 4
  assert len(KEYS) // 4 <= len(near) <= len(KEYS) // 2          # about a third
  assert 2 * len(far_local) >= len(KEYS) - len(near)
  # no stage is dead
  for key in KEYS:
    spec = spec_of(key)
    read = {name for stage in spec['stages'] for name, _ in stage['loads']}
    assert read == {t['name'] for t in spec['inputs']} | {
        s['name'] for s in spec['stages'] if s['name'] not in spec['outputs']}, key


@pytest.mark.parametrize('key', KEYS)
def test_every_program_is_taken(key):
  spec = spec_of(key)
  lowered = specmod.inline_pointwise(spec)
  text, table = generated(key)
  fused = fused_of(table)
  name = '%s_fused_k1' % spec['app_name']
  assert (fused[0]['name'], fused[0]['depth']) == (name, 1)
  assert all(contract.FAMILY['stream'](k) and k['fill_rows'] == 0 for k in fused)
  cols = kernel.default_cols(spec)
  assert all(k['cols'] == cols for k in fused)
  assert all(k['segs'] == keywords_of(key).get('segs', kernel_stream1d.DEFAULT_SEGS)
             for k in fused)
  note = kernel_common.read_meta_from_source(text).get('far_taps')
  if is_far(key):
    assert note == name
    assert all(max(k['halo']) > k['cols'] for k in fused)
    plain = kernel.generate(spec, **dict(keywords_of(key), far_taps=False))[1]
    assert all(k['kind'] == 'stage' for k in plain)         # refused without the switch
  else:
    assert note is None
    with_switch, same = kernel.generate(spec, **dict(keywords_of(key), far_taps=True))
    assert same == table and without_meta(with_switch) == without_meta(text)
  # the family's depths up to `iterate`, less those that leave a segment no cell to store -
  # each of them with its note
  want = []
  for depth in kernel.STREAM1D_DEPTHS:
    if depth > spec['iterate']:
      continue
    try:
      geo = kernel_stream1d.geometry(lowered, depth, cols)
      want.append(depth)
      k = fused[len(want) - 1]
      assert (k['depth'], k['w_out'], k['halo']) == (
          depth, geo['w_out'], [geo['halo_lo'], geo['halo_hi']]), (key, depth)
    except kernel_stream2d.NotFusable as refusal:
      assert 'leaves no output cells' in str(refusal)
      assert '// depth %d not fused: %s' % (depth, refusal) in text, (key, depth)
  assert [k['depth'] for k in fused] == want
  assert refused_depths(key) == [d for d in kernel.STREAM1D_DEPTHS
                                 if d <= spec['iterate'] and d not in want]


def features_of(key):
  """What program `key` covers, from its lowered spec and its table - nothing from names."""
  spec = spec_of(key)
  lowered = specmod.inline_pointwise(spec)
  elem, lane = lane_class(key)
  fused = fused_of(generated(key)[1])
  cols = fused[0]['cols']
  found = {('end', spec['inputs'][0]['c_type']), ('lane', elem, lane)}
  if cols == 1:
    found.add('one cell per lane')
  lo, hi = hops_of(key)
  hops = max(lo, hi)
  found.add('hops %s' % (hops if hops <= 4 else '5 to 7' if hops < 8 else 8))
  if (lo, hi) == (8, 8):
    found.add('8 lanes on either side')
  inputs = {t['name'] for t in spec['inputs']}
  for stage in lowered['stages']:
    for name, rel in stage['loads']:
      if hops >= 2 and abs(rel[0]) == hops * cols:
        found.add('offset %shops C' % '+-'[rel[0] < 0])
      if hops >= 2 and abs(rel[0]) == (hops - 1) * cols + 1:
        found.add('offset %s((hops - 1) C + 1)' % '+-'[rel[0] < 0])
      if name not in inputs and abs(rel[0]) > cols:
        found.add('far read of a local')
        if specmod.tensor_c_types(lowered)[name] != spec['inputs'][0]['c_type']:
          found.add('far read of a local of another type')
      if elem == 2 and abs(rel[0]) in (2, 3):
        found.add('16-bit read around the dword')
  for c_type in local_types(lowered):
    if c_type != spec['inputs'][0]['c_type']:
      found.add(('local of the other type', elem))
  found.add({None: 'two-sided box', 'first': 'head box', 'last': 'tail box'}[edge_of(spec)])
  for k in fused:
    if k['depth'] in (8, 12):
      found.add('depth %d' % k['depth'])
    for side, halo in zip(('halo_lo', 'halo_hi'), k['halo']):
      if halo == 0:
        found.add('%s == 0' % side)
    if k['segs'] != kernel_stream1d.DEFAULT_SEGS:
      found.add('segs %d' % k['segs'])
  refused = refused_depths(key)
  if refused:
    found.add('a refused depth')
    if is_far(key):
      found.add('a refused depth in a far program')
    if len(refused) >= 2:
      found.add('two refused depths')
  for cast, plain in expression_texts(lowered):
    if cast:
      found.add(('operator', 'cast'))
    for group, pattern in OPERATOR_GROUPS.items():
      if re.search(pattern, plain):
        found.add(('operator', group))
  return found


WANTED = (
    [('end', t) for t in ('uint16_t', 'int16_t', 'int32_t', 'uint32_t', 'float', 'int64_t',
                          'double')] +
    # each element size at each lane width it can have
    [('lane', elem, lane) for elem, lanes in sorted(random_programs.LINE_LANES.items())
     for lane in lanes] +
    ['one cell per lane', 'hops 1', 'hops 2', 'hops 3', 'hops 4', 'hops 5 to 7', 'hops 8',
     '8 lanes on either side', 'offset +hops C', 'offset -hops C',
     'offset +((hops - 1) C + 1)', 'offset -((hops - 1) C + 1)', '16-bit read around the dword',
     'far read of a local', 'far read of a local of another type'] +
    [('local of the other type', elem) for elem in (2, 4, 8)] +
    ['head box', 'tail box', 'two-sided box', 'depth 8', 'depth 12', 'a refused depth',
     'a refused depth in a far program', 'two refused depths', 'halo_lo == 0', 'halo_hi == 0',
     'segs 2', 'segs 8', ('operator', 'cast')] +
    [('operator', group) for group in OPERATOR_GROUPS])


def test_the_set_covers_what_the_samples_do_not():
  have = {}
  for key in KEYS:
    for f in features_of(key):
      have.setdefault(f, []).append(key)
  missing = [f for f in WANTED if f not in have]
  assert not missing, missing
  for f in WANTED:
    print(f, have[f])


def test_fixture_set_is_what_the_script_writes():
  """One fixture per program whose windows all contain the store point - at least five in
  six -, a manifest row that says why for each of the others; names, types, lengths and
  digests as recorded; 16-bit inputs over the whole range of the type, wider integers within
  +-2^20, floats of both signs; the output varies over its box; and the first segment's last
  stored cell of every kernel of the table lies inside the box."""
  assert len(MANIFEST) == len(KEYS)
  assert sorted(FIXTURES.values()) == sorted(os.listdir(os.path.join(GOLDEN, FAMILY)))
  with_answer = [key for key in KEYS if contains_the_store_point(spec_of(key))]
  assert sorted(FIXTURES) == sorted(with_answer) and 6 * len(with_answer) >= 5 * len(KEYS)
  for key in KEYS:
    if key not in FIXTURES:
      assert int(key[2:]) % 8 == 7
      assert MANIFEST['%s.%s' % (FAMILY, key)] == dict(
          key=key, reference_cpu_path='one-sided window: loops leave the arrays')
      continue
    spec = spec_of(key)
    entry, meta = PROGRAMS[key], MANIFEST[FIXTURES[key]]
    (n,) = entry['grid']
    assert FIXTURES[key] == key + '.npz'
    assert meta['dims'] == [n] and meta['iterate'] == entry['iterate'] and meta['key'] == key
    path = os.path.join(GOLDEN, FAMILY, FIXTURES[key])
    assert os.path.getsize(path) < 16 << 10
    data = np.load(path)
    (source,), (name,) = spec['inputs'], spec['outputs']
    assert sorted(data.files) == sorted(['in_' + source['name'], 'out_' + name])
    a, out = data['in_' + source['name']], data['out_' + name]
    dtype = np.dtype(specmod.NUMPY_NAME[source['c_type']])
    assert a.dtype == out.dtype == dtype and a.shape == out.shape == (n,)
    if dtype.kind == 'f':
      assert a.min() < -1 and a.max() > 1 and np.isfinite(out).all()
    elif dtype.itemsize == 2:
      info = np.iinfo(dtype)
      assert int(a.min()) - info.min <= (info.max - info.min) // 50 >= info.max - int(a.max())
    else:
      assert int(np.abs(a.astype(np.int64)).max()) <= 1 << 20 < 2 * int(a.max())
      assert dtype.kind == 'u' or int(a.min()) < -(1 << 19)
    assert hashlib.sha256(out.tobytes()).hexdigest() == meta['sha256'][name], key
    lowered = specmod.inline_pointwise(spec)
    lo, hi = specmod.iteration_margins(lowered, entry['iterate'])[-1]
    assert lo[0] + hi[0] == margin_of(spec, entry['iterate'])
    box = out[lo[0]:n - hi[0]]
    assert box.size >= SEAM_MARGIN and len(np.unique(box)) > box.size // 2, key
    assert not out[:lo[0]].any() and not out[n - hi[0]:].any()
    for k in fused_of(generated(key)[1]):
      # the launch of all iterations' first launch: its first segment starts on the box's
      # first cell rounded down to the lane
      first_lo = specmod.iteration_margins(lowered, k['depth'])[-1][0][0]
      assert first_lo - first_lo % k['cols'] + k['w_out'] < n - hi[0], (key, k['name'])


@pytest.fixture(scope='module')
def oracles():
  """{program: (the -fwrapv oracle at -O2, at -O0)}, built side by side."""
  def built(key):
    spec = spec_of(key)
    return key, (gpu_util.make_wrap_oracle(spec), gpu_util.make_wrap_oracle(spec, opt='-O0'))
  with concurrent.futures.ThreadPoolExecutor(max(1, min(8, _cpu_quota()))) as pool:
    return dict(pool.map(built, KEYS))


@pytest.mark.parametrize('key', KEYS)
def test_the_inputs_of_the_gpu_test_are_admissible(key, oracles):
  """Part (c) of the GPU test on the CPU, with the oracle alone: gpu_util.wide_inputs at the
  default span of exponents, the lengths and seeds random1d gives, every depth of the table
  alone.  The box is not empty, the oracles at -O0 and at -O2 agree byte for byte - no
  float leaves the range of the integer it is converted to, which the two would not agree
  on -, and a float program's values on the box are finite.  Parts (b), (d) and (e) draw
  gpu_util.random_inputs, floats in [0, 1) and integers from 0: their lengths stay within
  MAX_CELLS."""
  spec = spec_of(key)
  (name,) = spec['outputs']
  wrap, plain = oracles[key]
  floaty = spec['inputs'][0]['c_type'] in FLOATS
  for k in fused_of(generated(key)[1]):
    iterate = k['depth']
    m = margin_of(spec, iterate)
    assert max(lengths(k, m)) <= MAX_CELLS and min(lengths(k, m)) == m + 1, (key, k['name'])
    assert max(lengths(k, margin_of(spec, spec['iterate']))) <= MAX_CELLS
    for n in wide_lengths(k, m):
      inputs = gpu_util.wide_inputs(spec, (n,), seed=wide_seed(key, n))
      want = wrap.run(inputs, iterate=iterate)[name]
      lo, hi = contract.box_of(spec, name, (n,), iterate)
      box = want[lo[0]:hi[0]]
      assert box.size == n - m > 0, (key, n)
      assert plain.run(inputs, iterate=iterate)[name][lo[0]:hi[0]].tobytes() == box.tobytes(), (
          key, k['name'], n)
      if floaty:
        assert np.isfinite(box).all(), (key, k['name'], n)
      assert len(np.unique(box)) > min(box.size, 16) // 2, (key, k['name'], n)


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
def test_the_unit_compiles_without_scratch(key, figures):
  """With -Werror=array-bounds, from the compiler's resource report: no scratch, no spilled
  VGPR, no LDS.  The table's est_vgprs is printed beside the compiler's count and not
  asserted on: nothing consumes it for this family, and it is below the count for most of
  these kernels (profiles/r20_random1d.txt)."""
  text, table = generated(key)
  for k in fused_of(table):
    found = figures[key][k['name']]
    print('%-6s %-16s cols %d segs %d  est_vgprs %3d  compiled %3d' % (
        key, k['name'], k['cols'], k['segs'], k['est_vgprs'], found['vgpr_count']))
    assert found['private_segment_fixed_size'] == 0, (k['name'], found)
    assert found['vgpr_spill_count'] == 0, (k['name'], found)
    assert found['vgpr_count'] > 0
    assert found['group_segment_fixed_size'] == 0       # no LDS
