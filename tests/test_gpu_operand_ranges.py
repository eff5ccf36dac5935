"""Full-width operands through every kernel family and element type, on a real MI355X.

The other GPU files vary geometry; their operands come from narrow families (floats in
[0, 1) or [0.5, 1.5) with float32's mantissa whatever the type, integers in 0..199 or
0..255): one dword of every 8-byte element is constant, no narrow element has its top bit
set, every float sum adds positive numbers of one magnitude.  The generated kernels move
data in element-width-specific ways - an 8-byte element crosses lanes as two 32-bit DPP
shifts, 2- and 1-byte ones go through an `int`, rows are punned through LDS arrays of
another type - which such operands cannot see (test_the_gap_is_real shows it).

Here every run uses gpu_util.wide_inputs (integers over the whole range of the type,
floats sign * m * 2^e over 25 binades at the type's own mantissa) in a guarded arena
(test_gpu_memory_contract.hold: box == oracle BYTE for byte, guards intact, inputs
unchanged, the named family and depth among the launches) against the oracle built with
-fwrapv, as the kernels are (gpu_util.make_wrap_oracle: signed overflow wraps, which the
product promises - DESIGN.md section 2).

  * test_every_family_of_a_type: iteration chains per element type; every (family, depth)
    of the generator's table is forced and checked at two shapes, and the set of families
    per type is asserted (a generator change that adds or drops one shows up);
  * test_shipped_rows / test_shipped_tables: the shipped code objects, every family and
    depth they carry; sobel2d on full-range uint16;
  * test_the_gap_is_real: a kernel text that moves only one dword of an 8-byte element
    across lanes FAILS on these operands.

One JIT compilation per (type, dimension): double, int64, uint16, uint8 in every session,
the other six with SODA_TEST_ALL_FORMS=1."""
import contextlib
import os

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from test_gpu_memory_contract import (ALL_FORMS, FAMILY, SHIPPED_2D, SHIPPED_3D, box_of, hold,
                                      margins_of, opened)

pytestmark = pytest.mark.gpu

_HEAD = 'kernel: %s\nburst width: 512\nunroll factor: 1\niterate: %d\n'
# 5-point and 7-point windows, neighbours added AND subtracted (values cancel), one
# multiply by a literal (values grow; integers wrap)
CHAIN = {
    2: 'input {t}: a(64, *)\noutput {t}: b(0, 0) = '
       '(a(0, 0) - a(-1, 0) + a(1, 0) - a(0, -1) + a(0, 1)) * {lit}\n',
    3: 'input {t}: a(32, 32, *)\noutput {t}: b(0, 0, 0) = (a(0, 0, 0) - a(-1, 0, 0) + '
       'a(1, 0, 0) - a(0, -1, 0) + a(0, 1, 0) - a(0, 0, -1) + a(0, 0, 1)) * {lit}\n',
}
SUMS = {2: 'input {t}: a(64, *)\noutput {t}: b(0, 0) = '
           'a(0, 0) + a(-1, 0) + a(1, 0) + a(0, -1) + a(0, 1)\n'}
LITERAL = {'double': '0.75', 'float': '0.75f'}
# `iterate` of the text caps how deep the fused kernels go: 2-D up to depth 12 (the
# wave-pipelined forms of the narrow types and of float), 3-D up to depth 4 (block form
# and wave-pipelined form)
CAP = {2: 13, 3: 5}

TYPES = ('double', 'int64', 'uint64', 'int32', 'uint32', 'int16', 'uint16', 'int8', 'uint8',
         'float')
EVERY_SESSION = ('double', 'int64', 'uint16', 'uint8')
# What kernel.generate emits per element type, as (dimension, family): 8-byte elements
# have the single-wavefront streaming kernels only (2-D to depth 12, 3-D depth 1), 2- and
# 1-byte ones take the wave-pipelined form from depth 8 / 4 in 2-D and have no fused 3-D
# kernel, the deep 3-D forms (block, wave-pipelined) exist for 4-byte elements.
_WORD = {(2, 'stage'), (2, 'stream'), (3, 'stage'), (3, 'stream'), (3, 'blk'), (3, 'wp')}
_LONG = {(2, 'stage'), (2, 'stream'), (3, 'stage'), (3, 'stream')}
_NARROW = {(2, 'stage'), (2, 'stream'), (2, 'wp'), (3, 'stage')}
EXPECTED = {'double': _LONG, 'int64': _LONG, 'uint64': _LONG,
            'int32': _WORD, 'uint32': _WORD, 'float': _WORD | {(2, 'wp')},
            'int16': _NARROW, 'uint16': _NARROW, 'int8': _NARROW, 'uint8': _NARROW}


def chain_spec(c_type, dim, cap=None, text=CHAIN):
  src = (_HEAD + text[dim]).format(t=c_type, lit=LITERAL.get(c_type, '3'))
  return specmod.spec_from_stencil(frontend.loads(
      src % ('w%s%dd' % (c_type, dim), cap or CAP[dim])))


def family_of(k):
  (name,) = [f for f, is_a in FAMILY.items() if is_a(k)]
  return name


@contextlib.contextmanager
def preferring(prog, k):
  """Where the table holds several fused kernels of k's depth (3-D: single-wavefront,
  block form and wave-pipelined form) the run time takes the cheapest per launch;
  SODA_HIP_PREFER (behind SODA_HIP_TUNING, as tools/calibrate.py uses it) names the one to
  take instead.  It changes which kernel runs, never what it computes - and hold() asserts
  from the schedule that it did run."""
  same = [o for o in prog.kernels if o['kind'] == 'fused' and o['depth'] == k['depth']]
  if k['kind'] != 'fused' or len(same) < 2:
    yield
    return
  saved = {n: os.environ.get(n) for n in ('SODA_HIP_TUNING', 'SODA_HIP_PREFER')}
  os.environ['SODA_HIP_TUNING'] = '1'
  os.environ['SODA_HIP_PREFER'] = k['name'][k['name'].index('_fused_'):]
  try:
    yield
  finally:
    for n, v in saved.items():
      if v is None:
        os.environ.pop(n, None)
      else:
        os.environ[n] = v


def forcing(spec, k):
  """(iterate, split, max_depth) that make kernel k the first launch of a sweep."""
  if k['kind'] == 'stage':
    chain = len(spec['inputs']) == len(spec['outputs'])
    return (2 if chain else 1), None, -1
  d = k['depth']
  if len(spec['inputs']) != len(spec['outputs']):
    assert d == 1, k['name']          # not a chain: one iteration, one fused launch
    return 1, None, 1
  return d + 1, [d, 1], d


def shapes_for(spec, k, iterate):
  """Two array shapes from the kernel's own table entry: one ragged and two strips /
  tiles and a third wide, one just above the smallest array the kernel takes (its
  min_extent; without one: a box of a few cells)."""
  dim = spec['dim']
  m = margins_of(spec, iterate)
  least = list(k.get('min_extent') or [0, 0]) + [0]
  tile = k['tile']
  big = [m[0] + 2 * tile[0] + tile[0] // 3 + 5]
  small = [max(least[0], m[0] + 4) + 1]
  if dim == 2:
    big.append(m[1] + 67)
    small.append(m[1] + 3)
  else:
    big += [m[1] + 2 * max(tile[1], 8) + 3, m[2] + 9]
    small += [max(least[1], m[1] + 3) + 1, m[2] + 3]
  big = [max(b, l + 1) for b, l in zip(big, least)]
  return tuple(reversed(big)), tuple(reversed(small))


def hold_wide(prog, orc, key, k, shape, mode, seed=None):
  """One guarded run of kernel k on full-width operands (see hold)."""
  spec = prog.spec
  iterate, split, max_depth = forcing(spec, k)
  family = family_of(k)
  inputs = gpu_util.wide_inputs_of(key, spec, shape, seed=seed or gpu_util.SEED + sum(shape))
  prog.set_max_depth(max_depth)
  try:
    with preferring(prog, k):
      launched = hold(prog, orc, shape, iterate, mode, family,
                      k['depth'] if family != 'stage' else None, split=split, inputs=inputs)
  finally:
    prog.set_max_depth(0)
  assert k['name'] in [l['name'] for l in launched], (k['name'], [l['name'] for l in launched])


# ---- every family the generator has for a type ----------------------------------------------

@pytest.mark.parametrize('c_type', [t for t in TYPES if ALL_FORMS or t in EVERY_SESSION])
def test_every_family_of_a_type(c_type):
  seen = set()
  for dim in (2, 3):
    spec = chain_spec(c_type, dim)
    text, table = kernel.generate(spec)
    assert {(dim, family_of(k)) for k in table} == {e for e in EXPECTED[c_type] if e[0] == dim}
    prog = host.open_program(source=text, spec=spec)
    try:
      assert [k['name'] for k in prog.kernels] == [k['name'] for k in table]
      orc = gpu_util.make_wrap_oracle(spec)
      for k in prog.kernels:
        iterate = forcing(spec, k)[0]
        for shape, mode in zip(shapes_for(spec, k, iterate), ('pool', 'aligned')):
          hold_wide(prog, orc, None, k, shape, mode)
        seen.add((dim, family_of(k)))
    finally:
      prog.close()
      prog.blob.unload()
  assert seen == EXPECTED[c_type], (c_type, sorted(seen))


def test_the_types_of_a_plain_session_cover_every_family():
  """double / int64 / uint16 / uint8 reach stage, stream and the 2-D wave-pipelined form;
  the deep 3-D forms exist for 4-byte elements only, and those run on full-width
  operands from the shipped code objects and the 3-D random programs in every session."""
  assert set().union(*(EXPECTED[t] for t in EVERY_SESSION)) == _LONG | _NARROW
  assert set(EXPECTED) == set(TYPES) and set(EVERY_SESSION) < set(TYPES)


# ---- the shipped code objects ---------------------------------------------------------------

_WRAP = {}


def opened_wrap(app, prebuilt):
  """The memory-contract file's program of this name (one per session, shared with it)
  and the -fwrapv oracle."""
  prog, _ = opened(app, prebuilt=prebuilt)
  if app not in _WRAP:
    _WRAP[app] = gpu_util.make_wrap_oracle(prog.spec)
  return prog, _WRAP[app]


@pytest.mark.parametrize('app,prebuilt,family,depth,iterate,split,max_depth',
                         SHIPPED_2D + SHIPPED_3D)
def test_shipped_rows(app, prebuilt, family, depth, iterate, split, max_depth):
  """Every row of the memory-contract file's SHIPPED_2D / SHIPPED_3D - the same program,
  family, depth, iteration count, split and depth limit - once on full-width operands;
  sobel2d on full-range uint16 (mag_x * mag_x then overflows `int`: it wraps)."""
  prog, orc = opened_wrap(app, prebuilt)
  spec = prog.spec
  ks = [k for k in prog.kernels if FAMILY[family](k) and (family == 'stage' or k['depth'] == depth)]
  assert ks, (app, family, depth)
  k = ks[0]
  big, small = shapes_for(spec, k, iterate)
  if family == 'wp' and spec['dim'] == 3:
    # below the block form's smallest array, where only the wave-pipelined kernel can run
    # (test_shipped_3d_kernels): twice its own smallest array and a bit
    blk = [o for o in prog.kernels if FAMILY['blk'](o) and o['depth'] == depth]
    assert blk and k['min_extent'][0] < blk[0]['min_extent'][0]
    big = (big[0], big[1], blk[0]['min_extent'][0] - 3)
    assert big[2] > k['min_extent'][0] + 16
  inputs = gpu_util.wide_inputs_of(app, spec, big, seed=gpu_util.SEED + sum(big))
  prog.set_max_depth(max_depth)
  try:
    hold(prog, orc, big, iterate, 'pool', family, depth if family != 'stage' else None,
         split=split, inputs=inputs)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('app', ['blur', 'jacobi2d', 'jacobi3d', 'seidel2d', 'heat3d',
                                 'sobel2d', 'denoise2d', 'denoise3d', 'skew2d'])
def test_shipped_tables(app):
  """The eight sample programs and skew2d from their prebuilt code objects: EVERY kernel
  of the table (jacobi2d: the packed forms of depth 12, 16, 20 and 24; the 3-D programs:
  block form and wave-pipelined form of depth 4), each forced and found in the schedule."""
  prog, orc = opened_wrap(app, True)
  spec = prog.spec
  assert any(k['kind'] == 'fused' for k in prog.kernels)
  stages = [k for k in prog.kernels if k['kind'] == 'stage']
  for k in stages[:1] + [k for k in prog.kernels if k['kind'] == 'fused']:
    iterate = forcing(spec, k)[0]
    for shape, mode in zip(shapes_for(spec, k, iterate), ('pool', 'sixteen')):
      hold_wide(prog, orc, app, k, shape, mode)


# ---- the gap is real ------------------------------------------------------------------------

# the 8-byte branches of lane_neighbour and lane_neighbour_or (kernel_common.py): the line
# that moves one dword of the element to the neighbouring lane.  Without it the element
# keeps its OWN lane's dword: wrong arithmetic, the same loads and stores.
_SHIFT = {
    'hi': ('    h.hi = BELOW ? dpp_from_below(h.hi) : dpp_from_above(h.hi);\n',
           '    h.hi = BELOW ? __builtin_amdgcn_update_dpp(e.hi, h.hi, 0x138, 0xf, 0xf, false)\n'
           '                 : __builtin_amdgcn_update_dpp(e.hi, h.hi, 0x130, 0xf, 0xf, false);\n'),
    'lo': ('    h.lo = BELOW ? dpp_from_below(h.lo) : dpp_from_above(h.lo);\n',
           '    h.lo = BELOW ? __builtin_amdgcn_update_dpp(e.lo, h.lo, 0x138, 0xf, 0xf, false)\n'
           '                 : __builtin_amdgcn_update_dpp(e.lo, h.lo, 0x130, 0xf, 0xf, false);\n'),
}


def box_differs(prog, orc, inputs, family='stream', depth=1):
  """Cells of the valid box of one depth-1 sweep that differ from the oracle."""
  spec = prog.spec
  shape = inputs[0].shape
  dims = tuple(reversed(shape))
  prog.set_max_depth(depth)
  launched = [k for k, _ in prog.schedule(dims, 1)]
  assert [family_of(k) for k in launched] == [family], [k['name'] for k in launched]
  got = prog.run_numpy(inputs, iterate=1)[0]
  want = orc.run(inputs, iterate=1)[spec['outputs'][0]]
  lo, hi = box_of(spec, spec['outputs'][0], dims, 1)
  sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
  assert got[sl].size > 1000
  return int(np.count_nonzero(got[sl].view('<u8') != want[sl].view('<u8')))


@pytest.mark.parametrize('c_type,half', [('int64', 'hi'), ('double', 'lo')])
def test_the_gap_is_real(c_type, half):
  """A kernel text whose lane shifts move only ONE dword of an 8-byte element - int64: the
  low one (additions only), double: the high one; one iteration - differs from the oracle
  on full-width operands, and the unmodified text does not.  The mutation is arithmetic
  only: every address, load and store is the unmodified kernel's.  (What the narrow
  operands of the other files make of it is printed, not asserted: with integers in
  0..199 the high dword is 0 in every lane, with float32 values widened the low one.)"""
  spec = chain_spec(c_type, 2, cap=1, text=SUMS if c_type == 'int64' else CHAIN)
  text, table = kernel.generate(spec)
  assert [family_of(k) for k in table] == ['stage', 'stream']
  wrong = text
  for line in _SHIFT[half]:
    assert text.count(line) == 1, line
    wrong = wrong.replace(line, '')
  assert len(wrong) < len(text)
  orc = gpu_util.make_wrap_oracle(spec)
  shape = (67, 1189)
  wide = gpu_util.wide_inputs(spec, shape)
  rng = np.random.default_rng(gpu_util.SEED)
  if c_type == 'double':      # the operands of test_gpu_random_programs' oracle case
    narrow = [(rng.random(shape, dtype=np.float32) + np.float32(0.5)).astype(np.float64)]
  else:
    narrow = [rng.integers(0, 200, size=shape).astype(np.int64)]
  counts = {}
  for what, src in (('unmodified', text), ('mutated', wrong)):
    prog = host.open_program(source=src, spec=spec)
    try:
      counts[what] = (box_differs(prog, orc, wide), box_differs(prog, orc, narrow))
    finally:
      prog.close()
      prog.blob.unload()
  print('%s, lane shift without the %s dword: cells that differ (full-width, narrow operands):'
        ' unmodified %s, mutated %s' % (c_type, half, counts['unmodified'], counts['mutated']))
  assert counts['unmodified'] == (0, 0), counts
  assert counts['mutated'][0] > 0, counts
