"""The sweep's memory contract (include/soda_hip.h: soda_hip_sweep, soda_hip_run_slab), per
kernel family, on a real MI355X:

  in[j] is never written; any cell of out[j] may be written, nothing outside the array is;
  slabs: a is never written (world 1 receives no rows), b and c as out.

Every case runs in a guarded arena (gpu_util.run_guarded / run_slab_guarded: all arrays of
the run back to back in ONE allocation between guard bands of seeded random bytes) and
asserts all three: the valid box equals the oracle's bit for bit, every guard byte is unchanged,
every input is bit-identical.  That the checker can fail is shown in
tests/test_guarded_arena.py.

The one-sided programs head* / tail* put the valid box on the array's first / last
element, which no sample does (only blur starts at cell (0, 0); none ends on the last
cell): that is where an edge store would leave the array.  Shapes come from each kernel's
own table entry (tile, min_extent, origin_align, edge_slack).

Array starts: every shape of a family's list runs from a pool allocator's placement
('pool': 4, 20, 36 ... bytes into a 64-byte piece, element-aligned, never a multiple of
16) AND from one of 'aligned' (multiples of 64) / 'sixteen' (16, 32, 48 bytes in),
alternating - half of the runs are off the 16-byte grid, and each shape meets them.

Forced generator forms cost a JIT compilation each: those on tail2d / tail3d (the box
ends on the array's last element), the shipped block form on head3d and the seidel2d and
blur wave-pipelined forms run in every session, the others with SODA_TEST_ALL_FORMS=1 (the
suite's switch for such forms).  Stage
intermediates and the ping-pong partner of a plain sweep live in plan scratch and are out
of reach (gpu_util); the slab entry covers the partner."""
import os

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel, kernel_common
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util

pytestmark = pytest.mark.gpu

ALL_FORMS = bool(os.environ.get('SODA_TEST_ALL_FORMS'))

_HEAD = '''
kernel: %s
burst width: 512
unroll factor: 1
iterate: %d
'''
TEXT = {
    # reads at offsets >= 0 only: cell 0 of the array is a valid cell
    'head2d': _HEAD + 'input float: a(64, *)\noutput float: b(0, 0) = '
              '(a(0, 0) + a(1, 0) + a(2, 0) + a(0, 1) + a(0, 2)) * 0.2f\n',
    'head3d': _HEAD + 'input float: a(32, 32, *)\noutput float: b(0, 0, 0) = '
              '(a(0, 0, 0) + a(1, 0, 0) + a(0, 1, 0) + a(0, 0, 1) + a(2, 0, 0)) * 0.2f\n',
    'head1d': _HEAD + 'input float: a(*)\noutput float: b(0) = '
              '(a(0) + a(1) * 2.0f + a(2)) * 0.25f\n',
    # reads at offsets <= 0 only: the LAST element of the array is a valid cell
    'tail2d': _HEAD + 'input float: a(64, *)\noutput float: b(0, 0) = '
              '(a(0, 0) + a(-1, 0) + a(-2, 0) + a(0, -1) + a(0, -2)) * 0.2f\n',
    'tail3d': _HEAD + 'input float: a(32, 32, *)\noutput float: b(0, 0, 0) = '
              '(a(0, 0, 0) + a(-1, 0, 0) + a(0, -1, 0) + a(0, 0, -1) + a(-2, 0, 0)) * 0.2f\n',
    'tail1d': _HEAD + 'input float: a(*)\noutput float: b(0) = '
              '(a(0) + a(-1) * 2.0f + a(-2)) * 0.25f\n',
    'tail4d': _HEAD + 'input float: a(8, 6, 5, *)\noutput float: b(0, 0, 0, 0) = '
              '(a(0,0,0,0) + a(-1,0,0,0) + a(0,-1,0,0) + a(0,0,-1,0) + a(0,0,0,-1)) * 0.25f\n',
    'head4d': _HEAD + 'input float: a(8, 6, 5, *)\noutput float: b(0, 0, 0, 0) = '
              '(a(0,0,0,0) + a(1,0,0,0) + a(0,1,0,0) + a(0,0,1,0) + a(0,0,0,1)) * 0.25f\n',
    'smooth1d': _HEAD + 'input float: a(*)\noutput float: b(0) = '
                '(a(-1) + a(0) * 2.0f + a(1)) * 0.25f\n',
    # two outputs with different one-sided windows: per-stage kernels only
    'two_out': _HEAD + 'input float: a(64, *)\noutput float: sx(0, 0) = a(0, 0) + a(1, 0)\n'
               'output float: sy(0, 0) = a(0, 0) - a(0, -3)\n',
}
# `iterate` of the program text only caps how deep the fused kernels go
CAP = {'head2d': 13, 'tail2d': 13, 'head3d': 5, 'tail3d': 5, 'two_out': 1}


def spec_of(app, cap=None):
  if app in TEXT:
    return specmod.spec_from_stencil(frontend.loads(TEXT[app] % (app, cap or CAP.get(app, 3))))
  return gpu_util.load_spec(app, iterate=cap) if cap else gpu_util.load_spec(app)


def box_of(spec, name, dims, iterate):
  lo, hi = specmod.iteration_boxes(spec, iterate)[-1][name]
  return [-v for v in lo], [n - v for n, v in zip(dims, hi)]


# Checked on the CPU, at import: the box of a head* program starts on element 0 of every
# dimension whatever the iteration count, that of a tail* program ends on the last one
# (blur's start at cell 0 is asserted per run, in hold()).
for _app in TEXT:
  if _app[:4] in ('head', 'tail'):
    _spec = spec_of(_app)
    for _it in (1, 3, 13):
      _dims = [1000] * _spec['dim']
      _lo, _hi = box_of(_spec, _spec['outputs'][0], _dims, _it)
      assert (_lo == [0] * _spec['dim']) == (_app[:4] == 'head'), (_app, _lo)
      assert (_hi == _dims) == (_app[:4] == 'tail'), (_app, _hi)
      assert all(b > a for a, b in zip(_lo, _hi))

_CACHE = {}


def opened(app, cap=None, prebuilt=False, **gen):
  """One program (and its oracle) per (app, generator options) and session."""
  key = (app, cap, prebuilt, tuple(sorted((k, str(v)) for k, v in gen.items())))
  if key not in _CACHE:
    if prebuilt:
      prog = gpu_util.open_prebuilt(app)
      spec = prog.spec
    else:
      spec = spec_of(app, cap)
      text, _ = kernel.generate(spec, **gen)
      prog = host.open_program(source=text, spec=spec)
    _CACHE[key] = (prog, gpu_util.make_oracle(spec))
  return _CACHE[key]


FAMILY = {
    'stage': lambda k: k['kind'] == 'stage',
    'stream': lambda k: k['kind'] == 'fused' and not k.get('groups') and not k.get('stack'),
    'wp': lambda k: k['kind'] == 'fused' and bool(k.get('groups')),
    'blk': lambda k: k['kind'] == 'fused' and bool(k.get('stack')),
}
SKEWS = ('pool', 'aligned', 'sixteen')


def modes_of(i):
  """The array placements shape number i of a list runs from: 'pool' always, and
  'aligned' / 'sixteen' in turn."""
  return ('pool', ('aligned', 'sixteen')[i % 2])


def skews_for(mode, n, itemsize):
  if mode == 'pool':                    # 4, 20, 36 ... bytes into a 64-byte piece
    return gpu_util.pool_skews(n, itemsize)
  if mode == 'sixteen':                 # 16, 32, 48 ... bytes in
    return [(16 * (i + 1)) % 64 for i in range(n)]
  return None


def hold(prog, orc, shape, iterate, mode, family=None, depth=None, split=None, seed=None,
         edge=None, small_ints=False, inputs=None):
  """One guarded run: box == oracle bit for bit, guards intact, inputs unchanged, and the
  launches included the family (and depth) the case names.  `edge`: 'first' / 'last' -
  the box must start on element 0 / end on the array's last element.  `inputs`: the
  caller's operands instead of gpu_util.random_inputs (tests/test_gpu_operand_ranges.py)."""
  spec = prog.spec
  dims = tuple(reversed(shape))
  if inputs is None:
    inputs = gpu_util.random_inputs(spec, shape, seed=seed or gpu_util.SEED + sum(shape),
                                    small_ints=small_ints)
  assert all(a.shape == tuple(shape) for a in inputs)
  if split:
    prog.set_split(dims, iterate, split)
  try:
    launched = [k for k, _ in prog.schedule(dims, iterate)]
    n = len(spec['inputs']) + len(spec['outputs'])
    outs, bad, timing = gpu_util.run_guarded(
        prog, inputs, iterate, skews=skews_for(mode, n, inputs[0].dtype.itemsize))
  finally:
    if split:
      prog.set_split(dims, iterate, [])
  what = (spec['app_name'], shape, iterate, mode, [k['name'] for k in launched])
  if family:
    hits = [k for k in launched if FAMILY[family](k) and depth in (None, k['depth'])]
    assert hits, ('no %s kernel of depth %s among the launches' % (family, depth), what)
  if depth is not None and family != 'stage':
    assert timing['max_depth'] == depth, (timing, what)
  want = orc.run(inputs, iterate=iterate)
  for name, got in zip(spec['outputs'], outs):
    lo, hi = box_of(spec, name, dims, iterate)
    if edge == 'first':
      assert lo == [0] * len(dims), (lo, what)
    if edge == 'last':
      assert hi == list(dims), (hi, what)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    g, w = np.ascontiguousarray(got[sl]), np.ascontiguousarray(want[name][sl])
    assert g.size > 0, what
    differ = np.argwhere(g.view(np.uint8) != w.view(np.uint8))
    assert differ.size == 0, ('%d bytes of the box differ, first at %s' % (
        len(differ), differ[0]), name, what)
  assert bad == [], (bad, what)
  return launched


def edge_of(app):
  return {'head': 'first', 'tail': 'last'}.get(app[:4], 'first' if app == 'blur' else None)


def entry(prog, family, depth):
  ks = [k for k in prog.kernels if FAMILY[family](k) and (depth is None or k['depth'] == depth)]
  assert ks, (family, depth, [k['name'] for k in prog.kernels])
  return ks[0]


def margins_of(spec, iterate):
  """Cells the box of `iterate` iterations is shorter than the array, per dimension."""
  lo, hi = specmod.iteration_boxes(spec, iterate)[-1][spec['outputs'][0]]
  return [b - a for a, b in zip(lo, hi)]


def edge_tiles(k, lo, hi):
  """The launcher's placement of a row of tiles of a kernel with edge_slack (schedule.cpp,
  launch geometry, dimension 0) for a box [lo, hi): (first tile's origin, tiles)."""
  slack, align, tile = k['edge_slack'], k['origin_align'], k['tile'][0]
  x0 = (lo + slack) - (lo + slack) % align
  if x0 >= hi:
    x0 = lo - lo % align
  nx = max(1, -(-(hi - x0 - slack) // tile))
  if nx == 1 and hi > x0 + tile:
    x0 = lo - lo % align
    nx = max(1, -(-(hi - x0 - slack) // tile))
  return x0, nx


def slack_width(k, spec, depth):
  """The smallest width at which the depth-`depth` launch of kernel k (the first of a
  split [depth, ...]) places two or more tiles and its LAST tile stores columns beyond its
  own `tile` (the slack), and - where the box start allows it at all: lo + slack must
  cross an origin_align boundary - its FIRST tile reaches back to the box's start too.
  Returns (width, first tile stretches)."""
  lo_m, hi_m = specmod.iteration_boxes(spec, depth)[-1][spec['outputs'][0]]
  lo = -lo_m[0]
  tile, least = k['tile'][0], (k.get('min_extent') or [0, 0])[0]
  align = k['origin_align']
  possible = lo % align != 0 and lo % align + k['edge_slack'] >= align
  for w in range(max(least, tile), least + 4 * tile):
    x0, nx = edge_tiles(k, lo, w - hi_m[0])
    last = w - hi_m[0] > x0 + nx * tile
    first = x0 > lo
    if nx >= 2 and last and (first or not possible):
      return w, first
  raise AssertionError('no width makes the edge tiles of %s use the slack' % k['name'])


def widths(k, floor, cell=4):
  """Widths around the kernel's own constants: its smallest array and one more, one tile
  and one more, two tiles plus the edge slack, and every residue the 16-cell vector rows
  and the 64-byte pieces distinguish."""
  tile, least = k['tile'][0], (k.get('min_extent') or [0, 0])[0]
  slack = k.get('edge_slack', 0)
  ws = [least, least + 1, tile, tile + 1, 2 * tile + slack, 2 * tile + slack + floor]
  base = max(least, 16 * -(-floor // 16) + 64)
  base -= base % 16
  ws += [base + r for r in (0, 1, 15, 16, 17, 31, 33)] + [base + 64 // cell]
  return sorted({w for w in ws if w > floor and w >= least})


def outer_extents(chunk, margin, floor):
  """Extents of the streamed (outermost) dimension: BOX extents - the array's minus the
  margin of the run - of one chunk + 1 and two chunks - 1, i.e. chunk remainders of 1 and
  of chunk - 1 against the entry's default chunk (tile's outer entry) and against any
  run-time chunk that divides it (the launcher picks the chunk of a streaming launch
  itself, from 8 rows up in steps of 4: on these small boxes usually 8, and
  chunk + 1 = 1, 2 chunk - 1 = 7 mod 8 for the 64- and 256-row defaults); plus a box of
  a few rows, a whole number of chunks and an odd size."""
  return [margin + chunk + 1, margin + 2 * chunk - 1, floor + 3, margin + 2 * chunk,
          margin + 70]


def shapes_2d(k, spec, iterate, floor):
  chunk = k['tile'][1] if k['tile'][1] > 1 else 64
  hs = outer_extents(chunk, margins_of(spec, iterate)[1], floor)
  return [(hs[i % len(hs)], w) for i, w in enumerate(widths(k, floor))]


def shapes_3d(k, spec, iterate, floor, extra_widths=()):
  ty, least_y = k['tile'][1], (k.get('min_extent') or [0, 0])[1]
  chunk = k['tile'][2] if k['tile'][2] > 1 else 64
  ys = sorted({y for y in (least_y, least_y + 1, ty, ty + 1, 2 * ty + 3, floor + 2, floor + 33)
               if y > floor and y >= least_y})
  zs = outer_extents(chunk, margins_of(spec, iterate)[2], floor)
  zs = [zs[0], zs[1], zs[2], zs[4] - 50]
  ws = sorted(set(widths(k, floor)) | set(extra_widths))
  return [(zs[i % len(zs)], ys[i % len(ys)], w) for i, w in enumerate(ws)]


def sweep_shapes(prog, orc, app, family, depth, iterate, split=None, max_depth=0, reach=2,
                 small_ints=False, need_both_edge_tiles=False):
  k = entry(prog, family, depth)
  floor = reach * iterate + 1
  if prog.spec['dim'] == 2:
    shapes = shapes_2d(k, prog.spec, iterate, floor)
  else:
    extra = []
    if k.get('edge_slack'):
      # a width at which the edge tiles of the deep launch really use the slack
      w, first = slack_width(k, prog.spec, depth)
      assert first or not need_both_edge_tiles, (k['name'], w)
      extra.append(w)
    shapes = shapes_3d(k, prog.spec, iterate, floor, extra)
  assert len(shapes) >= 8, shapes
  prog.set_max_depth(max_depth)
  try:
    for i, shape in enumerate(shapes):
      for mode in modes_of(i):
        hold(prog, orc, shape, iterate, mode, family, depth if family != 'stage' else None,
             split=split, edge=edge_of(app), small_ints=small_ints)
  finally:
    prog.set_max_depth(0)


# ---- shipped forms: what kernel.generate picks by itself --------------------------------
# the symmetric samples from the prebuilt code objects, head* / tail* compiled here

SHIPPED_2D = [
    # (app, prebuilt, family, depth, iterate, split, max_depth)
    ('blur', True, 'stage', 0, 2, None, -1),
    ('sobel2d', True, 'stage', 0, 1, None, -1),
    ('two_out', False, 'stage', 0, 1, None, -1),
    ('jacobi2d', True, 'stream', 1, 3, [1, 1, 1], 1),
    ('jacobi2d', True, 'stream', 2, 5, [2, 2, 1], 2),
    ('skew2d', True, 'stream', 2, 4, [2, 2], 2),
    ('blur', True, 'stream', 1, 2, None, 1),
    ('head2d', False, 'stream', 1, 2, [1, 1], 1),
    ('tail2d', False, 'stream', 1, 2, [1, 1], 1),
    ('head2d', False, 'stream', 2, 5, [2, 2, 1], 2),
    ('tail2d', False, 'stream', 2, 5, [2, 2, 1], 2),
    ('head2d', False, 'stage', 0, 2, None, -1),
    ('tail2d', False, 'stage', 0, 2, None, -1),
    ('jacobi2d', True, 'wp', 12, 13, [12, 1], 0),
    ('jacobi2d', True, 'wp', 24, 25, [24, 1], 0),
    ('head2d', False, 'wp', 12, 13, [12, 1], 0),
    ('tail2d', False, 'wp', 12, 13, [12, 1], 0),
]


@pytest.mark.parametrize('app,prebuilt,family,depth,iterate,split,max_depth', SHIPPED_2D)
def test_shipped_2d_kernels(app, prebuilt, family, depth, iterate, split, max_depth):
  prog, orc = opened(app, prebuilt=prebuilt)
  reach = 3 if app in ('skew2d', 'two_out') else 2
  sweep_shapes(prog, orc, app, family, depth if family != 'stage' else None, iterate, split,
               max_depth, reach=reach, small_ints=(app == 'sobel2d'))


SHIPPED_3D = [
    ('jacobi3d', True, 'stage', 0, 2, None, -1),
    ('head3d', False, 'stage', 0, 2, None, -1),
    ('tail3d', False, 'stage', 0, 2, None, -1),
    ('jacobi3d', True, 'stream', 1, 1, [1], 1),
    ('heat3d', True, 'stream', 2, 3, [2, 1], 2),
    ('head3d', False, 'stream', 2, 3, [2, 1], 2),
    ('tail3d', False, 'stream', 2, 3, [2, 1], 2),
    ('jacobi3d', True, 'wp', 4, 5, [4, 1], 0),
    ('heat3d', True, 'wp', 4, 4, [4], 0),
    ('head3d', False, 'wp', 4, 5, [4, 1], 0),
    ('tail3d', False, 'wp', 4, 5, [4, 1], 0),
]


@pytest.mark.parametrize('app,prebuilt,family,depth,iterate,split,max_depth', SHIPPED_3D)
def test_shipped_3d_kernels(app, prebuilt, family, depth, iterate, split, max_depth):
  """The shipped table carries the block form AND the wave-pipelined kernel at depth 4
  and the run time picks per launch: below the block form's 128 x 64 array only the
  wave-pipelined one can run, which is what the 'wp' cases here rely on (asserted from
  the launches); the block form alone is in test_forced_3d_forms."""
  prog, orc = opened(app, prebuilt=prebuilt)
  if family == 'wp':
    k = entry(prog, 'wp', 4)
    blk = entry(prog, 'blk', 4)
    assert k['min_extent'][0] < blk['min_extent'][0]
    # shapes narrower than the block form's smallest array
    prog.set_max_depth(0)
    floor = 2 * iterate + 1
    shapes = [s for s in shapes_3d(k, prog.spec, iterate, floor) if s[2] < blk['min_extent'][0]]
    assert len(shapes) >= 6, shapes
    for i, shape in enumerate(shapes):
      for mode in modes_of(i):
        hold(prog, orc, shape, iterate, mode, 'wp', 4, split=split, edge=edge_of(app))
    # and at and above it: depth 4 in whichever form the scheduler takes
    for i, shape in enumerate(shapes_3d(blk, prog.spec, iterate, floor)[:6]):
      for mode in modes_of(i):
        hold(prog, orc, shape, iterate, mode, None, 4, split=split, edge=edge_of(app))
    return
  sweep_shapes(prog, orc, app, family, depth if family != 'stage' else None, iterate, split,
               max_depth)


@pytest.mark.parametrize('app,shape,iterate', [
    ('smooth1d', (100003,), 3), ('head1d', (100003,), 3), ('tail1d', (100003,), 3),
    ('tail1d', (1025,), 2), ('head1d', (1023,), 1),
    ('hyper4d', (11, 23, 31, 203), 2), ('head4d', (7, 9, 11, 129), 2),
    ('tail4d', (7, 9, 11, 129), 2), ('tail4d', (5, 6, 7, 64), 1)])
def test_one_and_four_dimensional_programs(app, shape, iterate):
  prog, orc = opened(app, prebuilt=(app == 'hyper4d'))
  for mode in SKEWS:
    hold(prog, orc, shape, iterate, mode, 'stage', edge=edge_of(app))


# ---- forced generator forms ---------------------------------------------------------------

_WP_2D = (dict(wave_groups=4, pairs=2, vgpr_budget=250, ring=12, max_period=12, waves_per_eu=4),
          dict(wave_groups=4, pairs=2, vgpr_budget=250, ring=6, waves_per_eu=3))
_FORCED_2D = (
    [(app, 'stream', d, dict(depths=[d], **o))
     for app in ('jacobi2d', 'head2d', 'tail2d')
     for d, o in ((1, dict(align='exact')), (1, dict(align='store')), (2, dict(align='store')),
                  (1, dict(nontemporal=2)), (2, dict(nontemporal=3)))] +
    # the four SHIPPED_FORMS of test_gpu_parity.py, jacobi2d's two on head2d / tail2d as well
    [(app, 'wp', 12, dict(depths=[12], **o))
     for app in ('jacobi2d', 'head2d', 'tail2d') for o in _WP_2D] +
    [('seidel2d', 'wp', 12, dict(depths=[12], wave_groups=4, pairs=2, vgpr_budget=250, ring=6)),
     ('blur', 'wp', 8, dict(depths=[8], wave_groups=4, vgpr_budget=200, ring=6))])
# every session: all forms on tail2d, and the seidel2d and blur forms (no one-sided
# program takes those); on jacobi2d and head2d with SODA_TEST_ALL_FORMS=1
FORCED_2D = [c for c in _FORCED_2D if ALL_FORMS or c[0] in ('tail2d', 'seidel2d', 'blur')]


@pytest.mark.parametrize('app,family,depth,options', FORCED_2D)
def test_forced_2d_forms(app, family, depth, options):
  prog, orc = opened(app, cap=31, **options)
  iterate = depth + 1
  sweep_shapes(prog, orc, app, family, depth, iterate, split=[depth, 1],
               max_depth=0)


_FORCED_3D = (
    [(app, 'stream', 2, dict(depths=[2], deep3d_from=3, nt=2))
     for app in ('tail3d', 'head3d', 'jacobi3d')] +
    [(app, 'wp', 4, dict(deep3d='wp', **o))
     for app in ('tail3d', 'head3d', 'heat3d')
     for o in (dict(), dict(wp_nt=2), dict(wp_nt=4), dict(wp_pairs=0))] +
    [(app, 'blk', 4, dict(deep3d='blk', **o))
     for app in ('tail3d', 'head3d', 'jacobi3d')
     for o in (dict(), dict(blk_wide_stores=1, blk_nt=2), dict(blk_wide_stores=0),
               dict(blk_edge=1), dict(blk_edge=0), dict(blk_mask_loads=0))])
# every session: all forms on tail3d (the box ends on the array's last element) and the
# shipped block form on head3d; the rest with SODA_TEST_ALL_FORMS=1
FORCED_3D = [c for c in _FORCED_3D if ALL_FORMS or c[0] == 'tail3d' or
             (c[0], c[1], c[3]) == ('head3d', 'blk', dict(deep3d='blk'))]


@pytest.mark.parametrize('app,family,depth,options', FORCED_3D)
def test_forced_3d_forms(app, family, depth, options):
  """One form ALONE next to the shallow kernels, so the launches cannot pick another.
  For entries with an edge_slack the widths include one at which, by the launcher's own
  placement rule (edge_tiles), the last tile of the depth-4 launch stores the columns the
  alignment dropped and - on tail3d, asserted - the first tile reaches back too."""
  # (no `depths` for the deep forms: the program's iteration count, 5, caps the table at
  # depth 4, and an explicit depth 4 would add a single-wavefront kernel of that depth)
  prog, orc = opened(app, cap=5, **options)
  iterate = depth + 1
  k = entry(prog, family, depth)
  assert bool(k.get('edge_slack')) == (family == 'blk' and options.get('blk_edge', 1) == 1), k
  # tail3d's depth-4 box starts 8 columns in: there the first tile reaches back as well
  sweep_shapes(prog, orc, app, family, depth, iterate, split=[depth, 1], max_depth=0,
               need_both_edge_tiles=(app == 'tail3d' and bool(k.get('edge_slack'))))


# ---- launches beyond the Infinity Cache: the non-temporal and wide-store instantiations ----

@pytest.mark.parametrize('alone', [True, False])
def test_large_tail3d_grid_beyond_the_infinity_cache(alone):
  """The shipped block form switches to its non-temporal, whole-64-byte-piece stores by
  itself (nt & 4, wide_stores == 2) when the LAUNCH's box - inputs plus outputs - is
  beyond the Infinity Cache; the array alone stays below that size.  In the shipped
  table the scheduler gives the depth-4 launch of this program to the wave-pipelined
  kernel (which has no such instantiation) and the depth-1 launch to the block form;
  with the block form alone in the table (deep3d='blk': the same entries, nothing else
  forced) the depth-4 launch is the block form's too.  Both are run."""
  prog, orc = opened('tail3d', cap=5, deep3d='blk') if alone else opened('tail3d')
  spec = prog.spec
  shape, iterate, deep = (172, 481, 513), 5, 4
  dims = tuple(reversed(shape))
  assert int(np.prod(shape)) * 4 < kernel_common.NT_STREAMING_BYTES

  def box_bytes(level):       # of the launch that produces `level`: inputs + outputs
    lo, hi = box_of(spec, spec['outputs'][0], dims, level)
    return 2 * 4 * int(np.prod([b - a for a, b in zip(lo, hi)]))
  # past the threshold by geometry (5 %), not by a plane
  assert box_bytes(deep) > 1.05 * kernel_common.NT_STREAMING_BYTES
  assert box_bytes(iterate) > 1.05 * kernel_common.NT_STREAMING_BYTES
  launched = hold(prog, orc, shape, iterate, 'pool', 'blk' if alone else None, deep,
                  split=[deep, 1], edge='last')
  assert [k['depth'] for k in launched] == [deep, 1], [k['name'] for k in launched]
  streaming = [k for k in launched if k.get('stack')]
  assert streaming and (not alone or launched[0].get('stack')), [k['name'] for k in launched]
  for k in streaming:
    assert k.get('wide_stores') == 2 and k.get('nt', 0) & 4, k


def test_large_jacobi2d_8192_at_depth_4():
  """The stream_chunk launch rule of the shallow 2-D kernels on a box of 2 x 256 MiB."""
  prog, orc = opened('jacobi2d', prebuilt=True)
  prog.set_max_depth(4)
  try:
    hold(prog, orc, (8192, 8192), 7, 'pool', 'stream', 4)
  finally:
    prog.set_max_depth(0)


# ---- through soda_hip_run_slab, world 1: the ping-pong partner is the caller's too -------

@pytest.mark.parametrize('app,prebuilt,shape,iterate,exchange,max_depth', [
    ('jacobi2d', True, (300, 900), 50, 24, 0),       # super-steps of 24, 24 and 2
    ('jacobi2d', True, (300, 900), 50, 24, 16),
    ('jacobi2d', True, (300, 900), 50, 24, 8),
    ('jacobi2d', True, (211, 517), 7, 3, 1),
    ('jacobi3d', True, (45, 70, 131), 9, 4, 0),
    ('heat3d', True, (45, 70, 131), 9, 4, 0),
    ('tail2d', False, (270, 777), 13, 5, 0),
    ('head2d', False, (270, 777), 13, 5, 0),
    ('tail3d', False, (40, 70, 135), 5, 2, 0),
    ('head3d', False, (40, 70, 135), 5, 2, 0)])
def test_run_slab_world_1(app, prebuilt, shape, iterate, exchange, max_depth):
  prog, orc = opened(app, prebuilt=prebuilt)
  spec = prog.spec
  dims = tuple(reversed(shape))
  (a,) = gpu_util.random_inputs(spec, shape)
  want = orc.run([a], iterate=iterate)[spec['outputs'][0]]
  lo, hi = box_of(spec, spec['outputs'][0], dims, iterate)
  sl = tuple(slice(p, q) for p, q in zip(reversed(lo), reversed(hi)))
  if edge_of(app) == 'first':
    assert lo == [0] * len(dims)
  if edge_of(app) == 'last':
    assert hi == list(dims)
  prog.set_max_depth(max_depth)
  try:
    # what the setting makes of the super-steps (run_slab sweeps `exchange` iterations at
    # a time, the rest at the end), against what the scheduler takes without a limit: no
    # launch deeper than asked, and where the free choice is deeper than the limit (on
    # this grid it takes 12 + 12 for 24 iterations: limits 8 and 1 bind, 16 does not) the
    # limited run is a DIFFERENT, shallower schedule - the setting is not a no-op
    steps = sorted({min(exchange, iterate - done) for done in range(0, iterate, exchange)})
    deepest = {n: max(k['depth'] for k, _ in prog.schedule(dims, n)) for n in steps}
    prog.set_max_depth(0)
    free = {n: max(k['depth'] for k, _ in prog.schedule(dims, n)) for n in steps}
    prog.set_max_depth(max_depth)
    assert free[exchange] > 1, free               # fused kernels serve the slab path
    if max_depth > 0:
      assert all(d <= max_depth for d in deepest.values()), (deepest, max_depth)
      if max_depth in (1, 8):
        assert free[exchange] > max_depth >= deepest[exchange], (deepest, free)
    else:
      assert deepest == free
    for mode in SKEWS:
      got, n_ex, bad = gpu_util.run_slab_guarded(
          prog, a, iterate, exchange, skews=skews_for(mode, 3, a.dtype.itemsize))
      assert n_ex == 0
      g, w = np.ascontiguousarray(got[sl]), np.ascontiguousarray(want[sl])
      assert g.size > 0 and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (app, mode)
      assert bad == [], (bad, app, shape, mode)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('app,prebuilt,shape,done,more', [
    ('jacobi2d', True, (260, 700), 5, 12), ('tail2d', False, (260, 700), 3, 12),
    ('head2d', False, (150, 531), 4, 2), ('jacobi3d', True, (40, 66, 131), 2, 4),
    ('tail3d', False, (40, 66, 131), 1, 4)])
def test_resumed_sweeps_with_valid_margins(app, prebuilt, shape, done, more):
  """valid_lo / valid_hi: the input holds level `done` on its box and ANYTHING outside
  (here: random bits); `more` iterations on top give level done + more on its box."""
  prog, orc = opened(app, prebuilt=prebuilt)
  spec = prog.spec
  dims = tuple(reversed(shape))
  name = spec['outputs'][0]
  (a,) = gpu_util.random_inputs(spec, shape)
  lo, hi = box_of(spec, name, dims, done)
  level = np.random.default_rng(11).integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(
      np.float32).copy()
  sl = tuple(slice(p, q) for p, q in zip(reversed(lo), reversed(hi)))
  level[sl] = orc.run([a], iterate=done)[name][sl]
  want = orc.run([a], iterate=done + more)[name]
  for mode in SKEWS:
    outs, bad, _ = gpu_util.run_guarded(
        prog, [level], more, skews=skews_for(mode, 2, 4), valid_lo=lo,
        valid_hi=[n - v for n, v in zip(dims, hi)])
    flo, fhi = box_of(spec, name, dims, done + more)
    fsl = tuple(slice(p, q) for p, q in zip(reversed(flo), reversed(fhi)))
    g, w = np.ascontiguousarray(outs[0][fsl]), np.ascontiguousarray(want[fsl])
    assert g.size > 0 and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (app, mode)
    assert bad == [], (bad, app, mode)


@pytest.mark.parametrize('app,shape,iterate', [
    ('jacobi2d', (203, 517), 9), ('blur', (130, 515), 3), ('heat3d', (37, 45, 70), 5)])
def test_the_arena_path_is_not_a_different_computation(app, shape, iterate):
  prog, _ = opened(app, prebuilt=True)
  spec = prog.spec
  inputs = gpu_util.random_inputs(spec, shape)
  plain = prog.run_numpy(inputs, iterate=iterate)
  outs, bad, _ = gpu_util.run_guarded(prog, inputs, iterate,
                                      skews=gpu_util.pool_skews(len(inputs) + len(plain),
                                                                inputs[0].dtype.itemsize))
  assert bad == []
  dims = tuple(reversed(shape))
  for name, p, g in zip(spec['outputs'], plain, outs):
    lo, hi = box_of(spec, name, dims, iterate)
    sl = tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))
    assert p[sl].size > 0 and np.array_equal(
        np.ascontiguousarray(p[sl]).view(np.uint8), np.ascontiguousarray(g[sl]).view(np.uint8))
