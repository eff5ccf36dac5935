"""Fused 1-D kernels: all stages of `depth` iterations of a program over one array
(`input float: a(*)`, one input feeding one output of its type) in one launch.

A 1-D program has no outer dimension to stream along, so nothing of kernel_stream2d's
pipeline applies: no lags, no windows, no rotation, no row loop.  What stays is the
lane mapping and the overlapped tiling of its x half:

  * one wavefront computes a SEGMENT of 64*C consecutive cells, lane l holding C of
    them (one `C*sizeof(T)`-byte vector load per lane).  A level - one stage of one
    iteration - is C registers, so all `depth` iterations of all stages stay in
    registers and the register file does not limit the depth;
  * neighbours inside a lane are other registers, across lanes they come from lane-1 /
    lane+1 through DPP wave shifts folded into the consuming operation
    (kernel_stream2d.lane_operand);
  * segments overlap by the window composed over `depth` iterations, padded to whole
    vectors: the halo is recomputed, never exchanged, and HBM sees one read and one
    write per cell per `depth` updates (plus the halo re-reads);
  * there is no row loop to keep loads in flight under, so a wavefront takes `segs`
    segments, spaced four segments apart - the four wavefronts of a workgroup then load
    one contiguous run per step - and issues all their loads before the first level.

A wavefront whose segments all lie inside the array loads whole vectors (INTERIOR);
any other takes the guarded path, where cells outside the array read as 0.  Such values
reach only cells outside the launch's box (the box is the composed window).  Stores go
to the box intersected with the segment's own w_out cells, as a per-lane range of its C
cells.  Vector accesses are declared aligned to the element only: the caller's arrays
start anywhere.

`hops` (the far-tap form, kernel.generate's `far_taps`): an x-neighbour may lie up to `hops`
lanes away, lane_operand chaining one wave shift per lane; one hop prints the text above.
What a shift delivers to the first and last `hops` lanes of a wavefront falls inside the
padded halo: a cell is wrong only where a read of its level, or of a level below it, left
the segment, so the wrong cells at either end are at most the window composed so far, and
the halo is that window over all `depth` iterations padded up to whole vectors.
"""

from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_stream2d import (LANES, WAVES_PER_BLOCK, NotFusable, check_reach, kernel_name,
                              lane_operand)

DEFAULT_SEGS = 4
# lanes an x-neighbour may lie away in the far-tap form (emit's `hops`).  The chain is cheap:
# every link of a chain of wave shifts is itself an operand some nearer tap reads, so a window
# of radius R lanes costs about 2R moves per column and level next to its 2(2R + 1) arithmetic
# operations, and a level stays C registers at any depth.  What bounds the form is the halo:
# a segment of 64 lanes loses `hops` of them per side, level and iteration.  At 8 lanes per
# side a float depth-1 segment still keeps 192 of 256 cells and depth 2 half of them; beyond
# that the halo, not the chain, makes the form pointless.
MAX_HOPS_1D = 8


class Level:
  """One tensor of one iteration: C registers per lane.  Shaped like
  kernel_stream2d.Instance as far as lane_operand reads it (a window of one row that
  nothing lags behind)."""
  lag, keep = 0, 1

  def __init__(self, ident, tensor, c_type, stage=None):
    self.ident, self.tensor, self.c_type, self.stage = ident, tensor, c_type, stage
    self.reads = {}             # (name in the expression, offset) -> Level


def build_levels(spec, depth):
  """The levels of `depth` iterations in execution order, the loaded input first; the
  last one is the output that goes to HBM."""
  if spec['dim'] != 1:
    raise NotFusable('stream1d handles 1-D programs')
  if len(spec['inputs']) != 1 or len(spec['outputs']) != 1:
    raise NotFusable('stream1d handles one input feeding one output (%d input(s), '
                     '%d output(s))' % (len(spec['inputs']), len(spec['outputs'])))
  types = specmod.tensor_c_types(spec)
  source = spec['inputs'][0]
  if types[spec['outputs'][0]] != source['c_type']:
    raise NotFusable('the output (%s) is not of the input\'s type (%s)'
                     % (types[spec['outputs'][0]], source['c_type']))
  elem = specmod.ELEM_SIZE[source['c_type']]
  if elem not in (2, 4, 8):
    raise NotFusable('element size of %s' % source['name'])
  for name, c_type in types.items():
    if specmod.ELEM_SIZE[c_type] != elem:
      raise NotFusable('tensors of different widths (%s)' % name)
  levels = [Level('in_%s' % source['name'], source['name'], source['c_type'])]
  current = {source['name']: levels[0]}
  for it in range(depth):
    for stage in spec['stages']:
      level = Level('k%d_%s' % (it, stage['name']), stage['name'], stage['c_type'], stage)
      for tensor, rel in stage['loads']:
        level.reads[(tensor, tuple(rel))] = current[tensor]
      levels.append(level)
      current[stage['name']] = level
    current[source['name']] = current[spec['outputs'][0]]
  return levels


def geometry(spec, depth, cols):
  """Segment geometry for `depth` fused iterations: kernel_stream2d.geometry's x half
  with align='none'."""
  lo, hi = specmod.iteration_margins(spec, depth)[-1]
  halo_lo = -(-lo[0] // cols) * cols      # padded up to whole vectors
  halo_hi = -(-hi[0] // cols) * cols
  w_out = LANES * cols - halo_lo - halo_hi
  if w_out < cols:
    raise NotFusable('depth %d leaves no output cells in a segment' % depth)
  return dict(x_lo=lo[0], x_hi=hi[0], halo_lo=halo_lo, halo_hi=halo_hi, w_out=w_out,
              origin_align=cols)


def far_vgprs(levels, cols):
  """What reads beyond the neighbour lane keep alive while a level is computed, in 32-bit
  words: 0 for a program without them.  A wave shift folds into the operation that consumes
  it, a chain of shifts does not: every link beyond the first is a move into a register of
  its own, shared by the cells that read the same column through it.  A link stays alive
  while a cell of the level still has to read it; one that only leads on to the next link
  lives for one move.  Per level, the distinct links some cell reads - per source, side,
  column and lane beyond the first - and one level of partial sums in flight; the levels run
  one after the other, so the costliest one counts.  In a full window (lowpass1d, dfir1d,
  acoustic1d) every link is read: 2 sides x C columns x (lanes - 1); in a sparse one
  (skewfir1d's three taps) only the chains' ends are.  Held against the compiler's counts
  (hipcc 7.2, gfx950; extra over the estimate without this term, at every depth): lowpass1d
  28 against +26, dfir1d 28 against +26, skewfir1d 14 against +2 / +0, acoustic1d 28 where
  the whole kernel stays 8 under the estimate without it.  tests/test_far1d_codegen.py holds
  every shipped kernel to its estimate."""
  worst = 0
  for level in levels:
    links = {}
    for (tensor, rel), src in level.reads.items():
      for j in range(rel[0], rel[0] + cols):
        if abs(j // cols) >= 2:
          links[id(src), j < 0, j % cols, abs(j // cols)] = \
              max(1, specmod.ELEM_SIZE[src.c_type] // 4)
    if links:
      worst = max(worst, sum(links.values()) +
                  cols * max(1, specmod.ELEM_SIZE[level.c_type] // 4))
  return worst


def emit_vector_load(emit_line, function, vec, T, C, elem):
  """The vector type `vec` of C cells of T, aligned to the element only, and the load of
  one lane's vector through it: whole when the wavefront is INTERIOR, else cell by cell
  with cells outside the array reading as 0.  (kernel_fields1d prints one per element
  type.)"""
  emit_line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(%d)));'
            % (T, vec, C, elem))
  emit_line('template <bool INTERIOR>')
  emit_line('DEV %s %s(const %s* __restrict__ g, const i64 x, const i64 W) {'
            % (vec, function, T))
  emit_line('  if (INTERIOR) return *(const %s*)(g + x);' % vec)
  emit_line('  %s v;' % vec)
  for c in range(C):
    emit_line('  v[%d] = (x + %d >= 0 && x + %d < W) ? g[x + %d] : (%s)0;' % (c, c, c, c, T))
  emit_line('  return v;')
  emit_line('}')


def emit(spec, depth, cols=None, segs=DEFAULT_SEGS, hops=1):
  """Returns (text, kernel table entry) for one fused depth of a 1-D program.  hops: how many
  lanes away an x-neighbour may lie (1 .. MAX_HOPS_1D; one hop prints the neighbour-lane
  text)."""
  levels = build_levels(spec, depth)
  in_type = spec['inputs'][0]['c_type']
  elem = specmod.ELEM_SIZE[in_type]
  if cols is None:
    cols = max(1, 16 // elem)
  C = cols
  segs = int(segs)
  if segs < 1:
    raise ValueError('segs: %r' % (segs,))
  check_reach(levels, cols, hops, MAX_HOPS_1D)
  geo = geometry(spec, depth, cols)
  index = tensor_index(spec)
  name = kernel_name(spec, depth)
  T = builtin_type(in_type)
  final = levels[-1]
  vec = 'vec_%s' % name
  stride = WAVES_PER_BLOCK * geo['w_out']       # between the segments of one wavefront
  # A rough figure for the table, which nothing consumes for this family: the loaded
  # vectors of all segments (16 bytes = 4 registers each at the default C), two levels of
  # one segment unpacked to a register (pair) per cell, and ten for addresses and ranges.
  # Compiled: float and double 34 at segs = 4, 58 at segs = 8; uint16 about 50.
  # Reads beyond the neighbour lane add far_vgprs (0 without them).
  est_vgprs = segs * -(-C * elem // 4) + 2 * C * max(1, elem // 4) + 10 + far_vgprs(levels, C)

  o = []
  emit_line = o.append
  emit_line('// fused depth-%d 1-D kernel: %d level(s) of %d cell(s) per lane, %d segment(s) '
            'per wavefront,' % (depth, len(levels) - 1, C, segs))
  emit_line('// segment = %d cells (%d out + halo %d/%d), workgroup = %d cells out'
            % (LANES * C, geo['w_out'], geo['halo_lo'], geo['halo_hi'],
               segs * stride))
  emit_vector_load(emit_line, '%s_load' % name, vec, T, C, elem)
  # one segment: every level from the loaded cells, then the store.  Every lane computes
  # every level (the DPP operands are read with all lanes active); only the store is
  # conditional
  emit_line('DEV void %s_segment(const soda_hip_args& a, %s* __restrict__ g_out, const i64 xs, '
            'const i64 x, const %s v) {' % (name, T, vec))
  emit_line('  %s %s[1][%d];' % (T, levels[0].ident, C))
  emit_line('  ' + ' '.join('%s[0][%d] = v[%d];' % (levels[0].ident, c, c) for c in range(C)))
  for level in levels[1:]:
    emit_line('  %s %s[1][%d];' % (builtin_type(level.c_type), level.ident, C))
    for c in range(C):
      def load(tensor, rel, c=c, level=level):
        return lane_operand(level, level.reads[(tensor, tuple(rel))], (rel[0], 0), 0, c, C)
      cell_assignment(level.stage, '%s[0][%d]' % (level.ident, c), load, emit_line, '  ')
  # the cells of this segment that are stored, as this lane's own range [c_lo, c_hi) of
  # its C cells: the box intersected with the segment's w_out cells
  emit_line('  const i64 st_lo = xs > a.box_lo[0] ? xs : a.box_lo[0];')
  emit_line('  const i64 st_hi = xs + %d < a.box_hi[0] ? xs + %d : a.box_hi[0];'
            % (geo['w_out'], geo['w_out']))
  emit_line('  const int c_lo = (int)(st_lo - x < 0 ? 0 : st_lo - x > %d ? %d : st_lo - x);'
            % (C, C))
  emit_line('  const int c_hi = (int)(st_hi - x < 0 ? 0 : st_hi - x > %d ? %d : st_hi - x);'
            % (C, C))
  emit_line('  %s* q = g_out + x;' % T)
  emit_line('  if (c_lo == 0 && c_hi == %d) {' % C)
  emit_line('    %s r;' % vec)
  emit_line('    ' + ' '.join('r[%d] = %s[0][%d];' % (c, final.ident, c) for c in range(C)))
  emit_line('    *(%s*)q = r;' % vec)
  emit_line('  } else {')
  for c in range(C):
    emit_line('    if (%d >= c_lo && %d < c_hi) q[%d] = %s[0][%d];' % (c, c, c, final.ident, c))
  emit_line('  }')
  emit_line('}')
  emit_line('template <bool INTERIOR>')
  emit_line('DEV void %s_wave(const soda_hip_args& a, const i64 xs, const i64 x) {' % name)
  emit_line('  const i64 W = a.dims[0];')
  emit_line('  const %s* __restrict__ g_in = (const %s*)a.tensor[%d];'
            % (T, T, index[spec['inputs'][0]['name']]))
  emit_line('  %s* __restrict__ g_out = (%s*)a.tensor[%d];' % (T, T, index[final.tensor]))
  # all loads first: they are what a wavefront keeps in flight
  for s in range(segs):
    emit_line('  const %s v%d = %s_load<INTERIOR>(g_in, x + %d, W);' % (vec, s, name, s * stride))
  for s in range(segs):
    emit_line('  %s_segment(a, g_out, xs + %d, x + %d, v%d);' % (name, s * stride, s * stride, s))
  emit_line('}')
  emit_line('')
  emit_line('GLOBAL WG_SIZE(%d) void %s(soda_hip_args a) {' % (WAVES_PER_BLOCK * LANES, name))
  emit_line('  const int lane = lane_id();')
  emit_line('  const int wave = __builtin_amdgcn_workitem_id_x() >> 6;')
  emit_line('  const i64 x_origin = a.box_lo[0] - a.box_lo[0] %% %d;' % geo['origin_align'])
  emit_line('  const unsigned block_x = __builtin_amdgcn_workgroup_id_x();')
  # segment s of wavefront w: number block * 4 segs + 4 s + w of the launch
  emit_line('  const i64 xs = x_origin + ((i64)block_x * %d + wave) * %d;'
            % (WAVES_PER_BLOCK * segs, geo['w_out']))
  emit_line('  if (xs >= a.box_hi[0]) return;')
  emit_line('  const i64 x = xs - %d + lane * %d;' % (geo['halo_lo'], C))
  # (segments past the box's end inside the array are loaded and computed like the
  # others - no branch around a load - and store nothing)
  emit_line('  const bool interior = xs - %d >= 0 && xs + %d <= a.dims[0];'
            % (geo['halo_lo'], (segs - 1) * stride - geo['halo_lo'] + LANES * C))
  emit_line('  if (interior) %s_wave<true>(a, xs, x);' % name)
  emit_line('  else %s_wave<false>(a, xs, x);' % name)
  emit_line('}')
  entry = dict(name=name, kind='fused', depth=depth, stage=-1,
               block=[WAVES_PER_BLOCK * LANES, 1, 1],
               tile=[segs * stride, 1, 1, 1],
               origin_align=geo['origin_align'], fill_rows=0,
               cols=C, segs=segs, est_vgprs=est_vgprs,
               halo=[geo['halo_lo'], geo['halo_hi']], w_out=geo['w_out'])
  return '\n'.join(o) + '\n', entry
