"""Fused 1-D kernels for iterated programs over SEVERAL fields: as many outputs as inputs,
output j feeding input j of the next iteration (the 1-D wave equation's u and u_prev, a
transmission line's e and h, coupled pairs; kernel_stream2d.multi_field).

The shape is kernel_stream1d's with N fields: one wavefront per SEGMENT of 64*C cells, every
level of every iteration in registers, x-neighbours by DPP, segments overlapping by the
window composed over `depth` iterations - here the hull of that window over all fields -
and `segs` segments per wavefront, four segments apart, all of whose segs x N vector loads
are issued before the first level.  What this form adds is kernel_fields2d's x half:

  * every input is loaded, and the last iteration's level of EVERY output goes to HBM, from
    the registers a later stage of that iteration reads it from;
  * each output is defined on a box of its own and the whole of that box is the contract.
    The launch's box is the intersection of the outputs' boxes; soda_hip_args.param[1..2]
    carry, per output, by how many cells its box is wider on either side (include/
    soda_hip.h, `param`).  The launcher tiles the UNION of the boxes and the kernel does the
    same; a segment stores the cells of output j that lie in j's box and in the segment's
    own w_out cells, as a per-lane range of the lane's C cells.  The extras change along a
    sweep, so they are launch arguments, not constants;
  * nothing about the union is assumed beyond its lying inside the array: a wavefront whose
    segments all lie inside the array loads whole vectors (INTERIOR), any other takes the
    guarded path where cells outside the array read as 0.  Such values reach only cells
    outside every output's box (boxes are the composed windows).

`hops` (the far-tap form, kernel.generate's `far_taps`) is kernel_stream1d's: x-neighbours up
to `hops` lanes away through chained wave shifts.  What a shift delivers to the first and
last `hops` lanes of a wavefront falls inside the padded halo, which is the hull of the
composed windows of all fields: a wrong cell is one whose reads, level by level, left the
segment.
"""

from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_stream1d import MAX_HOPS_1D, Level, emit_vector_load, far_vgprs, geometry
from .kernel_stream2d import (LANES, WAVES_PER_BLOCK, NotFusable, check_reach, kernel_name,
                              lane_operand, multi_field)

# soda_hip_args.param[1..2]: two 8-bit extras per output, four outputs to a word
MAX_OUTPUTS = 6
MAX_EXTRA = 255
MAX_LOADS_IN_FLIGHT = 8         # vector loads per lane a wavefront issues before it computes


def default_segs(n_fields):
  return min(4, max(1, MAX_LOADS_IN_FLIGHT // n_fields))


def output_extras(spec, done, depth):
  """Per output, (lo, hi): by how many cells its box after `done` + `depth` iterations is
  wider than the intersection of all outputs' boxes - what the launcher packs into
  param[1..2] for the launch that takes level `done` to `done` + `depth` (csrc/schedule.cpp,
  pack_output_extras, computes the same from its own boxes)."""
  boxes = specmod.iteration_boxes(spec, done + depth)[-1]
  mlo, mhi = specmod.iteration_margins(spec, done + depth)[-1]
  return [(mlo[0] + boxes[name][0][0], mhi[0] - boxes[name][1][0]) for name in spec['outputs']]


def pack_extras(extras):
  """[param[1], param[2], param[3]] for a list of per-output extras."""
  words = [0, 0, 0]
  for j, ex in enumerate(extras):
    assert j < MAX_OUTPUTS and all(0 <= v <= MAX_EXTRA for v in ex), (j, ex)
    words[j // 4] |= (ex[0] | ex[1] << 8) << (16 * (j % 4))
  return words


def unpack_extras(words, n):
  """The inverse of pack_extras for n outputs."""
  return [((words[j // 4] >> (16 * (j % 4))) & 255, (words[j // 4] >> (16 * (j % 4) + 8)) & 255)
          for j in range(n)]


def build_levels(spec, depth):
  """(levels of `depth` iterations in execution order, the loaded inputs first; the last
  iteration's level of every output, in output order)."""
  if spec['dim'] != 1:
    raise NotFusable('fields1d handles 1-D programs')
  if not multi_field(spec):
    raise NotFusable('fields1d handles programs whose outputs feed their inputs pairwise')
  if len(spec['outputs']) > MAX_OUTPUTS:
    raise NotFusable('%d outputs: the launch arguments carry the boxes of %d'
                     % (len(spec['outputs']), MAX_OUTPUTS))
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  if elem not in (2, 4, 8):
    raise NotFusable('element size of %s' % spec['inputs'][0]['name'])
  if any(specmod.ELEM_SIZE[t['c_type']] != elem for t in spec['inputs']):
    raise NotFusable('fields of different widths')
  for name, c_type in specmod.tensor_c_types(spec).items():
    if specmod.ELEM_SIZE[c_type] != elem:
      raise NotFusable('tensors of different widths (%s)' % name)
  levels = [Level('in_%s' % t['name'], t['name'], t['c_type']) for t in spec['inputs']]
  current = {level.tensor: level for level in levels}
  for it in range(depth):
    for stage in spec['stages']:
      level = Level('k%d_%s' % (it, stage['name']), stage['name'], stage['c_type'], stage)
      for tensor, rel in stage['loads']:
        level.reads[(tensor, tuple(rel))] = current[tensor]
      levels.append(level)
      current[stage['name']] = level
    # output j feeds input j of the next iteration
    for t, o in zip(spec['inputs'], spec['outputs']):
      current[t['name']] = current[o]
  return levels, [current[o] for o in spec['outputs']]


def emit(spec, depth, cols=None, segs=None, hops=1):
  """Returns (text, kernel table entry) for one fused depth of a multi-field 1-D program.
  hops: how many lanes away an x-neighbour may lie (1 .. kernel_stream1d.MAX_HOPS_1D)."""
  levels, finals = build_levels(spec, depth)
  N = len(finals)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  if cols is None:
    cols = max(1, 16 // elem)
  C = cols
  segs = default_segs(N) if segs is None else int(segs)
  if segs < 1:
    raise ValueError('segs: %r' % (segs,))
  check_reach(levels, cols, hops, MAX_HOPS_1D)
  geo = geometry(spec, depth, cols)
  index = tensor_index(spec)
  name = kernel_name(spec, depth)
  stride = WAVES_PER_BLOCK * geo['w_out']       # between the segments of one wavefront
  regs = max(1, elem // 4)                      # per cell
  # A rough figure for the table, which nothing consumes for this family: the loaded
  # vectors of all fields of all segments, three iterations' worth of levels of one segment
  # (one being read, one being written, the finals) and ten plus two per output for
  # addresses and ranges.
  # Reads beyond the neighbour lane add kernel_stream1d.far_vgprs (0 without them).
  est_vgprs = segs * N * -(-C * elem // 4) + 3 * N * C * regs + 10 + 2 * N + \
      far_vgprs(levels, C)

  o = []
  emit_line = o.append
  emit_line('// fused depth-%d 1-D kernel over %d fields: %d level(s) of %d cell(s) per lane, '
            '%d segment(s) per wavefront,' % (depth, N, len(levels) - N, C, segs))
  emit_line('// segment = %d cells (%d out + halo %d/%d), workgroup = %d cells out'
            % (LANES * C, geo['w_out'], geo['halo_lo'], geo['halo_hi'], segs * stride))
  vec = {}
  for c_type in sorted({t['c_type'] for t in spec['inputs']}):
    vec[c_type] = 'vec_%s_%s' % (name, c_type)
    emit_vector_load(emit_line, '%s_load_%s' % (name, c_type), vec[c_type],
                     builtin_type(c_type), C, elem)
  # the box of output j along x: the launch's box widened by the extras of param[1..2]
  emit_line('struct %s_boxes { i64 lo[%d], hi[%d]; };' % (name, N, N))
  emit_line('DEV %s_boxes %s_output_boxes(const soda_hip_args& a) {' % (name, name))
  emit_line('  %s_boxes b;' % name)
  for j in range(N):
    emit_line('  { const i64 e = a.param[%d] >> %d;' % (1 + j // 4, 16 * (j % 4)))
    emit_line('    b.lo[%d] = a.box_lo[0] - (e & 255); b.hi[%d] = a.box_hi[0] + '
              '((e >> 8) & 255); }' % (j, j))
  emit_line('  return b;')
  emit_line('}')
  # one segment: every level from the loaded cells, then the stores.  Every lane computes
  # every level (the DPP operands are read with all lanes active); only the stores are
  # conditional
  emit_line('DEV void %s_segment(const soda_hip_args& a, const %s_boxes& b, const i64 xs, '
            'const i64 x%s) {' % (name, name, ''.join(
                ', const %s v_%s' % (vec[t['c_type']], t['name']) for t in spec['inputs'])))
  for level in levels[:N]:
    emit_line('  %s %s[1][%d];' % (builtin_type(level.c_type), level.ident, C))
    emit_line('  ' + ' '.join('%s[0][%d] = v_%s[%d];' % (level.ident, c, level.tensor, c)
                              for c in range(C)))
  for level in levels[N:]:
    emit_line('  %s %s[1][%d];' % (builtin_type(level.c_type), level.ident, C))
    for c in range(C):
      def load(tensor, rel, c=c, level=level):
        return lane_operand(level, level.reads[(tensor, tuple(rel))], (rel[0], 0), 0, c, C)
      cell_assignment(level.stage, '%s[0][%d]' % (level.ident, c), load, emit_line, '  ')
  # the cells of this segment that output j stores, as this lane's own range [c_lo, c_hi)
  # of its C cells: j's box intersected with the segment's w_out cells
  for j, final in enumerate(finals):
    T = builtin_type(final.c_type)
    emit_line('  {  // %s' % final.tensor)
    emit_line('    const i64 st_lo = xs > b.lo[%d] ? xs : b.lo[%d];' % (j, j))
    emit_line('    const i64 st_hi = xs + %d < b.hi[%d] ? xs + %d : b.hi[%d];'
              % (geo['w_out'], j, geo['w_out'], j))
    emit_line('    const int c_lo = (int)(st_lo - x < 0 ? 0 : st_lo - x > %d ? %d : st_lo - x);'
              % (C, C))
    emit_line('    const int c_hi = (int)(st_hi - x < 0 ? 0 : st_hi - x > %d ? %d : st_hi - x);'
              % (C, C))
    emit_line('    %s* q = (%s*)a.tensor[%d] + x;' % (T, T, index[final.tensor]))
    emit_line('    if (c_lo == 0 && c_hi == %d) {' % C)
    emit_line('      %s r;' % vec[final.c_type])
    emit_line('      ' + ' '.join('r[%d] = %s[0][%d];' % (c, final.ident, c) for c in range(C)))
    emit_line('      *(%s*)q = r;' % vec[final.c_type])
    emit_line('    } else {')
    for c in range(C):
      emit_line('      if (%d >= c_lo && %d < c_hi) q[%d] = %s[0][%d];'
                % (c, c, c, final.ident, c))
    emit_line('    }')
    emit_line('  }')
  emit_line('}')
  emit_line('template <bool INTERIOR>')
  emit_line('DEV void %s_wave(const soda_hip_args& a, const %s_boxes& b, const i64 xs, '
            'const i64 x) {' % (name, name))
  emit_line('  const i64 W = a.dims[0];')
  for t in spec['inputs']:
    T = builtin_type(t['c_type'])
    emit_line('  const %s* __restrict__ g_%s = (const %s*)a.tensor[%d];'
              % (T, t['name'], T, index[t['name']]))
  # all loads first: they are what a wavefront keeps in flight
  for s in range(segs):
    for t in spec['inputs']:
      emit_line('  const %s v%d_%s = %s_load_%s<INTERIOR>(g_%s, x + %d, W);'
                % (vec[t['c_type']], s, t['name'], name, t['c_type'], t['name'], s * stride))
  for s in range(segs):
    emit_line('  %s_segment(a, b, xs + %d, x + %d%s);' % (name, s * stride, s * stride, ''.join(
        ', v%d_%s' % (s, t['name']) for t in spec['inputs'])))
  emit_line('}')
  emit_line('')
  emit_line('GLOBAL WG_SIZE(%d) void %s(soda_hip_args a) {' % (WAVES_PER_BLOCK * LANES, name))
  emit_line('  const int lane = lane_id();')
  emit_line('  const int wave = __builtin_amdgcn_workitem_id_x() >> 6;')
  emit_line('  const %s_boxes b = %s_output_boxes(a);' % (name, name))
  # the union of the outputs' boxes is what the segments cover (the launcher sizes the grid
  # by the same rule: csrc/schedule.cpp, make_launch)
  emit_line('  i64 lo_x = b.lo[0], hi_x = b.hi[0];')
  for j in range(1, N):
    emit_line('  if (b.lo[%d] < lo_x) lo_x = b.lo[%d]; if (b.hi[%d] > hi_x) hi_x = b.hi[%d];'
              % (j, j, j, j))
  emit_line('  const i64 x_origin = lo_x - lo_x %% %d;' % geo['origin_align'])
  emit_line('  const unsigned block_x = __builtin_amdgcn_workgroup_id_x();')
  # segment s of wavefront w: number block * 4 segs + 4 s + w of the launch
  emit_line('  const i64 xs = x_origin + ((i64)block_x * %d + wave) * %d;'
            % (WAVES_PER_BLOCK * segs, geo['w_out']))
  emit_line('  if (xs >= hi_x) return;')
  emit_line('  const i64 x = xs - %d + lane * %d;' % (geo['halo_lo'], C))
  # (segments past the union's end inside the array are loaded and computed like the
  # others - no branch around a load - and store nothing)
  emit_line('  const bool interior = xs - %d >= 0 && xs + %d <= a.dims[0];'
            % (geo['halo_lo'], (segs - 1) * stride - geo['halo_lo'] + LANES * C))
  emit_line('  if (interior) %s_wave<true>(a, b, xs, x);' % name)
  emit_line('  else %s_wave<false>(a, b, xs, x);' % name)
  emit_line('}')
  entry = dict(name=name, kind='fused', depth=depth, stage=-1,
               block=[WAVES_PER_BLOCK * LANES, 1, 1],
               tile=[segs * stride, 1, 1, 1],
               origin_align=geo['origin_align'], fill_rows=0,
               cols=C, segs=segs, est_vgprs=est_vgprs,
               halo=[geo['halo_lo'], geo['halo_hi']], w_out=geo['w_out'], fields=N)
  return '\n'.join(o) + '\n', entry
