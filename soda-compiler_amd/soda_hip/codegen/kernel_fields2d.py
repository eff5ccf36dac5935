"""Fused 2-D kernels for iterated programs over SEVERAL fields: as many outputs as
inputs, output j feeding input j of the next iteration (the wave equation's u and
u_prev, reaction-diffusion pairs, FDTD field triples; kernel_stream2d.multi_field).

The pipeline, the register windows, the strips and the chunks are kernel_stream2d's:
one wavefront per strip of 64*C columns, every instance of every iteration in
registers, x-neighbours by DPP, strips and chunks overlapping by the window composed
over `depth` iterations - here the hull of that window over all fields.  What this
form adds:

  * every input is streamed, one row of each per step, and the last iteration's
    instance of EVERY output goes to HBM.  An output that a later stage of the same
    iteration reads is kept in its window and stored from there;
  * each output is defined on a box of its own (reference host.py:1082-1091) and the
    whole of that box is the contract.  The launch's box is the intersection of the
    outputs' boxes; soda_hip_args.param[1..3] carry, per output, by how many cells its
    box is wider on each of the four sides (include/soda_hip.h, `param`).  The launcher
    tiles the UNION of the boxes - the launch's box widened by the largest extra per
    side - and the kernel does the same; a strip or chunk stores the cells of output j
    that lie in j's box.  The extras change along a sweep (they depend on how many
    iterations are done and on the depth), so they are launch arguments, not constants;
  * nothing about the union is assumed beyond its lying inside the array: rows are
    clamped into the array on both sides, columns outside it read as 0.  Such values
    reach only cells outside every output's box (boxes are the composed windows).

The same form serves, at depth 1, one-pass programs with several outputs that feed nothing
back (kernel_stream2d.rectangular: `#inputs != #outputs`, or outputs of other types than the
inputs): the pairing of output j with input j only matters between iterations.  Every
tensor is then of one element width, of any type at that width.

One guarded row loop serves every depth (no branch-free steady-state copy as in the
single-field form): the per-output store ranges would double its variants.  What the loop
keeps per output is small on purpose - the rows it stores as a range of 32-bit step
numbers, the columns as a per-lane range - so that the wave-uniform state fits the SGPR
file: the kernels compile with no SGPR parked in VGPR lanes.
"""

from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_stream2d import (DEFAULT_MAX_PERIOD, LANES, WAVES_PER_BLOCK, NotFusable,
                              build_pipeline, check_reach,
                              estimated_vgprs, geometry, kernel_name, lane_operand,
                              multi_field, rectangular, rotation_period, set_first_steps,
                              slot)

# soda_hip_args.param[1..3]: four 8-bit extras per output, 32 bits each
MAX_OUTPUTS = 6
MAX_EXTRA = 255


def output_extras(spec, done, depth):
  """Per output, (lo_x, lo_y, hi_x, hi_y): by how many cells its box after `done` +
  `depth` iterations is wider than the intersection of all outputs' boxes - what the
  launcher packs into param[1..3] for the launch that takes level `done` to `done` +
  `depth` (csrc/schedule.cpp, pack_output_extras, computes the same from its own boxes)."""
  boxes = specmod.iteration_boxes(spec, done + depth)[-1]
  mlo, mhi = specmod.iteration_margins(spec, done + depth)[-1]
  out = []
  for name in spec['outputs']:
    lo, hi = boxes[name]
    out.append((mlo[0] + lo[0], mlo[1] + lo[1], mhi[0] - hi[0], mhi[1] - hi[1]))
  return out


def pack_extras(extras):
  """[param[1], param[2], param[3]] for a list of per-output extras."""
  words = [0, 0, 0]
  for j, ex in enumerate(extras):
    assert j < MAX_OUTPUTS and all(0 <= v <= MAX_EXTRA for v in ex), (j, ex)
    word = ex[0] | ex[1] << 8 | ex[2] << 16 | ex[3] << 24
    words[j // 2] |= word << (32 * (j % 2))
  return words


def emit(spec, depth, cols=None, chunk_rows=256, prefetch=3, max_period=DEFAULT_MAX_PERIOD,
         vgpr_budget=244, waves_per_eu=0, skip_fill=1, hops=1):
  """Returns (text, kernel table entry) for one fused depth of a multi-field program, or
  for depth 1 of a rectangular one (kernel_stream2d.rectangular).  hops: as in
  kernel_stream2d.emit."""
  rect = depth == 1 and rectangular(spec)
  if not multi_field(spec) and not rect:
    raise NotFusable('fields2d handles programs whose outputs feed their inputs pairwise')
  if len(spec['outputs']) > MAX_OUTPUTS:
    raise NotFusable('%d outputs: the launch arguments carry the boxes of %d'
                     % (len(spec['outputs']), MAX_OUTPUTS))
  index = tensor_index(spec)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  if any(specmod.ELEM_SIZE[t['c_type']] != elem for t in spec['inputs']):
    raise NotFusable('fields of different widths')
  if rect and any(specmod.ELEM_SIZE[t] != elem for t in specmod.tensor_c_types(spec).values()):
    # (outputs and locals need not be of an input's type, but of its width: one lane
    # holds the same columns of every tensor)
    raise NotFusable('tensors of different widths')
  if cols is None:
    cols = max(1, 16 // elem)
  C = cols
  insts, _ = build_pipeline(spec, depth, prefetch, fields=True)
  geo = geometry(spec, depth, cols, chunk_rows, 'none')
  check_reach(insts, cols, hops)
  finals = [inst for inst in insts if inst.final]
  # (an output that a later stage reads lives in its window, `keep` rows, and is stored
  # from the newest one; the others go to HBM straight from a row of temporaries)
  period = rotation_period(insts, max_period)
  est_vgprs = estimated_vgprs(insts, cols)
  if est_vgprs > vgpr_budget:
    raise NotFusable('depth %d would need about %d VGPRs (budget %d)'
                     % (depth, est_vgprs, vgpr_budget))
  set_first_steps(insts, geo['y_lo'])
  name = kernel_name(spec, depth)
  L = max(inst.lag for inst in finals)
  out_of = {id(current): j for j, current in
            enumerate(next(i for i in finals if i.tensor == o) for o in spec['outputs'])}

  o = []
  emit_line = o.append
  emit_line('// fused depth-%d kernel over %d fields: %d stage instance(s), rotation '
            'period %d,' % (depth, len(finals), len([i for i in insts if i.stage]), period))
  emit_line('// strip = %d columns (%d out + halo %d/%d), chunk = %d rows, '
            'prefetch %d rows'
            % (LANES * C, geo['w_out'], geo['halo_lo'], geo['halo_hi'], chunk_rows, prefetch))
  emit_line('//   instance            lag keep')
  for inst in insts:
    emit_line('//   %-18s %4d %4d%s' % (inst.ident, inst.lag, inst.keep,
                                        '  -> HBM' if inst.final else ''))
  vec = {}
  # (a rectangular program may store an output of a type no input has)
  for c_type in sorted({t['c_type'] for t in spec['inputs']} | {i.c_type for i in finals}):
    vec[c_type] = 'vec_%s_%s' % (name, c_type)
    emit_line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(%d)));'
              % (builtin_type(c_type), vec[c_type], C, elem))
  # the box of output j: the launch's box widened by the extras of param[1..3]
  emit_line('struct %s_boxes { i64 lo_x[%d], lo_y[%d], hi_x[%d], hi_y[%d]; };'
            % ((name,) + (len(finals),) * 4))
  emit_line('DEV %s_boxes %s_output_boxes(const soda_hip_args& a) {' % (name, name))
  emit_line('  %s_boxes b;' % name)
  for j in range(len(finals)):
    emit_line('  { const i64 e = a.param[%d] >> %d;' % (1 + j // 2, 32 * (j % 2)))
    emit_line('    b.lo_x[%d] = a.box_lo[0] - (e & 255); b.lo_y[%d] = a.box_lo[1] - '
              '((e >> 8) & 255);' % (j, j))
    emit_line('    b.hi_x[%d] = a.box_hi[0] + ((e >> 16) & 255); b.hi_y[%d] = '
              'a.box_hi[1] + ((e >> 24) & 255); }' % (j, j))
  emit_line('  return b;')
  emit_line('}')
  # The per-column conditions of the two rare paths (a load at the array's edge, a lane
  # that stores part of its columns) do not change along the row loop, so the compiler
  # would keep each as a 64-bit lane mask in a pair of SGPRs for the whole loop: eight
  # pairs and more, which the SGPR file does not have.  Passing the per-lane operand
  # through an empty asm makes it recompute them where they are used.
  emit_line('template <typename T> DEV void %s_opaque(T& v) { asm volatile("" : "+v"(v)); }'
            % name)
  emit_line('template <bool INTERIOR>')
  emit_line('DEV void %s_strip(const soda_hip_args& a, const %s_boxes& b, const i64 xs, '
            'const i64 x, const i64 y0, const i64 y1) {' % (name, name))
  emit_line('  const i64 W = a.dims[0], H = a.dims[1];')
  # the row loop counts steps in 32 bits: a chunk is far shorter than 2^31 rows
  emit_line('  const int steps = (int)(y1 - y0) + %d;' % (L + geo['y_lo']))
  for t in spec['inputs']:
    emit_line('  const %s* __restrict__ g_%s = (const %s*)a.tensor[%d];' % (
        builtin_type(t['c_type']), t['name'], builtin_type(t['c_type']),
        index[t['name']]))
  for inst in finals:
    j = out_of[id(inst)]
    T = builtin_type(inst.c_type)
    emit_line('  %s* __restrict__ g_out%d = (%s*)a.tensor[%d];' % (T, j, T, index[inst.tensor]))
    # columns of this strip that output j stores, as this lane's own range [c_lo, c_hi)
    # of its C columns: two registers per output instead of a lane mask per column
    emit_line('  const i64 st_lo%d = xs > b.lo_x[%d] ? xs : b.lo_x[%d];' % (j, j, j))
    emit_line('  const i64 st_hi%d = xs + %d < b.hi_x[%d] ? xs + %d : b.hi_x[%d];'
              % (j, geo['w_out'], j, geo['w_out'], j))
    emit_line('  const int c_lo%d = (int)(st_lo%d - x < 0 ? 0 : st_lo%d - x > %d ? %d : st_lo%d - x);'
              % (j, j, j, C, C, j))
    emit_line('  const int c_hi%d = (int)(st_hi%d - x < 0 ? 0 : st_hi%d - x > %d ? %d : st_hi%d - x);'
              % (j, j, j, C, C, j))
    # rows of this chunk that output j stores, as the steps [n_lo, n_hi) of the row loop
    # at which they leave the pipeline: step m stores row y0 - y_lo + m - lag
    emit_line('  const i64 sy_lo%d = b.lo_y[%d] < y0 ? y0 : b.lo_y[%d] > y1 ? y1 : b.lo_y[%d];'
              % (j, j, j, j))
    emit_line('  const i64 sy_hi%d = b.hi_y[%d] < y0 ? y0 : b.hi_y[%d] > y1 ? y1 : b.hi_y[%d];'
              % (j, j, j, j))
    emit_line('  const int n_lo%d = (int)(sy_lo%d - y0) + %d, n_hi%d = (int)(sy_hi%d - y0) + %d;'
              % (j, j, geo['y_lo'] + inst.lag, j, j, geo['y_lo'] + inst.lag))
  for inst in insts:
    if inst.keep:
      emit_line('  %s %s[%d][%d];' % (builtin_type(inst.c_type), inst.ident, inst.keep, C))
  # windows start as zeros so that the prologue computes on defined values
  for inst in insts:
    for r in range(inst.keep):
      emit_line('  ' + ' '.join('%s[%d][%d] = 0;' % (inst.ident, r, c) for c in range(C)))
  emit_line('  // load head: first input row the chunk depends on')
  emit_line('  i64 head = y0 - %d;' % geo['y_lo'])
  prologue_steps = max(i.first_step for i in insts)
  prologue_steps = -(-prologue_steps // period) * period if skip_fill else 0
  emit_line('  int n = 0;')

  def emit_body(guarded):
    for u in range(period):
      emit_line('    {  // unrolled step %d' % u)
      for inst in insts:
        ctype = builtin_type(inst.c_type)
        if inst.stage is None:
          s = slot(inst, u, 0)
          emit_line('      {  // load row head+%d of %s' % (u, inst.tensor))
          emit_line('        i64 row = head + %d; if (row > H - 1) row = H - 1; '
                    'if (row < 0) row = 0;' % u)
          emit_line('        const %s* p = g_%s + row * W + x;' % (ctype, inst.tensor))
          emit_line('        if (INTERIOR) {')
          emit_line('          const %s v = *(const %s*)p;' % (vec[inst.c_type], vec[inst.c_type]))
          for c in range(C):
            emit_line('          %s[%d][%d] = v[%d];' % (inst.ident, s, c, c))
          emit_line('        } else {')
          # (recomputed per row: see <kernel>_opaque above)
          emit_line('          i64 xe = x; %s_opaque(xe);' % name)
          for c in range(C):
            emit_line('          %s[%d][%d] = (xe + %d >= 0 && xe + %d < W) ? p[%d] : (%s)0;'
                      % (inst.ident, s, c, c, c, c, ctype))
          emit_line('        }')
          emit_line('      }')
          continue
        skip = guarded and inst.first_step > u
        if skip:
          emit_line('      if (n + %d >= %d) {' % (u, inst.first_step))
        by_name = {(load_name, rel): src for src, rel, load_name in inst.reads}
        in_window = inst.keep > 0
        row_name = 'row_%s' % inst.ident
        if not in_window:
          emit_line('      %s %s[%d];' % (ctype, row_name, C))
        cell = (lambda c, inst=inst, u=u: '%s[%d][%d]' % (inst.ident, slot(inst, u, 0), c)) \
            if in_window else (lambda c, row_name=row_name: '%s[%d]' % (row_name, c))
        for c in range(C):
          def load(tensor, rel, u=u, c=c, inst=inst, by_name=by_name):
            return lane_operand(inst, by_name[(tensor, tuple(rel))], tuple(rel), u, c, C)
          cell_assignment(inst.stage, cell(c), load, emit_line, '      ')
        if inst.final:
          j = out_of[id(inst)]
          emit_line('      {  // store row head+%d-%d of %s' % (u, inst.lag, inst.tensor))
          emit_line('        const i64 y = head + %d;' % (u - inst.lag))
          emit_line('        if (n + %d >= n_lo%d && n + %d < n_hi%d) {' % (u, j, u, j))
          emit_line('          %s* q = g_out%d + y * W + x;' % (ctype, j))
          emit_line('          if (c_lo%d == 0 && c_hi%d == %d) {' % (j, j, C))
          emit_line('            %s v;' % vec[inst.c_type])
          for c in range(C):
            emit_line('            v[%d] = %s;' % (c, cell(c)))
          emit_line('            *(%s*)q = v;' % vec[inst.c_type])
          emit_line('          } else {')
          emit_line('            int lo = c_lo%d, hi = c_hi%d; %s_opaque(lo); %s_opaque(hi);'
                    % (j, j, name, name))
          for c in range(C):
            emit_line('            if (%d >= lo && %d < hi) q[%d] = %s;' % (c, c, c, cell(c)))
          emit_line('          }')
          emit_line('        }')
          emit_line('      }')
        if skip:
          emit_line('      }')
      emit_line('    }')

  if prologue_steps:
    emit_line('  // pipeline fill: instances start as their windows become useful')
    emit_line('  for (; n < %d && n < steps; n += %d, head += %d) {'
              % (prologue_steps, period, period))
    emit_body(True)
    emit_line('  }')
  emit_line('  for (; n < steps; n += %d, head += %d) {' % (period, period))
  emit_body(False)
  emit_line('  }')
  emit_line('}')
  emit_line('')
  occupancy = ''
  if waves_per_eu > 0:
    occupancy = ' __attribute__((amdgpu_waves_per_eu(%d, %d)))' % (waves_per_eu, waves_per_eu)
  emit_line('GLOBAL WG_SIZE(%d)%s void %s(soda_hip_args a) {'
            % (WAVES_PER_BLOCK * LANES, occupancy, name))
  emit_line('  const int lane = lane_id();')
  emit_line('  const int wave = __builtin_amdgcn_workitem_id_x() >> 6;')
  emit_line('  const %s_boxes b = %s_output_boxes(a);' % (name, name))
  # the union of the outputs' boxes is what strips and chunks cover (the launcher sizes
  # the grid by the same rule: csrc/schedule.cpp, make_launch)
  emit_line('  i64 lo_x = b.lo_x[0], lo_y = b.lo_y[0], hi_x = b.hi_x[0], hi_y = b.hi_y[0];')
  for j in range(1, len(finals)):
    emit_line('  if (b.lo_x[%d] < lo_x) lo_x = b.lo_x[%d]; if (b.lo_y[%d] < lo_y) lo_y = '
              'b.lo_y[%d];' % (j, j, j, j))
    emit_line('  if (b.hi_x[%d] > hi_x) hi_x = b.hi_x[%d]; if (b.hi_y[%d] > hi_y) hi_y = '
              'b.hi_y[%d];' % (j, j, j, j))
  emit_line('  const i64 x_origin = lo_x - lo_x %% %d;' % geo['origin_align'])
  emit_line('  const unsigned block_x = __builtin_amdgcn_workgroup_id_x();')
  emit_line('  const unsigned block_y = __builtin_amdgcn_workgroup_id_y();')
  emit_line('  const i64 strip = (i64)block_x * %d + wave;' % WAVES_PER_BLOCK)
  emit_line('  const i64 xs = x_origin + strip * %d;' % geo['w_out'])
  emit_line('  if (xs >= hi_x) return;')
  emit_line('  const i64 x = xs - %d + lane * %d;' % (geo['halo_lo'], C))
  emit_line('  const i64 chunk = a.param[0] > 0 ? a.param[0] : %d;' % chunk_rows)
  emit_line('  const i64 y0 = lo_y + (i64)block_y * chunk;')
  emit_line('  if (y0 >= hi_y) return;')
  emit_line('  const i64 y1 = y0 + chunk < hi_y ? y0 + chunk : hi_y;')
  emit_line('  const bool interior = xs - %d >= 0 && xs - %d + %d <= a.dims[0];'
            % (geo['halo_lo'], geo['halo_lo'], LANES * C))
  emit_line('  if (interior) %s_strip<true>(a, b, xs, x, y0, y1);' % name)
  emit_line('  else %s_strip<false>(a, b, xs, x, y0, y1);' % name)
  emit_line('}')
  entry = dict(name=name, kind='fused', depth=depth, stage=-1,
               block=[WAVES_PER_BLOCK * LANES, 1, 1],
               tile=[WAVES_PER_BLOCK * geo['w_out'], chunk_rows, 1, 1],
               origin_align=geo['origin_align'],
               fill_rows=L + geo['y_lo'],
               cols=C, prefetch=prefetch, period=period, est_vgprs=est_vgprs,
               halo=[geo['halo_lo'], geo['halo_hi']], w_out=geo['w_out'],
               steady=0, fields=len(finals))
  return '\n'.join(o) + '\n', entry
