"""Fused 3-D kernels for iterated programs over SEVERAL fields: as many outputs as
inputs, output j feeding input j of the next iteration (a leapfrog wave equation's u and
u_prev, FDTD field triples; kernel_stream2d.multi_field).

The form is kernel_stream3d's, with the relation to it that kernel_fields2d has to
kernel_stream2d: one wavefront owns a (64*C) x R tile of every live plane, z is streamed,
x-neighbours come by DPP wave shifts, y-neighbours from the lane's own registers, tiles
and z chunks overlap by the window composed over `depth` iterations - here the hull of
that window over all fields.  No LDS, no barrier.  What this form adds:

  * every input is streamed, one plane tile of each per step, and the last iteration's
    instance of EVERY output goes to HBM.  An output that a later stage of the same
    iteration reads is kept in its window and stored from there;
  * each output is defined on a box of its own (reference host.py:1082-1091) and the
    whole of that box is the contract, in all three dimensions.  The launch's box is the
    intersection of the outputs' boxes; soda_hip_args.param[1 + j] carries, for output
    j, by how many cells its box is wider on each of the six sides (include/soda_hip.h,
    `param`).  The launcher tiles the UNION of the boxes and the kernel does the same; a
    tile stores the cells of output j that lie in j's box: its columns as a per-lane
    range, its rows as a range of the tile's row numbers, its planes as a range of the
    plane loop's step numbers;
  * nothing about the union is assumed beyond its lying inside the array: planes and
    rows are clamped into the array on both sides, columns outside it read as 0.  Such
    values reach only cells outside every output's box (boxes are the composed windows).

At depth 1 the form also takes one-pass programs with several outputs that feed nothing back
(kernel_stream2d.rectangular), as kernel_fields2d does.
"""

from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_stream2d import (LANES, WAVES_PER_BLOCK, NotFusable, multi_field,
                              rectangular, rotation_period, slot)
from .kernel_stream3d import kernel_name, pipeline

# soda_hip_args.param[1..3]: six 8-bit extras per output, one word each
MAX_OUTPUTS = 3
MAX_EXTRA = 255
# (rows, columns) per lane that emit() tries when the caller names none
TILE_SHAPES = tuple((r, c) for c in (2, 1) for r in (16, 12, 8))


def output_extras(spec, done, depth):
  """Per output, (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z): by how many cells its box after
  `done` + `depth` iterations is wider than the intersection of all outputs' boxes - what
  the launcher packs into param[1 + j] for the launch that takes level `done` to `done` +
  `depth` (csrc/schedule.cpp, pack_output_extras, computes the same from its own boxes)."""
  boxes = specmod.iteration_boxes(spec, done + depth)[-1]
  mlo, mhi = specmod.iteration_margins(spec, done + depth)[-1]
  out = []
  for name in spec['outputs']:
    lo, hi = boxes[name]
    out.append(tuple(mlo[d] + lo[d] for d in range(3)) +
               tuple(mhi[d] - hi[d] for d in range(3)))
  return out


def pack_extras(extras):
  """[param[1], param[2], param[3]] for a list of per-output extras."""
  words = [0, 0, 0]
  for j, ex in enumerate(extras):
    assert j < MAX_OUTPUTS and all(0 <= v <= MAX_EXTRA for v in ex), (j, ex)
    words[j] = sum(v << (8 * i) for i, v in enumerate(ex))
  return words


def tile_geometry(spec, depth, rows, cols):
  """Halo and output cells of a (64 * cols) x rows tile under the hull of the windows
  composed over `depth` iterations."""
  lo, hi = specmod.iteration_margins(spec, depth)[-1]
  halo_lo = -(-lo[0] // cols) * cols      # padded up to whole vectors
  halo_hi = -(-hi[0] // cols) * cols
  w_out = LANES * cols - halo_lo - halo_hi
  r_out = rows - lo[1] - hi[1]
  return dict(lo=lo, hi=hi, halo_lo=halo_lo, halo_hi=halo_hi, w_out=w_out, r_out=r_out,
              kept=max(0, w_out) * max(0, r_out) / float(LANES * cols * rows))


def shapes_by_kept_fraction(spec, depth, shapes=TILE_SHAPES):
  """The tile shapes ordered by how much of the tile survives the halo (most first;
  among equals the larger tile)."""
  return sorted(shapes, key=lambda s: (-tile_geometry(spec, depth, s[0], s[1])['kept'],
                                       -s[0] * s[1]))


def emit(spec, depth, cols=2, rows=16, chunk_planes=64, prefetch=0, max_period=12,
         vgpr_budget=250, waves_per_eu=0):
  """Returns (text, kernel table entry) for one fused depth of a 3-D multi-field program, or
  for depth 1 of a rectangular one (kernel_stream2d.rectangular)."""
  rect = depth == 1 and rectangular(spec)
  if spec['dim'] != 3 or not (multi_field(spec) or rect):
    raise NotFusable('fields3d handles 3-D programs whose outputs feed their inputs pairwise')
  if len(spec['outputs']) > MAX_OUTPUTS:
    raise NotFusable('%d outputs: the launch arguments carry the boxes of %d'
                     % (len(spec['outputs']), MAX_OUTPUTS))
  types = specmod.tensor_c_types(spec)
  index = tensor_index(spec)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  if any(specmod.ELEM_SIZE[t] != elem for t in types.values()):
    raise NotFusable('fields of different widths')
  if elem not in (4, 8):
    raise NotFusable('fields3d handles 4- and 8-byte elements')
  C, R = cols, rows
  insts, _ = pipeline(spec, depth, prefetch, fields=True)
  geo = tile_geometry(spec, depth, R, C)
  lo, hi = geo['lo'], geo['hi']
  halo_lo, w_out, r_out = geo['halo_lo'], geo['w_out'], geo['r_out']
  y_lo, y_hi = lo[1], hi[1]
  if w_out < C or r_out < 1:
    raise NotFusable('depth %d leaves no output cells in a %dx%d tile'
                     % (depth, LANES * C, R))
  for inst in insts:
    for src, rel, _ in inst.reads:
      if abs(rel[0]) > C:
        raise NotFusable('x offset %d exceeds the %d columns a lane holds'
                         % (rel[0], C))
  finals = [inst for inst in insts if inst.final]
  period = rotation_period(insts, max_period)
  per_elem = max(1, elem // 4)
  est_vgprs = sum(inst.keep * R * C * per_elem for inst in insts) + \
      R * C * per_elem + 24
  if est_vgprs > vgpr_budget:
    raise NotFusable('depth %d would need about %d VGPRs in %dx%d tiles (budget %d)'
                     % (depth, est_vgprs, LANES * C, R, vgpr_budget))
  stage_boxes = specmod.iteration_boxes(spec, depth)
  name = kernel_name(spec, depth)
  L = max(inst.lag for inst in finals)
  out_of = {id(current): j for j, current in
            enumerate(next(i for i in finals if i.tensor == o) for o in spec['outputs'])}
  n_out = len(finals)

  o = []
  line = o.append
  line('// fused depth-%d 3-D kernel over %d fields: tile %d x %d per wavefront (%d x %d out),'
       % (depth, n_out, LANES * C, R, w_out, r_out))
  line('// rotation period %d, prefetch %d planes, ~%d VGPRs' % (period, prefetch, est_vgprs))
  for inst in insts:
    line('//   %-18s lag %2d keep %2d%s' % (inst.ident, inst.lag, inst.keep,
                                           '  -> HBM' if inst.final else ''))
  vec = {}
  # (a rectangular program may store an output of a type no input has)
  for c_type in sorted({t['c_type'] for t in spec['inputs']} | {i.c_type for i in finals}):
    vec[c_type] = 'vec_%s_%s' % (name, c_type)
    line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(%d)));'
         % (builtin_type(c_type), vec[c_type], C, elem))
  # the box of output j: the launch's box widened by the extras of param[1 + j]
  line('struct %s_boxes { i64 lo[%d][3], hi[%d][3]; };' % (name, n_out, n_out))
  line('DEV %s_boxes %s_output_boxes(const soda_hip_args& a) {' % (name, name))
  line('  %s_boxes b;' % name)
  for j in range(n_out):
    line('  { const i64 e = a.param[%d];' % (1 + j))
    for d in range(3):
      line('    b.lo[%d][%d] = a.box_lo[%d] - ((e >> %d) & 255); '
           'b.hi[%d][%d] = a.box_hi[%d] + ((e >> %d) & 255);'
           % (j, d, d, 8 * d, j, d, d, 24 + 8 * d))
    line('  }')
  line('  return b;')
  line('}')
  # per-lane conditions that do not change along the plane loop (a load at the array's
  # edge, a lane that stores part of its columns) would each stay a 64-bit lane mask in
  # a pair of SGPRs for the whole loop; passed through an empty asm they are recomputed
  # where they are used (kernel_fields2d: the same device)
  line('template <typename T> DEV void %s_opaque(T& v) { asm volatile("" : "+v"(v)); }'
       % name)
  # ... and so would the wave-uniform ones: whether row r of the tile lies in output j's
  # box, for every r and j, hoisted out of the plane loop into scalar registers the file
  # does not have.  The same device with a scalar operand
  line('template <typename T> DEV void %s_opaque_s(T& v) { asm volatile("" : "+s"(v)); }'
       % name)
  line('template <bool INTERIOR>')
  line('DEV void %s_tile(const soda_hip_args& a, const %s_boxes& b, const i64 xs, '
       'const i64 x, const i64 yb, const i64 z0, const i64 z1) {' % (name, name))
  line('  const i64 W = a.dims[0], H = a.dims[1], D = a.dims[2];')
  line('  const i64 plane = W * H;')
  # rows of the tile, clamped into the array (clamped rows only feed halo cells);
  # wave-uniform, so they live in scalar registers - as 32-bit distances from the
  # tile's first row in the array, y_base, one register each: with three fields in and
  # three out the scalar file has no room for R 64-bit offsets
  line('  const i64 y_base = yb < 0 ? 0 : (yb > H - 1 ? H - 1 : yb);')
  line('  const i64 row_base = y_base * W;')
  line('  int row_dy[%d];' % R)
  for r in range(R):
    line('  { i64 y = yb + %d; y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y); '
         'row_dy[%d] = (int)(y - y_base); }' % (r, r))
  # the plane loop counts steps in 32 bits: a chunk is far shorter than 2^31 planes
  line('  const int steps = (int)(z1 - z0) + %d;' % (L + lo[2]))
  for t in spec['inputs']:
    line('  const %s* __restrict__ g_%s = (const %s*)a.tensor[%d];' % (
        builtin_type(t['c_type']), t['name'], builtin_type(t['c_type']),
        index[t['name']]))
  for inst in finals:
    j = out_of[id(inst)]
    T = builtin_type(inst.c_type)
    line('  %s* __restrict__ g_out%d = (%s*)a.tensor[%d];' % (T, j, T, index[inst.tensor]))
    # columns of this tile that output j stores, as this lane's own range [c_lo, c_hi)
    # of its C columns
    line('  const i64 st_lo%d = xs > b.lo[%d][0] ? xs : b.lo[%d][0];' % (j, j, j))
    line('  const i64 st_hi%d = xs + %d < b.hi[%d][0] ? xs + %d : b.hi[%d][0];'
         % (j, w_out, j, w_out, j))
    line('  const int c_lo%d = (int)(st_lo%d - x < 0 ? 0 : st_lo%d - x > %d ? %d : st_lo%d - x);'
         % (j, j, j, C, C, j))
    line('  const int c_hi%d = (int)(st_hi%d - x < 0 ? 0 : st_hi%d - x > %d ? %d : st_hi%d - x);'
         % (j, j, j, C, C, j))
    # rows of this tile that output j stores, as the tile's row numbers [r_lo, r_hi)
    line('  const int r_lo%d = (int)(b.lo[%d][1] - yb < 0 ? 0 : b.lo[%d][1] - yb > %d ? %d : '
         'b.lo[%d][1] - yb);' % (j, j, j, R, R, j))
    line('  const int r_hi%d = (int)(b.hi[%d][1] - yb < 0 ? 0 : b.hi[%d][1] - yb > %d ? %d : '
         'b.hi[%d][1] - yb);' % (j, j, j, R, R, j))
    # planes of this chunk that output j stores, as the steps [n_lo, n_hi) of the plane
    # loop at which they leave the pipeline: step m stores plane z0 - lo_z + m - lag
    line('  const i64 sz_lo%d = b.lo[%d][2] < z0 ? z0 : b.lo[%d][2] > z1 ? z1 : b.lo[%d][2];'
         % (j, j, j, j))
    line('  const i64 sz_hi%d = b.hi[%d][2] < z0 ? z0 : b.hi[%d][2] > z1 ? z1 : b.hi[%d][2];'
         % (j, j, j, j))
    line('  const int n_lo%d = (int)(sz_lo%d - z0) + %d, n_hi%d = (int)(sz_hi%d - z0) + %d;'
         % (j, j, lo[2] + inst.lag, j, j, lo[2] + inst.lag))
  for inst in insts:
    if inst.keep:
      line('  %s %s[%d][%d][%d];' % (builtin_type(inst.c_type), inst.ident, inst.keep, R, C))
  # windows start as zeros so that the first steps compute on defined values
  for inst in insts:
    for k in range(inst.keep):
      for r in range(R):
        line('  ' + ' '.join('%s[%d][%d][%d] = 0;' % (inst.ident, k, r, c) for c in range(C)))
  line('  i64 head = z0 - %d;' % lo[2])
  line('  for (int n = 0; n < steps; n += %d, head += %d) {' % (period, period))

  def operand(reader, src, rel, u, r, c):
    back = reader.lag - src.lag - rel[2]
    assert 0 <= back < src.keep, (reader.ident, src.ident, rel, back, src.keep)
    rr = min(max(r + rel[1], 0), R - 1)      # clamped rows are halo rows
    row = '%s[%d][%d]' % (src.ident, slot(src, u, back), rr)
    j = c + rel[0]
    if 0 <= j < C:
      return '%s[%d]' % (row, j)
    if j < 0:
      return 'from_lane_below(%s[%d])' % (row, C + j)
    return 'from_lane_above(%s[%d])' % (row, j - C)

  for u in range(period):
    line('    {  // unrolled step %d' % u)
    for inst in insts:
      ctype = builtin_type(inst.c_type)
      if inst.stage is None:
        s = slot(inst, u, 0)
        line('      {  // load plane head+%d of %s' % (u, inst.tensor))
        line('        i64 zz = head + %d; if (zz > D - 1) zz = D - 1; if (zz < 0) zz = 0;' % u)
        line('        const %s* p = g_%s + zz * plane + row_base;' % (ctype, inst.tensor))
        line('        if (INTERIOR) {')
        for r in range(R):
          line('          { const %s v = *(const %s*)(p + row_dy[%d] * W + x);%s }' % (
              vec[inst.c_type], vec[inst.c_type], r,
              ''.join(' %s[%d][%d][%d] = v[%d];' % (inst.ident, s, r, c, c)
                      for c in range(C))))
        line('        } else {')
        # (recomputed per plane: see <kernel>_opaque above)
        line('          i64 xe = x; %s_opaque(xe);' % name)
        for r in range(R):
          for c in range(C):
            line('          %s[%d][%d][%d] = (xe + %d >= 0 && xe + %d < W) ? '
                 'p[row_dy[%d] * W + xe + %d] : (%s)0;' % (inst.ident, s, r, c, c, c, r, c, ctype))
        line('        }')
        line('      }')
        continue
      stage = inst.stage
      by_name = {(load_name, rel): src for src, rel, load_name in inst.reads}
      in_window = inst.keep > 0
      tile_name = 'tile_%s' % inst.ident
      if not in_window:
        line('      %s %s[%d][%d];' % (ctype, tile_name, R, C))
      cell = (lambda r, c, inst=inst, u=u: '%s[%d][%d][%d]' % (
          inst.ident, slot(inst, u, 0), r, c)) if in_window else \
          (lambda r, c, tile_name=tile_name: '%s[%d][%d]' % (tile_name, r, c))
      # rows whose whole dependency cone lies inside the tile; the others could only
      # produce halo garbage and are left as they are
      blo, bhi = stage_boxes[inst.iteration][stage['name']]
      for r in range(-blo[1], R - bhi[1]):
        for c in range(C):
          def load(tensor, rel, u=u, r=r, c=c, inst=inst, by_name=by_name):
            return operand(inst, by_name[(tensor, tuple(rel))], tuple(rel), u, r, c)
          cell_assignment(stage, cell(r, c), load, line, '      ')
      if inst.final:
        j = out_of[id(inst)]
        line('      {  // store plane head+%d-%d of %s' % (u, inst.lag, inst.tensor))
        if rect:
          # (with outputs and inputs in unequal numbers the compiler turns the address of
          # every stored row of every output into an induction variable of the plane loop,
          # a pair of scalar registers each, which the file does not have: the plane
          # number passes through the empty asm and the addresses are computed per plane)
          line('        i64 z = head + %d; %s_opaque_s(z);' % (u - inst.lag, name))
        else:
          line('        const i64 z = head + %d;' % (u - inst.lag))
        line('        if (n + %d >= n_lo%d && n + %d < n_hi%d) {' % (u, j, u, j))
        line('          %s* q = g_out%d + z * plane + row_base + x;' % (ctype, j))
        line('          int r_lo = r_lo%d, r_hi = r_hi%d; %s_opaque_s(r_lo); %s_opaque_s(r_hi);'
             % (j, j, name, name))
        line('          int lo = c_lo%d, hi = c_hi%d; %s_opaque(lo); %s_opaque(hi);'
             % (j, j, name, name))
        line('          if (lo == 0 && hi == %d) {' % C)
        for r in range(y_lo, R - y_hi):
          line('            if (%d >= r_lo && %d < r_hi) { %s v;%s *(%s*)(q + row_dy[%d] * W) = v; }'
               % (r, r, vec[inst.c_type],
                  ''.join(' v[%d] = %s;' % (c, cell(r, c)) for c in range(C)),
                  vec[inst.c_type], r))
        line('          } else {')
        for r in range(y_lo, R - y_hi):
          line('            if (%d >= r_lo && %d < r_hi) {%s }' % (
              r, r, ''.join(' if (%d >= lo && %d < hi) q[row_dy[%d] * W + %d] = %s;'
                                  % (c, c, r, c, cell(r, c)) for c in range(C))))
        line('          }')
        line('        }')
        line('      }')
    line('    }')
  line('  }')
  line('}')
  line('')
  occupancy = ''
  if waves_per_eu > 0:
    occupancy = ' __attribute__((amdgpu_waves_per_eu(%d, %d)))' % (waves_per_eu, waves_per_eu)
  line('GLOBAL WG_SIZE(%d)%s void %s(soda_hip_args a) {'
       % (WAVES_PER_BLOCK * LANES, occupancy, name))
  line('  const int lane = lane_id();')
  line('  const int wave = __builtin_amdgcn_workitem_id_x() >> 6;')
  line('  const %s_boxes b = %s_output_boxes(a);' % (name, name))
  # the union of the outputs' boxes is what tiles and chunks cover (the launcher sizes
  # the grid by the same rule: csrc/schedule.cpp, make_launch)
  line('  i64 lo[3], hi[3];')
  line('  for (int d = 0; d < 3; ++d) { lo[d] = b.lo[0][d]; hi[d] = b.hi[0][d]; }')
  for j in range(1, n_out):
    line('  for (int d = 0; d < 3; ++d) { if (b.lo[%d][d] < lo[d]) lo[d] = b.lo[%d][d]; '
         'if (b.hi[%d][d] > hi[d]) hi[d] = b.hi[%d][d]; }' % (j, j, j, j))
  line('  const i64 x_origin = lo[0] - lo[0] %% %d;' % C)
  line('  const i64 strip = (i64)__builtin_amdgcn_workgroup_id_x() * %d + wave;'
       % WAVES_PER_BLOCK)
  line('  const i64 xs = x_origin + strip * %d;' % w_out)
  line('  if (xs >= hi[0]) return;')
  line('  const i64 x = xs - %d + lane * %d;' % (halo_lo, C))
  line('  const i64 ys = lo[1] + (i64)__builtin_amdgcn_workgroup_id_y() * %d;' % r_out)
  line('  if (ys >= hi[1]) return;')
  line('  const i64 yb = ys - %d;' % y_lo)
  line('  const i64 chunk = a.param[0] > 0 ? a.param[0] : %d;' % chunk_planes)
  line('  const i64 z0 = lo[2] + (i64)__builtin_amdgcn_workgroup_id_z() * chunk;')
  line('  if (z0 >= hi[2]) return;')
  line('  const i64 z1 = z0 + chunk < hi[2] ? z0 + chunk : hi[2];')
  line('  const bool interior = xs - %d >= 0 && xs - %d + %d <= a.dims[0];'
       % (halo_lo, halo_lo, LANES * C))
  line('  if (interior) %s_tile<true>(a, b, xs, x, yb, z0, z1);' % name)
  line('  else %s_tile<false>(a, b, xs, x, yb, z0, z1);' % name)
  line('}')
  entry = dict(name=name, kind='fused', depth=depth, stage=-1,
               block=[WAVES_PER_BLOCK * LANES, 1, 1],
               tile=[WAVES_PER_BLOCK * w_out, r_out, chunk_planes, 1],
               origin_align=C, fill_rows=L + lo[2], cols=C, rows=R, prefetch=prefetch,
               period=period, est_vgprs=est_vgprs, w_out=w_out, r_out=r_out,
               halo=[geo['halo_lo'], geo['halo_hi']], fields=n_out)
  return '\n'.join(o) + '\n', entry
