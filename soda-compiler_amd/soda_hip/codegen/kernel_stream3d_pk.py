"""Fused 3-D kernels for 8- and 16-bit volumes: kernel_stream3d's construction with the
windows kept PACKED (kernel.generate's `packed_cells`).

kernel_stream3d keeps one VGPR per cell, whatever the cell's width: a `uint16` 7-point chain
in 8 x 8 tiles (16-byte lane loads) then asks for 280 registers at depth 1 and 472 at depth 2
and compiles at the 256-register ceiling, one wave per SIMD (docs/DESIGN_HISTORY.md).  Here

  * a window slot of a 1- or 2-byte instance is `unsigned w[keep][R][C*elem/4]`: the dwords
    as the lane's 8- or 16-byte vector load delivered them, nothing unpacked at load time; a
    4-byte local (the float intermediate of a 16-bit filter) keeps one register per cell;
  * an x-neighbour in the next lane comes through ONE wave shift of the dword that holds it,
    hoisted per row of the reading instance (a radius-2 `uint8` row: one shift per side);
  * a cell is extracted where it is used - `(T)(dword >> shift)`, T the element type, so the
    cast zero-extends unsigned types and sign-extends `int8` / `int16` and C's integer
    promotions are those of the reference's loop nest.  The stage's expression text stays
    that of cell_assignment: no packed 16-bit arithmetic (`/` and `>>` do not commute with
    16-bit wraparound); v_bfe, SDWA or shifts are the compiler's choice;
  * a narrow instance's row is assembled into dwords with shifts and ors; a final
    instance's row leaves as one 8- or 16-byte vector per lane, per cell only in lanes that
    straddle the store range.  Tiles overhanging the array build their dwords from guarded
    per-cell loads.

Everything else is kernel_stream3d: planes streamed along z, a (64*C) x R tile per
wavefront, tiles overlapping by the composed window, no LDS, no barrier, the same table
entry.  Depths 1 and 2.
"""
from . import kernel_common
from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_stream2d import LANES, WAVES_PER_BLOCK, NotFusable, rotation_period
from .kernel_stream3d import kernel_name, pipeline

MAX_DEPTH = 2
# (rows, columns) per lane by element width: lane loads of 8 or 16 bytes.  Eight rows: a
# wavefront alone exposes every plane's load latency, so what pays is wavefronts, not tile -
# measured at 512^3 / 256^3, depth 1 against the per-stage schedule (profiles/
# r19_packed3d.txt, the shape sweep): smooth3d 16 x 4 at two waves per SIMD 0.72 / 0.44 x,
# 12 x 4 at three 0.83 / 0.81 x, 8 x 4 at four 1.22 / 1.08 x; skewvol3d 16 x 8 0.82 / 0.76 x,
# 12 x 8 1.36 / 0.86 x, 8 x 8 1.57 / 1.03 x.  Taller tiles left the list.
TILE_SHAPES = {2: ((8, 8), (8, 4)), 1: ((8, 16), (8, 8))}
# (waves per SIMD, register budget): the occupancy levels kernel.packed3d_kernels tries, most
# waves first - the first level at which a shape fits is taken
OCCUPANCY_LEVELS = ((4, 128), (3, 168), (2, 240))
# what a lane holds besides its windows: addresses in flight, the cells and dwords of the row
# in the making, the dwords that crossed lanes (read off the compiler's resource reports under
# the occupancy attribute: 8 x 4 tiles 64 registers for 48 of windows and 120 for 96, 8 x 8
# uint8 tiles 75 for 64).  Those reports were of rows with no more crossing registers than
# the lane's own dwords.  A stage that reads several rows or tensors across the lane's edge
# crosses more (`crossings`, the count row_crossings() takes from the reads), and each such
# register costs about four: the shifted copy, what is extracted from it, and the same for
# the rows the compiler makes side by side - capped at two per cell of the row.  (Two int16
# inputs and a uint8 local in 8-column lanes, 8 crossing registers in the local's rows: 80
# registers of windows, 139 in all with no ceiling, 159 with a trivial output stage, 125
# with the same operands and no x offset.  36 on top of the windows made it a four-waves
# kernel that spilled 29 registers to scratch; 52 make it a three-waves kernel.)
def overhead_vgprs(rows, cols, dwords, crossings=0):
  beyond = min(4 * max(0, crossings - dwords), 2 * cols)
  return 2 * rows + cols + dwords + beyond + 8


def row_crossings(insts, cols):
  """The most registers of the two neighbour lanes that a row of `cols` cells of one stage
  reads: the wave shifts emit() hoists per row."""
  crossings = 0
  for inst in insts:
    if inst.stage is None:
      continue
    crossed = set()
    for src, rel, _ in inst.reads:
      per = 4 // specmod.ELEM_SIZE[src.c_type] if specmod.ELEM_SIZE[src.c_type] < 4 else 1
      for c in range(cols):
        j = c + rel[0]
        if j < 0 or j >= cols:
          crossed.add((src.ident, rel[1], rel[2], j < 0, (j % cols) // per))
    crossings = max(crossings, len(crossed))
  return crossings


_UNSIGNED = {1: 'unsigned char', 2: 'unsigned short'}


def class_refusal(spec):
  """Why the LOWERED program `spec` is outside the form's class; None if it is inside."""
  if spec['dim'] != 3:
    return 'the packed-cell form handles 3-D programs'
  if len(spec['outputs']) != 1:
    return 'the packed-cell form handles single-output programs'
  types = specmod.tensor_c_types(spec)
  ends = [t['c_type'] for t in spec['inputs']] + [types[spec['outputs'][0]]]
  if '_Float16' in types.values():
    return 'half is outside the packed-cell form'
  if len(set(specmod.ELEM_SIZE[t] for t in ends)) != 1:
    return 'inputs and output of different widths'
  if specmod.ELEM_SIZE[ends[0]] not in (1, 2):
    return 'the packed-cell form handles 1- and 2-byte elements'
  for name, c_type in types.items():
    if specmod.ELEM_SIZE[c_type] not in (1, 2, 4):
      return 'local %s has %d-byte elements' % (name, specmod.ELEM_SIZE[c_type])
  return None


def regs_per_row(c_type, cols):
  """Registers a lane spends on one row of `cols` cells: dwords for a narrow type."""
  return cols * min(4, specmod.ELEM_SIZE[c_type]) // 4


def tile_geometry(spec, depth, rows, cols):
  margins = specmod.iteration_margins(spec, depth)
  lo, hi = margins[-1] if len(spec['inputs']) == len(spec['outputs']) else margins[0]
  halo_lo = -(-lo[0] // cols) * cols
  halo_hi = -(-hi[0] // cols) * cols
  w_out = LANES * cols - halo_lo - halo_hi
  r_out = rows - lo[1] - hi[1]
  return dict(lo=lo, hi=hi, halo_lo=halo_lo, halo_hi=halo_hi, w_out=w_out, r_out=r_out,
              kept=max(0, w_out) * max(0, r_out) / float(LANES * cols * rows))


def shapes_by_kept_fraction(spec, depth):
  """The element width's tile shapes ordered by how much of the tile survives the halo (most
  first; among equals the larger tile), as kernel_fields3d.shapes_by_kept_fraction."""
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  return sorted(TILE_SHAPES.get(elem, ()),
                key=lambda s: (-tile_geometry(spec, depth, s[0], s[1])['kept'], -s[0] * s[1]))


def extract(dword, c_type, sub):
  """Cell `sub` of a packed dword, typed as the reference types it."""
  bits = 8 * specmod.ELEM_SIZE[c_type] * sub
  return '((%s)(%s%s))' % (builtin_type(c_type), dword, ' >> %d' % bits if bits else '')


def pack(cells, c_type, first):
  """The dword of the cells `first` ... of a row of typed values `cells`."""
  elem = specmod.ELEM_SIZE[c_type]
  parts = []
  for sub in range(4 // elem):
    text = '(unsigned)(%s)%s' % (_UNSIGNED[elem], cells(first + sub))
    parts.append('(%s << %d)' % (text, 8 * elem * sub) if sub else text)
  return ' | '.join(parts)


def emit(spec, depth, cols=8, rows=8, chunk_planes=64, prefetch=0, max_period=12,
         vgpr_budget=128, waves_per_eu=4, nt=0):
  """Returns (text, kernel table entry) for one fused depth; the entry has the fields of
  kernel_stream3d's.  nt: as there.  waves_per_eu: the occupancy the budget is for, said to
  the compiler - left to itself it schedules for one wave per SIMD (512 registers) and takes
  440 where 140 do."""
  why = class_refusal(spec)
  if why:
    raise NotFusable(why)
  if depth > MAX_DEPTH:
    raise NotFusable('the packed-cell form goes %d iterations deep' % MAX_DEPTH)
  types = specmod.tensor_c_types(spec)
  index = tensor_index(spec)
  in_type = spec['inputs'][0]['c_type']
  out_name = spec['outputs'][0]
  out_type = types[out_name]
  elem = specmod.ELEM_SIZE[in_type]
  if depth > 1 and (len(spec['inputs']) != 1 or in_type != out_type):
    raise NotFusable('depth > 1 needs one input feeding one output of its type')
  C, R = cols, rows
  if C * elem not in (8, 16):
    raise NotFusable('%d columns of %d bytes: lane loads are 8 or 16 bytes' % (C, elem))
  DW = C * elem // 4
  insts, final = pipeline(spec, depth, prefetch)
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
  period = rotation_period(insts, max_period)
  # dwords, not cells
  est_vgprs = sum(inst.keep * R * regs_per_row(inst.c_type, C) for inst in insts) + \
      overhead_vgprs(R, C, DW, row_crossings(insts, C))
  if est_vgprs > vgpr_budget:
    raise NotFusable('depth %d would need about %d VGPRs in %d x %d tiles (budget %d)'
                     % (depth, est_vgprs, R, C, vgpr_budget))
  stage_boxes = specmod.iteration_boxes(spec, depth)
  name = kernel_name(spec, depth)
  L = final.lag
  T_out = builtin_type(out_type)
  o = []
  line = o.append
  line('// fused depth-%d 3-D kernel, packed cells: tile %d x %d per wavefront (%d x %d out),'
       % (depth, LANES * C, R, w_out, r_out))
  line('// %d dwords per lane and row, rotation period %d, prefetch %d planes, ~%d VGPRs'
       % (DW, period, prefetch, est_vgprs))
  for inst in insts:
    line('//   %-18s lag %2d keep %2d%s' % (inst.ident, inst.lag, inst.keep,
                                           '  -> HBM' if inst.final else ''))
  vec = 'vec_%s' % name
  line('typedef unsigned %s __attribute__((ext_vector_type(%d), aligned(%d)));'
       % (vec, DW, elem))
  line('template <bool INTERIOR, bool NT = %s>' % ('true' if nt & 2 else 'false'))
  line('DEV void %s_tile(const soda_hip_args& a, const i64 xs, const int lane_x, '
       'const i64 yb, const i64 z0, const i64 z1) {' % name)
  line('  const i64 W = a.dims[0], H = a.dims[1], D = a.dims[2];')
  line('  const i64 plane = W * H;')
  line('  const i64 st_lo = xs > a.box_lo[0] ? xs : a.box_lo[0];')
  line('  const i64 st_hi = xs + %d < a.box_hi[0] ? xs + %d : a.box_hi[0];'
       % (w_out, w_out))
  # The wavefront's first column x0 is wave-uniform (the kernel's entry reads it with
  # readfirstlane), so a row's address is a scalar base plus the lane's 32-bit byte offset
  # (global_load ... v_offset, s[base]) and every guard compares 32-bit cells of the tile
  # row, lane_x + c, with scalars: the cells inside the array, the cells to store.
  line('  const i64 x0 = xs - %d;' % halo_lo)
  line('  const unsigned lane_bytes = (unsigned)lane_x * %d;' % elem)
  line('  const int in_lo = x0 < 0 ? (int)-x0 : 0;')
  line('  const int in_hi = W - x0 < %d ? (int)(W - x0) : %d;' % (LANES * C, LANES * C))
  line('  const int cs_lo = (int)(st_lo - x0), cs_hi = (int)(st_hi - x0);')
  # A tile overhanging the array (every tile of an array up to two tiles wide): the lanes
  # whose cells all lie inside load their vector as an interior lane does, a lane that
  # straddles the array's edge - one per side at most - loads cell by cell, guarded, and
  # the lanes outside hold zeros (they feed halo cells only).  The same three ways out:
  # a vector per lane inside the store range, guarded cells where a lane straddles it,
  # nothing from the halo lanes.
  line('  const bool ld_vec = INTERIOR || (lane_x >= in_lo && lane_x + %d <= in_hi);' % C)
  line('  const bool ld_part = !ld_vec && lane_x + %d > in_lo && lane_x < in_hi;' % C)
  line('  const bool st_vec = lane_x >= cs_lo && lane_x + %d <= cs_hi;' % C)
  line('  const bool st_part = !st_vec && lane_x + %d > cs_lo && lane_x < cs_hi;' % C)
  # rows of the tile, clamped into the array (clamped rows only feed halo cells)
  line('  i64 row_y[%d];' % R)
  for r in range(R):
    line('  { i64 y = yb + %d; y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y); '
         'row_y[%d] = y * W; }' % (r, r))
  for t in spec['inputs']:
    line('  const %s* __restrict__ g_%s = (const %s*)a.tensor[%d];' % (
        builtin_type(t['c_type']), t['name'], builtin_type(t['c_type']),
        index[t['name']]))
  line('  %s* __restrict__ g_out = (%s*)a.tensor[%d];' % (T_out, T_out, index[out_name]))

  def packed(inst):
    return specmod.ELEM_SIZE[inst.c_type] < 4

  for inst in insts:
    if inst.keep:
      line('  %s %s[%d][%d][%d];' % (
          'unsigned' if packed(inst) else builtin_type(inst.c_type), inst.ident,
          inst.keep, R, regs_per_row(inst.c_type, C)))
  for inst in insts:
    for k in range(inst.keep):
      for r in range(R):
        line('  ' + ' '.join('%s[%d][%d][%d] = 0;' % (inst.ident, k, r, c)
                             for c in range(regs_per_row(inst.c_type, C))))
  line('  i64 head = z0 - %d;' % lo[2])
  line('  const i64 steps = (z1 - z0) + %d;' % (L + lo[2]))
  line('  for (i64 n = 0; n < steps; n += %d, head += %d) {' % (period, period))

  def slot(inst, u, back):
    return (u - back) % inst.keep

  def operand(reader, src, rel, u, r, c, crossings, own):
    """The operand text of one read; a register of the neighbour lane goes through
    `crossings`, {(side, register text): variable}, hoisted by the caller."""
    back = reader.lag - src.lag - rel[2]
    assert 0 <= back < src.keep, (reader.ident, src.ident, rel, back, src.keep)
    rr = min(max(r + rel[1], 0), R - 1)      # clamped rows are halo rows
    row = '%s[%d][%d]' % (src.ident, slot(src, u, back), rr)
    per = 4 // specmod.ELEM_SIZE[src.c_type] if packed(src) else 1
    j = c + rel[0]
    side = None
    if j < 0:
      side, j = 'below', C + j
    elif j >= C:
      side, j = 'above', j - C
    reg = '%s[%d]' % (row, j // per)
    if packed(src):
      own.add(reg)
    if side:
      key = (side, reg)
      if key not in crossings:
        crossings[key] = 'pk_%s%d' % (side[0], len(crossings))
      reg = crossings[key]
    return extract(reg, src.c_type, j % per) if packed(src) else reg

  for u in range(period):
    line('    {  // unrolled step %d' % u)
    for inst in insts:
      ctype = builtin_type(inst.c_type)
      if inst.stage is None:
        s = slot(inst, u, 0)
        per = 4 // elem
        line('      {  // load plane head+%d of %s' % (u, inst.tensor))
        line('        i64 zz = head + %d; if (zz > D - 1) zz = D - 1;' % u)
        line('        const %s* p = g_%s + zz * plane;' % (ctype, inst.tensor))
        line('        if (INTERIOR) {')
        for r in range(R):
          line('          { const %s v = *(const %s*)((const char*)(p + row_y[%d] + x0) + '
               'lane_bytes);%s }' % (
              vec, vec, r, ''.join(' %s[%d][%d][%d] = v[%d];' % (
                  inst.ident, s, r, d, d) for d in range(DW))))
        line('        } else {')
        for r in range(R):
          line('          { const %s* pr = (const %s*)((const char*)(p + row_y[%d] + x0) + '
               'lane_bytes);' % (ctype, ctype, r))
          line('            if (ld_vec) { const %s v = *(const %s*)pr;%s }' % (
              vec, vec, ''.join(' %s[%d][%d][%d] = v[%d];' % (inst.ident, s, r, d, d)
                                for d in range(DW))))
          line('            else if (ld_part) {')
          for d in range(DW):
            line('              %s[%d][%d][%d] = %s;' % (inst.ident, s, r, d, pack(
                lambda c: '((lane_x + %d >= in_lo && lane_x + %d < in_hi) ? pr[%d] : (%s)0)'
                % (c, c, c, ctype), inst.c_type, d * per)))
          line('            } else {%s }' % ''.join(
              ' %s[%d][%d][%d] = 0;' % (inst.ident, s, r, d) for d in range(DW)))
          line('          }')
        line('        }')
        line('      }')
        continue
      stage = inst.stage
      by_name = {}
      for src, rel, load_name in inst.reads:
        by_name[(load_name, rel)] = src
      per = 4 // specmod.ELEM_SIZE[inst.c_type] if packed(inst) else 1
      if inst.final:
        line('      const i64 z = head + %d;  // store plane head+%d-%d' % (u - L, u, L))
        line('      const bool z_stored = z >= z0 && z < z1;')
        line('      %s* q = g_out + z * plane;' % T_out)
      # rows whose whole dependency cone lies inside the tile; the others could
      # only produce halo garbage and are left at zero
      blo, bhi = stage_boxes[inst.iteration][stage['name']]
      for r in range(-blo[1], R - bhi[1]):
        crossings, own, body = {}, set(), []
        for c in range(C):
          def load(tensor, rel, u=u, r=r, c=c, inst=inst, by_name=by_name,
                   crossings=crossings, own=own):
            return operand(inst, by_name[(tensor, tuple(rel))], tuple(rel), u, r, c,
                           crossings, own)
          target = 'cell[%d]' % c if packed(inst) else \
              '%s[%d][%d][%d]' % (inst.ident, slot(inst, u, 0), r, c)
          cell_assignment(stage, target, load, body.append, '        ')
        line('      {  // row %d of %s' % (r, inst.ident))
        # The packed registers the row reads, made opaque: the compiler would otherwise keep
        # every extracted cell for its later readers - the rows below, the next planes'
        # steps of the unrolled loop - and so unpack the whole window into registers after
        # all.  No instruction; each row extracts what it reads (SDWA / v_bfe operands).
        for reg in sorted(own):
          line('        asm("" : "+v"(%s));' % reg)
        # one wave shift per neighbour register the row needs, every lane active
        for (side, reg), var in crossings.items():
          line('        const auto %s = from_lane_%s(%s);' % (var, side, reg))
        if packed(inst):
          line('        %s cell[%d];' % (ctype, C))
        o.extend(body)
        if packed(inst) and not inst.final:
          for d in range(C // per):
            line('        %s[%d][%d][%d] = %s;' % (
                inst.ident, slot(inst, u, 0), r, d,
                pack(lambda c: 'cell[%d]' % c, inst.c_type, d * per)))
        if inst.final and y_lo <= r < R - y_hi:
          line('        if (z_stored && yb + %d >= a.box_lo[1] && yb + %d < a.box_hi[1]) {'
               % (r, r))
          line('          %s* qr = (%s*)((char*)(q + row_y[%d] + x0) + lane_bytes);'
               % (T_out, T_out, r))
          line('          if (st_vec) {')
          line('            %s v;%s' % (vec, ''.join(
              ' v[%d] = %s;' % (d, pack(lambda c: 'cell[%d]' % c, inst.c_type, d * per))
              for d in range(DW))))
          if nt & 6:
            line('            if (NT) __builtin_nontemporal_store(v, (%s*)qr); '
                 'else *(%s*)qr = v;' % (vec, vec))
          else:
            line('            *(%s*)qr = v;' % vec)
          line('          } else if (st_part) {')
          for c in range(C):
            line('            if (lane_x + %d >= cs_lo && lane_x + %d < cs_hi) '
                 'qr[%d] = cell[%d];' % (c, c, c, c))
          line('          }')
          line('        }')
        line('      }')
    line('    }')
  line('  }')
  line('}')
  line('')
  occupancy = ''
  if waves_per_eu > 0:
    occupancy = ' __attribute__((amdgpu_waves_per_eu(%d, %d)))' % (waves_per_eu,
                                                                   waves_per_eu)
  line('GLOBAL WG_SIZE(%d)%s void %s(soda_hip_args a) {'
       % (WAVES_PER_BLOCK * LANES, occupancy, name))
  line('  const int lane = lane_id();')
  # (wave-uniform, and said so: the strip's columns and `interior` then live in scalar
  # registers and the paths below are branches, not masks)
  line('  const int wave = __builtin_amdgcn_readfirstlane('
       '__builtin_amdgcn_workitem_id_x() >> 6);')
  line('  const i64 x_origin = a.box_lo[0] - a.box_lo[0] %% %d;' % C)
  line('  const i64 strip = (i64)__builtin_amdgcn_workgroup_id_x() * %d + wave;'
       % WAVES_PER_BLOCK)
  line('  const i64 xs = x_origin + strip * %d;' % w_out)
  line('  if (xs >= a.box_hi[0]) return;')
  line('  const int lane_x = lane * %d;' % C)
  line('  const i64 yb = a.box_lo[1] + (i64)__builtin_amdgcn_workgroup_id_y() * %d'
       ' - %d;' % (r_out, y_lo))
  line('  const i64 chunk = a.param[0] > 0 ? a.param[0] : %d;' % chunk_planes)
  line('  const i64 z0 = a.box_lo[2] + (i64)__builtin_amdgcn_workgroup_id_z() * chunk;')
  line('  const i64 z1 = z0 + chunk < a.box_hi[2] ? z0 + chunk : a.box_hi[2];')
  line('  const bool interior = xs - %d >= 0 && xs - %d + %d <= a.dims[0];'
       % (halo_lo, halo_lo, LANES * C))
  if nt & 4:
    cell_bytes = sum(specmod.ELEM_SIZE[types[n]] for n in
                     [t['name'] for t in spec['inputs']] + list(spec['outputs']))
    line('  const bool streaming = (a.box_hi[0] - a.box_lo[0]) * (a.box_hi[1] - a.box_lo[1]) '
         '* (a.box_hi[2] - a.box_lo[2]) * %d > %dll;' % (
             cell_bytes, kernel_common.NT_STREAMING_BYTES))
    line('  if (interior && streaming) %s_tile<true, true>(a, xs, lane_x, yb, z0, z1);' % name)
    line('  else if (interior) %s_tile<true>(a, xs, lane_x, yb, z0, z1);' % name)
  else:
    line('  if (interior) %s_tile<true>(a, xs, lane_x, yb, z0, z1);' % name)
  line('  else %s_tile<false>(a, xs, lane_x, yb, z0, z1);' % name)
  line('}')
  entry = dict(name=name, kind='fused', depth=depth, stage=-1,
               block=[WAVES_PER_BLOCK * LANES, 1, 1],
               tile=[WAVES_PER_BLOCK * w_out - C, r_out, chunk_planes, 1],
               fill_rows=L + lo[2], cols=C, rows=R, prefetch=prefetch,
               period=period, est_vgprs=est_vgprs, w_out=w_out, r_out=r_out)
  if nt:
    entry['nt'] = int(nt)
  return '\n'.join(o) + '\n', entry
