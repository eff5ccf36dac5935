"""Fused depth-1 3-D kernels for windows wider than a lane's columns: the plane that is
read in-plane lives in LDS, the z column in registers ("LDS planes").

The register forms (kernel_stream3d and its relatives) take x neighbours by DPP from the
adjacent lane and stop at |dx| <= C; a radius-r window also costs them 2r of a tile's rows.
High-order stars (the 8th-order Laplacian, iso3dfd) therefore get this shape instead:

  * a workgroup of W wavefronts owns TX x TY output cells and streams z.  Lane l holds C
    consecutive columns (one 16-byte vector) of RW consecutive rows; TX / C lanes make a
    row, so a wavefront owns a band of RW * 64 * C / TX rows and TY = W times that;
  * per input that is read off the z axis the lane keeps its OWN cells of the z window
    [zlo, zhi] in registers, one more plane being loaded ahead: reads (0, 0, dz) are
    registers;
  * the one plane `zc` that is read at (dx, dy) != (0, 0) lies in an LDS slot with its x / y
    halo.  The lanes write their own cells there from the registers they hold anyway; the
    halo ring is fetched one plane ahead, through registers.  Two slots, one barrier per
    plane: step n computes from slot n % 2 and fills slot (n + 1) % 2;
  * in-plane neighbours are read from LDS as whole aligned 16-byte vectors, each once per
    lane and step: the RW rows of a lane share their y neighbours, and what falls into the
    lane's own cells is not read at all;
  * inputs read only at (0, 0, 0) (a velocity model, u_prev) go from global memory to
    registers, one plane ahead: no LDS, no window.

Scope: one stage that is the one output, any number of inputs, one element width of 4 or 8
bytes, and per input ONE plane offset at which it is read off the z axis.  Depth 1 only.
Array edges as in kernel_stream3d: loads clamped into the array on all six sides, stores
inside the box only, any array size.

`fields=True` is the form over SEVERAL outputs, `<app>_fused_k1lf`: two or three stages that
are all outputs and read inputs only, in a multi_field program (a wave time loop: the new
field, the old field and the velocity model handed on) or a rectangular one (a high-order
gradient).  A Field is then the union of every stage's reads of that input.  Each output has
a box of its own under kernel_fields3d's contract: the launch's box is the intersection,
param[1 + j] carries output j's six extras, tiles and z chunks cover the union, and output
j stores a cell only inside j's box on all three axes.  An output that is one load at
(0, 0, 0) of an input of its own type is stored straight from the window registers.
"""
from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_fields3d import MAX_OUTPUTS
from .kernel_stream2d import LANES, NotFusable, multi_field, rectangular

LDS_CAP = 65536
# (wavefronts, rows per lane, lanes per tile row) that emit() chooses from when the caller
# names none: shapes_by_loaded_cells
SHAPES = tuple((w, rw, lx) for w in (8, 4) for rw in (4, 2, 1) for lx in (64, 32, 16))


def kernel_name(spec, fields=False):
  return '%s_fused_k1l%s' % (spec['app_name'], 'f' if fields else '')


class Field:
  """How the stage reads one input: its z window, and what it reads in the plane `zc`."""

  def __init__(self, name, c_type, rels):
    self.name, self.c_type, self.rels = name, c_type, rels
    off = [r for r in rels if (r[0], r[1]) != (0, 0)]
    planes = sorted({r[2] for r in off})
    if len(planes) > 1:
      raise NotFusable('input %s is read off the z axis at plane offsets %s: one plane of an '
                       'input lies in LDS' % (name, ' and '.join(map(str, planes))))
    self.lds = bool(off)
    self.zc = planes[0] if off else None
    self.zlo, self.zhi = min(r[2] for r in rels), max(r[2] for r in rels)
    self.keep = self.zhi - self.zlo + 2          # the window and the plane loaded ahead
    self.hx = (max([0] + [-r[0] for r in off]), max([0] + [r[0] for r in off]))
    self.hy = (max([0] + [-r[1] for r in off]), max([0] + [r[1] for r in off]))


def analyse(spec):
  """(stage, [Field]) of a program in scope; NotFusable names what keeps it out."""
  if spec['dim'] != 3:
    raise NotFusable('the LDS-plane form handles 3-D programs')
  if len(spec['outputs']) != 1:
    raise NotFusable('%d outputs: the LDS-plane form stores one' % len(spec['outputs']))
  if len(spec['stages']) != 1:
    raise NotFusable('%d stages: the LDS-plane form takes one stage, the output'
                     % len(spec['stages']))
  types = specmod.tensor_c_types(spec)
  widths = sorted({specmod.ELEM_SIZE[t] for t in types.values()})
  if len(widths) > 1:
    raise NotFusable('mixed element widths')
  if widths[0] not in (4, 8):
    raise NotFusable('%d-byte elements: the LDS-plane form handles 4- and 8-byte ones'
                     % widths[0])
  stage = spec['stages'][0]
  fields = []
  for t in spec['inputs']:
    rels = [tuple(rel) for name, rel in stage['loads'] if name == t['name']]
    if rels:
      fields.append(Field(t['name'], t['c_type'], rels))
  if not any(f.lds for f in fields):
    raise NotFusable('no read off the z axis: nothing for an LDS plane to share')
  return stage, fields


def analyse_fields(spec):
  """(stages, [Field]) of a program in the scope of the form over several outputs."""
  if spec['dim'] != 3:
    raise NotFusable('the LDS-plane form handles 3-D programs')
  if not 2 <= len(spec['outputs']) <= MAX_OUTPUTS:
    raise NotFusable('%d outputs: the LDS-plane form over fields stores 2 to %d'
                     % (len(spec['outputs']), MAX_OUTPUTS))
  produced = [s['name'] for s in spec['stages']]
  for stage in spec['stages']:
    for name, _ in stage['loads']:
      if name in produced:
        raise NotFusable('stage %s reads stage %s: the LDS-plane form over fields takes '
                         'stages that read inputs only' % (stage['name'], name))
  if produced != list(spec['outputs']):
    raise NotFusable('%d stages for %d outputs: the LDS-plane form over fields takes stages '
                     'that are outputs' % (len(produced), len(spec['outputs'])))
  if not (multi_field(spec) or rectangular(spec)):
    raise NotFusable('iterate %d over %d input(s) and %d output(s) that do not feed each '
                     'other pairwise' % (spec['iterate'], len(spec['inputs']),
                                         len(spec['outputs'])))
  types = specmod.tensor_c_types(spec)
  widths = sorted({specmod.ELEM_SIZE[t] for t in types.values()})
  if len(widths) > 1:
    raise NotFusable('mixed element widths')
  if widths[0] not in (4, 8):
    raise NotFusable('%d-byte elements: the LDS-plane form handles 4- and 8-byte ones'
                     % widths[0])
  fields = []
  for t in spec['inputs']:
    rels = []
    for stage in spec['stages']:
      rels += [tuple(rel) for name, rel in stage['loads']
               if name == t['name'] and tuple(rel) not in rels]
    if rels:
      fields.append(Field(t['name'], t['c_type'], rels))
  if not any(f.lds for f in fields):
    raise NotFusable('no read off the z axis: nothing for an LDS plane to share')
  return spec['stages'], fields


def passed_through(spec, stage):
  """The input an output hands on unchanged - one load at (0, 0, 0) of an input of the
  output's own type - or None."""
  loads = [(name, tuple(rel)) for name, rel in stage['loads']]
  if stage['lets'] or len(loads) != 1 or loads[0][1] != (0, 0, 0):
    return None
  name = loads[0][0]
  if stage['expr'].strip('() ') != '{%s:0,0,0}' % name:
    return None
  types = {t['name']: t['c_type'] for t in spec['inputs']}
  return name if types.get(name) == stage['c_type'] else None


def geometry(fields, elem, waves, rows, lanes_x):
  """Tile, LDS slot and halo of one shape, all in cells."""
  C = 16 // elem
  shared = [f for f in fields if f.lds]
  hx = [max(f.hx[s] for f in shared) for s in (0, 1)]
  hy = [max(f.hy[s] for f in shared) for s in (0, 1)]
  hxl, hxh = -(-hx[0] // C) * C, -(-hx[1] // C) * C      # whole vectors
  tx, ty = lanes_x * C, waves * (LANES // lanes_x) * rows
  pitch, slot_rows = hxl + tx + hxh, hy[0] + ty + hy[1]
  return dict(C=C, TX=tx, TY=ty, HXL=hxl, HXH=hxh, HYL=hy[0], HYH=hy[1], PITCH=pitch,
              ROWS=slot_rows, threads=waves * LANES,
              halo_vectors=(slot_rows * pitch - tx * ty) // C,
              lds_bytes=len(shared) * 2 * slot_rows * pitch * elem,
              loaded=slot_rows * pitch / float(tx * ty))


def lds_vectors(fields, C, rows):
  """The (field, row, vector) triples a lane reads from LDS per step: every in-plane read of
  every one of its cells, less what lies in its own cells."""
  seen = []
  for f in fields:
    for dx, dy, dz in f.rels:
      if (dx, dy) == (0, 0):
        continue
      for r in range(rows):
        for c in range(C):
          key = (f.name, r + dy, (c + dx) // C)
          if not (key[2] == 0 and 0 <= key[1] < rows) and key not in seen:
            seen.append(key)
  return seen


def estimate_vgprs(fields, elem, geo, rows, computed=1):
  """`computed`: the outputs whose cells are computed (all but those passed through)."""
  per, C = max(1, elem // 4), geo['C']
  shared = [f for f in fields if f.lds]
  halo_loads = -(-geo['halo_vectors'] // geo['threads'])
  return (sum(f.keep for f in fields) * rows * C * per +     # windows, planes ahead
          len(lds_vectors(fields, C, rows)) * 4 +            # neighbours out of LDS
          computed * rows * C * per +                        # the output cells
          halo_loads * (4 * len(shared) + 5) + 24)           # halo ring and its addresses


def shapes_by_loaded_cells(spec, shapes=SHAPES, fields=False):
  """The shapes ordered by cells loaded over cells stored, (TX + hx)(TY + hy) / (TX TY),
  least first (among equals as listed: more wavefronts, taller lanes first)."""
  _, fields = analyse_fields(spec) if fields else analyse(spec)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  return sorted(shapes, key=lambda s: geometry(fields, elem, *s)['loaded'])


def rotation(fields, max_period):
  """(period, {field: slots}): an EVEN unroll period (the LDS slot of a step is then known
  when the text is printed) of which every field's slot count is a divisor."""
  best = None
  for period in range(2, max_period + 1, 2):
    if max(f.keep for f in fields) > period:
      continue
    divisors = [d for d in range(1, period + 1) if period % d == 0]
    slots = {f.name: min(d for d in divisors if d >= f.keep) for f in fields}
    cost = (sum(slots.values()), period)
    if best is None or cost < best[0]:
      best = (cost, period, slots)
  if best is None:
    raise NotFusable('z window deeper than the rotation period limit %d' % max_period)
  return best[1], best[2]


def emit(spec, depth=1, waves=None, rows=None, lanes_x=None, chunk_planes=64,
         max_period=16, vgpr_budget=250, fields=False):
  """Returns (text, kernel table entry).  Without a shape: the first of
  shapes_by_loaded_cells that fits the register budget and the LDS cap.  `fields`: the
  form over several outputs, each stored inside its own box."""
  if depth != 1:
    raise NotFusable('the LDS-plane form is depth 1')
  several = bool(fields)
  if several:
    stages, fields = analyse_fields(spec)
  else:
    stage, fields = analyse(spec)
    stages = [stage]
  types = specmod.tensor_c_types(spec)
  index = tensor_index(spec)
  out_name = spec['outputs'][0]
  elem = specmod.ELEM_SIZE[types[out_name]]
  # per output, the input it hands on unchanged (stored from the window, no cells of its own)
  through = [passed_through(spec, st) if several else None for st in stages]
  if waves is None:
    error = None
    for shape in shapes_by_loaded_cells(spec, fields=several):
      try:
        return emit(spec, depth, *shape, chunk_planes=chunk_planes, max_period=max_period,
                    vgpr_budget=vgpr_budget, fields=several)
      except NotFusable as e:
        error = error or e
    raise error
  geo = geometry(fields, elem, waves, rows, lanes_x)
  C, RW, LX, NT = geo['C'], rows, lanes_x, geo['threads']
  TX, TY, HXL, HXH, HYL, HYH = (geo[k] for k in ('TX', 'TY', 'HXL', 'HXH', 'HYL', 'HYH'))
  PITCH, ROWS = geo['PITCH'], geo['ROWS']
  shape_text = '%d x %d tiles (%d wavefronts, %d rows per lane)' % (TX, TY, waves, RW)
  if geo['lds_bytes'] > LDS_CAP:
    raise NotFusable('%s would need %d bytes of LDS (cap %d)' % (shape_text, geo['lds_bytes'],
                                                                  LDS_CAP))
  est_vgprs = estimate_vgprs(fields, elem, geo, RW, computed=through.count(None))
  if est_vgprs > vgpr_budget:
    raise NotFusable('%s would need about %d VGPRs (budget %d)' % (shape_text, est_vgprs,
                                                                    vgpr_budget))
  period, slots = rotation(fields, max_period)
  fill = max(f.zhi - f.zlo + 1 for f in fields)
  shared = [f for f in fields if f.lds]
  name = kernel_name(spec, several)
  T_out = builtin_type(types[out_name])
  n_out = len(stages)
  # the halo ring of a slot as a list of vectors: the rows above and below at full pitch,
  # then the vectors left and right of the tile's own rows
  PV, TXV, HXLV, SV = PITCH // C, TX // C, HXL // C, (HXL + HXH) // C
  NTB, NH = (HYL + HYH) * PV, geo['halo_vectors']
  assert NH == NTB + TY * SV and NH > 0
  K = -(-NH // NT)
  by_name = {f.name: f for f in fields}

  o = []
  line = o.append
  line('// fused depth-1 3-D kernel%s, LDS planes: %s, halo x %d+%d y %d+%d,'
       % (' over %d outputs' % n_out if several else '', shape_text, HXL, HXH, HYL, HYH))
  line('// %d bytes of LDS, rotation period %d, %d planes walked before the first stored one, '
       '~%d VGPRs' % (geo['lds_bytes'], period, fill, est_vgprs))
  for f in fields:
    line('//   %-12s z window [%d, %d] in %d register slots%s' % (
        f.name, f.zlo, f.zhi, slots[f.name],
        ', plane %+d in LDS' % f.zc if f.lds else ''))
  vec, lvec = {}, {}
  for c_type in sorted({f.c_type for f in fields} | {st['c_type'] for st in stages}):
    vec[c_type] = 'vec_%s_%s' % (name, c_type)
    lvec[c_type] = 'lvec_%s_%s' % (name, c_type)
    line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(%d)));'
         % (builtin_type(c_type), vec[c_type], C, elem))
    line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(16)));'
         % (builtin_type(c_type), lvec[c_type], C))
  if several:
    # which of its cells a lane stores does not change along the plane loop: hoisted out of
    # it, each such condition would stay a 64-bit lane mask in a pair of SGPRs, for every
    # row, column and output - more than the scalar file has.  Passed through an empty asm
    # the lane's bits are opaque and the conditions are computed where they are used
    # (kernel_fields3d: the same device)
    line('template <typename T> DEV void %s_opaque(T& v) { asm volatile("" : "+v"(v)); }'
         % name)
  line('template <bool INTERIOR>')
  line('DEV void %s_tile(const soda_hip_args& a, %sconst i64 xs, const i64 ys, const i64 z0, '
       'const i64 z1, const int tid%s) {' % (name, ''.join(
           'const int cells%d, const int sn_lo%d, const int sn_hi%d, ' % (j, j, j)
           for j in range(n_out if several else 0)), ''.join(
           ', %s (*lds_%s)[%d][%d]' % (builtin_type(f.c_type), f.name, ROWS, PITCH)
           for f in shared)))
  line('  const i64 W = a.dims[0], H = a.dims[1], D = a.dims[2];')
  line('  const i64 plane = W * H;')
  line('  const int lx = tid %% %d, ly = tid / %d * %d;' % (LX, LX, RW))
  line('  const i64 x = xs + lx * %d, y = ys + ly;' % C)
  for f in fields:
    T = builtin_type(f.c_type)
    line('  const %s* __restrict__ g_%s = (const %s*)a.tensor[%d];' % (T, f.name, T,
                                                                      index[f.name]))
  if not several:
    line('  %s* __restrict__ g_out = (%s*)a.tensor[%d];' % (T_out, T_out, index[out_name]))
  for j, st in enumerate(stages if several else ()):
    T = builtin_type(st['c_type'])
    line('  %s* __restrict__ g_out%d = (%s*)a.tensor[%d];' % (T, j, T, index[st['name']]))
  # the lane's own rows and columns, clamped into the array (what a clamp changes feeds only
  # cells outside the box)
  line('  i64 row_off[%d], col[%d];' % (RW, C))
  for r in range(RW):
    line('  { i64 yy = y + %d; if (!INTERIOR) yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy); '
         'row_off[%d] = yy * W; }' % (r, r))
  for c in range(C):
    line('  { i64 xx = x + %d; if (!INTERIOR) xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx); '
         'col[%d] = xx; }' % (c, c))
  # the halo vectors this work-item fetches: where each lies in a slot and in a plane
  line('  int h_lds[%d]; i64 h_row[%d], h_x[%d];' % (K, K, K))
  for k in range(K):
    line('  {')
    line('    const int idx = tid + %d;' % (k * NT))
    line('    int row, vcol;')
    top = 'const int rh = idx / %d; vcol = idx %% %d; row = rh < %d ? rh : rh + %d;' % (
        PV, PV, HYL, TY)
    side = 'const int j = idx - %d; row = %d + j / %d; const int sv = j %% %d; ' \
        'vcol = sv < %d ? sv : sv + %d;' % (NTB, HYL, max(SV, 1), max(SV, 1), HXLV, TXV)
    if NTB and SV:
      line('    if (idx < %d) { %s } else { %s }' % (NTB, top, side))
    else:
      line('    { %s }' % (top if NTB else side))
    # (a work-item beyond the list keeps a position inside the slot and the plane: it
    # neither loads nor writes, the guard is `tid + k * threads < vectors`)
    line('    if (idx >= %d) { row = 0; vcol = 0; }' % NH)
    line('    h_lds[%d] = row * %d + vcol * %d;' % (k, PITCH, C))
    line('    i64 yy = ys - %d + row; if (!INTERIOR) yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);'
         % HYL)
    line('    h_row[%d] = yy * W; h_x[%d] = xs - %d + vcol * %d;' % (k, k, HXL, C))
    line('  }')
  for f in fields:
    T = builtin_type(f.c_type)
    line('  %s w_%s[%d][%d][%d];' % (T, f.name, slots[f.name], RW, C))
    for s in range(slots[f.name]):
      for r in range(RW):
        line('  ' + ' '.join('w_%s[%d][%d][%d] = 0;' % (f.name, s, r, c) for c in range(C)))
  line('  const i64 steps = (z1 - z0) + %d;' % fill)
  line('  for (i64 n = 0; n < steps; n += %d) {' % period)

  def own(f, u, dz, r, c):
    """The lane's own cell of plane z + dz at unrolled step u (z = the step's output plane;
    the plane z + zhi + 1 is the one the step loads)."""
    back = f.zhi + 1 - dz
    assert 0 <= back < slots[f.name], (f.name, dz, back)
    return 'w_%s[%d][%d][%d]' % (f.name, (u - back) % slots[f.name], r, c)

  def clamped_plane(expr):
    return 'i64 zz = %s; zz = zz < 0 ? 0 : (zz > D - 1 ? D - 1 : zz);' % expr

  for u in range(period):
    line('    {  // unrolled step %d: output plane z, slot %d read, slot %d filled' % (
        u, u % 2, (u + 1) % 2))
    if u:
      line('      if (n + %d >= steps) break;' % u)      # the whole workgroup leaves together
    line('      const i64 z = z0 + n + %d;' % (u - fill))
    for f in fields:
      T = builtin_type(f.c_type)
      line('      {  // own cells of plane z%+d of %s, one plane ahead' % (f.zhi + 1, f.name))
      line('        %s' % clamped_plane('z + %d' % (f.zhi + 1)))
      line('        const %s* p = g_%s + zz * plane;' % (T, f.name))
      for r in range(RW):
        cells = [own(f, u, f.zhi + 1, r, c) for c in range(C)]
        line('        if (INTERIOR) { const %s v = *(const %s*)(p + row_off[%d] + x);%s }' % (
            vec[f.c_type], vec[f.c_type], r,
            ''.join(' %s = v[%d];' % (cell, c) for c, cell in enumerate(cells))))
        line('        else {%s }' % ''.join(' %s = p[row_off[%d] + col[%d]];' % (cell, r, c)
                                           for c, cell in enumerate(cells)))
      line('      }')
    for f in shared:
      T = builtin_type(f.c_type)
      line('      %s halo_%s[%d];' % (lvec[f.c_type], f.name, K))
      line('      {  // halo ring of plane z%+d of %s' % (f.zc + 1, f.name))
      line('        %s' % clamped_plane('z + %d' % (f.zc + 1)))
      line('        const %s* p = g_%s + zz * plane;' % (T, f.name))
      for k in range(K):
        guard = '' if (k + 1) * NT <= NH else 'if (tid + %d < %d) ' % (k * NT, NH)
        line('        halo_%s[%d] = 0;' % (f.name, k))
        line('        %s{' % guard)
        line('          if (INTERIOR) { const %s v = *(const %s*)(p + h_row[%d] + h_x[%d]);%s }' % (
            vec[f.c_type], vec[f.c_type], k, k,
            ''.join(' halo_%s[%d][%d] = v[%d];' % (f.name, k, c, c) for c in range(C))))
        line('          else {%s }' % ''.join(
            ' { i64 xx = h_x[%d] + %d; xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx); '
            'halo_%s[%d][%d] = p[h_row[%d] + xx]; }' % (k, c, f.name, k, c, k)
            for c in range(C)))
        line('        }')
      line('      }')
    # compute: every step from the first one whose window is complete
    line('      if (n + %d >= %d) {' % (u, fill))
    wanted = lds_vectors(fields, C, RW)
    for fname, ry, vi in wanted:
      f = by_name[fname]
      line('        const %s l_%s_%s_%s = *(const %s*)&lds_%s[%d][%d + ly + %d][%d + lx * %d + %d];'
           % (lvec[f.c_type], fname, str(ry).replace('-', 'm'), str(vi).replace('-', 'm'),
              lvec[f.c_type], fname, u % 2, HYL, ry, HXL, C, vi * C))
    def load_of(u, r, c):
      def load(tensor, rel):
        f = by_name[tensor]
        dx, dy, dz = rel
        if (dx, dy) == (0, 0):
          return own(f, u, dz, r, c)
        ry, vi, e = r + dy, (c + dx) // C, (c + dx) % C
        if vi == 0 and 0 <= ry < RW:
          return own(f, u, dz, ry, e)
        return 'l_%s_%s_%s[%d]' % (tensor, str(ry).replace('-', 'm'),
                                   str(vi).replace('-', 'm'), e)
      return load

    if not several:
      line('        %s out_cells[%d][%d];' % (T_out, RW, C))
      for r in range(RW):
        for c in range(C):
          cell_assignment(stage, 'out_cells[%d][%d]' % (r, c), load_of(u, r, c), line,
                          '        ')
      line('        %s* q = g_out + z * plane;' % T_out)
      for r in range(RW):
        line('        if (y + %d >= a.box_lo[1] && y + %d < a.box_hi[1]) {' % (r, r))
        line('          if (x >= a.box_lo[0] && x + %d <= a.box_hi[0]) {' % C)
        line('            %s v;%s *(%s*)(q + row_off[%d] + x) = v;' % (
            vec[types[out_name]], ''.join(' v[%d] = out_cells[%d][%d];' % (c, r, c)
                                          for c in range(C)), vec[types[out_name]], r))
        line('          } else {')
        for c in range(C):
          line('            if (x + %d >= a.box_lo[0] && x + %d < a.box_hi[0]) '
               'q[row_off[%d] + x + %d] = out_cells[%d][%d];' % (c, c, r, c, r, c))
        line('          }')
        line('        }')
    if several:
      line('        const int m = (int)n + %d;' % u)
    for j, st in enumerate(stages if several else ()):
      # output j: the planes, rows and columns of its own box
      T, V = builtin_type(st['c_type']), vec[st['c_type']]
      line('        int mine%d = m >= sn_lo%d && m < sn_hi%d ? cells%d : 0; %s_opaque(mine%d);'
           % (j, j, j, j, name, j))
      line('        if (mine%d) {  // %s' % (j, st['name']))
      if through[j] is None:
        line('          %s out_cells[%d][%d];' % (T, RW, C))
        for r in range(RW):
          for c in range(C):
            cell_assignment(st, 'out_cells[%d][%d]' % (r, c), load_of(u, r, c), line,
                            '          ')
        cell = lambda r, c: 'out_cells[%d][%d]' % (r, c)
      else:     # handed on: the lane's own cells of plane z, as they lie in the window
        cell = lambda r, c, f=by_name[through[j]], u=u: own(f, u, 0, r, c)
      line('          %s* q = g_out%d + z * plane;' % (T, j))
      for r in range(RW):
        whole = ((1 << C) - 1) << (r * C)
        line('          if (mine%d & %d) {' % (j, whole))
        line('            if ((mine%d & %d) == %d) {' % (j, whole, whole))
        line('              %s v;%s *(%s*)(q + row_off[%d] + x) = v;' % (
            V, ''.join(' v[%d] = %s;' % (c, cell(r, c)) for c in range(C)), V, r))
        line('            } else {')
        for c in range(C):
          line('              if (mine%d & %d) q[row_off[%d] + x + %d] = %s;' % (
              j, 1 << (r * C + c), r, c, cell(r, c)))
        line('            }')
        line('          }')
      line('        }')
    line('      }')
    # the other slot gets the next step's plane: own cells from the window, halo ring
    for f in shared:
      for r in range(RW):
        line('      { %s v;%s *(%s*)&lds_%s[%d][%d + ly + %d][%d + lx * %d] = v; }' % (
            lvec[f.c_type], ''.join(' v[%d] = %s;' % (c, own(f, u, f.zc + 1, r, c))
                                    for c in range(C)),
            lvec[f.c_type], f.name, (u + 1) % 2, HYL, r, HXL, C))
      for k in range(K):
        guard = '' if (k + 1) * NT <= NH else 'if (tid + %d < %d) ' % (k * NT, NH)
        line('      %s*(%s*)(&lds_%s[%d][0][0] + h_lds[%d]) = halo_%s[%d];' % (
            guard, lvec[f.c_type], f.name, (u + 1) % 2, k, f.name, k))
    line('      soda_block_barrier();')
    line('    }')
  line('  }')
  line('}')
  line('')
  line('GLOBAL WG_SIZE(%d) void %s(soda_hip_args a) {' % (NT, name))
  for f in shared:
    line('  __attribute__((shared, aligned(16))) %s lds_%s[2][%d][%d];' % (
        builtin_type(f.c_type), f.name, ROWS, PITCH))
  line('  const int tid = __builtin_amdgcn_workitem_id_x();')
  lo, hi = ['a.box_lo[%d]' % d for d in range(3)], ['a.box_hi[%d]' % d for d in range(3)]
  if several:
    # the union of the outputs' boxes is what tiles and chunks cover (the launcher sizes
    # the grid by the same rule: csrc/schedule.cpp, make_launch)
    lo, hi = ['lo%d' % d for d in range(3)], ['hi%d' % d for d in range(3)]
    for d in range(3):
      for side, shift, sign in (('lo', 8 * d, '-'), ('hi', 24 + 8 * d, '+')):
        line('  i64 %s%d = 0;' % (side, d))
        for j in range(n_out):
          line('  { const i64 e = (a.param[%d] >> %d) & 255; if (e > %s%d) %s%d = e; }'
               % (1 + j, shift, side, d, side, d))
        line('  %s%d = a.box_%s[%d] %s %s%d;' % (side, d, side, d, sign, side, d))
  line('  const i64 x_origin = %s - %s %% %d;' % (lo[0], lo[0], C))
  line('  const i64 xs = x_origin + (i64)__builtin_amdgcn_workgroup_id_x() * %d;' % TX)
  line('  const i64 ys = %s + (i64)__builtin_amdgcn_workgroup_id_y() * %d;' % (lo[1], TY))
  line('  const i64 chunk = a.param[0] > 0 ? a.param[0] : %d;' % chunk_planes)
  line('  const i64 z0 = %s + (i64)__builtin_amdgcn_workgroup_id_z() * chunk;' % lo[2])
  # (the same for every work-item of the workgroup: nobody waits at a barrier for them)
  line('  if (xs >= %s || ys >= %s || z0 >= %s) return;' % tuple(hi))
  line('  const i64 z1 = z0 + chunk < %s ? z0 + chunk : %s;' % (hi[2], hi[2]))
  # the box of output j: the launch's box widened by the extras of param[1 + j], each
  # bound computed where it is used (eighteen 64-bit bounds kept would fill the scalar file)
  def box_lo(j, d):
    return '(a.box_lo[%d] - ((a.param[%d] >> %d) & 255))' % (d, 1 + j, 8 * d)

  def box_hi(j, d):
    return '(a.box_hi[%d] + ((a.param[%d] >> %d) & 255))' % (d, 1 + j, 24 + 8 * d)

  def within(what, first, size):
    """`what` as a distance from `first`, clamped into [0, size]"""
    return '(int)(%s - %s < 0 ? 0 : %s - %s > %s ? %s : %s - %s)' % (
        what, first, what, first, size, size, what, first)

  if several:
    line('  const int lx = tid %% %d, ly = tid / %d * %d;' % (LX, LX, RW))
  for j in range(n_out if several else 0):
    # what output j stores of this tile and chunk, worked out here, once for both paths, and
    # kept in three VECTOR registers per output (the one-output form leaves a dozen scalar
    # registers free, fewer than the bounds of three boxes).  Columns and rows: which of
    # the lane's own cells lie in j's box, bit r * C + c.  Planes: the steps of the plane
    # loop that compute them (step m computes plane z0 + m - fill)
    line('  int cells%d = 0;' % j)
    line('  {')
    line('    const int sx_lo = %s, sx_hi = %s;' % (within(box_lo(j, 0), 'xs', TX),
                                                  within(box_hi(j, 0), 'xs', TX)))
    line('    const int sy_lo = %s, sy_hi = %s;' % (within(box_lo(j, 1), 'ys', TY),
                                                  within(box_hi(j, 1), 'ys', TY)))
    for r in range(RW):
      line('    if (ly + %d >= sy_lo && ly + %d < sy_hi) {%s }' % (r, r, ''.join(
          ' if (lx * %d + %d >= sx_lo && lx * %d + %d < sx_hi) cells%d |= %d;'
          % (C, c, C, c, j, 1 << (r * C + c)) for c in range(C))))
    line('  }')
    line('  int sn_lo%d = %s + %d, sn_hi%d = %s + %d;' % (
        j, within(box_lo(j, 2), 'z0', '(z1 - z0)'), fill,
        j, within(box_hi(j, 2), 'z0', '(z1 - z0)'), fill))
    line('  %s_opaque(cells%d); %s_opaque(sn_lo%d); %s_opaque(sn_hi%d);'
         % (name, j, name, j, name, j))
  line('  const bool interior = xs - %d >= 0 && xs + %d <= a.dims[0] && '
       'ys - %d >= 0 && ys + %d <= a.dims[1];' % (HXL, TX + HXH, HYL, TY + HYH))
  args = 'a, %sxs, ys, z0, z1, tid%s' % (
      ''.join('cells%d, sn_lo%d, sn_hi%d, ' % (j, j, j) for j in range(n_out if several else 0)),
      ''.join(', lds_%s' % f.name for f in shared))
  line('  if (interior) %s_tile<true>(%s);' % (name, args))
  line('  else %s_tile<false>(%s);' % (name, args))
  line('}')
  loaded = len(shared) * ROWS * PITCH + (len(fields) - len(shared)) * TX * TY
  entry = dict(name=name, kind='fused', depth=1, stage=-1, block=[NT, 1, 1],
               tile=[TX, TY, chunk_planes, 1], origin_align=C, fill_rows=fill, cols=C,
               rows=RW, w_out=TX, r_out=TY, period=period, est_vgprs=est_vgprs,
               lds_bytes=geo['lds_bytes'], lds_planes=len(shared), waves=waves,
               halo=[HXL, HXH, HYL, HYH], loaded_cells=loaded)
  if several:
    entry['fields'] = n_out
  return '\n'.join(o) + '\n', entry
