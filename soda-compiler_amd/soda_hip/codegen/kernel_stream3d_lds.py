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
bytes, and per input ONE plane offset at which it is read off the z axis (several with
`ring=True`, below).  Depth 1 only.
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

`ring=True` lifts the one-plane condition of both forms, `<app>_fused_k1r` and `_k1rf`
(mixed derivatives d2/dxdz, lopsided windows, coupled fields).  An input read off the z axis
in the planes `planes`, plo = min, phi = max, gets a RING of S = phi - plo + 2 LDS slots:
at the step of output plane z they hold the planes z + plo .. z + phi, gaps nobody reads
included, and the step fills the slot of plane z + phi + 1 - own cells from the window
registers, the halo ring from the registers fetched at this step.  That slot held plane
z + plo - 1 (or an earlier one), last read one step and one barrier ago: one barrier per
plane still suffices.  The unroll period is a common multiple of every register slot count
and every S, either padded up to a divisor (ring_rotation), so every slot index stays a
literal; the two-slot form above is the case S = 2.  The halos hx / hy are hulls over all
planes; the lane's own cells are never read from LDS, in any plane.  The ring may take the
CU's whole LDS (RING_LDS_CAP); the two single-plane forms keep LDS_CAP.
"""
import types

from . import spec as specmod
from .kernel_common import builtin_type, cell_assignment, tensor_index
from .kernel_fields3d import MAX_OUTPUTS
from .kernel_stream2d import LANES, NotFusable, multi_field, rectangular

LDS_CAP = 65536
RING_LDS_CAP = 163840          # of the plane-ring form: the LDS of a gfx950 CU
# (wavefronts, rows per lane, lanes per tile row) that emit() chooses from when the caller
# names none: shapes_by_loaded_cells
SHAPES = tuple((w, rw, lx) for w in (8, 4) for rw in (4, 2, 1) for lx in (64, 32, 16))


def kernel_name(spec, fields=False, ring=False):
  return '%s_fused_k1%s%s' % (spec['app_name'], 'r' if ring else 'l', 'f' if fields else '')


class Field:
  """How the stage reads one input: its z window, and what it reads in the plane `zc` - with
  `ring` in the planes `planes`, of which [plo, phi] is the hull: the planes that lie in LDS."""

  def __init__(self, name, c_type, rels, ring=False):
    self.name, self.c_type, self.rels = name, c_type, rels
    off = [r for r in rels if (r[0], r[1]) != (0, 0)]
    planes = sorted({r[2] for r in off})
    if len(planes) > 1 and not ring:
      raise NotFusable('input %s is read off the z axis at plane offsets %s: one plane of an '
                       'input lies in LDS' % (name, ' and '.join(map(str, planes))))
    self.lds = bool(off)
    self.zc = planes[0] if off else None
    self.planes = planes
    self.plo, self.phi = (planes[0], planes[-1]) if off else (None, None)
    # LDS slots: the planes z + plo .. z + phi a step reads and the one it fills
    self.lds_slots = self.phi - self.plo + 2 if off else 0
    self.zlo, self.zhi = min(r[2] for r in rels), max(r[2] for r in rels)
    self.keep = self.zhi - self.zlo + 2          # the window and the plane loaded ahead
    self.hx = (max([0] + [-r[0] for r in off]), max([0] + [r[0] for r in off]))
    self.hy = (max([0] + [-r[1] for r in off]), max([0] + [r[1] for r in off]))


def analyse(spec, fields=False, ring=False):
  """(stages, [Field]) of a program in scope; NotFusable names what keeps it out.  `fields`:
  the scope of the form over several outputs, where a Field is the union of every stage's
  reads of that input.  `ring`: an input may be read off the z axis in several planes."""
  if spec['dim'] != 3:
    raise NotFusable('the LDS-plane form handles 3-D programs')
  if fields:
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
  else:
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
  found = []
  for t in spec['inputs']:
    rels = []
    for stage in spec['stages']:
      rels += [tuple(rel) for name, rel in stage['loads']
               if name == t['name'] and tuple(rel) not in rels]
    if rels:
      found.append(Field(t['name'], t['c_type'], rels, ring))
  if not any(f.lds for f in found):
    raise NotFusable('no read off the z axis: nothing for an LDS plane to share')
  return spec['stages'], found


def analyse_fields(spec):
  return analyse(spec, fields=True)


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


def planes_off_axis(spec):
  """{input: the sorted z offsets at which the program reads it at (dx, dy) != (0, 0)} of a
  3-D program."""
  planes = {t['name']: set() for t in spec['inputs']}
  for stage in spec['stages']:
    for name, rel in stage['loads']:
      if name in planes and (rel[0], rel[1]) != (0, 0):
        planes[name].add(rel[2])
  return {name: sorted(p) for name, p in planes.items()}


def geometry(fields, elem, waves, rows, lanes_x, lds_slots=None):
  """Tile, LDS slot and halo of one shape, all in cells.  `lds_slots`: {input: slots} of the
  plane ring; two slots per input without it."""
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
              lds_bytes=sum(lds_slots[f.name] if lds_slots else 2 for f in shared) *
              slot_rows * pitch * elem,
              loaded=slot_rows * pitch / float(tx * ty))


def lds_vectors(fields, C, rows, ring=False):
  """The (field, row, vector) triples a lane reads from LDS per step: every in-plane read of
  every one of its cells, less what lies in its own cells.  `ring`: (field, plane, row,
  vector), a vector of every plane apart."""
  seen = []
  for f in fields:
    for dx, dy, dz in f.rels:
      if (dx, dy) == (0, 0):
        continue
      for r in range(rows):
        for c in range(C):
          row, vi = r + dy, (c + dx) // C
          key = (f.name, dz, row, vi) if ring else (f.name, row, vi)
          if not (vi == 0 and 0 <= row < rows) and key not in seen:
            seen.append(key)
  return seen


def estimate_vgprs(fields, elem, geo, rows, computed=1, ring=False):
  """`computed`: the outputs whose cells are computed (all but those passed through)."""
  per, C = max(1, elem // 4), geo['C']
  shared = [f for f in fields if f.lds]
  halo_loads = -(-geo['halo_vectors'] // geo['threads'])
  # the plane-ring form also counts the sums in flight: the compiler interleaves the chains
  # of a lane's RW x C cells, some four partial terms per cell register.  Without them the
  # estimate was 21 to 68 registers short of hipcc's count at two and four rows per lane
  # (cross3d 233 for 268, skewcross3d 242 for 302) and the first shape by loaded cells
  # spilled; with them it is at most 9 below and 15 above it for the three samples in every
  # shape that fits
  in_flight = 4 * rows * C * per if ring else 0
  return (sum(f.keep for f in fields) * rows * C * per + in_flight +  # windows, planes ahead
          len(lds_vectors(fields, C, rows, ring)) * 4 +      # neighbours out of LDS
          computed * rows * C * per +                        # the output cells
          halo_loads * (4 * len(shared) + 5) + 24)           # halo ring and its addresses


def shapes_by_loaded_cells(spec, shapes=SHAPES, fields=False, ring=False):
  """The shapes ordered by cells loaded over cells stored, (TX + hx)(TY + hy) / (TX TY),
  least first (among equals as listed: more wavefronts, taller lanes first)."""
  _, fields = analyse(spec, fields, ring)
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


def ring_rotation(fields, max_period, lds_slots_cap):
  """(period, {field: register slots}, {shared field: LDS slots}) of the plane-ring form: the
  period is a common multiple of all of them, so that the register slot and the LDS slot of
  every access are known when the text is printed.  A count is padded up to a divisor of the
  period, LDS slots no further than `lds_slots_cap` in all; registers are the scarcer, so
  the fewest register slots win, then the fewest LDS slots, then the shortest period."""
  shared = [f for f in fields if f.lds]
  best = None
  for period in range(2, max_period + 1):
    if max(max(f.keep, f.lds_slots) for f in fields) > period:
      continue
    divisors = [d for d in range(1, period + 1) if period % d == 0]
    slots = {f.name: min(d for d in divisors if d >= f.keep) for f in fields}
    lds_slots = {f.name: min(d for d in divisors if d >= f.lds_slots) for f in shared}
    if sum(lds_slots.values()) > lds_slots_cap:
      continue
    cost = (sum(slots.values()), sum(lds_slots.values()), period)
    if best is None or cost < best[0]:
      best = (cost, period, slots, lds_slots)
  if best is None:
    raise NotFusable('z window deeper than the rotation period limit %d' % max_period)
  return best[1:]


def fit(fields, elem, computed, shape, max_period, vgpr_budget, ring=False):
  """The figures of one shape - its geometry, estimated VGPRs and rotation - as the record
  the printers share; NotFusable where it exceeds the LDS cap, the register budget or the
  rotation period limit."""
  k = types.SimpleNamespace(waves=shape[0], RW=shape[1], LX=shape[2], ring=ring)
  shared = [f for f in fields if f.lds]
  k.lds_slots = {f.name: f.lds_slots if ring else 2 for f in shared}
  vars(k).update(geometry(fields, elem, *shape, lds_slots=k.lds_slots))
  k.shape_text = '%d x %d tiles (%d wavefronts, %d rows per lane)' % (k.TX, k.TY, k.waves, k.RW)
  cap = RING_LDS_CAP if ring else LDS_CAP
  if k.lds_bytes > cap:
    raise NotFusable('%s would need %d bytes of LDS (cap %d)' % (k.shape_text, k.lds_bytes,
                                                                  cap))
  k.est_vgprs = estimate_vgprs(fields, elem, vars(k), k.RW, computed=computed, ring=ring)
  if k.est_vgprs > vgpr_budget:
    raise NotFusable('%s would need about %d VGPRs (budget %d)' % (k.shape_text, k.est_vgprs,
                                                                    vgpr_budget))
  if ring:
    slot_bytes = k.ROWS * k.PITCH * elem
    k.period, k.slots, k.lds_slots = ring_rotation(fields, max_period, cap // slot_bytes)
    k.lds_bytes = sum(k.lds_slots.values()) * slot_bytes
  else:
    k.period, k.slots = rotation(fields, max_period)
  return k


def first_fit(spec, several, fits, ring=False):
  """fits(shape) of the first of shapes_by_loaded_cells that it does not refuse; when all are
  refused, the FIRST shape's error."""
  error = None
  for shape in shapes_by_loaded_cells(spec, fields=several, ring=ring):
    try:
      return fits(shape)
    except NotFusable as e:
      error = error or e
  raise error


def clamp(v, n):
  """The index `v` clamped into [0, n - 1]."""
  return '%s < 0 ? 0 : (%s > %s - 1 ? %s - 1 : %s)' % (v, v, n, n, v)


def clamped_plane(expr):
  return 'i64 zz = %s; zz = %s;' % (expr, clamp('zz', 'D'))


def halo_guard(k, i):
  """The guard of a work-item's i-th halo vector, where that may lie beyond the list."""
  if (i + 1) * k.threads <= k.halo_vectors:
    return ''
  return 'if (tid + %d < %d) ' % (i * k.threads, k.halo_vectors)


def lds_vector(field, row, vi, dz=None):
  """The vector `vi` of row `row`, relative to the lane's own, read from `field`'s plane -
  in the plane-ring form from its plane z + `dz`."""
  name = lambda v: str(v).replace('-', 'm')
  if dz is None:
    return 'l_%s_%s_%s' % (field, name(row), name(vi))
  return 'l_%s_p%s_%s_%s' % (field, name(dz), name(row), name(vi))


def lds_slot(k, f, u, dz):
  """The LDS slot in which plane z + dz of `f` lies at unrolled step u, phi + 1 being the
  plane the step fills.  Two slots, one plane: u % 2 is read, (u + 1) % 2 is filled."""
  assert f.plo <= dz <= f.phi + 1
  return (u + dz - f.plo) % k.lds_slots[f.name]


def own(k, f, u, dz, r, c):
  """The lane's own cell of plane z + dz at unrolled step u (z = the step's output plane;
  the plane z + zhi + 1 is the one the step loads)."""
  back = f.zhi + 1 - dz
  assert 0 <= back < k.slots[f.name], (f.name, dz, back)
  return 'w_%s[%d][%d][%d]' % (f.name, (u - back) % k.slots[f.name], r, c)


def load_of(k, u, r, c):
  """A stage's loads for the lane's cell (r, c) at step u: window registers, LDS vectors."""
  def load(tensor, rel):
    f = k.by_name[tensor]
    dx, dy, dz = rel
    if (dx, dy) == (0, 0):
      return own(k, f, u, dz, r, c)
    ry, vi, e = r + dy, (c + dx) // k.C, (c + dx) % k.C
    if vi == 0 and 0 <= ry < k.RW:
      return own(k, f, u, dz, ry, e)
    return '%s[%d]' % (lds_vector(tensor, ry, vi, dz if k.ring else None), e)
  return load


def print_header(k, line):
  """The comment that describes the kernel, and the vector types of its tensors."""
  line('// fused depth-1 3-D kernel%s, LDS %s: %s, halo x %d+%d y %d+%d,'
       % (k.over, 'plane ring' if k.ring else 'planes', k.shape_text, k.HXL, k.HXH, k.HYL,
          k.HYH))
  line('// %d bytes of LDS, rotation period %d, %d planes walked before the first stored one, '
       '~%d VGPRs' % (k.lds_bytes, k.period, k.fill, k.est_vgprs))
  for f in k.fields:
    in_lds = ''
    if f.lds and k.ring:
      in_lds = ', planes %+d to %+d in %d LDS slots' % (f.plo, f.phi, k.lds_slots[f.name])
    elif f.lds:
      in_lds = ', plane %+d in LDS' % f.zc
    line('//   %-12s z window [%d, %d] in %d register slots%s' % (
        f.name, f.zlo, f.zhi, k.slots[f.name], in_lds))
  for c_type in sorted({f.c_type for f in k.fields} | {st['c_type'] for st in k.stages}):
    k.vec[c_type] = 'vec_%s_%s' % (k.name, c_type)
    k.lvec[c_type] = 'lvec_%s_%s' % (k.name, c_type)
    line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(%d)));'
         % (builtin_type(c_type), k.vec[c_type], k.C, k.elem))
    line('typedef %s %s __attribute__((ext_vector_type(%d), aligned(16)));'
         % (builtin_type(c_type), k.lvec[c_type], k.C))
  if k.masks:
    # which of its cells a lane stores does not change along the plane loop: hoisted out of
    # it, each such condition would stay a 64-bit lane mask in a pair of SGPRs, for every
    # row, column and output - more than the scalar file has.  Passed through an empty asm
    # the lane's bits are opaque and the conditions are computed where they are used
    # (kernel_fields3d: the same device)
    line('template <typename T> DEV void %s_opaque(T& v) { asm volatile("" : "+v"(v)); }'
         % k.name)


def print_tile_prologue(k, line):
  """The tile function up to its plane loop: addresses, clamped rows and columns, windows."""
  C, RW, K = k.C, k.RW, k.K
  line('template <bool INTERIOR>')
  line('DEV void %s_tile(const soda_hip_args& a, %sconst i64 xs, const i64 ys, const i64 z0, '
       'const i64 z1, const int tid%s) {' % (k.name, ''.join(
           'const int %s, ' % m for m in k.masks), ''.join(
           ', %s (*lds_%s)[%d][%d]' % (builtin_type(f.c_type), f.name, k.ROWS, k.PITCH)
           for f in k.shared)))
  line('  const i64 W = a.dims[0], H = a.dims[1], D = a.dims[2];')
  line('  const i64 plane = W * H;')
  line('  const int lx = tid %% %d, ly = tid / %d * %d;' % (k.LX, k.LX, RW))
  line('  const i64 x = xs + lx * %d, y = ys + ly;' % C)
  for f in k.fields:
    T = builtin_type(f.c_type)
    line('  const %s* __restrict__ g_%s = (const %s*)a.tensor[%d];' % (T, f.name, T,
                                                                      k.index[f.name]))
  for pointer, st in zip(k.out_pointers, k.stages):
    T = builtin_type(st['c_type'])
    line('  %s* __restrict__ %s = (%s*)a.tensor[%d];' % (T, pointer, T, k.index[st['name']]))
  # the lane's own rows and columns, clamped into the array (what a clamp changes feeds only
  # cells outside the box)
  line('  i64 row_off[%d], col[%d];' % (RW, C))
  for r in range(RW):
    line('  { i64 yy = y + %d; if (!INTERIOR) yy = %s; row_off[%d] = yy * W; }'
         % (r, clamp('yy', 'H'), r))
  for c in range(C):
    line('  { i64 xx = x + %d; if (!INTERIOR) xx = %s; col[%d] = xx; }'
         % (c, clamp('xx', 'W'), c))
  # the halo vectors this work-item fetches: where each lies in a slot and in a plane.  The
  # halo ring of a slot as a list of vectors: the rows above and below at full pitch, then
  # the vectors left and right of the tile's own rows
  PV, TXV, HXLV, SV = k.PITCH // C, k.TX // C, k.HXL // C, (k.HXL + k.HXH) // C
  NTB = (k.HYL + k.HYH) * PV
  assert k.halo_vectors == NTB + k.TY * SV
  line('  int h_lds[%d]; i64 h_row[%d], h_x[%d];' % (K, K, K))
  for i in range(K):
    line('  {')
    line('    const int idx = tid + %d;' % (i * k.threads))
    line('    int row, vcol;')
    top = 'const int rh = idx / %d; vcol = idx %% %d; row = rh < %d ? rh : rh + %d;' % (
        PV, PV, k.HYL, k.TY)
    side = 'const int j = idx - %d; row = %d + j / %d; const int sv = j %% %d; ' \
        'vcol = sv < %d ? sv : sv + %d;' % (NTB, k.HYL, max(SV, 1), max(SV, 1), HXLV, TXV)
    if NTB and SV:
      line('    if (idx < %d) { %s } else { %s }' % (NTB, top, side))
    else:
      line('    { %s }' % (top if NTB else side))
    # (a work-item beyond the list keeps a position inside the slot and the plane: it
    # neither loads nor writes, the guard is `tid + k * threads < vectors`)
    line('    if (idx >= %d) { row = 0; vcol = 0; }' % k.halo_vectors)
    line('    h_lds[%d] = row * %d + vcol * %d;' % (i, k.PITCH, C))
    line('    i64 yy = ys - %d + row; if (!INTERIOR) yy = %s;' % (k.HYL, clamp('yy', 'H')))
    line('    h_row[%d] = yy * W; h_x[%d] = xs - %d + vcol * %d;' % (i, i, k.HXL, C))
    line('  }')
  for f in k.fields:
    line('  %s w_%s[%d][%d][%d];' % (builtin_type(f.c_type), f.name, k.slots[f.name], RW, C))
    for s in range(k.slots[f.name]):
      for r in range(RW):
        line('  ' + ' '.join('w_%s[%d][%d][%d] = 0;' % (f.name, s, r, c) for c in range(C)))
  line('  const i64 steps = (z1 - z0) + %d;' % k.fill)
  line('  for (i64 n = 0; n < steps; n += %d) {' % k.period)


def print_loads_ahead(k, line, u):
  """Every input's own cells of the plane after its window, into the window's free slot."""
  for f in k.fields:
    T, V = builtin_type(f.c_type), k.vec[f.c_type]
    line('      {  // own cells of plane z%+d of %s, one plane ahead' % (f.zhi + 1, f.name))
    line('        %s' % clamped_plane('z + %d' % (f.zhi + 1)))
    line('        const %s* p = g_%s + zz * plane;' % (T, f.name))
    for r in range(k.RW):
      cells = [own(k, f, u, f.zhi + 1, r, c) for c in range(k.C)]
      line('        if (INTERIOR) { const %s v = *(const %s*)(p + row_off[%d] + x);%s }' % (
          V, V, r, ''.join(' %s = v[%d];' % (cell, c) for c, cell in enumerate(cells))))
      line('        else {%s }' % ''.join(' %s = p[row_off[%d] + col[%d]];' % (cell, r, c)
                                         for c, cell in enumerate(cells)))
    line('      }')


def print_halo_fetch(k, line):
  """The halo ring of the plane the step's LDS fill writes, into registers."""
  for f in k.shared:
    T, V = builtin_type(f.c_type), k.vec[f.c_type]
    line('      %s halo_%s[%d];' % (k.lvec[f.c_type], f.name, k.K))
    line('      {  // halo ring of plane z%+d of %s' % (f.phi + 1, f.name))
    line('        %s' % clamped_plane('z + %d' % (f.phi + 1)))
    line('        const %s* p = g_%s + zz * plane;' % (T, f.name))
    for i in range(k.K):
      line('        halo_%s[%d] = 0;' % (f.name, i))
      line('        %s{' % halo_guard(k, i))
      line('          if (INTERIOR) { const %s v = *(const %s*)(p + h_row[%d] + h_x[%d]);%s }' % (
          V, V, i, i,
          ''.join(' halo_%s[%d][%d] = v[%d];' % (f.name, i, c, c) for c in range(k.C))))
      line('          else {%s }' % ''.join(
          ' { i64 xx = h_x[%d] + %d; xx = %s; halo_%s[%d][%d] = p[h_row[%d] + xx]; }'
          % (i, c, clamp('xx', 'W'), f.name, i, c, i) for c in range(k.C)))
      line('        }')
    line('      }')


def print_lds_reads(k, line, u):
  """The in-plane neighbours of the lane's cells, as whole vectors from the slot u % 2 - in
  the plane-ring form from the slot of each vector's plane."""
  for key in lds_vectors(k.fields, k.C, k.RW, k.ring):
    fname, ry, vi = key[0], key[-2], key[-1]
    f = k.by_name[fname]
    dz = key[1] if k.ring else f.zc
    V = k.lvec[f.c_type]
    line('        const %s %s = *(const %s*)&lds_%s[%d][%d + ly + %d][%d + lx * %d + %d];'
         % (V, lds_vector(fname, ry, vi, dz if k.ring else None), V, fname,
            lds_slot(k, f, u, dz), k.HYL, ry, k.HXL, k.C, vi * k.C))


def print_compute(k, line, stage, u, indent):
  """The lane's RW x C cells of one stage, into out_cells."""
  line('%s%s out_cells[%d][%d];' % (indent, builtin_type(stage['c_type']), k.RW, k.C))
  for r in range(k.RW):
    for c in range(k.C):
      cell_assignment(stage, 'out_cells[%d][%d]' % (r, c), load_of(k, u, r, c), line, indent)


def store_in_launch_box(k, line, u):
  """One output, stored inside the launch's box a.box_lo/hi."""
  stage, = k.stages
  T, V, C = builtin_type(stage['c_type']), k.vec[stage['c_type']], k.C
  print_compute(k, line, stage, u, '        ')
  line('        %s* q = %s + z * plane;' % (T, k.out_pointers[0]))
  for r in range(k.RW):
    line('        if (y + %d >= a.box_lo[1] && y + %d < a.box_hi[1]) {' % (r, r))
    line('          if (x >= a.box_lo[0] && x + %d <= a.box_hi[0]) {' % C)
    line('            %s v;%s *(%s*)(q + row_off[%d] + x) = v;' % (
        V, ''.join(' v[%d] = out_cells[%d][%d];' % (c, r, c) for c in range(C)), V, r))
    line('          } else {')
    for c in range(C):
      line('            if (x + %d >= a.box_lo[0] && x + %d < a.box_hi[0]) '
           'q[row_off[%d] + x + %d] = out_cells[%d][%d];' % (c, c, r, c, r, c))
    line('          }')
    line('        }')


def store_in_own_boxes(k, line, u):
  """Several outputs, each inside its own box: the lane masks cells<j>, sn_lo<j>, sn_hi<j>."""
  C = k.C
  line('        const int m = (int)n + %d;' % u)
  for j, st in enumerate(k.stages):
    T, V = builtin_type(st['c_type']), k.vec[st['c_type']]
    line('        int mine%d = m >= sn_lo%d && m < sn_hi%d ? cells%d : 0; %s_opaque(mine%d);'
         % (j, j, j, j, k.name, j))
    line('        if (mine%d) {  // %s' % (j, st['name']))
    if k.through[j] is None:
      print_compute(k, line, st, u, '          ')
      cell = lambda r, c: 'out_cells[%d][%d]' % (r, c)
    else:     # handed on: the lane's own cells of plane z, as they lie in the window
      cell = lambda r, c, f=k.by_name[k.through[j]]: own(k, f, u, 0, r, c)
    line('          %s* q = %s + z * plane;' % (T, k.out_pointers[j]))
    for r in range(k.RW):
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


def print_lds_fill(k, line, u):
  """The other slot gets the next step's plane: own cells from the window, halo ring."""
  for f in k.shared:
    V = k.lvec[f.c_type]
    slot = lds_slot(k, f, u, f.phi + 1)
    if k.ring:
      # the slot held plane z + plo - 1 or, in a padded ring, an earlier one: nobody has read
      # it since the step before this one, and that step's barrier lies between - one barrier
      # per plane still suffices
      line('      // plane z%+d of %s into the slot of plane z%+d: last read %d step(s) ago, a '
           'barrier lies between' % (f.phi + 1, f.name, f.phi + 1 - k.lds_slots[f.name],
                                     k.lds_slots[f.name] - (f.phi - f.plo + 1)))
    for r in range(k.RW):
      line('      { %s v;%s *(%s*)&lds_%s[%d][%d + ly + %d][%d + lx * %d] = v; }' % (
          V, ''.join(' v[%d] = %s;' % (c, own(k, f, u, f.phi + 1, r, c)) for c in range(k.C)),
          V, f.name, slot, k.HYL, r, k.HXL, k.C))
    for i in range(k.K):
      line('      %s*(%s*)(&lds_%s[%d][0][0] + h_lds[%d]) = halo_%s[%d];' % (
          halo_guard(k, i), V, f.name, slot, i, f.name, i))


def print_step(k, line, u, store):
  """One unrolled step of the plane loop; `store` prints what it computes and stores."""
  if k.ring:
    line('    {  // unrolled step %d: output plane z, LDS slots %s filled' % (u, ', '.join(
        '%s %d' % (f.name, lds_slot(k, f, u, f.phi + 1)) for f in k.shared)))
  else:
    line('    {  // unrolled step %d: output plane z, slot %d read, slot %d filled' % (
        u, u % 2, (u + 1) % 2))
  if u:
    line('      if (n + %d >= steps) break;' % u)      # the whole workgroup leaves together
  line('      const i64 z = z0 + n + %d;' % (u - k.fill))
  print_loads_ahead(k, line, u)
  print_halo_fetch(k, line)
  # compute: every step from the first one whose window is complete
  line('      if (n + %d >= %d) {' % (u, k.fill))
  print_lds_reads(k, line, u)
  store(k, line, u)
  line('      }')
  print_lds_fill(k, line, u)
  line('      soda_block_barrier();')
  line('    }')


def print_origin_and_chunk(k, line, lo, hi):
  """The workgroup's tile and z chunk of the box [lo, hi)."""
  line('  const i64 x_origin = %s - %s %% %d;' % (lo[0], lo[0], k.C))
  line('  const i64 xs = x_origin + (i64)__builtin_amdgcn_workgroup_id_x() * %d;' % k.TX)
  line('  const i64 ys = %s + (i64)__builtin_amdgcn_workgroup_id_y() * %d;' % (lo[1], k.TY))
  line('  const i64 chunk = a.param[0] > 0 ? a.param[0] : %d;' % k.chunk_planes)
  line('  const i64 z0 = %s + (i64)__builtin_amdgcn_workgroup_id_z() * chunk;' % lo[2])
  # (the same for every work-item of the workgroup: nobody waits at a barrier for them)
  line('  if (xs >= %s || ys >= %s || z0 >= %s) return;' % tuple(hi))
  line('  const i64 z1 = z0 + chunk < %s ? z0 + chunk : %s;' % (hi[2], hi[2]))


def entry_over_launch_box(k, line):
  """One output: tiles and chunks cover the launch's box."""
  print_origin_and_chunk(k, line, ['a.box_lo[%d]' % d for d in range(3)],
                         ['a.box_hi[%d]' % d for d in range(3)])


def entry_over_own_boxes(k, line):
  """Several outputs: tiles and chunks cover the union of their boxes; the lane masks."""
  C = k.C
  n_out = len(k.stages)
  # the union of the outputs' boxes is what tiles and chunks cover (the launcher sizes
  # the grid by the same rule: csrc/schedule.cpp, make_launch)
  for d in range(3):
    for side, shift, sign in (('lo', 8 * d, '-'), ('hi', 24 + 8 * d, '+')):
      line('  i64 %s%d = 0;' % (side, d))
      for j in range(n_out):
        line('  { const i64 e = (a.param[%d] >> %d) & 255; if (e > %s%d) %s%d = e; }'
             % (1 + j, shift, side, d, side, d))
      line('  %s%d = a.box_%s[%d] %s %s%d;' % (side, d, side, d, sign, side, d))
  print_origin_and_chunk(k, line, ['lo%d' % d for d in range(3)],
                         ['hi%d' % d for d in range(3)])

  # the box of output j: the launch's box widened by the extras of param[1 + j], each
  # bound computed where it is used (eighteen 64-bit bounds kept would fill the scalar file)
  box_lo = lambda j, d: '(a.box_lo[%d] - ((a.param[%d] >> %d) & 255))' % (d, 1 + j, 8 * d)
  box_hi = lambda j, d: '(a.box_hi[%d] + ((a.param[%d] >> %d) & 255))' % (d, 1 + j,
                                                                         24 + 8 * d)

  def within(what, first, size):
    """`what` as a distance from `first`, clamped into [0, size]"""
    return '(int)(%s - %s < 0 ? 0 : %s - %s > %s ? %s : %s - %s)' % (
        what, first, what, first, size, size, what, first)

  line('  const int lx = tid %% %d, ly = tid / %d * %d;' % (k.LX, k.LX, k.RW))
  for j in range(n_out):
    # what output j stores of this tile and chunk, worked out here, once for both paths, and
    # kept in three VECTOR registers per output (the one-output form leaves a dozen scalar
    # registers free, fewer than the bounds of three boxes).  Columns and rows: which of
    # the lane's own cells lie in j's box, bit r * C + c.  Planes: the steps of the plane
    # loop that compute them (step m computes plane z0 + m - fill)
    line('  int cells%d = 0;' % j)
    line('  {')
    line('    const int sx_lo = %s, sx_hi = %s;' % (within(box_lo(j, 0), 'xs', k.TX),
                                                  within(box_hi(j, 0), 'xs', k.TX)))
    line('    const int sy_lo = %s, sy_hi = %s;' % (within(box_lo(j, 1), 'ys', k.TY),
                                                  within(box_hi(j, 1), 'ys', k.TY)))
    for r in range(k.RW):
      line('    if (ly + %d >= sy_lo && ly + %d < sy_hi) {%s }' % (r, r, ''.join(
          ' if (lx * %d + %d >= sx_lo && lx * %d + %d < sx_hi) cells%d |= %d;'
          % (C, c, C, c, j, 1 << (r * C + c)) for c in range(C))))
    line('  }')
    line('  int sn_lo%d = %s + %d, sn_hi%d = %s + %d;' % (
        j, within(box_lo(j, 2), 'z0', '(z1 - z0)'), k.fill,
        j, within(box_hi(j, 2), 'z0', '(z1 - z0)'), k.fill))
    line('  %s_opaque(cells%d); %s_opaque(sn_lo%d); %s_opaque(sn_hi%d);'
         % (k.name, j, k.name, j, k.name, j))


def print_entry(k, line, prologue):
  """The entry kernel: LDS slots, tile and chunk (`prologue`), the interior or the edge path."""
  line('GLOBAL WG_SIZE(%d) void %s(soda_hip_args a) {' % (k.threads, k.name))
  for f in k.shared:
    line('  __attribute__((shared, aligned(16))) %s lds_%s[%d][%d][%d];' % (
        builtin_type(f.c_type), f.name, k.lds_slots[f.name], k.ROWS, k.PITCH))
  line('  const int tid = __builtin_amdgcn_workitem_id_x();')
  prologue(k, line)
  line('  const bool interior = xs - %d >= 0 && xs + %d <= a.dims[0] && '
       'ys - %d >= 0 && ys + %d <= a.dims[1];' % (k.HXL, k.TX + k.HXH, k.HYL, k.TY + k.HYH))
  args = 'a, %sxs, ys, z0, z1, tid%s' % (''.join('%s, ' % m for m in k.masks),
                                        ''.join(', lds_%s' % f.name for f in k.shared))
  line('  if (interior) %s_tile<true>(%s);' % (k.name, args))
  line('  else %s_tile<false>(%s);' % (k.name, args))
  line('}')


def table_entry(k):
  loaded = len(k.shared) * k.ROWS * k.PITCH + (len(k.fields) - len(k.shared)) * k.TX * k.TY
  entry = dict(name=k.name, kind='fused', depth=1, stage=-1, block=[k.threads, 1, 1],
               tile=[k.TX, k.TY, k.chunk_planes, 1], origin_align=k.C, fill_rows=k.fill,
               cols=k.C, rows=k.RW, w_out=k.TX, r_out=k.TY, period=k.period,
               est_vgprs=k.est_vgprs, lds_bytes=k.lds_bytes, lds_planes=len(k.shared),
               waves=k.waves, halo=[k.HXL, k.HXH, k.HYL, k.HYH], loaded_cells=loaded)
  if k.masks:
    entry['fields'] = len(k.stages)
  if k.ring:
    entry['lds_ring'] = [k.lds_slots[f.name] for f in k.shared]
  return entry


def emit(spec, depth=1, waves=None, rows=None, lanes_x=None, chunk_planes=64,
         max_period=16, vgpr_budget=250, fields=False, ring=False):
  """Returns (text, kernel table entry).  Without a shape: the first of
  shapes_by_loaded_cells that fits the register budget and the LDS cap.  `fields`: the
  form over several outputs, each stored inside its own box.  `ring`: the plane-ring form,
  every plane of an input that is read off the z axis in a ring of LDS slots."""
  if depth != 1:
    raise NotFusable('the LDS-plane form is depth 1')
  several, ring = bool(fields), bool(ring)
  stages, fields = analyse(spec, several, ring)
  elem = specmod.ELEM_SIZE[specmod.tensor_c_types(spec)[spec['outputs'][0]]]
  # per output, the input it hands on unchanged (stored from the window, no cells of its own)
  through = [passed_through(spec, st) if several else None for st in stages]
  fits = lambda shape: fit(fields, elem, through.count(None), shape, max_period, vgpr_budget,
                           ring)
  k = first_fit(spec, several, fits, ring) if waves is None else fits((waves, rows, lanes_x))
  k.name, k.stages, k.fields, k.through = kernel_name(spec, several, ring), stages, fields, \
      through
  k.shared, k.by_name = [f for f in fields if f.lds], {f.name: f for f in fields}
  k.index, k.elem, k.chunk_planes = tensor_index(spec), elem, chunk_planes
  k.fill = max(f.zhi - f.zlo + 1 for f in fields)
  k.K = -(-k.halo_vectors // k.threads)
  k.vec, k.lvec = {}, {}
  assert k.halo_vectors > 0
  # what differs between the two forms, as data: the header's remark, the output pointers of
  # the tile function and the lane masks the entry kernel hands it (none for one output)
  n_out = len(stages)
  k.over = ' over %d outputs' % n_out if several else ''
  k.out_pointers = ['g_out%d' % j for j in range(n_out)] if several else ['g_out']
  k.masks = ['%s%d' % (m, j) for j in range(n_out if several else 0)
             for m in ('cells', 'sn_lo', 'sn_hi')]
  store = store_in_own_boxes if several else store_in_launch_box
  prologue = entry_over_own_boxes if several else entry_over_launch_box

  o = []
  print_header(k, o.append)
  print_tile_prologue(k, o.append)
  for u in range(k.period):
    print_step(k, o.append, u, store)
  o.append('  }\n}\n')
  print_entry(k, o.append, prologue)
  return '\n'.join(o) + '\n', table_entry(k)
