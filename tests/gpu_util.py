"""Helpers of the GPU tests: programs are opened through the C ABI from the
code objects that __graft_entry__.build() produced (or JIT-compiled from
freshly generated kernel text when a test wants non-default generator options)."""
import os

import numpy as np

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

from conftest import ROOT, SAMPLES

SEED = 20240607
BLOBS = os.path.join(ROOT, 'soda-compiler_amd', 'blobs')
# The checker's shared objects of the GPU tests go to tests/_oracle_build (cached,
# git-ignored), not oracle/_build: the driver records which in-tree .so files the
# GPU test processes load, alphabetically and capped - dozens of oracle/_build/*.so
# in front would push soda-compiler_amd/csrc/libsoda_hip.so (the product) off that list.
ORACLE_BUILD = os.path.join(ROOT, 'tests', '_oracle_build')


def make_oracle(spec, **kw):
  from oracle import soda_oracle
  return soda_oracle.Oracle(spec, build_dir=ORACLE_BUILD, **kw)


def sample_path(app):
  path = os.path.join(SAMPLES, app + '.soda')
  return path if os.path.exists(path) else os.path.join(SAMPLES, 'extra', app + '.soda')


def load_spec(app, **overrides):
  st = frontend.load(sample_path(app), **overrides)
  return specmod.spec_from_stencil(st)


def open_prebuilt(app):
  spec = load_spec(app)
  path = os.path.join(BLOBS, app + '.hsaco')
  assert os.path.exists(path), '%s missing: run __graft_entry__.build()' % path
  return host.open_program(blob=path, spec=spec)


def open_jit(app, iterate=None, **gen):
  spec = load_spec(app, iterate=iterate) if iterate else load_spec(app)
  text, _ = kernel.generate(spec, **gen)
  return host.open_program(source=text, spec=spec)


def random_inputs(spec, shape, seed=SEED, small_ints=False):
  rng = np.random.default_rng(seed)
  out = []
  for t in spec['inputs']:
    dt = np.dtype(specmod.NUMPY_NAME[t['c_type']])
    if dt.kind == 'f':
      out.append(rng.random(shape, dtype=np.float32).astype(dt))
    else:
      hi = 256 if small_ints else np.iinfo(dt).max + 1
      out.append(rng.integers(0, hi, size=shape).astype(dt))
  return out


# ---- full-width operands ------------------------------------------------------------------
#
# random_inputs' floats lie in [0, 1) with float32's mantissa whatever the type (the low
# dword of every such double is 0), and the random programs' integers in 0..199 (the high
# dword of every such int64 is 0): half of an 8-byte element is constant, no narrow
# element has its top bit set, and every float sum adds positive numbers of one magnitude.
# wide_inputs fills every bit of the element and mixes signs and exponents.

WIDE_EXPONENTS = 12        # floats: sign * m * 2^e, e in -12 .. 12
WIDE_EXPONENTS_HALF = 10   # _Float16 (largest finite 65504): e in -10 .. 10


def wide_array(dtype, shape, rng, exponents=None):
  """Integers: uniform over the whole range of the type.  Floats: sign * m * 2^e with a
  random sign, m uniform in [1, 2) on the type's OWN mantissa grid (52 / 23 / 10 bits -
  not float32 widened) and e uniform in -exponents .. exponents; every value is exact in
  the type, none is zero, subnormal, inf or NaN."""
  dt = np.dtype(dtype)
  if dt.kind != 'f':
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True)
  if exponents is None:
    exponents = WIDE_EXPONENTS_HALF if dt.itemsize == 2 else WIDE_EXPONENTS
  bits = np.finfo(dt).nmant
  m = 1.0 + rng.integers(0, 1 << bits, size=shape).astype(np.float64) * 2.0 ** -bits
  e = rng.integers(-exponents, exponents + 1, size=shape)
  sign = np.where(rng.integers(0, 2, size=shape) == 1, -1.0, 1.0)
  v = np.ldexp(m, e) * sign          # exact in float64: m has at most 52 fraction bits
  out = v.astype(dt)
  assert np.array_equal(out.astype(np.float64), v)
  return out


def wide_inputs(spec, shape, seed=SEED, exponents=None):
  """One array per input of the program, of the input's type (wide_array); the same
  arrays for the same seed."""
  rng = np.random.default_rng(seed)
  return [wide_array(specmod.NUMPY_NAME[t['c_type']], shape, rng, exponents)
          for t in spec['inputs']]


# Programs whose float results overflow on +-12 (a condition on the inputs, not on the
# product: tests/test_operand_ranges.py, test_wide_floats_do_not_overflow, holds every
# float program and sample to finite results on these spans).  Keys: sample names and the
# keys of tests/golden/random_programs.json.  At most five.
NARROWED_EXPONENTS = {
    # the output holds f r1, r1 of degree 6 in r0 = 4.9 u f: |u|, |f| < 2^13 would need
    # 1e100.  +-12 and +-8 overflow on the CPU, +-7 stays a factor 5 below FLT_MAX on one
    # seed, +-6 four orders of magnitude
    'denoise2d': 6,
}


def wide_inputs_of(key, spec, shape, seed=SEED):
  """wide_inputs with the exponent span of program `key`."""
  return wide_inputs(spec, shape, seed, NARROWED_EXPONENTS.get(key))


# The oracle the full-width cases are held to.  On full-range integers a signed sum or
# product overflows, which plain C++ leaves undefined - the plain oracle has no answer
# there (hence random_inputs' small_ints for sobel2d).  The product, however, PROMISES
# two's-complement wrap: every kernel is compiled with -fwrapv (codegen/kernel.py,
# runtime/host.py), so the oracle gets the same flag and integer
# arithmetic modulo 2^n is defined on both sides for any input.  -fwrapv only gives a
# meaning to what was undefined: wherever no signed overflow occurs this oracle equals the
# plain one (tests/test_operand_ranges.py holds -O2 against -O0 under it).
WRAP_FLAGS = ('-O2', '-fwrapv')


def make_wrap_oracle(spec, opt='-O2'):
  return make_oracle(spec, flags=(opt,) + WRAP_FLAGS[1:])


# ---- the sweep's memory contract (include/soda_hip.h: soda_hip_sweep, soda_hip_run_slab) ----
#
#   in[j]   never written;   out[j]  any cell may be written, nothing outside the array;
#   slabs:  a never written (world 1: it receives no rows), b and c as out.
#
# Program.run_numpy gives every array an allocation of its own and looks at the valid box
# only: a store a few bytes before or after an array lands in the allocator's padding.
# Here the arrays of a run lie back to back in ONE allocation, each between two guard
# bands; guards and outputs hold seeded random bytes (nothing a kernel stores by mistake -
# zeros, a repeated value, a copy of a row - reproduces them), and after the run the whole
# allocation comes back and is compared byte by byte.
#
# Out of reach: the intermediates of a multi-stage program and the ping-pong partner of a
# plain sweep live in the plan's own scratch allocations; seeing those needs a hook in the
# library, which there is not.  (run_slab_guarded covers the ping-pong partner of the
# one-input one-output programs: there all three arrays are the caller's.)

GUARD_MIN_BYTES = 4096
ARENA_PIECE = 64     # guards end on this boundary; array i then starts `skew[i]` bytes in


def guard_bytes(shape, itemsize):
  """Geometry, not measurement: at least 4 KiB and two rows of the array; with three or
  more dimensions one whole slice of the slowest dimension (3-D: a plane) plus two rows -
  a tile or chunk placed one row or one plane too far still lands in a guard."""
  row = int(shape[-1]) * itemsize
  n = 2 * row
  if len(shape) >= 3:
    n += int(np.prod(shape[1:])) * itemsize
  return max(GUARD_MIN_BYTES, n)


def pool_skews(n, itemsize):
  """Start offsets within a 64-byte piece the way a pool allocator hands out arrays:
  element-aligned, none a multiple of 16 bytes (4, 20, 36, 52 ... for 4-byte elements,
  2, 18, 34 ... for 2-byte ones)."""
  return [(itemsize + 16 * i) % ARENA_PIECE for i in range(n)]


class Arena:
  """Layout and checker.  `arrays`: [(name, role, shape, dtype)], role 'in' or 'out', in
  memory order.  All offsets are bytes from the arena's first byte; nothing here touches
  a device (tests/test_guarded_arena.py runs it on a numpy buffer)."""

  def __init__(self, arrays, skews=None, seed=SEED):
    skews = list(skews) if skews is not None else [0] * len(arrays)
    assert len(skews) == len(arrays)
    self.arrays = []          # dicts: name, role, shape, dtype, offset, nbytes
    self.guards = []          # dicts: offset, nbytes, before (name or None), after
    at, prev = 0, None
    for (name, role, shape, dtype), skew in zip(arrays, skews):
      dtype = np.dtype(dtype)
      assert role in ('in', 'out') and 0 <= skew < ARENA_PIECE and skew % dtype.itemsize == 0
      nbytes = int(np.prod(shape)) * dtype.itemsize
      g = max(guard_bytes(shape, dtype.itemsize), prev['guard'] if prev else 0)
      start = -(-(at + g) // ARENA_PIECE) * ARENA_PIECE + skew
      self.guards.append(dict(offset=at, nbytes=start - at,
                              before=prev['name'] if prev else None, after=name))
      prev = dict(name=name, role=role, shape=tuple(shape), dtype=dtype, offset=start,
                  nbytes=nbytes, guard=guard_bytes(shape, dtype.itemsize))
      self.arrays.append(prev)
      at = start + nbytes
    self.guards.append(dict(offset=at, nbytes=prev['guard'], before=prev['name'], after=None))
    self.nbytes = at + prev['guard']
    self.seed = seed
    self.before = None

  def array(self, name):
    return next(a for a in self.arrays if a['name'] == name)

  def offset(self, name):
    return self.array(name)['offset']

  def image(self, inputs):
    """The bytes to upload: seeded random bytes everywhere (guards AND outputs), the
    inputs ({name: array}) in their places.  Kept for check()."""
    rng = np.random.default_rng(self.seed)
    img = rng.integers(0, 256, size=self.nbytes, dtype=np.uint8)
    for a in self.arrays:
      if a['role'] == 'in':
        src = np.ascontiguousarray(inputs[a['name']])
        assert src.dtype == a['dtype'] and src.shape == a['shape'], (a['name'], src.dtype)
        img[a['offset']:a['offset'] + a['nbytes']] = src.reshape(-1).view(np.uint8)
    self.before = img
    return img

  def view(self, img, name):
    a = self.array(name)
    return img[a['offset']:a['offset'] + a['nbytes']].view(a['dtype']).reshape(a['shape'])

  def check(self, after):
    """Compares the downloaded arena with what was uploaded.  Returns (violations,
    outputs): a list of messages (empty = the contract held) and {name: raw output array,
    unspecified cells included}.  Bytes are compared, not values: -0.0f for +0.0f, or one
    NaN for another, is a write."""
    assert self.before is not None and after.dtype == np.uint8 and after.size == self.nbytes
    bad = []
    for i, g in enumerate(self.guards):
      lo, hi = g['offset'], g['offset'] + g['nbytes']
      hit = np.flatnonzero(self.before[lo:hi] != after[lo:hi])
      if hit.size == 0:
        continue
      first, last = lo + int(hit[0]), lo + int(hit[-1])
      where = []
      if g['before'] is not None:       # measured from the end of the array in front
        a = self.array(g['before'])
        row = a['shape'][-1] * a['dtype'].itemsize
        where.append('bytes +%d .. +%d past the end of %s (%.2f .. %.2f rows of %d bytes)' % (
            first - lo, last - lo, a['name'], (first - lo) / row, (last - lo + 1) / row, row))
      if g['after'] is not None:        # and back from the start of the one behind
        a = self.array(g['after'])
        row = a['shape'][-1] * a['dtype'].itemsize
        where.append('bytes -%d .. -%d before the start of %s (%.2f .. %.2f rows of %d bytes)'
                     % (hi - first, hi - last, a['name'], (hi - first) / row,
                        (hi - last - 1) / row, row))
      bad.append('guard %d (%s | %s, %d bytes): %d bytes changed, %s' % (
          i, g['before'] or 'arena start', g['after'] or 'arena end', g['nbytes'], hit.size,
          '; '.join(where)))
    outputs = {}
    for a in self.arrays:
      lo, hi = a['offset'], a['offset'] + a['nbytes']
      if a['role'] == 'out':
        outputs[a['name']] = after[lo:hi].copy().view(a['dtype']).reshape(a['shape'])
        continue
      hit = np.flatnonzero(self.before[lo:hi] != after[lo:hi])
      if hit.size:
        size = a['dtype'].itemsize
        cells = np.unique(hit // size)
        bad.append('input %s was written: %d bytes in %d elements, first element %s, last %s'
                   % (a['name'], hit.size, cells.size,
                      tuple(int(v) for v in np.unravel_index(int(cells[0]), a['shape'])),
                      tuple(int(v) for v in np.unravel_index(int(cells[-1]), a['shape']))))
    return bad, outputs


class DeviceArena:
  """An Arena in one device allocation (through the C ABI, like every GPU test)."""

  def __init__(self, arena, inputs):
    self.arena = arena
    self.mem = host.DeviceArray(arena.nbytes)
    self.mem.upload(arena.image(inputs))

  def ptr(self, name):
    return self.mem.ptr + self.arena.offset(name)

  def finish(self):
    """Downloads the whole arena once, frees it, returns Arena.check's pair."""
    from soda_hip.runtime import capi
    capi.check(capi.lib().soda_hip_stream_synchronize(None))
    try:
      after = self.mem.download((self.arena.nbytes,), np.uint8)
    finally:
      self.mem.free()
    return self.arena.check(after)


def run_guarded(prog, inputs, iterate, skews=None, seed=SEED, valid_lo=None, valid_hi=None):
  """Program.sweep on pointers into a guarded arena: guard | in0 | guard | in1 | ... |
  out0 | guard | ...  Returns (raw outputs in the program's order - unspecified cells hold
  whatever the kernels or the random fill left -, violations, timing).  The caller asserts
  `violations == []` AND compares the valid box with the oracle: a guard that is clean
  because nothing was stored proves nothing.  A fresh run goes through sweep_timed with no
  warm-up and one repeat - the same launches as sweep, once, and timing['max_depth'] says
  how deep they went; a resumed one (valid_lo / valid_hi) through sweep, timing None."""
  spec = prog.spec
  shape = inputs[0].shape
  dims = tuple(reversed(shape))
  names_in = ['in:' + t['name'] for t in spec['inputs']]
  names_out = ['out:' + o for o in spec['outputs']]
  arena = Arena([(n, 'in', shape, dt) for n, dt in zip(names_in, prog.in_dtypes)] +
                [(n, 'out', shape, dt) for n, dt in zip(names_out, prog.out_dtypes)],
                skews=skews, seed=seed)
  dev = DeviceArena(arena, dict(zip(names_in, inputs)))
  timing = None
  try:
    pin, pout = [dev.ptr(n) for n in names_in], [dev.ptr(n) for n in names_out]
    if valid_lo is None and valid_hi is None:
      timing = prog.sweep_timed(pin, pout, dims, iterate, warmup=0, repeats=1)
    else:
      prog.sweep(pin, pout, dims, iterate, valid_lo=valid_lo, valid_hi=valid_hi)
  finally:
    bad, outs = dev.finish()
  return [outs[n] for n in names_out], bad, timing


def run_slab_guarded(prog, a, iterate, exchange, skews=None, seed=SEED, order=0):
  """soda_hip_run_slab with world = 1 on a one-input one-output program: the level-0 slab
  `a` AND both ping-pong arrays b, c are the caller's, so all three sit between guards; a
  must come back bit-identical (a world of one receives no rows).  Returns (raw result
  array, number of exchanges, violations)."""
  import ctypes
  from soda_hip.runtime import capi
  spec = prog.spec
  assert len(spec['inputs']) == 1 and len(spec['outputs']) == 1
  dims = tuple(reversed(a.shape))
  arena = Arena([('a', 'in', a.shape, a.dtype), ('b', 'out', a.shape, a.dtype),
                 ('c', 'out', a.shape, a.dtype)], skews=skews, seed=seed)
  slab = capi.Slab(rank=0, world=1, reach_lo=spec['radius']['lo'][-1],
                   reach_hi=spec['radius']['hi'][-1], exchange=exchange,
                   own_first=0, own_last=dims[-1], order=order)
  for d, n in enumerate(dims):
    slab.dims[d] = n
  dev = DeviceArena(arena, dict(a=a))
  result, n_ex = ctypes.c_void_p(), ctypes.c_int()
  try:
    capi.check(capi.lib().soda_hip_run_slab(
        prog.handle, ctypes.byref(slab), None, dev.ptr('a'), dev.ptr('b'), dev.ptr('c'),
        iterate, None, ctypes.byref(result), ctypes.byref(n_ex)))
    which = {dev.ptr('b'): 'b', dev.ptr('c'): 'c'}.get(result.value)
  finally:
    bad, outs = dev.finish()
  assert which is not None, 'result is neither b nor c'
  return outs[which], n_ex.value, bad
