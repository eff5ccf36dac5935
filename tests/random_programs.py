"""Generator of random SODA programs for the parity tests: asymmetric and
one-sided windows, negative-only offsets, fan-in and fan-out DAGs, `let`s, casts,
integer division, several inputs, 2-D and 3-D.  Plain numpy, so that
tests/golden/make_golden.py (python3.9, next to the reference) and the tests
share it.  The texts the committed fixtures were made from are stored with them
(tests/golden/random_programs.json): numpy does not promise the same random
stream in every version."""
import numpy as np


def random_program(rng, seed):
  dim = 3 if rng.random() < 0.25 else 2
  floaty = rng.random() < 0.6
  dtype = rng.choice(['float', 'float', 'float', 'double']) if floaty else \
      rng.choice(['uint16', 'int32', 'int32', 'uint8', 'int64', 'int16'])
  n_inputs = 1 if rng.random() < 0.75 else 2
  n_locals = int(rng.integers(0, 4))
  iterate = int(rng.integers(1, 6)) if n_inputs == 1 else 1
  reach = 2 if dim == 2 else 1
  names = ['in%d' % i for i in range(n_inputs)]
  lines = ['kernel: rnd%d' % seed, 'burst width: 512', 'unroll factor: 2',
           'iterate: %d' % iterate]
  tile = ', '.join(['32'] * (dim - 1))
  for i, n in enumerate(names):
    lines.append('input %s: %s(%s, *)' % (dtype, n, tile) if i == n_inputs - 1
                 else 'input %s: %s' % (dtype, n))
  if n_inputs == 2:   # only the LAST input may carry the tile (reference quirk)
    lines[-2], lines[-1] = 'input %s: %s' % (dtype, names[0]), \
        'input %s: %s(%s, *)' % (dtype, names[1], tile)

  def offset():
    # sometimes one-sided windows: only negative or only positive offsets
    mode = rng.integers(0, 4)
    lo, hi = (-reach, reach) if mode < 2 else ((-reach, 0) if mode == 2 else (0, reach))
    return tuple(int(rng.integers(lo, hi + 1)) for _ in range(dim))

  def load(name):
    return '%s(%s)' % (name, ', '.join(map(str, offset())))

  def literal():
    if floaty:
      return rng.choice(['0.25f', '0.5f', '1.5f', '0.125f', '3.0f', '0.2f', '0.3'])
    return str(int(rng.integers(1, 5)))

  def expression(available, must_use):
    terms = []
    pool = list(must_use) + [rng.choice(available)
                             for _ in range(int(rng.integers(1, 4)))]
    for name in pool:
      t = load(name)
      r = rng.random()
      if r < 0.3:
        t = '%s * %s' % (t, literal())
      elif r < 0.4:
        t = '(%s - %s)' % (t, load(rng.choice(available)))
      elif r < 0.5 and not floaty:
        t = '(%s + %s) / 3' % (t, load(name))
      elif r < 0.5 and floaty:
        t = '%s / %s' % (t, literal())
      terms.append(t)
    text = terms[0]
    for t in terms[1:]:
      text += rng.choice([' + ', ' - ', ' + ']) + t
    if rng.random() < 0.3:
      text = '(%s) * %s' % (text, literal())
    return text

  available = list(names)
  unused = list(names)
  for k in range(n_locals):
    name = 'loc%d' % k
    use = [unused.pop(0)] if unused and rng.random() < 0.7 else []
    if rng.random() < 0.25:
      lines.append('local %s: t = %s %s(%s) = t + %s' % (
          dtype, expression(available, use), name, ', '.join(['0'] * dim),
          load(rng.choice(available))))
    else:
      lines.append('local %s: %s(%s) = %s' % (
          dtype, name, ', '.join(map(str, offset())), expression(available, use)))
    available.append(name)
    unused.append(name)
  # the output reads everything still unused, so that no stage is dead
  lines.append('output %s: out(%s) = %s' % (
      dtype, ', '.join(['0'] * dim), expression(available, unused)))
  return '\n'.join(lines) + '\n', dim, dtype, iterate




def operator_program(rng, seed):
  """Integer (and a few float-compare) programs over the operators the arithmetic
  generator above never emits: % & | ^ comparisons && || unary - ~ !, hexadecimal,
  octal and suffixed literals, casts between widths.  Every window contains the
  store point, so the reference's own CPU loops have a defined answer."""
  dim = 3 if rng.random() < 0.2 else 2
  dtype = str(rng.choice(['uint16', 'int32', 'uint8', 'int16', 'uint32', 'int64',
                          'int8', 'uint64']))
  other = str(rng.choice(['int32', 'uint16', 'int16', 'uint8']))
  iterate = int(rng.integers(1, 4))
  reach = 2 if dim == 2 else 1
  lines = ['kernel: ops%d' % seed, 'burst width: 512', 'unroll factor: 2',
           'iterate: %d' % iterate,
           'input %s: a(%s, *)' % (dtype, ', '.join(['32'] * (dim - 1)))]

  def ref(name, centre=False):
    idx = [0] * dim if centre else [int(rng.integers(-reach, reach + 1))
                                    for _ in range(dim)]
    return '%s(%s)' % (name, ', '.join(map(str, idx)))

  def literal():
    return str(rng.choice(['1', '2', '3', '5', '7', '0x0f', '0x3', '017', '3u', '6l',
                           '0xffu', '9']))

  def term(names):
    n = str(rng.choice(names))
    r = rng.random()
    if r < 0.15:
      return '(%s %% %s)' % (ref(n), str(rng.choice(['3', '5', '7', '0x10'])))
    if r < 0.30:
      return '(%s & %s)' % (ref(n), literal())
    if r < 0.40:
      return '(%s | %s)' % (ref(n), ref(str(rng.choice(names))))
    if r < 0.50:
      return '(%s ^ %s)' % (ref(n), ref(str(rng.choice(names))))
    if r < 0.60:
      return '(%s %s %s)' % (ref(n), str(rng.choice(['<', '<=', '>', '>=', '==', '!='])),
                             ref(str(rng.choice(names))))
    if r < 0.68:
      return '(%s > %s && %s != %s)' % (ref(n), literal(), ref(n), literal())
    if r < 0.74:
      return '(%s < %s || %s == %s)' % (ref(n), literal(), ref(str(rng.choice(names))),
                                        literal())
    if r < 0.80:
      return '(-%s)' % ref(n)
    if r < 0.86:
      return '(~%s & 0xff)' % ref(n)
    if r < 0.90:
      return '(!%s)' % ref(n)
    if r < 0.95:
      return '%s(%s) * %s' % (other, ref(n), literal())
    return '%s / %s' % (ref(n), str(rng.choice(['2', '3', '4'])))

  def expression(names):
    parts = [ref(str(rng.choice(names)), centre=True)]     # the store point is read
    parts += [term(names) for _ in range(int(rng.integers(2, 5)))]
    text = parts[0]
    for t in parts[1:]:
      text += str(rng.choice([' + ', ' - ', ' + '])) + t
    return text

  names = ['a']
  if rng.random() < 0.5:
    lines.append('local %s: m(%s) = %s' % (other, ', '.join(['0'] * dim),
                                           expression(names)))
    names.append('m')
  use = expression(names)
  if 'm' in names and 'm(' not in use:
    use += ' + ' + ref('m', centre=True)
  lines.append('output %s: out(%s) = %s' % (dtype, ', '.join(['0'] * dim), use))
  return '\n'.join(lines) + '\n', dim, dtype, iterate


def structure_program(rng, seed):
  """Programs that stress the STRUCTURE the other generators keep small: three
  inputs, windows reaching up to 4 cells, up to seven stages, several outputs
  (with `iterate` > 1 when inputs and outputs pair up), 3-D with two inputs, a local
  that only another local reads.  Every window contains the store point."""
  dim = 3 if rng.random() < 0.3 else 2
  dtype = str(rng.choice(['float', 'float', 'int32', 'double', 'uint16']))
  floaty = dtype in ('float', 'double')
  n_inputs = int(rng.integers(1, 4))
  n_outputs = int(rng.integers(1, 3))
  n_locals = int(rng.integers(1, 6))
  iterate = int(rng.integers(2, 6)) if n_inputs == n_outputs else 1
  reach = int(rng.integers(1, 5)) if dim == 2 else int(rng.integers(1, 3))
  ins = ['in%d' % i for i in range(n_inputs)]
  lines = ['kernel: st%d' % seed, 'burst width: 512', 'unroll factor: 4',
           'iterate: %d' % iterate]
  tile = ', '.join(['64'] * (dim - 1))
  for i, n in enumerate(ins):      # only the LAST input may carry the tile
    lines.append('input %s: %s(%s, *)' % (dtype, n, tile) if i == n_inputs - 1
                 else 'input %s: %s' % (dtype, n))

  def ref(name, centre=False):
    idx = [0] * dim if centre else [int(rng.integers(-reach, reach + 1))
                                    for _ in range(dim)]
    return '%s(%s)' % (name, ', '.join(map(str, idx)))

  def literal():
    return str(rng.choice(['0.25f', '0.5f', '0.125f', '2.0f'] if floaty
                          else ['1', '2', '3']))

  def expression(names, must):
    parts = [ref(str(rng.choice(names)), centre=True)]
    pool = list(must) + [str(rng.choice(names)) for _ in range(int(rng.integers(1, 4)))]
    for n in pool:
      t = ref(n)
      if rng.random() < 0.4:
        t = '%s * %s' % (t, literal())
      parts.append(t)
    text = parts[0]
    for t in parts[1:]:
      text += str(rng.choice([' + ', ' - ', ' + '])) + t
    if floaty and rng.random() < 0.5:
      text = '(%s) * %s' % (text, literal())
    return text

  names = list(ins)
  unused = list(ins)
  for k in range(n_locals):
    name = 'loc%d' % k
    must = [unused.pop(0)] if unused else []
    lines.append('local %s: %s(%s) = %s' % (dtype, name, ', '.join(['0'] * dim),
                                            expression(names, must)))
    names.append(name)
    unused.append(name)
  for k in range(n_outputs):
    share = [unused.pop(0) for _ in range((len(unused) + n_outputs - k - 1)
                                          // (n_outputs - k))] if unused else []
    lines.append('output %s: out%s(%s) = %s' % (
        dtype, '' if k == 0 else str(k), ', '.join(['0'] * dim),
        expression(names, share)))
  return '\n'.join(lines) + '\n', dim, dtype, iterate


def cube_program(rng, seed):
  """3-D iteration chains for the deep 3-D kernels (single-wave depth 2, wave-
  pipelined and block-form depth 4): one input, one output, optionally a local in
  between, 4..13 iterations, windows inside {-1,0,1}^3 INCLUDING diagonals (a read
  that leaves the band in y and the plane in z at once)."""
  dtype = str(rng.choice(['float', 'float', 'float', 'int32']))
  floaty = dtype == 'float'
  iterate = int(rng.integers(4, 14))
  lines = ['kernel: cube%d' % seed, 'burst width: 512', 'unroll factor: 2',
           'iterate: %d' % iterate, 'input %s: a(32, 32, *)' % dtype]

  def offsets(n):
    seen = {(0, 0, 0)}
    while len(seen) < n:
      seen.add(tuple(int(v) for v in rng.integers(-1, 2, size=3)))
    rest = sorted(seen - {(0, 0, 0)})
    rng.shuffle(rest)
    return [(0, 0, 0)] + [tuple(o) for o in rest]

  def expression(name):
    terms = []
    for o in offsets(int(rng.integers(4, 10))):
      t = '%s(%d, %d, %d)' % ((name,) + o)
      if rng.random() < 0.3:
        t += ' * %s' % (str(rng.choice(['0.5f', '0.25f', '2.0f'])) if floaty
                        else str(rng.choice(['2', '3'])))
      terms.append(t)
    text = terms[0]
    for t in terms[1:]:
      text += str(rng.choice([' + ', ' + ', ' - '])) + t
    scale = str(rng.choice(['0.125f', '0.0625f', '0.2f'])) if floaty else '1'
    return '(%s) * %s' % (text, scale) if floaty else text

  src = 'a'
  if rng.random() < 0.35:
    lines.append('local %s: m(0, 0, 0) = %s' % (dtype, expression('a')))
    src = 'm'
  lines.append('output %s: out(0, 0, 0) = %s' % (dtype, expression(src)))
  return '\n'.join(lines) + '\n', 3, dtype, iterate


def program_set(n_plain=40, n_deep=16, n_ops=16, n_struct=16, n_cube=12):
  """[(key, text, dim, iterate, shape)] - the programs of the GPU random tests."""
  out = []
  for seed in range(n_plain):
    rng = np.random.default_rng(1000 + seed)
    text, dim, dtype, iterate = random_program(rng, seed)
    out.append(('plain%d' % seed, text, dim, iterate))
  for seed in range(n_deep):
    rng = np.random.default_rng(5000 + seed)
    while True:
      text, dim, dtype, iterate = random_program(rng, seed)
      if dim == 2 and 'input %s: in1' % dtype not in text:
        break
    deep = int(rng.integers(8, 21))
    text = text.replace('iterate: %d\n' % iterate, 'iterate: %d\n' % deep)
    out.append(('deep%d' % seed, text, dim, deep))
  for seed in range(n_ops):
    rng = np.random.default_rng(9000 + seed)
    text, dim, dtype, iterate = operator_program(rng, seed)
    out.append(('ops%d' % seed, text, dim, iterate))
  for seed in range(n_struct):
    rng = np.random.default_rng(12000 + seed)
    text, dim, dtype, iterate = structure_program(rng, seed)
    out.append(('struct%d' % seed, text, dim, iterate))
  for seed in range(n_cube):
    rng = np.random.default_rng(15000 + seed)
    text, dim, dtype, iterate = cube_program(rng, seed)
    out.append(('cube%d' % seed, text, dim, iterate))
  return out


NARROW_ENDS = ('uint8', 'int8', 'uint16', 'int16')


def narrow_volume_program(rng, seed):
  """3-D programs of the packed-cell kernels' class (kernel.generate's `packed_cells`): one
  output, 1 or 2 inputs, all ends 8-bit or all 16-bit (the output, or the second input, now
  and then of the other signedness), 0 to 2 locals typed from {the end type, a type of the
  other narrow width, int32, float}; `iterate` 1 to 3 where one input feeds an output of its
  type (1 to 2 over a local, 1 over two).  x offsets stay within the columns C of the narrowest lane such a program gets (8
  cells of one byte, 4 of two), with +-C itself - the neighbour lane's same cell - and the
  offsets around a dword's width drawn on purpose; y and z within +-1.  Each axis is
  two-sided, lo-only or hi-only for the whole program, and a quarter of the programs reads
  no z neighbour at all.  The integer stages use operator_program's operators (with `&&` and
  `||` under a product: the reference prints their parentheses away, and at the top of a sum
  they would swallow it), a product that leaves 16 bits before it is divided, and the
  quotient of a difference (negative for unsigned ends: C's promotion to int).  Nothing
  overflows an int, converts an out-of-range float or divides by zero on any input, so the
  plain CPU loops have a defined answer.  Every stage reads the store point of a parent, so
  every window contains it - except in the programs of seed % 8 == 7, whose offsets on one
  axis are all negative: the reference's loops have no answer for those."""
  end = NARROW_ENDS[(seed + seed // 4) % 4]
  size = 1 if end.endswith('int8') else 2
  cols = 8 // size                       # the narrowest lane: 8 bytes
  per = 4 // size                        # cells in a dword
  flipped = {'uint8': 'int8', 'int8': 'uint8', 'uint16': 'int16', 'int16': 'uint16'}
  other_width = ('uint16', 'int16') if size == 1 else ('uint8', 'int8')
  negative_only = seed % 8 == 7
  n_inputs = 2 if rng.random() < 0.25 and not negative_only else 1
  in_types = [end] * n_inputs
  if n_inputs == 2 and rng.random() < 0.4:
    in_types[int(rng.integers(0, 2))] = flipped[end]
  out_type = flipped[end] if rng.random() < 0.15 and not negative_only else end
  n_locals = int(rng.integers(0, 3))
  chain = n_inputs == 1 and in_types[0] == out_type
  iterate = int(rng.integers(1, 4)) if chain else 1
  if negative_only:
    iterate = 2
  # (every local widens the window of an iteration: four stages deep at most, so the output
  # of all iterations keeps cells on a fixture grid of some ten rows and planes)
  iterate = min(iterate, 4 // (n_locals + 1))

  def axis_mode(reach, none=0.0):
    r = rng.random()
    if r < none:
      return (0, 0)
    mode = int(rng.integers(0, 4))
    return (-reach, reach) if mode < 2 else ((-reach, 0) if mode == 2 else (0, reach))

  spans = [axis_mode(cols), axis_mode(1), axis_mode(1, none=0.25)]
  if negative_only:                      # one axis with offsets below zero only
    axis = (0, 2, 1)[(seed // 8) % 3]
    spans[axis] = (-cols if axis == 0 else -1, -1)

  def x_offset(lo, hi):
    r = rng.random()
    if r < 0.3:
      pool = [-cols, cols]               # the same cell of the neighbour lane
    elif r < 0.55:
      pool = [-per - 1, -per, per, per + 1]          # past the dword, either side
    else:
      pool = [-2, -1, 0, 1, 2]
    pool = [v for v in pool if lo <= v <= hi] or [lo if lo else hi]
    return int(rng.choice(pool))

  def offset(nonzero=False):
    while True:
      at = (x_offset(*spans[0]),) + tuple(int(rng.integers(lo, hi + 1)) for lo, hi in spans[1:])
      if any(at) or not nonzero:
        return at

  types = {}

  def read(name, centre=False, nonzero=False):
    """A read as an integer operand: a float local goes through int32()."""
    at = (0, 0, 0) if centre else offset(nonzero)
    text = '%s(%d, %d, %d)' % ((name,) + at)
    if types[name] == 'int32' and types['.stage'] == 'int32':
      return 'int16(%s)' % text          # (sums of sums of 2e7 would pass an int)
    return 'int32(%s)' % text if types[name] == 'float' else text

  def small(name):
    # values within 17 bits: what may be multiplied (an int32 local may hold 1e8)
    return types[name] != 'int32' or types['.stage'] == 'int32'

  def literal():
    return str(rng.choice(['1', '2', '3', '5', '7', '0x0f', '0x3', '017', '3u', '6l',
                           '0xffu', '9']))

  def term(names, first, nonzero=False):
    other = names[int(rng.integers(0, len(names)))]
    a = read(first, nonzero=nonzero)
    r = rng.random()
    if r < 0.10:
      return '(%s %% %s)' % (a, str(rng.choice(['3', '5', '7', '0x10'])))
    if r < 0.20:
      return '(%s & %s)' % (a, literal())
    if r < 0.28:
      return '(%s | %s)' % (a, read(other))
    if r < 0.36:
      return '(%s ^ %s)' % (a, read(other))
    if r < 0.46:
      return '(%s %s %s)' % (a, str(rng.choice(['<', '<=', '>', '>=', '==', '!='])),
                             read(other))
    if r < 0.52:
      return '2 * (%s > %s && %s != %s)' % (a, literal(), read(first), literal())
    if r < 0.58:
      return '3 * (%s < %s || %s == %s)' % (a, literal(), read(other), literal())
    if r < 0.64:
      return '(-%s)' % a
    if r < 0.70:
      return '(~%s & 0xff)' % a
    if r < 0.74:
      return '(!%s)' % a
    if r < 0.80:
      cast = str(rng.choice(['int32', 'uint16', 'int16', 'uint8', 'int8'][not small(first):]))
      return '%s(%s) * %s' % (cast, a, literal())
    if r < 0.86:
      return '%s / %s' % (a, str(rng.choice(['2', '3', '4'])))
    if r < 0.93 and small(first):        # leaves 16 bits, then comes back
      return '(%s * %s) / %s' % (a, str(rng.choice(['300', '1000', '257'])),
                                 str(rng.choice(['7', '13', '11'])))
    return '(%s - %s) / %s' % (a, read(other), str(rng.choice(['3', '5', '2'])))

  def integer_expression(names, must):
    parts = [] if negative_only else [read(names[int(rng.integers(0, len(names)))],
                                           centre=True)]
    parts += [term(names, n, nonzero=True) for n in must]
    parts += [term(names, names[int(rng.integers(0, len(names)))])
              for _ in range(int(rng.integers(1, 4)))]
    text = parts[0]
    for t in parts[1:]:
      text += str(rng.choice([' + ', ' - ', ' + '])) + t
    return text

  def float_expression(names, must):
    # weights of at most 1 in sum over operands within 17 bits: back in int32's range
    names = [n for n in names if types[n] != 'int32']
    pool = list(must) + [names[int(rng.integers(0, len(names)))]
                         for _ in range(int(rng.integers(1, 3)))]
    weights = ['0.5f', '0.25f', '0.125f', '0.125f']
    parts = []
    for i, n in enumerate(pool):
      at = (0, 0, 0) if i == 0 and not negative_only and not must else offset(n in must)
      text = '%s(%d, %d, %d)' % ((n,) + at)
      parts.append('%s * %s' % (text if types[n] == 'float' else 'float(%s)' % text,
                                weights[i]))
    if not negative_only and must:       # the store point of a parent
      n = names[int(rng.integers(0, len(names)))]
      text = '%s(0, 0, 0)' % n
      parts.append('%s * %s' % (text if types[n] == 'float' else 'float(%s)' % text,
                                weights[len(pool)]))
    text = parts[0]
    for t in parts[1:]:
      text += str(rng.choice([' + ', ' - '])) + t
    return text

  lines = ['kernel: nv%d' % seed, 'burst width: 512', 'unroll factor: 2',
           'iterate: %d' % iterate]
  names = []
  for i, t in enumerate(in_types):       # only the LAST input may carry the tile
    name = 'in%d' % i
    lines.append('input %s: %s(32, 32, *)' % (t, name) if i == n_inputs - 1
                 else 'input %s: %s' % (t, name))
    types[name] = t
    names.append(name)
  unused = list(names)
  for k in range(n_locals):
    name = 'loc%d' % k
    t = str(rng.choice([end, str(rng.choice(other_width)), 'int32', 'float']))
    if t in ('int32', 'float') and size == 1 and n_locals == 2 and spans[2] == (-1, 1):
      t = end        # a register per cell over three planes, twice: beyond two waves per SIMD
    types['.stage'] = t
    must = []
    if unused and rng.random() < 0.7 and (t != 'float' or types[unused[0]] != 'int32'):
      must = [unused.pop(0)]
    body = float_expression(names, must) if t == 'float' else integer_expression(names, must)
    lines.append('local %s: %s(0, 0, 0) = %s' % (t, name, body))
    types[name] = t
    names.append(name)
    unused.append(name)
  # the output reads everything still unused, away from the store point: no stage is dead,
  # and no local is folded into its reader
  types['.stage'] = out_type
  lines.append('output %s: out(0, 0, 0) = %s' % (out_type, integer_expression(names, unused)))
  return '\n'.join(lines) + '\n', 3, end, iterate


# generate()'s keywords per program of narrow_volume_set, beside packed_cells=True: the lane
# width left to the generator's own choice, fixed to the narrow or to the wide lane of the
# element size, and the occupancy level a depth-2 kernel on 16-byte lanes needs
NARROW_VOLUME_KEYWORDS = {
    'nv8': dict(cols=8), 'nv9': dict(cols=4), 'nv10': dict(cols=16), 'nv11': dict(cols=16),
    'nv14': dict(cols=16), 'nv19': dict(cols=8), 'nv22': dict(cols=4),
}


# seeds left out of the set: three stages of six operands each, whose case - the run-time
# compile of the unrolled kernel above all - took 18 and 10 seconds on an MI355X, where the
# others take 0.5 to 8
NARROW_VOLUME_SLOW = (16, 18)


def narrow_volume_set(n=24):
  """[(key, text, dim, iterate, generate()'s keywords)] - the programs of
  tests/test_gpu_packed3d_random.py."""
  out = []
  for seed in range(n):
    if seed in NARROW_VOLUME_SLOW:
      continue
    rng = np.random.default_rng(21000 + seed)
    text, dim, dtype, iterate = narrow_volume_program(rng, seed)
    key = 'nv%d' % seed
    out.append((key, text, dim, iterate, dict(NARROW_VOLUME_KEYWORDS.get(key, {}))))
  return out


def write_narrow_volume_set(path):
  """tests/golden/packed3d_random_programs.json: text, iterate and generate()'s keywords per
  program, and the grid (x, y, z) of its reference fixture - 40 columns wider than what one
  tile of the kernel under test stores, so a tile seam lies inside the output's box; 11 rows
  and 7 planes, 9 and 5 where the arrays of the fixture would pass 185 000 bytes, more where
  the window of all iterations leaves fewer than three rows or no plane.  Needs the package."""
  import json
  import os
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, os.path.join(root, 'soda-compiler_amd'))
  from soda_hip import frontend
  from soda_hip.codegen import kernel
  from soda_hip.codegen import spec as specmod
  programs = {}
  for key, text, dim, iterate, keywords in narrow_volume_set():
    spec = specmod.spec_from_stencil(frontend.loads(text))
    _, table = kernel.generate(spec, packed_cells=True, **keywords)
    widest = max(k['w_out'] for k in table if k['kind'] == 'fused')
    cell = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']] * (len(spec['inputs']) + 1)
    lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), iterate)[-1]
    for rows, planes in ((11, 7), (9, 5)):
      # (at least three rows and one plane of output whatever the window)
      grid = (widest + 40, max(rows, lo[1] + hi[1] + 3), max(planes, lo[2] + hi[2] + 1))
      if grid[0] * grid[1] * grid[2] * cell <= 185000:
        break
    else:
      raise ValueError('%s: no grid of %d columns under 185 000 bytes' % (key, grid[0]))
    programs[key] = dict(text=text, dim=dim, iterate=iterate, generate=keywords,
                         grid=list(grid))
  with open(path, 'w') as f:
    json.dump(programs, f, indent=1, sort_keys=True)


if __name__ == '__main__':      # writes the program texts the fixtures are made from
  import json
  import os
  import sys
  here = os.path.dirname(os.path.abspath(__file__))
  if sys.argv[1:] == ['--narrow-volumes']:
    write_narrow_volume_set(os.path.join(here, 'golden', 'packed3d_random_programs.json'))
    sys.exit(0)
  with open(os.path.join(here, 'golden', 'random_programs.json'), 'w') as f:
    json.dump({k: dict(text=t, dim=d, iterate=i) for k, t, d, i in program_set()},
              f, indent=1, sort_keys=True)
