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


def integer_term(rng, read, small, names, first, nonzero=False):
  """One term of an integer stage over operator_program's operators, shared by
  narrow_volume_program and line_program: `read(name, nonzero=...)` gives an integer operand
  that loads tensor `name`, `small(name)` says whether that operand may be multiplied by a
  thousand without leaving an int.  (`&&` and `||` under a product: the reference prints
  their parentheses away, and at the top of a sum they would swallow it.)"""
  def literal():
    return str(rng.choice(['1', '2', '3', '5', '7', '0x0f', '0x3', '017', '3u', '6l',
                           '0xffu', '9']))
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

  def term(names, first, nonzero=False):
    return integer_term(rng, read, small, names, first, nonzero)

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


LINE_ENDS = ('uint16', 'int16', 'int32', 'uint32', 'float', 'int64', 'double')
LINE_SIZE = dict(uint16=2, int16=2, int32=4, uint32=4, float=4, int64=8, double=8)
# the other type of the same width a local may have: the signedness flip, int32 for float and
# float for int32, int64 <-> double
LINE_OTHER = dict(uint16='int16', int16='uint16', uint32='int32', int32='float', float='int32',
                  int64='double', double='int64')
# bytes of a lane per element size (default_cols follows `burst width`, 8 bits a byte): 16, 8
# and, for 4- and 8-byte elements, one cell
LINE_LANES = {2: (16, 8), 4: (16, 8, 4), 8: (16, 8)}
LINE_MAX_HOPS = 8                        # kernel_stream1d.MAX_HOPS_1D
# lanes away of the far programs, in the set's order; the first 8 is the program with 8 lanes
# on either side
LINE_HOPS = (2, 3, 8, 4, 5, 2, 6, 8, 3, 7, 4, 2, 8, 3, 5, 2, 4, 6, 3, 7, 2, 8)
LINE_MODES = ('both', 'lo', 'both', 'hi', 'both')
# iteration counts beyond 5: the depth-8 and depth-12 kernels; ln10 is a far program whose
# table stops at depth 2
LINE_DEEP = {3: 13, 12: 8, 21: 12, 10: 9}
# what a stage reads of a 4- / 8-byte integer tensor away from its store point: the low 16 bits
# or the quotient by this
LINE_REDUCE = {4: 16384, 8: 1048576}
LINE_TO_FLOAT = {4: 65536, 8: 1048576}   # the quotient a float stage converts


def line_program(rng, seed):
  """1-D programs of the fused 1-D kernels' class (kernel_stream1d; with reads beyond the
  neighbour lane, kernel.generate's `far_taps`): one input, one output of its type - the types
  of LINE_ENDS in turn -, 0 to 2 locals of the end type or of the other type of its width
  (LINE_OTHER).  `burst width` gives lanes of 16 or 8 bytes or of one 4- or 8-byte cell, C
  cells.  A third of the programs (seed % 3 == 0) stays within the neighbour lane; the others
  read up to `hops` lanes away (LINE_HOPS, 2 to 8), with offsets of exactly +-hops C and of
  +-((hops - 1) C + 1) placed on purpose - on a local where the program has one -, the offsets
  around a dword's width for 16-bit cells, and the rest anywhere in the span.  The axis is
  two-sided, lo-only or hi-only per program (LINE_MODES); seed % 8 == 7: negative offsets
  only.  `iterate` 1 to 5, 8 to 13 for LINE_DEEP.

  Integer stages are sums of integer_term's terms, float stages weighted sums with weights of
  at most 1 in sum.  What is restricted, and why - all of it because plain C++ has no defined
  answer otherwise, none of it for a kernel's sake:
    * a 4- or 8-byte integer tensor is an operand as its low 16 bits, as its quotient by
      LINE_REDUCE, or - at the store point - as its half: a stage's terms then stay below a
      quarter of the type's range whatever the tensor holds, and with the half of the store
      point below the range itself, at any iteration count (8 terms of at most 2^18 * 255, and 2^30, stay
      below 2^31; 8 of 2^45 * 255, and 2^62, below 2^63);
    * a float stage reads such a tensor as float(quotient by LINE_TO_FLOAT), so float values
      stay within 2^16 (2^43 for double) where the inputs do, and int32(f * s), s <= 4, the
      only way from float to integer, is in range - on the fixtures' inputs and on
      gpu_util.wide_inputs' 2^13 alike;
    * nothing divides by a tensor;
    * no operand and no sum starts with `(` where its last operand ends with `)`: the
      reference prints a chain of operands as `(` + text + `)` after taking every leading `(`
      and trailing `)` off the text, whether they match or not.  A comparison of
      `(a(3) / 16384)` with `int16(a(1))` so loses its parentheses to the sum around it, which
      then yields 0 or 1 in every cell; a sum from `((x * 257) / 11)` to `(3 * (...))` comes
      out unbalanced, which no compiler takes.  So the quotient goes under a cast, and a sum
      starts with a read.
  Every stage reads the store point of a parent, so every window contains it and the
  reference's loops have an answer - except in the negative-only programs.  The output reads
  everything still unused away from the store point: no stage is dead.
  Returns (text, end type, iterate, far)."""
  end = LINE_ENDS[seed % 7]
  size = LINE_SIZE[end]
  floaty_end = end in ('float', 'double')
  lanes = LINE_LANES[size]
  lane_bytes = lanes[(seed // 7 + seed % 7) % len(lanes)]
  cols = lane_bytes // size
  negative_only = seed % 8 == 7
  far = seed % 3 != 0
  far_index = seed - seed // 3 - 1
  hops = LINE_HOPS[far_index % len(LINE_HOPS)] if far else 1
  mode = LINE_MODES[seed % 5]
  eight_a_side = far and far_index == 2
  if eight_a_side:
    mode = 'both'
  reach = hops * cols
  span = {'both': (-reach, reach), 'lo': (-reach, 0), 'hi': (0, reach)}[mode]
  if negative_only:
    span = (-reach, -1)
  n_locals = (1, 2, 0)[far_index % 3] if far else int(rng.integers(0, 3))
  iterate = LINE_DEEP.get(seed, int(rng.integers(1, 6)))
  if eight_a_side:
    iterate = 5                          # depth 4 leaves no cell of a segment
  if negative_only:
    iterate = min(iterate, 3)
  # offsets placed on purpose, first the lane `hops` away itself or the first cell that needs
  # it (in turn), on either side the span has
  edge = reach if far_index % 2 == 0 or eight_a_side else (hops - 1) * cols + 1
  placed = [v for v in (edge, -edge, -reach if edge != reach else -(reach - cols + 1))
            if span[0] <= v <= span[1]] if far else []
  types = {'a': end}

  def x_offset():
    lo, hi = span
    r = rng.random()
    if r < 0.25:
      pool = [-reach, reach]             # the same cell of the lane `hops` away
    elif r < 0.45:
      pool = [-(reach - cols + 1), reach - cols + 1]     # the first cell that needs it
    elif r < 0.6 and size == 2:
      pool = [-3, -2, 2, 3]              # past the dword, either side
    elif r < 0.8:
      pool = [int(rng.integers(lo, hi + 1))]
    else:
      pool = [-2, -1, 0, 1, 2]
    pool = [v for v in pool if lo <= v <= hi] or [lo if lo else hi]
    return int(rng.choice(pool))

  def offset(name, nonzero=False):
    if nonzero and placed and (name != 'a' or n_locals == 0):
      return placed.pop(0)
    while True:
      at = x_offset()
      if at or not nonzero:
        return at

  def read(name, centre=False, nonzero=False):
    """A read as an integer operand."""
    at = 0 if centre else offset(name, nonzero)
    text = '%s(%d)' % (name, at)
    t = types[name]
    if t in ('float', 'double'):
      scale = str(rng.choice(['1.0', '2.0', '4.0'])) + ('f' if t == 'float' else '')
      return '%s(%s * %s)' % ('int32' if t == 'float' else 'int64', text, scale)
    if LINE_SIZE[t] == 2:
      return text
    if centre:
      return '%s / 2' % text
    if rng.random() < 0.5:
      return 'int16(%s)' % text
    # (under a cast: an operand that starts with `(` would cost the term around it its own
    # parentheses, see below)
    return 'int%d(%s / %d)' % (8 * LINE_SIZE[t], text, LINE_REDUCE[LINE_SIZE[t]])

  def term(names, first, nonzero=False):
    return integer_term(rng, read, lambda name: True, names, first, nonzero)

  def pick(names):
    return names[int(rng.integers(0, len(names)))]

  def again(must):
    """Further reads of the last tensor of `must` that offset() places: as many as it takes
    for every offset placed on purpose to be read."""
    takers = [n for n in must if n != 'a' or n_locals == 0]
    return [takers[-1]] * max(0, len(placed) - len(takers)) if takers else []

  def integer_expression(names, must):
    # the sum starts with a plain operand - the store point, or in the negative-only programs
    # a read as it is - and not with a term in parentheses
    parts = [read(pick(names), nonzero=True) if negative_only else
             read(pick(names), centre=True)]
    parts += [term(names, n, nonzero=True) for n in must + again(must)]
    parts += [term(names, pick(names)) for _ in range(int(rng.integers(1, 3)))]
    text = parts[0]
    for t in parts[1:]:
      text += str(rng.choice([' + ', ' - ', ' + '])) + t
    return text

  def float_expression(names, must, c_type):
    suffix = 'f' if c_type == 'float' else ''
    weights = ['0.25', '0.25', '0.125', '0.125', '0.125', '0.0625']

    def operand(name, at):
      text = '%s(%d)' % (name, at)
      t = types[name]
      if t in ('float', 'double'):
        return text
      return '%s(%s / %d)' % (c_type, text, LINE_TO_FLOAT[LINE_SIZE[t]])
    reads = [(n, True) for n in must + again(must)]
    reads += [(pick(names), False) for _ in range(int(rng.integers(1, 3)))]
    ats = [(n, offset(n, nonzero)) for n, nonzero in reads]
    if not negative_only:                # the store point of a parent
      ats.insert(0, (pick(names), 0))
    parts = ['%s * %s%s' % (operand(n, at), weights[i], suffix)
             for i, (n, at) in enumerate(ats[:len(weights)])]
    text = parts[0]
    for t in parts[1:]:
      text += str(rng.choice([' + ', ' - '])) + t
    return text

  def expression(c_type, names, must):
    if c_type in ('float', 'double'):
      return float_expression(names, must, c_type)
    return integer_expression(names, must)

  lines = ['kernel: ln%d' % seed, 'burst width: %d' % (8 * lane_bytes), 'unroll factor: 1',
           'iterate: %d' % iterate, 'input %s: a(*)' % end]
  names, unused = ['a'], ['a']
  for k in range(n_locals):
    name = 'loc%d' % k
    t = LINE_OTHER[end] if rng.random() < 0.6 else end
    must = [unused.pop(0)] if rng.random() < 0.7 else []
    lines.append('local %s: %s(0) = %s' % (t, name, expression(t, names, must)))
    types[name] = t
    names.append(name)
    unused.append(name)
  lines.append('output %s: out(0) = %s' % (end, expression(end, names, unused)))
  assert not placed, (seed, placed)
  return '\n'.join(lines) + '\n', end, iterate, far


def line_set(n=32):
  """[(key, text, dim, iterate, generate()'s keywords)] - the programs of
  tests/test_gpu_random1d.py: `far_taps` for those that read beyond the neighbour lane, and
  for a few of the set other segments per wavefront than the default four."""
  out = []
  for seed in range(n):
    if seed in LINE_SLOW:
      continue
    rng = np.random.default_rng(31000 + seed)
    text, end, iterate, far = line_program(rng, seed)
    keywords = dict(far_taps=True) if far else {}
    if seed % 8 == 2:
      keywords['segs'] = 2
    if seed % 16 == 5:
      keywords['segs'] = 8
    out.append(('ln%d' % seed, text, 1, iterate, keywords))
  return out


# seeds left out of the set because their case took too long on an MI355X: none.  The two
# cases above three times the set's median, ln3 and ln21 at 1.6 and 1.5 s, are the programs
# with a depth-12 kernel, which the set has to hold (profiles/r20_random1d.txt)
LINE_SLOW = ()
LINE_SEAM_MARGIN = 40      # cells a fixture is longer than the widest segment's and the box's


def write_line_set(path):
  """tests/golden/random1d_programs.json: text, iterate and generate()'s keywords per program,
  and the length of its reference fixture - the cells the widest segment of its table stores,
  plus what the box of all iterations is shorter than the array, plus 40: a segment seam of
  every kernel of the table lies inside the box.  Needs the package."""
  import json
  import os
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, os.path.join(root, 'soda-compiler_amd'))
  from soda_hip import frontend
  from soda_hip.codegen import kernel
  from soda_hip.codegen import spec as specmod
  programs = {}
  for key, text, dim, iterate, keywords in line_set():
    spec = specmod.spec_from_stencil(frontend.loads(text))
    _, table = kernel.generate(spec, **keywords)
    widest = max(k['w_out'] for k in table if k['kind'] == 'fused')
    lo, hi = specmod.iteration_margins(specmod.inline_pointwise(spec), iterate)[-1]
    programs[key] = dict(text=text, dim=dim, iterate=iterate, generate=keywords,
                         grid=[widest + lo[0] + hi[0] + LINE_SEAM_MARGIN])
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
  if sys.argv[1:] == ['--lines']:
    write_line_set(os.path.join(here, 'golden', 'random1d_programs.json'))
    sys.exit(0)
  with open(os.path.join(here, 'golden', 'random_programs.json'), 'w') as f:
    json.dump({k: dict(text=t, dim=d, iterate=i) for k, t, d, i in program_set()},
              f, indent=1, sort_keys=True)
