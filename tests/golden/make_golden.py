#!/opt/conda/bin/python3.9
"""Generate the golden fixtures under tests/golden/ from the REAL reference.

Run in the build container only (needs /root/reference and python3.9 with
`cached_property`; the reference does not import on python >= 3.10):

    /opt/conda/bin/python3.9 tests/golden/make_golden.py

What it does, per sample program of /root/reference/tests/src/*.soda:

 1. Splits the .soda text into statements with a small regex splitter and
    builds, by hand, the object tree textX would have built (textX itself is
    not installable here), using the reference's own node
    classes.  This splitter / expression reader is deliberately independent of
    the product parser in soda-compiler_amd/soda_hip/frontend.
 2. Feeds that tree to the reference's `soda.core.Stencil` and lets the
    reference's `soda.codegen.xilinx.host.print_code` emit its host program.
 3. Cuts the CPU golden loop nest out of the emitted `<app>_test`
    (the text between `int error_count = 0;` and `if(error_count==0)`), wraps
    it in a tiny harness, compiles it with g++ and runs it on small grids with
    the reference ramp input and with seeded random inputs.
 4. Stores inputs + every produced tensor as .npz fixtures, and the
    reference's analysis results (normalised stages, C expressions, loop bounds,
    STENCIL_DIM / STENCIL_DISTANCE) as analysis.json.

Only DATA produced by the reference is committed; none of its source text.
"""
import hashlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REF = '/root/reference'
sys.path.insert(0, os.path.join(REF, 'src'))

from haoda import ir                      # noqa: E402
from haoda import util as hutil           # noqa: E402
from soda import core, grammar            # noqa: E402
from soda.codegen.xilinx import host      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240607

# ----------------------------------------------------------------------------
# a tiny, independent reader for .soda text -> reference node classes
# ----------------------------------------------------------------------------
TOKEN = re.compile(r'''
    (?P<float>((\d*\.\d+|\d+\.)([+-]?[Ee]\d+)?|\d+[+-]?[Ee]\d+)[FfLl]?)
  | (?P<int>0[Xx][0-9a-fA-F]+[UuLl]*|0[Bb][01]+[UuLl]*|\d+[UuLl]*)
  | (?P<id>[A-Za-z_]\w*)
  | (?P<op>\|\||&&|==|!=|<=|>=|[-+*/%<>|^&~!(),\[\]=])
''', re.X)

CHAIN = [
    (ir.Expr, ('||',)), (ir.LogicAnd, ('&&',)), (ir.BinaryOr, ('|',)),
    (ir.Xor, ('^',)), (ir.BinaryAnd, ('&',)), (ir.EqCmp, ('==', '!=')),
    (ir.LtCmp, ('<=', '>=', '<', '>')), (ir.AddSub, ('+', '-')),
    (ir.MulDiv, ('*', '/', '%')),
]
FUNCS = set(re.findall(r"'(\w+)'", grammar.GRAMMAR.split('FuncName:')[1]
                       .split(';')[0]))
TYPE_RE = re.compile(r'^(u?int[1-9]\d*(_[1-9]\d*)?|float[1-9]\d*(_[1-9]\d*)?'
                     r'|float|double|half)$')


class Reader:
  def __init__(self, text):
    self.toks = []
    pos = 0
    while pos < len(text):
      if text[pos].isspace():
        pos += 1
        continue
      m = TOKEN.match(text, pos)
      if not m:
        raise ValueError('bad char %r' % text[pos:pos + 10])
      self.toks.append((m.lastgroup, m.group(0)))
      pos = m.end()
    self.i = 0

  def peek(self, k=0):
    return self.toks[self.i + k] if self.i + k < len(self.toks) else (None, None)

  def take(self, val=None):
    kind, tok = self.peek()
    if val is not None and tok != val:
      raise ValueError('expected %r got %r' % (val, tok))
    self.i += 1
    return tok

  def level(self, depth=0):
    if depth == len(CHAIN):
      return self.unary()
    cls, ops = CHAIN[depth]
    operands, operators = [self.level(depth + 1)], []
    while self.peek()[1] in ops:
      operators.append(self.take())
      operands.append(self.level(depth + 1))
    return cls(operand=operands, operator=operators)

  def unary(self):
    ops = []
    while self.peek()[1] in ('+', '-', '~', '!'):
      ops.append(self.take())
    return ir.Unary(operator=ops, operand=self.operand())

  def sint(self):
    sign = ''
    if self.peek()[1] in ('+', '-'):
      sign = self.take()
    return int(sign + self.take())

  def operand(self):
    kw = dict(cast=None, call=None, ref=None, num=None, var=None, expr=None)
    kind, tok = self.peek()
    if kind in ('float', 'int'):
      kw['num'] = self.take()
    elif tok == '(':
      self.take('(')
      kw['expr'] = self.level()
      self.take(')')
    elif kind == 'id' and self.peek(1)[1] == '(' and TYPE_RE.match(tok):
      self.take(); self.take('(')
      kw['cast'] = ir.Cast(haoda_type=tok, expr=self.level())
      self.take(')')
    elif kind == 'id' and self.peek(1)[1] == '(' and tok in FUNCS:
      self.take(); self.take('(')
      args = [self.level()]
      while self.peek()[1] == ',':
        self.take(',')
        args.append(self.level())
      self.take(')')
      kw['call'] = ir.Call(name=tok, arg=args)
    elif kind == 'id' and self.peek(1)[1] == '(':
      kw['ref'] = self.ref()
    elif kind == 'id':
      self.take()
      idx = []
      while self.peek()[1] == '[':
        self.take('['); idx.append(self.sint()); self.take(']')
      kw['var'] = ir.Var(name=tok, idx=idx)
    else:
      raise ValueError('unexpected token %r' % (tok,))
    return ir.Operand(**kw)

  def ref(self):
    name = self.take()
    self.take('(')
    idx = [self.sint()]
    while self.peek()[1] == ',':
      self.take(',')
      idx.append(self.sint())
    self.take(')')
    lat = None
    if self.peek()[1] == '~' and self.peek(1)[0] == 'int':   # `('~' lat=Int)?`
      self.take('~')
      lat = self.sint()
    return ir.Ref(name=name, idx=idx, lat=lat)

  def lets(self):
    """`(let=Let)*` in front of the stored reference: `[Type] name = Expr`."""
    out = []
    while True:
      (k0, t0), (k1, t1), (k2, t2) = self.peek(), self.peek(1), self.peek(2)
      if k0 == 'id' and TYPE_RE.match(t0) and k1 == 'id' and t2 == '=':
        self.take(); name = self.take(); self.take('=')
        out.append(ir.Let(haoda_type=t0, name=name, expr=self.level()))
      elif k0 == 'id' and t1 == '=':
        name = self.take(); self.take('=')
        out.append(ir.Let(haoda_type=None, name=name, expr=self.level()))
      else:
        return out


STMT = re.compile(r'^(kernel|burst\s+width|unroll\s+factor|iterate|input|local'
                  r'|output)\b', re.M)


def read_program(text):
  text = re.sub(r'#.*$', '', text, flags=re.M)
  cuts = [m.start() for m in STMT.finditer(text)] + [len(text)]
  prog = dict(inputs=[], locals=[], outputs=[])
  pos = 0
  for a, b in zip(cuts, cuts[1:]):
    head, body = text[a:b].split(':', 1)
    head = head.split()
    if head[0] == 'kernel':
      prog['app_name'] = body.strip()
    elif head[0] == 'burst':
      prog['burst_width'] = int(body)
    elif head[0] == 'unroll':
      prog['unroll_factor'] = int(body)
    elif head[0] == 'iterate':
      prog['iterate'] = int(body)
    elif head[0] == 'input':
      m = re.match(r'\s*(\w+)\s*(\(([^)]*)\))?\s*$', body)
      tiles = []
      if m.group(3) is not None:
        tiles = [int(x) for x in m.group(3).split(',')[:-1]]
      stmt = grammar.InputStmt(haoda_type=head[1], name=m.group(1),
                               tile_size=tiles, dram=[])
      stmt._tx_position = pos
      prog['inputs'].append(stmt)
    else:
      rd = Reader(body)
      lets = rd.lets()
      ref = rd.ref()
      rd.take('=')
      expr = rd.level()
      assert rd.peek() == (None, None), rd.peek()
      cls = grammar.LocalStmt if head[0] == 'local' else grammar.OutputStmt
      kw = dict(haoda_type=head[1], let=lets, ref=ref, expr=expr)
      if head[0] == 'output':
        kw['dram'] = []
      stmt = cls(**kw)
      stmt._tx_position = pos
      prog['locals' if head[0] == 'local' else 'outputs'].append(stmt)
    pos += 1
  # what grammar.SodaProgram.__init__ derives
  tile = None
  for s in prog['inputs']:
    if s.tile_size[:-1]:
      tile = s.tile_size
  if tile is None:
    tile = prog['inputs'][-1].tile_size
  prog['tile_size'] = tile
  prog['dim'] = len(tile)
  return prog


def build_stencil(path, iterate=None, text=None):
  if text is None:
    with open(path) as f:
      text = f.read()
  prog = read_program(text)
  core._overall_stencil_window_cache.clear()
  st = core.Stencil(
      burst_width=prog['burst_width'],
      iterate=prog['iterate'] if iterate is None else iterate,
      dram_in=None, dram_out=None, app_name=prog['app_name'],
      input_stmts=prog['inputs'], param_stmts=[],
      local_stmts=prog['locals'], output_stmts=prog['outputs'],
      dim=prog['dim'], tile_size=prog['tile_size'],
      unroll_factor=prog['unroll_factor'])
  return st


# ----------------------------------------------------------------------------
# reference analysis -> json
# ----------------------------------------------------------------------------
def analysis_of(st):
  inputs = tuple(map(st.tensors.get, st.input_names))
  out = dict(app_name=st.app_name, dim=st.dim, iterate=st.iterate,
             burst_width=st.burst_width, unroll_factor=st.unroll_factor,
             tile_size=list(st.tile_size),
             input_names=list(st.input_names),
             local_names=list(st.local_names),
             output_names=list(st.output_names),
             input_types=list(st.input_types),
             tensor_names=list(st.tensors),
             chronological=[t.name for t in st.chronological_tensors],
             stages=[])
  for t in st.chronological_tensors:
    if t.is_input():
      continue
    window = core.get_overall_stencil_window(inputs, t)
    sdim = core.get_stencil_dim(window)
    off = core.get_stencil_window_offset(window)
    def rel(obj, args, t=t):
      # loads become neutral placeholders `name[d0,d1,..]` holding the offset
      # RELATIVE to the store index (what host.py:1093-1102 indexes with)
      if isinstance(obj, ir.Ref):
        return ir.make_var('%s[%s]' % (obj.name, ','.join(
            str(a - b) for a, b in zip(obj.idx, t.st_ref.idx))))
      return obj
    out['stages'].append(dict(
        name=t.name, haoda_type=t.haoda_type, c_type=t.c_type,
        st_idx=list(t.st_ref.idx),
        expr_str=str(t.expr), c_expr=t.expr.visit(rel).c_expr,
        lets=[dict(name=l.name, haoda_type=l.haoda_type, c_type=l.c_type,
                   c_expr=l.expr.visit(rel).c_expr) for l in t.lets],
        loads={name: [list(r.idx) for r in refs]
               for name, refs in t.ld_refs.items()},
        window=[list(p) for p in window],
        loop_lo=list(off),
        loop_hi_margin=[sdim[d] - off[d] - 1 for d in range(st.dim)],
        is_output=t.is_output()))
  buf = io.StringIO()
  buf.name = 'host'
  host.print_code(st, buf)
  text = buf.getvalue()
  out['macros'] = {k: int(v) for k, v in re.findall(
      r'#define (STENCIL_DIM_\d|STENCIL_DISTANCE|BURST_WIDTH) (\d+)', text)}
  return out, text


# ----------------------------------------------------------------------------
# run the reference's emitted CPU golden loops
# ----------------------------------------------------------------------------
C_HEADERS = ('assert', 'float', 'math', 'stdbool', 'stddef', 'stdint', 'stdio',
             'stdlib', 'string')
CXX_HEADERS = ('algorithm', 'array', 'string', 'unordered_map')
NP_TYPES = {'uint8_t': np.uint8, 'uint16_t': np.uint16, 'uint32_t': np.uint32,
            'int8_t': np.int8, 'int16_t': np.int16, 'int32_t': np.int32,
            'int64_t': np.int64, 'uint64_t': np.uint64,
            'float': np.float32, 'double': np.float64}


def harness_source(st, host_text):
  body = host_text.split('int error_count = 0;', 1)[1]
  body = body.split('if(error_count==0)', 1)[0]
  # keep the CPU value of the program outputs: store result_<name> where the
  # emitted code would read the FPGA value, so the comparison is a no-op.
  body = re.sub(
      r'(?m)^(\s*)(\S+) val_fpga = (.*);\n(\s*)(\S+) val_cpu = (result_\w+);',
      r'\1\3 = \6;\n\1\2 val_fpga = \3;\n\4\5 val_cpu = \6;', body)
  src = []
  for h in C_HEADERS:
    src.append('#include <c%s>' % h)
  for h in CXX_HEADERS:
    src.append('#include <%s>' % h)
  src.append('typedef struct buffer_t { uint64_t dev; uint8_t* host; '
             'int32_t extent[4]; int32_t stride[4]; int32_t min[4]; '
             'int32_t elem_size; } buffer_t;')
  src.append('FILE* const* error_report = &stderr;')
  src.append('int main(int argc, char** argv) {')
  src.append('  int dims[4] = {0, 0, 0, 0};')
  src.append('  for (int d = 0; d < %d; ++d) dims[d] = atoi(argv[2 + d]);'
             % st.dim)
  src.append('  size_t n = 1; for (int d = 0; d < %d; ++d) n *= dims[d];'
             % st.dim)
  for t in st.tensors.values():
    src.append('  buffer_t %s; memset(&%s, 0, sizeof(buffer_t));'
               % (t.name, t.name))
    src.append('  %s* %s_img = new %s[n]();' % (t.c_type, t.name, t.c_type))
    src.append('  %s.stride[0] = 1;' % t.name)
    for d in range(1, st.dim):
      src.append('  %s.stride[%d] = %s;' % (
          t.name, d, '*'.join('dims[%d]' % x for x in range(d))))
  src.append('  FILE* fi = fopen(argv[1], "rb");')
  for name in st.input_names:
    t = st.tensors[name]
    src.append('  if (fread(%s_img, sizeof(%s), n, fi) != n) return 3;'
               % (name, t.c_type))
  src.append('  fclose(fi);')
  src.append('  int error_count = 0;')
  src.append(body)
  src.append('  if (error_count) return 4;')
  for t in st.tensors.values():
    if t.is_input():
      continue
    src.append('  { char p[4096]; snprintf(p, sizeof p, "%%s.%s", argv[1]); '
               'FILE* fo = fopen(p, "wb"); fwrite(%s_img, sizeof(%s), n, fo); '
               'fclose(fo); }' % (t.name, t.name, t.c_type))
  src.append('  return 0;')
  src.append('}')
  return '\n'.join(src) + '\n'


def make_inputs(st, dims, kind, rng):
  """dims[0] is the fastest-varying extent; numpy shape is reversed(dims)."""
  shape = tuple(reversed(dims))
  arrays = []
  for name, htype in zip(st.input_names, st.input_types):
    ctype = hutil.get_c_type(htype)
    dt = NP_TYPES[ctype]
    if kind == 'ramp':
      # the reference's own init pattern (host.py:1041-1048): p+q(+r), divided
      # by the sum of extents for float types (decided by the FIRST input type)
      grids = np.meshgrid(*[np.arange(n, dtype=np.int32) for n in shape],
                          indexing='ij')
      s = sum(grids)
      if hutil.is_float(st.input_types[0]):
        a = (s.astype(dt) / dt(sum(dims))).astype(dt)
      else:
        a = s.astype(dt)
    elif np.issubdtype(dt, np.floating):
      a = rng.random(shape, dtype=np.float32).astype(dt)
    else:
      hi = 256 if st.app_name == 'sobel2d' else np.iinfo(dt).max + 1
      a = rng.integers(0, hi, size=shape, dtype=dt)
    arrays.append(np.ascontiguousarray(a))
  return arrays


def run_reference(st, host_text, dims, inputs, flags, workdir):
  tag = hashlib.sha1((st.app_name + str(st.iterate) + flags).encode()).hexdigest()[:10]
  exe = os.path.join(workdir, 'h_%s' % tag)
  if not os.path.exists(exe):
    cpp = exe + '.cpp'
    with open(cpp, 'w') as f:
      f.write(harness_source(st, host_text))
    subprocess.check_call(['g++', '-std=c++11', '-fopenmp',
                           '-Wno-unused-result'] + flags.split() +
                          [cpp, '-o', exe])
  data = os.path.join(workdir, 'in_%s.bin' % tag)
  with open(data, 'wb') as f:
    for a in inputs:
      f.write(a.tobytes())
  subprocess.check_call([exe, data] + [str(d) for d in dims])
  result = {}
  shape = tuple(reversed(dims))
  for t in st.tensors.values():
    if t.is_input():
      continue
    dt = NP_TYPES[t.c_type]
    result[t.name] = np.fromfile(data + '.' + t.name, dtype=dt).reshape(shape)
  return result


CASES_2D = [(37, 29), (64, 48)]
CASES_3D = [(20, 18, 16), (33, 9, 12)]


EXTRA = os.path.join(os.path.dirname(HERE), 'samples', 'extra')


def write_family(out_dir, manifest_path, apps, cases, kinds=('ramp', 'random'),
                 refusal_prefix=None, refusals=()):
  """The loop of the make_<family>_golden.py scripts: every program of `apps`
  ((app of tests/samples/extra, iteration counts), ...) on every grid of `cases` (a tuple,
  or a function of the stencil) with every kind of input, through the reference's loops at
  -O0 and at -O2 -ffp-contract=off, which must agree.  Writes <out_dir>/<key>.<grid>.<kind>.npz
  and the manifest.  `refusals` names the ways in which the reference does not take a
  program that end in a manifest row '<refusal_prefix>.<key>' instead of an error here:
  'raises' (its analysis or host printer raises), 'fed_back' (an output is read by another
  stage: the emitted loops read the device's array there, main_extra) and 'compile' (the
  emitted loops do not compile)."""
  manifest = {}

  def refuse(key, why, said):
    manifest['%s.%s' % (refusal_prefix, key)] = dict(key=key, reference_cpu_path=why)
    print(key, said)

  with tempfile.TemporaryDirectory() as wd:
    for app, iterations in apps:
      for it in iterations:
        key = '%s.iter%d' % (app, it)
        try:
          st = build_stencil(os.path.join(EXTRA, app + '.soda'), iterate=it)
          ana, text = analysis_of(st)
        except Exception as e:      # the reference itself does not take the program
          if 'raises' not in refusals:
            raise
          refuse(key, 'the reference raises %s: %s' % (type(e).__name__, str(e)[:200]),
                 ': the reference raises %s %s' % (type(e).__name__, e))
          continue
        fed_back = [t['name'] for t in ana['stages']
                    if t['name'] in st.output_names and not t['is_output']]
        if fed_back and 'fed_back' in refusals:
          refuse(key, 'reads the device result of output(s) %s' % ', '.join(fed_back),
                 ': output read by another stage, no self-contained reference answer')
          continue
        for dims in (cases(st) if callable(cases) else cases):
          for kind in kinds:
            inputs = make_inputs(st, dims, kind, np.random.default_rng(SEED))
            try:
              r0 = run_reference(st, text, dims, inputs, '-O0', wd)
              r2 = run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
            except subprocess.CalledProcessError:
              if 'compile' not in refusals:
                raise
              refuse(key, 'does not compile',
                     ': the reference\'s emitted CPU loops do not compile')
              break
            outs = {n: r0[n] for n in st.output_names}
            for name in outs:
              if not np.array_equal(r0[name], r2[name], equal_nan=True):
                raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
            fx = '%s.%s.%s.npz' % (key, 'x'.join(map(str, dims)), kind)
            payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
            payload.update({'out_' + n: a for n, a in outs.items()})
            os.makedirs(out_dir, exist_ok=True)    # a family without a fixture: no directory
            np.savez_compressed(os.path.join(out_dir, fx), **payload)
            manifest[fx] = dict(key=key, dims=list(dims), kind=kind, iterate=it,
                                sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                        for n, a in outs.items()})
            print('wrote', fx)
          else:
            continue
          break
  os.makedirs(os.path.dirname(manifest_path), exist_ok=True)
  with open(manifest_path, 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


def main_extra():
  """Fixtures for the hand-written programs of tests/samples/extra (features no
  reference sample uses: let, casts, ~lat, two-argument C calls, one-sided
  windows), produced by the reference exactly like the sample fixtures.  Writes
  extra.*.npz, extra_analysis.json and extra_manifest.json; a program whose
  reference-emitted CPU loops do not compile is recorded as such."""
  analysis, manifest = {}, {}
  with tempfile.TemporaryDirectory() as wd:
    for fname in sorted(os.listdir(EXTRA)):
      app = fname[:-5]
      st = build_stencil(os.path.join(EXTRA, fname))
      ana, text = analysis_of(st)
      key = '%s.iter%d' % (app, st.iterate)
      analysis[key] = ana
      fed_back = [t['name'] for t in ana['stages']
                  if t['name'] in st.output_names and not t['is_output']]
      if fed_back:
        # an output that another stage reads: the emitted loops keep its CPU value
        # in a scalar, read the DEVICE's array for the dependent stages and never
        # compare it (host.py:1104-1118, core.py:146) - nothing self-contained
        manifest['extra.' + key] = dict(
            key=key, reference_cpu_path='reads the device result of output(s) %s'
            % ', '.join(fed_back))
        print(key, ': output read by another stage, no self-contained reference answer')
        continue
      for dims in {2: [(37, 29), (64, 48)], 3: CASES_3D,
                   4: [(12, 10, 9, 8), (9, 11, 7, 10)]}[st.dim]:
        for kind in ('ramp', 'random'):
          inputs = make_inputs(st, dims, kind, np.random.default_rng(SEED))
          try:
            r0 = run_reference(st, text, dims, inputs, '-O0', wd)
            r2 = run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
          except subprocess.CalledProcessError:
            manifest['extra.' + key] = dict(
                key=key, reference_cpu_path='does not compile')
            print(key, ': the reference\'s emitted CPU loops do not compile')
            break
          for name in r0:
            if not np.array_equal(r0[name], r2[name], equal_nan=True):
              raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
          fx = 'extra.%s.%s.%s.npz' % (key, 'x'.join(map(str, dims)), kind)
          payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
          payload.update({'out_' + n: a for n, a in r0.items()})
          np.savez_compressed(os.path.join(HERE, fx), **payload)
          manifest[fx] = dict(key=key, dims=list(dims), kind=kind,
                              sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                      for n, a in r0.items()})
          print('wrote', fx)
        else:
          continue
        break
  with open(os.path.join(HERE, 'extra_analysis.json'), 'w') as f:
    json.dump(analysis, f, indent=1, sort_keys=True)
  with open(os.path.join(HERE, 'extra_manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


def main_random():
  """The random programs of the GPU tests (tests/random_programs.py; texts in
  random_programs.json) through the reference: its analysis of each program and,
  where its emitted CPU loops compile, their result on seeded inputs.  Writes
  random_analysis.json, random_manifest.json and random.<key>.npz."""
  with open(os.path.join(HERE, 'random_programs.json')) as f:
    programs = json.load(f)
  analysis, manifest = {}, {}
  with tempfile.TemporaryDirectory() as wd:
    for key in sorted(programs):
      entry = programs[key]
      try:
        st = build_stencil(None, text=entry['text'])
        ana, text = analysis_of(st)
      except Exception as e:      # the reference itself rejects the program
        manifest['random.' + key] = dict(reference='raises %s' % type(e).__name__)
        print(key, 'reference raises', type(e).__name__, e)
        continue
      for stage in ana['stages']:      # (the point sets are large and derivable)
        stage.pop('window')
      analysis[key] = ana
      if any(min(t['loop_lo'] + t['loop_hi_margin']) < 0 for t in ana['stages']):
        # a window that excludes the store point: the emitted loops start at a
        # negative index or print `dims[0]--1`; either way no defined answer
        manifest['random.' + key] = dict(
            reference_cpu_path='one-sided window: loops leave the arrays')
        print(key, ': one-sided window, no defined reference answer')
        continue
      deep = st.iterate >= 8
      dims = ((100, 96) if deep else (45, 41)) if st.dim == 2 else (
          (44, 40, 38) if key.startswith('cube') else (21, 19, 17))
      rng = np.random.default_rng(SEED)
      shape = tuple(reversed(dims))
      inputs = []
      for htype in st.input_types:
        dt = NP_TYPES[hutil.get_c_type(htype)]
        if np.issubdtype(dt, np.floating):
          inputs.append((rng.random(shape, dtype=np.float32) +
                         np.float32(0.5)).astype(dt))
        else:
          inputs.append(rng.integers(0, 200, size=shape).astype(dt))
      # every run starts from a fresh harness tag: programs share app names
      st_tag = st.app_name
      st.app_name = '%s_%s' % (st_tag, key)
      try:
        r0 = run_reference(st, text, dims, inputs, '-O0', wd)
        r2 = run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
      except subprocess.CalledProcessError:
        manifest['random.' + key] = dict(reference_cpu_path='does not compile or run')
        print(key, ': the reference\'s emitted CPU loops do not compile / run')
        continue
      finally:
        st.app_name = st_tag
      outs = {n: r0[n] for n in st.output_names}
      for name in outs:
        if not np.array_equal(r0[name], r2[name], equal_nan=True):
          raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
      fx = 'random.%s.npz' % key
      payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
      payload.update({'out_' + n: a for n, a in outs.items()})
      np.savez_compressed(os.path.join(HERE, fx), **payload)
      manifest[fx] = dict(key=key, dims=list(dims), iterate=st.iterate,
                          sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                  for n, a in outs.items()})
      print('wrote', fx)
  with open(os.path.join(HERE, 'random_analysis.json'), 'w') as f:
    json.dump(analysis, f, sort_keys=True, separators=(',', ':'))
  with open(os.path.join(HERE, 'random_manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


def main():
  if len(sys.argv) > 1 and sys.argv[1] == '--extra':
    return main_extra()
  if len(sys.argv) > 1 and sys.argv[1] == '--random':
    return main_random()
  samples = sorted(os.listdir(os.path.join(REF, 'tests/src')))
  analysis = {}
  manifest = {}
  with tempfile.TemporaryDirectory() as wd:
    for fname in samples:
      app = fname[:-5]
      path = os.path.join(REF, 'tests/src', fname)
      base = build_stencil(path)
      multi = len(base.input_names) == len(base.output_names) and \
          base.input_types == base.output_types
      iterates = [1, 2, 3, 4] if multi else [1]
      for it in iterates:
        st = build_stencil(path, iterate=it)
        ana, text = analysis_of(st)
        key = '%s.iter%d' % (app, it)
        analysis[key] = ana
        cases = CASES_2D if st.dim == 2 else CASES_3D
        for dims in cases:
          for kind in ('ramp', 'random'):
            rng = np.random.default_rng(SEED)
            inputs = make_inputs(st, dims, kind, rng)
            r0 = run_reference(st, text, dims, inputs, '-O0', wd)
            r2 = run_reference(st, text, dims, inputs,
                               '-O2 -ffp-contract=off', wd)
            for name in r0:
              if not np.array_equal(r0[name], r2[name], equal_nan=True):
                raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
            fx = '%s.%s.%s.npz' % (key, 'x'.join(map(str, dims)), kind)
            payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
            payload.update({'out_' + n: a for n, a in r0.items()})
            np.savez_compressed(os.path.join(HERE, fx), **payload)
            manifest[fx] = dict(
                key=key, dims=list(dims), kind=kind,
                sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                        for n, a in r0.items()})
            print('wrote', fx)
    # BASELINE cfg1: blur 2000x100 ramp, sha256 + full result
    st = build_stencil(os.path.join(REF, 'tests/src/blur.soda'))
    ana, text = analysis_of(st)
    dims = (2000, 100)
    inputs = make_inputs(st, dims, 'ramp', np.random.default_rng(SEED))
    r0 = run_reference(st, text, dims, inputs, '-O0', wd)
    fx = 'blur.iter1.2000x100.ramp.npz'
    np.savez_compressed(os.path.join(HERE, fx),
                        **{'out_' + n: a for n, a in r0.items()})
    manifest[fx] = dict(key='blur.iter1', dims=list(dims), kind='ramp',
                        sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                for n, a in r0.items()})
  with open(os.path.join(HERE, 'analysis.json'), 'w') as f:
    json.dump(analysis, f, indent=1, sort_keys=True)
  with open(os.path.join(HERE, 'manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
  main()
