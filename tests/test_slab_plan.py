"""The plan of a multi-GPU slab run (soda-compiler_amd/csrc/slab_plan.cpp) on the CPU: it
is pure arithmetic over the program and the slab descriptor, so a probe built with the
host compiler alone (tests/slab_probe.cpp) plans full-size runs here, and every rank's
plan - layout, every super-step's messages, pieces, margins and where the next exchange
goes out - is compared line by line with what soda_hip/runtime/dist.py, the independent
implementation, does: its own drivers (run_slab, run_recut) run over a recording engine,
a recording schedule and a recording torch.distributed, on arrays without memory."""
import functools
import os
import struct
import subprocess

import pytest
import torch

from soda_hip import frontend
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import capi, host
from soda_hip.runtime import dist as sdist

from conftest import ROOT, SAMPLES

CSRC = os.path.join(ROOT, 'soda-compiler_amd', 'csrc')
SOURCES = [os.path.join(ROOT, 'tests', 'slab_probe.cpp'), os.path.join(CSRC, 'slab_plan.cpp'),
           os.path.join(CSRC, 'schedule.cpp')]
FIELD_APPS = ('wave2d', 'fdtd2d', 'skewpair2d', 'wave3d', 'maxwell3d')
SERIAL, BANDS = capi.SLAB_SERIAL, capi.SLAB_BANDS_FIRST
TALLY = dict(cases=0, lines=0, differing=0)     # what the record of a run quotes


def build_probe(exe, *flags):
  # the host compiler alone: no ROCm include path, no HIP library
  subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', *flags, '-I',
                         os.path.join(ROOT, 'include'), '-I', CSRC, *SOURCES, '-o', str(exe)])
  return str(exe)


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  return build_probe(tmp_path_factory.mktemp('slab') / 'slab_probe')


@functools.lru_cache(maxsize=None)
def program(app):
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  return specmod.spec_from_stencil(frontend.load(path))


def reach_of(spec):
  return spec['radius']['lo'][-1], spec['radius']['hi'][-1]


def case(app, dims, world, exchange, iterate, order=SERIAL, static=True, reach=None):
  """One run: every rank of it is planned and compared.  Static cut: `exchange` is the
  period wanted (soda_hip_slab_exchange / SlabPlan clamp it)."""
  return dict(app=app, dims=tuple(dims), world=world, exchange=exchange, iterate=iterate,
              order=order, static=static, reach=reach or reach_of(program(app)))


def descriptor(c, who, **changed):
  slab = capi.Slab(rank=who, world=c['world'], reach_lo=c['reach'][0], reach_hi=c['reach'][1],
                   exchange=c['exchange'], order=c['order'],
                   cut=capi.SLAB_CUT_STATIC if c['static'] else capi.SLAB_CUT_RECUT)
  for d, v in enumerate(c['dims']):
    slab.dims[d] = v
  slab.own_first, slab.own_last = sdist.slab_bounds(c['dims'][-1], c['world'])[who]
  for name, value in changed.items():
    setattr(slab, name, value)
  return slab


def ask(probe, path, app, requests):
  """requests = [(iterate, fields, wanted, descriptor)] of one program -> the probe's lines
  per request, the 'case' line dropped and its rc in front: [(rc, [line])]."""
  desc = host.program_desc(specmod.inline_pointwise(program(app)))
  req = bytes(desc) + struct.pack('=i', len(requests))
  for iterate, fields, wanted, slab in requests:
    req += struct.pack('=3i', iterate, fields, wanted) + bytes(slab)
  path.write_bytes(req)
  out = []
  for line in subprocess.check_output([probe, str(path)], text=True).splitlines():
    if line.startswith('case '):
      out.append((int(line.split()[3]), []))
    else:
      out[-1][1].append(line)
  assert len(out) == len(requests)
  return out


# ---- what dist.py does, in the probe's words ----------------------------------------------
class Wire:
  """torch.distributed's point-to-point interface (as Recorder of
  tests/test_gpu_fields_slabs.py), recording every message: its first row and rows."""
  isend, irecv = 's', 'r'

  def __init__(self):
    self.ops = []

  def P2POp(self, op, rows, peer):
    per_row = 1
    for n in rows.shape[1:]:
      per_row *= n
    assert rows.storage_offset() % per_row == 0
    self.ops.append((op, peer, rows.storage_offset() // per_row, rows.shape[0]))

  def batch_isend_irecv(self, ops):
    return []


class Order:
  """SerialSchedule / StreamSchedule, recording where the drivers call it."""
  skip_exchange = False

  def __init__(self, overlapped, wire, log):
    self.overlapped, self.wire, self.log = overlapped, wire, log

  def exchange(self, fn):
    start = len(self.wire.ops)
    fn()
    self.log.append(('X', self.wire.ops[start:]))

  def before_super_step(self):
    self.log.append(('S',))

  def after_bands(self):
    self.log.append(('B',))


class Engine:
  def __init__(self, log):
    self.log = log

  def sweep(self, src, dst, local_dims, iterations, valid_lo, valid_hi, rows=None,
            final_only=False):
    self.log.append(('P', rows or (0, local_dims[-1]), final_only, valid_lo, valid_hi,
                     iterations))


def flat(margins):
  """one (lo or hi) margin, or one per field -> the values in the probe's order"""
  if margins and hasattr(margins[0], '__len__'):
    return [v for m in margins for v in m]
  return list(margins)


def expected(c, rank):
  """The probe's lines for one rank of a run, from dist.py: (rc, lines)."""
  spec = program(c['app'])
  n = len(spec['inputs'])
  dims = list(c['dims'])
  try:
    plan = sdist.make_plan(c['static'], dims, rank, c['world'], c['reach'][0], c['reach'][1],
                           c['exchange'], c['iterate'])
  except ValueError as e:
    return -8, ['error %s' % e]
  several = n > 1
  table = (specmod.iteration_field_margins if several else specmod.iteration_margins)(
      spec, c['iterate'])
  types = specmod.tensor_c_types(spec)
  shape = tuple(reversed(plan.local_dims))
  levels = [[torch.empty(shape, device='meta') for _ in range(n)] for _ in range(3)]
  arrays = levels if several else [level[0] for level in levels]
  wire, log = Wire(), []
  sdist.run_plan(Engine(log), plan, arrays, c['iterate'], sdist.table_margins_of(table), wire,
                 schedule=Order(c['order'] == BANDS, wire, log))
  # the drivers' calls, super-step by super-step: [X] S P.. [B X P] ... and one S at the end
  steps, sent, carried, banded = [], None, None, False
  for event in log:
    if event[0] == 'X':
      group = event[1]
      assert group == group[:len(group) // n] * n      # the same rows for every field
      if banded:      # beside the interior: the NEXT super-step's group
        steps[-1]['after'] = len(steps[-1]['pieces']) - 1
        carried, banded = group[:len(group) // n], False
      else:
        sent = group[:len(group) // n]
    elif event[0] == 'S':
      steps.append(dict(before=carried if sent is None else sent, pieces=[], after=-1))
      sent = None
    elif event[0] == 'B':
      banded = True
    else:
      steps[-1]['pieces'].append(event[1:])
  steps.pop()
  if c['static']:
    spans, done = [], 0
    while done < c['iterate']:
      spans.append((done, min(plan.exchange, c['iterate'] - done)))
      done += spans[-1][1]
  else:
    spans = plan.steps
  assert len(steps) == len(spans)
  (first, last), offset = sdist.result_rows(plan)
  sizes = [specmod.ELEM_SIZE[types[t['name']]] for t in spec['inputs']]
  inner = 1
  for v in dims[:-1]:
    inner *= v
  lines = ['period %d' % plan.exchange] if c['static'] else []
  lines.append('layout %d %d %d %d %d bytes %s' % (
      plan.local_extent, plan.ghost_lo, first, last, offset,
      ' '.join(str(size * inner) for size in sizes)))
  for (done, step), st in zip(spans, steps):
    lines.append('S %d %d %d' % (done, step, st['after']))
    lines += ['M %s %d %d %d' % m for m in (st['before'] or [])]
    for (r0, r1), final_only, lo, hi, iterations in st['pieces']:
      assert iterations == step
      lines.append('P %d %d %d lo %s hi %s' % (r0, r1, final_only,
                                               ' '.join(map(str, flat(lo))),
                                               ' '.join(map(str, flat(hi)))))
  return 0, lines


def compare(probe, tmp_path, cases):
  """Every rank of every case: the probe's lines against dist.py's.  Returns the probe's
  lines per (case index, rank)."""
  by_app = {}
  for i, c in enumerate(cases):
    by_app.setdefault(c['app'], []).append(i)
  got = {}
  for app, indices in by_app.items():
    n = len(program(app)['inputs'])
    keys = [(i, rank) for i in indices for rank in range(cases[i]['world'])]
    requests = [(cases[i]['iterate'], n, cases[i]['exchange'] if cases[i]['static'] else 0,
                 descriptor(cases[i], rank)) for i, rank in keys]
    for key, answer in zip(keys, ask(probe, tmp_path / (app + '.req'), app, requests)):
      got[key] = answer
  for (i, rank), (rc, lines) in got.items():
    want_rc, want = expected(cases[i], rank)
    differing = sum(a != b for a, b in zip(lines, want)) + abs(len(lines) - len(want))
    TALLY['cases'] += 1
    TALLY['lines'] += len(want)
    TALLY['differing'] += differing
    assert rc == want_rc and lines == want, (cases[i], rank)
  return {key: lines for key, (rc, lines) in got.items()}


def far_messages(lines, rank):
  """messages of a rank's plan, sends and receives, whose partner is not a neighbour"""
  return sum(1 for l in lines if l.startswith('M ') and abs(int(l.split()[2]) - rank) > 1)


# ---- the static cut -----------------------------------------------------------------------
def test_static_cut(probe, tmp_path):
  cases = []
  for order in (SERIAL, BANDS):
    for world in (1, 2, 3, 4, 8):
      for wanted in (1, 3, 4, 10):
        cases.append(case('jacobi2d', (64, 48), world, wanted, 10, order))
      cases.append(case('jacobi3d', (20, 18, 16), world, 2, 5, order))
      # one-sided and uneven reach
      for reach in ((2, 1), (1, 0), (0, 1), (1, 3)):
        cases.append(case('jacobi2d', (64, 48), world, 2, 7, order, reach=reach))
    cases.append(case('jacobi2d', (16384, 16384), 4, 96, 1000, order))
    cases.append(case('jacobi2d', (16384, 16384), 8, 96, 1000, order))
    cases.append(case('jacobi3d', (512, 512, 512), 8, 32, 200, order))
  got = compare(probe, tmp_path, cases)
  banded = [i for i, c in enumerate(cases) if c['order'] == BANDS and c['world'] > 1]
  assert any(l.startswith('S ') and not l.endswith(' -1') for i in banded for l in got[i, 0])
  # a one-sided window ships nothing one way
  i = cases.index(case('jacobi2d', (64, 48), 2, 2, 7, SERIAL, reach=(1, 0)))
  assert [l for l in got[i, 0] if l.startswith('M')][:1] == ['M s 1 22 2']
  assert [l for l in got[i, 1] if l.startswith('M')][:1] == ['M r 0 0 2']


def test_thin_slabs_are_swept_whole(probe, tmp_path):
  """64x23 on 4 ranks, reach 2, 3 wanted: the period clamps to 2 and no rank has rows for
  two bands and an interior (the band rows of the first rank would start below 0)."""
  cases = [case('jacobi2d', (64, 23), 4, 3, 6, order, reach=(2, 2)) for order in (SERIAL, BANDS)]
  got = compare(probe, tmp_path, cases)
  for rank in range(4):
    assert got[0, rank] == got[1, rank] and got[1, rank][0] == 'period 2'
    pieces = [l.split() for l in got[1, rank] if l.startswith('P')]
    assert len(pieces) == 3 and all(p[1] == '0' and p[3] == '0' for p in pieces)


# ---- the re-cut ---------------------------------------------------------------------------
def test_recut(probe, tmp_path):
  cases = []
  for order in (SERIAL, BANDS):
    for world in (1, 2, 3, 4, 8):
      cases.append(case('jacobi2d', (64, 48), world, 3, 10, order, static=False))
      cases.append(case('jacobi3d', (20, 18, 16), world, 2, 5, order, static=False))
      cases.append(case('jacobi2d', (64, 48), world, 2, 7, order, static=False, reach=(2, 1)))
      cases.append(case('jacobi2d', (64, 48), world, 4, 9, order, static=False, reach=(0, 1)))
  compare(probe, tmp_path, cases)


def test_recut_full_size(probe, tmp_path):
  """The runs the stand-in's small shapes cannot reach: thin slabs whose partners lie beyond
  the neighbours, and ranks that end with no rows."""
  cases = [case(*a, order=BANDS, static=False, **k) for a, k in (
      (('jacobi2d', (16384, 16384), 4, 96, 1000), {}),
      (('jacobi2d', (16384, 16384), 8, 96, 1000), {}),
      (('jacobi3d', (512, 512, 512), 8, 16, 200), {}),
      (('jacobi3d', (512, 512, 512), 8, 32, 200), {}),
      (('jacobi2d', (40, 23), 3, 3, 5), dict(reach=(2, 2))),
      (('jacobi2d', (40, 23), 3, 3, 11), {}))]      # one row left: two ranks end with none
  cases += [dict(c, order=SERIAL) for c in cases]
  got = compare(probe, tmp_path, cases)
  for i, want in ((0, 0), (1, 0), (2, 12), (3, 44), (4, 4)):
    c = cases[i]
    assert sum(far_messages(got[i, rank], rank) for rank in range(c['world'])) == want
    plans = [sdist.RecutPlan(list(c['dims']), rank, c['world'], *c['reach'], c['exchange'],
                             c['iterate']) for rank in range(c['world'])]
    assert sum(1 for p in plans for s in range(len(p.steps)) for side in p.messages(s)
               for q, _ in side if abs(q - p.rank) > 1) == want
  layouts = [got[5, rank][0].split() for rank in range(3)]
  assert sum(int(l[4]) - int(l[3]) for l in layouts) == 1
  assert sum(l[3] == l[4] for l in layouts) == 2
  for rank in range(3):     # a rank that ends without rows swept nothing in the last super-step
    tail = got[5, rank][max(k for k, l in enumerate(got[5, rank]) if l.startswith('S')):]
    assert any(l.startswith('P') for l in tail) == (layouts[rank][3] != layouts[rank][4])


# ---- programs over several fields ---------------------------------------------------------
@pytest.mark.parametrize('app', FIELD_APPS)
def test_programs_over_several_fields(probe, tmp_path, app):
  """At the shapes of tests/test_gpu_fields_slabs.py: each field's own margins on the global
  sides of every dimension, row_bytes per field."""
  spec = program(app)
  dims, iterate = ((64, 48), 4) if spec['dim'] == 2 else ((20, 18, 16), 3)
  cases = [case(app, dims, world, wanted, iterate)
           for world in (1, 2, 3, 4) for wanted in (1, 2, iterate)]
  got = compare(probe, tmp_path, cases)
  n, dim = len(spec['inputs']), spec['dim']
  assert n > 1
  # world 2, an exchange every iteration: the upper rank's last sweep starts from each
  # field's own margins after iterate - 1 iterations, its lower side cut
  assert (cases[3]['world'], cases[3]['exchange']) == (2, 1)
  last = [l.split() for l in got[3, 1] if l.startswith('P')][-1]
  own = specmod.iteration_field_margins(spec, iterate)[iterate - 2]
  assert last[5:5 + n * dim] == [str(0 if d == dim - 1 else v) for lo, _ in own
                                 for d, v in enumerate(lo)]
  assert last[6 + n * dim:] == [str(v) for _, hi in own for v in hi]
  assert len({(lo, hi) for lo, hi in own}) > 1 or app == 'wave3d'
  sizes = specmod.tensor_c_types(spec)
  inner = dims[0] * (dims[1] if dim == 3 else 1)
  assert got[3, 1][1].split()[7:] == [str(specmod.ELEM_SIZE[sizes[t['name']]] * inner)
                                      for t in spec['inputs']]


# ---- refusals -----------------------------------------------------------------------------
def test_refusals(probe, tmp_path):
  """Every refusal of the plan: the code and the text the callers of soda_hip_run_slab,
  soda_hip_run_slab_fields and soda_hip_slab_layout are promised."""
  c = case('jacobi2d', (512, 400), 2, 8, 4)
  recut = dict(c, static=False)
  asks = [
      (0, 1, 0, descriptor(c, 0), 'iterate must be >= 1'),
      (4, 1, 0, descriptor(c, 0, order=7), 'slab order 7'),
      (4, 1, 0, descriptor(c, 0, cut=9), 'slab cut 9'),
      (4, 0, 0, descriptor(c, 0, cut=9), 'slab cut 9'),
      (4, 1, 0, descriptor(c, 0, exchange=0), 'slab descriptor out of range'),
      (4, 1, 0, descriptor(c, 0, rank=2), 'slab descriptor out of range'),
      (4, 1, 0, descriptor(c, 0, reach_lo=-1), 'slab descriptor out of range'),
      (4, 1, 0, descriptor(c, 0, own_last=0), 'slab of 0 own rows is thinner than its ghost '
       'regions (8 x 1)'),
      (4, 1, 0, descriptor(c, 0, exchange=201), 'slab of 200 own rows is thinner than its '
       'ghost regions (201 x 1)'),
      (4, 1, 0, descriptor(recut, 0, own_last=150), 're-cut slabs: rank 0 of 2 must be handed '
       'rows [0, 200) of 400 (the even cut), not [0, 150)'),
      (0, 0, 0, descriptor(recut, 0), 'slab descriptor out of range'),
      (4, 1, 0, descriptor(recut, 0, exchange=0), 'slab descriptor out of range'),
      (4, 1, 3, descriptor(case('jacobi2d', (64, 7), 4, 3, 4, reach=(2, 2)), 0),
       'cannot cut 7 rows into 4 slabs: the smallest slab (1 rows) is thinner than the '
       'stencil reach (2)'),
      (4, 1, 0, descriptor(dict(c, dims=(512, 0)), 0, cut=capi.SLAB_CUT_RECUT),
       'slab descriptor: 0 rows')]
  answers = ask(probe, tmp_path / 'refused.req', 'jacobi2d', [a[:4] for a in asks])
  for (rc, lines), a in zip(answers, asks):
    assert rc == -8 and lines == ['error ' + a[4]], a
  # the layout alone looks at neither `iterate` nor the order of a static cut
  (rc, lines), = ask(probe, tmp_path / 'layout.req', 'jacobi2d',
                     [(0, 0, 0, descriptor(c, 1, order=7))])
  assert rc == 0 and lines == ['layout 208 8 200 400 8 bytes']
  # the NULL path
  (rc, lines), = ask(probe, tmp_path / 'null.req', 'jacobi2d', [(4, 1, -1, descriptor(c, 0))])
  assert rc == -12 and lines == ['error NULL argument']
  # programs the slab drivers do not take
  (rc, lines), = ask(probe, tmp_path / 'outchain.req', 'outchain',
                     [(1, 1, 0, descriptor(case('outchain', (64, 48), 2, 1, 1), 0))])
  assert rc == -8 and lines == ['error slabs: programs with as many outputs as inputs']
  for fields in (0, 2):
    (rc, lines), = ask(probe, tmp_path / 'wave2d.req', 'wave2d',
                       [(4, fields, 0, descriptor(case('wave2d', (64, 48), 2, 1, 4,
                                                       static=False), 0))])
    assert rc == -8 and lines == ['error slabs: static cut only for programs over several '
                                  'fields']


# ---- the probe under the sanitizers -------------------------------------------------------
def test_the_probe_runs_clean_under_the_sanitizers(tmp_path):
  """Host code only, a stand-alone program: the full-size requests once more, through a
  probe built with -fsanitize=address,undefined."""
  exe = build_probe(tmp_path / 'slab_probe_san', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all')
  cases = [case('jacobi2d', (16384, 16384), 8, 96, 1000, BANDS, static=static)
           for static in (True, False)]
  cases += [case('jacobi3d', (512, 512, 512), 8, e, 200, BANDS, static=False) for e in (16, 32)]
  cases += [case('jacobi2d', (40, 23), 3, 3, 11, BANDS, static=False),
            case('jacobi2d', (64, 23), 4, 3, 6, BANDS, reach=(2, 2))]
  for app in ('jacobi2d', 'jacobi3d'):
    requests = [(c['iterate'], 1, c['exchange'] if c['static'] else 0, descriptor(c, rank))
                for c in cases if c['app'] == app for rank in range(c['world'])]
    for rc, lines in ask(exe, tmp_path / (app + '.req'), app, requests):
      assert rc == 0 and lines
  requests = [(4, 2, 2, descriptor(case('wave2d', (64, 48), 3, 2, 4), rank)) for rank in range(3)]
  for rc, lines in ask(exe, tmp_path / 'wave2d.req', 'wave2d', requests):
    assert rc == 0 and lines
