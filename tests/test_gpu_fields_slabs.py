"""Programs over several fields, resumed and as slabs, on a real MI355X through the C ABI.

Resume: t1 iterations, then t2 more with every field's own valid region
(soda_hip_sweep_fields, margins from soda_hip_plan_field_margins), end bit for bit on the
boxes of t1 + t2 iterations in one call - the reference's fixtures - with the fused kernels
and per stage, in guarded arenas.  Slabs: soda_hip_run_slab_fields over the test-only RCCL
stand-in (worlds 2 to 4, ranks = host threads) and with world 1 between guards, and the
Python driver (gloo ranks sharing the GPU) on the same programs.

On the commit before these entries existed the binding has no soda_hip_plan_field_margins
and the slab entries answer SODA_HIP_ERR_CONSTRAINT ("slabs: one-input one-output
programs") for these programs."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from soda_hip.codegen import spec as specmod
from soda_hip.runtime import capi
from soda_hip.runtime import dist as sdist

import gpu_util
from conftest import ROOT
from test_gpu_parity import build_rccl_standin

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
APPS_2D = ('wave2d', 'fdtd2d', 'mixpair2d', 'skewpair2d')
APPS_3D = ('wave3d', 'maxwell3d')
SLAB_APPS = ('wave2d', 'skewpair2d', 'fdtd2d', 'wave3d', 'maxwell3d')
CHILD_SECONDS = 150      # every GPU child process runs under a limit of its own

_CACHE = {}


def opened(app):
  if app not in _CACHE:
    prog = gpu_util.open_prebuilt(app)
    _CACHE[app] = (prog, gpu_util.make_oracle(prog.spec))
  return _CACHE[app]


def fixture_of(app, iterate, dims):
  sub = 'fields' if len(dims) == 2 else 'fields3d'
  return np.load(os.path.join(GOLDEN, sub, '%s.iter%d.%s.random.npz' % (
      app, iterate, 'x'.join(map(str, dims)))))


def own_box(spec, name, dims, iterate):
  lo, hi = specmod.iteration_boxes(spec, iterate)[-1][name]
  return tuple(slice(-lo[d], dims[d] - hi[d]) for d in reversed(range(spec['dim'])))


def same_bits(a, b):
  return np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                        np.ascontiguousarray(b).view(np.uint8))


def resume(prog, inputs, first, more):
  """`first` iterations from a fresh start, then `more` from the raw result - unspecified
  cells and all - with every field's own valid region.  Both in guarded arenas."""
  level, bad, _ = gpu_util.run_guarded(prog, inputs, first)
  assert bad == [], bad
  margins = prog.field_margins(first)
  assert margins == specmod.iteration_field_margins(prog.spec, first)[-1]
  # output j feeds input j (the dtypes agree for these programs)
  level = [a.astype(dt, copy=False) for a, dt in zip(level, prog.in_dtypes)]
  out, bad, _ = gpu_util.run_guarded(prog, level, more, seed=gpu_util.SEED + 1,
                                     valid_lo=[lo for lo, _ in margins],
                                     valid_hi=[hi for _, hi in margins])
  assert bad == [], bad       # guards intact, the inputs bit-identical afterwards
  return out


def check_resumed(app, dims, total, want_of, depths=(2, -1)):
  prog, _ = opened(app)
  spec = prog.spec
  try:
    for max_depth in depths:
      prog.set_max_depth(max_depth)
      for first in range(1, total):
        kinds = {k['kind'] for k, _ in prog.schedule(dims, total - first)}
        assert kinds == ({'fused'} if max_depth > 0 else {'stage'})
        got = resume(prog, want_of('inputs'), first, total - first)
        for name, g in zip(spec['outputs'], got):
          sl = own_box(spec, name, dims, total)
          assert g[sl].size > 0
          assert same_bits(g[sl], want_of(name)[sl]), (app, dims, max_depth, first, name)
  finally:
    prog.set_max_depth(0)


@pytest.mark.parametrize('dims', [(64, 48), (37, 29)])
@pytest.mark.parametrize('app', APPS_2D)
def test_resumed_2d_sweeps_end_on_the_fixture(app, dims):
  """4 = 1 + 3 = 2 + 2 = 3 + 1 against the reference's iterate-4 fixture."""
  data = fixture_of(app, 4, dims)
  spec = opened(app)[0].spec
  inputs = [data['in_' + t['name']] for t in spec['inputs']]
  check_resumed(app, dims, 4, lambda n: inputs if n == 'inputs' else data['out_' + n])


@pytest.mark.parametrize('app', APPS_3D)
def test_resumed_3d_sweeps_end_on_the_fixture(app):
  """3 = 1 + 2 = 2 + 1 against the reference's iterate-3 fixture."""
  dims = (20, 18, 16)
  data = fixture_of(app, 3, dims)
  spec = opened(app)[0].spec
  inputs = [data['in_' + t['name']] for t in spec['inputs']]
  check_resumed(app, dims, 3, lambda n: inputs if n == 'inputs' else data['out_' + n])


@pytest.mark.parametrize('app,dims,total', [
    ('wave2d', (300, 61), 4), ('fdtd2d', (300, 61), 4), ('skewpair2d', (300, 61), 4),
    ('mixpair2d', (300, 61), 4), ('wave3d', (70, 20, 24), 3), ('maxwell3d', (70, 20, 24), 3)])
def test_resumed_sweeps_on_ragged_sizes(app, dims, total):
  """A 2-D size that crosses a strip seam and a 3-D one that crosses a tile, against the
  oracle."""
  prog, orc = opened(app)
  inputs = gpu_util.random_inputs(prog.spec, tuple(reversed(dims)))
  want = orc.run(inputs, iterate=total)
  check_resumed(app, dims, total, lambda n: inputs if n == 'inputs' else want[n])


def test_regions_too_far_apart_are_an_error_not_a_wrong_box():
  prog, _ = opened('wave2d')
  dims = (1000, 48)
  try:
    prog.set_max_depth(1)
    with pytest.raises(capi.SodaHipError, match='limit 255'):
      prog.schedule_fields(dims, 1, valid_lo=[(0, 0), (300, 0)])
    plan = prog.schedule_fields(dims, 1, valid_lo=[(0, 0), (200, 0)])
    assert len(plan) == 1 and plan[0]['lo'] == [200, 1] and plan[0]['hi'] == [999, 47]
  finally:
    prog.set_max_depth(0)


# ---- slabs ------------------------------------------------------------------------------
def slab_inputs(app):
  dims = (64, 48) if app in APPS_2D else (20, 18, 16)
  iterate = 4 if app in APPS_2D else 3
  return dims, iterate, fixture_of(app, iterate, dims)


class Recorder:
  """torch.distributed's point-to-point interface, recording what the Python driver's
  exchange would send."""
  isend, irecv = 'send', 'recv'

  def __init__(self):
    self.sent = []

  def P2POp(self, op, rows, peer):
    if op == 'send':
      self.sent.append(rows.numel() * rows.element_size())
    return None

  def batch_isend_irecv(self, ops):
    return []


def python_driver_traffic(spec, dims, world, exchange, iterate):
  """(messages, bytes) the Python driver sends over the whole run: exchange_ghosts on
  arrays of the slabs' shapes, once per super-step and rank."""
  import torch
  r_lo, r_hi = spec['radius']['lo'][-1], spec['radius']['hi'][-1]
  rec = Recorder()
  for rank in range(world):
    plan = sdist.SlabPlan(list(dims), rank, world, r_lo, r_hi, exchange)
    assert plan.exchange == exchange
    fields = [torch.zeros(tuple(reversed(plan.local_dims))) for _ in spec['inputs']]
    for _ in range(-(-iterate // exchange)):
      sdist.exchange_ghosts(fields, plan, rec)
  return len(rec.sent), sum(rec.sent)


@pytest.mark.parametrize('world', [2, 3, 4])
def test_run_slab_fields_over_the_rccl_standin(tmp_path, world):
  """soda_hip_run_slab_fields, one process, `world` host threads: every rank's own rows of
  every output equal the reference's fixture on that output's own box; the stand-in's
  counters equal the Python driver's messages and bytes."""
  standin = build_rccl_standin(tmp_path)
  cases = []
  for app in SLAB_APPS:
    dims, iterate, data = slab_inputs(app)
    for wanted, max_depth in ((1, 2), (2, -1), (iterate, 2)):
      cases.append([app, list(dims), world, iterate, wanted, max_depth])
      np.savez(tmp_path / ('case%d.in.npz' % (len(cases) - 1)),
               **{k: data[k] for k in data.files if k.startswith('in_')})
  (tmp_path / 'cases.json').write_text(json.dumps(cases))
  r = subprocess.run(
      [sys.executable, os.path.join(ROOT, 'tests', 'rccl_standin_fields_worker.py'), standin,
       str(tmp_path / 'cases.json'), str(tmp_path)], capture_output=True, text=True,
      timeout=CHILD_SECONDS)
  assert r.returncode == 0, r.stderr[-3000:]
  for index, (app, dims, _, iterate, wanted, max_depth) in enumerate(cases):
    spec = gpu_util.load_spec(app)
    _, _, data = slab_inputs(app)
    got = [np.zeros(tuple(reversed(dims)), dtype=data['out_' + o].dtype)
           for o in spec['outputs']]
    metas = []
    for rank in range(world):
      meta = json.load(open(tmp_path / ('case%d.rank%d.json' % (index, rank))))
      own = np.load(tmp_path / ('case%d.rank%d.npz' % (index, rank)))
      for j in range(len(got)):
        got[j][meta['first']:meta['last']] = own['out%d' % j]
      metas.append(meta)
    assert metas[0]['first'] == 0 and metas[-1]['last'] == dims[-1]
    assert all(a['last'] == b['first'] for a, b in zip(metas, metas[1:]))
    period = metas[0]['exchange']
    assert 1 <= period <= wanted
    for j, o in enumerate(spec['outputs']):
      sl = own_box(spec, o, dims, iterate)
      assert data['out_' + o][sl].size > 0
      assert same_bits(got[j][sl], data['out_' + o][sl]), (app, world, wanted, max_depth, o)
    messages, nbytes = python_driver_traffic(spec, dims, world, period, iterate)
    assert messages > 0
    for meta in metas:
      assert meta['exchanges'] == -(-iterate // period)
      assert (meta['messages'], meta['bytes']) == (messages, nbytes), (app, world, wanted)


@pytest.mark.parametrize('app', SLAB_APPS)
def test_run_slab_fields_with_one_rank_between_guards(app):
  """world = 1: the three arrays of every field sit between guards; `a` comes back bit for
  bit, nothing outside an array is touched, the result equals the fixture per output box."""
  prog, _ = opened(app)
  spec = prog.spec
  dims, iterate, data = slab_inputs(app)
  n = len(spec['inputs'])
  shape = tuple(reversed(dims))
  inputs = {'a%d' % j: data['in_' + t['name']] for j, t in enumerate(spec['inputs'])}
  layout = [('a%d' % j, 'in', shape, prog.in_dtypes[j]) for j in range(n)]
  layout += [('%s%d' % (x, j), 'out', shape, prog.in_dtypes[j]) for x in 'bc' for j in range(n)]
  try:
    for exchange, max_depth in ((1, 2), (2, -1), (iterate, 2)):
      prog.set_max_depth(max_depth)
      arena = gpu_util.Arena(layout, skews=gpu_util.pool_skews(3 * n, 4 if app != 'mixpair2d' else 2))
      hull = prog.margins(1)
      slab = capi.Slab(rank=0, world=1, reach_lo=hull[0][-1], reach_hi=hull[1][-1],
                       exchange=exchange, own_first=0, own_last=dims[-1])
      for d, v in enumerate(dims):
        slab.dims[d] = v
      dev = gpu_util.DeviceArena(arena, inputs)
      result, count = (ctypes.c_void_p * n)(), ctypes.c_int()
      try:
        ptrs = [(ctypes.c_void_p * n)(*[dev.ptr('%s%d' % (x, j)) for j in range(n)])
                for x in 'abc']
        capi.check(capi.lib().soda_hip_run_slab_fields(
            prog.handle, ctypes.byref(slab), None, ptrs[0], ptrs[1], ptrs[2], iterate, None,
            result, ctypes.byref(count)))
        names = [{dev.ptr('b%d' % j): 'b%d' % j, dev.ptr('c%d' % j): 'c%d' % j}.get(result[j])
                 for j in range(n)]
      finally:
        bad, outs = dev.finish()
      assert bad == [], bad
      assert count.value == 0 and None not in names
      for j, o in enumerate(spec['outputs']):
        sl = own_box(spec, o, dims, iterate)
        assert same_bits(outs[names[j]][sl], data['out_' + o][sl]), (app, exchange, o)
  finally:
    prog.set_max_depth(0)


def free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  return port


@pytest.mark.parametrize('app', ['wave2d', 'wave3d'])
def test_python_driver_with_two_ranks_on_one_gpu(tmp_path, app):
  """soda_hip.runtime.dist: HipEngine and run_slab with one array per field and the
  library's own per-field margins, two gloo ranks sharing the GPU."""
  dims, iterate, data = slab_inputs(app)
  spec = gpu_util.load_spec(app)
  np.savez(tmp_path / 'in.npz', **{k: data[k] for k in data.files if k.startswith('in_')})
  world = 2
  env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(free_port()),
             WORLD_SIZE=str(world), OMP_NUM_THREADS='2')
  procs = [subprocess.Popen(
      [sys.executable, os.path.join(ROOT, 'tests', 'dist_gpu_fields_worker.py'), app,
       str(tmp_path / 'in.npz'), str(iterate), '2', '2', str(tmp_path)],
      env=dict(env, RANK=str(rank), LOCAL_RANK=str(rank))) for rank in range(world)]
  try:
    for p in procs:
      assert p.wait(timeout=CHILD_SECONDS) == 0
  finally:
    for p in procs:
      if p.poll() is None:
        p.kill()
  got = [np.zeros(tuple(reversed(dims)), dtype=np.float32) for _ in spec['outputs']]
  for rank in range(world):
    meta = json.load(open(tmp_path / ('rank%d.json' % rank)))
    own = np.load(tmp_path / ('rank%d.npz' % rank))
    assert meta['exchange'] == 2 and meta['exchanges'] == -(-iterate // 2)
    for j in range(len(got)):
      got[j][meta['start']:meta['stop']] = own['out%d' % j]
  for j, o in enumerate(spec['outputs']):
    sl = own_box(spec, o, dims, iterate)
    assert data['out_' + o][sl].size > 0
    assert same_bits(got[j][sl], data['out_' + o][sl]), (app, o)
