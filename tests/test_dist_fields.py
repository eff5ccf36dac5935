"""Slabs over SEVERAL fields (soda_hip.runtime.dist: run_slab, exchange_ghosts and
SlabPlan.valid_margins with a list of arrays per level and a margin per field) under gloo
on the CPU, with an engine built on the oracle: worlds 2, 3 and 4, the programs with
output j feeding input j, exchange periods 1, 2 and the whole run.

Every rank's own rows of every output equal one process's on every cell of that output's
OWN box (the outputs' boxes differ), and one group per super-step carries one send and
one receive per field and neighbour."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import dist as sdist
from oracle import soda_oracle

from conftest import ROOT, SAMPLES

PROGRAMS = [('wave2d', (64, 48)), ('skewpair2d', (64, 48)), ('fdtd2d', (64, 48)),
            ('wave3d', (20, 18, 16)), ('maxwell3d', (20, 18, 16))]
ITERATES = (3, 4)


def free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  return port


def load(app):
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  return specmod.spec_from_stencil(frontend.load(path))


def admitted(spec, dims, world, exchange):
  """The thin-slab rule (SlabPlan): the ghost region of `exchange` iterations is not
  deeper than the thinnest slab."""
  r_lo, r_hi = spec['radius']['lo'][-1], spec['radius']['hi'][-1]
  try:
    return sdist.SlabPlan(dims, 0, world, r_lo, r_hi, exchange).exchange == exchange
  except ValueError:
    return False


def cases_of(world):
  cases = []
  for app, dims in PROGRAMS:
    spec = load(app)
    for iterate in ITERATES:
      for exchange in sorted({1, 2, iterate}):
        if admitted(spec, list(dims), world, exchange):
          cases.append((app, list(dims), iterate, exchange))
  return cases


def test_every_program_runs_on_three_or_more_ranks():
  for app, _ in PROGRAMS:
    assert any(c[0] == app for world in (3, 4) for c in cases_of(world)), app
    for world in (2, 3, 4):      # ... and on every world with several periods
      assert len({c[3] for c in cases_of(world) if c[0] == app}) >= 2, (app, world)


@pytest.fixture(scope='module')
def single_process():
  """{(app, iterate): ([inputs], {output: array})}: one process's answer, computed once"""
  memo = {}

  def get(app, dims, iterate):
    if (app, iterate) not in memo:
      spec = load(app)
      rng = np.random.default_rng(99)
      full = [rng.random(tuple(reversed(dims)), dtype=np.float32) for _ in spec['inputs']]
      memo[app, iterate] = soda_oracle.Oracle(spec).run(full, iterate=iterate)
    return memo[app, iterate]
  return get


@pytest.mark.parametrize('world', [2, 3, 4])
def test_field_slabs_match_single_process(tmp_path, world, single_process):
  cases = cases_of(world)
  assert cases
  (tmp_path / 'cases.json').write_text(json.dumps(cases))
  env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(free_port()),
             WORLD_SIZE=str(world), OMP_NUM_THREADS='2')
  procs = [subprocess.Popen(
      [sys.executable, os.path.join(ROOT, 'tests', 'dist_fields_worker.py'),
       str(tmp_path / 'cases.json'), str(tmp_path)],
      env=dict(env, RANK=str(rank), LOCAL_RANK=str(rank))) for rank in range(world)]
  for p in procs:
    assert p.wait(timeout=300) == 0
  for index, (app, dims, iterate, exchange) in enumerate(cases):
    spec = load(app)
    n = len(spec['inputs'])
    want = single_process(app, dims, iterate)
    boxes = specmod.iteration_boxes(spec, iterate)[-1]
    got = [np.full(tuple(reversed(dims)), np.nan, dtype=np.float32) for _ in range(n)]
    metas = []
    for rank in range(world):
      meta = json.load(open(tmp_path / ('case%d.rank%d.json' % (index, rank))))
      own = np.load(tmp_path / ('case%d.rank%d.npz' % (index, rank)))
      for j in range(n):
        got[j][meta['start']:meta['stop']] = own['out%d' % j]
      metas.append(meta)
    assert metas[0]['start'] == 0 and metas[-1]['stop'] == dims[-1]
    assert all(a['stop'] == b['start'] for a, b in zip(metas, metas[1:]))
    for j, o in enumerate(spec['outputs']):
      lo, hi = boxes[o]
      box = tuple(slice(-lo[d], dims[d] - hi[d]) for d in reversed(range(spec['dim'])))
      assert want[o][box].size > 0, (app, o)
      # every cell of the output's own box, bit for bit, whichever rank holds it
      assert np.array_equal(got[j][box], want[o][box]), (app, iterate, exchange, o)
    # one group per super-step; in it one send and one receive per field and neighbour
    # (a window that reaches one way only has nothing to ship the other way)
    r_lo, r_hi = spec['radius']['lo'][-1], spec['radius']['hi'][-1]
    steps = -(-iterate // exchange)
    row_bytes = 4 * int(np.prod(dims[:-1]))
    for rank, meta in enumerate(metas):
      assert meta['exchanges'] == steps and len(meta['groups']) == steps
      for group in meta['groups']:
        expected = []
        for _ in range(n):
          if rank > 0:
            expected += [['send', rank - 1, exchange * r_hi * row_bytes],
                         ['recv', rank - 1, exchange * r_lo * row_bytes]]
          if rank < world - 1:
            expected += [['send', rank + 1, exchange * r_lo * row_bytes],
                         ['recv', rank + 1, exchange * r_hi * row_bytes]]
        assert group == [m for m in expected if m[2] > 0], (app, rank)
        for peer in {m[1] for m in group}:
          assert sum(m[0] == 'send' and m[1] == peer for m in group) in (0, n)
          assert sum(m[0] == 'recv' and m[1] == peer for m in group) in (0, n)
