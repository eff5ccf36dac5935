"""Worker of tests/test_dist_fields.py: one rank of a gloo process group running the
static-cut slab driver of soda_hip.runtime.dist on programs over SEVERAL fields, with a
CPU engine built on the oracle.  One group runs every case of a JSON list (program, size,
iterations, exchange period), so that the suite starts a few processes and not hundreds."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

from soda_hip import frontend                      # noqa: E402
from soda_hip.codegen import spec as specmod       # noqa: E402
from soda_hip.runtime import dist as sdist         # noqa: E402
from oracle import soda_oracle                     # noqa: E402


def resumed_boxes(spec, iterations, valid_lo, valid_hi):
  """spec.iteration_boxes with input j starting on the box (-valid_lo[j], valid_hi[j])
  instead of the zero box: what soda_hip_sweep_fields defines its outputs on."""
  windows = specmod.stage_windows(spec)
  ins = [t['name'] for t in spec['inputs']]
  feed = {n: ([-v for v in lo], list(hi)) for n, lo, hi in zip(ins, valid_lo, valid_hi)}
  result = []
  for _ in range(iterations):
    boxes = dict(feed)
    for stage in spec['stages']:
      lo = hi = None
      for parent, (wlo, whi) in windows[stage['name']].items():
        plo, phi = boxes[parent]
        clo = [a + b for a, b in zip(plo, wlo)]
        chi = [a + b for a, b in zip(phi, whi)]
        lo = clo if lo is None else [min(a, b) for a, b in zip(lo, clo)]
        hi = chi if hi is None else [max(a, b) for a, b in zip(hi, chi)]
      boxes[stage['name']] = ([min(0, v) for v in lo], [max(0, v) for v in hi])
    result.append({s['name']: boxes[s['name']] for s in spec['stages']})
    feed = {i: boxes[o] for i, o in zip(ins, spec['outputs'])}
  return result


class FieldsOracleEngine:
  """sweep() with the contract of soda_hip_sweep_fields: src and dst hold one array per
  field, valid_lo / valid_hi one margin per field; output j is written on its own box
  only (everything else of dst keeps its poison)."""

  def __init__(self, spec):
    self.spec = spec
    self.oracle = soda_oracle.Oracle(spec)
    self.regions = []       # (valid_lo, valid_hi) of every sweep, for the worker's checks

  def sweep(self, src, dst, local_dims, iterations, valid_lo, valid_hi, rows=None,
            final_only=False):
    spec = self.spec
    assert rows is None and not final_only       # serial order only
    ins = [t['name'] for t in spec['inputs']]
    outs = spec['outputs']
    assert len(src) == len(dst) == len(valid_lo) == len(valid_hi) == len(ins)
    self.regions.append(([list(v) for v in valid_lo], [list(v) for v in valid_hi]))
    boxes = resumed_boxes(spec, iterations, valid_lo, valid_hi)
    cur = [t.numpy() for t in src]
    for k in range(iterations):
      arrays = {s['name']: np.zeros_like(cur[0], dtype=self.oracle.dtype(s['name']))
                for s in spec['stages']}
      arrays.update(dict(zip(ins, cur)))
      self.oracle._call(arrays, tuple(local_dims), boxes[k])
      cur = [arrays[o] for o in outs]
    for j, o in enumerate(outs):
      lo, hi = boxes[iterations - 1][o]
      box = tuple(slice(-l, n - h) for l, h, n in reversed(list(zip(lo, hi, local_dims))))
      dst[j][box] = torch.from_numpy(cur[j])[box]


class CountingDist:
  """torch.distributed with every batch of point-to-point operations counted."""

  def __init__(self):
    self.groups = []        # per batch: [(kind, peer, bytes)]
    self.P2POp, self.isend, self.irecv = dist.P2POp, dist.isend, dist.irecv

  def batch_isend_irecv(self, ops):
    self.groups.append([('send' if op.op is dist.isend else 'recv', op.peer,
                         op.tensor.numel() * op.tensor.element_size()) for op in ops])
    return dist.batch_isend_irecv(ops)


def main():
  cases_path, out_dir = sys.argv[1:3]
  rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
  dist.init_process_group(backend='gloo')
  specs, engines = {}, {}
  for index, (app, dims, iterate, exchange) in enumerate(json.load(open(cases_path))):
    if app not in specs:
      sample = os.path.join(ROOT, 'tests', 'samples', app + '.soda')
      if not os.path.exists(sample):
        sample = os.path.join(ROOT, 'tests', 'samples', 'extra', app + '.soda')
      specs[app] = specmod.spec_from_stencil(frontend.load(sample))
      engines[app] = FieldsOracleEngine(specs[app])
    spec, engine = specs[app], engines[app]
    n = len(spec['inputs'])
    # the reach: the hull over the fields of one iteration's margins
    r_lo, r_hi = spec['radius']['lo'][-1], spec['radius']['hi'][-1]
    plan = sdist.SlabPlan(dims, rank, world, r_lo, r_hi, exchange)
    assert plan.exchange == exchange       # the test picked an admissible pair
    rng = np.random.default_rng(99)
    full = [rng.random(tuple(reversed(dims)), dtype=np.float32) for _ in range(n)]
    shape = tuple(reversed(plan.local_dims))
    # rows nobody filled are NaN: a sweep that read one into a compared cell would show
    levels = [[torch.full(shape, float('nan')) for _ in range(n)] for _ in range(3)]
    for j in range(n):
      levels[0][j][plan.ghost_lo:plan.ghost_lo + plan.own] = torch.from_numpy(
          full[j][plan.start:plan.stop])
    table = specmod.iteration_field_margins(spec, iterate)
    counting = CountingDist()
    engine.regions = []
    result, exchanges = sdist.run_slab(engine, plan, levels, iterate,
                                       sdist.fields_margins_of(table), counting)
    # every sweep was told every field's own region: 0 towards a neighbour, the field's
    # own margin after the iterations done so far on every global side of every dimension
    done = 0
    for lo, hi in engine.regions:
      want = sdist.fields_margins_of(table)(done)
      for j in range(n):
        wlo, whi = list(want[j][0]), list(want[j][1])
        if plan.has_lo:
          wlo[-1] = 0
        if plan.has_hi:
          whi[-1] = 0
        assert lo[j] == wlo and hi[j] == whi, (app, done, j, lo[j], hi[j], wlo, whi)
      done += min(exchange, iterate - done)
    assert done == iterate
    np.savez(os.path.join(out_dir, 'case%d.rank%d.npz' % (index, rank)),
             **{'out%d' % j: result[j][plan.ghost_lo:plan.ghost_lo + plan.own].numpy()
                for j in range(n)})
    with open(os.path.join(out_dir, 'case%d.rank%d.json' % (index, rank)), 'w') as f:
      json.dump(dict(start=plan.start, stop=plan.stop, exchanges=exchanges,
                     groups=counting.groups), f)
  dist.barrier()
  dist.destroy_process_group()


if __name__ == '__main__':
  main()
