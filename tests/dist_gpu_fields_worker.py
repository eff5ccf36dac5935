"""Worker of tests/test_gpu_fields_slabs.py: one rank of a gloo group; the ranks share
the ONE GPU and run the REAL kernels of a program over several fields through
soda_hip.runtime.dist (HipEngine and run_slab with one array per field, per-field
margins).  Ghost rows travel through the host (gloo) because RCCL refuses two ranks on one
device; everything else is the production path."""
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
from soda_hip.runtime import dist as sdist, host   # noqa: E402


def main():
  app, inputs_path, iterate, exchange, max_depth, out_dir = sys.argv[1:7]
  iterate, exchange, max_depth = int(iterate), int(exchange), int(max_depth)
  rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
  dist.init_process_group(backend='gloo')
  torch.cuda.set_device(0)
  sample = os.path.join(ROOT, 'tests', 'samples', app + '.soda')
  if not os.path.exists(sample):
    sample = os.path.join(ROOT, 'tests', 'samples', 'extra', app + '.soda')
  spec = specmod.spec_from_stencil(frontend.load(sample))
  prog = host.open_program(
      blob=os.path.join(ROOT, 'soda-compiler_amd', 'blobs', app + '.hsaco'), spec=spec)
  prog.set_max_depth(max_depth)
  data = np.load(inputs_path)
  full = [data['in_' + t['name']] for t in spec['inputs']]
  dims = list(reversed(full[0].shape))
  r_lo, r_hi = spec['radius']['lo'][-1], spec['radius']['hi'][-1]
  plan = sdist.SlabPlan(dims, rank, world, r_lo, r_hi, exchange)
  dev = torch.device('cuda', 0)
  shape = tuple(reversed(plan.local_dims))
  levels = [[torch.full(shape, float('nan'), dtype=torch.float32, device=dev) for _ in full]
            for _ in range(3)]
  for j, f in enumerate(full):
    levels[0][j][plan.ghost_lo:plan.ghost_lo + plan.own] = torch.from_numpy(
        f[plan.start:plan.stop]).to(dev)
  # the library's own per-field margins, level by level: what a caller without the spec has
  table = [prog.field_margins(k) for k in range(1, iterate + 1)]
  assert table == specmod.iteration_field_margins(spec, iterate)
  order = sdist.TimedSerialSchedule(torch, host_sync=True)
  result, exchanges = sdist.run_slab(sdist.HipEngine(prog, torch), plan, levels, iterate,
                                     sdist.fields_margins_of(table), dist, schedule=order)
  torch.cuda.synchronize()
  np.savez(os.path.join(out_dir, 'rank%d.npz' % rank),
           **{'out%d' % j: r[plan.ghost_lo:plan.ghost_lo + plan.own].cpu().numpy()
              for j, r in enumerate(result)})
  with open(os.path.join(out_dir, 'rank%d.json' % rank), 'w') as f:
    json.dump(dict(start=plan.start, stop=plan.stop, exchange=plan.exchange,
                   exchanges=exchanges), f)
  dist.barrier()
  prog.close()
  dist.destroy_process_group()


if __name__ == '__main__':
  main()
