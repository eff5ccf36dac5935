#!/usr/bin/env python3
"""One-pass programs with several outputs (grad2d, blend2d at 16384 x 16384; grad3d, mix3d
at 512 x 512 x 512), the fused depth-1 kernel over all outputs (kernel.generate's
`fuse_outputs`, kernel_fields2d / kernel_fields3d) against the per-stage schedule, on one
GPU, both from the code object __graft_entry__.build() makes with the switch
(<app>.fused.hsaco), in one process, alternating.

fused     = soda_hip_plan_set_max_depth(plan, 1): one launch, every input read once (plus
            the halo), every output written once;
per-stage = the default schedule of such a program (set_max_depth(-1) forces it): one
            launch per stage, every operand from HBM, every local through HBM.

A round times `--repeats` back-to-back sweeps of one schedule between device events and
takes their mean; the rounds of the two schedules alternate, the first `--warmup` rounds
are dropped, and the median, the fastest and the slowest of the `--sweeps` timed rounds
are reported.  The fused kernel is FASTER if its median is below the per-stage median by
more than the spread (the larger max - min of the two).  After the timing both schedules'
outputs are compared bit for bit on every output's own box, at the size timed.

These programs are not iterated, so traffic is stated per cell: algorithmic bytes
(N_in + N_out) x sizeof(T), the per-stage schedule's (every stage reads each tensor it
names once and writes its result) and the fused kernel's with its halo (derived from the
table, not measured); the rates are algorithmic bytes x valid cells over the measured time.
Registers and scratch come from the code object's metadata.  `--static` prints the derived
and the compiler's figures and times nothing (no GPU needed).

    python tools/rect_bench.py [--apps APP ...] [--size2d W H] [--size3d W H D]
                               [--sweeps K] [--repeats R] [--static] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tools')):
  if p not in sys.path:
    sys.path.insert(0, p)


def traffic(spec, k):
  """(algorithmic, per-stage, fused with halo) bytes per cell; derived from the program
  and the table entry."""
  from soda_hip.codegen import spec as specmod
  lowered = specmod.inline_pointwise(spec)
  types = specmod.tensor_c_types(lowered)
  alg = specmod.algorithmic_bytes_per_update(spec)
  staged = sum(specmod.ELEM_SIZE[types[t]] for stage in lowered['stages']
               for t in sorted({name for name, _ in stage['loads']}) + [stage['name']])
  kept = k['w_out'] / (64.0 * k['cols'])
  if 'rows' in k:
    kept *= k['r_out'] / float(k['rows'])
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  fused = (len(spec['inputs']) / kept + len(spec['outputs'])) * elem
  return alg, staged, fused, kept


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=None, help='default: grad2d blend2d grad3d mix3d')
  ap.add_argument('--size2d', nargs=2, type=int, default=[16384, 16384])
  ap.add_argument('--size3d', nargs=3, type=int, default=[512, 512, 512])
  ap.add_argument('--sweeps', type=int, default=7, help='timed rounds per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=2, help='untimed rounds per schedule')
  ap.add_argument('--repeats', type=int, default=40, help='sweeps per round')
  ap.add_argument('--static', action='store_true',
                  help='the static figures only (registers, derived traffic): no GPU')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.sweeps >= 3
  import __graft_entry__ as entry
  import fields_bench
  from soda_hip import frontend
  from soda_hip.codegen import kernel, spec as specmod
  apps = args.apps or list(entry.RECT_APPS)
  lines = [
      'Fused one-pass kernels over several outputs (kernel.generate: fuse_outputs) against the',
      'per-stage schedule.  tools/rect_bench.py: rounds of %d back-to-back sweeps between device'
      % args.repeats,
      'events, the two schedules alternating, %d untimed rounds, then the median (min .. max) of'
      % args.warmup,
      '%d timed rounds, per sweep.  FASTER: the medians differ by more than the spread (the larger'
      % args.sweeps,
      'max - min).  Bytes per cell are derived, rates are algorithmic bytes x valid cells over the',
      'measured time.  Register figures: code-object metadata (hipcc, gfx950).',
      'Scope not met: 3-D tiles take at most %d rows x inputs (kernel.RECT3D_INPUT_ROWS, fitted to'
      % kernel.RECT3D_INPUT_ROWS,
      'grad3d and mix3d) and the smallest tile has 8 rows, so a 3-D program with more than FOUR',
      'inputs keeps its per-stage kernels; 2-D programs take any number of inputs.', '']
  for app in apps:
    spec = specmod.spec_from_stencil(frontend.load(entry.sample_path(app)))
    dim = spec['dim']
    dims = tuple(args.size2d if dim == 2 else args.size3d)
    shape = tuple(reversed(dims))
    blob = entry.blob_path(app, fuse_outputs=True)
    table = kernel.generate(spec, fuse_outputs=True)[1]
    k = table[-1]
    assert k['kind'] == 'fused' and k['depth'] == 1, k
    alg, staged, fused_bytes, kept = traffic(spec, k)
    static = [
        '  bytes per cell: algorithmic %d, per-stage %d (%d launches), fused %.2f with its halo '
        '(%.3f of a %s kept)' % (alg, staged, len(table) - 1, fused_bytes, kept,
                                 'tile' if 'rows' in k else 'strip')]
    figures = fields_bench.isa_figures(blob, {k['name']: 1}) if os.path.exists(blob) else {}
    static += fields_bench.isa_lines(figures, {k['name']: 1})
    if args.static:
      lines.append('%s: NOT MEASURED (static figures only)' % app)
      lines += static
      continue
    import numpy as np
    from soda_hip.runtime import host
    prog = host.open_program(blob=blob, spec=spec)
    assert prog.kernels[-1]['name'] == k['name']
    rng = np.random.default_rng(7)
    cells = int(np.prod(shape))
    din = [host.DeviceArray(cells * dt.itemsize) for dt in prog.in_dtypes]
    dout = [host.DeviceArray(cells * dt.itemsize) for dt in prog.out_dtypes]
    for d, dt in zip(din, prog.in_dtypes):
      a = rng.random(shape, dtype=np.float32)
      d.upload(a.astype(dt) if dt.kind == 'f' else (a * 1000).astype(dt))
      del a
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    schedules = [('fused', 1), ('per-stage', -1)]
    times = {name: [] for name, _ in schedules}
    launches = {}

    def run(name, limit, repeats):
      prog.set_max_depth(limit)
      try:
        launches[name] = [e['name'] for e, _ in prog.schedule(dims, 1)]
        return prog.sweep_timed(pin, pout, dims, 1, warmup=0, repeats=repeats)
      finally:
        prog.set_max_depth(0)

    for r in range(args.warmup + args.sweeps):     # alternating: drift hits both alike
      for name, limit in schedules:
        t = run(name, limit, args.repeats)
        if r >= args.warmup:
          times[name].append(t['kernel_us'] / 1e3)
    assert launches['fused'] == [k['name']], launches
    assert len(launches['per-stage']) == len(table) - 1, launches
    # both schedules' results at this size, bit for bit on every output's own box
    results = {}
    for name, limit in schedules:
      for d in dout:
        d.zero()
      run(name, limit, 1)
      results[name] = [d.download(shape, dt) for d, dt in zip(dout, prog.out_dtypes)]
    boxes = specmod.iteration_boxes(spec, 1)[-1]
    valid = 0
    same = True
    for j, o in enumerate(spec['outputs']):
      lo, hi = boxes[o]
      sl = tuple(slice(-lo[d], dims[d] - hi[d]) for d in reversed(range(dim)))
      a, b = results['fused'][j][sl], results['per-stage'][j][sl]
      valid = max(valid, a.size)
      same = same and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                     np.ascontiguousarray(b).view(np.uint8))
    del results
    for d in din + dout:
      d.free()
    prog.close()
    med = {n: statistics.median(ts) for n, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    verdict = 'FASTER' if med['per-stage'] - med['fused'] > spread else \
        'SLOWER' if med['fused'] - med['per-stage'] > spread else 'NO DIFFERENCE beyond the spread'
    lines.append('%s %s, %d timed rounds of %d sweeps each (ms per sweep: median, min .. max)'
                 % (app, ' x '.join(map(str, dims)), args.sweeps, args.repeats))
    for name, _ in schedules:
      ts = sorted(times[name])
      lines.append('  %-10s %8.3f  %8.3f .. %-8.3f  %6.2f TB/s algorithmic  [%d launch(es)]' % (
          name, med[name], ts[0], ts[-1], alg * valid / (med[name] * 1e-3) / 1e12,
          len(launches[name])))
    lines.append('  fused is %s: %.2f x per-stage (spread %.3f ms); outputs %s on every box'
                 % (verdict, med['per-stage'] / med['fused'], spread,
                    'bit-identical' if same else 'DIFFER'))
    lines += static
    print(json.dumps(dict(app=app, dims=list(dims), ms=med, spread_ms=spread, verdict=verdict,
                          speedup=med['per-stage'] / med['fused'], identical=bool(same),
                          bytes_per_cell=dict(algorithmic=alg, per_stage=staged,
                                              fused=fused_bytes), isa=figures)), flush=True)
    assert same, '%s: fused and per-stage outputs differ' % app
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
