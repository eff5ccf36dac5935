#!/usr/bin/env python3
"""Long 1-D windows (lowpass1d, dfir1d, skewfir1d, acoustic1d on 2^27 cells, `--iterate`
iterations): the far-tap fused kernels (kernel.generate's `far_taps`; kernel_stream1d /
kernel_fields1d with chained wave shifts) against the per-stage schedule, on one GPU, both
from the code object __graft_entry__.build() makes with the switch (<app>.taps.hsaco), in one
process, alternating - the protocol of tools/far2d/far2d_bench.py.

limit N   = what a `--hip-far-taps` product runs: the blob's schedule under the depth limit
            its generated entry points set (switches.depth_limit_of): the launcher admits
            fused 1-D kernels only under a limit;
depth d   = the same sweep with its split fixed to launches of <app>_fused_k<d> only
            (soda_hip_plan_set_split), for every fused depth of the table;
per-stage = the same blob under set_max_depth(-1): one launch per stage and iteration, one
            cell per work-item, every tap a global load - what these programs run without
            the switch.

`--cols C` adds the same fused depths with C cells per lane instead of the default 16-byte
lanes (8 floats or 4 doubles: 32-byte lanes, half the hops and half the halo share), as rows
`depth d cC`, from a second code object generated with `cols=C`: `--blob-dir`/<app>.taps.c<C>
.hsaco, built there with hipcc when missing.  Name the apps the width applies to.

First every schedule runs once and its outputs are compared with the per-stage outputs bit
for bit on every output's box, at the size timed: nothing is timed unless they are identical.
A round times `--repeats` back-to-back sweeps of one schedule between device events and takes
their mean; the rounds of the schedules alternate, the first `--warmup` rounds are dropped,
and the median, the fastest and the slowest of the `--sweeps` timed rounds are reported, per
sweep, per launch and per iteration.  A schedule is FASTER than per-stage if its median is
below the per-stage median by more than the spread (the larger max - min of the two).

Registers and spills come from the code object's metadata, code sizes from its symbol table.

    python tools/far1d/far1d_bench.py [--apps APP ...] [--cols C] [--blob-dir DIR] [--cells N]
                                      [--iterate N] [--sweeps K] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tools'),
          os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=None,
                  help='default: lowpass1d dfir1d skewfir1d acoustic1d (far_taps)')
  ap.add_argument('--cols', type=int, default=None,
                  help='also time the fused depths with this many cells per lane')
  ap.add_argument('--blob-dir', default=None,
                  help='where the code objects of --cols are kept (default: a temporary one)')
  ap.add_argument('--cells', type=int, default=1 << 27, help='cells of the array')
  ap.add_argument('--iterate', type=int, default=24,
                  help='iterations per sweep: a multiple of every fused depth')
  ap.add_argument('--sweeps', type=int, default=7, help='timed rounds per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=2, help='untimed rounds per schedule')
  ap.add_argument('--repeats', type=int, default=3, help='sweeps per round')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.sweeps >= 3
  import numpy as np
  import __graft_entry__ as entry
  from soda_hip import frontend
  from soda_hip.codegen import kernel, switches, spec as specmod
  from soda_hip.runtime import host
  from codegen_util import code_bytes, static_figures  # tests/: a code object's notes
  apps = args.apps or list(entry.FAR_TAPS_APPS)
  iterate = args.iterate
  dims = (args.cells,)
  blob_dir = args.blob_dir or tempfile.mkdtemp()
  lines = [
      'Far-tap fused 1-D kernels (kernel.generate: far_taps) against the per-stage schedule of',
      'the same code object.  tools/far1d/far1d_bench.py: outputs of every schedule compared bit for',
      'bit with the per-stage outputs first; then rounds of %d back-to-back sweeps between device'
      % args.repeats,
      'events, the schedules alternating, %d untimed rounds, then the median (min .. max) of %d'
      % (args.warmup, args.sweeps),
      'timed rounds.  A sweep = %d iterations.  FASTER: the medians differ by more than the spread'
      % iterate,
      '(the larger max - min of the two series).  Register figures: code-object metadata (hipcc,',
      'gfx950).', '']
  for app in apps:
    spec = specmod.spec_from_stencil(frontend.load(entry.sample_path(app)))
    limit, _ = switches.depth_limit_of(spec, dict(far_taps=True))
    assert limit > 0, app
    default = 'limit %d' % limit
    # (label suffix, code object, table): the shipped blob, and the one of --cols
    variants = [('', entry.blob_path(app, far_taps=True), kernel.generate(spec, far_taps=True)[1])]
    if args.cols:
      text, table = kernel.generate(spec, far_taps=True, cols=args.cols)
      path = os.path.join(blob_dir, '%s.taps.c%d.hsaco' % (app, args.cols))
      if not os.path.exists(path):
        os.makedirs(blob_dir, exist_ok=True)
        kernel.compile_to_code_object(text, path)
      variants.append((' c%d' % args.cols, path, table))
    progs = []
    for _, blob, table in variants:
      prog = host.open_program(blob=blob, spec=spec)
      assert prog.kernels == table, blob
      assert all(iterate % k['depth'] == 0 for k in table if k['kind'] == 'fused'), (app, iterate)
      progs.append(prog)
    stage_names = [e['name'] for e in variants[0][2] if e['kind'] == 'stage']
    rng = np.random.default_rng(7)
    din = [host.DeviceArray(args.cells * dt.itemsize) for dt in progs[0].in_dtypes]
    dout = [host.DeviceArray(args.cells * dt.itemsize) for dt in progs[0].out_dtypes]
    for d, dt in zip(din, progs[0].in_dtypes):
      a = rng.random(dims, dtype=np.float32)
      d.upload(a.astype(dt))
      del a
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    # (name, program, depth limit, fixed split, the entry every launch is held to)
    schedules = [(default, progs[0], limit, None, None)]
    for (suffix, _, table), prog in zip(variants, progs):
      schedules += [('depth %d%s' % (k['depth'], suffix), prog, limit,
                     [k['depth']] * (iterate // k['depth']), k)
                    for k in table if k['kind'] == 'fused']
    schedules.append(('per-stage', progs[0], -1, None, None))
    launches = {}

    def run(name, prog, depth_limit, split, repeats):
      prog.set_max_depth(depth_limit)
      if split:
        prog.set_split(dims, iterate, split)
      try:
        launches[name] = [e['name'] for e, _ in prog.schedule(dims, iterate)]
        return prog.sweep_timed(pin, pout, dims, iterate, warmup=0, repeats=repeats)
      finally:
        if split:
          prog.set_split(dims, iterate, [])
        prog.set_max_depth(0)

    # every schedule's results at this size, bit for bit on every output's box, first
    boxes = []
    for name in spec['outputs']:
      lo, hi = specmod.iteration_boxes(spec, iterate)[-1][name]
      boxes.append(slice(-lo[0], dims[0] - hi[0]))
    reference, same = None, {}
    for name, prog, depth_limit, split, _ in reversed(schedules):
      for d in dout:
        d.zero()
      run(name, prog, depth_limit, split, 1)
      got = [np.ascontiguousarray(d.download(dims, dt)[sl])
             for d, dt, sl in zip(dout, prog.out_dtypes, boxes)]
      if reference is None:
        reference = got
      same[name] = all(np.array_equal(g.view(np.uint8), r.view(np.uint8))
                       for g, r in zip(got, reference))
      del got
    del reference
    assert launches['per-stage'] == stage_names * iterate, launches['per-stage'][:8]
    assert all(n.startswith(app + '_fused_k') for n in launches[default]), launches[default]
    for name, _, _, split, k in schedules:
      if k is not None:
        assert launches[name] == [k['name']] * len(split), (name, launches[name][:8])
    assert all(same.values()), '%s: outputs differ from the per-stage outputs: %s' % (app, same)
    times = {s[0]: [] for s in schedules}
    for r in range(args.warmup + args.sweeps):     # alternating: drift hits all alike
      for name, prog, depth_limit, split, _ in schedules:
        t = run(name, prog, depth_limit, split, args.repeats)
        if r >= args.warmup:
          times[name].append(t['kernel_us'] / 1e3)
    updates = specmod.valid_cells(spec, dims, iterate)
    alg = specmod.algorithmic_bytes_per_update(spec)
    med = {n: statistics.median(ts) for n, ts in times.items()}
    lines.append('%s %d cells x %d, %d timed rounds of %d sweeps each; outputs of all schedules '
                 'bit-identical on every box' % (app, dims[0], iterate, args.sweeps, args.repeats))
    lines.append('  schedule     ms per sweep: median  min .. max      launches  us per launch  '
                 'us per iteration  Gcell/s  TB/s alg.  against per-stage')
    record = dict(app=app, dims=list(dims), iterate=iterate, ms=med, schedules={})
    for name, _, _, _, _ in schedules:
      ts = sorted(times[name])
      spread = max(ts[-1] - ts[0], max(times['per-stage']) - min(times['per-stage']))
      verdict = '' if name == 'per-stage' else (
          'FASTER' if med['per-stage'] - med[name] > spread else
          'SLOWER' if med[name] - med['per-stage'] > spread else 'NO DIFFERENCE beyond the spread')
      n = len(launches[name])
      lines.append('  %-10s %12.3f  %10.3f .. %-10.3f %6d  %13.1f  %16.1f  %7.1f  %9.2f  %s' % (
          name, med[name], ts[0], ts[-1], n, med[name] * 1e3 / n, med[name] * 1e3 / iterate,
          updates / (med[name] * 1e-3) / 1e9, alg * updates / (med[name] * 1e-3) / 1e12,
          '' if name == 'per-stage' else '%.2f x, %s (spread %.3f ms)' % (
              med['per-stage'] / med[name], verdict, spread)))
      record['schedules'][name] = dict(ms=med[name], min_ms=ts[0], max_ms=ts[-1], launches=n,
                                       speedup=med['per-stage'] / med[name], verdict=verdict)
    lines.append('  %s schedule: %s' % (default, ' '.join(
        '%d x %s' % (launches[default].count(n), n) for n in sorted(set(launches[default])))))
    for suffix, blob, table in variants:
      for k in table:
        if k['kind'] != 'fused':
          continue
        f = static_figures(blob, k['name'])
        lines.append('  %-22s %d cells per lane, halo %d/%d, %3d of %3d cells out; %s' % (
            k['name'] + suffix, k['cols'], k['halo'][0], k['halo'][1], k['w_out'], 64 * k['cols'],
            '%d VGPRs (estimate %d), %d SGPRs, scratch %d B, spills %d VGPR / %d SGPR, code %d B'
            % (f['vgpr_count'], k['est_vgprs'], f['sgpr_count'], f['private_segment_fixed_size'],
               f['vgpr_spill_count'], f['sgpr_spill_count'], code_bytes(blob, k['name']))
            if f else '(no code object here)'))
    lines.append('')
    for d in din + dout:
      d.free()
    for prog in progs:
      prog.close()
    print(json.dumps(record), flush=True)
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
