#!/usr/bin/env python3
"""The packed-cell fused 3-D kernels (kernel.generate's `packed_cells`; kernel_stream3d_pk)
against the per-stage schedule, on one GPU, both from the code object
__graft_entry__.build() makes with the switch (<app>.pk.hsaco), in one process, alternating -
the protocol of tools/lds3d/lds3d_bench.py and tools/far/far_bench.py, whose judge() decides.

For each sample (smooth3d, skewvol3d, sdiff3d, castvol3d: 8- and 16-bit integer volumes) and
each of `--sizes` (default 512 and 256: cubes of that edge):

default   = what a product of `--hip-packed-cells` runs: the blob's default schedule;
depth d   = the same sweep with its split fixed to launches of <app>_fused_k<d> only
            (soda_hip_plan_set_split), for every fused depth of the table;
per-stage = the same blob under set_max_depth(-1): one launch per stage and iteration, one
            cell per work-item, 1- or 2-byte accesses - what these programs run without the
            switch.

First every schedule runs once and its outputs are compared with the per-stage outputs bit
for bit on the output's box, at the size timed: nothing is timed unless they are identical.
Inputs are seeded random integers over the whole range of the element type.  A round times
`--repeats` back-to-back sweeps of one schedule between device events and takes their mean;
the rounds of the schedules alternate, the first `--warmup` rounds are dropped, and the
median, the fastest and the slowest of the `--sweeps` timed rounds are reported.  A schedule
is FASTER than per-stage if its median is below the per-stage median by more than the spread
(the larger max - min of the two).  A depth that is not FASTER leaves
kernel.PACKED3D_DEPTHS; its figure stays in the profile.

Registers and spills come from the code object's metadata, code sizes from its symbol table.

    python tools/packed3d/packed3d_bench.py [--apps APP ...] [--sizes N ...] [--iterate N]
                                            [--sweeps K] [--warmup W] [--repeats R]
                                            [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tools'),
          os.path.join(ROOT, 'tools', 'far'), os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

from far_bench import BASELINE, judge      # noqa: E402 - the rule of every FASTER

ON = dict(packed_cells=True)
DEFAULT = 'default'


def parse_args(argv=None):
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=None,
                  help='default: smooth3d skewvol3d sdiff3d castvol3d')
  ap.add_argument('--sizes', nargs='+', type=int, default=[512, 256],
                  help='edges of the cubes timed')
  ap.add_argument('--iterate', type=int, default=4,
                  help='iterations per sweep: a multiple of every fused depth')
  ap.add_argument('--sweeps', type=int, default=7, help='timed rounds per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=2, help='untimed rounds per schedule')
  ap.add_argument('--repeats', type=int, default=3, help='sweeps per round')
  ap.add_argument('--out', default=None)
  args = ap.parse_args(argv)
  if args.sweeps < 3:
    ap.error('--sweeps: at least 3 timed rounds make a spread')
  return args


def schedules_of(table, iterate):
  """The schedules timed for a kernel table, in the report's order: [(name, depth limit, fixed
  split or None, the entry every launch is held to or None)] - the default schedule, one row
  per fused depth with the split that fixes it, and LAST the per-stage schedule of the same
  blob (depth limit -1), which every other row is paired with."""
  fused = [k for k in table if k['kind'] == 'fused']
  if not fused:
    raise ValueError('no fused kernel in the table: was the blob generated with packed_cells?')
  for k in fused:
    if iterate % k['depth']:
      raise ValueError('--iterate %d is no multiple of depth %d' % (iterate, k['depth']))
  rows = [(DEFAULT, 0, None, None)]
  rows += [('depth %d' % k['depth'], 0, [k['depth']] * (iterate // k['depth']), k)
           for k in fused]
  rows.append((BASELINE, -1, None, None))
  return rows


def report_lines(app, dims, iterate, rows, launches, updates, bytes_per_update):
  """The report of one program at one size: a header and one line per schedule of judge()'s
  `rows`, {schedule: figures}; launches: {schedule: [kernel names]}."""
  out = ['%s %s x %d; outputs of all schedules bit-identical on the box' % (
      app, ' x '.join(map(str, dims)), iterate),
         '  schedule     ms per sweep: median  min .. max      launches  us per launch  '
         'us per iteration  Gcell/s  TB/s alg.  against per-stage']
  for name, row in rows.items():
    ms, n = row['ms'], len(launches[name])
    out.append('  %-10s %12.3f  %10.3f .. %-10.3f %6d  %13.1f  %16.1f  %7.1f  %9.2f  %s' % (
        name, ms, row['min_ms'], row['max_ms'], n, ms * 1e3 / n, ms * 1e3 / iterate,
        updates / (ms * 1e-3) / 1e9, bytes_per_update * updates / (ms * 1e-3) / 1e12,
        '' if name == BASELINE else '%.2f x, %s (spread %.3f ms)' % (
            row['speedup'], row['verdict'], row['spread'])))
  return out


def main(argv=None):
  args = parse_args(argv)
  import numpy as np
  import __graft_entry__ as entry
  from soda_hip import frontend
  from soda_hip.codegen import kernel, spec as specmod
  from soda_hip.runtime import host
  from codegen_util import code_bytes, static_figures  # tests/: a code object's notes
  apps = args.apps or list(entry.PACKED_CELLS_APPS)
  iterate = args.iterate
  lines = [
      'Packed-cell fused 3-D kernels (kernel.generate: packed_cells) against the per-stage',
      'schedule of the same code object.  tools/packed3d/packed3d_bench.py: outputs of every',
      'schedule compared bit for bit with the per-stage outputs first; then rounds of %d'
      % args.repeats,
      'back-to-back sweeps between device events, the schedules alternating, %d untimed rounds,'
      % args.warmup,
      'then the median (min .. max) of %d timed rounds.  A sweep = %d iterations.  FASTER: the'
      % (args.sweeps, iterate),
      'medians differ by more than the spread (the larger max - min of the two series).',
      'Register figures: code-object metadata (hipcc, gfx950).', '']
  for app in apps:
    spec = specmod.spec_from_stencil(frontend.load(entry.sample_path(app)))
    blob = entry.blob_path(app, **ON)
    table = kernel.generate(spec, **ON)[1]
    schedules = schedules_of(table, iterate)
    prog = host.open_program(blob=blob, spec=spec)
    assert prog.kernels == table, blob
    stage_names = [e['name'] for e in table if e['kind'] == 'stage']
    for edge in args.sizes:
      dims = (edge, edge, edge)
      shape = tuple(reversed(dims))
      rng = np.random.default_rng(7)
      n_cells = int(np.prod(shape))
      din = [host.DeviceArray(n_cells * dt.itemsize) for dt in prog.in_dtypes]
      dout = [host.DeviceArray(n_cells * dt.itemsize) for dt in prog.out_dtypes]
      for d, dt in zip(din, prog.in_dtypes):
        info = np.iinfo(dt)
        d.upload(rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True))
      pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
      launches = {}

      def run(name, depth_limit, split, repeats):
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

      lo, hi = specmod.iteration_boxes(spec, iterate)[-1][spec['outputs'][0]]
      box = tuple(slice(-lo[d], dims[d] - hi[d]) for d in reversed(range(3)))
      reference, same = None, {}
      for name, depth_limit, split, _ in reversed(schedules):      # per-stage first
        for d in dout:
          d.zero()
        run(name, depth_limit, split, 1)
        got = np.ascontiguousarray(dout[0].download(shape, prog.out_dtypes[0])[box])
        if reference is None:
          reference = got
        same[name] = np.array_equal(got.view(np.uint8), reference.view(np.uint8))
        del got
      del reference
      assert launches[BASELINE] == stage_names * iterate, launches[BASELINE][:8]
      assert all(n.startswith(app + '_fused_k') for n in launches[DEFAULT]), launches[DEFAULT]
      for name, _, split, k in schedules:
        if k is not None:
          assert launches[name] == [k['name']] * len(split), (name, launches[name][:8])
      assert all(same.values()), '%s: outputs differ from the per-stage outputs: %s' % (app, same)
      times = {s[0]: [] for s in schedules}
      for r in range(args.warmup + args.sweeps):     # alternating: drift hits all alike
        for name, depth_limit, split, _ in schedules:
          t = run(name, depth_limit, split, args.repeats)
          if r >= args.warmup:
            times[name].append(t['kernel_us'] / 1e3)
      rows = judge(times)
      lines += report_lines(app, dims, iterate, rows, launches,
                            specmod.valid_cells(spec, dims, iterate),
                            specmod.algorithmic_bytes_per_update(spec))
      lines.append('  %s schedule: %s' % (DEFAULT, ' '.join(
          '%d x %s' % (launches[DEFAULT].count(n), n) for n in sorted(set(launches[DEFAULT])))))
      lines.append('')
      print(json.dumps(dict(app=app, dims=list(dims), iterate=iterate,
                            schedules={n: dict(ms=r['ms'], min_ms=r['min_ms'],
                                               max_ms=r['max_ms'], speedup=r['speedup'],
                                               verdict=r['verdict'])
                                       for n, r in rows.items()})), flush=True)
      for d in din + dout:
        d.free()
    for k in table:
      if k['kind'] != 'fused':
        continue
      f = static_figures(blob, k['name'])
      lines.append('  %-22s tile %d x %d per wavefront, %d x %d out, period %d; %s' % (
          k['name'], 64 * k['cols'], k['rows'], k['w_out'], k['r_out'], k['period'],
          '%d VGPRs (estimate %d), %d SGPRs, scratch %d B, spills %d VGPR / %d SGPR, code %d B'
          % (f['vgpr_count'], k['est_vgprs'], f['sgpr_count'], f['private_segment_fixed_size'],
             f['vgpr_spill_count'], f['sgpr_spill_count'], code_bytes(blob, k['name']))
          if f else '(no code object here)'))
    lines.append('')
    prog.close()
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
