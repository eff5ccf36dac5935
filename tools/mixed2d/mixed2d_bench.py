#!/usr/bin/env python3
"""The mixed-width fused 2-D kernels (kernel.generate: mixed_widths; kernel_stream2d with every
tensor's loads and stores in its own width) against the per-stage schedule, on one GPU, in one
process, alternating - the protocol of tools/far/far_bench.py.

The samples (edge8f, tone16, quant2d, dsum2d; <app>.mw.hsaco) run one iteration on a
`--size` x `--size` array, once per LANE SHAPE: the columns a lane holds of every tensor, from
the shape in which the widest end fills a lane's 16 bytes to the one in which the narrowest
does (kernel.mixed_shapes), as far as the register estimate takes them.

cC        = the sweep from the code object generated with `cols=C`: one launch of
            <app>_fused_k1 in the default schedule.  The shape the shipped blob has is marked
            `shipped`; the others are built into `--blob-dir` with hipcc when missing
            (`--build-only`: build them and stop, no GPU needed);
per-stage = the shipped blob under set_max_depth(-1): one launch per stage, one cell per
            work-item, every local through memory - what these programs run without the switch.

First every schedule runs once and its output is compared with the per-stage output bit for
bit on the output's box, at the size timed: nothing is timed unless they are identical.  A
round times `--repeats` back-to-back sweeps of one schedule between device events and takes
their mean; the rounds of the schedules alternate, the first `--warmup` rounds are dropped,
and the median, the fastest and the slowest of the `--sweeps` timed rounds are reported.  A
schedule is FASTER than per-stage if its median is below the per-stage median by more than the
spread (the larger max - min of the two): far_bench.judge().

Registers and spills come from the code object's metadata, code sizes from its symbol table.

    python tools/mixed2d/mixed2d_bench.py [--apps APP ...] [--size N] [--blob-dir DIR]
                                          [--build-only] [--sweeps K] [--repeats R] [--out FILE]
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

BASELINE = 'per-stage'
ON = dict(mixed_widths=True)


def shapes_taken(spec):
  """[(cols, table)] of the lane shapes of kernel.mixed_shapes that make the kernel."""
  from soda_hip.codegen import kernel
  out = []
  for cols in sorted(kernel.mixed_shapes(spec)):
    table = kernel.generate(spec, cols=cols, **ON)[1]
    if any(k['kind'] == 'fused' for k in table):
      out.append((cols, table))
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=None,
                  help='default: the samples of mixed_widths (edge8f tone16 quant2d dsum2d)')
  ap.add_argument('--size', type=int, default=16384, help='columns and rows of the array')
  ap.add_argument('--blob-dir', default=os.path.join(ROOT, 'tools', 'mixed2d', 'blobs'),
                  help='where the code objects of the lane shapes are kept')
  ap.add_argument('--build-only', action='store_true',
                  help='build the code objects of every lane shape and stop')
  ap.add_argument('--sweeps', type=int, default=7, help='timed rounds per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=2, help='untimed rounds per schedule')
  ap.add_argument('--repeats', type=int, default=5, help='sweeps per round')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.sweeps >= 3
  import numpy as np
  import __graft_entry__ as entry
  from soda_hip import frontend
  from soda_hip.codegen import kernel, spec as specmod
  apps = args.apps or list(entry.MIXED_WIDTHS_APPS)
  specs = {app: specmod.spec_from_stencil(frontend.load(entry.sample_path(app))) for app in apps}
  shipped = {app: [k for k in kernel.generate(specs[app], **ON)[1] if k['kind'] == 'fused'][0]
             for app in apps}

  def blob_of(app, cols):
    return os.path.join(args.blob_dir, '%s.mw.c%d.hsaco' % (app, cols))

  for app in apps:
    for cols, _ in shapes_taken(specs[app]):
      if not os.path.exists(blob_of(app, cols)):
        os.makedirs(args.blob_dir, exist_ok=True)
        kernel.compile_to_code_object(kernel.generate(specs[app], cols=cols, **ON)[0],
                                      blob_of(app, cols))
  if args.build_only:
    return
  from soda_hip.runtime import host
  from codegen_util import code_bytes, static_figures  # tests/: a code object's notes
  from far_bench import judge
  dims = (args.size, args.size)
  shape = tuple(reversed(dims))
  lines = [
      'Mixed-width fused 2-D kernels (kernel.generate: mixed_widths) against the per-stage',
      'schedule of the shipped code object, per lane shape (cC: C columns of every tensor per',
      'lane).  tools/mixed2d/mixed2d_bench.py: the output of every schedule compared bit for bit',
      'with the per-stage output first; then rounds of %d back-to-back sweeps between device'
      % args.repeats,
      'events, the schedules alternating, %d untimed rounds, then the median (min .. max) of %d'
      % (args.warmup, args.sweeps),
      'timed rounds.  A sweep = 1 iteration.  FASTER: the medians differ by more than the spread',
      '(the larger max - min of the two series).  Register figures: code-object metadata (hipcc,',
      'gfx950).', '']
  for app in apps:
    spec = specs[app]
    variants = shapes_taken(spec)
    progs = {}
    for cols, table in variants:
      prog = host.open_program(blob=blob_of(app, cols), spec=spec)
      assert prog.kernels == table, blob_of(app, cols)
      progs[cols] = prog
    base = host.open_program(blob=entry.blob_path(app, **ON), spec=spec)
    stage_names = [e['name'] for e in base.kernels if e['kind'] == 'stage']
    rng = np.random.default_rng(7)
    n_cells = int(np.prod(shape))
    din = [host.DeviceArray(n_cells * dt.itemsize) for dt in base.in_dtypes]
    dout = [host.DeviceArray(n_cells * dt.itemsize) for dt in base.out_dtypes]
    for d, dt in zip(din, base.in_dtypes):
      a = rng.random(shape, dtype=np.float32).astype(dt) if dt.kind == 'f' else \
          rng.integers(0, np.iinfo(dt).max + 1, size=shape, dtype=dt)
      d.upload(a)
      del a
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    schedules = [('c%d' % cols, progs[cols], 0) for cols, _ in variants]
    schedules.append((BASELINE, base, -1))
    launches = {}

    def run(name, prog, depth_limit, repeats):
      prog.set_max_depth(depth_limit)
      try:
        launches[name] = [e['name'] for e, _ in prog.schedule(dims, 1)]
        return prog.sweep_timed(pin, pout, dims, 1, warmup=0, repeats=repeats)
      finally:
        prog.set_max_depth(0)

    (out_name,) = spec['outputs']
    lo, hi = specmod.iteration_boxes(spec, 1)[-1][out_name]
    box = tuple(slice(-lo[d], dims[d] - hi[d]) for d in reversed(range(2)))
    reference, same = None, {}
    for name, prog, depth_limit in reversed(schedules):
      dout[0].zero()
      run(name, prog, depth_limit, 1)
      got = np.ascontiguousarray(dout[0].download(shape, prog.out_dtypes[0])[box])
      if reference is None:
        reference = got
      same[name] = np.array_equal(got.view(np.uint8), reference.view(np.uint8))
      del got
    del reference
    assert launches[BASELINE] == stage_names, launches[BASELINE]
    for name, _, _ in schedules[:-1]:
      assert launches[name] == [app + '_fused_k1'], (name, launches[name])
    assert all(same.values()), '%s: outputs differ from the per-stage output: %s' % (app, same)
    times = {s[0]: [] for s in schedules}
    for r in range(args.warmup + args.sweeps):     # alternating: drift hits all alike
      for name, prog, depth_limit in schedules:
        t = run(name, prog, depth_limit, args.repeats)
        if r >= args.warmup:
          times[name].append(t['kernel_us'] / 1e3)
    updates = specmod.valid_cells(spec, dims, 1)
    alg = specmod.algorithmic_bytes_per_update(spec)
    rows = judge(times)
    lines.append('%s %d x %d, %d timed rounds of %d sweeps each; outputs of all schedules '
                 'bit-identical on the box' % (app, dims[0], dims[1], args.sweeps, args.repeats))
    lines.append('  schedule     ms per sweep: median  min .. max      launches  Gcell/s  '
                 'TB/s alg.  against per-stage')
    record = dict(app=app, dims=list(dims), shipped=shipped[app]['cols'], schedules={})
    for name, row in rows.items():
      ms = row['ms']
      mark = ' shipped' if name == 'c%d' % shipped[app]['cols'] else ''
      lines.append('  %-10s %12.3f  %10.3f .. %-10.3f %6d  %7.1f  %9.2f  %s' % (
          name, ms, row['min_ms'], row['max_ms'], len(launches[name]),
          updates / (ms * 1e-3) / 1e9, alg * updates / (ms * 1e-3) / 1e12,
          '' if name == BASELINE else '%.2f x, %s (spread %.3f ms)%s' % (
              row['speedup'], row['verdict'], row['spread'], mark)))
      record['schedules'][name] = dict(ms=ms, min_ms=row['min_ms'], max_ms=row['max_ms'],
                                       speedup=row['speedup'], verdict=row['verdict'])
    for cols, table in variants:
      (k,) = [e for e in table if e['kind'] == 'fused']
      f = static_figures(blob_of(app, cols), k['name'])
      lines.append('  %-8s %s, halo %d/%d, %3d of %4d columns out; %s' % (
          'c%d' % cols, 'seam-free' if k.get('exact') else 'overlapping', k['halo'][0],
          k['halo'][1], k['w_out'], 64 * k['cols'],
          '%d VGPRs (estimate %d), %d SGPRs, scratch %d B, spills %d VGPR / %d SGPR, code %d B'
          % (f['vgpr_count'], k['est_vgprs'], f['sgpr_count'], f['private_segment_fixed_size'],
             f['vgpr_spill_count'], f['sgpr_spill_count'], code_bytes(blob_of(app, cols), k['name']))
          if f else '(no code object here)'))
    lines.append('')
    for d in din + dout:
      d.free()
    for prog in list(progs.values()) + [base]:
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
