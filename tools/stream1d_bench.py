#!/usr/bin/env python3
"""Iterated 1-D programs, fused (codegen/kernel_stream1d.py) against per-stage, on one GPU:
smooth1d and fir1d at 2^27 cells x 96 iterations.  One warm-up sweep per schedule, then
the median of event-timed sweeps, the schedules interleaved so that clock drift hits all
of them alike.

Per program: the per-stage schedule (set_max_depth(-1)), the planner's own split of the
fused depths under set_max_depth(12) (without a limit these programs run per stage), and
every fused depth of the table alone (the sweep as N / d launches of depth d, the rest at
depth 1).  The per-stage schedule is one launch per stage per iteration, the whole array
through HBM every time.  It stands for the commit before the fused 1-D kernels, which had
nothing else for these programs: the stage kernels' text is byte for byte that commit's
(kernel_stage.py is unchanged) and the launcher's per-stage path is the same, so both
sides are timed in one process, on one device, interleaved.

A depth SHIPS if its median time per sweep is below the per-stage one by more than the
run-to-run spread: the larger of the two schedules' (max - min) over the timed sweeps.
Registers, scratch and spills per kernel are read from the code object's metadata.  The
kernels are built by hipcc like the shipped code objects (into --blobs, reused from there
when present).  Prints one JSON line per program and writes the table to --out.

    python tools/stream1d_bench.py [--apps APP ...] [--cells N] [--iterate N] [--segs S]
                                   [--sweeps K] [--blobs DIR] [--out FILE] [--append]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'
FIGURES = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
           'private_segment_fixed_size')


def isa_figures(blob, names):
  """{kernel: metadata figures} from the code object's notes."""
  if not os.path.exists(READELF):
    return {}
  notes = subprocess.check_output([READELF, '--notes', blob]).decode()
  out = {}
  for block in notes.split('- .agpr_count'):
    m = re.search(r'\.name:\s+(\S+)', block)
    if not m or m.group(1) not in names:
      continue
    out[m.group(1)] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, block).group(1))
                       for k in FIGURES}
  return out


def blob_of(app, spec, segs, folder):
  """The program's code object with `segs` segments per wavefront: from `folder` when it
  is there, else built into it."""
  from soda_hip.codegen import kernel
  path = os.path.join(folder, '%s_segs%d.hsaco' % (app, segs))
  if not os.path.exists(path):
    os.makedirs(folder, exist_ok=True)
    text, _ = kernel.generate(spec, segs=segs)
    kernel.compile_to_code_object(text, path)
  return path


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=['smooth1d', 'fir1d'])
  ap.add_argument('--cells', type=int, default=1 << 27)
  ap.add_argument('--iterate', type=int, default=96)
  ap.add_argument('--segs', type=int, default=None,
                  help='segments per wavefront (default: the generator\'s)')
  ap.add_argument('--sweeps', type=int, default=7, help='timed sweeps per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=1)
  ap.add_argument('--blobs', default=None, help='folder of code objects to reuse / fill')
  ap.add_argument('--build-only', action='store_true',
                  help='build the code objects into --blobs and stop (needs no GPU)')
  ap.add_argument('--out', default=None)
  ap.add_argument('--append', action='store_true', help='append to --out')
  args = ap.parse_args()
  import numpy as np
  from soda_hip import frontend
  from soda_hip.codegen import kernel_stream1d
  from soda_hip.codegen import spec as specmod
  assert args.sweeps >= 3
  segs = args.segs or kernel_stream1d.DEFAULT_SEGS
  folder = args.blobs or tempfile.mkdtemp(prefix='stream1d_bench_')
  samples = os.path.join(ROOT, 'tests', 'samples', 'extra')
  specs = {app: specmod.spec_from_stencil(frontend.load(os.path.join(samples, app + '.soda'),
                                                        iterate=args.iterate))
           for app in args.apps}
  blobs = {app: blob_of(app, specs[app], segs, folder) for app in args.apps}
  if args.build_only:
    print('\n'.join(blobs.values()))
    return
  from soda_hip.runtime import host
  dims = (args.cells,)
  compiler = ''
  try:
    hipcc = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
    m = re.search(r'HIP version: (\S+)', subprocess.check_output([hipcc, '--version']).decode())
    compiler = m.group(1) if m else ''
  except (OSError, subprocess.CalledProcessError):
    pass
  lines = [
      'Fused 1-D kernels (codegen/kernel_stream1d.py), %d segments per wavefront, against the '
      'per-stage schedule' % segs,
      'tools/stream1d_bench.py: %d warm-up, then the median of event-timed sweeps, schedules '
      'interleaved.' % args.warmup,
      'per-stage = set_max_depth(-1): it stands for the commit before these kernels, whose stage',
      'kernels have byte for byte this text and which had nothing else for these programs.',
      'A depth SHIPS if its median is below the per-stage median by more than the spread (the larger',
      'max - min of the two).  Register figures: code-object metadata, hipcc HIP %s, gfx950.'
      % (compiler or '(unknown)'), '']
  for app in args.apps:
    spec = specs[app]
    prog = host.open_program(blob=blobs[app], spec=spec)
    rng = np.random.default_rng(7)
    din = [host.DeviceArray(args.cells * dt.itemsize) for dt in prog.in_dtypes]
    dout = [host.DeviceArray(args.cells * dt.itemsize) for dt in prog.out_dtypes]
    for d, dt in zip(din, prog.in_dtypes):
      d.upload(rng.random((args.cells,), dtype=np.float32).astype(dt))
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    depths = sorted(k['depth'] for k in prog.kernels if k['kind'] == 'fused')
    schedules = [('per-stage', -1, None), ('chosen', 12, None)]
    for d in depths:
      split = [d] * (args.iterate // d) + [1] * (args.iterate % d)
      schedules.append(('depth %d' % d, 0, split))
    times = {name: [] for name, _, _ in schedules}
    launches = {}

    def run(name, limit, split, timed):
      prog.set_max_depth(limit)
      if split:
        prog.set_split(dims, args.iterate, split)
      try:
        if name not in launches:
          launches[name] = [k['depth'] if k['kind'] == 'fused' else 0
                            for k, _ in prog.schedule(dims, args.iterate)]
        t = prog.sweep_timed(pin, pout, dims, args.iterate, warmup=0, repeats=1)
      finally:
        if split:
          prog.set_split(dims, args.iterate, [])
        prog.set_max_depth(0)
      if timed:
        times[name].append(t['kernel_us'] / 1e3)

    for _ in range(args.warmup):
      for name, limit, split in schedules:
        run(name, limit, split, False)
    for _ in range(args.sweeps):        # alternating: drift hits every schedule alike
      for name, limit, split in schedules:
        run(name, limit, split, True)
    for d in din + dout:
      d.free()
    alg = specmod.algorithmic_bytes_per_update(spec)
    result = dict(app=app, cells=args.cells, iterate=args.iterate, sweeps=args.sweeps,
                  segs=segs, algorithmic_bytes_per_update=alg, schedules={})
    lines.append('%s %d cells x %d, %d timed sweeps each (ms per sweep: median, min .. max)'
                 % (app, args.cells, args.iterate, args.sweeps))
    stage = sorted(times['per-stage'])
    stage_med, stage_range = statistics.median(stage), stage[-1] - stage[0]
    for name, limit, split in schedules:
      ts = sorted(times[name])
      med = statistics.median(ts)
      fused = [d for d in launches[name] if d]
      split_text = 'per-stage, %d launches' % len(launches[name]) if not fused else \
          ' + '.join('%d x depth %d' % (fused.count(d), d) for d in sorted(set(fused), reverse=True))
      entry = dict(ms=med, ms_min=ts[0], ms_max=ts[-1], split=split_text,
                   us_per_iteration=med * 1e3 / args.iterate)
      tail = ''
      if split:
        spread = max(stage_range, ts[-1] - ts[0])
        ships = stage_med - med > spread
        entry.update(spread_ms=spread, ships=ships)
        tail = ', spread %.3f ms: %s' % (spread, 'SHIPS' if ships else 'DOES NOT SHIP')
      result['schedules'][name] = entry
      lines.append('  %-10s %8.3f  %8.3f .. %-8.3f  %7.2f us per iteration%s  [%s]' % (
          name, med, ts[0], ts[-1], med * 1e3 / args.iterate, tail, split_text))
    fused_names = {k['name']: k['depth'] for k in prog.kernels if k['kind'] == 'fused'}
    figures = isa_figures(blobs[app], fused_names)
    result['isa'] = figures
    for kname in sorted(figures, key=fused_names.get):
      f = figures[kname]
      lines.append('  %-22s %3d VGPRs, %3d SGPRs, scratch %d B, spills %d VGPR / %d SGPR' % (
          kname, f['vgpr_count'], f['sgpr_count'], f['private_segment_fixed_size'],
          f['vgpr_spill_count'], f['sgpr_spill_count']))
    lines.append('  algorithmic bytes per cell-update: %d; a fused launch of depth d moves them once '
                 'per d iterations plus the halo' % alg)
    lines.append('')
    print(json.dumps(result))
    prog.close()
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.append else 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
