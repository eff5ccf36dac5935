#!/usr/bin/env python3
"""Multi-field programs, fused against per-stage, on one GPU: wave2d and fdtd2d at
8192 x 8192 x 100 iterations or, with `--apps 3d` (wave3d and maxwell3d), at
384 x 384 x 384 x 20, under bench.py's protocol (warm-up sweeps, then the median
of event-timed sweeps; sweeps are repeated until the timed region is long enough for
steady clocks).

Per program: the scheduler's own split of the fused depths (set_max_depth(8); without a
limit these programs run per stage until this measurement admits a depth), the per-stage
schedule, and every fused depth of
the table alone (the sweep as N / d launches of depth d), alternating so that clock
drift hits all of them alike.  The per-stage schedule is set_max_depth(-1): one launch
per stage per iteration, every field through HBM every iteration.  It stands for the
commit before the fused multi-field kernels, which had nothing else for these programs:
the stage kernels' text is byte for byte that commit's (kernel_stage.py is unchanged) and
the launcher's per-stage path is the same, so both sides are timed in one process, on one
device, interleaved.

A depth SHIPS if its median time per iteration is below the per-stage one by more than
the run-to-run spread: the larger of the two schedules' (max - min) over the timed sweeps.
Registers, occupancy and scratch per kernel are read from the code object's metadata; for
the 3-D kernels the tile and the fraction of it that survives the halo come from the table.
Prints one JSON line per program and writes the whole table to the file given with --out.

    python tools/fields_bench.py [--apps 2d | 3d | APP ...] [--size W H [D]] [--iterate N]
                                 [--sweeps K] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)


READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'
DEFAULTS = {'2d': ('wave2d', 'fdtd2d'), '3d': ('wave3d', 'maxwell3d')}


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
                       for k in ('vgpr_count', 'sgpr_count', 'vgpr_spill_count',
                                 'sgpr_spill_count', 'private_segment_fixed_size')}
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=['2d'],
                  help="'2d' = wave2d fdtd2d, '3d' = wave3d maxwell3d, or sample names of "
                  'one dimensionality')
  ap.add_argument('--size', nargs='+', type=int, default=None,
                  help='default 8192 8192, for 3-D programs 384 384 384')
  ap.add_argument('--iterate', type=int, default=None, help='default 100, for 3-D programs 20')
  ap.add_argument('--sweeps', type=int, default=7, help='timed sweeps per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  import numpy as np
  import __graft_entry__ as entry
  from soda_hip import frontend
  from soda_hip.codegen import spec as specmod
  from soda_hip.runtime import host
  assert args.sweeps >= 3
  args.apps = [a for name in args.apps for a in DEFAULTS.get(name, (name,))]
  dim = specmod.spec_from_stencil(frontend.load(entry.sample_path(args.apps[0])))['dim']
  args.size = args.size or ([8192, 8192] if dim == 2 else [384, 384, 384])
  args.iterate = args.iterate or (100 if dim == 2 else 20)
  assert len(args.size) == dim, '--size needs %d extents' % dim
  dims = tuple(args.size)
  shape = tuple(reversed(dims))
  compiler = ''
  try:
    hipcc = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
    m = re.search(r'HIP version: (\S+)', subprocess.check_output([hipcc, '--version']).decode())
    compiler = m.group(1) if m else ''
  except (OSError, subprocess.CalledProcessError):
    pass
  lines = [
      'Multi-field fused %d-D kernels (codegen/kernel_fields%dd.py) against the per-stage schedule'
      % (dim, dim),
      'tools/fields_bench.py: warm-up, then the median of event-timed sweeps, schedules interleaved.',
      'per-stage = set_max_depth(-1): it stands for the commit before these kernels, whose stage',
      'kernels have byte for byte this text and which had nothing else for these programs.',
      'A depth SHIPS if its median is below the per-stage median by more than the spread (the larger',
      'max - min of the two).  Register figures: code-object metadata, hipcc HIP %s, gfx950.'
      % (compiler or '(unknown)'), '']
  for app in args.apps:
    spec = specmod.spec_from_stencil(frontend.load(entry.sample_path(app)))
    assert spec['dim'] == dim, '%s is not a %d-D program' % (app, dim)
    blob = entry.blob_path(app)
    prog = host.open_program(blob=blob, spec=spec)
    rng = np.random.default_rng(7)
    cells = int(np.prod(shape))
    din = [host.DeviceArray(cells * dt.itemsize) for dt in prog.in_dtypes]
    dout = [host.DeviceArray(cells * dt.itemsize) for dt in prog.out_dtypes]
    for d, dt in zip(din, prog.in_dtypes):
      d.upload(rng.random(shape, dtype=np.float32).astype(dt))
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    depths = sorted(k['depth'] for k in prog.kernels if k['kind'] == 'fused')
    schedules = [('chosen', 8, None), ('per-stage', -1, None)]
    for d in depths:
      split = [d] * (args.iterate // d) + [1] * (args.iterate % d)
      schedules.append(('depth %d' % d, d, split))
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
    result = dict(app=app, dims=list(dims), iterate=args.iterate, sweeps=args.sweeps,
                  algorithmic_bytes_per_update=alg, schedules={})
    lines.append('%s %s x %d, %d timed sweeps each (ms per sweep: median, min .. max)'
                 % (app, ' x '.join(map(str, dims)), args.iterate, args.sweeps))
    stage = sorted(times['per-stage'])
    stage_med, stage_range = statistics.median(stage), stage[-1] - stage[0]
    for name, limit, split in schedules:
      ts = sorted(times[name])
      med = statistics.median(ts)
      fused = [d for d in launches[name] if d]
      split_text = 'per-stage, %d launches' % len(launches[name]) if not fused else \
          ' + '.join('%d x depth %d' % (fused.count(d), d) for d in sorted(set(fused), reverse=True))
      entry_ = dict(ms=med, ms_min=ts[0], ms_max=ts[-1], split=split_text,
                    us_per_iteration=med * 1e3 / args.iterate)
      tail = ''
      if split:
        spread = max(stage_range, ts[-1] - ts[0])
        ships = stage_med - med > spread
        entry_.update(us_per_launch=med * 1e3 / len(split), spread_ms=spread, ships=ships)
        tail = ', %.1f us per launch, spread %.3f ms: %s' % (
            med * 1e3 / len(split), spread, 'SHIPS' if ships else 'DOES NOT SHIP')
      result['schedules'][name] = entry_
      lines.append('  %-10s %8.3f  %8.3f .. %-8.3f  %7.2f us per iteration%s  [%s]' % (
          name, med, ts[0], ts[-1], med * 1e3 / args.iterate, tail, split_text))
    fused_names = {k['name']: k['depth'] for k in prog.kernels if k['kind'] == 'fused'}
    figures = isa_figures(blob, fused_names)
    result['isa'] = figures
    for kname in sorted(figures, key=fused_names.get):
      f = figures[kname]
      lines.append('  %-22s %3d VGPRs, %d waves per SIMD, %3d SGPRs, scratch %d B, spills '
                   '%d VGPR / %d SGPR' % (
                       kname, f['vgpr_count'], min(8, 512 // (-(-f['vgpr_count'] // 8) * 8)),
                       f['sgpr_count'], f['private_segment_fixed_size'],
                       f['vgpr_spill_count'], f['sgpr_spill_count']))
    for k in sorted((k for k in prog.kernels if k['kind'] == 'fused' and 'rows' in k),
                    key=lambda k: k['depth']):
      lines.append('  %-22s tile %d x %d per wavefront, %d x %d stored: %.2f of it kept' % (
          k['name'], 64 * k['cols'], k['rows'], k['w_out'], k['r_out'],
          k['w_out'] * k['r_out'] / (64.0 * k['cols'] * k['rows'])))
    lines.append('  algorithmic bytes per cell-update: %d (per-stage moves more: every stage '
                 'reads its operands from and writes its result to HBM)' % alg)
    print(json.dumps(result))
    prog.close()
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
