#!/usr/bin/env python3
"""Multi-field programs, fused against per-stage, on one GPU: wave2d and fdtd2d at
8192 x 8192 x 100 iterations or, with `--apps 3d` (wave3d and maxwell3d), at
384 x 384 x 384 x 20 or, with `--apps 1d` (wave1d and fdtd1d), at 2^27 cells x 96, under
bench.py's protocol (warm-up sweeps, then the median
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
For the 1-D kernels the derived HBM bytes per cell-update of every depth stand next to the
register figures; `--static` prints those two and times nothing (no GPU needed).
Prints one JSON line per program and writes the whole table to the file given with --out.

    python tools/fields_bench.py [--apps 1d | 2d | 3d | APP ...] [--size W [H [D]]]
                                 [--iterate N] [--sweeps K] [--static] [--out FILE]
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
DEFAULTS = {'1d': ('wave1d', 'fdtd1d'), '2d': ('wave2d', 'fdtd2d'), '3d': ('wave3d', 'maxwell3d')}
SIZES = {1: [1 << 27], 2: [8192, 8192], 3: [384, 384, 384]}
ITERATE = {1: 96, 2: 100, 3: 20}


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


def traffic_lines(spec, kernels):
  """Derived, not measured: HBM bytes per cell-update of the per-stage schedule (every stage
  reads each tensor it names once and writes its result) and of every fused 1-D depth (a
  segment loads 64 * cols cells of every field for the w_out it stores, once per `depth`
  updates)."""
  from soda_hip.codegen import spec as specmod
  lowered = specmod.inline_pointwise(spec)
  types = specmod.tensor_c_types(lowered)
  staged = sum(specmod.ELEM_SIZE[types[t]] for stage in lowered['stages']
               for t in sorted({name for name, _ in stage['loads']}) + [stage['name']])
  lines = ['  derived HBM bytes per cell-update: per-stage %d' % staged]
  for k in sorted((k for k in kernels if k['kind'] == 'fused' and k.get('fields') and
                   k['fill_rows'] == 0), key=lambda k: k['depth']):
    elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
    per = (len(spec['inputs']) * 64.0 * k['cols'] / k['w_out'] + len(spec['outputs'])) * \
        elem / k['depth']
    lines.append('  %-22s %5.2f B per cell-update (segment %d cells, %d stored, %d segments '
                 'per wavefront)' % (k['name'], per, 64 * k['cols'], k['w_out'], k['segs']))
  return lines


def isa_lines(figures, depth_of):
  return ['  %-22s %3d VGPRs, %d waves per SIMD, %3d SGPRs, scratch %d B, spills '
          '%d VGPR / %d SGPR' % (
              kname, f['vgpr_count'], min(8, 512 // (-(-f['vgpr_count'] // 8) * 8)),
              f['sgpr_count'], f['private_segment_fixed_size'],
              f['vgpr_spill_count'], f['sgpr_spill_count'])
          for kname, f in sorted(figures.items(), key=lambda kf: depth_of[kf[0]])]


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=['2d'],
                  help="'1d' = wave1d fdtd1d, '2d' = wave2d fdtd2d, '3d' = wave3d maxwell3d, or sample names of "
                  'one dimensionality')
  ap.add_argument('--size', nargs='+', type=int, default=None,
                  help='default 8192 8192, for 3-D programs 384 384 384, for 1-D ones 2^27')
  ap.add_argument('--iterate', type=int, default=None,
                  help='default 100, for 3-D programs 20, for 1-D ones 96')
  ap.add_argument('--static', action='store_true',
                  help='the static figures only (registers, derived traffic): no GPU')
  ap.add_argument('--sweeps', type=int, default=7, help='timed sweeps per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  import __graft_entry__ as entry
  from soda_hip import frontend
  from soda_hip.codegen import spec as specmod
  assert args.sweeps >= 3
  args.apps = [a for name in args.apps for a in DEFAULTS.get(name, (name,))]
  dim = specmod.spec_from_stencil(frontend.load(entry.sample_path(args.apps[0])))['dim']
  args.size = args.size or SIZES[dim]
  args.iterate = args.iterate or ITERATE[dim]
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
    if args.static:
      from soda_hip.codegen import kernel
      table = kernel.generate(spec)[1]
      depth_of = {k['name']: k['depth'] for k in table if k['kind'] == 'fused'}
      lines.append('%s: NOT YET MEASURED (static figures only)' % app)
      lines += isa_lines(isa_figures(blob, depth_of), depth_of)
      lines += traffic_lines(spec, table) if dim == 1 else []
      continue
    import numpy as np
    from soda_hip.runtime import host
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
    lines += isa_lines(figures, fused_names)
    if dim == 1:
      lines += traffic_lines(spec, prog.kernels)
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
