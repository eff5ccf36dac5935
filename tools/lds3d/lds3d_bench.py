#!/usr/bin/env python3
"""High-order 3-D stencils (star3d, iso3dfd, skewstar3d at 512 x 512 x 512, star3d and
skewstar3d at their own `iterate`): the LDS-plane kernel (kernel.generate's `lds_planes`,
kernel_stream3d_lds) against the per-stage schedule, on one GPU, both from the code object
__graft_entry__.build() makes with the switch (<app>.lds.hsaco), in one process,
alternating - the protocol of tools/rect_bench.py.

lds       = the blob's default schedule: one launch of <app>_fused_k1l per iteration;
per-stage = the same blob under set_max_depth(-1): one launch per iteration of the stage
            kernel, one cell per work-item, every operand a global load - what these
            programs run without the switch.

A round times `--repeats` back-to-back sweeps of one schedule between device events and
takes their mean; the rounds of the two schedules alternate, the first `--warmup` rounds
are dropped, and the median, the fastest and the slowest of the `--sweeps` timed rounds
are reported.  The LDS-plane kernel is FASTER if its median is below the per-stage median
by more than the spread (the larger max - min of the two).  After the timing both
schedules' outputs are compared bit for bit on the output's box, at the size timed.

Then the shape candidates of kernel_stream3d_lds.SHAPES that fit the register budget and
the LDS cap, one at a time (`--candidates N`: the first N in the generator's order; the
shipped shape is the first): `--shape-rounds` timed rounds each, median per sweep.  Their
code objects come from `--build-candidates` (no GPU needed: hipcc, into the blobs
directory) or, where that was not run, from a run-time compile.

`--fields`: the same protocol for the form over several outputs (kernel.generate's
`lds_fields`; acoustic3d, skewwave3d, deriv3d from <app>.ldsf.hsaco, each at its own
`iterate`).  There `lds` is the blob under set_max_depth(1) - a fused kernel over several
outputs is not in the default schedule - and per-stage one launch per stage and iteration;
every output is compared on its own box; no shape candidates are timed.

`--ring`: the same protocol for the plane-ring form (kernel.generate's `lds_ring`; cross3d,
skewcross3d, coupled3d from <app>.ldsr.hsaco, each at its own `iterate`), `lds` being the
blob under set_max_depth(1).  Every shape of kernel_stream3d_lds.SHAPES that fits is a
candidate (`--candidates 0`: all), the rule's shape first, so the best shape at or below
64 KiB of LDS is among them; a candidate's every output is compared on its own box, and its
fastest and slowest round are printed besides the median.

Registers, LDS and scratch come from the code object's metadata.  `--static` prints the
derived and the compiler's figures and times nothing (no GPU needed).

    python tools/lds3d/lds3d_bench.py [--apps APP ...] [--size W H D] [--sweeps K] [--repeats R]
                                [--candidates N] [--static] [--build-candidates] [--out FILE]
                                [--fields | --ring]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tools'),
          os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)


def static_line(kname, f):
  if not f:
    return '  %-22s (no code object here)' % kname
  return ('  %-22s %3d VGPRs, %3d SGPRs, LDS %d B, scratch %d B, spills %d VGPR / %d SGPR' % (
      kname, f['vgpr_count'], f['sgpr_count'], f['group_segment_fixed_size'],
      f['private_segment_fixed_size'], f['vgpr_spill_count'], f['sgpr_spill_count']))


def fitting_shapes(spec, ring=False):
  """The shapes the generator would take, in its order, with their entries."""
  from soda_hip.codegen import kernel_stream2d, kernel_stream3d_lds
  from soda_hip.codegen import spec as specmod
  lowered = specmod.inline_pointwise(spec)
  form = dict(fields=len(spec['outputs']) > 1, ring=True) if ring else {}
  out = []
  for shape in kernel_stream3d_lds.shapes_by_loaded_cells(lowered, **form):
    try:
      out.append((shape, kernel_stream3d_lds.emit(lowered, 1, *shape, **form)[1]))
    except kernel_stream2d.NotFusable:
      pass
  return out


def candidate_path(entry, app, shape, ring=False):
  return os.path.join(entry.BLOBS, '%s.lds%s.%dx%dx%d.hsaco' % (
      (app, 'r' if ring else '') + tuple(shape)))


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--apps', nargs='+', default=None, help='default: star3d iso3dfd skewstar3d')
  ap.add_argument('--size', nargs=3, type=int, default=[512, 512, 512])
  ap.add_argument('--sweeps', type=int, default=7, help='timed rounds per schedule (>= 3)')
  ap.add_argument('--warmup', type=int, default=2, help='untimed rounds per schedule')
  ap.add_argument('--repeats', type=int, default=10, help='sweeps per round')
  ap.add_argument('--candidates', type=int, default=6, help='shape candidates timed per app')
  ap.add_argument('--shape-rounds', type=int, default=3)
  ap.add_argument('--static', action='store_true',
                  help='the static figures only (registers, LDS, derived traffic): no GPU')
  ap.add_argument('--build-candidates', action='store_true',
                  help='compile the candidates\' code objects (hipcc) and exit: no GPU')
  ap.add_argument('--fields', action='store_true',
                  help='the form over several outputs (lds_fields) instead of lds_planes')
  ap.add_argument('--ring', action='store_true',
                  help='the plane-ring form (lds_ring) instead of lds_planes')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert args.sweeps >= 3 and not (args.fields and args.ring)
  import __graft_entry__ as entry
  from soda_hip import frontend
  from soda_hip.codegen import kernel, spec as specmod
  from codegen_util import static_figures  # tests/: a code object's notes
  apps = args.apps or list(entry.LDS_FIELDS_APPS if args.fields else
                           entry.LDS_RING_APPS if args.ring else entry.LDS3D_APPS)
  if args.fields:
    args.candidates = 0
  on = dict(lds_ring=True) if args.ring else dict(lds_planes=True)    # of the candidates
  dims = tuple(args.size)
  shape = tuple(reversed(dims))
  lines = [
      'LDS-plane kernels for high-order 3-D stencils (kernel.generate: %s) against the'
      % ('lds_fields' if args.fields else 'lds_ring' if args.ring else 'lds_planes'),
      'per-stage schedule.  tools/lds3d/lds3d_bench.py: rounds of %d back-to-back sweeps between device'
      % args.repeats,
      'events, the two schedules alternating, %d untimed rounds, then the median (min .. max) of'
      % args.warmup,
      '%d timed rounds, per sweep (a sweep = `iterate` iterations).  FASTER: the medians differ by'
      % args.sweeps,
      'more than the spread (the larger max - min).  Bytes per cell are derived from the table,',
      'rates are algorithmic bytes x valid cell-updates over the measured time.  Register and LDS',
      'figures: code-object metadata (hipcc, gfx950).'] + ([] if args.fields else [
          'Shape candidates: (wavefronts, rows per lane, lanes per tile row), %d timed rounds each, '
          'median%s.' % (args.shape_rounds, ' (min .. max)' if args.ring else '')]) + ['']
  for app in apps:
    spec = specmod.spec_from_stencil(frontend.load(entry.sample_path(app)))
    iterate = spec['iterate']
    if args.fields:
      from soda_hip.codegen import switches
      blob = entry.blob_path(app, lds_fields=True)
      table = kernel.generate(spec, **switches.for_program(spec, lds_fields=True))[1]
    else:
      blob = entry.blob_path(app, **on)
      table = kernel.generate(spec, **on)[1]
    k = table[-1]
    several = len(spec['outputs']) > 1
    assert k['kind'] == 'fused' and k['name'] == app + (
        '_fused_k1lf' if args.fields else
        '_fused_k1r' + 'f' * several if args.ring else '_fused_k1l'), k
    stage_names = [e['name'] for e in table if e['kind'] == 'stage']
    shapes = [] if args.fields else fitting_shapes(spec, args.ring)
    shapes = shapes[:max(1, args.candidates) if args.candidates or not args.ring else None]
    assert args.fields or (shapes[0][1]['tile'] == k['tile'] and
                           shapes[0][1]['block'] == k['block'])
    if args.build_candidates:
      for cand, _ in shapes[1:]:
        text = kernel.generate(spec, lds_shape=cand, **on)[0]
        kernel.compile_to_code_object(text, candidate_path(entry, app, cand, args.ring))
        print('built', candidate_path(entry, app, cand, args.ring))
      continue
    elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
    alg = specmod.algorithmic_bytes_per_update(spec)
    cells = k['tile'][0] * k['tile'][1]
    n_loads = sum(len(st['loads']) for st in specmod.inline_pointwise(spec)['stages'])
    static = [
        '  bytes per cell: algorithmic %d; LDS-plane kernel %.2f with its halo (tile %d x %d, '
        '%d wavefronts, %d rows per lane, halo x %d+%d y %d+%d); per-stage %d global loads of '
        '%d B per cell' % ((alg, k['step_bytes'] / float(cells), k['tile'][0], k['tile'][1],
                            k['waves'], k['rows']) + tuple(k['halo']) + (n_loads, elem)),
        static_line(k['name'], static_figures(blob, k['name']))] + [
            static_line(name, static_figures(blob, name)) for name in stage_names]
    if args.static:
      lines.append('%s: NOT MEASURED (static figures only)' % app)
      lines += static
      for cand, e in shapes[1:]:
        lines.append(static_line('  shape %s' % (cand,), static_figures(
            candidate_path(entry, app, cand, args.ring), k['name'])))
      continue
    import numpy as np
    from soda_hip.runtime import host
    prog = host.open_program(blob=blob, spec=spec)
    assert prog.kernels[-1]['name'] == k['name']
    rng = np.random.default_rng(7)
    n_cells = int(np.prod(shape))
    din = [host.DeviceArray(n_cells * dt.itemsize) for dt in prog.in_dtypes]
    dout = [host.DeviceArray(n_cells * dt.itemsize) for dt in prog.out_dtypes]
    for d, dt in zip(din, prog.in_dtypes):
      a = rng.random(shape, dtype=np.float32)
      d.upload(a.astype(dt))
      del a
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    fused_limit = 1 if args.fields or args.ring else 0
    schedules = [('lds', fused_limit), ('per-stage', -1)]
    times = {name: [] for name, _ in schedules}
    launches = {}

    def run(program, name, limit, repeats):
      program.set_max_depth(limit)
      try:
        launches[name] = [e['name'] for e, _ in program.schedule(dims, iterate)]
        return program.sweep_timed(pin, pout, dims, iterate, warmup=0, repeats=repeats)
      finally:
        program.set_max_depth(0)

    for r in range(args.warmup + args.sweeps):     # alternating: drift hits both alike
      for name, limit in schedules:
        t = run(prog, name, limit, args.repeats)
        if r >= args.warmup:
          times[name].append(t['kernel_us'] / 1e3)
    assert launches['lds'] == [k['name']] * iterate, launches
    assert launches['per-stage'] == stage_names * iterate, launches
    # both schedules' results at this size, bit for bit on every output's box
    results = {}
    for name, limit in schedules:
      for d in dout:
        d.zero()
      run(prog, name, limit, 1)
      results[name] = [d.download(shape, dt) for d, dt in zip(dout, prog.out_dtypes)]
    same = True
    references, slices = [], []     # (the shape candidates below: per output, its box)
    for j, name in enumerate(spec['outputs']):
      lo, hi = specmod.iteration_boxes(spec, iterate)[-1][name]
      sl = tuple(slice(-lo[d], dims[d] - hi[d]) for d in (2, 1, 0))
      a, b = results['lds'][j][sl], results['per-stage'][j][sl]
      same = same and bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                          np.ascontiguousarray(b).view(np.uint8)))
      if j == 0 or args.ring:
        references.append(np.ascontiguousarray(b).copy())
        slices.append(sl)
    del results, a, b
    updates = specmod.valid_cells(spec, dims, iterate)
    med = {n: statistics.median(ts) for n, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    verdict = 'FASTER' if med['per-stage'] - med['lds'] > spread else \
        'SLOWER' if med['lds'] - med['per-stage'] > spread else 'NO DIFFERENCE beyond the spread'
    lines.append('%s %s x %d, %d timed rounds of %d sweeps each (ms per sweep: median, min .. max)'
                 % (app, ' x '.join(map(str, dims)), iterate, args.sweeps, args.repeats))
    for name, _ in schedules:
      ts = sorted(times[name])
      lines.append('  %-10s %8.3f  %8.3f .. %-8.3f  %6.2f TB/s algorithmic, %6.1f Gcell/s  '
                   '[%d launch(es)]' % (
                       name, med[name], ts[0], ts[-1], alg * updates / (med[name] * 1e-3) / 1e12,
                       updates / (med[name] * 1e-3) / 1e9, len(launches[name])))
    lines.append('  lds is %s: %.2f x per-stage (spread %.3f ms); outputs %s on the box'
                 % (verdict, med['per-stage'] / med['lds'], spread,
                    'bit-identical' if same else 'DIFFER'))
    lines += static
    record = dict(app=app, dims=list(dims), iterate=iterate, ms=med, spread_ms=spread,
                  verdict=verdict, speedup=med['per-stage'] / med['lds'], identical=same,
                  shapes={})
    # the shape candidates, one at a time, each checked against the per-stage result
    for cand, e in shapes:
      path = candidate_path(entry, app, cand, args.ring)
      if cand == shapes[0][0]:
        other, how = prog, 'shipped'
      elif os.path.exists(path):
        other, how = host.open_program(blob=path, spec=spec), 'prebuilt'
      else:
        other, how = host.open_program(source=kernel.generate(
            spec, lds_shape=cand, **on)[0], spec=spec), 'run-time compile'
      assert other.kernels[-1]['tile'] == e['tile'] and other.kernels[-1]['block'] == e['block']
      ts = []
      for r in range(1 + args.shape_rounds):
        t = run(other, 'shape', fused_limit, args.repeats)
        if r:
          ts.append(t['kernel_us'] / 1e3)
      assert launches['shape'] == [k['name']] * iterate
      for d in dout:
        d.zero()
      run(other, 'shape', fused_limit, 1)
      ok = True
      for j, (reference, sl) in enumerate(zip(references, slices)):
        got = np.ascontiguousarray(dout[j].download(shape, prog.out_dtypes[j])[sl])
        ok = ok and bool(np.array_equal(got.view(np.uint8), reference.view(np.uint8)))
        del got
      f = static_figures(path if other is not prog else blob, k['name'])
      lines.append('  shape %-12s tile %3d x %-3d %8.3f ms%s  %.2f x per-stage  loaded/stored %.3f  '
                   '%s VGPRs, LDS %d B  %s%s' % (
                       cand, e['tile'][0], e['tile'][1], statistics.median(ts),
                       ' (%.3f .. %.3f)' % (min(ts), max(ts)) if args.ring else '',
                       med['per-stage'] / statistics.median(ts),
                       e['loaded_cells'] / float(e['tile'][0] * e['tile'][1]) /
                       max(1, e['lds_planes']) if len(spec['inputs']) == 1 else
                       e['lds_bytes'] / float(sum(e.get('lds_ring', [2]))) / elem /
                       (e['tile'][0] * e['tile'][1]),
                       f.get('vgpr_count', '?'), e['lds_bytes'], how,
                       '' if ok else '  OUTPUT DIFFERS'))
      record['shapes'][str(cand)] = dict(ms=statistics.median(ts), min_ms=min(ts),
                                         max_ms=max(ts), lds_bytes=e['lds_bytes'],
                                         identical=ok)
      same = same and ok
      if other is not prog:
        other.close()
        other.blob.unload()
    for d in din + dout:
      d.free()
    prog.close()
    print(json.dumps(record), flush=True)
    assert same, '%s: LDS-plane and per-stage outputs differ' % app
  text = '\n'.join(lines) + '\n'
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
