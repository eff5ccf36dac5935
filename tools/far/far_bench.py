#!/usr/bin/env python3
"""The far-reach fused kernels of one switch of kernel.generate (`--switch`) against the
per-stage schedule, on one GPU, both from the code object __graft_entry__.build() makes with
the switch, in one process, alternating - the protocol of tools/lds3d/lds3d_bench.py.

far_lanes = high-order 2-D stencils (star2d and skewfar2d at 16384 x 16384, dstar2d and
            acoustic2d at 8192 x 8192; <app>.far.hsaco): kernel_stream2d / kernel_fields2d with
            chained wave shifts;
far_taps  = long 1-D windows (lowpass1d, dfir1d, skewfir1d, acoustic1d on `--cells` cells;
            <app>.taps.hsaco): kernel_stream1d / kernel_fields1d with chained wave shifts.

default   = what a product of the switch's flag runs: the blob's default schedule.  Where the
            launcher admits the fused kernels only under a depth limit - over several fields
            (acoustic2d), and every 1-D one - under the limit the generated entry points set
            (switches.depth_limit_of); the row is then labelled `limit N`;
depth d   = the same sweep with its split fixed to launches of <app>_fused_k<d> only
            (soda_hip_plan_set_split), for every fused depth of the table;
per-stage = the same blob under set_max_depth(-1): one launch per stage and iteration, one
            cell per work-item, every operand a global load - what these programs run
            without the switch.

`--cols C` adds the same fused depths with C cells per lane instead of the default 16-byte
lanes (1-D, 8 floats or 4 doubles: 32-byte lanes, half the hops and half the halo share), as
rows `depth d cC`, from a second code object generated with `cols=C`: `--blob-dir`/<app><the
switch's suffix>.c<C>.hsaco, built there with hipcc when missing.  Name the apps the width
applies to.

First every schedule runs once and its outputs are compared with the per-stage outputs bit
for bit on every output's box, at the size timed: nothing is timed unless they are identical.
A round times `--repeats` back-to-back sweeps of one schedule between device events and takes
their mean; the rounds of the schedules alternate, the first `--warmup` rounds are dropped,
and the median, the fastest and the slowest of the `--sweeps` timed rounds are reported, per
sweep, per launch and per iteration.  A schedule is FASTER than per-stage if its median is
below the per-stage median by more than the spread (the larger max - min of the two): judge().

Registers and spills come from the code object's metadata, code sizes from its symbol table.

    python tools/far/far_bench.py --switch far_lanes|far_taps [--apps APP ...] [--cols C]
                                  [--blob-dir DIR] [--cells N] [--iterate N] [--sweeps K]
                                  [--repeats R] [--out FILE]
"""
import argparse
import collections
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

SIZES_2D = {4: (16384, 16384), 8: (8192, 8192)}      # by element size: float, double
BASELINE = 'per-stage'

# What differs between the switches.  apps: the samples' list in __graft_entry__; title: of
# the report; dims(args, element size): of the array, x first; size: how the report prints
# them; figures: a fused kernel's line of geometry from its table entry.
Form = collections.namedtuple('Form', 'apps title dims size figures')
FORMS = dict(
    far_lanes=Form(
        'FAR_LANES_APPS', 'Far-lane fused 2-D kernels',
        lambda args, elem: SIZES_2D[elem], lambda dims: ' x '.join(map(str, dims)),
        lambda k: 'period %2d, halo %d/%d, %3d columns out' % (
            k['period'], k['halo'][0], k['halo'][1], k['w_out'])),
    far_taps=Form(
        'FAR_TAPS_APPS', 'Far-tap fused 1-D kernels',
        lambda args, elem: (args.cells,), lambda dims: '%d cells' % dims,
        lambda k: '%d cells per lane, halo %d/%d, %3d of %3d cells out' % (
            k['cols'], k['halo'][0], k['halo'][1], k['w_out'], 64 * k['cols'])))


def judge(times):
  """The figures and the verdict of every schedule from its timed rounds, {schedule: [ms]}
  with the per-stage series under BASELINE: {schedule: dict(ms, min_ms, max_ms, speedup,
  spread, verdict)}.  ms is the median; the spread is the larger max - min of the schedule's
  series and the per-stage one; a schedule is FASTER or SLOWER than per-stage only if the
  medians differ by MORE than the spread.  The per-stage row has no verdict."""
  base = times[BASELINE]
  base_ms = statistics.median(base)
  rows = {}
  for name, series in times.items():
    ms, lo, hi = statistics.median(series), min(series), max(series)
    spread = max(hi - lo, max(base) - min(base))
    verdict = '' if name == BASELINE else (
        'FASTER' if base_ms - ms > spread else
        'SLOWER' if ms - base_ms > spread else 'NO DIFFERENCE beyond the spread')
    rows[name] = dict(ms=ms, min_ms=lo, max_ms=hi, speedup=base_ms / ms, spread=spread,
                      verdict=verdict)
  return rows


def main():
  ap = argparse.ArgumentParser(description=__doc__,
                               formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--switch', required=True, choices=sorted(FORMS),
                  help='the switch of kernel.generate whose kernels are timed')
  ap.add_argument('--apps', nargs='+', default=None,
                  help="default: the switch's samples (far_lanes: star2d dstar2d skewfar2d "
                  'acoustic2d; far_taps: lowpass1d dfir1d skewfir1d acoustic1d)')
  ap.add_argument('--cols', type=int, default=None,
                  help='also time the fused depths with this many cells per lane')
  ap.add_argument('--blob-dir', default=None,
                  help='where the code objects of --cols are kept (default: a temporary one)')
  ap.add_argument('--cells', type=int, default=1 << 27, help='cells of the 1-D array')
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
  form, on = FORMS[args.switch], {args.switch: True}
  apps = args.apps or list(getattr(entry, form.apps))
  iterate = args.iterate
  blob_dir = args.blob_dir or tempfile.mkdtemp()
  lines = [
      '%s (kernel.generate: %s) against the per-stage schedule of' % (form.title, args.switch),
      'the same code object.  tools/far/far_bench.py: outputs of every schedule compared bit for',
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
    limit, _ = switches.depth_limit_of(spec, on)
    default = 'limit %d' % limit if limit else 'default'
    # (label suffix, code object, table): the shipped blob, and the one of --cols
    variants = [('', entry.blob_path(app, **on), kernel.generate(spec, **on)[1])]
    if args.cols:
      text, table = kernel.generate(spec, cols=args.cols, **on)
      path = os.path.join(blob_dir, '%s%s.c%d.hsaco' % (app, switches.blob_suffix(on), args.cols))
      if not os.path.exists(path):
        os.makedirs(blob_dir, exist_ok=True)
        kernel.compile_to_code_object(text, path)
      variants.append((' c%d' % args.cols, path, table))
    progs = []
    for _, blob, table in variants:
      fused = [k for k in table if k['kind'] == 'fused']
      assert fused and all(iterate % k['depth'] == 0 for k in fused), (app, iterate)
      prog = host.open_program(blob=blob, spec=spec)
      assert prog.kernels == table, blob
      progs.append(prog)
    stage_names = [e['name'] for e in variants[0][2] if e['kind'] == 'stage']
    dims = form.dims(args, specmod.ELEM_SIZE[spec['inputs'][0]['c_type']])
    shape = tuple(reversed(dims))
    rng = np.random.default_rng(7)
    n_cells = int(np.prod(shape))
    din = [host.DeviceArray(n_cells * dt.itemsize) for dt in progs[0].in_dtypes]
    dout = [host.DeviceArray(n_cells * dt.itemsize) for dt in progs[0].out_dtypes]
    for d, dt in zip(din, progs[0].in_dtypes):
      a = rng.random(shape, dtype=np.float32)
      d.upload(a.astype(dt))
      del a
    pin, pout = [d.ptr for d in din], [d.ptr for d in dout]
    # (name, program, depth limit, fixed split, the entry every launch is held to)
    schedules = [(default, progs[0], limit, None, None)]
    for (suffix, _, table), prog in zip(variants, progs):
      schedules += [('depth %d%s' % (k['depth'], suffix), prog, limit,
                     [k['depth']] * (iterate // k['depth']), k)
                    for k in table if k['kind'] == 'fused']
    schedules.append((BASELINE, progs[0], -1, None, None))
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
      boxes.append(tuple(slice(-lo[d], dims[d] - hi[d]) for d in reversed(range(len(dims)))))
    reference, same = None, {}
    for name, prog, depth_limit, split, _ in reversed(schedules):
      for d in dout:
        d.zero()
      run(name, prog, depth_limit, split, 1)
      got = [np.ascontiguousarray(d.download(shape, dt)[sl])
             for d, dt, sl in zip(dout, prog.out_dtypes, boxes)]
      if reference is None:
        reference = got
      same[name] = all(np.array_equal(g.view(np.uint8), r.view(np.uint8))
                       for g, r in zip(got, reference))
      del got
    del reference
    assert launches[BASELINE] == stage_names * iterate, launches[BASELINE][:8]
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
    rows = judge(times)
    lines.append('%s %s x %d, %d timed rounds of %d sweeps each; outputs of all schedules '
                 'bit-identical on every box' % (app, form.size(dims), iterate, args.sweeps,
                                                 args.repeats))
    lines.append('  schedule     ms per sweep: median  min .. max      launches  us per launch  '
                 'us per iteration  Gcell/s  TB/s alg.  against per-stage')
    record = dict(app=app, dims=list(dims), iterate=iterate,
                  ms={name: row['ms'] for name, row in rows.items()}, schedules={})
    for name, row in rows.items():
      ms, n = row['ms'], len(launches[name])
      lines.append('  %-10s %12.3f  %10.3f .. %-10.3f %6d  %13.1f  %16.1f  %7.1f  %9.2f  %s' % (
          name, ms, row['min_ms'], row['max_ms'], n, ms * 1e3 / n, ms * 1e3 / iterate,
          updates / (ms * 1e-3) / 1e9, alg * updates / (ms * 1e-3) / 1e12,
          '' if name == BASELINE else '%.2f x, %s (spread %.3f ms)' % (
              row['speedup'], row['verdict'], row['spread'])))
      record['schedules'][name] = dict(ms=ms, min_ms=row['min_ms'], max_ms=row['max_ms'],
                                       launches=n, speedup=row['speedup'],
                                       verdict=row['verdict'])
    lines.append('  %s schedule: %s' % (default, ' '.join(
        '%d x %s' % (launches[default].count(n), n) for n in sorted(set(launches[default])))))
    for suffix, blob, table in variants:
      for k in table:
        if k['kind'] != 'fused':
          continue
        f = static_figures(blob, k['name'])
        lines.append('  %-22s %s; %s' % (
            k['name'] + suffix, form.figures(k),
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
