#!/usr/bin/env python3
"""Golden fixtures for the 2-D samples that read beyond the neighbour lane (tests/samples/extra:
star2d, dstar2d, skewfar2d, acoustic2d) from the REAL reference, by make_golden.py's recipe
and with its functions, as make_lds3d_ring_golden.py does for the 3-D plane-ring samples: the
reference reads the program, emits its host, the CPU loops are cut out and compiled with g++
at -O0 and at -O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_far2d_golden.py       (the interpreter of make_golden.py)

Two grids per case, (x, y): (301, 53), wider than the 240 columns a float strip stores at
most, so a strip seam lies inside every valid box, and the small odd (71, 57).  The largest
composed window, star2d's radius 8 iterated three times, takes 24 cells per side: every
output box keeps at least 5 cells each way.  Ramp and seeded-random inputs.  Writes
far2d/*.npz and far2d_manifest.json: 44 fixtures.  Only DATA produced by the reference is
committed.
"""
import hashlib
import json
import os
import tempfile

import numpy as np

import make_golden as mg

APPS = (('star2d', (1, 2, 3)), ('dstar2d', (1, 2, 4)), ('skewfar2d', (1, 2)),
        ('acoustic2d', (1, 2, 3)))
CASES = ((301, 53), (71, 57))
OUT = os.path.join(mg.HERE, 'far2d')


def main():
  os.makedirs(OUT, exist_ok=True)
  manifest = {}
  with tempfile.TemporaryDirectory() as wd:
    for app, iterations in APPS:
      path = os.path.join(mg.EXTRA, app + '.soda')
      for it in iterations:
        st = mg.build_stencil(path, iterate=it)
        _, text = mg.analysis_of(st)
        key = '%s.iter%d' % (app, it)
        for dims in CASES:
          for kind in ('ramp', 'random'):
            inputs = mg.make_inputs(st, dims, kind, np.random.default_rng(mg.SEED))
            r0 = mg.run_reference(st, text, dims, inputs, '-O0', wd)
            r2 = mg.run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
            outs = {n: r0[n] for n in st.output_names}
            for name in outs:
              if not np.array_equal(r0[name], r2[name], equal_nan=True):
                raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
            fx = '%s.%s.%s.npz' % (key, 'x'.join(map(str, dims)), kind)
            payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
            payload.update({'out_' + n: a for n, a in outs.items()})
            np.savez_compressed(os.path.join(OUT, fx), **payload)
            manifest[fx] = dict(key=key, dims=list(dims), kind=kind, iterate=it,
                                sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                        for n, a in outs.items()})
            print('wrote', fx)
  with open(os.path.join(mg.HERE, 'far2d_manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
  main()
