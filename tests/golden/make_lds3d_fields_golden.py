#!/opt/conda/bin/python3.9
"""Golden fixtures for the high-order 3-D samples with several outputs (tests/samples/extra:
acoustic3d, skewwave3d, deriv3d) from the REAL reference, by make_lds3d_golden.py's recipe
and with make_golden.py's functions: the reference reads the program, emits its host, the
CPU loops are cut out and compiled with g++ at -O0 and at -O2 -ffp-contract=off (both must
agree).

    /opt/conda/bin/python3.9 tests/golden/make_lds3d_fields_golden.py

Grids (41, 19, 18) and (23, 27, 21) as (x, y, z), ramp and seeded-random inputs.  iterate 1
and 2 for acoustic3d and skewwave3d (iterate 3 of skewwave3d no longer fits 23 columns), 1
for deriv3d, one pass.  Writes lds3d_fields/*.npz and lds3d_fields_manifest.json.  Only
DATA produced by the reference is committed.
"""
import hashlib
import json
import os
import tempfile

import numpy as np

import make_golden as mg

APPS = (('acoustic3d', (1, 2)), ('skewwave3d', (1, 2)), ('deriv3d', (1,)))
CASES = ((41, 19, 18), (23, 27, 21))
OUT = os.path.join(mg.HERE, 'lds3d_fields')


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
  with open(os.path.join(mg.HERE, 'lds3d_fields_manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
  main()
