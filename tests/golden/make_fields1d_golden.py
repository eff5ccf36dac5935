#!/opt/conda/bin/python3.9
"""Golden fixtures for the 1-D samples over several fields (tests/samples/extra: wave1d,
skewpair1d, fdtd1d, mixpair1d; output j feeds input j when iterating) from the REAL
reference, by make_golden.py's recipe and with its functions: the reference reads the
program, emits its host, the CPU loops are cut out and compiled with g++ at -O0 and at
-O2 -ffp-contract=off (both must agree).

    /opt/conda/bin/python3.9 tests/golden/make_fields1d_golden.py

iterate 1..4, ramp and seeded-random inputs, lengths 37 and 300.  Writes fields1d/*.npz
and fields1d_manifest.json.  Where the reference does not get that far with a 1-D program
- its analysis or its host printer raises, or the emitted loops do not compile - the
manifest records the step and the error instead (the way extra_manifest.json records
outchain), and no fixture exists for that case.
Only DATA produced by the reference is committed.
"""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

import make_golden as mg

APPS = ('wave1d', 'skewpair1d', 'fdtd1d', 'mixpair1d')
LENGTHS = ((37,), (300,))
OUT = os.path.join(mg.HERE, 'fields1d')


def main():
  manifest = {}
  with tempfile.TemporaryDirectory() as wd:
    for app in APPS:
      path = os.path.join(mg.EXTRA, app + '.soda')
      for it in (1, 2, 3, 4):
        key = '%s.iter%d' % (app, it)
        try:
          st = mg.build_stencil(path, iterate=it)
          ana, text = mg.analysis_of(st)
        except Exception as e:      # the reference itself does not take the program
          manifest['fields1d.' + key] = dict(
              key=key, reference_cpu_path='the reference raises %s: %s' % (
                  type(e).__name__, str(e)[:200]))
          print(key, ': the reference raises', type(e).__name__, e)
          continue
        for dims in LENGTHS:
          for kind in ('ramp', 'random'):
            inputs = mg.make_inputs(st, dims, kind, np.random.default_rng(mg.SEED))
            try:
              r0 = mg.run_reference(st, text, dims, inputs, '-O0', wd)
              r2 = mg.run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
            except subprocess.CalledProcessError:
              manifest['fields1d.' + key] = dict(key=key, reference_cpu_path='does not compile')
              print(key, ': the reference\'s emitted CPU loops do not compile')
              break
            outs = {n: r0[n] for n in st.output_names}
            for name in outs:
              if not np.array_equal(r0[name], r2[name], equal_nan=True):
                raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
            fx = '%s.%s.%s.npz' % (key, 'x'.join(map(str, dims)), kind)
            payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
            payload.update({'out_' + n: a for n, a in outs.items()})
            os.makedirs(OUT, exist_ok=True)
            np.savez_compressed(os.path.join(OUT, fx), **payload)
            manifest[fx] = dict(key=key, dims=list(dims), kind=kind, iterate=it,
                                sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                        for n, a in outs.items()})
            print('wrote', fx)
          else:
            continue
          break
  with open(os.path.join(mg.HERE, 'fields1d_manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
  main()
