#!/opt/conda/bin/python3.9
"""Golden fixtures for the one-pass samples with several outputs and `#inputs != #outputs`
or outputs of other types than the inputs (tests/samples/extra: grad2d, blend2d, grad3d,
mix3d) from the REAL reference, by make_golden.py's recipe and with its functions: the
reference reads the program, emits its host, the CPU loops are cut out and compiled with
g++ at -O0 and at -O2 -ffp-contract=off (both must agree).

    /opt/conda/bin/python3.9 tests/golden/make_rect_golden.py

iterate 1, ramp and seeded-random inputs, the grids of make_golden.CASES_2D / CASES_3D.
Writes rect/*.npz and rect/manifest.json.  A program in which an output is read by another
stage has no self-contained reference answer (the emitted loops read the device's array
there, make_golden.py: main_extra); it is recorded as such in the manifest.
Only DATA produced by the reference is committed.
"""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

import make_golden as mg

APPS = ('grad2d', 'blend2d', 'grad3d', 'mix3d')
OUT = os.path.join(mg.HERE, 'rect')


def main():
  os.makedirs(OUT, exist_ok=True)
  manifest = {}
  with tempfile.TemporaryDirectory() as wd:
    for app in APPS:
      st = mg.build_stencil(os.path.join(mg.EXTRA, app + '.soda'), iterate=1)
      ana, text = mg.analysis_of(st)
      key = '%s.iter1' % app
      fed_back = [t['name'] for t in ana['stages']
                  if t['name'] in st.output_names and not t['is_output']]
      if fed_back:
        manifest['rect.' + key] = dict(
            key=key, reference_cpu_path='reads the device result of output(s) %s'
            % ', '.join(fed_back))
        print(key, ': output read by another stage, no self-contained reference answer')
        continue
      for dims in (mg.CASES_2D if st.dim == 2 else mg.CASES_3D):
        for kind in ('ramp', 'random'):
          inputs = mg.make_inputs(st, dims, kind, np.random.default_rng(mg.SEED))
          try:
            r0 = mg.run_reference(st, text, dims, inputs, '-O0', wd)
            r2 = mg.run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
          except subprocess.CalledProcessError:
            manifest['rect.' + key] = dict(key=key, reference_cpu_path='does not compile')
            print(key, ': the reference\'s emitted CPU loops do not compile')
            break
          outs = {n: r0[n] for n in st.output_names}
          for name in outs:
            if not np.array_equal(r0[name], r2[name], equal_nan=True):
              raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
          fx = '%s.%s.%s.npz' % (key, 'x'.join(map(str, dims)), kind)
          payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
          payload.update({'out_' + n: a for n, a in outs.items()})
          np.savez_compressed(os.path.join(OUT, fx), **payload)
          manifest[fx] = dict(key=key, dims=list(dims), kind=kind, iterate=1,
                              sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                      for n, a in outs.items()})
          print('wrote', fx)
        else:
          continue
        break
  with open(os.path.join(OUT, 'manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
  main()
