#!/usr/bin/env python3
"""Golden fixtures for the random programs of the packed-cell 3-D kernels (tests/
random_programs.py: narrow_volume_program; texts, iteration counts and grids in
packed3d_random_programs.json) from the REAL reference, by make_golden.py's recipe and with its
functions, in main_random's pattern: the reference reads the program text, emits its host, the
CPU loops are cut out and compiled with g++ at -O0 and at -O2 -ffp-contract=off (both must
agree).

    python3 tests/golden/make_packed3d_random_golden.py       (the interpreter of make_golden.py)

One grid per program, (x, y, z), recorded with the text: 40 columns wider than one tile of the
kernel under test stores, so a tile seam lies inside the output's box, by 11 rows and 7 planes
(9 and 5 for the widest two-input programs: every file stays under 200 KB).  Inputs are seeded
and uniform over the WHOLE range of the element type, negative values included.  A program
with a window that excludes the store point gets a manifest row that says so instead of a
fixture: the emitted loops leave the arrays there.  Writes packed3d_random/*.npz and
packed3d_random_manifest.json.  Only DATA produced by the reference is committed.
"""
import hashlib
import json
import os
import tempfile

import numpy as np

import make_golden as mg

FAMILY = 'packed3d_random'
OUT = os.path.join(mg.HERE, FAMILY)


def main():
  with open(os.path.join(mg.HERE, FAMILY + '_programs.json')) as f:
    programs = json.load(f)
  manifest = {}
  with tempfile.TemporaryDirectory() as wd:
    for key in sorted(programs):
      entry = programs[key]
      st = mg.build_stencil(None, text=entry['text'])
      ana, text = mg.analysis_of(st)
      assert st.iterate == entry['iterate'] and st.dim == 3
      if any(min(t['loop_lo'] + t['loop_hi_margin']) < 0 for t in ana['stages']):
        manifest['%s.%s' % (FAMILY, key)] = dict(
            key=key, reference_cpu_path='one-sided window: loops leave the arrays')
        print(key, ': one-sided window, no defined reference answer')
        continue
      dims = tuple(entry['grid'])
      rng = np.random.default_rng(mg.SEED)
      inputs = []
      for htype in st.input_types:
        dt = np.dtype(mg.NP_TYPES[mg.hutil.get_c_type(htype)])
        assert dt.kind in 'iu' and dt.itemsize <= 2
        info = np.iinfo(dt)
        inputs.append(rng.integers(info.min, info.max, size=tuple(reversed(dims)), dtype=dt,
                                   endpoint=True))
      st.app_name = '%s_%s' % (st.app_name, FAMILY)     # a harness tag of its own
      r0 = mg.run_reference(st, text, dims, inputs, '-O0', wd)
      r2 = mg.run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
      outs = {n: r0[n] for n in st.output_names}
      for name in outs:
        if not np.array_equal(r0[name], r2[name]):
          raise SystemExit('O0/O2 disagree: %s %s' % (key, name))
      fx = '%s.npz' % key
      payload = {'in_' + n: a for n, a in zip(st.input_names, inputs)}
      payload.update({'out_' + n: a for n, a in outs.items()})
      os.makedirs(OUT, exist_ok=True)
      np.savez_compressed(os.path.join(OUT, fx), **payload)
      manifest[fx] = dict(key=key, dims=list(dims), iterate=st.iterate,
                          sha256={n: hashlib.sha256(a.tobytes()).hexdigest()
                                  for n, a in outs.items()})
      print('wrote', fx, os.path.getsize(os.path.join(OUT, fx)))
  with open(os.path.join(mg.HERE, FAMILY + '_manifest.json'), 'w') as f:
    json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == '__main__':
  main()
