#!/usr/bin/env python3
"""Golden fixtures for the random programs of the fused 1-D kernels (tests/random_programs.py:
line_program; texts, iteration counts and lengths in random1d_programs.json) from the REAL
reference, by make_golden.py's recipe and with its functions, in main_random's pattern: the
reference reads the program text, emits its host, the CPU loops are cut out and compiled with
g++ at -O0 and at -O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_random1d_golden.py       (the interpreter of make_golden.py)

One length per program, recorded with the text: the cells the widest segment of the kernels
under test stores, plus what the box of all iterations is shorter than the array, plus 40, so
a segment seam of every kernel lies inside the output's box.  Inputs are seeded: 16-bit
integers uniform over the WHOLE range of the type, 32- and 64-bit integers within +-2^20
(where no sum or product of the generator leaves the type), floats in (-2, 2) with both
signs.  A program with a window that excludes the store point gets a manifest row that says
so instead of a fixture: the emitted loops leave the arrays there.  Writes random1d/*.npz and
random1d_manifest.json.  Only DATA produced by the reference is committed.
"""
import hashlib
import json
import os
import tempfile

import numpy as np

import make_golden as mg

FAMILY = 'random1d'
OUT = os.path.join(mg.HERE, FAMILY)


def inputs_of(st, dims, rng):
  out = []
  for htype in st.input_types:
    dt = np.dtype(mg.NP_TYPES[mg.hutil.get_c_type(htype)])
    shape = tuple(reversed(dims))
    if dt.kind == 'f':
      out.append(((rng.random(shape) * 4.0 - 2.0).astype(np.float32)).astype(dt))
    elif dt.itemsize == 2:
      info = np.iinfo(dt)
      out.append(rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True))
    else:
      lo = 0 if dt.kind == 'u' else -(1 << 20)
      out.append(rng.integers(lo, 1 << 20, size=shape, dtype=dt, endpoint=True))
  return out


def main():
  with open(os.path.join(mg.HERE, FAMILY + '_programs.json')) as f:
    programs = json.load(f)
  manifest = {}
  with tempfile.TemporaryDirectory() as wd:
    for key in sorted(programs):
      entry = programs[key]
      st = mg.build_stencil(None, text=entry['text'])
      ana, text = mg.analysis_of(st)
      assert st.iterate == entry['iterate'] and st.dim == 1
      if any(min(t['loop_lo'] + t['loop_hi_margin']) < 0 for t in ana['stages']):
        manifest['%s.%s' % (FAMILY, key)] = dict(
            key=key, reference_cpu_path='one-sided window: loops leave the arrays')
        print(key, ': one-sided window, no defined reference answer')
        continue
      dims = tuple(entry['grid'])
      inputs = inputs_of(st, dims, np.random.default_rng(mg.SEED))
      st.app_name = '%s_%s' % (st.app_name, FAMILY)     # a harness tag of its own
      r0 = mg.run_reference(st, text, dims, inputs, '-O0', wd)
      r2 = mg.run_reference(st, text, dims, inputs, '-O2 -ffp-contract=off', wd)
      outs = {n: r0[n] for n in st.output_names}
      for name in outs:
        if r0[name].tobytes() != r2[name].tobytes():
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
