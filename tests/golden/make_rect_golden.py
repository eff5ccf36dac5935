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
import os

import make_golden as mg

APPS = tuple((app, (1,)) for app in ('grad2d', 'blend2d', 'grad3d', 'mix3d'))
OUT = os.path.join(mg.HERE, 'rect')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(OUT, 'manifest.json'),
                  APPS, lambda st: mg.CASES_2D if st.dim == 2 else mg.CASES_3D,
                  refusal_prefix='rect', refusals=('fed_back', 'compile'))
