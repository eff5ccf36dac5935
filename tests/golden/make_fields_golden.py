#!/opt/conda/bin/python3.9
"""Golden fixtures for the multi-field samples (tests/samples/extra: wave2d, fdtd2d,
skewpair2d, mixpair2d) from the REAL reference, by make_golden.py's recipe and with its
functions: the reference reads the program, emits its host, the CPU loops are cut out
and compiled with g++ at -O0 and at -O2 -ffp-contract=off (both must agree).

    /opt/conda/bin/python3.9 tests/golden/make_fields_golden.py

iterate 1..4, ramp and seeded-random inputs, grids 37 x 29 and 64 x 48.  Writes
fields/*.npz and fields_manifest.json.  A program in which an output is read by another
stage has no self-contained reference answer (the emitted loops read the device's array
there, make_golden.py: main_extra); it is recorded as such in the manifest.
Only DATA produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = tuple((app, (1, 2, 3, 4)) for app in ('wave2d', 'fdtd2d', 'skewpair2d', 'mixpair2d'))
OUT = os.path.join(mg.HERE, 'fields')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'fields_manifest.json'),
                  APPS, mg.CASES_2D, refusal_prefix='fields',
                  refusals=('fed_back', 'compile'))
