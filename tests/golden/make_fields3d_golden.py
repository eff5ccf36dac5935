#!/opt/conda/bin/python3.9
"""Golden fixtures for the 3-D multi-field samples (tests/samples/extra: wave3d,
maxwell3d) from the REAL reference, by make_golden.py's recipe and with its
functions: the reference reads the program, emits its host, the CPU loops are cut out
and compiled with g++ at -O0 and at -O2 -ffp-contract=off (both must agree).

    /opt/conda/bin/python3.9 tests/golden/make_fields3d_golden.py

iterate 1..3, ramp and seeded-random inputs, the grids of make_golden.CASES_3D.  Writes
fields3d/*.npz and fields3d_manifest.json.  A program in which an output is read by another
stage has no self-contained reference answer (the emitted loops read the device's array
there, make_golden.py: main_extra); it is recorded as such in the manifest.
Only DATA produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = tuple((app, (1, 2, 3)) for app in ('wave3d', 'maxwell3d'))
OUT = os.path.join(mg.HERE, 'fields3d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'fields3d_manifest.json'),
                  APPS, mg.CASES_3D, refusal_prefix='fields3d',
                  refusals=('fed_back', 'compile'))
