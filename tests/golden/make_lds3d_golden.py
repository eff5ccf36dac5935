#!/opt/conda/bin/python3.9
"""Golden fixtures for the high-order 3-D samples (tests/samples/extra: star3d, iso3dfd,
skewstar3d) from the REAL reference, by make_golden.py's recipe and with its functions:
the reference reads the program, emits its host, the CPU loops are cut out and compiled
with g++ at -O0 and at -O2 -ffp-contract=off (both must agree).

    /opt/conda/bin/python3.9 tests/golden/make_lds3d_golden.py

make_golden.CASES_3D is too small for a radius-4 window iterated twice (17 cells per side
at least): the grids here are (41, 19, 18) and (23, 27, 21) as (x, y, z).  iterate 1 and 2
(iso3dfd, one pass over three inputs: 1), ramp and seeded-random inputs.  Writes
lds3d/*.npz and lds3d_manifest.json.  Only DATA produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = (('star3d', (1, 2)), ('iso3dfd', (1,)), ('skewstar3d', (1, 2)))
CASES = ((41, 19, 18), (23, 27, 21))
OUT = os.path.join(mg.HERE, 'lds3d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'lds3d_manifest.json'),
                  APPS, CASES)
