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
import os

import make_golden as mg

APPS = (('acoustic3d', (1, 2)), ('skewwave3d', (1, 2)), ('deriv3d', (1,)))
CASES = ((41, 19, 18), (23, 27, 21))
OUT = os.path.join(mg.HERE, 'lds3d_fields')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'lds3d_fields_manifest.json'),
                  APPS, CASES)
