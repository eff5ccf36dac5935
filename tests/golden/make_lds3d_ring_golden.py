#!/usr/bin/env python3
"""Golden fixtures for the 3-D samples with mixed z terms (tests/samples/extra: cross3d,
skewcross3d, coupled3d) from the REAL reference, by make_golden.py's recipe and with its
functions, as make_lds3d_golden.py does for the high-order stars: the reference reads the
program, emits its host, the CPU loops are cut out and compiled with g++ at -O0 and at
-O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_lds3d_ring_golden.py       (the interpreter of make_golden.py)

The grids are make_lds3d_golden.py's, (41, 19, 18) and (23, 27, 21) as (x, y, z): a radius-4
window iterated twice needs 17 cells per side.  iterate 1 and 2, ramp and seeded-random
inputs.  Writes lds3d_ring/*.npz and lds3d_ring_manifest.json: 24 fixtures.  Only DATA
produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = (('cross3d', (1, 2)), ('skewcross3d', (1, 2)), ('coupled3d', (1, 2)))
CASES = ((41, 19, 18), (23, 27, 21))
OUT = os.path.join(mg.HERE, 'lds3d_ring')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'lds3d_ring_manifest.json'),
                  APPS, CASES)
