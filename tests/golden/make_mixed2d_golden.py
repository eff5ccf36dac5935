#!/usr/bin/env python3
"""Golden fixtures for the 2-D samples whose inputs and output differ in element width
(tests/samples/extra: edge8f, tone16, quant2d, dsum2d) and for mask2d, two inputs of one width
and different types, from the REAL reference, by make_golden.py's recipe and with its
functions, as make_far2d_golden.py does for the far-lane samples: the reference reads the
program, emits its host, the CPU loops are cut out and compiled with g++ at -O0 and at
-O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_mixed2d_golden.py       (the interpreter of make_golden.py)

Three grids per case, (x, y): (301, 53) and the small odd (71, 57), and (1100, 11): a strip of
the mixed-width kernels stores up to 1024 columns (16 columns per lane where the narrowest
element fills the lane's 16 bytes), so only the third puts a strip seam inside every valid box
whatever the lane shape.  The largest window, tone16's, takes 2 cells per side: every output
box keeps at least 8 cells each way.  Ramp and seeded-random inputs.  Writes mixed2d/*.npz and
mixed2d_manifest.json: 30 fixtures.  Only DATA produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = (('edge8f', (1,)), ('tone16', (1,)), ('quant2d', (1,)), ('dsum2d', (1,)),
        ('mask2d', (1,)))
CASES = ((301, 53), (71, 57), (1100, 11))
OUT = os.path.join(mg.HERE, 'mixed2d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'mixed2d_manifest.json'),
                  APPS, CASES)
