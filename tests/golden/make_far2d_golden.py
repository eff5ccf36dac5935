#!/usr/bin/env python3
"""Golden fixtures for the 2-D samples that read beyond the neighbour lane (tests/samples/extra:
star2d, dstar2d, skewfar2d, acoustic2d) from the REAL reference, by make_golden.py's recipe
and with its functions, as make_lds3d_ring_golden.py does for the 3-D plane-ring samples: the
reference reads the program, emits its host, the CPU loops are cut out and compiled with g++
at -O0 and at -O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_far2d_golden.py       (the interpreter of make_golden.py)

Two grids per case, (x, y): (301, 53), wider than the 240 columns a float strip stores at
most, so a strip seam lies inside every valid box, and the small odd (71, 57).  The largest
composed window, star2d's radius 8 iterated three times, takes 24 cells per side: every
output box keeps at least 5 cells each way.  Ramp and seeded-random inputs.  Writes
far2d/*.npz and far2d_manifest.json: 44 fixtures.  Only DATA produced by the reference is
committed.
"""
import os

import make_golden as mg

APPS = (('star2d', (1, 2, 3)), ('dstar2d', (1, 2, 4)), ('skewfar2d', (1, 2)),
        ('acoustic2d', (1, 2, 3)))
CASES = ((301, 53), (71, 57))
OUT = os.path.join(mg.HERE, 'far2d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'far2d_manifest.json'),
                  APPS, CASES)
