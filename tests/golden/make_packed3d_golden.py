#!/usr/bin/env python3
"""Golden fixtures for the 3-D samples over 8- and 16-bit volumes (tests/samples/extra:
smooth3d, skewvol3d, sdiff3d, castvol3d) from the REAL reference, by make_golden.py's recipe
and with its functions, as make_far2d_golden.py does for the far-lane 2-D samples: the
reference reads the program, emits its host, the CPU loops are cut out and compiled with g++
at -O0 and at -O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_packed3d_golden.py       (the interpreter of make_golden.py)

Two grids per case, (x, y, z): (600, 11, 7), wider than the 496 columns a packed-cell tile
stores at most (uint8 in 8-column lanes; 248 for the uint16 samples), so a tile seam lies
inside every valid box, with few rows and planes; and the small odd (37, 13, 9).  The largest
composed window, smooth3d's radius 1 iterated three times, takes 3 cells per side: every
output box keeps at least one plane.  Ramp and seeded-random inputs.  The reference's host
compiles all four element types (uint16, uint8, int16, and the float local of castvol3d): no
type was replaced.  Writes packed3d/*.npz and packed3d_manifest.json: 24 fixtures.  Only DATA
produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = (('smooth3d', (1, 2, 3)), ('skewvol3d', (1,)), ('sdiff3d', (1,)), ('castvol3d', (1,)))
CASES = ((600, 11, 7), (37, 13, 9))
OUT = os.path.join(mg.HERE, 'packed3d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'packed3d_manifest.json'),
                  APPS, CASES)
