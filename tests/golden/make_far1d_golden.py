#!/usr/bin/env python3
"""Golden fixtures for the 1-D samples that read beyond the neighbour lane (tests/samples/extra:
lowpass1d, dfir1d, skewfir1d, acoustic1d) from the REAL reference, by make_golden.py's recipe
and with its functions, as make_far2d_golden.py does for the 2-D far-lane samples: the
reference reads the program, emits its host, the CPU loops are cut out and compiled with g++
at -O0 and at -O2 -ffp-contract=off (both must agree).

    python3 tests/golden/make_far1d_golden.py       (the interpreter of make_golden.py)

Two lengths per case: 701, wider than the 224 cells a float segment stores at most, so a
segment seam lies inside every valid box, and 157.  The largest composed window, lowpass1d's
radius 16 iterated four times, takes 64 cells per side: 157 leaves a box of 29 cells.  Ramp
and seeded-random inputs.  Writes far1d/*.npz and far1d_manifest.json: 48 fixtures.  Only
DATA produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = (('lowpass1d', (1, 2, 3, 4)), ('dfir1d', (1, 2, 4)), ('skewfir1d', (1, 2)),
        ('acoustic1d', (1, 2, 3)))
LENGTHS = ((701,), (157,))
OUT = os.path.join(mg.HERE, 'far1d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'far1d_manifest.json'),
                  APPS, LENGTHS)
