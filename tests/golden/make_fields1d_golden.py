#!/opt/conda/bin/python3.9
"""Golden fixtures for the 1-D samples over several fields (tests/samples/extra: wave1d,
skewpair1d, fdtd1d, mixpair1d; output j feeds input j when iterating) from the REAL
reference, by make_golden.py's recipe and with its functions: the reference reads the
program, emits its host, the CPU loops are cut out and compiled with g++ at -O0 and at
-O2 -ffp-contract=off (both must agree).

    /opt/conda/bin/python3.9 tests/golden/make_fields1d_golden.py

iterate 1..4, ramp and seeded-random inputs, lengths 37 and 300.  Writes fields1d/*.npz
and fields1d_manifest.json.  Where the reference does not get that far with a 1-D program
- its analysis or its host printer raises, or the emitted loops do not compile - the
manifest records the step and the error instead (the way extra_manifest.json records
outchain), and no fixture exists for that case.
Only DATA produced by the reference is committed.
"""
import os

import make_golden as mg

APPS = tuple((app, (1, 2, 3, 4)) for app in ('wave1d', 'skewpair1d', 'fdtd1d', 'mixpair1d'))
LENGTHS = ((37,), (300,))
OUT = os.path.join(mg.HERE, 'fields1d')

if __name__ == '__main__':
  mg.write_family(OUT, os.path.join(mg.HERE, 'fields1d_manifest.json'),
                  APPS, LENGTHS, refusal_prefix='fields1d',
                  refusals=('raises', 'compile'))
