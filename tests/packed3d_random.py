"""What the two test files on the random programs of the packed-cell 3-D kernels share
(tests/test_packed3d_random_codegen.py, tests/test_gpu_packed3d_random.py): the committed texts
(tests/golden/packed3d_random_programs.json, written by `random_programs.py --narrow-volumes`),
the reference's manifest, and ONE map from a program to generate()'s keywords, so that the
kernels whose text and resources the CPU test pins are the kernels the GPU test runs."""
import json
import os

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod

from conftest import GOLDEN

FAMILY = 'packed3d_random'
with open(os.path.join(GOLDEN, FAMILY + '_programs.json')) as f:
  PROGRAMS = json.load(f)
with open(os.path.join(GOLDEN, FAMILY + '_manifest.json')) as f:
  MANIFEST = json.load(f)
KEYS = sorted(PROGRAMS, key=lambda k: int(k[2:]))
# {program: fixture file} of the programs the reference's loops have an answer for
FIXTURES = {v['key']: k for k, v in MANIFEST.items() if k.endswith('.npz')}
SEAM_MARGIN = 40      # columns a fixture's grid is wider than one tile's stored columns


def keywords_of(key):
  """generate()'s keywords for program `key`: the switch and what the JSON records."""
  return dict(PROGRAMS[key]['generate'], packed_cells=True)


def spec_of(key):
  return specmod.spec_from_stencil(frontend.loads(PROGRAMS[key]['text']))


_GENERATED = {}


def generated(key):
  """(kernel text, table) of program `key` under keywords_of."""
  if key not in _GENERATED:
    _GENERATED[key] = kernel.generate(spec_of(key), **keywords_of(key))
  return _GENERATED[key]


def fused_of(table):
  return [k for k in table if k['kind'] == 'fused']


def lane_bytes(spec, k):
  """Bytes of the vector a lane loads and stores per row in the fused entry `k`."""
  return k['cols'] * specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
