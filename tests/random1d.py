"""What the two test files on the random programs of the fused 1-D kernels share
(tests/test_random1d_codegen.py, tests/test_gpu_random1d.py): the committed texts
(tests/golden/random1d_programs.json, written by `random_programs.py --lines`), the reference's
manifest, and ONE map from a program to generate()'s keywords, so that the kernels whose text
and resources the CPU test pins are the kernels the GPU test runs; and, without a GPU, what the
GPU test runs them on: the lengths from an entry's constants, the splits of an iteration count
over a table with gaps, the subsets of its parts (d) and (e), the full-width inputs."""
import json
import os

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod

from conftest import GOLDEN
from switch_form_gpu import line_lengths as lengths, splits_of      # noqa: F401

FAMILY = 'random1d'
with open(os.path.join(GOLDEN, FAMILY + '_programs.json')) as f:
  PROGRAMS = json.load(f)
with open(os.path.join(GOLDEN, FAMILY + '_manifest.json')) as f:
  MANIFEST = json.load(f)
KEYS = sorted(PROGRAMS, key=lambda k: int(k[2:]))
# {program: fixture file} of the programs the reference's loops have an answer for
FIXTURES = {v['key']: k for k, v in MANIFEST.items() if k.endswith('.npz')}
SEAM_MARGIN = 40      # cells a fixture is longer than the widest segment's and the box's
MAX_CELLS = 25000     # the longest array of the GPU test: three tiles and 17 cells


def keywords_of(key):
  """generate()'s keywords for program `key`: what the JSON records, the switch included."""
  return dict(PROGRAMS[key]['generate'])


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


def margin_of(spec, iterate):
  """Cells the box of `iterate` iterations is shorter than the array."""
  lo, hi = specmod.iteration_boxes(spec, iterate)[-1][spec['outputs'][0]]
  return hi[0] - lo[0]


def edge_of(spec):
  """'first' / 'last': the output's box starts on the array's first element / ends on its
  last one, whatever the iteration count."""
  lo, hi = specmod.iteration_margins(spec, 1)[-1]
  return None if lo[0] and hi[0] else ('last' if lo[0] else 'first')


def refused_depths(key):
  """The depths of the family's list within `iterate` that the table of `key` lacks."""
  have = {k['depth'] for k in fused_of(generated(key)[1])}
  return [d for d in kernel.STREAM1D_DEPTHS if d <= PROGRAMS[key]['iterate'] and d not in have]


def hops_of(key):
  """Lanes the farthest read of program `key` lies away, per side (lo, hi)."""
  cols = fused_of(generated(key)[1])[0]['cols']
  offsets = [rel[0] for stage in spec_of(key)['stages'] for _, rel in stage['loads']]
  return (max([0] + [-(-(-o) // cols) for o in offsets if o < 0]),
          max([0] + [-(-o // cols) for o in offsets if o > 0]))


def lane_class(key):
  """(element size, bytes of a lane) of program `key`."""
  spec = spec_of(key)
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  return elem, elem * fused_of(generated(key)[1])[0]['cols']


def reads_far_local(key):
  """A stage reads a computed level beyond the neighbour lane."""
  spec = spec_of(key)
  cols = fused_of(generated(key)[1])[0]['cols']
  inputs = {t['name'] for t in spec['inputs']}
  return any(name not in inputs and abs(rel[0]) > cols
             for stage in spec['stages'] for name, rel in stage['loads'])


def guarded(key):
  """The programs of part (d) of the GPU test: every head and every tail program, the first
  program (in the set's order) of each element size at each lane width, the program with 8
  lanes on either side, and those whose table lacks a depth."""
  first = next(k for k in KEYS if lane_class(k) == lane_class(key))
  return (key == first or edge_of(spec_of(key)) is not None or hops_of(key) == (8, 8) or
          bool(refused_depths(key)))


def resumed(key):
  """The programs of part (e): the first of each element width that iterates at least
  twice, and the first far program with a local that does."""
  def first(cond):
    return next(k for k in KEYS if PROGRAMS[k]['iterate'] >= 2 and cond(k))
  elem = lane_class(key)[0]
  return key in (first(lambda k: lane_class(k)[0] == elem), first(reads_far_local))


def wide_seed(key, n):
  """The seed of gpu_util.wide_inputs for program `key` on `n` cells."""
  return 20240607 + n + int(key[2:])


def wide_lengths(k, m):
  """The lengths of the full-width runs of entry `k`: a segment and a cell, a tile and 35."""
  return (k['w_out'] + m + 1, k['tile'][0] + 35 + m)
