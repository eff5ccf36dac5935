"""Random programs over 8- and 16-bit volumes (tests/random_programs.py:
narrow_volume_program; the texts in tests/golden/packed3d_random_programs.json) through the
packed-cell 3-D kernels (kernel_stream3d_pk; kernel.generate's `packed_cells`) on a real
MI355X, compiled at run time (hiprtc) under the keywords tests/packed3d_random.py maps each
program to - the kernels whose coverage and resources tests/test_packed3d_random_codegen.py
pins: 16-byte lane loads and stores, int8, two inputs, locals of another width, int32 and
float locals, x offsets of a whole lane, one-sided and negative-only windows, programs
without a z reach, and the operators no sample uses.  Every comparison is of bytes:

  (a) the reference's own run of the program (tests/golden/packed3d_random/<key>.npz), whole
      arrays as run_numpy hands them back - the box equals the reference, zero outside it;
  (b) the CPU oracle on shapes from the depth-1 entry's own constants
      (switch_form_gpu.volume_shapes_of): the one-cell box, one tile plus a column and a row
      on the fewest planes, a chunk seam, the ragged 2 x 3 tiles with 29 planes;
  (c) full-width operands (gpu_util.wide_inputs) against the oracle built with -fwrapv, on
      the ragged shape;
  (d) the sweep's memory contract on the ragged shape in guarded arenas, the deepest kernel,
      for the programs on 16-byte lanes, those whose box touches the array's first or last
      element, and the first program of each end type.

(a) - (c) run in the default schedule, limited to depth 1, per stage and - an even iteration
count over a depth-2 kernel - split into launches of depth 2; every launch of a run that is
not per stage is one of the form's fused kernels (prog.schedule)."""
import concurrent.futures
import os

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel, kernel_common
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
import switch_form_gpu as harness
from packed3d_random import (FAMILY, FIXTURES, KEYS, PROGRAMS, SEAM_MARGIN, fused_of, generated,
                             lane_bytes, spec_of)
from test_gpu_memory_contract import hold
from test_gpu_random_programs import PROGRAMS as RANDOM_PROGRAMS, run_case

pytestmark = pytest.mark.gpu

MAX_CELLS = 8 << 20


def edge_of(spec):
  """'first' / 'last': the output's box starts on the array's first element / ends on its
  last one (no offset below / above zero on any axis) - where a store one cell too far
  leaves the array."""
  lo, hi = specmod.iteration_margins(spec, 1)[-1]
  return None if any(lo) and any(hi) else ('last' if any(lo) else 'first')


def guarded(key):
  """The programs of part (d): a fused kernel on 16-byte lanes, a box that touches the
  array's first or last element, or the first program (in the set's order) whose input is
  of its type."""
  spec = spec_of(key)
  end = spec['inputs'][-1]['c_type']
  first = next(k for k in KEYS if spec_of(k)['inputs'][-1]['c_type'] == end)
  return key == first or edge_of(spec) is not None or any(
      lane_bytes(spec, k) == 16 for k in fused_of(generated(key)[1]))


def runs_of(fused, iterate):
  """(max depth, split) of the runs every case is held to."""
  runs = [(0, None), (1, None), (-1, None)]
  if len(fused) == 2 and iterate % 2 == 0:
    runs.append((0, [2] * (iterate // 2)))
  return runs


def check(prog, inputs, want, iterate, what, whole=False):
  """`want` on the output's box in every run of runs_of; whole: on the whole array, which is
  zero outside the box."""
  spec = prog.spec
  (name,) = spec['outputs']
  shape = inputs[0].shape
  dims = tuple(reversed(shape))
  fused = fused_of(prog.kernels)
  names = {k['name'] for k in fused}
  _, _, sl = harness.slices_of(spec, name, shape, iterate)
  assert want[sl].size > 0, (what, shape)
  outside = np.ones(shape, dtype=bool)
  outside[sl] = False
  for max_depth, split in runs_of(fused, iterate):
    said = (spec['app_name'], what, shape, iterate, max_depth, split)
    prog.set_max_depth(max_depth)
    try:
      if split:
        prog.set_split(dims, iterate, split)
      launched = [k for k, _ in prog.schedule(dims, iterate)]
      if max_depth == -1:
        assert all(k['kind'] == 'stage' for k in launched), said
      else:
        # no case passes by running the per-stage kernels
        assert launched and all(k['kind'] == 'fused' and k['name'] in names
                                for k in launched), (said, [k['name'] for k in launched])
        assert sum(k['depth'] for k in launched) == iterate, said
        if max_depth == 1:
          assert all(k['depth'] == 1 for k in launched), said
        if split:
          assert [k['depth'] for k in launched] == split, said
      (got,) = prog.run_numpy(inputs, iterate=iterate)
    finally:
      if split:
        prog.set_split(dims, iterate, [])
      prog.set_max_depth(0)
    assert got.dtype == want.dtype and got.shape == want.shape, said
    differ = np.argwhere(np.ascontiguousarray(got[sl]).view(np.uint8) !=
                         np.ascontiguousarray(want[sl]).view(np.uint8))
    assert differ.size == 0, ('%d bytes of the box differ, first at %s' % (
        len(differ), differ[0]), said, PROGRAMS.get(spec['app_name'], {}).get('text'))
    if whole:
      assert not got[outside].any(), said
      assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), said


@pytest.mark.parametrize('key', KEYS)
def test_random_narrow_volume_program(key):
  entry = PROGRAMS[key]
  iterate = entry['iterate']
  spec = spec_of(key)
  (name,) = spec['outputs']
  text, table = generated(key)
  assert kernel_common.read_meta_from_source(text)['packed_cells'] == '%s_fused_k1' % key
  # the two checkers compile (g++) beside the kernels (hiprtc), not after them
  with concurrent.futures.ThreadPoolExecutor(2) as pool:
    plain_orc = pool.submit(gpu_util.make_oracle, spec)
    wrap_orc = pool.submit(gpu_util.make_wrap_oracle, spec)
    prog = host.open_program(source=text, spec=spec)
  try:
    orc, wrap = plain_orc.result(), wrap_orc.result()
    fused = fused_of(prog.kernels)
    assert prog.kernels == table and fused and fused[0]['depth'] == 1
    # (a) the reference's run
    if key in FIXTURES:
      data = np.load(os.path.join(harness.GOLDEN, FAMILY, FIXTURES[key]))
      inputs = [np.ascontiguousarray(data['in_' + t['name']]) for t in spec['inputs']]
      assert inputs[0].shape[-1] >= fused[0]['w_out'] + SEAM_MARGIN
      check(prog, inputs, data['out_' + name], iterate, 'reference fixture', whole=True)
    # (b) the oracle on the shapes of the depth-1 entry's constants
    shapes = harness.volume_shapes_of(fused[0], harness.box_margins(spec, iterate))
    for shape in shapes:
      assert shape[0] * shape[1] * shape[2] <= MAX_CELLS, shape
      inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
      check(prog, inputs, orc.run(inputs, iterate=iterate)[name], iterate, 'oracle')
    # (c) every bit of the element in use, signed overflow wrapping on both sides
    ragged = shapes[-1]
    inputs = gpu_util.wide_inputs(spec, ragged, seed=gpu_util.SEED + len(key))
    check(prog, inputs, wrap.run(inputs, iterate=iterate)[name], iterate,
          'oracle, full-width operands')
    # (d) the memory contract: the deepest kernel alone, as many iterations as it fuses
    if guarded(key):
      deepest = fused[-1]
      depth = deepest['depth']
      shape = harness.volume_shapes_of(deepest, harness.box_margins(spec, depth))[-1]
      assert shape[0] * shape[1] * shape[2] <= MAX_CELLS, shape
      for mode in ('pool', 'sixteen'):
        launched = hold(prog, orc, shape, depth, mode, 'stream', depth, split=[depth],
                        edge=edge_of(spec))
        assert [k['name'] for k in launched] == [deepest['name']]
  finally:
    prog.close()
    prog.blob.unload()


def test_the_guarded_subset_holds_every_wide_lane_and_every_end_type():
  subset = [key for key in KEYS if guarded(key)]
  ends = {spec_of(key)['inputs'][-1]['c_type'] for key in subset}
  assert ends == {'uint8_t', 'int8_t', 'uint16_t', 'int16_t'}
  lanes = {(lane_bytes(spec_of(key), k), k['depth'])
           for key in subset for k in fused_of(generated(key)[1])[-1:]}
  assert {(16, 1), (16, 2)} <= lanes and len(subset) < len(KEYS)
  assert {edge_of(spec_of(key)) for key in subset} == {None, 'first', 'last'}


@pytest.mark.parametrize('key', ['ops5', 'plain5', 'plain7', 'plain8', 'plain22'])
def test_the_narrow_volumes_of_the_random_set_with_the_switch(key):
  """The five 3-D programs over 8- and 16-bit volumes of tests/golden/random_programs.json,
  which the default generate() leaves to the per-stage kernels: run_case's three checks
  with packed_cells=True, on a grid with a tile seam inside the box."""
  entry = RANDOM_PROGRAMS[key]
  spec = specmod.spec_from_stencil(frontend.loads(entry['text']))
  fused = fused_of(kernel.generate(spec, packed_cells=True)[1])
  assert fused and fused[0]['name'].endswith('_fused_k1')
  lo, hi = specmod.iteration_margins(spec, entry['iterate'])[-1]
  shape = (lo[2] + hi[2] + 9, lo[1] + hi[1] + 13,
           max(k['w_out'] for k in fused) + SEAM_MARGIN + lo[0] + hi[0])
  table = run_case(key, shape, np.random.default_rng(21000 + len(key)), packed_cells=True)
  assert [k['name'] for k in fused_of(table)] == [k['name'] for k in fused]
