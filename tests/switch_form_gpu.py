"""What the GPU tests of the opt-in kernel forms share (tests/test_gpu_lds3d.py,
test_gpu_lds3d_fields.py, test_gpu_lds3d_ring.py, test_gpu_far2d.py): one record per form
says what differs, the functions here run it; and the lengths and splits of the 1-D forms'
tests (test_gpu_far1d.py, test_gpu_random1d.py).  Everything goes through the C ABI from the
prebuilt `<app><suffix>.hsaco` of the form's switch; every comparison is of bytes."""
import collections
import json
import os

import numpy as np

from soda_hip.codegen import kernel, switches
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

import gpu_util
from conftest import ROOT
from test_gpu_memory_contract import box_of, hold

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SHORTEST_CHUNK = 8            # csrc/schedule.cpp: chunk_rows_min

# keyword:  the switch of kernel.generate (codegen/switches.py: suffix, depth limit)
# family:   tests/golden/<family>/*.npz and <family>_manifest.json, the reference's fixtures
# fixtures: app -> how many of them
# kernels:  spec -> [(name, depth), ...] of the fused entries of the table
# limit:    spec -> the depth limit the fused runs are under, as the file expects it; it is
#           held against switches.depth_limit_of, which sets it
# margins:  (spec, iterate) -> cells per dimension the launch's box is shorter than the array
# check:    (fused entries, spec): what else the form's entries are held to
# whole:    (output, iterate) -> it is handed on unchanged, its box is the whole array
Form = collections.namedtuple('Form', 'keyword family fixtures kernels limit margins check whole',
                              defaults=(lambda fused, spec: None, lambda name, iterate: False))


def box_margins(spec, iterate):
  """The first output's box of `iterate` iterations against the array, (x, y, z): the
  programs of one output."""
  lo, hi = specmod.iteration_boxes(spec, iterate)[-1][spec['outputs'][0]]
  return [b - a for a, b in zip(lo, hi)]


def hull_margins(spec, iterate):
  """The intersection of the outputs' boxes after `iterate` iterations against the array:
  the hull's lo + hi margin, (x, y, z)."""
  lo, hi = specmod.iteration_margins(spec, iterate)[-1]
  return [a + b for a, b in zip(lo, hi)]


def lowered_hull_margins(spec, iterate):
  """hull_margins of the program as the 2-D generators lower it, pointwise stages inlined."""
  return hull_margins(specmod.inline_pointwise(spec), iterate)


_CACHE = {}
_MANIFESTS = {}


def opened(form, app):
  """(program from the prebuilt code object generated with the form's switch, oracle)"""
  if (form.keyword, app) not in _CACHE:
    spec = gpu_util.load_spec(app)
    path = os.path.join(gpu_util.BLOBS,
                        app + switches.BY_KEYWORD[form.keyword].suffix + '.hsaco')
    assert os.path.exists(path), '%s missing: run __graft_entry__.build()' % path
    prog = host.open_program(blob=path, spec=spec)
    _CACHE[form.keyword, app] = (prog, gpu_util.make_oracle(spec))
  return _CACHE[form.keyword, app]


def fused_of(form, prog):
  """The fused entries of the table: the form's names and depths, and its own checks."""
  fused = [k for k in prog.kernels if k['kind'] == 'fused']
  assert [(k['name'], k['depth']) for k in fused] == form.kernels(prog.spec)
  form.check(fused, prog.spec)
  return fused


def limit_of(form, prog):
  """The depth limit of a fused run, as the entry points of a product generated with the
  switch set it (switches.depth_limit_of): 0 is the default schedule."""
  limit, _ = switches.depth_limit_of(prog.spec, {form.keyword: True})
  assert limit == form.limit(prog.spec)
  return limit


def fused_and_staged(form, prog, inputs, iterate, depth=None):
  """The arrays of the fused schedule - every launch one of the form's kernels; `depth`: the
  split fixed to launches of that depth - and the per-stage run's."""
  dims = tuple(reversed(inputs[0].shape))
  stages = [k['name'] for k in prog.kernels if k['kind'] == 'stage']
  expected = form.kernels(prog.spec)
  try:
    prog.set_max_depth(limit_of(form, prog))
    if depth is not None:
      assert iterate % depth == 0
      prog.set_split(dims, iterate, [depth] * (iterate // depth))
    launched = [k for k, _ in prog.schedule(dims, iterate)]
    assert all(k['kind'] == 'fused' for k in launched), [k['name'] for k in launched]
    assert sum(k['depth'] for k in launched) == iterate
    if depth is not None:
      assert [k['depth'] for k in launched] == [depth] * (iterate // depth)
    if [d for _, d in expected] == [1]:      # one kernel of depth 1: nothing else is launched
      assert [k['name'] for k in launched] == [expected[0][0]] * iterate
    got = prog.run_numpy(inputs, iterate=iterate)
    if depth is not None:
      prog.set_split(dims, iterate, [])
    prog.set_max_depth(-1)
    assert [k['name'] for k, _ in prog.schedule(dims, iterate)] == stages * iterate
    staged = prog.run_numpy(inputs, iterate=iterate)
  finally:
    prog.set_max_depth(0)
  return got, staged


def fixtures(form, app):
  """The whole arrays equal the reference's: each output on its box, zero outside; the same
  arrays per stage."""
  prog, _ = opened(form, app)
  spec = prog.spec
  fused_of(form, prog)
  if form.family not in _MANIFESTS:
    with open(os.path.join(GOLDEN, form.family + '_manifest.json')) as f:
      _MANIFESTS[form.family] = json.load(f)
  n = 0
  for fx, meta in sorted(_MANIFESTS[form.family].items()):
    if not meta['key'].startswith(app + '.'):
      continue
    data = np.load(os.path.join(GOLDEN, form.family, fx))
    inputs = [data['in_' + t['name']] for t in spec['inputs']]
    got, staged = fused_and_staged(form, prog, inputs, meta['iterate'])
    for name, g, s in zip(spec['outputs'], got, staged):
      want = data['out_' + name]
      assert np.array_equal(g.view(np.uint8), want.view(np.uint8)), (fx, name)
      assert np.array_equal(s.view(np.uint8), want.view(np.uint8)), (fx, name, 'per stage')
    n += 1
  assert n == form.fixtures(app)


def shapes_of(form, k, spec, iterate):
  """Shapes from the constants of the entry `k`, slowest dimension first: an intersection box
  of one cell each way (wider outputs then live almost entirely outside the launch's box);
  one tile (2-D: one strip) plus one column and one row with fewer planes (rows) than
  fill_rows + 1; two of the shortest chunks less one plane (row), a few cells wide, so the
  window restarts at a chunk seam; a ragged grid of several tiles each way - 3-D: 2 x 3
  tiles plus odd remainders, 29 planes, clamped loads on all six sides; 2-D: two workgroup
  tiles plus 37 columns by 60 rows, strips whose halo lanes, more than one per side, hang
  over both ends of the rows, chunks whose fill rows are clamped at the top and bottom."""
  assert k['fill_rows'] >= 2
  if spec['dim'] == 2:
    mx, my = form.margins(spec, iterate)
    assert k['tile'][0] == 4 * k['w_out']
    return [(my + 1, mx + 1),
            (my + k['fill_rows'] - 1, k['w_out'] + 1 + mx),
            (my + 2 * SHORTEST_CHUNK - 1, mx + 5),
            (my + 60, 2 * k['tile'][0] + 37 + mx)]
  mx, my, mz = form.margins(spec, iterate)
  tx, ty = k['tile'][:2]
  return [(mz + 1, my + 1, mx + 1),
          (mz + k['fill_rows'] - 1, ty + 1 + my, tx + 1 + mx),
          (mz + 2 * SHORTEST_CHUNK - 1, my + 3, mx + 5),
          (mz + 29, 3 * ty + 5 + my, 2 * tx + 37 + mx)]


def volume_shapes_of(k, margins):
  """shapes_of for the 3-D entry `k` of a program that may reach nowhere along z (fill_rows 0:
  no z offset at all; 1: one-sided), `margins` (x, y, z) as Form.margins gives them: the same
  four shapes, the second with the fewest planes that leave the box one - below the fill
  where there is one to stay below."""
  mx, my, mz = margins
  tx, ty = k['tile'][:2]
  return [(mz + 1, my + 1, mx + 1),
          (mz + max(1, k['fill_rows'] - 1), ty + 1 + my, tx + 1 + mx),
          (mz + 2 * SHORTEST_CHUNK - 1, my + 3, mx + 5),
          (mz + 29, 3 * ty + 5 + my, 2 * tx + 37 + mx)]


def line_lengths(k, m):
  """Array lengths from the constants of the fused 1-D entry `k`, m = cells the launch's box
  is shorter than the array: a box of one cell, of half a segment, of one segment and of one
  cell more, of one workgroup tile less and plus one cell, and three tiles and 17 cells."""
  w_out, tile = k['w_out'], k['tile'][0]
  assert tile == 4 * k['segs'] * w_out
  return [m + 1, m + w_out // 2, m + w_out, m + w_out + 1, m + tile - 1, m + tile + 1,
          3 * tile + 17]


def splits_of(depths, iterate):
  """`iterate` as launches of the table's depths under every limit, deepest first and
  shallowest first.  (The depths need not be consecutive: a table may lack one that leaves a
  segment no cell, and the shallower ones fill what it would have taken.)"""
  out = []
  for limit in depths:
    s = []
    for d in sorted(depths, reverse=True):
      while d <= limit and sum(s) + d <= iterate:
        s.append(d)
    for split in (s, s[::-1]):
      if split not in out:
        out.append(split)
  return out


def wide_shape_of(form, k, spec, iterate):
  """The shape of the full-width-operand run: one tile and an odd remainder."""
  if spec['dim'] == 2:
    mx, my = form.margins(spec, iterate)
    return (my + 23, k['tile'][0] + 35 + mx)
  mx, my, mz = form.margins(spec, iterate)
  return (mz + 11, k['tile'][1] + 9 + my, k['tile'][0] + 35 + mx)


def slices_of(spec, name, shape, iterate):
  """(lo, hi, slices of the array) of an output's box, lo and hi as (x, y[, z])."""
  lo, hi = box_of(spec, name, tuple(reversed(shape)), iterate)
  return lo, hi, tuple(slice(a, b) for a, b in zip(reversed(lo), reversed(hi)))


def check_shape(form, prog, orc, shape, iterate, depth=None):
  """Random inputs of `shape`: every output's box against the oracle, the whole arrays
  against the per-stage run."""
  spec = prog.spec
  inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
  want = orc.run(inputs, iterate=iterate)
  got, staged = fused_and_staged(form, prog, inputs, iterate, depth)
  for name, g, s in zip(spec['outputs'], got, staged):
    lo, hi, sl = slices_of(spec, name, shape, iterate)
    if form.whole(name, iterate):
      assert lo == [0] * len(shape) and hi == list(reversed(shape))
    assert g[sl].size > 0, (name, shape, iterate)
    assert np.array_equal(np.ascontiguousarray(g[sl]).view(np.uint8),
                          np.ascontiguousarray(want[name][sl]).view(np.uint8)), \
        (name, shape, iterate, depth)
    assert np.array_equal(g.view(np.uint8), s.view(np.uint8)), (name, shape, iterate, depth)


def picked(form, prog, iterate, depth):
  """(the entry the run is held to, the split that fixes it): the form's only entry in its
  own schedule where `depth` is None, else the one of that depth in launches of that depth."""
  fused = fused_of(form, prog)
  if depth is None:
    (k,) = fused
    return k, None
  (k,) = [e for e in fused if e['depth'] == depth]
  return k, [depth] * (iterate // depth)


def held(form, prog, orc, k, split, shape, iterate, mode, inputs=None):
  """test_gpu_memory_contract.hold under the form's depth limit: every launch is `k`."""
  prog.set_max_depth(limit_of(form, prog))
  try:
    launched = hold(prog, orc, shape, iterate, mode, 'stream', k['depth'], split=split,
                    inputs=inputs)
    assert [e['name'] for e in launched] == [k['name']] * (iterate // k['depth'])
  finally:
    prog.set_max_depth(0)


def memory_contract(form, app, iterate, cases, depth=None):
  """gpu_util.run_guarded on `cases`, ((index into shapes_of, placements), ...), `iterate`
  iterations in the entry of picked(): every output's box equals the oracle, guards intact,
  inputs unchanged."""
  prog, orc = opened(form, app)
  k, split = picked(form, prog, iterate, depth)
  shapes = shapes_of(form, k, prog.spec, iterate)
  for index, modes in cases:
    for mode in modes:
      held(form, prog, orc, k, split, shapes[index], iterate, mode)


def full_width_operands(form, app, iterate, c_type, depth=None, inputs_of=None):
  """Mixed signs and exponents over the element's whole mantissa - gpu_util.wide_inputs at
  the default span, or `inputs_of(app, spec, shape)` -, `iterate` iterations in the entry of
  picked().  The oracle's values on every output's box are finite: no NaN payload enters
  the byte comparison."""
  prog, orc = opened(form, app)
  spec = prog.spec
  assert spec['inputs'][0]['c_type'] == c_type
  k, split = picked(form, prog, iterate, depth)
  shape = wide_shape_of(form, k, spec, iterate)
  inputs = inputs_of(app, spec, shape) if inputs_of else gpu_util.wide_inputs(spec, shape)
  want = orc.run(inputs, iterate=iterate)
  for name in spec['outputs']:
    _, _, sl = slices_of(spec, name, shape, iterate)
    assert want[name][sl].size > 0 and np.isfinite(want[name][sl]).all(), name
  held(form, prog, orc, k, split, shape, iterate, 'pool', inputs)


def run_time_compile(form, app, iterate, plain_kinds, depth=None):
  """host.open_program(spec=..., <switch>=True): the offline build's table, bit-exact on the
  ragged shape (`depth`: check_shape's) and the blob's bytes there; without the switch the
  per-stage kernels only."""
  spec = gpu_util.load_spec(app)
  blob_prog, orc = opened(form, app)
  on = {form.keyword: True}
  prog = host.open_program(spec=spec, **on)
  try:
    assert prog.kernels == kernel.generate(spec, **on)[1]
    assert prog.kernels == blob_prog.kernels
    shape = shapes_of(form, fused_of(form, prog)[-1], spec, iterate)[-1]
    check_shape(form, prog, orc, shape, iterate, depth)
    inputs = gpu_util.random_inputs(spec, shape, seed=gpu_util.SEED + sum(shape))
    got, _ = fused_and_staged(form, prog, inputs, iterate)
    same, _ = fused_and_staged(form, blob_prog, inputs, iterate)
    for g, s in zip(got, same):
      assert np.array_equal(g.view(np.uint8), s.view(np.uint8))
  finally:
    prog.close()
    prog.blob.unload()
  plain = host.open_program(spec=spec)
  try:
    assert [k['kind'] for k in plain.kernels] == plain_kinds
  finally:
    plain.close()
    plain.blob.unload()
