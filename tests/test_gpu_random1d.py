"""Random 1-D programs (tests/random_programs.py: line_program; the texts in
tests/golden/random1d_programs.json) through the fused 1-D kernels (kernel_stream1d, in the
default form and under kernel.generate's `far_taps` with up to 8 lanes a side) on a real
MI355X, compiled at run time (hiprtc) under the keywords tests/random1d.py maps each program
to - the kernels whose coverage and resources tests/test_random1d_codegen.py pins: every
element type of 2, 4 and 8 bytes, locals of the other type of the same width, far reads of
computed levels, lanes of 16, 8 and 4 bytes down to one cell, offsets on the lane `hops` away,
tables that lack a depth, and the integer operators.  Every comparison is of bytes:

  (a) the reference's own run of the program (tests/golden/random1d/<key>.npz), the whole
      array - the box equals the reference, zero outside it -, per stage, under the depth
      limit and in every explicit split;
  (b) the CPU oracle on lengths from each entry's own constants (switch_form_gpu.line_lengths):
      every kernel alone at as many iterations as it fuses, then the program's `iterate` in
      every split the table gives, deepest first and shallowest first; the whole array against
      the per-stage run as well;
  (c) full-width operands (gpu_util.wide_inputs) against the oracle built with -fwrapv, every
      depth alone, in guarded arenas; a float program's values are finite;
  (d) the sweep's memory contract in guarded arenas, the deepest kernel and one iteration
      more, for the programs of random1d.guarded;
  (e) a sweep resumed from the margins the first part returned, guards intact, for the
      programs of random1d.resumed.

No fused 1-D kernel is in the default schedule: every fused run is under the depth limit of
the table's deepest kernel, and every run that is not per stage is held to launches of the
table's fused kernels whose depths sum to the iteration count."""
import concurrent.futures
import os

import numpy as np
import pytest

from soda_hip.codegen import kernel_common
from soda_hip.runtime import host

import gpu_util
import switch_form_gpu as harness
import test_gpu_memory_contract as contract
from random1d import (FAMILY, FIXTURES, KEYS, MAX_CELLS, PROGRAMS, SEAM_MARGIN, edge_of,
                      fused_of, generated, guarded, hops_of, keywords_of, lane_class, lengths,
                      margin_of, reads_far_local, refused_depths, resumed, spec_of, splits_of,
                      wide_lengths, wide_seed)

FLOATS = ('float', 'double')


def differing(got, want):
  return np.argwhere(np.ascontiguousarray(got).view(np.uint8) !=
                     np.ascontiguousarray(want).view(np.uint8))


def check(prog, inputs, want, iterate, splits, what, whole=False):
  """`want` on the output's box per stage, under the depth limit and in every split of
  `splits`, the whole array of every fused run against the per-stage run's; whole: `want` on
  the whole array, which is zero outside the box."""
  spec = prog.spec
  (name,) = spec['outputs']
  (n,) = inputs[0].shape
  dims = (n,)
  fused = fused_of(prog.kernels)
  names = {k['name'] for k in fused}
  limit = max(k['depth'] for k in fused)
  lo, hi = contract.box_of(spec, name, dims, iterate)
  sl = slice(lo[0], hi[0])
  assert want[sl].size == n - margin_of(spec, iterate) > 0, (what, n)
  staged = None
  try:
    for split in [None, 'limit'] + list(splits):
      said = (spec['app_name'], what, n, iterate, split)
      prog.set_max_depth(-1 if split is None else limit)
      if isinstance(split, list):
        prog.set_split(dims, iterate, split)
      try:
        launched = [k for k, _ in prog.schedule(dims, iterate)]
        (got,) = prog.run_numpy(inputs, iterate=iterate)
      finally:
        if isinstance(split, list):
          prog.set_split(dims, iterate, [])
      if split is None:
        assert [k['kind'] for k in launched] == ['stage'] * (iterate * len(spec['stages'])), said
        staged = got
      else:
        # no case passes by running the per-stage kernels
        assert launched and all(k['kind'] == 'fused' and k['name'] in names
                                for k in launched), (said, [k['name'] for k in launched])
        assert sum(k['depth'] for k in launched) == iterate, said
        if isinstance(split, list):
          assert [k['depth'] for k in launched] == split, said
      assert got.dtype == want.dtype and got.shape == want.shape, said
      differ = differing(got[sl], want[sl])
      assert differ.size == 0, ('%d bytes of the box differ, first at %s' % (
          len(differ), differ[0]), said, PROGRAMS[spec['app_name']]['text'])
      assert differing(got, staged).size == 0, said
      if whole:
        assert not got[:lo[0]].any() and not got[hi[0]:].any(), said
        assert differing(got, want).size == 0, said
  finally:
    prog.set_max_depth(0)


def resumed_sweeps(prog, iterate):
  """t1 iterations, then t2 more from the margins the first run returned - unspecified cells
  holding random bytes -: the bytes of t1 + t2 in one call on the box, guards intact."""
  spec = prog.spec
  (name,) = spec['outputs']
  fused = fused_of(prog.kernels)
  names = {k['name'] for k in fused}
  deep = fused[-1]
  n = deep['tile'][0] + 37 + margin_of(spec, iterate)
  dims = (n,)
  (a,) = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
  prog.set_max_depth(deep['depth'])
  try:
    for t1 in range(1, min(iterate, 5)):
      t2 = iterate - t1
      lo, hi = prog.margins(t1)
      level = np.random.default_rng(11).integers(0, 256, size=n * a.itemsize,
                                                 dtype=np.uint8).view(a.dtype).copy()
      level[lo[0]:n - hi[0]] = prog.run_numpy([a], iterate=t1)[0][lo[0]:n - hi[0]]
      whole = prog.run_numpy([a], iterate=iterate)[0]
      launched = [e for e, _ in prog.schedule(dims, t2, valid_lo=lo, valid_hi=hi)]
      assert launched and all(e['kind'] == 'fused' and e['name'] in names for e in launched)
      assert sum(e['depth'] for e in launched) == t2, (t1, t2)
      outs, bad, _ = gpu_util.run_guarded(prog, [level], t2, valid_lo=lo, valid_hi=hi,
                                          skews=gpu_util.pool_skews(2, a.itemsize))
      flo, fhi = contract.box_of(spec, name, dims, iterate)
      sl = slice(flo[0], fhi[0])
      assert whole[sl].size > 0 and len(np.unique(whole[sl])) > 1
      assert differing(outs[0][sl], whole[sl]).size == 0, (spec['app_name'], n, t1, t2)
      assert bad == [], (bad, spec['app_name'], n, t1, t2)
  finally:
    prog.set_max_depth(0)


@pytest.mark.gpu
@pytest.mark.parametrize('key', KEYS)
def test_random_line_program(key):
  entry = PROGRAMS[key]
  iterate = entry['iterate']
  spec = spec_of(key)
  (name,) = spec['outputs']
  text, table = generated(key)
  if keywords_of(key).get('far_taps'):
    assert kernel_common.read_meta_from_source(text)['far_taps'] == '%s_fused_k1' % key
  # the two checkers compile (g++) beside the kernels (hiprtc), not after them
  with concurrent.futures.ThreadPoolExecutor(2) as pool:
    plain_orc = pool.submit(gpu_util.make_oracle, spec)
    wrap_orc = pool.submit(gpu_util.make_wrap_oracle, spec)
    prog = host.open_program(source=text, spec=spec)
  try:
    orc, wrap = plain_orc.result(), wrap_orc.result()
    fused = fused_of(prog.kernels)
    assert prog.kernels == table and fused and fused[0]['depth'] == 1
    depths = [k['depth'] for k in fused]
    splits = splits_of(depths, iterate)
    assert all(sum(s) == iterate for s in splits) and [1] * iterate in splits
    # (a) the reference's run
    if key in FIXTURES:
      data = np.load(os.path.join(harness.GOLDEN, FAMILY, FIXTURES[key]))
      inputs = [np.ascontiguousarray(data['in_' + spec['inputs'][0]['name']])]
      assert inputs[0].shape[0] == max(k['w_out'] for k in fused) + margin_of(spec, iterate) + \
          SEAM_MARGIN
      check(prog, inputs, data['out_' + name], iterate, splits, 'reference fixture', whole=True)
    # (b) the oracle on the lengths of each entry's constants: every kernel alone ...
    for k in fused:
      for n in lengths(k, margin_of(spec, k['depth'])):
        assert n <= MAX_CELLS, (k['name'], n)
        inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
        check(prog, inputs, orc.run(inputs, iterate=k['depth'])[name], k['depth'],
              [[k['depth']]], 'oracle, %s alone' % k['name'])
    # ... then the program's own iteration count in every split
    if iterate > 1:
      for n in sorted({n for k in fused for n in lengths(k, margin_of(spec, iterate))}):
        assert n <= MAX_CELLS, n
        inputs = gpu_util.random_inputs(spec, (n,), seed=gpu_util.SEED + n)
        check(prog, inputs, orc.run(inputs, iterate=iterate)[name], iterate, splits, 'oracle')
    # (c) every bit of the element in use, signed overflow wrapping on both sides
    prog.set_max_depth(depths[-1])
    try:
      for i, k in enumerate(fused):
        depth = k['depth']
        for j, n in enumerate(wide_lengths(k, margin_of(spec, depth))):
          inputs = gpu_util.wide_inputs(spec, (n,), seed=wide_seed(key, n))
          if spec['inputs'][0]['c_type'] in FLOATS:
            lo, hi = contract.box_of(spec, name, (n,), depth)
            assert np.isfinite(wrap.run(inputs, iterate=depth)[name][lo[0]:hi[0]]).all()
          launched = contract.hold(prog, wrap, (n,), depth, contract.SKEWS[(i + j) % 3],
                                   'stream', depth, split=[depth], inputs=inputs)
          assert [e['name'] for e in launched] == [k['name']]
      # (d) the memory contract: the deepest kernel and one iteration more
      if guarded(key):
        deepest = fused[-1]
        split = [depths[-1], 1] if iterate > depths[-1] else [depths[-1]]
        for n in lengths(deepest, margin_of(spec, sum(split))):
          for mode in contract.SKEWS:
            launched = contract.hold(prog, orc, (n,), sum(split), mode, 'stream', depths[-1],
                                     split=split, edge=edge_of(spec))
            assert [e['depth'] for e in launched] == split
            assert all(e['kind'] == 'fused' for e in launched)
    finally:
      prog.set_max_depth(0)
    # (e) resumed sweeps
    if resumed(key):
      resumed_sweeps(prog, iterate)
  finally:
    prog.close()
    prog.blob.unload()


def test_the_subsets_hold_what_they_are_for():
  """Without a GPU: part (d) runs every head and every tail program, the first program of
  each element size at each lane width, the programs with 8 lanes on either side and those
  whose table lacks a depth, and not the whole set; part (e) one program per element width
  and a far program with a local, each with iterations to split."""
  subset = [key for key in KEYS if guarded(key)]
  assert len(subset) < len(KEYS)
  assert {lane_class(key) for key in subset} == {lane_class(key) for key in KEYS} == {
      (2, 16), (2, 8), (4, 16), (4, 8), (4, 4), (8, 16), (8, 8)}
  edges = [key for key in KEYS if edge_of(spec_of(key)) is not None]
  assert {edge_of(spec_of(key)) for key in edges} == {'first', 'last'} and set(edges) <= set(subset)
  assert any(hops_of(key) == (8, 8) for key in subset)
  lacking = [key for key in KEYS if refused_depths(key)]
  assert lacking and set(lacking) <= set(subset)
  again = [key for key in KEYS if resumed(key)]
  assert {lane_class(key)[0] for key in again} == {2, 4, 8} and len(again) <= 4
  assert any(reads_far_local(key) for key in again)
  assert all(PROGRAMS[key]['iterate'] >= 2 for key in again)
