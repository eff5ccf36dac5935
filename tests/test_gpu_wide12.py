"""The 12-column-lane deep 2-D kernels (`jacobi2d_fused_k24w` / `k20w`,
kernel_stream2d_wp.emit with cols=6) on the GPU: forced with a fixed split and the run
time's SODA_HIP_PREFER hook, run between guards, and compared bit for bit with the oracle
on every valid cell.

Shapes: widths 768 (one strip, exactly min_extent), 769 (a second strip of one column's
worth of box, moved inside the array), 1487 (two strips, a ragged seam: 1487 - 48 = 1439
box columns, one short of two tiles) and 1440 + 768 - 1 = 2207 (the last strip moved inside
the array); heights 61 (fewer rows than the 51 fill rows plus one rotation period) and 200;
24 iterations (k24w alone), 25 (k24w and a depth-1 tail) and 44 (k24w + k20w)."""
import contextlib
import os

import numpy as np
import pytest

import gpu_util

pytestmark = pytest.mark.gpu

WIDTHS = (768, 769, 1487, 1440 + 768 - 1)
# (height, iterate, split): 44 iterations leave no row of a 61-row array
RUNS = ((61, 24, [24]), (61, 25, [24, 1]), (200, 24, [24]), (200, 25, [24, 1]),
        (200, 44, [24, 20]))
WIDE = {24: 'jacobi2d_fused_k24w', 20: 'jacobi2d_fused_k20w'}


@pytest.fixture(scope='module')
def prog():
  p = gpu_util.open_prebuilt('jacobi2d')
  yield p
  p.close()


@pytest.fixture(scope='module')
def orc(prog):
  return gpu_util.make_oracle(prog.spec)


@contextlib.contextmanager
def preferring_wide():
  """Same-depth alternatives are chosen per launch by price; the tuning hook names the form
  to take wherever it can run (it changes which kernel runs, never what it computes)."""
  saved = {n: os.environ.get(n) for n in ('SODA_HIP_TUNING', 'SODA_HIP_PREFER')}
  os.environ['SODA_HIP_TUNING'] = '1'
  os.environ['SODA_HIP_PREFER'] = 'w'
  try:
    yield
  finally:
    for n, v in saved.items():
      if v is None:
        os.environ.pop(n, None)
      else:
        os.environ[n] = v


def uniform(shape):
  return np.random.default_rng(gpu_util.SEED + shape[1]).random(shape, dtype=np.float32)


def signed_ramp(shape):
  """Negative values, zeros and positive ones in every row and across every seam."""
  h, w = shape
  y, x = np.mgrid[0:h, 0:w]
  return (((x * 7 + y * 13) % 41) - 20).astype(np.float32) * np.float32(0.125)


def check(prog, orc, a, iterate, split, expect, margin=(0, 0)):
  """One guarded sweep of `a` (valid inside `margin` = (x, y) cells from every edge) under
  `split`; the launched kernels must be `expect` and every valid cell the oracle's."""
  shape = a.shape
  dims = (shape[1], shape[0])
  mx, my = margin
  valid = dict(valid_lo=(mx, my), valid_hi=(mx, my)) if mx or my else {}
  prog.set_split(dims, iterate, split)
  try:
    with preferring_wide():
      names = [k['name'] for k, _ in prog.schedule(dims, iterate, **valid)]
      assert names[:len(expect)] == expect, (dims, iterate, names)
      outs, bad, _ = gpu_util.run_guarded(prog, [a], iterate, **valid)
  finally:
    prog.set_split(dims, iterate, [])
  assert bad == [], (dims, iterate, bad[:3])
  inner = a[my:shape[0] - my, mx:shape[1] - mx]
  want = orc.run([np.ascontiguousarray(inner)], iterate=iterate)[prog.spec['outputs'][0]]
  sl = orc.valid_slices((inner.shape[1], inner.shape[0]), iterate)
  got = outs[0][my:shape[0] - my, mx:shape[1] - mx]
  assert want[sl].size > 0
  assert np.array_equal(got[sl], want[sl]), (dims, iterate, margin)


@pytest.mark.parametrize('width', WIDTHS)
def test_wide12_matches_the_oracle(prog, orc, width):
  for height, iterate, split in RUNS:
    expect = [WIDE.get(d, 'jacobi2d_fused_k%d' % d) for d in split]
    check(prog, orc, uniform((height, width)), iterate, split, expect)


@pytest.mark.parametrize('width', (769, 1487))
def test_wide12_signed_values_through_the_seams(prog, orc, width):
  check(prog, orc, signed_ramp((200, width)), 44, [24, 20], [WIDE[24], WIDE[20]])
  check(prog, orc, signed_ramp((61, width)), 24, [24], [WIDE[24]])


def test_wide12_box_origin_off_the_vector_grid(prog, orc):
  """A valid-region margin of (1, 2): the box starts at column 25, the strips at 24."""
  for width in (771, 1489):
    check(prog, orc, uniform((204, width)), 24, [24], [WIDE[24]], margin=(1, 2))
    check(prog, orc, signed_ramp((204, width)), 25, [24, 1],
          [WIDE[24], 'jacobi2d_fused_k1'], margin=(1, 2))


def test_a_narrow_grid_falls_back_to_the_shipped_kernels(prog, orc):
  """Below 768 columns the 12-column-lane kernels cannot run (min_extent): the shipped
  depth-24 kernel takes the launch, whatever the hook prefers."""
  for width in (767, 600):
    check(prog, orc, uniform((120, width)), 24, [24], ['jacobi2d_fused_k24'])
    check(prog, orc, signed_ramp((120, width)), 44, [24, 20],
          ['jacobi2d_fused_k24', 'jacobi2d_fused_k20'])
