"""bench.py --dump-outputs: the arrays a caller of the timed sweep receives (zero outside
each output's own box), whole when they fit the byte budget, else a seeded sample that
holds the same cells on every run."""
import os
import sys

import numpy as np

from conftest import ROOT, SAMPLES

sys.path.insert(0, ROOT)
import bench                                        # noqa: E402
from soda_hip import frontend                       # noqa: E402
from soda_hip.codegen import spec as specmod        # noqa: E402


class FakeOutput:
  """Stands in for host.DeviceArray: a download of what the sweep left in the buffer."""

  def __init__(self, raw):
    self.raw = raw

  def download(self, shape, dtype):
    assert self.raw.dtype == dtype
    return self.raw.reshape(shape).copy()


class FakeProgram:
  def __init__(self, dtypes):
    self.out_dtypes = [np.dtype(d) for d in dtypes]


def jacobi2d(iterate):
  st = frontend.load(os.path.join(SAMPLES, 'jacobi2d.soda'), iterate=iterate)
  return specmod.spec_from_stencil(st)


def test_whole_output_is_zero_outside_its_box(tmp_path):
  spec = jacobi2d(3)
  dims = [40, 30]
  raw = np.random.default_rng(5).random((30, 40), dtype=np.float32) + 1
  bench.dump_outputs(str(tmp_path), spec, FakeProgram(['float32']), [FakeOutput(raw)],
                     dims, 3)
  got = np.load(tmp_path / (spec['outputs'][0] + '.npy'))
  assert got.dtype == np.float32 and got.shape == raw.shape
  lo, hi = specmod.iteration_margins(spec, 3)[-1]
  sl = (slice(lo[1], 30 - hi[1]), slice(lo[0], 40 - hi[0]))
  assert np.array_equal(got[sl], raw[sl])
  outside = np.ones(raw.shape, bool)
  outside[sl] = False
  assert outside.any() and not got[outside].any()


def test_large_output_is_a_seeded_sample(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 1000)
  spec = jacobi2d(2)
  dims = [300, 200]
  raw = np.random.default_rng(6).integers(1, 1 << 30, size=(200, 300)).astype(np.uint32)
  name = spec['outputs'][0] + '.npy'
  program = FakeProgram(['uint32'])     # 32-bit integers: exact in float64
  bench.dump_outputs(str(tmp_path / 'a'), spec, program, [FakeOutput(raw)], dims, 2)
  bench.dump_outputs(str(tmp_path / 'b'), spec, program, [FakeOutput(raw)], dims, 2)
  got = np.load(tmp_path / 'a' / name)
  assert np.array_equal(got, np.load(tmp_path / 'b' / name))
  assert got.dtype == np.float64 and 400 < got.size <= 500    # 4000 bytes of float64
  assert got.size * got.itemsize <= bench.DUMP_BYTES
  idx = np.unique(np.random.default_rng(bench.SEED).integers(0, raw.size, size=500))
  lo, hi = specmod.iteration_margins(spec, 2)[-1]
  y, x = np.unravel_index(idx, raw.shape)
  inside = (y >= lo[1]) & (y < 200 - hi[1]) & (x >= lo[0]) & (x < 300 - hi[0])
  assert np.array_equal(got, np.where(inside, raw.reshape(-1)[idx], 0))
  assert (~inside).any() and inside.any()
