"""The full-width operands of the GPU suite (gpu_util.wide_inputs) and the oracle they are
held to (gpu_util.make_wrap_oracle), checked on the CPU:

  * the inputs really fill the element: both dwords of an 8-byte element, every byte of a
    narrower one, both signs, twenty binades and more, nothing that is not finite;
  * wrap semantics are STABLE: for every committed program with a signed integer tensor
    (and blur and sobel2d, whose uint16 arithmetic goes through `int`) the oracle built with
    -O2 -fwrapv equals the one built with -O0 -fwrapv cell for cell - the optimiser finds
    no other undefined behaviour to exploit, so there is one answer to hold a kernel to;
  * the float inputs do not overflow: every float / double program and sample stays finite
    on its whole valid box.  That is a condition on the INPUTS (an inf or a NaN would
    compare equal whatever the kernel did to the operands that made it), not on the product.

The shared objects go to tests/_oracle_build (cached); a first run compiles them in
parallel."""
import concurrent.futures
import json
import os

import numpy as np
import pytest

from soda_hip import frontend
from soda_hip.codegen import spec as specmod

import gpu_util
from conftest import GOLDEN

with open(os.path.join(GOLDEN, 'random_programs.json')) as f:
  PROGRAMS = json.load(f)
SAMPLES = ('blur', 'jacobi2d', 'jacobi3d', 'seidel2d', 'heat3d', 'sobel2d', 'denoise2d',
           'denoise3d')
SIGNED = ('int8_t', 'int16_t', 'int32_t', 'int64_t')
FLOATS = ('float', 'double', '_Float16')


def spec_of(key):
  if key in PROGRAMS:
    return specmod.spec_from_stencil(frontend.loads(PROGRAMS[key]['text']))
  return gpu_util.load_spec(key)


def iterate_of(key, spec):
  return PROGRAMS[key]['iterate'] if key in PROGRAMS else spec['iterate']


def tensor_types(spec):
  return {t['c_type'] for t in spec['inputs']} | {s['c_type'] for s in spec['stages']}


def shape_of(key, spec, iterate):
  """A small grid on which every output keeps at least 20 cells per dimension."""
  shape = [61, 333] if spec['dim'] == 2 else [24, 27, 150]
  if key.startswith('deep'):
    shape = [120, 300]
  boxes = specmod.iteration_boxes(spec, iterate)[-1]
  for name in spec['outputs']:
    lo, hi = boxes[name]
    for d in range(spec['dim']):
      axis = spec['dim'] - 1 - d
      shape[axis] = max(shape[axis], hi[d] - lo[d] + 20)
  return tuple(shape)


def boxes_of(spec, shape, iterate):
  """{output: numpy slices of its own valid box}"""
  out = {}
  for name in spec['outputs']:
    lo, hi = specmod.iteration_boxes(spec, iterate)[-1][name]
    out[name] = tuple(slice(-lo[d], shape[::-1][d] - hi[d]) for d in reversed(range(spec['dim'])))
  return out


KEYS = sorted(PROGRAMS) + list(SAMPLES)
SPECS = {k: spec_of(k) for k in KEYS}
WRAP_KEYS = [k for k in KEYS if tensor_types(SPECS[k]) & set(SIGNED)] + ['blur', 'sobel2d']
FLOAT_KEYS = [k for k in KEYS if tensor_types(SPECS[k]) & set(FLOATS)]


@pytest.fixture(scope='module')
def built():
  """Every shared object of this file, compiled side by side where the cache lacks it."""
  jobs = [(k, '-O2') for k in sorted(set(WRAP_KEYS + FLOAT_KEYS))] + \
         [(k, '-O0') for k in WRAP_KEYS]
  with concurrent.futures.ThreadPoolExecutor(min(8, len(os.sched_getaffinity(0)))) as pool:
    return dict(zip(jobs, pool.map(
        lambda j: gpu_util.make_wrap_oracle(SPECS[j[0]], opt=j[1]), jobs)))


# ---- the inputs ---------------------------------------------------------------------------

@pytest.mark.parametrize('c_type', sorted(specmod.NUMPY_NAME))
def test_wide_inputs_fill_the_element(c_type):
  dt = np.dtype(specmod.NUMPY_NAME[c_type])
  spec = dict(inputs=[dict(c_type=c_type), dict(c_type=c_type)])
  a, b = gpu_util.wide_inputs(spec, (40, 300), seed=5)
  assert a.dtype == dt and a.shape == (40, 300) and a.flags['C_CONTIGUOUS']
  again = gpu_util.wide_inputs(spec, (40, 300), seed=5)
  assert np.array_equal(a.view(np.uint8), again[0].view(np.uint8))
  assert np.array_equal(b.view(np.uint8), again[1].view(np.uint8))
  assert not np.array_equal(a, b)
  assert not np.array_equal(a, gpu_util.wide_inputs(spec, (40, 300), seed=6)[0])
  n = a.size
  lanes = a.reshape(-1).view(np.uint8).reshape(n, dt.itemsize)
  # every byte of the element varies (the top byte of a float holds the sign and seven
  # exponent bits: 2 x 13 values over the 25 binades; that of a double the sign and the
  # exponent's seven HIGH bits: 2 x 2 values - the dwords are looked at below)
  for i in range(dt.itemsize):
    assert len(np.unique(lanes[:, i])) >= (16 if (c_type, i) != ('double', 7) else 4), (c_type, i)
  if dt.itemsize == 8:
    halves = a.reshape(-1).view('<u4').reshape(n, 2)
    assert len(np.unique(halves[:, 0])) >= 0.9 * n, c_type
    assert len(np.unique(halves[:, 1])) >= 1000, c_type
    assert np.count_nonzero(halves[:, 0]) >= 0.99 * n, c_type
  if dt.kind in 'if':
    assert (a < 0).sum() > n // 3 and (a > 0).sum() > n // 3, c_type
  if dt.kind == 'f':
    assert np.isfinite(a).all()
    binades = np.unique(np.frexp(np.abs(a.astype(np.float64)))[1])
    assert len(binades) >= 20, binades
    assert np.abs(a).min() >= np.finfo(dt).tiny            # no zero, no subnormal
    # the mantissa is drawn on the type's own grid: its last bit is set in half of them
    last = a.reshape(-1).view('<u%d' % dt.itemsize) & 1
    assert 0.4 * n < last.sum() < 0.6 * n
  else:
    info = np.iinfo(dt)
    assert a.min() < info.min + (int(info.max) - int(info.min)) // 64
    assert a.max() > info.max - (int(info.max) - int(info.min)) // 64


def test_the_exponent_span_is_a_parameter():
  spec = dict(inputs=[dict(c_type='double')])
  (a,) = gpu_util.wide_inputs(spec, (40, 300), exponents=3)
  e = np.frexp(np.abs(a))[1] - 1
  assert e.min() == -3 and e.max() == 3
  (h,) = gpu_util.wide_inputs(dict(inputs=[dict(c_type='_Float16')]), (40, 300))
  e = np.frexp(np.abs(h.astype(np.float64)))[1] - 1
  assert e.min() == -gpu_util.WIDE_EXPONENTS_HALF and e.max() == gpu_util.WIDE_EXPONENTS_HALF
  assert gpu_util.WIDE_EXPONENTS_HALF < gpu_util.WIDE_EXPONENTS == 12


def test_at_most_five_programs_have_a_narrowed_span():
  assert len(gpu_util.NARROWED_EXPONENTS) <= 5
  assert set(gpu_util.NARROWED_EXPONENTS) <= set(FLOAT_KEYS)


# ---- the oracle ---------------------------------------------------------------------------

def test_the_programs_are_all_here():
  # 23 programs with a signed integer tensor + blur + sobel2d; 55 float programs + 6 samples
  assert len(PROGRAMS) == 100 and len(WRAP_KEYS) == 25 and len(FLOAT_KEYS) == 55 + 6


@pytest.mark.parametrize('key', WRAP_KEYS)
def test_wrap_semantics_are_stable(built, key):
  spec = SPECS[key]
  iterate = iterate_of(key, spec)
  shape = shape_of(key, spec, iterate)
  inputs = gpu_util.wide_inputs_of(key, spec, shape)
  o2 = built[key, '-O2'].run(inputs, iterate=iterate)
  o0 = built[key, '-O0'].run(inputs, iterate=iterate)
  for name, sl in boxes_of(spec, shape, iterate).items():
    a, b = np.ascontiguousarray(o2[name][sl]), np.ascontiguousarray(o0[name][sl])
    assert a.size > 0, (key, name, shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (key, name)
    if a.dtype.itemsize == 8 and a.dtype.kind != 'f':
      # the results, too, use the high dword
      assert len(np.unique(a.reshape(-1).view('<u4')[1::2])) > 100, (key, name)


@pytest.mark.parametrize('key', FLOAT_KEYS)
def test_wide_floats_do_not_overflow(built, key):
  spec = SPECS[key]
  iterate = iterate_of(key, spec)
  shape = shape_of(key, spec, iterate)
  inputs = gpu_util.wide_inputs_of(key, spec, shape)
  got = built[key, '-O2'].run(inputs, iterate=iterate)
  for name, sl in boxes_of(spec, shape, iterate).items():
    a = got[name][sl]
    assert a.size > 0, (key, name, shape)
    if a.dtype.kind == 'f':
      assert np.isfinite(a).all(), (key, name, int((~np.isfinite(a)).sum()), a.size)
      # and not a field of zeros either: the operands reach the result
      assert len(np.unique(a)) > a.size // 2, (key, name)
