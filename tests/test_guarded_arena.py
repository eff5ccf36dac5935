"""The checker of the GPU memory-contract tests (gpu_util.Arena) on a numpy stand-in for
the device: a byte buffer and a fake "sweep" that stores where it is told.  Every planted
violation below must make Arena.check report a failure - this is the proof that the GPU
assertions of tests/test_gpu_memory_contract.py can fail; nothing on a GPU is made to
misbehave for it."""
import numpy as np
import pytest

import gpu_util

SHAPES = [((70, 257), np.float32), ((130, 515), np.uint16), ((12, 33, 70), np.float32),
          ((1003,), np.float32), ((5, 6, 7, 40), np.float32)]


def make(shape, dtype, skews):
  dtype = np.dtype(dtype)
  arena = gpu_util.Arena([('in:a', 'in', shape, dtype), ('in:w', 'in', shape, dtype),
                          ('out:b', 'out', shape, dtype), ('out:c', 'out', shape, dtype)],
                         skews=skews)
  rng = np.random.default_rng(7)
  if dtype.kind == 'f':
    ins = [rng.random(shape, dtype=np.float32).astype(dtype) for _ in range(2)]
  else:
    ins = [rng.integers(0, 65536, size=shape).astype(dtype) for _ in range(2)]
  image = arena.image({'in:a': ins[0], 'in:w': ins[1]})
  return arena, ins, image.copy()      # the copy is the stand-in's device memory


def store(device, arena, name, element, value):
  """The fake kernel: one element store at `element` elements from the start of `name`
  (negative, or beyond the array's size: outside it)."""
  a = arena.array(name)
  size = a['dtype'].itemsize
  at = a['offset'] + element * size
  device[at:at + size] = np.array([value], dtype=a['dtype']).view(np.uint8)


def flip(device, arena, name, element):
  """... storing a value that differs from what was there in every byte."""
  a = arena.array(name)
  size = a['dtype'].itemsize
  at = a['offset'] + element * size
  device[at:at + size] ^= 0xff


def cells(shape):
  return int(np.prod(shape))


def skew_sets(dtype):
  size = np.dtype(dtype).itemsize
  return [None, gpu_util.pool_skews(4, size)]


CASES = [(s, d, k) for s, d in SHAPES for k in (0, 1)]


@pytest.mark.parametrize('shape,dtype,skewed', CASES)
def test_layout(shape, dtype, skewed):
  skews = skew_sets(dtype)[skewed]
  arena, ins, device = make(shape, dtype, skews)
  size = np.dtype(dtype).itemsize
  row = shape[-1] * size
  want = max(4096, 2 * row + (cells(shape[1:]) * size if len(shape) >= 3 else 0))
  assert gpu_util.guard_bytes(shape, size) == want
  # guards and arrays tile the arena, in order, without gaps
  pieces = sorted([(g['offset'], g['nbytes']) for g in arena.guards] +
                  [(a['offset'], a['nbytes']) for a in arena.arrays])
  at = 0
  for off, n in pieces:
    assert off == at and n > 0
    at += n
  assert at == arena.nbytes and len(arena.guards) == len(arena.arrays) + 1
  assert all(g['nbytes'] >= want for g in arena.guards)
  for i, a in enumerate(arena.arrays):
    assert a['offset'] % size == 0
    assert a['offset'] % 64 == (skews[i] if skews else 0)
  if skews:
    assert all(a['offset'] % 16 != 0 for a in arena.arrays)
  assert arena.nbytes < 8 << 20
  # outputs and guards are not a constant, and two arenas with one seed agree
  assert len(np.unique(arena.view(device, 'out:b').view(np.uint8))) > 200
  assert np.array_equal(make(shape, dtype, skews)[2], device)
  # the inputs are where the pointers say
  assert np.array_equal(arena.view(device, 'in:a'), ins[0])
  assert np.array_equal(arena.view(device, 'in:w'), ins[1])


@pytest.mark.parametrize('shape,dtype,skewed', CASES)
def test_an_untouched_arena_and_stores_anywhere_inside_the_outputs_pass(shape, dtype, skewed):
  arena, ins, device = make(shape, dtype, skew_sets(dtype)[skewed])
  bad, outs = arena.check(device)
  assert bad == [] and sorted(outs) == ['out:b', 'out:c']
  # first and last element of each output, and a full overwrite: valid box or not
  n = cells(shape)
  for name in ('out:b', 'out:c'):
    store(device, arena, name, 0, 3)
    store(device, arena, name, n - 1, 5)
  bad, outs = arena.check(device)
  assert bad == []
  assert outs['out:b'].reshape(-1)[0] == 3 and outs['out:c'].reshape(-1)[-1] == 5
  arena.view(device, 'out:b')[...] = 0
  arena.view(device, 'out:c')[...] = 1
  bad, outs = arena.check(device)
  assert bad == [] and (outs['out:b'] == 0).all() and (outs['out:c'] == 1).all()


@pytest.mark.parametrize('shape,dtype,skewed', CASES)
@pytest.mark.parametrize('name', ['in:a', 'in:w', 'out:b', 'out:c'])
def test_one_element_directly_after_the_last_array_element_fails(shape, dtype, skewed, name):
  arena, ins, device = make(shape, dtype, skew_sets(dtype)[skewed])
  flip(device, arena, name, cells(shape))
  bad, _ = arena.check(device)
  assert len(bad) == 1 and 'guard' in bad[0], bad
  # the report places the damage: it starts at byte +0 past the end of this array
  assert 'bytes +0 .. +' in bad[0] and 'past the end of %s ' % name in bad[0], bad


@pytest.mark.parametrize('shape,dtype,skewed', CASES)
@pytest.mark.parametrize('name', ['in:a', 'in:w', 'out:b', 'out:c'])
def test_one_element_directly_before_the_first_array_element_fails(shape, dtype, skewed, name):
  arena, ins, device = make(shape, dtype, skew_sets(dtype)[skewed])
  flip(device, arena, name, -1)
  bad, _ = arena.check(device)
  assert len(bad) == 1 and 'guard' in bad[0], bad
  assert '.. -1 before the start of %s ' % name in bad[0], bad


@pytest.mark.parametrize('shape,dtype,skewed', CASES)
def test_one_byte_in_the_middle_of_any_guard_fails(shape, dtype, skewed):
  arena, ins, clean = make(shape, dtype, skew_sets(dtype)[skewed])
  for i, g in enumerate(arena.guards):
    device = clean.copy()
    at = g['offset'] + g['nbytes'] // 2
    device[at] ^= 0x10
    bad, _ = arena.check(device)
    assert len(bad) == 1 and bad[0].startswith('guard %d ' % i), bad
    assert ': 1 bytes changed' in bad[0]
  # a whole row one row past the end of the last array: the report says how far
  device = clean.copy()
  last = arena.arrays[-1]
  row = last['shape'][-1] * last['dtype'].itemsize
  at = last['offset'] + last['nbytes'] + row
  device[at:at + row] ^= 0xff
  bad, _ = arena.check(device)
  assert len(bad) == 1 and 'bytes +%d .. +%d past the end of out:c' % (row, 2 * row - 1) in bad[0]
  assert '%d bytes changed' % row in bad[0] and '(1.00 .. 2.00 rows' in bad[0]


@pytest.mark.parametrize('shape,dtype,skewed', CASES)
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_one_changed_input_element_fails(shape, dtype, skewed, where):
  arena, ins, device = make(shape, dtype, skew_sets(dtype)[skewed])
  n = cells(shape)
  element = dict(first=0, middle=n // 2, last=n - 1)[where]
  flip(device, arena, 'in:w', element)
  bad, _ = arena.check(device)
  assert len(bad) == 1 and bad[0].startswith('input in:w was written'), bad
  assert 'in 1 elements' in bad[0]
  assert 'first element %s,' % (tuple(int(v) for v in np.unravel_index(element, shape)),) \
      in bad[0], bad
  assert np.array_equal(arena.view(device, 'in:a'), ins[0])


def test_positive_zero_rewritten_as_negative_zero_fails():
  """Bits are compared, not values: == would call this input unchanged."""
  shape = (70, 257)
  arena = gpu_util.Arena([('in:a', 'in', shape, np.float32), ('out:b', 'out', shape, np.float32)],
                         skews=[4, 20])
  a = np.random.default_rng(1).random(shape, dtype=np.float32)
  a[33, 100] = 0.0
  device = arena.image({'in:a': a}).copy()
  assert arena.check(device)[0] == []
  arena.view(device, 'in:a')[33, 100] = -0.0
  assert np.array_equal(arena.view(device, 'in:a'), a)          # equal as values ...
  bad, _ = arena.check(device)
  assert len(bad) == 1 and bad[0].startswith('input in:a was written: 1 bytes in 1 elements'), bad
  assert 'first element (33, 100), last (33, 100)' in bad[0]
  # and a NaN rewritten with another payload
  a[5, 5] = np.nan
  device = arena.image({'in:a': a}).copy()
  arena.view(device, 'in:a').view(np.uint32)[5, 5] ^= 1
  assert len(arena.check(device)[0]) == 1


def test_each_violation_is_reported_on_its_own():
  shape = (40, 100)
  arena, ins, device = make(shape, np.float32, gpu_util.pool_skews(4, 4))
  store(device, arena, 'out:b', -1, 1.0)
  store(device, arena, 'out:c', cells(shape), 1.0)
  store(device, arena, 'in:a', 17, 2.0)
  bad, _ = arena.check(device)
  assert len(bad) == 3 and sum(b.startswith('guard') for b in bad) == 2


def test_pool_skews():
  assert gpu_util.pool_skews(4, 4) == [4, 20, 36, 52]
  assert gpu_util.pool_skews(3, 2) == [2, 18, 34]
  assert gpu_util.pool_skews(5, 4)[4] == 4
  with pytest.raises(AssertionError):       # element alignment is the floor
    gpu_util.Arena([('a', 'in', (4, 4), np.float32)], skews=[2])
