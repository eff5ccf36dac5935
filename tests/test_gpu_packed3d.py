"""Packed-cell 3-D kernels (kernel_stream3d_pk; kernel.generate's `packed_cells`) on a real
MI355X, all through the C ABI from `<app>.pk.hsaco`: the reference's fixtures array for array,
shapes taken from each entry's own constants - the output's box against the oracle, the whole
arrays against the per-stage run -, the sweep's memory contract in guarded arenas (where an
over-wide vector store or a misaligned row shows), the whole value range of each element type,
and the run-time compile with the switch.  Every comparison is of bytes
(tests/switch_form_gpu.py).  The kernels run in the default schedule: no depth limit."""
import functools

import pytest

import switch_form_gpu as harness

pytestmark = pytest.mark.gpu

APPS = ('smooth3d', 'skewvol3d', 'sdiff3d', 'castvol3d')
DEPTHS = {'smooth3d': [1, 2], 'skewvol3d': [1], 'sdiff3d': [1], 'castvol3d': [1]}
TYPES = {'smooth3d': 'uint16_t', 'skewvol3d': 'uint8_t', 'sdiff3d': 'int16_t',
         'castvol3d': 'uint16_t'}


def _check(fused, spec):
  for k in fused:      # lane loads of 8 or 16 bytes, the fields of kernel_stream3d's entries
    assert k['cols'] * {'uint8_t': 1}.get(TYPES[spec['app_name']], 2) in (8, 16)
    assert k['tile'][:2] == [4 * k['w_out'] - k['cols'], k['r_out']]


FORM = harness.Form(
    keyword='packed_cells', family='packed3d',
    fixtures=lambda app: 4 * (3 if app == 'smooth3d' else 1),
    kernels=lambda spec: [('%s_fused_k%d' % (spec['app_name'], d), d)
                          for d in DEPTHS[spec['app_name']]],
    limit=lambda spec: 0, margins=harness.box_margins, check=_check)

opened = functools.partial(harness.opened, FORM)
check_shape = functools.partial(harness.check_shape, FORM)
fused_of = functools.partial(harness.fused_of, FORM)
shapes_of = functools.partial(harness.shapes_of, FORM)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  harness.fixtures(FORM, app)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every kernel of the table on every shape of shapes_of, as many iterations as it fuses:
  the one-cell box, one tile plus a row and a column with fewer planes than the fill, the
  chunk seam, the ragged 2 x 3 tiles with clamped loads on all six sides."""
  prog, orc = opened(app)
  for k in fused_of(prog):
    for shape in shapes_of(k, prog.spec, k['depth']):
      assert shape[0] * shape[1] * shape[2] <= 8 << 20
      check_shape(prog, orc, shape, k['depth'], k['depth'])


def test_the_schedule_mixes_depths():
  """smooth3d, three iterations: `_k2` then `_k1`, on the ragged shape."""
  prog, orc = opened('smooth3d')
  deep = fused_of(prog)[-1]
  shape = shapes_of(deep, prog.spec, 3)[-1]
  dims = tuple(reversed(shape))
  assert [k['name'] for k, _ in prog.schedule(dims, 3)] == ['smooth3d_fused_k2',
                                                            'smooth3d_fused_k1']
  check_shape(prog, orc, shape, 3, None)


@pytest.mark.parametrize('app', APPS)
def test_memory_contract(app):
  """The ragged shape with the deepest kernel, from the pool allocator's placement and from
  multiples of 16 bytes: inputs unchanged, guards intact."""
  deepest = DEPTHS[app][-1]
  harness.memory_contract(FORM, app, deepest, ((-1, ('pool', 'sixteen')),), depth=deepest)


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """The whole value range of each type (gpu_util.wide_inputs: uniform over the type, mixed
  signs for int16): two iterations in smooth3d's depth-2 kernel, one in the others'."""
  deepest = DEPTHS[app][-1]
  harness.full_width_operands(FORM, app, deepest, TYPES[app], depth=deepest)


def test_run_time_compile_with_the_switch():
  harness.run_time_compile(FORM, 'castvol3d', 1, ['stage', 'stage'], depth=1)
