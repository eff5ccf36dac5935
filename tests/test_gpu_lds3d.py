"""LDS-plane kernels for high-order 3-D stencils (soda_hip/codegen/kernel_stream3d_lds.py) on
a real MI355X, all through the C ABI from `<app>.lds.hsaco`: the reference's fixtures array
for array, shapes taken from the entry's own constants against the oracle and against the
per-stage run, the sweep's memory contract in guarded arenas, full-width operands, and the
run-time compile with the switch.  Every comparison is of bytes (tests/switch_form_gpu.py)."""
import functools

import pytest

import gpu_util
import switch_form_gpu as harness
from switch_form_gpu import SHORTEST_CHUNK  # noqa: F401  (read from here by other modules)

pytestmark = pytest.mark.gpu

APPS = ('star3d', 'iso3dfd', 'skewstar3d')
# one kernel in the default schedule (depth limit 0); one output: the margins are its box's
FORM = harness.Form(
    keyword='lds_planes', family='lds3d',
    fixtures=lambda app: 4 if app == 'iso3dfd' else 8,
    kernels=lambda spec: [(spec['app_name'] + '_fused_k1l', 1)],
    limit=lambda spec: 0, margins=harness.box_margins)


opened = functools.partial(harness.opened, FORM)
check_shape = functools.partial(harness.check_shape, FORM)


def shapes_of(prog, iterate):
  (k,) = harness.fused_of(FORM, prog)
  return harness.shapes_of(FORM, k, prog.spec, iterate)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  harness.fixtures(FORM, app)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every shape of shapes_of at the program's first iteration: the box against the oracle,
  the whole array against the per-stage run."""
  prog, orc = opened(app)
  for shape in shapes_of(prog, 1):
    check_shape(prog, orc, shape, 1)


@pytest.mark.parametrize('iterate', (2, 3, 4))
def test_star3d_iterated(iterate):
  """The shrinking boxes and the ping-pong: the smallest and the ragged shape."""
  prog, orc = opened('star3d')
  shapes = shapes_of(prog, iterate)
  for shape in (shapes[0], shapes[-1]):
    check_shape(prog, orc, shape, iterate)


def test_skewstar3d_iterated():
  prog, orc = opened('skewstar3d')
  check_shape(prog, orc, shapes_of(prog, 3)[-1], 3)


@pytest.mark.parametrize('app,iterate', [('star3d', 1), ('star3d', 3), ('iso3dfd', 1),
                                         ('skewstar3d', 2)])
def test_memory_contract(app, iterate):
  """The smallest and the ragged shape, from the pool allocator's placement and from
  multiples of 64 and 16 bytes."""
  harness.memory_contract(FORM, app, iterate, ((0, ('pool', 'aligned')),
                                               (-1, ('pool', 'sixteen'))))


@pytest.mark.parametrize('app,iterate', [('star3d', 2), ('iso3dfd', 1), ('skewstar3d', 2)])
def test_full_width_operands(app, iterate):
  """In float (star3d, iso3dfd) and in double (skewstar3d), on gpu_util.wide_inputs_of's
  span for the program."""
  harness.full_width_operands(FORM, app, iterate,
                              'double' if app == 'skewstar3d' else 'float',
                              inputs_of=gpu_util.wide_inputs_of)


def test_run_time_compile_with_the_switch():
  harness.run_time_compile(FORM, 'skewstar3d', 2, ['stage'])
