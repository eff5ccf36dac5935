"""LDS-plane kernels over several outputs (soda_hip/codegen/kernel_stream3d_lds.py with
fields=True) on a real MI355X, all through the C ABI from `<app>.ldsf.hsaco` under a depth
limit of 1: the reference's fixtures array for array, shapes taken from the entry's own
constants - every output on its own box against the oracle, the whole arrays against the
per-stage run -, the ping-pong of three fields over several iterations, the sweep's memory
contract in guarded arenas, full-width operands, and the run-time compile with the switch.
Every comparison is of bytes (tests/switch_form_gpu.py)."""
import functools

import pytest

import switch_form_gpu as harness

pytestmark = pytest.mark.gpu

APPS = ('acoustic3d', 'skewwave3d', 'deriv3d')


def _check(fused, spec):
  assert fused[0]['fields'] == len(spec['outputs'])


FORM = harness.Form(
    keyword='lds_fields', family='lds3d_fields',
    fixtures=lambda app: 4 if app == 'deriv3d' else 8,
    kernels=lambda spec: [(spec['app_name'] + '_fused_k1lf', 1)],
    limit=lambda spec: 1, margins=harness.hull_margins, check=_check)


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
  """Every shape of shapes_of at one iteration."""
  prog, orc = opened(app)
  for shape in shapes_of(prog, 1):
    check_shape(prog, orc, shape, 1)


@pytest.mark.parametrize('app,iterate', [('acoustic3d', 2), ('acoustic3d', 3), ('acoustic3d', 4),
                                         ('skewwave3d', 2), ('skewwave3d', 3)])
def test_iterated(app, iterate):
  """The ping-pong of every field, extras that grow and boxes that shrink with the level: the
  smallest and the ragged shape."""
  prog, orc = opened(app)
  shapes = shapes_of(prog, iterate)
  for shape in (shapes[0], shapes[-1]):
    check_shape(prog, orc, shape, iterate)


@pytest.mark.parametrize('app,iterate', [('acoustic3d', 3), ('skewwave3d', 2), ('deriv3d', 1)])
def test_memory_contract(app, iterate):
  """The smallest and the ragged shape, from the pool allocator's placement and from
  multiples of 64 and 16 bytes."""
  harness.memory_contract(FORM, app, iterate, ((0, ('pool', 'aligned')),
                                               (-1, ('pool', 'sixteen'))))


@pytest.mark.parametrize('app,iterate', [('acoustic3d', 2), ('skewwave3d', 2), ('deriv3d', 1)])
def test_full_width_operands(app, iterate):
  """In float (acoustic3d, deriv3d) and in double (skewwave3d)."""
  harness.full_width_operands(FORM, app, iterate,
                              'double' if app == 'skewwave3d' else 'float')


def test_run_time_compile_with_the_switch():
  harness.run_time_compile(FORM, 'skewwave3d', 2, ['stage', 'stage'])
