"""LDS plane-ring kernels (soda_hip/codegen/kernel_stream3d_lds.py with ring=True) on a real
MI355X, all through the C ABI from `<app>.ldsr.hsaco` under a depth limit of 1: the
reference's fixtures array for array, shapes taken from the entry's own constants - every
output on its own box against the oracle, the whole arrays against the per-stage run -, box
depths at which the plane loop leaves at every unrolled step, two iterations, the sweep's
memory contract in guarded arenas, full-width operands, and the run-time compile with the
switch.  Every comparison is of bytes (tests/switch_form_gpu.py)."""
import functools

import pytest

import switch_form_gpu as harness

pytestmark = pytest.mark.gpu

APPS = ('cross3d', 'skewcross3d', 'coupled3d')


def name_of(spec):
  return '%s_fused_k1r%s' % (spec['app_name'], 'f' if len(spec['outputs']) > 1 else '')


def _check(fused, spec):
  (k,) = fused
  assert len(k['lds_ring']) == k['lds_planes'] and all(k['period'] % s == 0
                                                       for s in k['lds_ring'])
  assert k.get('fields') == (len(spec['outputs']) if len(spec['outputs']) > 1 else None)


# coupled3d's velc is handed on: its box never shrinks, the whole array is compared
FORM = harness.Form(
    keyword='lds_ring', family='lds3d_ring', fixtures=lambda app: 8,
    kernels=lambda spec: [(name_of(spec), 1)], limit=lambda spec: 1,
    margins=harness.hull_margins, check=_check, whole=lambda name, iterate: name == 'velc')


opened = functools.partial(harness.opened, FORM)
check_shape = functools.partial(harness.check_shape, FORM)


def entry_of(prog):
  (k,) = harness.fused_of(FORM, prog)
  return k


def shapes_of(prog, iterate):
  return harness.shapes_of(FORM, entry_of(prog), prog.spec, iterate)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  harness.fixtures(FORM, app)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every shape of shapes_of at one iteration."""
  prog, orc = opened(app)
  for shape in shapes_of(prog, 1):
    check_shape(prog, orc, shape, 1)


@pytest.mark.parametrize('app', APPS)
def test_the_plane_loop_leaves_at_every_unrolled_step(app):
  """What the ring adds: one tile, box depths of 1 to `period` planes.  A chunk of `depth`
  planes walks fill_rows + depth steps (the shortest chunk is 8 planes: the deepest boxes
  may be cut in two, which leave at other steps still), so the plane loop leaves at every
  unrolled step and every LDS slot is the last one filled."""
  prog, orc = opened(app)
  k = entry_of(prog)
  mx, my, mz = FORM.margins(prog.spec, 1)
  left_at = set()
  for depth in range(1, k['period'] + 1):
    left_at.add((k['fill_rows'] + depth) % k['period'])
    check_shape(prog, orc, (mz + depth, my + 3, mx + 5), 1)
  assert left_at == set(range(k['period']))


@pytest.mark.parametrize('app', APPS)
def test_iterated(app):
  """Two iterations: the ping-pong of every field, extras that grow and boxes that shrink,
  on the smallest and on the ragged shape.  coupled3d's velc is compared on the whole array
  (FORM.whole)."""
  prog, orc = opened(app)
  shapes = shapes_of(prog, 2)
  for shape in (shapes[0], shapes[-1]):
    check_shape(prog, orc, shape, 2)


@pytest.mark.parametrize('app', APPS)
def test_memory_contract(app):
  """The ragged shape, two iterations, from the pool allocator's placement and from
  multiples of 16 bytes."""
  harness.memory_contract(FORM, app, 2, ((-1, ('pool', 'sixteen')),))


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """In float (cross3d, coupled3d) and in double (skewcross3d), two iterations."""
  harness.full_width_operands(FORM, app, 2, 'double' if app == 'skewcross3d' else 'float')


def test_run_time_compile_with_the_switch():
  harness.run_time_compile(FORM, 'cross3d', 2, ['stage'])
