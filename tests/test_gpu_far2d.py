"""Far-lane 2-D kernels (kernel_stream2d / kernel_fields2d with `hops`; kernel.generate's
`far_lanes`) on a real MI355X, all through the C ABI from `<app>.far.hsaco`: the reference's
fixtures array for array, shapes taken from each entry's own constants - every output on its
own box against the oracle, the whole arrays against the per-stage run -, the sweep's memory
contract in guarded arenas, full-width operands, and the run-time compile with the switch.
Every comparison is of bytes (tests/switch_form_gpu.py).

star2d, dstar2d and skewfar2d run their fused kernels in the default schedule.  acoustic2d's
are kernels over several fields, which the launcher admits only under a positive depth limit
(csrc/schedule.cpp, plans_fused - as for wave2d and every other multi-field program): every
entry point generated with the switch sets that limit (switches.depth_limit_of), and the
fused runs here are those under the same limit, from the same function."""
import functools
import os

import pytest

from soda_hip.codegen import switches
from soda_hip.runtime import host

import gpu_util
import switch_form_gpu as harness

pytestmark = pytest.mark.gpu

APPS = ('star2d', 'dstar2d', 'skewfar2d', 'acoustic2d')
DEPTHS = {'star2d': [1, 2], 'dstar2d': [1, 2, 4], 'skewfar2d': [1, 2], 'acoustic2d': [1, 2]}


def _check(fused, spec):
  assert max(k['halo'][0] for k in fused) > fused[0]['cols']     # a halo wider than one lane


# the depth limit: none (the default schedule) for the single-array programs, the deepest
# kernel's for the one over fields; acoustic2d's pc is handed on at the first iteration
FORM = harness.Form(
    keyword='far_lanes', family='far2d',
    fixtures=lambda app: 4 * (2 if app == 'skewfar2d' else 3),
    kernels=lambda spec: [('%s_fused_k%d' % (spec['app_name'], d), d)
                          for d in DEPTHS[spec['app_name']]],
    limit=lambda spec: max(DEPTHS['acoustic2d']) if len(spec['outputs']) > 1 else 0,
    margins=harness.lowered_hull_margins, check=_check,
    whole=lambda name, iterate: name == 'pc' and iterate == 1)


opened = functools.partial(harness.opened, FORM)
check_shape = functools.partial(harness.check_shape, FORM)
fused_of = functools.partial(harness.fused_of, FORM)
shapes_of = functools.partial(harness.shapes_of, FORM)


@pytest.mark.parametrize('app', APPS)
def test_fixtures(app):
  harness.fixtures(FORM, app)


@pytest.mark.parametrize('app', APPS)
def test_shapes(app):
  """Every kernel of the table on every shape of shapes_of, as many iterations as it fuses."""
  prog, orc = opened(app)
  for k in fused_of(prog):
    for shape in shapes_of(k, prog.spec, k['depth']):
      assert shape[0] * shape[1] <= 2100 * 130
      check_shape(prog, orc, shape, k['depth'], k['depth'])


@pytest.mark.parametrize('app', APPS)
def test_the_schedule_mixes_depths(app):
  """One iteration more than the deepest kernel fuses: the sweep ends in a shallower kernel,
  on the ragged shape."""
  prog, orc = opened(app)
  deep = fused_of(prog)[-1]
  iterate = deep['depth'] + 1
  check_shape(prog, orc, shapes_of(deep, prog.spec, iterate)[-1], iterate, None)


@pytest.mark.parametrize('app', APPS)
def test_memory_contract(app):
  """The ragged shape with the deepest kernel, from the pool allocator's placement and from
  multiples of 16 bytes."""
  deepest = DEPTHS[app][-1]
  harness.memory_contract(FORM, app, deepest, ((-1, ('pool', 'sixteen')),), depth=deepest)


@pytest.mark.parametrize('app', APPS)
def test_full_width_operands(app):
  """In float (star2d, skewfar2d) and in double (dstar2d, acoustic2d), two iterations in the
  depth-2 kernel."""
  harness.full_width_operands(
      FORM, app, 2, 'double' if app in ('dstar2d', 'acoustic2d') else 'float', depth=2)


def test_the_products_limit_admits_the_kernels_over_fields():
  """What a `--hip-far-lanes` product of acoustic2d runs: under the limit its entry points
  set, every launch is one of the far-lane kernels - without it the launcher keeps a program
  over several fields per stage -, and the generated `<app>_test` passes with the switch."""
  prog, _ = opened('acoustic2d')
  spec = prog.spec
  limit, flags = switches.depth_limit_of(spec, dict(far_lanes=True))
  assert (limit, flags) == (2, ['--hip-far-lanes'])
  dims = (301, 53)
  try:
    prog.set_max_depth(limit)
    assert [k['name'] for k, _ in prog.schedule(dims, 3)] == [
        'acoustic2d_fused_k2', 'acoustic2d_fused_k1']
    prog.set_max_depth(0)
    assert all(k['kind'] == 'stage' for k, _ in prog.schedule(dims, 3))
  finally:
    prog.set_max_depth(0)
  blob = os.path.join(gpu_util.BLOBS, 'acoustic2d.far.hsaco')
  assert host.app_test(spec, blob, [301, 53, 0, 0], iterate=3, far_lanes=True) == 0


def test_run_time_compile_with_the_switch():
  harness.run_time_compile(FORM, 'skewfar2d', 2, ['stage', 'stage'], depth=2)
