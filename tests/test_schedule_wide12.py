"""Plans of the headline sweeps with the 12-column-lane kernels in the table
(tests/schedule_probe.cpp, no GPU): boxes and depths add up as before, and a launch that
goes to a `w` kernel has ceil(box width / 720) workgroups along x."""
import test_schedule as ts
from test_schedule import probe  # noqa: F401  (the fixture that builds the probe)


def test_wide12_launches_in_the_headline_plans(probe, tmp_path):  # noqa: F811
  cases = ts.variants([ts.case((16384, 16384), 1000), ts.case((8192, 8192), 100)])
  spec, table = ts.program('jacobi2d', 1000)
  names = [k['name'] for k in table]
  assert 'jacobi2d_fused_k24w' in names and 'jacobi2d_fused_k20w' in names
  wide = 0
  for w, static in ((2, 0), (3, 0)):
    for c, r in ts.plan(probe, tmp_path, 'jacobi2d', 1000, cases, w, static):
      assert r['rc'] == 0, r['error']
      ts.check_depths_and_boxes(spec, table, c, r)
      assert sum(table[l['kernel']]['depth'] for l in r['launches']) == c['iterate']
      for l in r['launches']:
        k = table[l['kernel']]
        if not k['name'].endswith('w'):
          continue
        wide += 1
        assert k['tile'][0] == 720
        origin = l['lo'][0] - l['lo'][0] % k['origin_align']
        assert l['grid'][0] == ts.ceil_div(l['hi'][0] - origin, k['tile'][0])
        if l['lo'][0] % k['origin_align'] == 0:
          assert l['grid'][0] == ts.ceil_div(l['hi'][0] - l['lo'][0], k['tile'][0])
  assert wide > 0      # the measured prices send launches of these sweeps to the form
