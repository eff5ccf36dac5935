"""The launch planner (soda-compiler_amd/csrc/schedule.cpp) on the CPU: it is pure
arithmetic over the program, the kernel table and four device facts, so a probe built
with the host compiler alone (tests/schedule_probe.cpp) plans full-size sweeps here and
every launch is checked: depths, boxes, output extras, buffer routing, chunks and the LDS
padding, XCD placements, folded rows, the edge-slack origin."""
import functools
import os
import struct
import subprocess

import pytest

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod
from soda_hip.runtime import host

from conftest import ROOT, SAMPLES

CSRC = os.path.join(ROOT, 'soda-compiler_amd', 'csrc')
CUS = 256
LDS_PER_CU = 160 * 1024
FACTS = [(w, static) for w in (1, 2, 4) for static in (0, 64 * 1024)]
BEYOND_CACHE = 288.0 * 1024 * 1024      # schedule.h: kBeyondCacheBytes
FIELDS = ('wave2d', 'fdtd2d', 'skewpair2d', 'mixpair2d')


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  exe = tmp_path_factory.mktemp('schedule') / 'schedule_probe'
  # the host compiler alone: no ROCm include path, no HIP library
  subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I',
                         os.path.join(ROOT, 'include'), '-I', CSRC,
                         os.path.join(ROOT, 'tests', 'schedule_probe.cpp'),
                         os.path.join(CSRC, 'schedule.cpp'), '-o', str(exe)])
  return str(exe)


@functools.lru_cache(maxsize=None)
def program(app, iterate):
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  spec = specmod.spec_from_stencil(frontend.load(path, iterate=iterate))
  table = kernel.generate(spec)[1]
  # the plan runs the lowered program the kernels were generated from (host.Program)
  return specmod.inline_pointwise(spec), table


def case(dims, iterate, max_depth=0, split=()):
  return dict(dims=tuple(dims), iterate=iterate, max_depth=max_depth, split=tuple(split))


def variants(cases):
  """Every case with out_final_only off and on, on a fresh array and on one whose valid
  region carries margins."""
  out = []
  for c in cases:
    n = len(c['dims'])
    for final_only in (0, 1):
      for lo, hi in (((0,) * n, (0,) * n), (tuple(1 + d % 2 for d in range(n)),
                                             tuple(2 - d % 2 for d in range(n)))):
        out.append(dict(c, final_only=final_only, valid_lo=lo, valid_hi=hi))
  return out


def plan(probe, tmp_path, app, gen_iterate, cases, w, static):
  """Plans `cases` of one program under one set of device facts: [(case, result)],
  result = dict(rc, error, needs, depth, launches=[dict]) as the probe prints it."""
  spec, table = program(app, gen_iterate)
  n = len(table)
  pad4 = lambda v, fill: list(v) + [fill] * (4 - len(v))
  req = struct.pack('=i', n) + bytes(host.program_desc(spec)) + bytes(host.kernel_descs(table))
  req += struct.pack('=iq', CUS, LDS_PER_CU) + struct.pack('=%di' % n, *[CUS * w] * n)
  req += struct.pack('=%di' % n, *[static] * n) + struct.pack('=i', len(cases))
  for c in cases:
    req += struct.pack('=4i8i4q4i4i', c['max_depth'], c['final_only'], c['iterate'],
                       len(c['split']), *(list(c['split']) + [0] * (8 - len(c['split']))),
                       *pad4(c['dims'], 1), *pad4(c['valid_lo'], 0), *pad4(c['valid_hi'], 0))
  path = tmp_path / ('%s_%d_%d_%d.req' % (app, gen_iterate, w, static))
  path.write_bytes(req)
  results = []
  for line in subprocess.check_output([probe, str(path)], text=True).splitlines():
    f = line.split()
    if f[0] == 'case':
      results.append(dict(rc=int(f[3]), depth=int(f[7]), needs=[int(v) for v in f[9:12]],
                          error='', launches=[]))
    elif f[0] == 'error':
      results[-1]['error'] = line[6:]
    else:
      assert f[0] == 'L'
      results[-1]['launches'].append(dict(
          kernel=int(f[1]), lo=[int(v) for v in f[3:7]], hi=[int(v) for v in f[8:12]],
          grid=[int(v) for v in f[13:16]], param=[int(v) for v in f[17:21]],
          lds=int(f[22]), est_us=float(f[24]), buf=f[26:]))
  assert len(results) == len(cases)
  return list(zip(cases, results))


def ceil_div(a, b):
  return -(-a // b)


def tensor_names(spec):
  return [t['name'] for t in spec['inputs']] + [s['name'] for s in spec['stages']]


def hull(spec, boxes):
  """margins of the outputs' boxes of one level, as the planner's output_margins"""
  dim = spec['dim']
  lo = [max(-boxes[o][0][d] for o in spec['outputs']) for d in range(dim)]
  hi = [max(boxes[o][1][d] for o in spec['outputs']) for d in range(dim)]
  return lo, hi


def extras_of(launch, j):
  word = ((launch['param'][1 + j // 2] & (2 ** 64 - 1)) >> (32 * (j % 2))) & 0xffffffff
  return [(word >> (8 * i)) & 0xff for i in range(4)]


def steps_of(spec, table, launches):
  """The launches grouped into the sweep's steps: one fused launch, or the launches of
  one iteration's stages."""
  steps = []
  for l in launches:
    k = table[l['kernel']]
    if k['kind'] == 'fused' or not steps or steps[-1][0]['buf'] != l['buf'] or \
        table[steps[-1][-1]['kernel']]['stage'] >= k['stage']:
      steps.append([])
    steps[-1].append(l)
  return steps


def check_depths_and_boxes(spec, table, c, r):
  dim, dims = spec['dim'], c['dims']
  names = tensor_names(spec)
  n_in = len(spec['inputs'])
  launches = r['launches']
  fused = [table[l['kernel']]['kind'] == 'fused' for l in launches]
  assert all(fused) or not any(fused)
  levels = specmod.iteration_boxes(spec, c['iterate'])
  for l in launches:
    for d in range(dim):      # inside the array and not empty
      assert 0 <= l['lo'][d] < l['hi'][d] <= dims[d]
    assert l['lo'][dim:] == [0] * (4 - dim) and l['hi'][dim:] == [1] * (4 - dim)
  if all(fused):
    assert sum(table[l['kernel']]['depth'] for l in launches) == c['iterate']
    assert r['depth'] == max(table[l['kernel']]['depth'] for l in launches)
    if c['max_depth'] > 0:
      assert r['depth'] <= c['max_depth']
    done = 0
    for l in launches:
      done += table[l['kernel']]['depth']
      mlo, mhi = hull(spec, levels[done - 1])
      for d in range(dim):
        assert l['lo'][d] == c['valid_lo'][d] + mlo[d]
        assert l['hi'][d] == dims[d] - c['valid_hi'][d] - mhi[d]
      if dim == 2 and len(spec['outputs']) > 1:
        for j, o in enumerate(spec['outputs']):
          ex = extras_of(l, j)
          assert all(0 <= v <= 255 for v in ex)
          olo, ohi = levels[done - 1][o]
          for d in range(2):      # unpacked, the output's own box: inside the array too
            assert l['lo'][d] - ex[d] == c['valid_lo'][d] - olo[d] >= 0
            assert l['hi'][d] + ex[2 + d] == dims[d] - c['valid_hi'][d] - ohi[d] <= dims[d]
        for j in range(len(spec['outputs']), 6):
          assert extras_of(l, j) == [0, 0, 0, 0]
  else:
    assert c['max_depth'] <= 0 or not any(k['kind'] == 'fused' and k['depth'] == 1
                                          for k in table)
    assert r['depth'] == 1
    assert len(launches) == c['iterate'] * len(spec['stages'])
    for i, l in enumerate(launches):
      it, s = divmod(i, len(spec['stages']))
      assert table[l['kernel']]['stage'] == n_in + s
      blo, bhi = levels[it][names[n_in + s]]
      for d in range(dim):
        assert l['lo'][d] == c['valid_lo'][d] - blo[d]
        assert l['hi'][d] == dims[d] - c['valid_hi'][d] - bhi[d]


def check_routing(spec, table, c, r):
  n_in, n_out = len(spec['inputs']), len(spec['outputs'])
  names = tensor_names(spec)
  out_index = [names.index(o) for o in spec['outputs']]
  steps = steps_of(spec, table, r['launches'])
  m = len(steps)
  written = None
  for i, step in enumerate(steps):
    buf = step[0]['buf']
    for l in step:
      assert l['buf'] == buf
      named = [b for b in l['buf'] if b[0] != '-']
      assert len(set(named)) == len(named)      # nothing read and written in one launch
    reads = buf[:n_in]
    writes = [buf[t] for t in out_index]
    if i == 0:
      assert reads == ['i%d' % j for j in range(n_in)]
    elif n_in == n_out:
      assert reads == written       # exactly what the step before wrote
    kinds = {b[0] for b in writes}
    assert len(kinds) == 1 and [int(b[1:]) for b in writes] == list(range(n_out))
    if i == m - 1:
      assert kinds == {'o'}
    elif c['final_only']:
      assert kinds <= {'a', 'b'}
    else:
      assert kinds <= {'a', 'o'}
    for t, b in enumerate(buf[n_in:]):
      local = table[step[0]['kernel']]['kind'] == 'stage' and n_in + t not in out_index
      assert (b == 'l%d' % t) if local else (b[0] != 'l' and (n_in + t in out_index) == (b != '-0'))
    written = writes
  tags = {b[0] for l in r['launches'] for b in l['buf']}
  assert 'b' not in tags or (c['final_only'] and m > 2)
  assert r['needs'] == [int('a' in tags), int('b' in tags), int('l' in tags)]
  assert ('a' in tags) == (m > 1) and ('b' in tags) == (bool(c['final_only']) and m > 2)


def real_tiles(spec, k, l):
  """tiles along x, y and chunks along z of a 3-D launch, from the box alone"""
  ext = [l['hi'][d] - l['lo'][d] for d in range(3)]
  nx = ceil_div(ext[0] + (l['lo'][0] % k['origin_align'] if k.get('origin_align', 0) > 1 else 0),
                k['tile'][0])
  return nx, ceil_div(ext[1], k['tile'][1]), ceil_div(ext[2], l['param'][0])


def check_edge_slack(k, l):
  """include/soda_hip.h, soda_hip_kernel.edge_slack: the three cases"""
  slack, align, tile = k['edge_slack'], k['origin_align'], k['tile'][0]
  lo, hi = l['lo'][0], l['hi'][0]
  down = lambda v: v - v % align
  x0 = down(lo + slack)
  nx = max(1, ceil_div(hi - x0 - slack, tile))
  if (nx == 1 and hi > x0 + tile) or hi <= x0:
    x0 = down(lo)
    nx = max(1, ceil_div(hi - x0 - slack, tile))
  assert (l['param'][1] >> 32, l['param'][2] & 0xffff) == (x0, nx)
  # and what the kernel makes of it covers the box: the first tile, when it starts inside
  # the box, reaches `slack` columns back; otherwise the last one `slack` columns on
  shifted = lo < x0
  assert x0 - (slack if shifted else 0) <= lo
  assert x0 + nx * tile + (0 if shifted and nx == 1 else slack) >= hi
  return nx


def check_placement(spec, k, l, w):
  """3-D kernels that place their tiles themselves: decoded as the kernels do
  (kernel_stream3d_wp.py / kernel_stream3d_blk.py: L = workgroup id)."""
  assert l['grid'][1:] == [1, 1] and l['grid'][0] % 8 == 0
  sx, sy = l['param'][1] & 0xffff, (l['param'][1] >> 16) & 0xffff
  nsx, nsy = l['param'][2] & 0xffff, l['param'][2] >> 16
  runs = l['param'][3]
  nx, ny, nz = real_tiles(spec, k, l)
  if k.get('edge_slack', 0) > 0 and k.get('origin_align', 0) > 1 and k['xcd_tiles'] < 0:
    nx = check_edge_slack(k, l)
  else:
    assert l['param'][1] >> 32 == 0
  if k['xcd_tiles'] < 0:
    assert (sx, sy, nsx, nsy) == (1, 1, nx, ny) and runs == ceil_div(nx * ny * nz, 8)
    assert l['grid'][0] == 8 * runs
  else:
    assert runs == 0 and 1 <= sx * sy <= max(1, k['xcd_tiles'])
    assert (nsx, nsy) == (ceil_div(nx, sx), ceil_div(ny, sy))
    assert l['grid'][0] == ceil_div(nsx * nsy * nz, 8) * 8 * sx * sy
  seen = set()
  per_xcd = [0] * 8
  s = sx * sy
  for wg in range(l['grid'][0]):
    i = wg >> 3
    g = (wg & 7) * runs + i if runs else (i // s) * 8 + (wg & 7)
    within = 0 if runs else i % s
    tile = ((g % nsx) * sx + within % sx, ((g // nsx) % nsy) * sy + within // sx,
            g // (nsx * nsy))
    if tile[0] < nx and tile[1] < ny and tile[2] < nz:
      assert tile not in seen
      seen.add(tile)
      per_xcd[wg & 7] += 1
  assert len(seen) == nx * ny * nz      # every real tile once, padding ids on none
  even = ceil_div(nx * ny * nz, 8)
  assert max(per_xcd) <= even + max(1, even * 3 // 100)


def check_grids(spec, table, c, r, w, static):
  dim = spec['dim']
  sizes = specmod.tensor_c_types(spec)
  io_bytes = sum(specmod.ELEM_SIZE[sizes[t['name']]] for t in spec['inputs']) + \
      sum(specmod.ELEM_SIZE[sizes[o]] for o in spec['outputs'])
  for l in r['launches']:
    k = table[l['kernel']]
    lo, hi = list(l['lo']), list(l['hi'])
    if k['kind'] == 'fused' and dim == 2 and len(spec['outputs']) > 1:
      ex = [extras_of(l, j) for j in range(len(spec['outputs']))]
      for d in range(2):      # the grid covers the union of the outputs' boxes
        lo[d] -= max(e[d] for e in ex)
        hi[d] += max(e[2 + d] for e in ex)
    ext = [hi[d] - lo[d] for d in range(dim)]
    assert l['grid'][1] <= 65535 and l['grid'][2] <= 65535
    streaming = k.get('fill_rows', 0) > 0 and dim >= 2
    placed = dim == 3 and k.get('xcd_tiles', 0) != 0
    if streaming:
      chunk = l['param'][0]
      assert chunk >= 1
      if not placed:
        chunks = l['grid'][dim - 1]
        assert chunk * chunks >= ext[dim - 1] > chunk * (chunks - 1)
      cells = 1.0
      for e in ext:
        cells *= e
      cap = k.get('stream_wgs_per_cu', 0) if cells * io_bytes > BEYOND_CACHE else 0
      if cap > 0 and CUS * w > cap * CUS and static * cap <= LDS_PER_CU:
        total = static + l['lds']
        assert total * cap <= LDS_PER_CU < total * (cap + 1)
      else:         # no cap, one the occupancy keeps anyway, or one static LDS rules out
        assert l['lds'] == 0
    else:
      assert l['lds'] == 0 and l['est_us'] == 0
    if placed:
      check_placement(spec, k, l, w)
    elif k['kind'] == 'stage':
      rows = 1
      for e in ext[1:]:
        rows *= e
      if dim > 3 or (dim > 1 and max(ext[1:]) > 65535):
        assert l['grid'][1] * l['grid'][2] >= rows and l['param'][0] == 1
        assert l['grid'][1] == min(rows, 65535)
      else:
        assert l['grid'][1:dim] == ext[1:3]
      assert l['grid'][0] * k['tile'][0] >= ext[0]
    elif not streaming or dim == 2:
      align = k.get('origin_align', 0)
      assert l['grid'][0] == ceil_div(ext[0] + (lo[0] % align if align > 1 else 0), k['tile'][0])
    # kernels that move their tiles inside the array instead of guarding them
    if k.get('min_extent', [0, 0])[0] > 0:
      assert c['dims'][0] >= k['min_extent'][0] and c['dims'][1] >= k['min_extent'][1]
      assert dim < 3 or c['dims'][0] * c['dims'][1] < 2 ** 30 - 16


def check_all(probe, tmp_path, app, cases, facts=FACTS):
  by_iterate = {}
  for c in variants(cases):
    by_iterate.setdefault(c['iterate'], []).append(c)
  planned = []
  for iterate, group in by_iterate.items():
    spec, table = program(app, iterate)
    for w, static in facts:
      for c, r in plan(probe, tmp_path, app, iterate, group, w, static):
        assert r['rc'] == 0, (c, r['error'])
        assert r['launches']
        check_depths_and_boxes(spec, table, c, r)
        check_routing(spec, table, c, r)
        check_grids(spec, table, c, r, w, static)
        planned.append((c, r, table))
  return planned


def test_jacobi2d(probe, tmp_path):
  planned = check_all(probe, tmp_path, 'jacobi2d', [
      case((16384, 16384), 1000), case((8192, 8192), 100), case((12288, 8192), 25),
      case((256, 600000), 1, max_depth=1), case((256, 600000), 1, max_depth=-1),
      case((37, 29), 4), case((37, 29), 4, max_depth=-1),
      # (three steps: the fewest that need the plan's second array under out_final_only)
      case((37, 29), 3, max_depth=1), case((37, 29), 3, max_depth=-1),
      # (the shallow kernels are the ones whose calibration record names a cap)
      case((16384, 16384), 2, max_depth=2)])
  for c, r, table in planned:
    kinds = {table[l['kernel']]['kind'] for l in r['launches']}
    assert kinds == ({'stage'} if c['max_depth'] < 0 else {'fused'})
    if c['dims'] == (256, 600000) and c['max_depth'] == 1:
      # chunks never outnumber what grid.y takes
      assert r['launches'][0]['param'][0] >= ceil_div(600000 - 5, 65535)
  # a cap was realised with LDS padding somewhere (and check_grids saw the cases where
  # the occupancy or the static LDS keeps it anyway)
  assert any(l['lds'] > 0 for c, r, t in planned for l in r['launches'])


def test_blur(probe, tmp_path):
  check_all(probe, tmp_path, 'blur', [case((16384, 16384), 1)])


def test_jacobi3d(probe, tmp_path):
  planned = check_all(probe, tmp_path, 'jacobi3d', [case((512, 512, 512), 200),
                                                    case((128, 128, 128), 8),
                                                    case((512, 512, 512), 2, max_depth=2)])
  forms = {(t[l['kernel']].get('xcd_tiles', 0) > 0) - (t[l['kernel']].get('xcd_tiles', 0) < 0)
           for c, r, t in planned for l in r['launches']}
  assert {-1, 1} & forms       # the placements were exercised


def test_heat3d(probe, tmp_path):
  check_all(probe, tmp_path, 'heat3d', [case((64, 64, 64), 20)])


def test_hyper4d_rows_are_folded(probe, tmp_path):
  planned = check_all(probe, tmp_path, 'hyper4d', [case((40, 14, 13, 33), 3),
                                                   case((11, 23, 31, 203), 2)])
  assert all(l['param'][0] == 1 for c, r, t in planned for l in r['launches'])


def test_outchain_more_outputs_than_inputs(probe, tmp_path):
  check_all(probe, tmp_path, 'outchain', [case((64, 48), 1), case((37, 29), 1)])
  spec, table = program('outchain', 1)
  c = variants([case((64, 48), 2)])[0]
  (_, r), = plan(probe, tmp_path, 'outchain', 1, [c], 1, 0)
  assert r['rc'] == -8 and 'as many outputs as inputs' in r['error']


@pytest.mark.parametrize('app', FIELDS)
def test_multi_field_programs(probe, tmp_path, app):
  splits = {1: (1,), 2: (1, 1), 3: (2, 1), 4: (2, 2)}
  cases = [case(dims, iterate, max_depth)
           for dims in ((64, 48), (37, 29)) for iterate in (1, 2, 3, 4)
           for max_depth in (0, 1, 2, 4)]
  cases += [case((64, 48), iterate, 0, split) for iterate, split in splits.items()]
  planned = check_all(probe, tmp_path, app, cases, facts=[(1, 0), (4, 64 * 1024)])
  for c, r, table in planned:
    kinds = {table[l['kernel']]['kind'] for l in r['launches']}
    depths = sorted({k['depth'] for k in table if k['kind'] == 'fused'})
    if not depths:
      assert kinds == {'stage'}
    elif c['max_depth'] == 0 and not c['split']:
      assert kinds == {'stage'}        # not in the default schedule until measured
    else:
      assert kinds == {'fused'}
      if c['split'] and all(d in depths for d in c['split']):
        assert [table[l['kernel']]['depth'] for l in r['launches']] == list(c['split'])


def test_fused_kernels_are_skipped_where_they_cannot_run(probe, tmp_path):
  """Kernels that move their tiles inside the array (min_extent) need an array of that
  size and, in 3-D, planes below 2^30 - 16 cells."""
  spec, table = program('jacobi3d', 8)
  unguarded = lambda l: table[l['kernel']].get('min_extent', [0, 0])[0] > 0
  smallest = min(k['min_extent'][0] for k in table if k.get('min_extent', [0, 0])[0] > 0)
  for dims, iterate, allowed in (((smallest - 1, 96, 40), 8, False),
                                 ((32768, 32768, 8), 1, False),     # 2^30 cells a plane
                                 ((32768, 32764, 8), 1, True)):
    for c, r in plan(probe, tmp_path, 'jacobi3d', 8, variants([case(dims, iterate)]), 2, 0):
      assert r['rc'] == 0, r['error']
      assert any(unguarded(l) for l in r['launches']) == allowed
      check_depths_and_boxes(spec, table, c, r)
      check_routing(spec, table, c, r)
      check_grids(spec, table, c, r, 2, 0)


def test_an_empty_box_is_not_listed(probe, tmp_path):
  spec, table = program('jacobi2d', 4)
  for max_depth, full in ((-1, 4), (1, 4)):
    c = dict(case((6, 6), 4, max_depth), final_only=0, valid_lo=(0, 0), valid_hi=(0, 0))
    (_, r), = plan(probe, tmp_path, 'jacobi2d', 4, [c], 1, 0)
    assert r['rc'] == 0 and 0 < len(r['launches']) < full
    for l in r['launches']:
      assert all(l['lo'][d] < l['hi'][d] for d in range(2))
