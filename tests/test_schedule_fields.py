"""The launch planner with a valid region per input (csrc/schedule.cpp:
build_schedule_fields, behind soda_hip_sweep_fields), on the CPU through a probe built with
the host compiler alone (tests/schedule_fields_probe.cpp).

A program over several fields leaves every field on a box of its own.  Resuming it - k2
iterations from the per-field margins of k1 - must end on exactly the boxes of k1 + k2
iterations in one go (spec.iteration_boxes), launch by launch, with the fused kernels
(each output's box unpacked from the launch's extras) and per stage."""
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
PROGRAMS = {'skewpair2d': [(64, 48), (300, 61)], 'fdtd2d': [(64, 48), (37, 29)],
            'maxwell3d': [(20, 18, 16), (70, 20, 24)]}
TOTAL = 5          # every k1 + k2 <= TOTAL


@pytest.fixture(scope='module')
def probes(tmp_path_factory):
  out = {}
  for name in ('schedule_fields_probe', 'schedule_probe'):
    exe = tmp_path_factory.mktemp('schedule_fields') / name
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I',
                           os.path.join(ROOT, 'include'), '-I', CSRC,
                           os.path.join(ROOT, 'tests', name + '.cpp'),
                           os.path.join(CSRC, 'schedule.cpp'), '-o', str(exe)])
    out[name] = str(exe)
  return out


@functools.lru_cache(maxsize=None)
def program(app):
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  spec = specmod.spec_from_stencil(frontend.load(path, iterate=TOTAL))
  table = kernel.generate(spec)[1]
  return specmod.inline_pointwise(spec), table


def pad4(v, fill):
  return list(v) + [fill] * (4 - len(v))


def header(spec, table):
  n = len(table)
  req = struct.pack('=i', n) + bytes(host.program_desc(spec)) + bytes(host.kernel_descs(table))
  req += struct.pack('=iq', CUS, LDS_PER_CU) + struct.pack('=%di' % n, *[CUS * 2] * n)
  return req + struct.pack('=%di' % n, *[0] * n)


def parse(text, n_cases):
  results = []
  for line in text.splitlines():
    f = line.split()
    if f[0] == 'case':
      results.append(dict(rc=int(f[3]), depth=int(f[7]), error='', launches=[], lines=[]))
    elif f[0] == 'error':
      results[-1]['error'] = line[6:]
    else:
      assert f[0] == 'L'
      results[-1]['lines'].append(line)
      results[-1]['launches'].append(dict(
          kernel=int(f[1]), lo=[int(v) for v in f[3:7]], hi=[int(v) for v in f[8:12]],
          param=[int(v) for v in f[17:21]]))
  assert len(results) == n_cases
  return results


def plan_fields(probes, tmp_path, app, cases):
  """cases: dict(dims, iterate, max_depth, lo=[per input], hi=[per input], entry)."""
  spec, table = program(app)
  req = header(spec, table) + struct.pack('=i', len(cases))
  for c in cases:
    req += struct.pack('=4i4q', c['max_depth'], 0, c['iterate'], c.get('entry', 0),
                       *pad4(c['dims'], 1))
    for side in ('lo', 'hi'):
      for v in c[side]:
        req += struct.pack('=4i', *pad4(v, 0))
  path = tmp_path / (app + '.fields.req')
  path.write_bytes(req)
  out = subprocess.check_output([probes['schedule_fields_probe'], str(path)], text=True)
  return parse(out, len(cases))


def plan_single(probes, tmp_path, app, cases):
  """The same through tests/schedule_probe.cpp: build_schedule, one margin."""
  spec, table = program(app)
  req = header(spec, table) + struct.pack('=i', len(cases))
  for c in cases:
    req += struct.pack('=4i8i4q4i4i', c['max_depth'], 0, c['iterate'], 0, *[0] * 8,
                       *pad4(c['dims'], 1), *pad4(c['lo'][0], 0), *pad4(c['hi'][0], 0))
  path = tmp_path / (app + '.single.req')
  path.write_bytes(req)
  out = subprocess.check_output([probes['schedule_probe'], str(path)], text=True)
  return parse(out, len(cases))


def extras_of(dim, launch, j):
  """{lo of dimension 0 .. dim - 1, hi of dimension 0 .. dim - 1} of output j
  (include/soda_hip.h: soda_hip_args.param)"""
  if dim == 2:
    word = ((launch['param'][1 + j // 2] & (2 ** 64 - 1)) >> (32 * (j % 2))) & 0xffffffff
  else:
    word = launch['param'][1 + j] & (2 ** 64 - 1)
  return [(word >> (8 * i)) & 0xff for i in range(2 * dim)]


def margins_after(spec, k):
  """per input: (lo, hi) of the output that feeds it, after k iterations of a fresh run"""
  dim = spec['dim']
  if k == 0:
    return [((0,) * dim, (0,) * dim) for _ in spec['inputs']]
  return specmod.iteration_field_margins(spec, k)[-1]


def resumed_cases(spec, dims):
  cases = []
  for k1 in range(TOTAL):
    for k2 in range(1, TOTAL - k1 + 1):
      m = margins_after(spec, k1)
      for max_depth in (1, 2, -1):      # fused one deep, fused up to two deep, per stage
        cases.append(dict(dims=dims, iterate=k2, max_depth=max_depth, k1=k1,
                          lo=[lo for lo, _ in m], hi=[hi for _, hi in m]))
  return cases


@pytest.mark.parametrize('app', sorted(PROGRAMS))
def test_resumed_schedules_end_on_the_boxes_of_one_run(probes, tmp_path, app):
  spec, table = program(app)
  dim = spec['dim']
  names = [t['name'] for t in spec['inputs']] + [s['name'] for s in spec['stages']]
  n_in = len(spec['inputs'])
  levels = specmod.iteration_boxes(spec, TOTAL)
  seen = set()
  for dims in PROGRAMS[app]:
    cases = resumed_cases(spec, dims)
    for c, r in zip(cases, plan_fields(probes, tmp_path, app, cases)):
      assert r['rc'] == 0, (c, r['error'])
      launches = r['launches']
      assert launches, c
      fused = [table[l['kernel']]['kind'] == 'fused' for l in launches]
      assert all(fused) == (c['max_depth'] > 0) and (all(fused) or not any(fused)), c
      if all(fused):
        assert r['depth'] <= c['max_depth']
        assert sum(table[l['kernel']]['depth'] for l in launches) == c['iterate']
        done = c['k1']
        for l in launches:
          done += table[l['kernel']]['depth']
          own = []
          for j, o in enumerate(spec['outputs']):
            ex = extras_of(dim, l, j)
            olo, ohi = levels[done - 1][o]
            box = [(l['lo'][d] - ex[d], l['hi'][d] + ex[dim + d]) for d in range(dim)]
            # the unpacked box: the output's own box of ONE run of `done` iterations,
            # inside the array
            assert box == [(-olo[d], dims[d] - ohi[d]) for d in range(dim)], (c, j, done)
            assert all(0 <= a < b <= dims[d] for d, (a, b) in enumerate(box))
            own.append(box)
          # the launch's box is the intersection of the outputs' boxes
          for d in range(dim):
            assert l['lo'][d] == max(b[d][0] for b in own)
            assert l['hi'][d] == min(b[d][1] for b in own)
          seen.add((c['k1'], done - c['k1'], 'fused'))
      else:
        assert len(launches) == c['iterate'] * len(spec['stages'])
        for i, l in enumerate(launches):
          it, s = divmod(i, len(spec['stages']))
          assert table[l['kernel']]['stage'] == n_in + s
          blo, bhi = levels[c['k1'] + it][names[n_in + s]]
          for d in range(dim):
            assert l['lo'][d] == -blo[d] and l['hi'][d] == dims[d] - bhi[d]
            assert 0 <= l['lo'][d] < l['hi'][d] <= dims[d]
        seen.add((c['k1'], c['iterate'], 'staged'))
  for k1 in range(TOTAL):
    for k2 in range(1, TOTAL - k1 + 1):
      assert (k1, k2, 'fused') in seen and (k1, k2, 'staged') in seen


@pytest.mark.parametrize('app', sorted(PROGRAMS))
def test_one_margin_for_all_inputs_is_the_single_margin_plan(probes, tmp_path, app):
  """Zero margins, and one margin repeated for every input: the per-field entry, the
  single-margin entry called on the same planner after resumed compositions have filled
  its memo tables, and the single-margin entry on a planner of its own print the same
  launches, byte for byte."""
  spec, _ = program(app)
  dim = spec['dim']
  n_in = len(spec['inputs'])
  for dims in PROGRAMS[app]:
    flat = []
    for lo, hi in (((0,) * dim, (0,) * dim),
                   (tuple(1 + d % 2 for d in range(dim)), tuple(2 - d % 2 for d in range(dim)))):
      for iterate in (1, 3):
        for max_depth in (2, -1):
          flat.append(dict(dims=dims, iterate=iterate, max_depth=max_depth,
                           lo=[lo] * n_in, hi=[hi] * n_in))
    mixed = []
    for c in flat:      # a resumed composition in between, then both entries
      m = margins_after(spec, 2)
      mixed += [dict(c, lo=[lo for lo, _ in m], hi=[hi for _, hi in m]), c, dict(c, entry=1)]
    got = plan_fields(probes, tmp_path, app, mixed)
    want = plan_single(probes, tmp_path, app, flat)
    for i, w in enumerate(want):
      assert w['rc'] == 0 and w['lines']
      assert got[3 * i + 1]['lines'] == w['lines']
      assert got[3 * i + 2]['lines'] == w['lines']
      assert got[3 * i]['rc'] == 0 and got[3 * i]['lines'] != w['lines']


@pytest.mark.parametrize('app,dims', [('wave2d', (1000, 48)), ('wave3d', (700, 20, 24))])
def test_an_extra_beyond_a_byte_is_an_error(probes, tmp_path, app, dims):
  """The last input (the field of the step before, which only the first output reads)
  defined 300 cells further in than the other: the second output's box would be more than
  255 cells wider than the launch's box, which the launch arguments cannot say - an error
  under the fused kernels, never a truncated byte; per stage (no extras) the same regions
  plan."""
  spec, _ = program(app)
  dim = spec['dim']
  n_in = len(spec['inputs'])
  zero = (0,) * dim
  lo = [zero] * (n_in - 1) + [(300,) + zero[1:]]
  cases = [dict(dims=dims, iterate=1, max_depth=1, lo=lo, hi=[zero] * n_in),
           dict(dims=dims, iterate=1, max_depth=-1, lo=lo, hi=[zero] * n_in),
           dict(dims=dims, iterate=1, max_depth=1, lo=[zero] * n_in, hi=lo)]
  fused, staged, high = plan_fields(probes, tmp_path, app, cases)
  assert fused['rc'] == -22 and 'limit 255' in fused['error'], fused
  assert high['rc'] == -22 and 'limit 255' in high['error'], high
  assert staged['rc'] == 0 and staged['launches']
  # 255 itself still fits
  lo = [zero] * (n_in - 1) + [(255,) + zero[1:]]
  ok, = plan_fields(probes, tmp_path, app,
                    [dict(dims=dims, iterate=1, max_depth=1, lo=lo, hi=[zero] * n_in)])
  assert ok['rc'] == 0 and ok['launches']
  assert max(max(extras_of(dim, ok['launches'][0], j)) for j in range(len(spec['outputs']))) == 255
