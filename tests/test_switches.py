"""The table of opt-in kernel forms (soda_hip/codegen/switches.py) against everything that
reads it, without a GPU: the command line, kernel.generate's keywords, the generated Python
host, the functions that pass switches on, the samples and INTEGRATION.md."""
import argparse
import inspect
import io
import itertools
import os

import pytest

import __graft_entry__ as entry
from soda_hip.codegen import backend, host_shim, kernel, kernel_stream2d, switches
from soda_hip.runtime import host

from conftest import ROOT
from codegen_util import spec_of

ROWS = switches.SWITCHES
COMBINATIONS = [dict(zip([s.keyword for s in ROWS], bits))
                for bits in itertools.product((False, True), repeat=len(ROWS))]


def test_every_flag_parses_and_reads_back_through_the_table():
  parser = argparse.ArgumentParser()
  backend.add_arguments(parser)
  assert switches.from_args(parser.parse_args([])) == {s.keyword: False for s in ROWS}
  for row in ROWS:
    args = parser.parse_args([row.flag])
    assert getattr(args, row.dest) is True
    assert switches.from_args(args) == {s.keyword: s is row for s in ROWS}
  # the order of `--help` is the order of the table
  text = parser.format_help()
  assert sorted(ROWS, key=lambda s: text.index(s.flag)) == list(ROWS)


def test_every_keyword_is_a_parameter_of_generate():
  parameters = inspect.signature(kernel.generate).parameters
  for row in ROWS:
    assert parameters[row.keyword].default is False


def test_keywords_flags_and_suffixes_are_unique():
  for column in ('keyword', 'flag', 'dest', 'suffix'):
    values = [getattr(s, column) for s in ROWS]
    assert len(set(values)) == len(values) and all(values), column
  assert {s.note for s in ROWS if s.note} <= {s.keyword for s in ROWS}


@pytest.mark.parametrize('on', COMBINATIONS, ids=lambda on: '+'.join(k for k in on if on[k]) or '-')
def test_the_shim_sets_the_depth_limit_where_a_row_needs_it(on):
  """The line is there exactly when a row with `depth_limit` is on; its comment names the
  flags of those rows that were given and no other flag of the table."""
  out = io.StringIO()
  host_shim.print_code(spec_of('grad3d'), out, **on)
  lines = [l for l in out.getvalue().splitlines() if 'program.set_max_depth(1)' in l]
  limiting = [s for s in ROWS if s.depth_limit and on[s.keyword]]
  assert len(lines) == (1 if limiting else 0)
  assert switches.depth_limit(on) == bool(limiting)
  for line in lines:
    comment = line.split('#', 1)[1]
    assert [w for w in comment.split() if w.startswith('--')] == [s.flag for s in limiting]
  for row in ROWS:
    assert (', %s=True' % row.keyword in out.getvalue()) == on[row.keyword]


def test_a_name_that_is_no_row_is_a_type_error():
  with pytest.raises(TypeError, match='no_such_switch'):
    host.open_program(spec=spec_of('jacobi2d'), no_such_switch=True)
  with pytest.raises(TypeError, match='no_such_switch'):
    entry.blob_path('x', no_such_switch=True)
  with pytest.raises(TypeError, match='no_such_switch'):
    host_shim.print_code(spec_of('jacobi2d'), io.StringIO(), no_such_switch=True)
  assert entry.blob_path('x', fuse_outputs=True).endswith('x.fused.hsaco')
  assert entry.blob_path('x', lds_planes=True).endswith('x.lds.hsaco')
  assert entry.blob_path('x', lds_fields=True, fuse_outputs=True).endswith('x.ldsf.hsaco')
  assert entry.blob_path('x').endswith('x.hsaco')


def test_for_program_adds_fuse_outputs_for_one_pass_programs_under_lds_fields():
  """Among the samples the LDS forms are built for (build()'s LDS3D_APPS and LDS_FIELDS_APPS)
  deriv3d alone gets `fuse_outputs` along with `lds_fields`.  The rule is the one build_blob
  and tools/lds3d/lds3d_bench.py applied by hand - a one-pass program with several outputs,
  kernel_stream2d.rectangular - so the other five rectangular samples (grad2d, blend2d,
  grad3d, mix3d, outchain) get it as well, as build_blob(app, lds_fields=True) gave it to
  them before; no other sample does, and no other switch adds anything."""
  samples = os.path.join(ROOT, 'tests', 'samples')
  apps = sorted(f[:-5] for d in (samples, os.path.join(samples, 'extra'))
                for f in os.listdir(d) if f.endswith('.soda'))
  assert set(entry.LDS3D_APPS + entry.LDS_FIELDS_APPS) <= set(apps) and len(apps) > 30
  added = []
  for app in apps:
    spec = spec_of(app)
    got = switches.for_program(spec, lds_fields=True)
    assert got in (dict(lds_fields=True), dict(lds_fields=True, fuse_outputs=True)), app
    assert ('fuse_outputs' in got) == kernel_stream2d.rectangular(spec), app
    if 'fuse_outputs' in got:
      added.append(app)
    for row in ROWS:
      if row.keyword != 'lds_fields':
        assert switches.for_program(spec, **{row.keyword: True}) == {row.keyword: True}, app
    assert switches.for_program(spec) == {}
  assert added == sorted(entry.FUSED_OUTPUT_APPS + ('deriv3d',))
  assert [a for a in added if a in entry.LDS3D_APPS + entry.LDS_FIELDS_APPS] == ['deriv3d']


def test_every_flag_is_documented_in_the_integration_guide():
  with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
    text = f.read()
  for row in ROWS:
    assert '`%s`' % row.flag in text, row.flag
