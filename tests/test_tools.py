"""tools/: every script that is kept (not under tools/archive/) at least starts - `--help`
prints its usage and exits 0 without touching a GPU, the reference or the network."""
import glob
import importlib.util
import os
import subprocess
import sys

import pytest

from conftest import ROOT

TOOLS = sorted(glob.glob(os.path.join(ROOT, 'tools', '*.py')))
# the reference-plugin check runs under the container's python3.9 with /root/reference
CONTAINER_ONLY = {'check_reference_plugin.py'}


@pytest.mark.parametrize('path', [p for p in TOOLS if os.path.basename(p) not in CONTAINER_ONLY],
                         ids=os.path.basename)
def test_tool_prints_its_usage(path):
  r = subprocess.run([sys.executable, path, '--help'], capture_output=True, text=True,
                     timeout=120)
  assert r.returncode == 0, r.stderr[-1000:]
  assert len(r.stdout.strip()) > 40, r.stdout


def test_far_bench_calls_a_schedule_faster_only_beyond_the_spread():
  """tools/far/far_bench.py's judge(): the rule behind every FASTER of the far-reach forms'
  profiles.  The medians must differ by MORE than the larger max - min of the two series."""
  spec = importlib.util.spec_from_file_location(
      'far_bench', os.path.join(ROOT, 'tools', 'far', 'far_bench.py'))
  far_bench = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(far_bench)
  verdicts = (('faster', [6.0, 7.0, 8.0], 'FASTER'),                # 5 below, spread 2
              ('slower', [16.0, 17.0, 18.0], 'SLOWER'),             # 5 above, spread 2
              ('just below', [9.5, 10.0, 11.5], 'NO DIFFERENCE beyond the spread'),   # 2, 2
              ('just above', [13.0, 14.0, 15.0], 'NO DIFFERENCE beyond the spread'),  # 2, 2
              # 6 below, but of the two spreads the larger counts, and its own is 10
              ('noisy', [2.0, 6.0, 12.0], 'NO DIFFERENCE beyond the spread'))
  times = {name: series for name, series, _ in verdicts}
  times['per-stage'] = [13.0, 11.0, 12.0]                           # median 12, spread 2
  rows = far_bench.judge(times)
  assert list(rows) == list(times)                                  # the report's row order
  assert {name: rows[name]['verdict'] for name, _, _ in verdicts} == \
      {name: verdict for name, _, verdict in verdicts}
  assert rows['faster'] == dict(ms=7.0, min_ms=6.0, max_ms=8.0, speedup=12.0 / 7.0, spread=2.0,
                                verdict='FASTER')
  assert rows['just below']['ms'] == 10.0 and rows['just below']['spread'] == 2.0
  assert rows['just above']['ms'] == 14.0 and rows['just above']['spread'] == 2.0
  assert rows['noisy']['spread'] == 10.0
  assert rows['per-stage'] == dict(ms=12.0, min_ms=11.0, max_ms=13.0, speedup=1.0, spread=2.0,
                                   verdict='')


def test_archive_is_described():
  """Probes whose question is closed live under tools/archive/ with a line each in its
  README (script, question, where the answer is recorded)."""
  names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, 'tools', 'archive',
                                                                     '*.py')))
  text = open(os.path.join(ROOT, 'tools', 'archive', 'README.md')).read()
  assert names and all('`%s`' % n in text for n in names)
  assert len(TOOLS) <= 30
