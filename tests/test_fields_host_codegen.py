"""The generated C++ host of a program over several fields: `<app>_multi_gpu` drives
soda_hip_run_slab_fields with the static cut (CPU: the text and that it compiles)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, SAMPLES


def run_sodac(*args):
  return subprocess.run([sys.executable, os.path.join(ROOT, 'soda-compiler_amd', 'sodac')] +
                        list(args), capture_output=True, text=True)


@pytest.mark.parametrize('app,n', [('wave2d', 2), ('fdtd2d', 3), ('maxwell3d', 3)])
def test_generated_multi_gpu_host_of_a_multi_field_program_compiles(tmp_path, app, n):
  src = tmp_path / (app + '_host.cpp')
  r = run_sodac(os.path.join(SAMPLES, 'extra', app + '.soda'), '--hip-host-cpp', str(src))
  assert r.returncode == 0, r.stderr
  text = src.read_text()
  assert 'extern "C" int %s_multi_gpu(' % app in text
  assert 'soda_hip_run_slab_fields(' in text and 'soda_hip_run_slab(' not in text
  assert 'slab.cut = SODA_HIP_SLAB_CUT_STATIC;' in text and 'SODA_HIP_SLAB_CUT_RECUT' not in text
  assert 'slab.order = SODA_HIP_SLAB_SERIAL;' in text
  assert 'n_fields = %d;' % n in text and 'soda_hip_plan_field_margins(' in text
  subprocess.check_call(['g++', '-std=c++17', '-fsyntax-only', '-fopenmp', '-Wall', '-Werror',
                         '-DSODA_HIP_MAIN', '-DSODA_HIP_MULTI_GPU',
                         '-D__HIP_PLATFORM_AMD__', '-I', '/opt/rocm/include', '-I',
                         os.path.join(ROOT, 'include'), str(src)])
