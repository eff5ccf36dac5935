"""What the codegen tests of the kernel families share (tests/test_*_codegen.py; the bench
tools read code objects with it too): where the tools are, a sample's spec, the notes of a
generated text, and a kernel's resource figures from a code object's notes."""
import os
import re
import subprocess

from soda_hip import frontend
from soda_hip.codegen import kernel
from soda_hip.codegen import spec as specmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, 'tests', 'samples')
HIPCC = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'
SODAC = os.path.join(ROOT, 'soda-compiler_amd', 'sodac')
FIGURES = ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
           'sgpr_count', 'group_segment_fixed_size')


def spec_of(app, **kw):
  path = os.path.join(SAMPLES, app + '.soda')
  if not os.path.exists(path):
    path = os.path.join(SAMPLES, 'extra', app + '.soda')
  return specmod.spec_from_stencil(frontend.load(path, **kw))


def spec_of_text(text):
  return specmod.spec_from_stencil(frontend.loads(text))


def notes_of(text):
  return [l for l in text.splitlines() if l.startswith('// ') and 'not fused' in l]


def without_meta(text):
  return text[:text.index('const char soda_hip_meta[]')]


def code_object_figures(path, kernel_names):
  """{kernel name: {figure: int}} (FIGURES) from the notes of the code object at `path`, for
  those of `kernel_names` it holds; none of them twice."""
  notes = subprocess.check_output([READELF, '--notes', path]).decode()
  out = {}
  for block in notes.split('- .agpr_count'):
    for name in kernel_names:
      if re.search(r'\.name:\s+%s\n' % re.escape(name), block):
        assert name not in out, (name, 'in two blocks')
        out[name] = {key: int(re.search(r'^\s*\.%s:\s+(\d+)' % key, block, re.M).group(1))
                     for key in FIGURES}
  return out


def resource_figures(text, kernel_names, out_path, extra_flags=()):
  """The kernel text compiled for gfx950 into `out_path`: code_object_figures of exactly
  one block per kernel."""
  kernel.compile_to_code_object(text, out_path, extra_flags=list(extra_flags))
  out = code_object_figures(out_path, kernel_names)
  assert sorted(out) == sorted(set(kernel_names)), (sorted(out), kernel_names)
  return out


def static_figures(blob, kname):
  """For the bench tools: FIGURES of one kernel of the code object `blob`, {} where there is
  no code object (or no llvm-readelf, or no such kernel) here."""
  if not (os.path.exists(READELF) and os.path.exists(blob)):
    return {}
  return code_object_figures(blob, [kname]).get(kname, {})


def code_bytes(blob, kname):
  """Size of one kernel's code from the code object's symbol table."""
  symbols = subprocess.check_output([READELF, '-s', blob]).decode()
  m = re.search(r'^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s.*\s%s$' % re.escape(kname), symbols, re.M)
  return int(m.group(1)) if m else 0
