#!/usr/bin/env python3
"""One line per case of what kernel.generate() returns: the sha256 of the text, the kernel
names of the table and a digest of the table entries - or, for a case that raises, the
exception.  Needs no GPU and no hipcc.  Two trees that print the same lines generate the
same kernels; run it in both and diff the outputs (a refactoring of the generator's
selection must give zero differing lines, the error lines included).

usage: kernel_text_digests.py [output file]
"""
import glob
import hashlib
import json
import os
import sys

if '--help' in sys.argv or '-h' in sys.argv:
  print(__doc__)
  sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tests')]
from soda_hip import frontend                                   # noqa: E402
from soda_hip.codegen import kernel, spec as specmod            # noqa: E402
# the option sets of the GPU tests come from the tests themselves (importing them needs no GPU)
import test_gpu_memory_contract as contract                     # noqa: E402
import test_gpu_parity as parity                                # noqa: E402

SAMPLES = os.path.join(ROOT, 'tests', 'samples')
ITERATES = (None, 1, 3, 4, 8, 15, 100, 1000)
FAMILIES = ('jacobi2d', 'wave2d', 'jacobi3d', 'denoise3d')      # one program per kernel family
WP = dict(wave_groups=4, pairs=2, vgpr_budget=250)
# (program, iterate, options): the literal sets of tests/*.py and tools/*.py not imported above
LITERAL = [(app, 4 if app in ('jacobi2d', 'seidel2d') else None, dict(max_depth=4))
           for app in parity.APPS] + [
    ('jacobi2d', 8, dict(depths=[8], wave_groups=4)),
    ('jacobi2d', 8, dict(depths=[8], wave_groups=4, pairs=1, vgpr_budget=250)),
    ('jacobi2d', 8, dict(depths=[8], ring=6, **WP)),
    ('jacobi2d', 8, dict(depths=[8], ring=12, max_period=12, **WP)),
    ('jacobi2d', 8, dict(depths=[8], wave_groups=4, sync=3)),              # TypeError
    ('jacobi3d', 8, dict(blk_skip_fill=1)), ('jacobi3d', 8, dict(blk_asm_sched=1)),  # TypeError
    ('jacobi3d', 8, dict(blk_prefetch=1)), ('jacobi3d', 8, dict(wp_pairs=1)),
    ('heat3d', 8, dict(blk_pairs=0)), ('jacobi3d', 8, dict(deep3d_from=3)),
    ('jacobi3d', 4, dict(depths=[4], deep3d='blk', blk_prefetch=0, blk_ring=2, blk_pairs=1)),
    ('jacobi3d', 4, dict(depths=[4], deep3d='blk', blk_mask_loads=0)),
    ('blur', None, dict(nontemporal=0)), ('denoise3d', None, dict(inline=False)),
    ('jacobi2d', 4, dict()), ('tail3d', 5, dict(deep3d='blk')),
    ('jacobi2d', 12, dict(depths=[12], cols=4, chunk_rows=128, prefetch=2)),
    ('jacobi3d', 8, dict(rows=8)), ('jacobi3d', 8, dict(rows=12, cols=1)),
    ('denoise3d', None, dict(rows=12, cols=1)), ('denoise3d', None, dict(cols=2)),
    ('blur', 8, dict(align='store64')), ('jacobi2d', 12, dict(align='full', prefetch=4)),
    ('blur', 31, dict(wave_groups=0)), ('seidel2d', 31, dict(wave_groups=1)),
    ('jacobi2d', 1000, dict(max_depth=8)), ('jacobi2d', 1000, dict(max_depth=16)),
    ('jacobi2d', 1000, dict(depths=[3, 6, 16])), ('jacobi2d', 1000, dict(vgpr_budget=120)),
    ('wave2d', 8, dict(depths=[2, 3])), ('wave2d', 8, dict(vgpr_budget=64)),
    ('wave2d', 8, dict(max_depth=2)), ('fdtd2d', 8, dict(skip_fill=0, waves_per_eu=2)),
] + [(app, 31, o) for app, o in parity.SHIPPED_FORMS + parity.EXPERIMENTAL_FORMS] + [
    (app, iterate, o) for app, o, _, iterate in (
        ('blur', dict(nontemporal=2), 0, 1), ('jacobi2d', dict(nontemporal=3), 0, 5),
        ('sobel2d', dict(nontemporal=2), 0, 1), ('denoise3d', dict(nt=2), 0, 1),
        ('jacobi3d', dict(nt=2, wp_nt=2, blk_nt=3), 0, 7),
        ('heat3d', dict(nt=2, wp_nt=4, blk_nt=2), 0, 6))] + [
    ('heat3d', 9, dict(depths=[2, 4], **o)) for o in (
        dict(), dict(wp_pairs=0), dict(wp_prefetch=1), dict(wp_pairs=1, wp_waves_per_eu=3),
        dict(wp_loader=1, wp_waves_per_eu=3), dict(wp_split=1), dict(wp_pairs=1, wp_rows=12))] + [
    (app, 13, dict(depths=[2, 4], deep3d='blk', **o)) for app, o in (
        ('jacobi3d', dict()), ('jacobi3d', dict(blk_prefetch=1)), ('heat3d', dict()),
        ('heat3d', dict(blk_pairs=0)), ('jacobi3d', dict(blk_mask_loads=0)),
        ('jacobi3d', dict(blk_lean_fill=0)), ('heat3d', dict(blk_wide_stores=1, blk_nt=2)),
        ('jacobi3d', dict(blk_wide_stores=0)), ('jacobi3d', dict(blk_pairs=1)),
        ('heat3d', dict(blk_stack=4, blk_prefetch=0, blk_pairs=1, blk_ring=2)))] + [
    (c[0], 31, c[3]) for c in contract._FORCED_2D] + [
    (c[0], 5, c[3]) for c in contract._FORCED_3D] + [
    # tools/calibrate.py: one depth, one form
    (app, 100, dict(depths=[d], **({'deep3d': form} if form else {})))
    for app, d, form in (('jacobi2d', 24, None), ('blur', 8, None), ('jacobi3d', 4, 'blk'),
                         ('jacobi3d', 4, 'wp'), ('heat3d', 2, 'blk'), ('wave2d', 4, None))]
# tools pass one option set across programs of different families: every distinct set of
# the list above on one program of each family (an option is refused, used or dropped)
CROSSED = []
for _, _, o in LITERAL:
  if o and o not in CROSSED:
    CROSSED.append(o)


def spec_of(app, iterate):
  if app in contract.TEXT:
    return contract.spec_of(app, iterate)
  kw = {} if iterate is None else dict(iterate=iterate)
  path = os.path.join(SAMPLES, app + '.soda')
  path = path if os.path.exists(path) else os.path.join(SAMPLES, 'extra', app + '.soda')
  return specmod.spec_from_stencil(frontend.load(path, **kw))


def line(name, make_spec, options):
  try:
    text, table = kernel.generate(make_spec(), **options)
  except Exception as e:      # recorded, not raised: the error is part of the behaviour
    return '%s %s: %s' % (name, type(e).__name__, e)
  entries = hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest()[:16]
  return '%s %s %s %s' % (name, hashlib.sha256(text.encode()).hexdigest(),
                          ','.join(k['name'] for k in table), entries)


def cases():
  show = lambda o: json.dumps(o, sort_keys=True, separators=(',', ':'))
  for path in sorted(glob.glob(os.path.join(SAMPLES, '*.soda')) +
                     glob.glob(os.path.join(SAMPLES, 'extra', '*.soda'))):
    app = os.path.basename(path)[:-5]
    for iterate in ITERATES:
      yield 'sample/%s/%s' % (app, iterate), (lambda a=app, i=iterate: spec_of(a, i)), {}
    yield 'unfused/%s' % app, (lambda a=app: spec_of(a, None)), dict(fused=False)
  with open(os.path.join(ROOT, 'tests', 'golden', 'random_programs.json')) as f:
    programs = json.load(f)
  for key in sorted(programs):
    make = lambda k=key: specmod.spec_from_stencil(frontend.loads(programs[k]['text']))
    yield 'random/%s' % key, make, {}
    if key.startswith('cube'):    # tests/test_gpu_random_programs.py: the block form alone
      yield 'random/%s/blk' % key, make, dict(deep3d='blk')
      yield 'random/%s/blk_pairs' % key, make, dict(deep3d='blk', blk_pairs=1)
  for n, (app, iterate, options) in enumerate(LITERAL):
    yield 'option/%d/%s/%s/%s' % (n, app, iterate, show(options)), \
        (lambda a=app, i=iterate: spec_of(a, i)), options
  for n, options in enumerate(CROSSED):
    for app in FAMILIES:
      yield 'crossed/%d/%s/%s' % (n, app, show(options)), \
          (lambda a=app: spec_of(a, None if a == 'denoise3d' else 31)), options


if __name__ == '__main__':
  out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else sys.stdout
  for case in cases():
    out.write(line(*case) + '\n')
