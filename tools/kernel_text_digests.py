#!/usr/bin/env python3
"""One line per case of what kernel.generate() returns: the sha256 of the text, the kernel
names of the table and a digest of the table entries - or, for a case that raises, the
exception.  Needs no GPU and no hipcc.  Two trees that print the same lines generate the
same kernels; run it in both and diff the outputs (a refactoring of the generator's
selection must give zero differing lines, the error lines included).

The opt-in switches of generate() (fuse_outputs, lds_planes, lds_fields, lds_ring) are cases
too (the cases of the first three are printed first and as they were before `lds_ring`
existed, those with `lds_ring` after them, those with `far_lanes` after these, those with
`far_taps` after those, those with `mixed_widths` last: an older tree's output is a
prefix-wise subset), and
what is derived from them outside the generator has lines of its own: `host/...`, the sha256
of the generated Python and C++ host texts per combination of switches, and `file/...`, the
name of the prebuilt code object per combination build() uses.

usage: kernel_text_digests.py [output file]
"""
import glob
import hashlib
import io
import itertools
import json
import os
import sys

if '--help' in sys.argv or '-h' in sys.argv:
  print(__doc__)
  sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'soda-compiler_amd'), os.path.join(ROOT, 'tests')]
from soda_hip import frontend                                   # noqa: E402
from soda_hip.codegen import (host_cpp, host_shim, kernel, kernel_fields2d,  # noqa: E402
                              kernel_fields3d, kernel_stream3d_lds)
from soda_hip.codegen import spec as specmod                    # noqa: E402
import __graft_entry__ as entry                                 # noqa: E402
# the option sets of the GPU tests come from the tests themselves (importing them needs no GPU)
import test_gpu_memory_contract as contract                     # noqa: E402
import test_gpu_parity as parity                                # noqa: E402
import test_lds3d_codegen as lds3d                              # noqa: E402
import test_lds3d_fields_codegen as lds3d_fields                # noqa: E402
import test_rect_codegen as rect                                # noqa: E402

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

SWITCHES = ('fuse_outputs', 'lds_planes', 'lds_fields', 'lds_ring')
BEFORE_RING = SWITCHES[:3]
# the samples the LDS-plane forms take, with the switches that give them their kernel
LDS_SAMPLES = [(app, dict(lds_planes=True)) for app in lds3d.APPS] + [
    (app, lds3d_fields.switches(app)) for app in lds3d_fields.APPS]
RING_SAMPLES = [(app, dict(lds_ring=True)) for app in entry.LDS_RING_APPS]
FAR_SAMPLES = [(app, dict(far_lanes=True)) for app in entry.FAR_LANES_APPS]
TAPS_SAMPLES = [(app, dict(far_taps=True)) for app in entry.FAR_TAPS_APPS]
MIXED_SAMPLES = [(app, dict(mixed_widths=True)) for app in entry.MIXED_WIDTHS_APPS]
HOST_PROGRAMS = ('jacobi2d', 'grad2d', 'grad3d', 'star3d', 'acoustic3d', 'deriv3d')
HOST_CPP_SWITCHES = ('fuse_outputs', 'lds_fields')      # the keywords host_cpp.print_code took


def combinations(names):
  """Every subset of the switches `names`, as keyword arguments (those that are on)."""
  return [{n: True for n, on in zip(names, bits) if on}
          for bits in itertools.product((False, True), repeat=len(names))]


def inline_texts():
  """(key, program text): what tests/test_rect_codegen.py, test_lds3d_codegen.py and
  test_lds3d_fields_codegen.py feed to generate() besides the samples.  The module-level
  texts are imported; those the rect tests build inside their functions are restated from
  the tests' own header line and limits."""
  for name in ('TWO_PLANES', 'TWO_STAGES', 'TWO_OUTPUTS', 'TWO_BYTES'):
    yield 'lds3d/' + name, getattr(lds3d, name)
  yield 'lds3d/axis', lds3d._HEAD % 'axis' + 'input float: a(32, 32, *)\n' \
      'output float: b(0, 0, 0) = a(0, 0, 3) + a(0, 0, -3)\n'
  for name in ('STAGE_READS_STAGE', 'FOUR_OUTPUTS', 'MIXED_WIDTHS', 'TWO_BYTES', 'TWO_PLANES'):
    yield 'lds3d_fields/' + name, getattr(lds3d_fields, name)
  head = rect._HEAD
  for dim, limit, tile in ((2, kernel_fields2d.MAX_OUTPUTS, '(32, *)'),
                           (3, kernel_fields3d.MAX_OUTPUTS, '(32, 32, *)')):
    zero = ', '.join('0' * dim)
    one = zero.replace('0', '1', 1)
    for n in (limit, limit + 1):
      yield 'rect/many/%d/%d' % (dim, n), head % ('many', 1) + 'input float: a%s\n' % tile + \
          ''.join('output float: o%d(%s) = a(%s) * %d.0f\n' % (j, zero, zero, j + 2)
                  for j in range(n))
    yield 'rect/wide_out/%d' % dim, head % ('widths', 1) + 'input float: a%s\n' % tile + \
        'output float: o(%s) = a(%s) * 2.0f\noutput double: p(%s) = a(%s) * 0.5\n' % (
            (zero,) * 4)
    yield 'rect/wide_local/%d' % dim, head % ('widths', 1) + 'input float: a%s\n' % tile + \
        'local double: m(%s) = a(%s) * 0.5\n' % (zero, zero) + \
        'output float: o(%s) = float(m(%s)) + a(%s)\n' % (zero, one, zero) + \
        'output float: p(%s) = float(m(%s)) - a(%s)\n' % (zero, zero, one)
    for n in (4, 5, 7):
      rows = ['input float: f%d%s' % (j, tile if j == n - 1 else '') for j in range(n)]
      rows += ['output float: o(%s) = %s' % (zero, ' + '.join('f%d(%s)' % (j, zero)
                                                               for j in range(n))),
               'output float: p(%s) = f0(%s) * 2.0f' % (zero, one)]
      yield 'rect/wide/%d/%d' % (dim, n), head % ('wide', 1) + '\n'.join(rows) + '\n'
  far2 = head % ('far', 1) + 'input float: a(32, *)\n' \
      'output float: o(0, 0) = a(0, 0) + a(5, 0)\noutput float: p(0, 0) = a(0, 1)\n'
  yield 'rect/far2', far2
  yield 'rect/near2', far2.replace('a(5, 0)', 'a(4, 0)')
  yield 'rect/far3', head % ('far', 1) + 'input float: a(32, 32, *)\n' \
      'output float: o(0, 0, 0) = a(0, 0, 0) + a(-3, 0, 0)\noutput float: p(0, 0, 0) = a(0, 1, 0)\n'


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
  # the opt-in switches: each alone and all together on every sample ...
  together = [{n: True} for n in BEFORE_RING] + [{n: True for n in BEFORE_RING}]
  with_ring = [dict(lds_ring=True), {n: True for n in SWITCHES}]
  for path in sorted(glob.glob(os.path.join(SAMPLES, '*.soda')) +
                     glob.glob(os.path.join(SAMPLES, 'extra', '*.soda'))):
    app = os.path.basename(path)[:-5]
    for on in together:
      yield 'switch/%s/%s' % (app, show(on)), (lambda a=app: spec_of(a, None)), on
  # ... the samples the LDS-plane forms take in every shape (refused ones included) and at
  # the iteration counts that change their default depths ...
  for app, on in LDS_SAMPLES:
    for shape in kernel_stream3d_lds.SHAPES:
      yield 'lds_shape/%s/%s' % (app, show(shape)), (lambda a=app: spec_of(a, None)), \
          dict(on, lds_shape=shape)
    for iterate in (1, 2, 3, None):
      yield 'lds_iterate/%s/%s' % (app, iterate), (lambda a=app, i=iterate: spec_of(a, i)), on
  # ... and the program texts of the switches' own tests
  for key, text in inline_texts():
    make = lambda t=text: specmod.spec_from_stencil(frontend.loads(t))
    for on in [{}] + together:
      yield 'inline/%s/%s' % (key, show(on)), make, on
  # `lds_ring`: alone and with the other three on every sample and program text, and its
  # samples in every shape and at the iteration counts
  for path in sorted(glob.glob(os.path.join(SAMPLES, '*.soda')) +
                     glob.glob(os.path.join(SAMPLES, 'extra', '*.soda'))):
    app = os.path.basename(path)[:-5]
    for on in with_ring:
      yield 'switch/%s/%s' % (app, show(on)), (lambda a=app: spec_of(a, None)), on
  for app, on in RING_SAMPLES:
    for shape in kernel_stream3d_lds.SHAPES:
      yield 'lds_shape/%s/%s' % (app, show(shape)), (lambda a=app: spec_of(a, None)), \
          dict(on, lds_shape=shape)
    for iterate in (1, 2, 3, None):
      yield 'lds_iterate/%s/%s' % (app, iterate), (lambda a=app, i=iterate: spec_of(a, i)), on
  for key, text in inline_texts():
    make = lambda t=text: specmod.spec_from_stencil(frontend.loads(t))
    for on in with_ring:
      yield 'inline/%s/%s' % (key, show(on)), make, on
  # `far_lanes`: alone and with the other four on every sample and program text, and its
  # samples at the iteration counts that change their depths
  with_far = [dict(far_lanes=True), dict({n: True for n in SWITCHES}, far_lanes=True)]
  for path in sorted(glob.glob(os.path.join(SAMPLES, '*.soda')) +
                     glob.glob(os.path.join(SAMPLES, 'extra', '*.soda'))):
    app = os.path.basename(path)[:-5]
    for on in with_far:
      yield 'switch/%s/%s' % (app, show(on)), (lambda a=app: spec_of(a, None)), on
  for app, on in FAR_SAMPLES:
    for iterate in (1, 2, 3, None):
      yield 'far_iterate/%s/%s' % (app, iterate), (lambda a=app, i=iterate: spec_of(a, i)), on
  for key, text in inline_texts():
    make = lambda t=text: specmod.spec_from_stencil(frontend.loads(t))
    for on in with_far:
      yield 'inline/%s/%s' % (key, show(on)), make, on
  # `far_taps`: alone and with the other five on every sample and program text, and its
  # samples at the iteration counts that change their depths (8: a segment keeps no cells)
  with_taps = [dict(far_taps=True), dict({n: True for n in SWITCHES}, far_lanes=True,
                                         far_taps=True)]
  for path in sorted(glob.glob(os.path.join(SAMPLES, '*.soda')) +
                     glob.glob(os.path.join(SAMPLES, 'extra', '*.soda'))):
    app = os.path.basename(path)[:-5]
    for on in with_taps:
      yield 'switch/%s/%s' % (app, show(on)), (lambda a=app: spec_of(a, None)), on
  for app, on in TAPS_SAMPLES:
    for iterate in (1, 2, 3, 8, None):
      yield 'taps_iterate/%s/%s' % (app, iterate), (lambda a=app, i=iterate: spec_of(a, i)), on
    yield 'taps_cols/%s' % app, (lambda a=app: spec_of(a, None)), dict(on, cols=8)
  for key, text in inline_texts():
    make = lambda t=text: specmod.spec_from_stencil(frontend.loads(t))
    for on in with_taps:
      yield 'inline/%s/%s' % (key, show(on)), make, on
  # `mixed_widths`: alone on every sample and program text, and its samples in every lane
  # shape of kernel.mixed_shapes (a shape over the register estimate keeps its stage kernels)
  for path in sorted(glob.glob(os.path.join(SAMPLES, '*.soda')) +
                     glob.glob(os.path.join(SAMPLES, 'extra', '*.soda'))):
    app = os.path.basename(path)[:-5]
    yield 'switch/%s/mixed_widths' % app, (lambda a=app: spec_of(a, None)), dict(mixed_widths=True)
  for app, on in MIXED_SAMPLES:
    for cols in sorted(kernel.mixed_shapes(spec_of(app, None))):
      yield 'mixed_cols/%s/%d' % (app, cols), (lambda a=app: spec_of(a, None)), dict(on, cols=cols)
  for key, text in inline_texts():
    make = lambda t=text: specmod.spec_from_stencil(frontend.loads(t))
    yield 'inline/%s/mixed_widths' % key, make, dict(mixed_widths=True)


def digest(text):
  return hashlib.sha256(text.encode()).hexdigest()


def host_lines():
  """`host/...`: the generated host texts per combination of switches, one program per
  class; `file/...`: the code object names of the combinations build() uses."""
  show = lambda o: ','.join(sorted(o)) or '-'
  for app in HOST_PROGRAMS:
    spec = spec_of(app, None)
    for on in combinations(BEFORE_RING) + [dict(o, lds_ring=True)
                                           for o in combinations(BEFORE_RING)]:
      out = io.StringIO()
      try:
        host_shim.print_code(spec, out, **on)
        yield 'host/shim/%s/%s %s' % (app, show(on), digest(out.getvalue()))
      except Exception as e:
        yield 'host/shim/%s/%s %s: %s' % (app, show(on), type(e).__name__, e)
    for on in combinations(HOST_CPP_SWITCHES):
      out = io.StringIO()
      try:
        table = kernel.generate(spec, **on)[1]
        host_cpp.print_code(spec, table, out, lowered=specmod.inline_pointwise(spec), **on)
        yield 'host/cpp/%s/%s %s' % (app, show(on), digest(out.getvalue()))
      except Exception as e:
        yield 'host/cpp/%s/%s %s: %s' % (app, show(on), type(e).__name__, e)
  every = entry.APPS + entry.EXTRA_APPS + entry.FIELD_APPS + entry.FIELD3D_APPS + \
      entry.FIELD1D_APPS + entry.RECT_APPS + entry.LDS3D_APPS + entry.LDS_FIELDS_APPS
  for apps, on in ((every, {}), (entry.FUSED_OUTPUT_APPS, dict(fuse_outputs=True)),
                   (entry.LDS3D_APPS, dict(lds_planes=True)),
                   (entry.LDS_FIELDS_APPS, dict(lds_fields=True)),
                   (entry.LDS_RING_APPS, {}), (entry.LDS_RING_APPS, dict(lds_ring=True))):
    for app in apps:
      yield 'file/%s/%s %s' % (app, show(on), os.path.basename(entry.blob_path(app, **on)))
  for app in HOST_PROGRAMS + entry.FAR_LANES_APPS:
    out = io.StringIO()
    host_shim.print_code(spec_of(app, None), out, far_lanes=True)
    yield 'host/shim/%s/far_lanes %s' % (app, digest(out.getvalue()))
  for on in ({}, dict(far_lanes=True)):
    for app in entry.FAR_LANES_APPS:
      yield 'file/%s/%s %s' % (app, show(on), os.path.basename(entry.blob_path(app, **on)))
  for app in HOST_PROGRAMS + entry.FAR_TAPS_APPS:
    out = io.StringIO()
    host_shim.print_code(spec_of(app, None), out, far_taps=True)
    yield 'host/shim/%s/far_taps %s' % (app, digest(out.getvalue()))
  for on in ({}, dict(far_taps=True)):
    for app in entry.FAR_TAPS_APPS:
      yield 'file/%s/%s %s' % (app, show(on), os.path.basename(entry.blob_path(app, **on)))
  for app in HOST_PROGRAMS + entry.MIXED_WIDTHS_APPS:
    out = io.StringIO()
    host_shim.print_code(spec_of(app, None), out, mixed_widths=True)
    yield 'host/shim/%s/mixed_widths %s' % (app, digest(out.getvalue()))
  for on in ({}, dict(mixed_widths=True)):
    for app in entry.MIXED_WIDTHS_APPS:
      yield 'file/%s/%s %s' % (app, show(on), os.path.basename(entry.blob_path(app, **on)))


if __name__ == '__main__':
  out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else sys.stdout
  for case in cases():
    out.write(line(*case) + '\n')
  for text in host_lines():
    out.write(text + '\n')
