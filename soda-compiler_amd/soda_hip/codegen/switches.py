"""The opt-in kernel forms of kernel.generate(): one row per switch, and what follows from it.

A switch is a boolean keyword of generate() that adds one kernel form to the programs in its
class.  Everything outside the generator that has to know a switch - the command line, the
generated hosts, the run-time's depth limit, the name of the prebuilt code object - reads it
here: an opt-in form more is a row more - of SWITCHES, the forms for windows and outputs the
default forms refuse, or of ELEMENT_SWITCHES, the forms by element width, or of MIXED_SWITCHES, the forms for
tensors of different widths; readers take EVERY.
Data and pure functions only.  (The far-reach
switches' depth limit depends on the program: depth_limit_of reads it off kernel.FAR_FORMS,
where such a form is a row as well.)
"""
import collections

# keyword:     of kernel.generate() and of every function that passes switches on
# flag, dest:  of the command line (backend.add_arguments), in the order of `--help`
# suffix:      of the prebuilt code object's name, <app><suffix>.hsaco
# depth_limit: the form's kernel stores several outputs and is not in the default schedule: it
#              is launched under soda_hip_plan_set_max_depth(plan, 1)
# note:        the key of soda_hip_meta under which generate() says what the switch did
Switch = collections.namedtuple('Switch', 'keyword flag dest help suffix depth_limit note')
SWITCHES = (
    Switch('fuse_outputs', '--hip-fuse-outputs', 'hip_fuse_outputs',
           'one fused depth-1 kernel for a one-pass 2-D / 3-D program '
           'with several outputs (launched under a depth limit of 1: '
           'soda_hip_plan_set_max_depth)', '.fused', True, None),
    Switch('lds_planes', '--hip-lds-planes', 'hip_lds_planes',
           'one fused depth-1 kernel with the in-plane neighbours in LDS '
           'for a one-stage 3-D program no other fused form takes (high-order '
           'stars); it runs in the default schedule', '.lds', False, 'lds_planes'),
    Switch('lds_fields', '--hip-lds-fields', 'hip_lds_fields',
           'one fused depth-1 kernel with the in-plane neighbours in LDS '
           'for a 3-D program with two or three outputs that read inputs only '
           '(launched under a depth limit of 1: soda_hip_plan_set_max_depth)',
           '.ldsf', True, 'lds_fields'),
    Switch('far_taps', '--hip-far-taps', 'hip_far_taps',
           'the fused 1-D kernels for a program that reads an x-neighbour beyond the next '
           'lane (float FIRs of more than 9 taps, double stencils of radius 3 and up): the '
           'same forms with chained wave shifts, up to 8 lanes away.  Fused 1-D kernels are '
           'not in the default schedule: the program is launched under the depth limit of '
           'its deepest kernel (soda_hip_plan_set_max_depth)', '.taps', False, 'far_taps'),
    Switch('far_lanes', '--hip-far-lanes', 'hip_far_lanes',
           'the fused 2-D kernels for a program that reads an x-neighbour beyond the next '
           'lane or keeps a window above 12 rows (float stars of radius 5 and up, double '
           'ones of radius 3 and up): the same forms with chained wave shifts.  The kernels '
           'of a program over one array run in the default schedule; a program over several '
           'fields is launched under the depth limit of its deepest kernel '
           '(soda_hip_plan_set_max_depth)', '.far', False, 'far_lanes'),
    Switch('lds_ring', '--hip-lds-ring', 'hip_lds_ring',
           'one fused depth-1 kernel with a ring of planes in LDS for a 3-D program '
           'that reads an input off the z axis in several planes (mixed derivatives), '
           'with one to three outputs (launched under a depth limit of 1: '
           'soda_hip_plan_set_max_depth)', '.ldsr', True, 'lds_ring'),
)
# ... and the forms that differ by ELEMENT WIDTH, not by window or outputs: a table of their
# own with the same columns.  Everything that reads the switches reads ALL, both tables in this
# order; a further form by element width is a row more here.
ELEMENT_SWITCHES = (
    Switch('packed_cells', '--hip-packed-cells', 'hip_packed_cells',
           'the fused 3-D kernels for a program over 8- or 16-bit integer volumes (one '
           'output, inputs and output of one width): one tile per wavefront with the '
           'windows kept packed, four or two cells per register, at depths 1 and 2; they '
           'run in the default schedule', '.pk', False, 'packed_cells'),
)
ALL = SWITCHES + ELEMENT_SWITCHES
# ... and the forms for programs whose tensors DIFFER in element width (ELEMENT_SWITCHES: one
# narrow width throughout, cells packed; here: every tensor moved in its own width): a table of
# their own with the same columns, a further such form is a row more here.  ALL stays the two
# tables above; everything that reads the switches reads EVERY, the three tables in this order.
MIXED_SWITCHES = (
    Switch('mixed_widths', '--hip-mixed-widths', 'hip_mixed_widths',
           'one fused depth-1 kernel for a 2-D program with one output whose inputs and '
           'output differ in element width (8- or 16-bit pixels filtered in float, float '
           'quantised to integers): every tensor is loaded and stored in its own width; it '
           'runs in the default schedule', '.mw', False, 'mixed_widths'),
)
EVERY = ALL + MIXED_SWITCHES
BY_KEYWORD = {s.keyword: s for s in EVERY}


def given(on):
  """The rows of the switches that are on in the keyword arguments `on`, in table order.  A
  name that is no row is refused as Python refuses an unknown keyword."""
  for name in on:
    if name not in BY_KEYWORD:
      raise TypeError("got an unexpected keyword argument '%s'" % name)
  return [s for s in EVERY if on.get(s.keyword)]


def from_args(args, rows=SWITCHES):
  """{keyword: bool} of every switch of `rows` (the command line reads EVERY), read from an
  argparse namespace."""
  return {s.keyword: bool(getattr(args, s.dest, False)) for s in rows}


def depth_limit_flags(on):
  """The flags given among those whose kernel needs the depth limit."""
  return [s.flag for s in given(on) if s.depth_limit]


def depth_limit(on):
  """Do these switches need the depth limit that admits a kernel over several outputs?"""
  return bool(depth_limit_flags(on))


def depth_limit_of(spec, on):
  """The depth limit the entry points generated for `spec` with the switches `on` set before
  they run, and the flags that ask for it: (0, []) for none.  1 where a switch makes a fused
  kernel over several outputs; under a far-reach switch (the rows of kernel.FAR_FORMS, in
  that order: `far_lanes`, `far_taps`), for a program whose fused kernels the switch makes
  and the default schedule does not hold - 2-D over several fields, 1-D over one array or
  several - the depth of the deepest (kernel.far_depth_limit).  The far-reach switches
  concern disjoint programs."""
  if depth_limit(on):
    return 1, depth_limit_flags(on)
  from . import kernel
  for form in kernel.FAR_FORMS:
    limit = kernel.far_depth_limit(form, spec) if on.get(form.switch) else 0
    if limit:
      return limit, [BY_KEYWORD[form.switch].flag]
  return 0, []


def keyword_text(on):
  """`, <keyword>=True` per switch that is on: the tail of a generated call."""
  return ''.join(', %s=True' % s.keyword for s in given(on))


def blob_suffix(on):
  """What the switches add to a code object's name; `lds_fields` alone decides `.ldsf`."""
  suffixes = [s.suffix for s in given(on)]
  return BY_KEYWORD['lds_fields'].suffix if on.get('lds_fields') else ''.join(suffixes)


def for_program(spec, **on):
  """The switches to generate `spec` with when `on` is asked for: a one-pass program with
  several outputs (kernel_stream2d.rectangular) is in any fused form's class only under
  `fuse_outputs`, so the LDS form over fields brings it along."""
  from . import kernel_stream2d
  if given(on) and on.get('lds_fields') and kernel_stream2d.rectangular(spec):
    return dict(on, fuse_outputs=True)
  return on
