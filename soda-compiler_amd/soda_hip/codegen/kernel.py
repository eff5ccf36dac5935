"""HIP kernel printer: program spec -> one translation unit of gfx950 kernels.

Counterpart of the reference's HLS kernel printer (reference
src/soda/codegen/xilinx/hls_kernel.py:146-189): same input (the analysed
stencil), and the arithmetic of every stage is the same expression text
(hls_kernel.py:487-489 `WriteData(..., c_type(expr.c_expr))`); everything around
it is designed for a GPU instead of an FPGA dataflow region.

The unit holds
  * one per-stage kernel per stage (kernel_stage.py), always;
  * the fused kernels of the program's family, at the depths selected below:
      multi-field 2-D   kernel_fields2d
      multi-field 3-D   kernel_fields3d
      one pass, several outputs, 2-D / 3-D (kernel_stream2d.rectangular): the same two
                        forms at depth 1, only with `fuse_outputs=True`
      multi-field 1-D   kernel_fields1d (kernel_stream1d's segments over N fields)
      single-array 1-D  kernel_stream1d (segments of one wavefront, no streaming)
      single-array 2-D  kernel_stream2d (one strip per wavefront) or, deep,
                        kernel_stream2d_wp (wave-pipelined)
      3-D, depth 1-2    kernel_stream3d (one tile per wavefront)
      3-D chains        kernel_stream3d_blk (block form) and / or
                        kernel_stream3d_wp (wave-pipelined)
      3-D, one stage, windows wider than a lane's columns: kernel_stream3d_lds (the
                        in-plane neighbours from an LDS plane), only with `lds_planes=True`
                        and only where no other form made a depth-1 kernel;
      3-D, two or three outputs that read inputs only, windows wider than a lane's columns:
                        the same form over several outputs (<app>_fused_k1lf), only with
                        `lds_fields=True` and only where no other form made a depth-1 kernel;
      3-D, either of the two with an input read in-plane in SEVERAL planes (mixed z terms):
                        the same form with a ring of planes in LDS (<app>_fused_k1r, _k1rf),
                        only with `lds_ring=True` and only where no other form made a
                        depth-1 kernel;
      2-D, x-neighbours beyond the next lane or windows above 12 rows: kernel_stream2d /
                        kernel_fields2d with chained wave shifts, only with `far_lanes=True`;
      1-D, x-neighbours beyond the next lane (FIRs of more than 9 float taps, double
                        stencils of radius 3 and up): kernel_stream1d / kernel_fields1d with
                        chained wave shifts, only with `far_taps=True`;
      3-D, 8- and 16-bit integer volumes, depth 1-2: kernel_stream3d_pk (kernel_stream3d with
                        packed windows), only with `packed_cells=True`;
      2-D, one output, inputs and output of different element widths (8- or 16-bit pixels
                        filtered in float, float quantised to integers): kernel_stream2d at
                        depth 1 with every tensor's loads and stores in its own width, only
                        with `mixed_widths=True`;
  * `soda_hip_meta`, JSON describing the program and the kernel table, which
    libsoda_hip.so reads back from the loaded blob.

generate() is the driver: one function per family (FAMILIES) selects forms, depths and
options, form_options() says which options a form receives.  The opt-in forms' switches
are the rows of switches.py; what differs between the forms of a kind, the rows of LdsForm
(the LDS-plane forms) and of FAR_FORMS (the far-reach forms).
"""
import collections
import functools
import hashlib
import inspect
import json
import os
import re
import subprocess
import tempfile

from .. import __version__
from . import (kernel_common, kernel_fields1d, kernel_fields2d, kernel_fields3d, kernel_stage,
               kernel_stream1d, kernel_stream2d, kernel_stream2d_wp, kernel_stream3d,
               kernel_stream3d_blk, kernel_stream3d_lds, kernel_stream3d_pk,
               kernel_stream3d_wp)
from . import spec as specmod
from . import switches

DEFAULT_MAX_DEPTH = 12
# Wavefronts per strip for deep fused 2-D kernels: 0 = single-wave form only,
# N > 1 = always the wave-pipelined form (kernel_stream2d_wp), -1 = choose: the
# wave-pipelined form (4 wavefronts, packed pairs when the program allows) where
# the single-wave form would need more than AUTO_WP_VGPRS registers or does not
# fit at all.  Measured on MI355X at 16384x16384 (tools/tune.py): jacobi2d depth
# 12 (188 VGPRs) single-wave 543 us vs 545-570 us pipelined; seidel2d depth 12
# (236 VGPRs) 684 us vs 588 us; blur depth 8 (single-wave impossible, depth 4 is
# its limit) 4402 vs 3499 Gcell/s.
WAVE_GROUPS = -1
AUTO_WP_VGPRS = 200
AUTO_WP_GROUPS = 4
AUTO_WP_BUDGET = 200
AUTO_WP_RING = 6               # LDS ring slots of the packed form (4 rows in flight)
AUTO_WP_SQUEEZE_VGPRS = 152
# Depths beyond 12 for programs the packed wave-pipelined form covers.  16 runs at
# four workgroups per CU (128 VGPRs, 12-slot ring); 20 and 24 keep 5 / 6 levels
# per wavefront and are capped at 168 VGPRs = three workgroups per CU.  Measured
# per iteration, jacobi2d, same box (tools/chunk_sweep.py; us at 16384^2 / 8192^2 /
# the 16384 x 2432 slab of an 8-GPU run): depth 16 36.7 / 9.89 / 6.27, depth 20
# 34.6 / 9.46 / 5.90, depth 24 33.2 / 9.17 / 5.83.  Past 24 the four-wavefront
# form spills (depth 28: 49.7), 5 or 6 wavefronts per workgroup load the four
# SIMDs unevenly (depth 20 on 5: 41.7, depth 32 on 6: 47.2) and 7 or 8
# (depth 28 / 32: 33.9 / 34.0) are no better than depth 24 on four.
PACKED_DEEP_DEPTHS = (16, 20, 24)
PACKED_DEEP_DEPTH = PACKED_DEEP_DEPTHS[0]
PACKED_DEEP_WAVES_PER_EU = 3      # for the depths above 16
# ... and at these depths a second kernel NEXT TO it, `<app>_fused_k<d>w`: lanes of 12 columns
# as six pairs {c, c+6} (kernel_stream2d_wp.emit, cols=6), strips of 768 columns that keep
# 720 at depth 24 (0.9375 against 464 of 512 = 0.906) and 32 instead of 2 x 22 instructions
# per level-row of 12 cells; 256 registers = two workgroups per CU.  The run-time prices
# both per launch (csrc/schedule.cpp: fused_list), as it does the two 3-D depth-4 forms.
# Not depth 16: that kernel keeps four workgroups per CU at 128 registers.  Option
# `wide12`: 0 = never, 1 = next to the shipped kernel, 2 = instead of it (tools).
WIDE12_DEPTHS = (20, 24)
WIDE12_OPTIONS = dict(cols=6, pairs=2, ring=AUTO_WP_RING, waves_per_eu=2, vgpr_budget=256,
                      suffix='w')
WIDE12_DEFAULT = 1
# packable programs: the packed + ring form also replaces the single-wave form
# from this depth on (jacobi2d 16384^2 per launch: depth 12 570 vs 617 us, depth 8
# 501 vs 470 us - the single-wave form stays below)
PACKED_FROM_DEPTH = 12
WAVE_PIPELINE_MIN_DEPTH = 4
# Shallow fused kernels are HBM-bound: their strips start and end on 128-byte
# lines (kernel_stream2d.geometry, align='full'; +7..10 % measured at depth 1-2,
# nothing at 4, a loss from depth 8 on where the VALU bounds and the extra halo
# columns cost more than the alignment saves).
ALIGN_FULL_MAX_DEPTH = 2
# ... and their stores bypass the caches on arrays beyond the Infinity Cache
NT_AUTO_MAX_DEPTH_2D = 2
# rows a wavefront of the seam-free depth-1 form keeps in flight (16384^2 with two
# workgroups per CU, 3 / 6 / 9 rows: jacobi2d 419 / 414 / 415 us, sobel2d 270 / 253 / 242)
EXACT_PREFETCH = 6
# 3-D: depths beyond the single-wave form, built wave-pipelined (kernel_stream3d_wp)
DEEP_3D_DEPTHS = (4,)
BLOCK_3D_SHALLOW_DEPTHS = (1, 2)
# 3-D programs light on arithmetic get TWO depth-4 kernels: the wave-pipelined one
# (64 x 32 tiles, three workgroups per CU) and the block form (128 x 64 tiles, one
# 8-wavefront workgroup per CU, input planes prefetched one ahead); the run-time
# prices both per launch.  jacobi3d per depth-4 launch, same call: 512^3 375 vs
# 314 us, 256^3 49 vs 55, 128^3 27 vs 45; cfg5 (boxes 504^3 .. 112^3) 6.44 vs 6.04
# ms with either alone, 5.87 ms with the per-launch choice.  heat3d (packed pair-rows
# in the wave-pipelined form): 392 vs 378 us per 512^3 launch.
DEEP_3D_FORM = 'both'
BLOCK_3D_OPTIONS = dict(stack=8, prefetch=1, vgpr_budget=300, nt=4, mask_loads=1,
                        wide_stores=2, edge=1)
# The block form's input planes: through a two-slot LDS ring (LDS-direct loads, no
# prefetch registers) where the program's edge rows leave the LDS for it, else one
# plane ahead in registers.  Per depth-4 launch inside the 512^3 array of cfg5 (same
# chunking): box 496 242 vs 247 us, 456 205 vs 219, 416 152 vs 166, 352 117 vs 130,
# 256 53 vs 74; heat3d 512^3 x20, block form alone: 1.94 vs 1.96 ms
# (profiles/r03_blk_variants.txt); the ring's freed registers make room for packed
# pair-rows in heavy programs.
# mask_loads: ragged tiles fetch only what a stored cell depends on (the buffer form of the
# LDS-direct load; cfg5 per launch: box 424 161 -> 157 us, 400 140 -> 135, 368 128 -> 120,
# 360 118 -> 108; boxes that fill their tiles unchanged; the sweep -1.5 %)
# wide_stores: row segments leave in whole 64-byte pieces - the cells between the box
# and the next 64-byte boundary (unspecified by contract, read by nobody) are stored
# along, in launches beyond the Infinity Cache (2; 1 = always: boxes of 232^3 .. 336^3
# +1 %): cfg5 with this form alone 4.95 -> 4.79 ms, box 496 225 -> 210 us, 440 172 -> 156
# lean_fill: the levels a chunk's first steps do not need are skipped there (a second,
# guarded copy of the row loop for the trips at a chunk's ends; round 4): cfg5 with this
# form alone 4.81 -> 4.66 ms, per launch box 400 130.5 -> 125.6 us, 256 55.0 -> 48.8,
# 224 42.8 -> 37.3 (profiles/r04_blk_lean_fill.txt)
# edge: the first and last tile of a row store the 8 valid columns the 64-byte alignment
# drops (kernel_stream3d_blk.emit; soda_hip_kernel.edge_slack): cfg5's boxes 464, 456, 336,
# 328, 240, 232 and 112 lose a tile column (round 6)
BLOCK_3D_RING_OPTIONS = dict(stack=8, prefetch=0, ring=2, vgpr_budget=300, nt=4,
                             mask_loads=1, wide_stores=2, lean_fill=1, edge=1)
# ... for programs light enough on arithmetic: jacobi3d (weight 7) 417 us per
# depth-4 launch against 2 x 374 us at depth 2, heat3d (15) 622 us against
# 2 x 411 us; heavier programs are VALU-bound at depth 2 already
DEEP_3D_MAX_WEIGHT = 20
PACKED_3D_LIGHT_WEIGHT = 10
# ... and only programs that are light on arithmetic (denoise2d, ~70 weighted
# operations per cell, is VALU-bound at depth 1 and loses 19 % to the narrower
# aligned strips; blur 20, sobel2d 28, jacobi2d 5 gain)
ALIGN_FULL_MAX_WEIGHT = 40

# depths of the multi-field form (kernel_fields2d)
FIELDS_DEPTHS = (1, 2, 4, 8)
FIELDS_OPTIONS = ('skip_fill', 'vgpr_budget', 'max_period', 'waves_per_eu')
# ... and of its 3-D counterpart (kernel_fields3d): with the planes of every field of every
# iteration in one wavefront's registers, depth 2 is as deep as two- and three-field
# programs go in tiles that keep any cells
FIELDS3D_DEPTHS = (1, 2)
FIELDS3D_OPTIONS = ('rows', 'vgpr_budget', 'max_period', 'waves_per_eu')
# Rectangular 3-D programs (one pass, several outputs; `fuse_outputs`): rows of a tile x
# inputs at most.  Every input adds a plane pointer and a row of loads per tile row to what
# the plane loop keeps in scalar registers: mix3d (three inputs, two outputs) in 16-row tiles
# compiles with one SGPR pair parked in a VGPR in its array-edge path, in 12-row tiles with
# 96 SGPRs and none; grad3d (one input, three outputs) takes 16 rows with 104 and none.
# The smallest tile has 8 rows, so a rectangular 3-D program has at most FOUR inputs; with
# more it keeps its per-stage kernels and a note (2-D has no such cap).  The figure rests on
# these two samples: a program that spills under it shows in the compiler's resource report
# (tests/test_rect_codegen.py reads it for every sample), not at run time.
RECT3D_INPUT_ROWS = 36
# depths of the 1-D form (kernel_stream1d), capped by the program's `iterate`: those of
# fused_depths.  A level is one vector per lane, so no depth is refused for registers; a
# depth that profiles/r10_stream1d.txt shows not to beat the per-stage schedule leaves
# this list.  Under `far_taps` the same list: every depth a far-tap segment keeps cells at (1, 2
# and 4 for the samples) beats the per-stage schedule by more than the spread
# (profiles/r17_far1d.txt, 2^27 cells x 24: the slowest against per stage, lowpass1d depth 4
# 9.343 against 13.547 ms and acoustic1d depth 1 27.067 against 36.782 ms), so none leaves it
STREAM1D_DEPTHS = (1, 2, 4, 8, 12)
STREAM1D_OPTIONS = ('segs',)
# the 1-D form over several fields (kernel_fields1d) takes the same depths and options
FIELDS1D_OPTIONS = STREAM1D_OPTIONS
# the LDS-plane 3-D form (kernel_stream3d_lds; `lds_planes`): `lds_shape` = (wavefronts, rows
# per lane, lanes per tile row) instead of the first shape that fits
LDS3D_OPTIONS = ('lds_shape',)

# the far-lane 2-D forms (`far_lanes`): kernel_stream2d / kernel_fields2d with x-neighbours up
# to MAX_HOPS lanes away and windows of up to this many rows (a radius-8 window keeps 17 rows
# and the 3 in flight; the row loop is unrolled by the period)
FAR_MAX_PERIOD = 24

# the packed-cell 3-D form (kernel_stream3d_pk; `packed_cells`): depths of an iteration chain,
# capped by the program's `iterate`, and the options its emit() receives (`cols` and `rows`
# fix the tile shape, `waves_per_eu` / `vgpr_budget` the occupancy level, instead of the first
# that fits).  The rule of the 1-D and far forms: a depth that does not beat the per-stage
# schedule by more than the spread leaves the list.  Both do (profiles/r19_packed3d.txt, 512^3 /
# 256^3 x 4: the slowest against per stage, castvol3d depth 1 at 256^3, 0.302 against 0.309 ms
# at a spread of 0.004; smooth3d depth 2 0.744 against 1.194 ms at 512^3)
PACKED3D_DEPTHS = (1, 2)
PACKED3D_OPTIONS = ('rows', 'vgpr_budget', 'max_period', 'waves_per_eu', 'nt', 'chunk_planes')

# the mixed-width 2-D form (kernel_stream2d with `mixed`; `mixed_widths`): a lane holds C
# consecutive cells of every tensor, so C decides how many bytes of each it moves.  The shapes
# run from the one in which the WIDEST end fills a lane's 16 bytes (C = 16 / widest: uint8 next
# to float then moves 4 bytes per lane) to the one in which the NARROWEST does (C = 16 /
# narrowest: the float side then moves 64 bytes per lane in four pieces and costs C registers
# per retained row), every power of two between them.  mixed_shapes() gives them in the order
# they are tried; a shape the register estimate refuses is skipped; `cols=` is the only shape.
# MIXED_WIDEST_FIRST: the order that won the measurement (profiles/r21_mixed2d.txt).
MIXED_WIDEST_FIRST = True


def mixed_end_sizes(spec):
  """Element sizes of the inputs and of the outputs, in that order."""
  types = specmod.tensor_c_types(spec)
  return [specmod.ELEM_SIZE[t['c_type']] for t in spec['inputs']] + \
      [specmod.ELEM_SIZE[types[o]] for o in spec['outputs']]


def mixed_shapes(spec, cols=None):
  """Columns per lane of the mixed-width form, in the order they are tried."""
  if cols:
    return [cols]
  sizes = mixed_end_sizes(spec)
  shapes = [c for c in (1, 2, 4, 8, 16) if 16 // max(sizes) <= c <= 16 // min(sizes)]
  return shapes if MIXED_WIDEST_FIRST else shapes[::-1]


def mixed_arguments(req):
  """What `mixed_widths` adds to kernel_stream2d.emit's arguments for this request:
  dict(mixed=True) for a 2-D program with one output whose inputs and output differ in
  element width, {} for every other program, whose text then stays what it is.  Leaves in
  req.meta_notes why a program is not in the class; mixed_note() says the rest."""
  spec = req.spec
  if not req.on['mixed_widths']:
    return {}
  key = switches.BY_KEYWORD['mixed_widths'].note
  types = specmod.tensor_c_types(spec)
  if len(set(mixed_end_sizes(spec))) == 1:
    req.meta_notes[key] = 'not concerned: inputs and output of one width'
  elif spec['dim'] != 2:
    req.meta_notes[key] = 'not fused: the mixed-width form handles 2-D programs'
  elif len(spec['outputs']) != 1:
    req.meta_notes[key] = 'not fused: the mixed-width form handles programs with one output'
  elif '_Float16' in [t['c_type'] for t in spec['inputs']] + [types[spec['outputs'][0]]]:
    req.meta_notes[key] = 'not fused: the mixed-width form does not take half elements'
  else:
    return dict(mixed=True)
  return {}


def mixed_note(req, notes):
  """The switch's entry of soda_hip_meta for a program in its class: the kernel made, or
  why there is none."""
  if not req.mixed:
    return
  made = [e['name'] for e in req.made if e['kind'] == 'fused' and e['depth'] == 1]
  why = [n[len('depth 1 not fused: '):] for n in notes if n.startswith('depth 1 not fused: ')]
  req.meta_notes[switches.BY_KEYWORD['mixed_widths'].note] = made[0] if made else \
      'not fused: %s' % (why + ['no 2-D form takes it'])[0]


# generator options of the fused 2-D forms that `generate` passes through:
# those both forms understand, and those only the wave-pipelined form has
SHARED_2D_OPTIONS = ('skip_fill', 'vgpr_budget', 'max_period', 'align', 'waves_per_eu')
WP_ONLY_OPTIONS = ('pairs', 'ring', 'split', 'prio', 'seam_probe')
# ... and those that choose among the 2-D forms (stream2d_kernels) and reach no emit()
SELECT_2D_OPTIONS = ('wide12',)

HIPCC_FLAGS = ['-x', 'hip', '--offload-arch=gfx950', '--cuda-device-only',
               '--no-gpu-bundle-output', '-O3', '-ffp-contract=off',
               '-fno-slp-vectorize', '-fwrapv', '-std=c++17']


_DOUBLE_LITERAL = re.compile(
    r'(?<![\w.])(?:\d+\.\d*|\.\d+|\d+(?=[eE]))(?:[eE][+-]?\d+)?(?![\w.])')


def dpp_combine_is_safe(spec):
  """True for programs whose arithmetic is float32 only: every tensor `float`,
  no double literal, no math call (those are the C double functions), no cast."""
  if any(t != 'float' for t in specmod.tensor_c_types(spec).values()):
    return False
  for stage in spec['stages']:
    for text in [stage['expr']] + [l['expr'] for l in stage['lets']]:
      plain = specmod.LOAD_RE.sub('x', text)
      if _DOUBLE_LITERAL.search(plain) or kernel_common.used_functions(
          dict(stages=[dict(expr=text, lets=[])])) or 'static_cast<' in plain:
        return False
  return True


def extra_flags(spec):
  """Per-program compiler flags beyond HIPCC_FLAGS.

  ROCm 7.2's DPP-combine pass (GCNDPPCombine) is only trusted on pure-float32
  programs.  Found by the parity tests:
    * INTEGER subtraction whose operand is a wave-shift DPP move is miscompiled
      (`v_mov_b32_dpp` folded into `v_sub[rev]_u32/_u16`: every lane wrong;
      sobel2d at depth >= 2, `o = l - a(2,0) + a(-2,0)` on int32);
    * a DPP move folded into `v_cvt_f64_f32` (a float operand meeting a double
      literal) yields an instruction the verifier rejects: the compile fails.
  -O0 and -amdgpu-dpp-combine=false are correct in both cases.  Float32
  add/sub/mul with a DPP operand is verified bit-exact and the fusion is worth
  ~10 % on the jacobi kernels, so float32-only programs keep the pass."""
  tuning = []
  if spec['dim'] == 2 and \
      kernel_stream2d_wp.packable(specmod.inline_pointwise(spec)):
    # The packed kernels run at a register cap under which the default scheduler
    # serialises whole level-rows on one accumulator pair; the ILP-first strategy
    # keeps the four cells of a row interleaved.  Scheduling only: same results.
    # Measured per launch on 16384^2: jacobi2d depth 16 566 -> 557 us, depth 12
    # 508 -> 505, seidel2d depth 16 620 -> 615, depth 8 506 -> 489; the other
    # depths within +-0.5 %.  Not for 3-D programs: hipcc then gives the packed
    # heat3d kernel 276 registers instead of 230 (one workgroup per CU, 647 us
    # per launch instead of 400).
    tuning = ['-mllvm', '-amdgpu-sched-strategy=max-ilp']
  if dpp_combine_is_safe(spec):
    return tuning
  return ['-mllvm', '-amdgpu-dpp-combine=false'] + tuning


FLAGS_MARK = '// SODA-HIP-FLAGS:'


def flags_from_text(text):
  """Extra flags recorded in generated kernel text (for run-time compiles)."""
  for line in text.splitlines()[:400]:
    if line.startswith(FLAGS_MARK):
      return line[len(FLAGS_MARK):].split()
  return []


# Issue cost of an operation in units of one f32 add (2 SIMD cycles per wave64
# instruction on gfx950).  Double precision runs at half the rate; a double division
# and a double square root compile to ~13 double instructions each (denoise2d's
# `1.0f / sqrt(...)`: 12 v_fma_f64, 3 v_mul_f64, 2 v_div_scale_f64, v_rsq_f64,
# v_rcp_f64, v_div_fmas_f64, v_div_fixup_f64, 2 v_ldexp_f64, 2 conversions per cell);
# a float division to ~10 single ones; an integer division by a literal to a
# multiply-high and shifts.  Other math calls are the double library functions.
OP_COST = dict(f32=1, f64=2, div_f32=10, div_f64=30, div_int=8, sqrt=30, cheap_call=4,
               call=60)
_CHEAP_CALLS = ('fabs', 'fmax', 'fmin', 'floor', 'ceil', 'trunc', 'round', 'rint',
                'nearbyint', 'copysign', 'abs', 'min', 'max', 'select')


def arithmetic_weight(spec):
  """VALU cost of one iteration per cell, in f32-add equivalents: the operators of
  all stages priced by OP_COST.  An expression is priced as DOUBLE arithmetic when
  it holds a double literal, a math call (the C double functions) or a
  double tensor - as the C++ promotion rules make (most of) it."""
  types = specmod.tensor_c_types(spec)
  weight = 0
  for stage in spec['stages']:
    texts = [(let['c_type'], let['expr']) for let in stage['lets']] + \
        [(stage['c_type'], stage['expr'])]
    for c_type, source in texts:
      operands = [types.get(t) for t, _ in specmod.LOAD_RE.findall(source)]
      text = re.sub(r'\{[^}]*\}', 'L', kernel_common.device_expr(source))
      calls = re.findall(r'soda_fn_(\w+)', text)
      heavy = [c for c in calls if c not in _CHEAP_CALLS]
      double = c_type == 'double' or 'double' in operands or bool(heavy) or \
          bool(_DOUBLE_LITERAL.search(text))
      integer = not double and c_type not in ('float', 'double', '_Float16')
      unit = OP_COST['f64'] if double else OP_COST['f32']
      weight += unit * len(re.findall(r'(?<=[\w)\s])[-+*](?=[\s\w(])', text))
      weight += text.count('/') * OP_COST[
          'div_f64' if double else 'div_int' if integer else 'div_f32']
      for c in calls:
        weight += OP_COST['sqrt'] if c == 'sqrt' else \
            OP_COST['cheap_call'] if c in _CHEAP_CALLS else OP_COST['call']
  return weight


def default_cols(spec):
  """Columns per lane: the widest vector (<= 16 bytes) the DSL's burst width
  allows; `burst width: 512` (64 bytes per FPGA burst) gives 16-byte lanes."""
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  vec = max(elem, min(16, spec['burst_width'] // 8))
  return max(1, vec // elem)


def fused_depths(spec, max_depth):
  if len(spec['inputs']) == 1 and len(spec['outputs']) == 1 and \
      spec['inputs'][0]['c_type'] == specmod.tensor_c_types(spec)[spec['outputs'][0]]:
    # no point in a kernel deeper than the program iterates
    # 12 is the measured sweet spot for 4-byte 5-point programs on MI355X
    # (two waves per SIMD at ~200 VGPRs; 16 drops to one wave, 8 is HBM-bound)
    return [d for d in (1, 2, 4, 8, 12)
            if d <= max_depth and d <= max(1, spec['iterate'])]
  if spec['dim'] == 2 and kernel_stream2d.multi_field(spec) and \
      len(spec['outputs']) <= kernel_fields2d.MAX_OUTPUTS:
    # several fields, output j feeding input j (kernel_fields2d): every field's windows
    # of every iteration share one wavefront's registers - 8 is as deep as two- and
    # three-field programs go before the budget check refuses
    return [d for d in FIELDS_DEPTHS
            if d <= max_depth and d <= max(1, spec['iterate'])]
  return [1]


# What a workgroup of the wave-pipelined forms spends per streamed row besides
# arithmetic (barrier, ring and hand-off traffic), as VALU-cycle equivalents
# summed over its wavefronts.  Fitted to jacobi2d at 16384^2, us per step of a full
# chip: depth 16 0.98 (four workgroups per CU), 20 0.84, 24 0.96 (three per CU)
# = workgroups per CU x (0.010 us x depth + 0.080 us).
WP_STEP_FIXED_CYCLES = 640


CALIBRATION_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                'calibration.json')
CALIBRATED_FIELDS = ('step_ns_full', 'step_ns_one', 'stream_gbps', 'fade_lo_mib',
                     'fade_hi_mib', 'stream_chunk')
# ... and one the generator sets a default for, which a measurement may replace (the cap
# on workgroups per CU that goes with the measured chunk)
MEASURED_OVER_DEFAULT = ('stream_wgs_per_cu',)
_calibration = None


def calibration_key(entry, spec):
  """Identity of a generated kernel for the calibration table: the program it
  computes and every figure of its table entry except the cost figures themselves -
  a change of the generator that changes the kernel's shape makes its measurement
  stale (the scheduler then falls back to the model) until tools/calibrate.py has
  run again."""
  # (edge_slack changes which tiles a launch has, not what a workgroup's step costs: the
  # streamed loop is the same text with and without it)
  shape = {k: v for k, v in entry.items()
           if k not in CALIBRATED_FIELDS + MEASURED_OVER_DEFAULT +
           ('step_valu', 'step_bytes', 'edge_slack')}
  digest = hashlib.sha1(json.dumps(shape, sort_keys=True).encode()).hexdigest()[:12]
  return '%s/%s/%s' % (kernel_common.program_hash(spec)[:12], entry['name'], digest)


def calibration():
  global _calibration
  if _calibration is None:
    try:
      with open(CALIBRATION_FILE) as f:
        _calibration = json.load(f).get('kernels', {})
    except (OSError, ValueError):
      _calibration = {}
  return _calibration


def annotate_cost(entry, spec):
  """Cost figures of a streaming kernel for the run-time scheduler
  (soda_hip_kernel.step_valu / step_bytes, include/soda_hip.h): VALU issue
  cycles and HBM bytes of ONE workgroup per streamed row or plane.  A wave64
  instruction on `n` lane-operations' worth of cells costs 2 cycles per cell it
  covers per lane (a packed instruction covers two cells in 4 cycles: the same)."""
  elem = specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
  weight = max(1, arithmetic_weight(spec))
  waves = entry['block'][0] // kernel_stream2d.LANES
  n_in, n_out = len(spec['inputs']), len(spec['outputs'])
  if spec['dim'] == 1:
    # no streamed dimension: the figures are per workgroup per LAUNCH - every level of
    # every segment of its wavefronts, and the cells it loads and stores
    lane_cells = entry['segs'] * entry['cols']
    valu = waves * entry['depth'] * weight * lane_cells * 2
    cells_in = waves * kernel_stream2d.LANES * lane_cells
    cells_out = entry['tile'][0]
  elif spec['dim'] == 2 and 'groups' in entry:    # wave-pipelined: one strip(-pair)
    lane_cells = entry['cols'] * (2 if entry.get('pairs') else 1)
    valu = entry['depth'] * weight * lane_cells * 2 + WP_STEP_FIXED_CYCLES
    cells_in, cells_out = kernel_stream2d.LANES * lane_cells, entry['tile'][0]
  elif spec['dim'] == 2:                          # one strip per wavefront
    valu = waves * entry['depth'] * weight * entry['cols'] * 2
    cells_in = waves * kernel_stream2d.LANES * entry['cols']
    cells_out = entry['tile'][0]
  elif 'lds_planes' in entry:                     # 3-D, in-plane neighbours from LDS:
    # every wavefront computes RW x C cells per lane; the planes in LDS come with their
    # halo ring, the other inputs tile for tile (kernel_stream3d_lds: loaded_cells)
    valu = waves * weight * entry['rows'] * entry['cols'] * 2
    cells_in, cells_out = entry['loaded_cells'], entry['tile'][0] * entry['tile'][1]
    n_in = 1
  elif 'groups' in entry:                         # 3-D, one level per wavefront
    lane_cells = entry['rows'] * entry['cols']
    valu = entry['depth'] * weight * lane_cells * 2 + WP_STEP_FIXED_CYCLES
    cells_in = kernel_stream2d.LANES * lane_cells
    cells_out = entry['tile'][0] * entry['tile'][1]
  else:                                           # 3-D, one tile per wavefront
    lane_cells = entry['rows'] * entry['cols']
    valu = waves * entry['depth'] * weight * lane_cells * 2
    cells_in = waves * kernel_stream2d.LANES * lane_cells
    cells_out = entry['tile'][0] * entry['tile'][1]
  entry['step_valu'] = int(valu)
  entry['step_bytes'] = int((n_in * cells_in + n_out * cells_out) * elem)
  sizes = mixed_end_sizes(spec)
  if len(set(sizes)) > 1 and spec['dim'] == 2 and entry.get('kind') == 'fused' and \
      n_out == 1 and 'groups' not in entry:
    # inputs and output of different widths (kernel_stream2d, `mixed`): summed per tensor
    entry['step_bytes'] = int(cells_in * sum(sizes[:n_in]) + cells_out * sizes[-1])
  # measured step times of exactly this kernel, when it has been calibrated
  # (soda_hip_kernel.step_ns_full / step_ns_one / stream_gbps)
  measured = calibration().get(calibration_key(entry, spec))
  if measured:
    for field in CALIBRATED_FIELDS:
      entry[field] = int(measured.get(field, 0))
    for field in MEASURED_OVER_DEFAULT:
      if field in measured:
        entry[field] = int(measured[field])
  return entry


def prefixed_options(options, prefix, emit):
  """The `<prefix>name=value` entries of `options` as keyword arguments of `emit`;
  a name `emit` does not take is an error, not a silently ignored knob."""
  known = inspect.signature(emit).parameters
  out = {}
  for key, value in options.items():
    if key.startswith(prefix):
      if key[len(prefix):] not in known:
        raise TypeError('%s: %s() has no option `%s`' % (key, emit.__module__,
                                                         key[len(prefix):]))
      out[key[len(prefix):]] = value
  return out



# Which of generate()'s `**fused_options` a kernel form receives: the one place that says so.
# Tools pass one option set across programs of different families, so what a form does not
# receive is dropped in silence, while a name that reaches an emit() which does not take it
# is a TypeError.  fields1d, fields2d, fields3d, stream1d and stream2d_wp receive the names
# listed for them (rectangular programs under `fuse_outputs` go through fields2d / fields3d
# and receive what those receive; `fuse_outputs` itself is an argument of generate(), not a
# form option); stream2d and
# stream3d every name but those held back for the other forms (a name nobody knows therefore
# ends in their emit()); stream3d_blk and stream3d_wp the `blk_` / `wp_` names, checked
# against the emit() by prefixed_options.
FORM_OPTIONS = dict(
    fields2d=lambda k: k in FIELDS_OPTIONS,
    fields3d=lambda k: k in FIELDS3D_OPTIONS,
    fields1d=lambda k: k in FIELDS1D_OPTIONS,
    stream1d=lambda k: k in STREAM1D_OPTIONS,
    stream2d=lambda k: k not in WP_ONLY_OPTIONS + STREAM1D_OPTIONS + SELECT_2D_OPTIONS and
    k not in ('nt', 'mixed'),       # (`mixed`: set by the switch `mixed_widths` alone)
    stream2d_wp=lambda k: k in SHARED_2D_OPTIONS + WP_ONLY_OPTIONS,
    stream3d=lambda k: not k.startswith(('wp_', 'blk_')) and
    k not in ('deep3d', 'deep3d_from', 'nontemporal') + STREAM1D_OPTIONS + LDS3D_OPTIONS +
    SELECT_2D_OPTIONS,
    stream3d_lds=lambda k: k in LDS3D_OPTIONS,
    stream3d_pk=lambda k: k in PACKED3D_OPTIONS)
PREFIXED_FORMS = dict(stream3d_blk=('blk_', kernel_stream3d_blk.emit),
                      stream3d_wp=('wp_', kernel_stream3d_wp.emit))


def form_options(form, options):
  if form in PREFIXED_FORMS:
    return prefixed_options(options, *PREFIXED_FORMS[form])
  return {k: v for k, v in options.items() if FORM_OPTIONS[form](k)}


def first_fusable(spec, depth, attempts):
  """(result, None) of the first `emit(spec, depth, **kwargs)` among the `(emit, kwargs)`
  of `attempts` that does not raise NotFusable; (None, the LAST error) when all do."""
  error = None
  for emit, kwargs in attempts:
    try:
      return emit(spec, depth, **kwargs), None
    except kernel_stream2d.NotFusable as e:
      error = e
  return None, error


class Request:
  """What generate() was asked for, normalised once; every family function receives it."""

  def __init__(self, spec, max_depth, cols, chunk_rows, prefetch, depths, wave_groups,
               options, on):
    self.spec, self.depths, self.options = spec, depths, options
    # the opt-in forms asked for ({keyword: bool}, codegen/switches.py), what each LDS-plane
    # form did ({key of soda_hip_meta: note}, lds3d_kernels), and the table entries made so
    # far: an LDS-plane form is emitted only where they hold no fused depth-1 kernel
    self.on = {s.keyword: bool(on[s.keyword]) for s in switches.EVERY}
    self.meta_notes, self.made = {}, []
    # what a far-reach switch adds to the arguments of its dimensionality's forms (FAR_FORMS;
    # generate()): the switches concern programs of different dimensionality, so one dict
    self.far = {}
    # ... and what `mixed_widths` adds for a program in its class (mixed_arguments)
    self.mixed = {}
    # one-pass programs with several outputs get the fields forms at depth 1 (opt-in:
    # profiles/r12_rect.txt); such a program is in nobody else's class
    fuse_outputs = self.on['fuse_outputs']
    self.rect = fuse_outputs and kernel_stream2d.rectangular(spec)
    if fuse_outputs and not self.rect and len(spec['outputs']) >= 2 and \
        spec['dim'] in (2, 3) and not kernel_stream2d.multi_field(spec):
      self.rect_refusal = ('outputs not fused: iterate %d over %d input(s) and %d output(s) '
                           'that do not feed each other pairwise' % (
                               spec['iterate'], len(spec['inputs']), len(spec['outputs'])))
    else:
      self.rect_refusal = None
    self.max_depth = DEFAULT_MAX_DEPTH if max_depth is None else max_depth
    self.cols, self.prefetch = cols, prefetch       # as given: a form may have its own default
    # columns per lane, rows per chunk and rows in flight of the 2-D strips
    self.strip = dict(cols=cols if cols else default_cols(spec),
                      chunk_rows=chunk_rows or 256,
                      prefetch=3 if prefetch is None else prefetch)
    self.groups = WAVE_GROUPS if wave_groups is None else wave_groups
    self.single_array = len(spec['inputs']) == len(spec['outputs']) == 1
    if spec['dim'] == 3 and kernel_stream2d.multi_field(spec):
      self.default_depths = [d for d in FIELDS3D_DEPTHS if d <= max(1, spec['iterate'])]
    elif spec['dim'] == 3:
      self.default_depths = [d for d in (1, 2) if d <= max(1, spec['iterate'])] \
          if self.single_array else [1]
    elif spec['dim'] == 1 and kernel_stream2d.multi_field(spec):
      self.default_depths = [d for d in STREAM1D_DEPTHS
                             if d <= self.max_depth and d <= max(1, spec['iterate'])]
    else:
      self.default_depths = list(fused_depths(spec, self.max_depth))
    # the program is an iteration chain the fused forms can deepen (anything else gets
    # depth 1 only, whatever `depths` asks for)
    self.chain = len(self.default_depths) > 1


def chain_depths(req):
  """The depths a multi-field family wants: its defaults, or depth 1 and those asked for."""
  if req.depths is not None:
    return sorted(set([1] + list(req.depths)))
  return req.default_depths


def fused_at_depths(req, notes, wanted, attempts_of):
  """The depth loop of the families that cannot do without their depth-1 kernel: per depth of
  `wanted` the first of `attempts_of(depth)`, a list of (emit, kwargs), that fuses.  A
  refused depth leaves a note and the loop goes on - unless it was depth 1: the scheduler
  needs depth 1, without it the program keeps its per-stage kernels.  attempts_of may raise
  NotFusable itself: nothing is left to try at this depth or a deeper one."""
  for depth in wanted:
    last = depth == 1
    try:
      found, error = first_fusable(req.spec, depth, attempts_of(depth))
    except kernel_stream2d.NotFusable as nothing_to_try:
      found, error, last = None, nothing_to_try, True
    if found is not None:
      yield found
      continue
    notes.append('depth %d not fused: %s' % (depth, error))
    if last:
      return


# The far-reach forms, one per switch: the fused forms of one dimensionality with x-neighbours
# beyond the next lane (chained wave shifts, emit's `hops`).  `name`: of the form in notes.
# `max_hops`: the lanes its emit() takes.  `window_rows`: for forms that also widen the row
# window (2-D: up to FAR_MAX_PERIOD rows), the rows the depth-1 pipeline keeps for the request;
# None where there is no window.  `needs_limit`: the programs whose fused kernels are outside
# the default schedule, so that a product of the switch runs under a depth limit
# (far_depth_limit).
FarForm = collections.namedtuple('FarForm', 'switch dim name max_hops window_rows needs_limit')


def window_rows_2d(req):
  """Rows of the widest window the 2-D forms' depth-1 pipeline keeps for this request."""
  spec = req.spec
  try:
    fields = kernel_stream2d.multi_field(spec) or kernel_stream2d.rectangular(spec)
    insts, _ = kernel_stream2d.build_pipeline(spec, 1, req.strip['prefetch'], fields=fields)
    return max(inst.keep for inst in insts)
  except kernel_stream2d.NotFusable:
    return 0          # no 2-D form takes it, whatever its reach: refused as ever


FAR_FORMS = (
    FarForm('far_lanes', 2, 'far-lane', kernel_stream2d.MAX_HOPS, window_rows_2d,
            kernel_stream2d.multi_field),
    FarForm('far_taps', 1, 'far-tap', kernel_stream1d.MAX_HOPS_1D, None, lambda spec: True))


def far_arguments(form, req):
  """What the form's switch adds to the arguments of its dimensionality's emit()s for this
  request: `hops`, the lanes the lowered program reads away (form.max_hops at most: beyond,
  emit refuses as ever), and for a windowed form FAR_MAX_PERIOD - for a program of the form's
  dimensionality that those emit()s refuse a depth-1 kernel today for an x offset beyond the
  neighbour lane or for a window above their period limit; {} for every other program, whose
  text then stays what it is.  Leaves in req.meta_notes why a program is not in the class;
  far_note() says the rest.  generate() collects the results in `req.far`."""
  spec = req.spec
  if not req.on[form.switch]:
    return {}
  key = switches.BY_KEYWORD[form.switch].note
  if spec['dim'] != form.dim:
    req.meta_notes[key] = 'not fused: the %s form handles %d-D programs' % (form.name, form.dim)
    return {}
  limit = kernel_stream2d.DEFAULT_MAX_PERIOD
  hops = max([1] + [kernel_stream2d.lanes_away(rel[0], req.strip['cols'])
                    for stage in spec['stages'] for _, rel in stage['loads']])
  if hops == 1 and not (form.window_rows and
                        form.window_rows(req) > req.options.get('max_period', limit)):
    req.meta_notes[key] = 'not concerned: every read within the neighbour lanes%s' % (
        ' and %d rows' % limit if form.window_rows else '')
    return {}
  if kernel_stream2d.rectangular(spec) and not req.rect:
    req.meta_notes[key] = _NOT_RECT[1]
    return {}
  return dict(hops=min(hops, form.max_hops),
              **(dict(max_period=FAR_MAX_PERIOD) if form.window_rows else {}))


def far_note(form, req, notes):
  """The switch's entry of soda_hip_meta for a program in its class: the depth-1 kernel made,
  or why there is none.  (req.far is shared: a program of the other form's dimensionality is
  not this form's to speak of.)"""
  if not (req.on[form.switch] and req.spec['dim'] == form.dim and req.far):
    return
  made = [e['name'] for e in req.made if e['kind'] == 'fused' and e['depth'] == 1]
  why = [n[len('depth 1 not fused: '):] for n in notes if n.startswith('depth 1 not fused: ')]
  req.meta_notes[switches.BY_KEYWORD[form.switch].note] = made[0] if made else \
      'not fused: %s' % (why + ['no %d-D form takes it' % form.dim])[0]


def far_depth_limit(form, spec):
  """The depth limit under which the entry points of a product of the form's switch run.  The
  launcher admits fused kernels outside the default schedule - those over several fields, and
  every 1-D one - only under a positive limit (csrc/schedule.cpp, plans_fused), so a program
  of form.needs_limit that the switch gives its kernels runs under the depth of the deepest
  of them; 0, no limit, for every other program - a single-array 2-D program's kernels are in
  the default schedule, and a program outside the switch's class runs as it does without the
  switch."""
  if spec['dim'] != form.dim or not form.needs_limit(spec):
    return 0
  text, table = generate(spec, **{form.switch: True})
  made = kernel_common.read_meta_from_source(text).get(switches.BY_KEYWORD[form.switch].note)
  depths = [k['depth'] for k in table if k['kind'] == 'fused']
  return max(depths) if depths and made in [k['name'] for k in table] else 0


def fields2d_kernels(req, notes):
  """Multi-field 2-D programs: kernel_fields2d at each depth; rectangular ones, when
  generate() was asked to fuse their outputs, at depth 1."""
  spec = req.spec
  if spec['dim'] == 2 and req.rect_refusal:
    notes.append(req.rect_refusal)
  if spec['dim'] != 2 or not (kernel_stream2d.multi_field(spec) or req.rect):
    return
  far = req.far
  yield from fused_at_depths(req, notes, [1] if req.rect else chain_depths(req), lambda depth: [
      (kernel_fields2d.emit, dict(req.strip, **dict(far, **form_options('fields2d', req.options))))])


def fields3d_kernels(req, notes):
  """Multi-field 3-D programs: kernel_fields3d at each depth, in the tile shape that keeps
  most of the tile among those the register budget takes; rectangular ones, when generate()
  was asked to fuse their outputs, at depth 1."""
  spec = req.spec
  if spec['dim'] == 3 and req.rect_refusal:
    notes.append(req.rect_refusal)
  if spec['dim'] != 3 or not (kernel_stream2d.multi_field(spec) or req.rect):
    return

  def attempts(depth):
    options = form_options('fields3d', req.options)
    shapes = [s for s in kernel_fields3d.shapes_by_kept_fraction(spec, depth)
              if not req.cols or s[1] == req.cols]
    if req.rect:
      shapes = [s for s in shapes if s[0] * len(spec['inputs']) <= RECT3D_INPUT_ROWS]
    if 'rows' in options:
      shapes = [(options.pop('rows'), req.cols or 2)]
    if not shapes:
      raise kernel_stream2d.NotFusable('%d inputs, 3-D tiles take %d rows x inputs' % (
          len(spec['inputs']), RECT3D_INPUT_ROWS))
    return [(kernel_fields3d.emit, dict(options, rows=rows, cols=lane_cols))
            for rows, lane_cols in shapes]
  yield from fused_at_depths(req, notes, [1] if req.rect else chain_depths(req), attempts)


def fields1d_kernels(req, notes):
  """Multi-field 1-D programs: kernel_fields1d at each depth."""
  spec = req.spec
  if spec['dim'] != 1 or not kernel_stream2d.multi_field(spec):
    return
  yield from fused_at_depths(req, notes, chain_depths(req), lambda depth: [
      (kernel_fields1d.emit, dict(req.far, **dict(form_options('fields1d', req.options),
                                                   cols=req.strip['cols'])))])


def stream1d_kernels(req, notes):
  """1-D programs over one array: kernel_stream1d at each depth."""
  spec = req.spec
  if spec['dim'] != 1 or kernel_stream2d.multi_field(spec):
    return
  wanted = [d for d in req.default_depths if d in STREAM1D_DEPTHS]
  if req.depths is not None:
    wanted = sorted(set([1] + [d for d in req.depths if req.chain or d == 1]))
  yield from fused_at_depths(req, notes, wanted, lambda depth: [
      (kernel_stream1d.emit, dict(req.far, **dict(form_options('stream1d', req.options),
                                                   cols=req.strip['cols'])))])


def stream2d_depths(req):
  spec, wanted = req.spec, list(req.default_depths)
  # one level deeper for programs the packed wave-pipelined form covers: it
  # is the only form with the registers for it and, fed through the LDS ring,
  # the only one that gains from it (jacobi2d 16384^2: depth 12 single-wave
  # 46.0 us per iteration, depth 16 packed + ring 39.5)
  if (req.chain and req.max_depth >= DEFAULT_MAX_DEPTH and req.single_array and
      req.groups == -1 and kernel_stream2d_wp.packable(spec)):
    wanted += [d for d in PACKED_DEEP_DEPTHS if spec['iterate'] >= d]
  if req.depths is not None:
    wanted = sorted(set([1] + [d for d in req.depths if req.chain or d == 1]))
  return wanted


def stream2d_single(req, depth, strip, notes, far):
  """The single-wave kernel of this depth (kernel_stream2d), or None with a note.  far: what
  far_arguments() adds to the form's arguments."""
  # the memory-bound depths store around the caches when a launch's box
  # does not fit the Infinity Cache (kernel_stream2d.emit: nontemporal)
  options = dict({'nontemporal': 4} if depth <= NT_AUTO_MAX_DEPTH_2D else {},
                 **dict(far, **dict(req.mixed, **form_options('stream2d', req.options))))
  # ... and where no STAGE is read across lanes (depth 1 of the samples) their
  # strips do not overlap at all (align='exact': whole 128-byte lines in and
  # out, the seam columns from one extra vector load per row and side)
  aligns = ['exact', 'full'] if strip.get('align') == 'full' else \
      [options.pop('align', None) or strip['align']]
  if req.mixed and len(aligns) > 1:
    # a narrow lane shape of this class may keep no whole line of its narrowest tensor
    # (kernel_stream2d.geometry refuses): then strips as wide as the halo allows
    aligns.append('none')
  attempts = []
  # (the mixed-width class: every lane shape of mixed_shapes in turn, each as aligned as it
  # can be; every other program has the one shape of `strip`)
  for lane_cols in mixed_shapes(req.spec, req.cols) if req.mixed else [strip['cols']]:
    for how in aligns:
      shape = dict(strip, align=how, cols=lane_cols)
      if how == 'exact' and req.prefetch is None:
        # six rows in flight per wavefront (two workgroups per CU on the arrays
        # that matter, soda_hip_kernel.stream_wgs_per_cu)
        shape['prefetch'] = EXACT_PREFETCH
      attempts.append((kernel_stream2d.emit, dict(shape, **options)))
  single, error = first_fusable(req.spec, depth, attempts)
  if single is None and req.mixed:
    # (the note names the refusal of the FIRST lane shape, the one the program would ship in,
    # in its last alignment - not that of the last shape tried, which is mostly the register
    # estimate's for the widest lanes)
    _, error = first_fusable(req.spec, depth, attempts[:len(aligns)])
  if single is None:
    notes.append('depth %d not fused: %s' % (depth, error))
  return single


# The wave-pipelined form at this depth: always when asked for by a number of wavefronts;
# when left to choose (WAVE_GROUPS, -1), where the single-wave form does not fit or needs
# more than AUTO_WP_VGPRS registers, and for packable programs from PACKED_FROM_DEPTH on
# (the measurements are at those constants).
def want_piped(req, depth, single):
  return depth >= WAVE_PIPELINE_MIN_DEPTH and (
      req.groups > 1 or (req.groups == -1 and (
          single is None or single[1]['est_vgprs'] > AUTO_WP_VGPRS or
          (depth >= PACKED_FROM_DEPTH and kernel_stream2d_wp.packable(req.spec)))))


# A chosen ring kernel a few registers over four workgroups per CU (128 VGPRs) is built a
# second time under that cap (stream2d_piped says how, per form).
def squeeze(req, options, entry):
  return (req.groups == -1 and options.get('ring') and
          'waves_per_eu' not in options and
          128 < entry['est_vgprs'] <= AUTO_WP_SQUEEZE_VGPRS)


def stream2d_piped(req, depth, strip, notes):
  """The wave-pipelined kernel of this depth (kernel_stream2d_wp), or None with a note."""
  spec, groups = req.spec, req.groups
  options = form_options('stream2d_wp', req.options)
  if groups == -1:
    options.setdefault('vgpr_budget', AUTO_WP_BUDGET)
    lane_bytes = strip['cols'] * specmod.ELEM_SIZE[spec['inputs'][0]['c_type']]
    if lane_bytes == 16:
      # input rows through the LDS ring: no prefetch registers (see
      # kernel_stream2d_wp.emit); needs 16-byte lanes
      options.setdefault('ring', AUTO_WP_RING)
    # packable programs: one 512-column strip per wavefront, its two halves
    # sharing register pairs (pairs=2; jacobi2d depth 16 per launch on
    # 16384^2: 597 us against 627 us for two 256-column strips, pairs=1)
    options.setdefault('pairs', 0 if not kernel_stream2d_wp.packable(spec)
                       else 2 if options.get('ring') else 1)
    if depth > PACKED_DEEP_DEPTH and options['pairs'] == 2:
      # 5-6 levels per wavefront: three workgroups per CU (168 VGPRs;
      # depth 24 left alone takes 174 = two per CU: 34.1 vs 33.2 us per
      # iteration at 16384^2)
      options.setdefault('waves_per_eu', PACKED_DEEP_WAVES_PER_EU)
  emit = kernel_stream2d_wp.emit
  piped, error = first_fusable(spec, depth, [
      (emit, dict(strip, groups=AUTO_WP_GROUPS if groups == -1 else groups, **options))])
  if piped is not None and squeeze(req, options, piped[1]):
    capped = None
    if options.get('pairs') == 2 and options['ring'] == AUTO_WP_RING \
        and 'max_period' not in options:
      # a few registers over four workgroups per CU: cap them at 128.  In
      # the wide form that pays only together with a 12-slot ring (10 rows
      # in flight) unrolled over 12 rows: jacobi2d depth 16, 16384^2, per
      # launch 578 us uncapped with ring 6, 830 us capped with ring 6,
      # 560 us capped with ring 12.
      capped = dict(options, ring=2 * AUTO_WP_RING, max_period=2 * AUTO_WP_RING)
    elif not options.get('pairs'):
      # the scalar form: let the compiler spill the few registers over the cap
      # (not the two-strip packed form: its scalar DPP adds then spill 45
      # registers and lose 60 %)
      capped = options
    if capped is not None:
      # (a capped kernel that does not fuse leaves the first one, and a note)
      again, error = first_fusable(spec, depth, [
          (emit, dict(strip, groups=AUTO_WP_GROUPS, waves_per_eu=4, **capped))])
      piped = again or piped
  if error is not None:
    notes.append('depth %d not wave-pipelined: %s' % (depth, error))
  return piped


def stream2d_wide12(req, depth, strip, piped, notes):
  """The 12-column-lane kernel of this depth next to (or instead of) the shipped wide packed
  kernel `piped`, or None: only where the default selection chose that form in 16-byte lanes."""
  how = int(req.options.get('wide12', WIDE12_DEFAULT))
  if not how or depth not in WIDE12_DEPTHS or req.groups != -1 or req.cols or \
      piped is None or piped[1].get('pairs') != 2 or piped[1]['cols'] != 4:
    return None
  options = dict(WIDE12_OPTIONS, **{k: v for k, v in form_options('stream2d_wp', req.options).items()
                                    if k not in WIDE12_OPTIONS})
  found, error = first_fusable(req.spec, depth, [
      (kernel_stream2d_wp.emit, dict(dict(strip, groups=AUTO_WP_GROUPS), **options))])
  if found is None:
    notes.append('depth %d not in 12-column lanes: %s' % (depth, error))
  return found


def stream2d_kernels(req, notes):
  """Single-array 2-D programs: per depth the wave-pipelined kernel, else the single-wave;
  at WIDE12_DEPTHS the 12-column-lane kernel as a same-depth alternative."""
  spec = req.spec
  if spec['dim'] != 2 or kernel_stream2d.multi_field(spec) or req.rect:
    return
  far = req.far
  for depth in stream2d_depths(req):
    strip = dict(req.strip)
    if 'align' not in req.options:
      # (deeper kernels keep the widest strips: strips on 64-byte pieces,
      # align='store64', gain 1.8 % on cfg2 in short runs and LOSE 1.3 % under the
      # bench protocol's sustained load - 0.949 vs 0.961 ms, three alternating pairs
      # in one call; cfg4 29.17 vs 29.22 ms)
      strip['align'] = 'full' if (
          depth <= ALIGN_FULL_MAX_DEPTH and
          arithmetic_weight(spec) <= ALIGN_FULL_MAX_WEIGHT) else 'none'
    single = piped = None
    if req.groups <= 1 or depth < WAVE_PIPELINE_MIN_DEPTH:
      single = stream2d_single(req, depth, strip, notes, far)
    if want_piped(req, depth, single):
      piped = stream2d_piped(req, depth, strip, notes)
      if piped is None and single is None and req.groups > 1:
        # asked for by a number of wavefronts and refused: the single-wave form after all
        single, error = first_fusable(spec, depth, [
            (kernel_stream2d.emit,
             dict(strip, **dict(far, **form_options('stream2d', req.options))))])
        if single is None:
          notes.append('depth %d not fused: %s' % (depth, error))
    # (the alternative first: whoever looks a depth up in the table finds the shipped kernel
    # last; the run-time takes neither by its place)
    wide12 = stream2d_wide12(req, depth, strip, piped, notes)
    if wide12 is not None:
      yield wide12
    if (piped is not None or single is not None) and not (
        wide12 is not None and int(req.options.get('wide12', WIDE12_DEFAULT)) == 2):
      yield piped if piped is not None else single


def stream3d_kernels(req, notes):
  """3-D programs, depths 1 and 2: one tile per wavefront (kernel_stream3d)."""
  spec, cols = req.spec, req.cols
  if spec['dim'] != 3 or kernel_stream2d.multi_field(spec) or req.rect:
    return
  wanted = req.default_depths
  if req.depths is not None:
    wanted = sorted(set([1] + list(req.depths))) if req.chain else [1]
  for depth in wanted:
    options = form_options('stream3d', req.options)
    # (rows, columns) per lane: the tallest tile the register file allows (taller
    # tiles waste less on the y halo).  Programs with several live tensors
    # (denoise3d, lowered to g and output over the inputs f and u) fit with one
    # column per lane: 12 rows (156 VGPRs, three wavefronts per SIMD) before 16
    # (235 VGPRs, two) - denoise3d per sweep at 256^3 / 512^3: 160 / 971 us against
    # 200 / 999 us, the two per-stage launches 165 / 1281 us
    narrow = [] if cols or len(spec['inputs']) == len(spec['outputs']) else \
        [(12, 1), (16, 1)]      # (iteration chains go deep in the forms below)
    shapes = [(options.pop('rows'), cols or 2)] if 'rows' in options else \
        [(16, cols or 2), (12, cols or 2)] + narrow
    options.setdefault('nt', 4)
    found, error = first_fusable(spec, depth, [
        (kernel_stream3d.emit, dict(options, rows=rows, cols=lane_cols))
        for rows, lane_cols in shapes])
    if found is None:
      notes.append('depth %d not fused: %s' % (depth, error))
    else:
      yield found


def deep3d_block(req, depth, notes):
  """The block form of this depth (kernel_stream3d_blk), or None with a note."""
  # block form: all levels in every wavefront, edge rows through LDS
  # (kernel_stream3d_blk).  Named <app>_fused_k<d>b; with 'both' it ships
  # NEXT TO the wave-pipelined kernel and the run-time picks per launch
  spec = req.spec
  given = form_options('stream3d_blk', req.options)
  heavy = arithmetic_weight(spec) > PACKED_3D_LIGHT_WEIGHT
  ring_forms = [dict(BLOCK_3D_RING_OPTIONS)]
  if heavy and kernel_stream2d_wp.packable(spec):
    # heavy plain-float programs: packed pair-rows first (heat3d 512^3 x20,
    # block form alone, clocks warm: 1.76 ms plain, 1.42 packed - 13.2 k instead
    # of 22.6 k VALU instructions per unrolled loop, 254 VGPRs without spills
    # now that the ring took the prefetch registers; a hand-ordered scalar
    # instruction stream, round 3's kernel_asm, reached 1.49 and is gone)
    # (and exact store ranges: whole 64-byte pieces cost this kernel 3 %,
    # heat3d 512^3 x20 1.37 -> 1.41 ms, where they gain jacobi3d's 2 %)
    ring_forms.insert(0, dict(BLOCK_3D_RING_OPTIONS, pairs=1, wide_stores=0))
  bases = [BLOCK_3D_OPTIONS] if 'prefetch' in given or 'ring' in given else \
      ring_forms + [BLOCK_3D_OPTIONS]
  found, error = first_fusable(spec, depth, [
      (kernel_stream3d_blk.emit, dict(base, **given)) for base in bases])
  if found is None:
    notes.append('depth %d not in block form: %s' % (depth, error))
  return found


def deep3d_piped(req, depth, notes):
  """The wave-pipelined kernel of this depth (kernel_stream3d_wp), or None with a note."""
  spec = req.spec
  options = form_options('stream3d_wp', req.options)
  options.setdefault('groups', min(depth * len(spec['stages']), 4))
  # (no non-temporal stores here: heat3d 512^3 x20 with this form alone 2.09 ms
  # without, 2.12 ms with wp_nt=4)
  if options.get('split', 2) == 2 and not options.get('loader') and \
      options.get('rows', 16) % 2 == 0 and kernel_stream2d_wp.packable(spec):
    # packed pair-rows (v_pk_*_f32) for programs heavy enough on arithmetic:
    # heat3d (weight 15) 459 us per launch scalar, 383-440 us packed at the
    # 230 VGPRs the compiler asks for (629 us capped at three workgroups per
    # CU: 360 spilled registers).  Light programs are bounded by memory and
    # keep the scalar form at three workgroups per CU: jacobi3d (weight 7),
    # cfg5 with the offline compiler: 6.23 ms scalar, 7.43 ms packed (36
    # spilled registers); hiprtc happens to favour the packed form (6.31 vs
    # 6.63 ms) - the shipped code objects are built by hipcc.
    options.setdefault('pairs', int(arithmetic_weight(spec) >
                                    PACKED_3D_LIGHT_WEIGHT))
    if options['pairs']:
      options.setdefault('waves_per_eu', 0)
  found, error = first_fusable(spec, depth, [(kernel_stream3d_wp.emit, options)])
  if found is None:
    notes.append('depth %d not wave-pipelined: %s' % (depth, error))
  return found


def deep3d_kernels(req, notes):
  """Light 3-D iteration chains: per depth the block form, the wave-pipelined or both."""
  spec, depths = req.spec, req.depths
  if spec['dim'] != 3:
    return
  # deeper than one wavefront's registers allow: one level per wavefront
  # The block form serves the shallow depths as well (deep3d_from=3: not): next to the
  # single-wave kernels above, which stay for arrays below its 128 x 64 tile and for
  # programs it does not take.  jacobi3d per launch, depth 1 / 2: 512^3 470 / 395 us
  # single-wave, 221 / 222 us block form (one read and one write of the array at 5.3
  # TB/s: 203 us); 256^3 67 / 65 against 33 / 35; heat3d 512^3 depth 2 464 -> 231.
  deep_from = req.options.get('deep3d_from', 1)
  deep = [d for d in sorted(set(depths if depths is not None else
                                BLOCK_3D_SHALLOW_DEPTHS + DEEP_3D_DEPTHS))
          if d >= deep_from and d <= max(1, spec['iterate'])]
  if not (req.single_array and (
      depths is not None or arithmetic_weight(spec) <= DEEP_3D_MAX_WEIGHT)):
    return
  form = req.options.get('deep3d', DEEP_3D_FORM)
  for depth in deep:
    if depth < 3 and form == 'wp':      # one level per wavefront needs >= 3 levels
      continue
    if form in ('blk', 'both'):
      found = deep3d_block(req, depth, notes)
      if found is not None:
        yield found
      # (a depth >= 3 the block form refused goes on to the wave-pipelined form,
      # with deep3d='blk' as well)
      if depth < 3 or (form == 'blk' and found is not None):
        continue
    found = deep3d_piped(req, depth, notes)
    if found is not None:
      yield found


def packed3d_kernels(req, notes):
  """3-D programs over 8- and 16-bit integer volumes, when generate() was asked for packed
  cells: kernel_stream3d_pk at depth 1, and at depth 2 for an iteration chain, in the tile
  shape that keeps most of the tile among those the register budget takes.  What the switch
  did goes into req.meta_notes, not into `notes`: apart from the metadata, the text of a
  program outside the class is the same with and without the switch."""
  if not req.on['packed_cells']:
    return
  spec = req.spec
  key = switches.BY_KEYWORD['packed_cells'].note
  types = specmod.tensor_c_types(spec)
  ends = [t['c_type'] for t in spec['inputs']] + [types[o] for o in spec['outputs']]
  if all(specmod.ELEM_SIZE[t] >= 4 for t in ends):
    req.meta_notes[key] = 'not concerned: 4- or 8-byte elements'
    return
  why = kernel_stream3d_pk.class_refusal(spec)
  if why:
    req.meta_notes[key] = 'not fused: %s' % why
    return
  chain = req.single_array and ends[0] == ends[-1]
  wanted = [d for d in PACKED3D_DEPTHS if d <= max(1, spec['iterate'])] if chain else [1]
  if req.depths is not None and chain:
    wanted = sorted(set([1] + [d for d in req.depths if d in PACKED3D_DEPTHS]))
  refusals = []

  def attempts(depth):
    options = form_options('stream3d_pk', req.options)
    shapes = [s for s in kernel_stream3d_pk.shapes_by_kept_fraction(spec, depth)
              if not req.cols or s[1] == req.cols]
    if 'rows' in options:
      shapes = [(options.pop('rows'), req.cols or shapes[0][1])]
    # stores around the caches for boxes beyond the Infinity Cache, as kernel_stream3d's
    options.setdefault('nt', 4)
    # most waves per SIMD first, then most of the tile kept (kernel_stream3d_pk.TILE_SHAPES
    # has the measurements); an occupancy or a budget given as an option is the only level
    levels = kernel_stream3d_pk.OCCUPANCY_LEVELS
    if 'waves_per_eu' in options or 'vgpr_budget' in options:
      levels = [(options.get('waves_per_eu', 2), options.get('vgpr_budget', 240))]
    return [(kernel_stream3d_pk.emit, dict(options, rows=rows, cols=lane_cols,
                                           waves_per_eu=waves, vgpr_budget=budget))
            for waves, budget in levels for rows, lane_cols in shapes]
  # (the cost figures of annotate_cost are the single-wave 3-D form's model: no calibration
  # key exists for these kernels, their price is unmeasured)
  made = None
  for found in fused_at_depths(req, refusals, wanted, attempts):
    made = made or found[1]['name']
    yield found
  req.meta_notes[key] = made or 'not fused: %s' % refusals[0][len('depth 1 not fused: '):]
  notes.extend(n for n in refusals if made)


# The LDS-plane forms (kernel_stream3d_lds), one per switch.  `fields`: the form over
# several outputs - for the plane ring, which takes one output or several, a function of the
# request.  `ring`: several planes of an input in LDS.  `refusals`: in the order they are
# checked, (condition, note) over the request and the name of a fused depth-1 kernel another
# family made ('' if none).  A rectangular program is in the fields form's class, as in
# anyone's, only under `fuse_outputs` (Request.rect).
LdsForm = collections.namedtuple('LdsForm', 'switch fields ring refusals')
_NOT_3D = (lambda req, have: req.spec['dim'] != 3,
           'not fused: the LDS-plane form handles 3-D programs')
_NOT_WANTED = (lambda req, have: bool(have), 'not wanted: {have}')
_NOT_RECT = (lambda req, have: kernel_stream2d.rectangular(req.spec) and not req.rect,
             'not fused: a one-pass program with several outputs is fused only with fuse_outputs')
LDS_PLANES = LdsForm('lds_planes', False, False, (_NOT_3D, _NOT_WANTED))
LDS_FIELDS = LdsForm('lds_fields', True, False, (
    (lambda req, have: len(req.spec['outputs']) < 2, 'not concerned: one output'),
    _NOT_WANTED, _NOT_3D, _NOT_RECT))
LDS_RING = LdsForm('lds_ring', lambda req: len(req.spec['outputs']) > 1, True, (
    _NOT_3D, _NOT_WANTED,
    (lambda req, have: all(len(planes) <= 1 for planes in
                           kernel_stream3d_lds.planes_off_axis(req.spec).values()),
     'not concerned: one plane per input, lds_planes / lds_fields take it'),
    _NOT_RECT))


def lds3d_kernels(form, req, notes):
  """3-D programs no other family gave a fused depth-1 kernel, when generate() was asked
  for this LDS-plane form: kernel_stream3d_lds, in the first shape that fits.  The forms
  come last in FAMILIES, the plane ring last of them.  What a form did goes into req.meta_notes under its switch's key of
  soda_hip_meta, not into `notes`: apart from the metadata, the text of a program the form
  does not take is the same with and without the switch."""
  if not req.on[form.switch]:
    return
  key = switches.BY_KEYWORD[form.switch].note
  have = ([e['name'] for e in req.made if e['kind'] == 'fused' and e['depth'] == 1] + [''])[0]
  for refused, note in form.refusals:
    if refused(req, have):
      req.meta_notes[key] = note.format(have=have)
      return
  shape = form_options('stream3d_lds', req.options).get('lds_shape')
  kwargs = dict(zip(('waves', 'rows', 'lanes_x'), shape)) if shape else {}
  kwargs['fields'] = form.fields(req) if callable(form.fields) else form.fields
  if form.ring:
    kwargs['ring'] = True
  found, error = first_fusable(req.spec, 1, [(kernel_stream3d_lds.emit, kwargs)])
  if found is None:
    req.meta_notes[key] = 'not fused: %s' % error
    return
  req.meta_notes[key] = found[1]['name']
  yield found


# the kernel families in the order their kernels enter the table; each yields the
# (text, entry) of the kernels it selects for this request and appends to `notes`
FAMILIES = (fields2d_kernels, fields3d_kernels, fields1d_kernels, stream1d_kernels,
            stream2d_kernels, stream3d_kernels, deep3d_kernels, packed3d_kernels,
            functools.partial(lds3d_kernels, LDS_PLANES),
            functools.partial(lds3d_kernels, LDS_FIELDS),
            functools.partial(lds3d_kernels, LDS_RING))


def generate(spec, max_depth=None, cols=None, chunk_rows=None, prefetch=None,
             fused=True, depths=None, inline=True, wave_groups=None,
             fuse_outputs=False, lds_planes=False, lds_fields=False, far_lanes=False,
             lds_ring=False, far_taps=False, packed_cells=False, mixed_widths=False,
             **fused_options):
  """Returns (kernel text, kernel table).  `depths` overrides the default set
  of fused depths (depth 1 is always included: the scheduler needs it).
  `fuse_outputs`: a one-pass 2-D / 3-D program with several outputs that is not
  multi_field (kernel_stream2d.rectangular) gets ONE fused depth-1 kernel that stores
  every output (kernel_fields2d / kernel_fields3d) besides its per-stage kernels; the
  run-time launches it under a depth limit of 1 (soda_hip_plan_set_max_depth).  Without
  it such a program keeps per-stage kernels only.
  `lds_planes`: a 3-D program of one stage that no other form gives a fused depth-1 kernel
  (a window wider than a lane's columns: stars of radius 3 and up) gets the LDS-plane
  kernel `<app>_fused_k1l` (kernel_stream3d_lds); every other program keeps its table and,
  apart from the entry `lds_planes` of soda_hip_meta that says what the switch did, its
  text.  Without it nothing changes.
  `lds_fields`: the same form over several outputs, `<app>_fused_k1lf`, for a 3-D program
  with two or three outputs that read inputs only (a wave time loop handing its fields on,
  a high-order gradient - the latter with `fuse_outputs` as well) and that no other form
  gives a fused depth-1 kernel; launched under a depth limit of 1 like every fused kernel
  over several outputs.  Every other program keeps its table and, apart from the entry
  `lds_fields` of soda_hip_meta, its text.  The two LDS switches concern disjoint programs
  and may be given together.
  `lds_ring`: the same form with a RING of planes in LDS, `<app>_fused_k1r` for one output
  and `<app>_fused_k1rf` for two or three, for a 3-D program in the scope of the two forms
  above that reads an input off the z axis in more than one plane (mixed derivatives
  d2/dxdz, rotated operators) and that no other form gives a fused depth-1 kernel; launched
  under a depth limit of 1.  A program that reads every input off the z axis in at most one
  plane is not concerned, so the three LDS switches concern disjoint programs and may be
  given together.  Every other program keeps its table and, apart from the entry `lds_ring`
  of soda_hip_meta, its text.
  `far_lanes`: a 2-D program that kernel_stream2d / kernel_fields2d refuse a depth-1 kernel
  because it reads an x-neighbour beyond the next lane (float stars of radius 5 and up,
  double ones of radius 3 and up) or keeps a window above 12 rows gets the same forms with
  chained wave shifts (`hops`, up to kernel_stream2d.MAX_HOPS lanes) and a rotation period of
  up to FAR_MAX_PERIOD, at the family's usual depths and under the usual names
  `<app>_fused_k<d>`, in the default schedule; a rectangular one with `fuse_outputs` as well.
  Every other program keeps its table and, apart from the entry `far_lanes` of
  soda_hip_meta, its text.
  `far_taps`: a 1-D program that kernel_stream1d / kernel_fields1d refuse because it reads an
  x-neighbour beyond the next lane (a float FIR of more than 9 taps, a double stencil of
  radius 3 and up) gets the same forms with chained wave shifts (`hops`, up to
  kernel_stream1d.MAX_HOPS_1D lanes), at the family's usual depths and under the usual names
  `<app>_fused_k<d>`; like every fused 1-D kernel they are launched under a depth limit
  (switches.depth_limit_of).  Every other program keeps its table and, apart from the entry
  `far_taps` of soda_hip_meta, its text.
  `packed_cells`: a 3-D program with one output whose inputs and output are integers of one
  width, 1 or 2 bytes (locals of 1, 2 or 4 bytes), gets kernel_stream3d's kernels with packed
  windows (kernel_stream3d_pk) under the usual names `<app>_fused_k1` and, for an iteration
  chain, `_k2`, in the default schedule.  Every other program keeps its table and, apart
  from the entry `packed_cells` of soda_hip_meta, its text.
  `mixed_widths`: a 2-D program with one output where some input's element size differs from
  another input's or from the output's (sizes of 1, 2, 4 or 8 bytes, no `half`; uint8 pixels
  to float, float and a uint8 map to uint16), which kernel_stream2d refuses with `inputs and
  output of different widths`, gets ONE kernel `<app>_fused_k1` of that form with every
  tensor's loads and stores in its own width, in the default schedule; depth 1 only, since
  the DSL iterates between equal types.  The lane shape is the first of mixed_shapes() the
  register estimate takes, or `cols`.  Not together with `far_lanes`: a program in the class
  that reads beyond the neighbour lane keeps its per-stage kernels.  Every other program
  keeps its table and, apart from the entry `mixed_widths` of soda_hip_meta, its text."""
  given = locals()      # every row of switches.EVERY is a parameter above: read by keyword
  # kernels are generated from the LOWERED program (pointwise-only locals folded
  # into their readers); the blob is still identified by the source program
  source = spec
  spec = specmod.inline_pointwise(spec) if inline else spec
  parts = [kernel_common.prelude(source, __version__)]
  if extra_flags(source):
    parts.append('%s %s\n' % (FLAGS_MARK, ' '.join(extra_flags(source))))
  wrappers = kernel_common.math_wrappers(kernel_common.used_functions(spec))
  if wrappers:
    parts.append('// math calls resolve as in the reference CPU path: C double '
                 'functions\n' + '\n'.join(wrappers) + '\n')
  text, table = kernel_stage.emit(spec)
  parts.append(text)
  notes = []
  req = Request(spec, max_depth, cols, chunk_rows, prefetch, depths, wave_groups,
                fused_options, {s.keyword: given[s.keyword] for s in switches.EVERY})
  for form in FAR_FORMS:
    req.far.update(far_arguments(form, req))
  req.mixed = mixed_arguments(req)
  for family in FAMILIES if fused else ():
    for ftext, entry in family(req, notes):
      parts.append(ftext)
      table.append(annotate_cost(entry, spec))
      req.made.append(entry)
  for form in FAR_FORMS:
    far_note(form, req, notes)
  mixed_note(req, notes)
  if notes:
    parts.append(''.join('// %s\n' % n for n in notes))
  extra = dict(program_hash=kernel_common.program_hash(source),
               source_stages=[s['name'] for s in source['stages']])
  extra.update(req.meta_notes)
  parts.append(kernel_common.meta_symbol(spec, table, extra=extra))
  return '\n'.join(parts), table


def compile_to_code_object(text, out_path, hipcc=None, extra_flags=()):
  """Offline build of the blob (the role `--xocl-hw-xo` plays in the reference:
  invoking the vendor tool chain from the compiler driver)."""
  hipcc = hipcc or os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
  with tempfile.NamedTemporaryFile('w', suffix='.hip', delete=False) as f:
    f.write(text)
    src = f.name
  try:
    subprocess.check_call([hipcc] + HIPCC_FLAGS + flags_from_text(text) +
                          list(extra_flags) + [src, '-o', out_path])
  finally:
    os.unlink(src)
  return out_path
