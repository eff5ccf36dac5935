"""The 12-column-lane deep 2-D kernels `<app>_fused_k24w` / `k20w` (kernel_stream2d_wp.emit
with cols=6, chosen by kernel.stream2d_wide12): what the generator emits, without a GPU.
Instruction counts of the compiled code are measured figures (profiles/r18_wide12.txt), not
assertions."""
import re
import subprocess

from soda_hip.codegen import kernel

from codegen_util import spec_of


def generated(**options):
  return kernel.generate(spec_of('jacobi2d', iterate=1000), **options)


def test_wide12_kernels_next_to_the_shipped_ones():
  text, table = generated()
  by_name = {k['name']: k for k in table}
  assert 'jacobi2d_fused_k16w' not in by_name       # depth 16 keeps four workgroups per CU
  # (the halo is padded to whole 6-column half-lanes: 24 columns at depth 20 as well)
  for depth, tile in ((24, 720), (20, 720)):
    w, shipped = by_name['jacobi2d_fused_k%dw' % depth], by_name['jacobi2d_fused_k%d' % depth]
    assert w['depth'] == shipped['depth'] == depth
    assert w['cols'] == 6 and w['pairs'] == 2 and w['ring'] == 6 and w['groups'] == 4
    assert w['tile'][0] == tile == 768 - 2 * 6 * -(-depth // 6) and w['min_extent'] == [768, 1]
    assert w['block'] == [256, 1, 1] and w['origin_align'] == 4
    assert w['est_vgprs'] <= 256
    assert w['fill_rows'] == shipped['fill_rows']
    # both carry a measured record: the run-time compares measured prices per launch
    assert w.get('step_ns_full', 0) > 0 and shipped.get('step_ns_full', 0) > 0
    # two workgroups per CU, each its own barrier domain of four wavefronts
    assert ('GLOBAL WG_SIZE(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void '
            'jacobi2d_fused_k%dw(' % depth) in text
  # LDS: 18 KB of hand-off rows and 18 KB of ring per workgroup, in 16-byte pieces [piece][lane]
  body = text[text.index('void jacobi2d_fused_k24w('):]
  assert 'float handoff[3][2][1][3][256];' in body and 'float in_ring[6][3][256];' in body


def test_header_lists_four_waves_of_six_levels():
  text, _ = generated(depths=[24], wide12=2)
  head = text[text.index('// fused depth-24 kernel, wave-pipelined: 4 wavefronts per strip'):]
  head = head[:head.index('typedef')]
  assert 'strip = 768 columns (720 out + halo 24/24)' in head
  levels = {}
  for wave, ident in re.findall(r'//   wave (\d)  (k\d+_\S+)', head):
    levels.setdefault(int(wave), []).append(ident)
  assert sorted(levels) == [0, 1, 2, 3]
  assert all(len(v) == 6 for v in levels.values()), levels


def test_wide12_option_and_the_unchanged_default_text():
  """wide12=0 is the generator without the form (every other kernel's text is the same
  with and without it), wide12=2 the form alone at its depths."""
  text1, table1 = generated()
  text0, table0 = generated(wide12=0)
  names0 = [k['name'] for k in table0]
  assert not [n for n in names0 if n.endswith('w')]
  assert [k['name'] for k in table1 if not k['name'].endswith('w')] == names0
  assert [k for k in table1 if not k['name'].endswith('w')] == table0
  for name in names0:
    start = 'void %s(soda_hip_args a) {' % name
    assert text1.count(start) == text0.count(start) == 1
  only = [k['name'] for k in generated(depths=[24, 20], wide12=2)[1] if k['kind'] == 'fused']
  assert only == ['jacobi2d_fused_k1', 'jacobi2d_fused_k20w', 'jacobi2d_fused_k24w']
  # programs outside the wide packed form, and narrower or wider lanes asked for, get none
  assert not [k for k in kernel.generate(spec_of('blur', iterate=100))[1]
              if k['name'].endswith('w')]
  assert not [k for k in kernel.generate(spec_of('jacobi2d', iterate=1000), cols=4)[1]
              if k['name'].endswith('w')]


def test_wide12_text_compiles_for_gfx950(tmp_path):
  text, _ = generated(depths=[24, 20], wide12=2)
  src = tmp_path / 'wide12.hip'
  src.write_text(text)
  flags = [f for f in kernel.HIPCC_FLAGS if f != '--no-gpu-bundle-output']
  subprocess.check_call(['/opt/rocm/bin/hipcc'] + flags + kernel.flags_from_text(text) +
                        ['-fsyntax-only', str(src)])
