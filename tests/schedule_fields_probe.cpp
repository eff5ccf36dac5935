// Test probe of the launch planner's per-field entry (soda-compiler_amd/csrc/schedule.cpp:
// build_schedule_fields), built by tests/test_schedule_fields.py with the host compiler
// alone.  As tests/schedule_probe.cpp, with a valid region per input.  Request (native
// endianness, no padding):
//   int32 n_kernels; soda_hip_program; soda_hip_kernel[n_kernels];
//   int32 cus; int64 lds_per_cu; int32 resident_blocks[n_kernels]; int32 static_lds[n_kernels];
//   int32 n_cases; then per case
//   int32 max_depth, out_final_only, iterate, entry; int64 dims[4];
//   int32 valid_lo[n_inputs][4], valid_hi[n_inputs][4]
// entry 0 = build_schedule_fields; 1 = build_schedule with the margins of input 0 (the
// single-margin entry).  ONE planner plans every case of a request, so that compositions
// from different regions share its memo tables as they do in a plan.
#include "schedule.h"

#include <cstdio>
#include <cstdlib>

namespace {

FILE* g_in;

template <typename T>
T get() {
  T v;
  if (fread(&v, sizeof v, 1, g_in) != 1) {
    fprintf(stderr, "schedule_fields_probe: request ends early\n");
    exit(2);
  }
  return v;
}

const char* kTag = "-ioabl";   // Buffer::Kind, in order

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: schedule_fields_probe REQUEST\n");
    return 2;
  }
  Planner plan;
  const int n = get<int32_t>();
  plan.prog = get<soda_hip_program>();
  for (int k = 0; k < n; ++k) plan.kernels.push_back(get<soda_hip_kernel>());
  plan.cus = get<int32_t>();
  plan.lds_per_cu = get<int64_t>();
  for (int k = 0; k < n; ++k) plan.resident_blocks.push_back(get<int32_t>());
  for (int k = 0; k < n; ++k) plan.static_lds.push_back(get<int32_t>());
  const int n_cases = get<int32_t>();
  for (int c = 0; c < n_cases; ++c) {
    plan.max_depth = get<int32_t>();
    plan.out_final_only = get<int32_t>() != 0;
    const int iterate = get<int32_t>();
    const int entry = get<int32_t>();
    int64_t dims[4];
    int32_t vlo[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS], vhi[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS];
    for (int d = 0; d < 4; ++d) dims[d] = get<int64_t>();
    for (int j = 0; j < plan.prog.n_inputs; ++j)
      for (int d = 0; d < 4; ++d) vlo[j][d] = get<int32_t>();
    for (int j = 0; j < plan.prog.n_inputs; ++j)
      for (int d = 0; d < 4; ++d) vhi[j][d] = get<int32_t>();
    std::vector<Launch> list;
    int depth = 0;
    ScratchNeeds needs;
    const int rc = entry == 1
        ? build_schedule(&plan, dims, iterate, vlo[0], vhi[0], &list, &depth, &needs)
        : build_schedule_fields(&plan, dims, iterate, vlo, vhi, &list, &depth, &needs);
    printf("case %d rc %d launches %zu depth %d needs %d %d %d\n", c, rc, rc ? 0 : list.size(),
           depth, needs.pingpong, needs.second, needs.locals);
    if (rc) {
      printf("error %s\n", g_last_error.c_str());
      continue;
    }
    for (const Launch& l : list) {
      const soda_hip_args& a = l.args;
      printf("L %d lo %lld %lld %lld %lld hi %lld %lld %lld %lld grid %u %u %u "
             "param %lld %lld %lld %lld lds %u est %.6f buf", l.kernel,
             (long long)a.box_lo[0], (long long)a.box_lo[1], (long long)a.box_lo[2],
             (long long)a.box_lo[3], (long long)a.box_hi[0], (long long)a.box_hi[1],
             (long long)a.box_hi[2], (long long)a.box_hi[3], l.grid[0], l.grid[1], l.grid[2],
             (long long)a.param[0], (long long)a.param[1], (long long)a.param[2],
             (long long)a.param[3], l.lds_bytes, l.est_us);
      for (int t = 0; t < n_tensors(plan.prog); ++t)
        printf(" %c%d", kTag[l.buffer[t].kind], (int)l.buffer[t].index);
      printf("\n");
    }
  }
  return 0;
}
