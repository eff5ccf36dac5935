// Test probe of the launch planner (soda-compiler_amd/csrc/schedule.cpp), built by
// tests/test_schedule.py with the host compiler alone: plans the cases of one binary
// request file and prints every launch.  Request (native endianness, no padding):
//   int32 n_kernels; soda_hip_program; soda_hip_kernel[n_kernels];
//   int32 cus; int64 lds_per_cu; int32 resident_blocks[n_kernels]; int32 static_lds[n_kernels];
//   int32 n_cases; then per case
//   int32 max_depth, out_final_only, iterate, n_split, split[8]; int64 dims[4];
//   int32 valid_lo[4], valid_hi[4]
#include "schedule.h"

#include <cstdio>
#include <cstdlib>

namespace {

FILE* g_in;

template <typename T>
T get() {
  T v;
  if (fread(&v, sizeof v, 1, g_in) != 1) {
    fprintf(stderr, "schedule_probe: request ends early\n");
    exit(2);
  }
  return v;
}

const char* kTag = "-ioabl";   // Buffer::Kind, in order

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: schedule_probe REQUEST\n");
    return 2;
  }
  Planner base;
  const int n = get<int32_t>();
  base.prog = get<soda_hip_program>();
  for (int k = 0; k < n; ++k) base.kernels.push_back(get<soda_hip_kernel>());
  base.cus = get<int32_t>();
  base.lds_per_cu = get<int64_t>();
  for (int k = 0; k < n; ++k) base.resident_blocks.push_back(get<int32_t>());
  for (int k = 0; k < n; ++k) base.static_lds.push_back(get<int32_t>());
  const int n_cases = get<int32_t>();
  for (int c = 0; c < n_cases; ++c) {
    Planner plan = base;      // memo tables and splits are per case
    plan.max_depth = get<int32_t>();
    plan.out_final_only = get<int32_t>() != 0;
    const int iterate = get<int32_t>();
    const int n_split = get<int32_t>();
    int32_t split[8], vlo[4], vhi[4];
    int64_t dims[4];
    for (int i = 0; i < 8; ++i) split[i] = get<int32_t>();
    for (int d = 0; d < 4; ++d) dims[d] = get<int64_t>();
    for (int d = 0; d < 4; ++d) vlo[d] = get<int32_t>();
    for (int d = 0; d < 4; ++d) vhi[d] = get<int32_t>();
    if (n_split > 0)
      plan.tuned_split[split_key(&plan, dims, iterate)] = std::vector<int>(split, split + n_split);
    std::vector<Launch> list;
    int depth = 0;
    ScratchNeeds needs;
    const int rc = build_schedule(&plan, dims, iterate, vlo, vhi, &list, &depth, &needs);
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
