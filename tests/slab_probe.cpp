// Test probe of the slab plan (soda-compiler_amd/csrc/slab_plan.cpp), built by
// tests/test_slab_plan.py with the host compiler alone: plans the runs of one binary
// request file and prints every super-step.  Request (native endianness, no padding):
//   soda_hip_program; int32 n_cases; then per case - one rank of one run -
//   int32 iterate, fields, wanted; soda_hip_slab
// wanted > 0: the exchange period is soda_hip_slab_exchange's answer for that wish (and
// printed); 0: the descriptor's own; < 0: that entry is handed no place for its answer.
#include "slab_plan.h"

#include <cstdio>
#include <cstdlib>

namespace {

FILE* g_in;

template <typename T>
T get() {
  T v;
  if (fread(&v, sizeof v, 1, g_in) != 1) {
    fprintf(stderr, "slab_probe: request ends early\n");
    exit(2);
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: slab_probe REQUEST\n");
    return 2;
  }
  Planner plan;
  plan.prog = get<soda_hip_program>();
  const int dim = plan.prog.dim;
  const int n_cases = get<int32_t>();
  for (int c = 0; c < n_cases; ++c) {
    const int iterate = get<int32_t>();
    const int fields = get<int32_t>();
    const int wanted = get<int32_t>();
    soda_hip_slab slab = get<soda_hip_slab>();
    SlabRun run;
    int rc = 0;
    if (wanted)
      rc = soda_hip_slab_exchange(slab.dims[dim - 1], slab.world, slab.reach_lo, slab.reach_hi,
                                  wanted, wanted > 0 ? &slab.exchange : nullptr);
    if (!rc) rc = plan_slab_run(&plan, &slab, iterate, fields, &run);
    printf("case %d rc %d\n", c, rc);
    if (rc) {
      printf("error %s\n", g_last_error.c_str());
      continue;
    }
    if (wanted > 0) printf("period %d\n", slab.exchange);
    printf("layout %lld %lld %lld %lld %lld bytes", (long long)run.local_extent,
           (long long)run.input_offset, (long long)run.result_first, (long long)run.result_last,
           (long long)run.result_offset);
    for (int j = 0; j < fields; ++j) printf(" %lld", (long long)run.row_bytes[j]);
    printf("\n");
    for (const SuperStep& st : run.steps) {
      printf("S %d %d %d\n", st.done, st.step, st.exchange_after);
      for (const SlabMessage& m : st.before)
        printf("M %c %d %lld %lld\n", m.send ? 's' : 'r', m.peer, (long long)m.first,
               (long long)m.rows);
      for (const SlabPiece& p : st.pieces) {
        printf("P %lld %lld %d lo", (long long)p.r0, (long long)p.r1, (int)p.final_only);
        for (int j = 0; j < fields; ++j)
          for (int d = 0; d < dim; ++d) printf(" %d", (int)p.valid_lo[j][d]);
        printf(" hi");
        for (int j = 0; j < fields; ++j)
          for (int d = 0; d < dim; ++d) printf(" %d", (int)p.valid_hi[j][d]);
        printf("\n");
      }
    }
  }
  fclose(g_in);
  return 0;
}
