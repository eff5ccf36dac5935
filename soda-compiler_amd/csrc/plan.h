// What soda_hip.cpp and slab.cpp share of the HIP side of libsoda_hip.so: the module
// and plan behind the C ABI's handles.  Internal: not part of include/soda_hip.h.
#ifndef SODA_HIP_PLAN_H_
#define SODA_HIP_PLAN_H_

#include "schedule.h"

#include <hip/hip_runtime.h>

#define HIP_TRY(code, call)                                                   \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess)                                                     \
      return fail((code), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                        \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

struct soda_hip_module {
  hipModule_t mod = nullptr;
  std::vector<char> image;
  std::string meta;
};

// the planner's state (program, kernels, device facts, knobs) plus the HIP handles
// and the device memory the plan owns
struct soda_hip_plan : Planner {
  soda_hip_module* module = nullptr;
  std::vector<hipFunction_t> funcs;
  // scratch: [0, n_outputs) ping-pong partner of the outputs (array A),
  // then one per non-output stage (only used by per-stage kernels)
  std::vector<void*> scratch;
  std::vector<size_t> scratch_bytes;
  std::vector<void*> scratch_b;      // second partner per output (array B, out_final_only)
  std::vector<size_t> scratch_b_bytes;
  // soda_hip_run_slab, bands-first order: the exchange runs on a stream the plan owns
  hipStream_t side = nullptr;
  hipEvent_t ev_main = nullptr, ev_landed = nullptr;
  // soda_hip_clock_probe_start / _finish
  hipFunction_t probe = nullptr;
  void* probe_buf = nullptr;
  bool probe_running = false;
  hipEvent_t probe_t0 = nullptr, probe_t1 = nullptr;
};

#endif  // SODA_HIP_PLAN_H_
