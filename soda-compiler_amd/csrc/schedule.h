// The launch planner of libsoda_hip.so (schedule.cpp): which kernel runs on which box
// with which grid and which buffers.  Pure arithmetic over the program, the kernel
// table and a few device facts - nothing here knows the HIP runtime, so the planner
// builds and is tested without a GPU (tests/test_schedule.py).  Internal: not part of
// the C ABI (include/soda_hip.h).
#ifndef SODA_HIP_SCHEDULE_H_
#define SODA_HIP_SCHEDULE_H_

#include "soda_hip.h"

#include <array>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

struct Box {
  int32_t lo[SODA_HIP_MAX_DIMS];  // <= 0
  int32_t hi[SODA_HIP_MAX_DIMS];  // >= 0
  bool set;
};

// Which buffer a launch means by one of its tensors; the runtime turns it into a
// pointer once the caller's arrays and the plan's own are known.
struct Buffer {
  enum Kind : uint8_t {
    NONE,     // the kernel does not touch this tensor
    INPUT,    // in[index]
    OUTPUT,   // out[index]
    ARRAY_A,  // the plan's ping-pong partner of output `index`
    ARRAY_B,  // the plan's second partner of output `index` (out_final_only)
    LOCAL     // the plan's array of stage `index` (per-stage kernels)
  };
  Kind kind = NONE;
  uint8_t index = 0;
};

struct Launch {
  int kernel;
  soda_hip_args args;       // tensor[] stays NULL here: see `buffer`
  Buffer buffer[SODA_HIP_MAX_TENSORS];   // by tensor index
  unsigned grid[3];
  double est_us;   // modelled duration (0 = the kernel carries no cost figures)
  unsigned lds_bytes = 0;   // dynamic LDS asked for only to cap the workgroups per CU
  long long rounds = 0;     // streaming kernels: chip-fulls of workgroups the price assumes
  long long resident = 0;   // ... and the workgroups one chip-full is (after any cap)
};

// the plan-owned arrays a launch list names
struct ScratchNeeds {
  bool pingpong = false;   // ARRAY_A
  bool second = false;     // ARRAY_B
  bool locals = false;     // LOCAL
};

// Composed boxes per iteration per tensor, grown on demand, from the boxes the inputs
// start on (lo <= 0 <= hi, relative to the margins all inputs share; empty = the zero
// box for every input: a fresh run, or one margin for all).
struct Growth {
  std::vector<Box> start;
  std::vector<std::vector<Box>> boxes;
  std::vector<Box> feed;
};

struct Planner {
  soda_hip_program prog{};
  std::vector<soda_hip_kernel> kernels;
  // device facts
  std::vector<int> resident_blocks;  // per kernel: workgroups the chip holds at once
  std::vector<int> static_lds;       // per kernel: bytes of LDS the code object declares
  int cus = 256;                     // compute units of the device the plan lives on
  int64_t lds_per_cu = 160 * 1024;   // LDS of one CU (gfx950: 160 KiB)
  // knobs
  int max_depth = 0;
  int chunk_rows_override = 0;       // SODA_HIP_CHUNK_ROWS, for tuning
  // shortest chunk the launcher considers: small grids need many short chunks to
  // reach every CU (jacobi3d 128^3, depth 4: 67 us per launch with 32-plane
  // chunks)
  int chunk_rows_min = 8;
  int wgs_per_cu_cap = 0;            // SODA_HIP_WGS_PER_CU, for tuning (see streaming_cap)
  // soda_hip_plan_set_out_final_only: `out` is written by the LAST launch of a sweep
  // only; the launches before it alternate between the plan's arrays A and B
  bool out_final_only = false;
  // while tuning: the modelled price of kernels of this depth is scaled by this
  // factor (how the candidate splits are generated); 0 = no bias
  int bias_depth = 0;
  double bias = 1.0;
  bool tuning = false;               // candidates are being timed: ignore tuned_split
  // memo tables
  // composed boxes of a run from inputs that share their region (Growth)
  Growth fresh;
  // ... and of resumed runs whose inputs differ, keyed by what each input's region lacks
  // beyond the shared margins (per input: lo of every dimension, then hi), so that
  // different starts do not collide
  std::map<std::vector<int32_t>, Growth> resumed;
  // XCD super-tile shape chosen per (kernel, tiles along x, y, chunks): the search
  // walks every super-tile and a sweep's launches mostly repeat a few grids
  mutable std::map<std::array<int64_t, 4>, std::pair<int, int>> xcd_shape;
  // soda_hip_plan_tune: the split of `iterate` (fused depths, deepest first) that ran
  // fastest on this device for arrays of these extents, keyed by dims + iterate (the
  // margins of a resumed or sharded run move the boxes by a few cells, not the
  // ranking); where an entry exists build_schedule uses it instead of its own split
  std::map<std::array<int64_t, 5>, std::vector<int>> tuned_split;
  // soda_hip_plan_tune, streaming launches: the (chunk length, workgroups per CU) that
  // ran fastest on THIS device for a kernel on a box of these extents, keyed by kernel
  // index + box extents; the chunk choice uses it instead of the kernel's calibration
  // record (stream_chunk / stream_wgs_per_cu were measured on one box of one round)
  std::map<std::array<int64_t, 5>, std::array<int, 2>> tuned_stream;
  // soda_hip_plan_tune, depths with several kernels (2-D `k24` / `k24w`, 3-D `k4` / `k4b`):
  // how a sweep of these extents ran fastest, keyed like tuned_split - 0 or no entry: every
  // launch takes the cheaper by price, 1: the table's first kernel of its depth that can
  // run, 2: its last
  std::map<std::array<int64_t, 5>, int> tuned_form;
};

// what follows stays inside libsoda_hip.so: the library exports its C ABI only
#pragma GCC visibility push(hidden)

// the detail text behind soda_hip_last_error(), per thread
extern thread_local std::string g_last_error;
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Experiment knobs (chunk length, XCD super-tile shape, schedule trace) are read
// from the environment ONLY when SODA_HIP_TUNING=1 is set as well: tools/ set it,
// nothing else does, so a stray variable cannot change how a production run is
// scheduled.  None of them can change results, only placement and chunking.
const char* tuning_env(const char* name);

int n_tensors(const soda_hip_program& p);
bool is_output_tensor(const soda_hip_program& p, int t);

// hull over the outputs after `iterations` iterations of a fresh run, as positive margins
void output_margins(Planner* plan, int iterations, int32_t* lo, int32_t* hi);
// the same per output (n_outputs rows)
void field_margins(Planner* plan, int iterations, int32_t (*lo)[SODA_HIP_MAX_DIMS],
                   int32_t (*hi)[SODA_HIP_MAX_DIMS]);

// the key of Planner::tuned_split
std::array<int64_t, 5> split_key(const Planner* plan, const int64_t* dims, int iterate);
// the key of Planner::tuned_stream
std::array<int64_t, 5> stream_key(const Planner* plan, int k, const soda_hip_args& args);

// bytes a launch streams: its box, every input and output
double footprint_of(const Planner* plan, const soda_hip_args& args);
// beyond this a launch's box does not fit the 256 MiB Infinity Cache (the kernels' own
// non-temporal paths switch at the same figure: kernel_common.NT_STREAMING_BYTES)
const double kBeyondCacheBytes = 288.0 * 1024 * 1024;

// Builds the launch list of one sweep and says which plan-owned arrays it names.
int build_schedule(Planner* plan, const int64_t* dims, int iterate, const int32_t* valid_lo,
                   const int32_t* valid_hi, std::vector<Launch>* list, int* max_depth_used,
                   ScratchNeeds* needs);
// The same with a valid region per input: valid_lo / valid_hi hold n_inputs rows of
// margins (NULL = none).  Output j of the sweep is defined on the box the composition
// gives from those regions; no output is defined outside the margins all inputs share.
int build_schedule_fields(Planner* plan, const int64_t* dims, int iterate,
                          const int32_t (*valid_lo)[SODA_HIP_MAX_DIMS],
                          const int32_t (*valid_hi)[SODA_HIP_MAX_DIMS],
                          std::vector<Launch>* list, int* max_depth_used, ScratchNeeds* needs);

#pragma GCC visibility pop

#endif  // SODA_HIP_SCHEDULE_H_
