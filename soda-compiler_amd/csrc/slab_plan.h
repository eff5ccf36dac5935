// The plan of a multi-GPU slab run (slab_plan.cpp): every super-step's messages, sweeps
// and margins and where the rows end up, as data.  Pure arithmetic over the program and
// the slab descriptor - no HIP, no RCCL - so it builds with the host compiler alone and
// full-size runs are checked on the CPU against soda_hip/runtime/dist.py
// (tests/test_slab_plan.py).  slab.cpp executes it.  Internal: not part of the C ABI.
#ifndef SODA_HIP_SLAB_PLAN_H_
#define SODA_HIP_SLAB_PLAN_H_

#include "schedule.h"

// rows [first, first + rows) of the LOCAL arrays, every field's, to or from a peer
struct SlabMessage {
  bool send;
  int peer;
  int64_t first, rows;
};

// one sweep: the sub-array of local rows [r0, r1) with each field's own valid margins
// (0 = the side is cut inside valid rows)
struct SlabPiece {
  int64_t r0, r1;
  bool final_only;    // only its last launch may write the destination (the rows beside
                      // its own are another piece's, and may be on their way to a peer)
  int32_t valid_lo[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS];
  int32_t valid_hi[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS];
};

struct SuperStep {
  int done = 0, step = 0;             // iterations before it, iterations it advances
  std::vector<SlabMessage> before;    // the group enqueued before its first sweep, in
                                      // order (empty: world 1, or nothing to ship)
  std::vector<SlabPiece> pieces;      // in order (none: the rank has no rows left)
  // bands first: the piece after which the NEXT super-step's `before` goes out on the side
  // stream, beside the pieces that follow; -1: that group waits for the super-step's end
  // (serial order, the last super-step, a thin slab, nothing to gain)
  int exchange_after = -1;
};

struct SlabRun {
  int64_t local_extent = 0;     // rows of the rank's arrays a, b, c
  int64_t input_offset = 0;     // where [own_first, own_last) of the input go (array a)
  int64_t result_first = 0, result_last = 0;    // GLOBAL rows of the result it ends with
  int64_t result_offset = 0;    // ... and the local row at which they start
  int64_t row_bytes[SODA_HIP_MAX_IO] = {};      // per field
  std::vector<SuperStep> steps;
};

#pragma GCC visibility push(hidden)

// The run of `iterate` iterations on this rank's slab of a program over `fields` arrays,
// with every check of the descriptor, `iterate`, the order and the cut (the texts of
// soda_hip_run_slab's refusals).  fields == 0: the layout alone - no super-steps, `iterate`
// matters to the re-cut only, the order is not looked at and the planner's tables are
// left as they are.
int plan_slab_run(Planner* plan, const soda_hip_slab* slab, int iterate, int fields,
                  SlabRun* run);

#pragma GCC visibility pop

#endif  // SODA_HIP_SLAB_PLAN_H_
