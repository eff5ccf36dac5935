// libsoda_hip.so -- the multi-GPU slab driver (soda_hip_run_slab, soda_hip_run_slab_fields
// and the entry points that describe a slab): it executes the plan of slab_plan.cpp, ghost
// exchanges over RCCL around soda_hip_sweep_fields.
#include "plan.h"
#include "slab_plan.h"

#include <dlfcn.h>

#include <cstdlib>
#include <string>
#include <vector>

namespace {

// RCCL is resolved at first use: a single-GPU caller never loads it.
struct Rccl {
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  int (*send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*error_string)(int) = nullptr;
  int (*comm_abort)(void*) = nullptr;
  bool ok = false;
};

const Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return x;
    x.group_start = (int (*)())dlsym(h, "ncclGroupStart");
    x.group_end = (int (*)())dlsym(h, "ncclGroupEnd");
    x.send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclSend");
    x.recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclRecv");
    x.error_string = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    x.comm_abort = (int (*)(void*))dlsym(h, "ncclCommAbort");
    x.ok = x.group_start && x.group_end && x.send && x.recv;
    return x;
  }();
  return r;
}

// The stream and the two events of the bands-first order, each under its own check (the
// clock probe creates the same stream; a half-built set must be completed, not skipped).
int side_stream(soda_hip_plan* plan) {
  if (!plan->side && hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking) != hipSuccess) {
    plan->side = nullptr;
    return fail(SODA_HIP_ERR_DEVICE_RUN, "side stream for the exchange: %s",
                hipGetErrorString(hipGetLastError()));
  }
  for (hipEvent_t* ev : {&plan->ev_main, &plan->ev_landed})
    if (!*ev && hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) {
      *ev = nullptr;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "event for the exchange stream: %s",
                  hipGetErrorString(hipGetLastError()));
    }
  return 0;
}

// what the two entry points check of the communicator before anything else
int communicator(const soda_hip_slab* slab, void* comm) {
  if (slab->world > 1 && !comm)
    return fail(SODA_HIP_ERR_NULL_ARGUMENT, "world %d needs an RCCL communicator", slab->world);
  if (slab->world > 1 && !rccl().ok)
    return fail(SODA_HIP_ERR_NO_DEVICE, "librccl.so could not be loaded: %s", dlerror());
  return 0;
}

// the caller's side of one run: what the plan's rows and groups are applied to
struct Executor {
  soda_hip_plan* plan;
  const soda_hip_slab* slab;
  const SlabRun* run;
  void* comm;
  int fields;
  void* stream;
  bool overlapped;              // the groups go out on the plan's side stream
  bool rccl_failed = false;     // the error came from RCCL itself (e.g. an aborted communicator)
  bool landed_pending = false;  // an exchange on the side stream main has not waited for
  int count = 0;
};

// ONE group carries every field's rows: the rows of one field are contiguous, so nothing
// is packed - field by field, the plan's messages in order (both sides of a pair enumerate
// the fields in the same order).  On the side stream the group follows everything enqueued
// on the main stream so far (the rows to be sent were produced there).
int exchange(Executor* x, void* const* arrays, const std::vector<SlabMessage>& messages) {
  x->count += x->slab->world > 1;
  hipStream_t on = as_stream(x->stream);
  if (x->overlapped) {
    on = x->plan->side;
    if (hipEventRecord(x->plan->ev_main, as_stream(x->stream)) != hipSuccess ||
        hipStreamWaitEvent(on, x->plan->ev_main, 0) != hipSuccess)
      return fail(SODA_HIP_ERR_DEVICE_RUN, "ordering the exchange stream failed");
  }
  if (!messages.empty()) {
    const Rccl& r = rccl();
    int e = r.group_start();
    for (int j = 0; j < x->fields; ++j)
      for (const SlabMessage& m : messages) {
        if (e) break;
        char* at = (char*)arrays[j] + m.first * x->run->row_bytes[j];
        const size_t bytes = (size_t)(m.rows * x->run->row_bytes[j]);
        e = m.send ? r.send(at, bytes, 0, m.peer, x->comm, on)
                   : r.recv(at, bytes, 0, m.peer, x->comm, on);
      }
    const int e2 = r.group_end();
    if (e || e2) {
      x->rccl_failed = true;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "RCCL ghost exchange failed: %s",
                  r.error_string ? r.error_string(e ? e : e2) : "?");
    }
  }
  if (x->overlapped) {
    if (hipEventRecord(x->plan->ev_landed, on) != hipSuccess)
      return fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventRecord failed");
    x->landed_pending = true;
  }
  return 0;
}

int ghosts_have_landed(Executor* x) {      // before a sweep reads ghost rows
  if (!x->landed_pending) return 0;
  x->landed_pending = false;
  if (hipStreamWaitEvent(as_stream(x->stream), x->plan->ev_landed, 0) != hipSuccess)
    return fail(SODA_HIP_ERR_DEVICE_RUN, "hipStreamWaitEvent failed");
  return 0;
}

// Every super-step of the plan in turn: its group, unless the super-step before sent it
// beside its interior; its pieces, a -> b -> c -> b ...; after piece `exchange_after` the
// next super-step's group.  A piece's intermediate launches must not write rows of the
// destination another piece has finished (they are being sent): out_final_only.
int super_steps(Executor* x, void* const* a, void* const* b, void* const* c, void** result) {
  soda_hip_plan* plan = x->plan;
  const SlabRun& run = *x->run;
  const int last = plan->prog.dim - 1;
  // test hook (SODA_HIP_TUNING=1 only): rank R fails at its K-th super-step
  int fail_rank = -1, fail_at = -1;
  if (const char* env = tuning_env("SODA_HIP_FAIL_RANK")) fail_rank = atoi(env);
  if (const char* env = tuning_env("SODA_HIP_FAIL_SUPERSTEP")) fail_at = atoi(env);
  int64_t dims[SODA_HIP_MAX_DIMS] = {1, 1, 1, 1};
  for (int d = 0; d < last; ++d) dims[d] = x->slab->dims[d];
  const bool was_final_only = plan->out_final_only;
  void* const* src = a;
  bool sent = false;            // src's ghost rows are (being) filled already
  int rc = 0;
  for (size_t k = 0; k < run.steps.size() && !rc; ++k) {
    const SuperStep& st = run.steps[k];
    void* const* dst = k % 2 ? c : b;
    if (!sent) rc = exchange(x, src, st.before);
    if (!rc) rc = ghosts_have_landed(x);
    if (rc) break;
    sent = false;
    if (x->slab->rank == fail_rank && (int)k == fail_at)
      return fail(SODA_HIP_ERR_DEVICE_RUN, "injected failure of rank %d at super-step %d",
                  fail_rank, fail_at);
    for (size_t i = 0; i < st.pieces.size() && !rc; ++i) {
      const SlabPiece& piece = st.pieces[i];
      void *from[SODA_HIP_MAX_IO], *to[SODA_HIP_MAX_IO];
      for (int j = 0; j < x->fields; ++j) {
        from[j] = (char*)src[j] + piece.r0 * run.row_bytes[j];
        to[j] = (char*)dst[j] + piece.r0 * run.row_bytes[j];
      }
      dims[last] = piece.r1 - piece.r0;
      plan->out_final_only = piece.final_only ? true : was_final_only;
      rc = soda_hip_sweep_fields(plan, from, to, dims, st.step, piece.valid_lo, piece.valid_hi,
                                 x->stream);
      plan->out_final_only = was_final_only;
      if (!rc && (int)i == st.exchange_after) {     // beside the pieces that follow
        rc = exchange(x, dst, run.steps[k + 1].before);
        sent = true;
      }
    }
    src = dst;
  }
  if (!rc) rc = ghosts_have_landed(x);
  if (rc) return rc;
  for (int j = 0; j < x->fields; ++j) result[j] = src[j];
  return 0;
}

// Runs a plan.  Everything that can be wrong with the call itself was found before: from
// here on a failure of THIS rank may leave peers waiting in ncclRecv for rows it will
// never send.  abort_on_error: after a failure of this rank's OWN (a launch, an allocation
// - not an error RCCL reports, which may be somebody's abort of this very communicator)
// the communicator is aborted before the error is returned (best effort - ncclCommAbort is
// local to the rank, include/soda_hip.h); otherwise the communicator is the caller's to
// abort, for every rank of its process.
int execute(soda_hip_plan* plan, const soda_hip_slab* slab, void* comm, const SlabRun& run,
            int fields, void* const* a, void* const* b, void* const* c, void* stream,
            void** result, int* exchanges) {
  Executor x{plan, slab, &run, comm, fields, stream,
             slab->order == SODA_HIP_SLAB_BANDS_FIRST && slab->world > 1};
  if (x.overlapped)
    if (int rc = side_stream(plan)) return rc;
  const int rc = super_steps(&x, a, b, c, result);
  if (rc && !x.rccl_failed && slab->abort_on_error && slab->world > 1 && comm &&
      rccl().comm_abort) {
    const std::string keep = g_last_error;
    (void)rccl().comm_abort(comm);
    g_last_error = keep + " (communicator aborted)";
  }
  if (!rc && exchanges) *exchanges = x.count;
  return rc;
}

}  // namespace

extern "C" {

int soda_hip_slab_extent(const soda_hip_plan* plan, const soda_hip_slab* slab,
                         int64_t local_dims[SODA_HIP_MAX_DIMS], int64_t* ghost_lo,
                         int64_t* ghost_hi) {
  if (!plan || !slab || !local_dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC)
    return fail(SODA_HIP_ERR_CONSTRAINT, "soda_hip_slab_extent describes the static cut; a "
                "re-cut run's arrays depend on the iteration count: soda_hip_slab_layout");
  int64_t input_offset;
  int rc = soda_hip_slab_layout(plan, slab, 1, local_dims, &input_offset, nullptr, nullptr,
                                nullptr);
  if (rc) return rc;
  if (ghost_lo) *ghost_lo = input_offset;
  if (ghost_hi)
    *ghost_hi = local_dims[plan->prog.dim - 1] - input_offset - (slab->own_last - slab->own_first);
  return 0;
}

int soda_hip_slab_layout(const soda_hip_plan* plan, const soda_hip_slab* slab, int iterate,
                         int64_t local_dims[SODA_HIP_MAX_DIMS], int64_t* input_offset,
                         int64_t* result_first, int64_t* result_last,
                         int64_t* result_offset) {
  if (!plan || !slab || !local_dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  SlabRun run;
  // (the layout alone reads the program and leaves the planner's tables as they are)
  int rc = plan_slab_run(const_cast<soda_hip_plan*>(plan), slab, iterate, 0, &run);
  if (rc) return rc;
  for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d)
    local_dims[d] = d < plan->prog.dim ? slab->dims[d] : 1;
  local_dims[plan->prog.dim - 1] = run.local_extent;
  if (input_offset) *input_offset = run.input_offset;
  if (result_first) *result_first = run.result_first;
  if (result_last) *result_last = run.result_last;
  if (result_offset) *result_offset = run.result_offset;
  return 0;
}

int soda_hip_run_slab(soda_hip_plan* plan, const soda_hip_slab* slab, void* comm,
                      void* a, void* b, void* c, int iterate, void* stream,
                      void** result, int* exchanges) {
  if (!plan || !slab || !a || !b || !c || !result)
    return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (plan->prog.n_inputs != 1 || plan->prog.n_outputs != 1)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: one-input one-output programs (programs "
                "over several fields: soda_hip_run_slab_fields)");
  int rc = communicator(slab, comm);
  if (rc) return rc;
  // Everything that can be wrong with the call itself is found before the first message
  // is enqueued: such an error leaves the communicator alone (the peers have not been
  // promised anything yet - the caller's own rendezvous, or its next call, sees it).
  SlabRun run;
  rc = plan_slab_run(plan, slab, iterate, 1, &run);
  if (rc) return rc;
  return execute(plan, slab, comm, run, 1, &a, &b, &c, stream, result, exchanges);
}

int soda_hip_run_slab_fields(soda_hip_plan* plan, const soda_hip_slab* slab, void* comm,
                             void* const* a, void* const* b, void* const* c, int iterate,
                             void* stream, void** result, int* exchanges) {
  if (!plan || !slab || !a || !b || !c || !result)
    return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  const soda_hip_program& p = plan->prog;
  const int n = p.n_inputs;
  for (int j = 0; j < n; ++j)
    if (!a[j] || !b[j] || !c[j])
      return fail(SODA_HIP_ERR_NULL_ARGUMENT, "an array of field %d is NULL", j);
  int rc = communicator(slab, comm);
  if (rc) return rc;
  // as soda_hip_run_slab: whatever is wrong with the call itself is found before the
  // first message is enqueued and leaves the communicator alone
  if (iterate < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "iterate must be >= 1");
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: static cut only for programs over several "
                "fields");
  if (slab->order != SODA_HIP_SLAB_SERIAL)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: serial order only for programs over several "
                "fields");
  SlabRun run;
  rc = plan_slab_run(plan, slab, iterate, n, &run);
  if (rc) return rc;
  for (int j = 0; j < n; ++j)     // field j's three arrays hold input j and output j in turn
    if (p.elem_size[j] != p.elem_size[p.output_tensor[j]])
      return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: output %d (%d bytes per cell) cannot feed "
                  "input %d (%d)", j, p.elem_size[p.output_tensor[j]], j, p.elem_size[j]);
  // the ghost rows must cover what ANY field reads in `exchange` iterations: the composed
  // margin of a field after k iterations is at most k x the hull of one iteration's
  int32_t lo[SODA_HIP_MAX_DIMS], hi[SODA_HIP_MAX_DIMS];
  output_margins(plan, 1, lo, hi);
  if (slab->world > 1 && (slab->reach_lo < lo[p.dim - 1] || slab->reach_hi < hi[p.dim - 1]))
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab reach %d / %d is below the program's %d / %d "
                "(soda_hip_plan_margins(plan, 1))", slab->reach_lo, slab->reach_hi,
                (int)lo[p.dim - 1], (int)hi[p.dim - 1]);
  return execute(plan, slab, comm, run, n, a, b, c, stream, result, exchanges);
}

}  // extern "C"
