// libsoda_hip.so -- the multi-GPU slab driver (soda_hip_run_slab and the entry points
// that describe a slab): ghost exchanges over RCCL around soda_hip_sweep.
#include "plan.h"

#include <dlfcn.h>

#include <algorithm>
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

struct SlabGeometry {
  int64_t own, ghost_lo, ghost_hi, extent, row_bytes;
  bool has_lo, has_hi;
};

int slab_geometry(const soda_hip_plan* plan, const soda_hip_slab* s, SlabGeometry* g) {
  const soda_hip_program& p = plan->prog;
  // the geometry is the same for every field of a program over several (output j feeds
  // input j); which driver runs it is the drivers' check
  if (p.n_inputs != p.n_outputs)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: programs with as many outputs as inputs");
  if (s->world < 1 || s->rank < 0 || s->rank >= s->world || s->exchange < 1 ||
      s->reach_lo < 0 || s->reach_hi < 0)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab descriptor out of range");
  g->own = s->own_last - s->own_first;
  g->has_lo = s->rank > 0;
  g->has_hi = s->rank < s->world - 1;
  g->ghost_lo = g->has_lo ? (int64_t)s->exchange * s->reach_lo : 0;
  g->ghost_hi = g->has_hi ? (int64_t)s->exchange * s->reach_hi : 0;
  // a ghost region deeper than a neighbour's own rows would ship rows it does
  // not own (runtime/dist.py: SlabPlan raises for the same reason)
  if (g->own < 1 || (s->world > 1 && g->own < (int64_t)s->exchange *
                                                 std::max(s->reach_lo, s->reach_hi)))
    return fail(SODA_HIP_ERR_CONSTRAINT,
                "slab of %lld own rows is thinner than its ghost regions (%d x %d)",
                (long long)g->own, s->exchange, std::max(s->reach_lo, s->reach_hi));
  g->extent = g->ghost_lo + g->own + g->ghost_hi;
  g->row_bytes = p.elem_size[0];
  for (int d = 0; d < p.dim - 1; ++d) g->row_bytes *= s->dims[d];
  return 0;
}

// ---- slabs re-cut to the shrinking valid box (runtime/dist.py: RecutPlan) ----
struct Rows {
  int64_t lo = 0, hi = 0;
  bool empty() const { return hi <= lo; }
};

Rows intersect(const Rows& a, const Rows& b) {
  Rows r;
  r.lo = std::max(a.lo, b.lo);
  r.hi = std::min(a.hi, b.hi);
  return r;
}

// world + 1 cut points of [lo, hi): as even as possible, the longer shares first
std::vector<int64_t> even_cut(int64_t lo, int64_t hi, int world) {
  const int64_t extent = std::max<int64_t>(0, hi - lo);
  const int64_t base = extent / world, extra = extent % world;
  std::vector<int64_t> pts(world + 1, lo);
  for (int r = 0; r < world; ++r) pts[r + 1] = pts[r] + base + (r < extra ? 1 : 0);
  return pts;
}

struct RecutStep {
  int done = 0, step = 0;
  std::vector<Rows> owned;      // per rank: rows of the INPUT level it holds
  std::vector<int64_t> cuts;    // world + 1 cut points of the OUTPUT level's rows
  std::vector<Rows> need;       // per rank: rows of the input level it reads (empty: none)
};

struct RecutTable {
  std::vector<RecutStep> steps;
  std::vector<Rows> final;      // per rank: rows of the result
  int64_t base = 0, extent = 0; // this rank's arrays span global rows [base, base + extent)
  int64_t row_bytes = 0;
};

int recut_table(const soda_hip_plan* plan, const soda_hip_slab* s, int iterate, RecutTable* t) {
  const soda_hip_program& p = plan->prog;
  if (p.n_inputs != 1 || p.n_outputs != 1)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: static cut only for programs over several "
                "fields");
  if (s->world < 1 || s->rank < 0 || s->rank >= s->world || s->exchange < 1 ||
      s->reach_lo < 0 || s->reach_hi < 0 || iterate < 1)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab descriptor out of range");
  const int64_t rows = s->dims[p.dim - 1];
  if (rows < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "slab descriptor: %lld rows", (long long)rows);
  const std::vector<int64_t> level0 = even_cut(0, rows, s->world);
  if (s->own_first != level0[s->rank] || s->own_last != level0[s->rank + 1])
    return fail(SODA_HIP_ERR_CONSTRAINT,
                "re-cut slabs: rank %d of %d must be handed rows [%lld, %lld) of %lld (the even "
                "cut), not [%lld, %lld)", s->rank, s->world, (long long)level0[s->rank],
                (long long)level0[s->rank + 1], (long long)rows, (long long)s->own_first,
                (long long)s->own_last);
  std::vector<Rows> level(s->world);
  for (int r = 0; r < s->world; ++r) { level[r].lo = level0[r]; level[r].hi = level0[r + 1]; }
  t->steps.clear();
  int64_t lo_hull = s->own_first, hi_hull = s->own_last;
  for (int done = 0; done < iterate;) {
    RecutStep st;
    st.done = done;
    st.step = std::min(s->exchange, iterate - done);
    const int64_t lo = (int64_t)(done + st.step) * s->reach_lo;
    const int64_t hi = rows - (int64_t)(done + st.step) * s->reach_hi;
    st.cuts = even_cut(lo, std::max(lo, hi), s->world);
    st.owned = level;
    st.need.assign(s->world, Rows{});
    for (int r = 0; r < s->world; ++r) {
      if (st.cuts[r + 1] <= st.cuts[r]) continue;
      st.need[r].lo = st.cuts[r] - (int64_t)st.step * s->reach_lo;
      st.need[r].hi = st.cuts[r + 1] + (int64_t)st.step * s->reach_hi;
    }
    if (!st.need[s->rank].empty()) {
      lo_hull = std::min(lo_hull, st.need[s->rank].lo);
      hi_hull = std::max(hi_hull, st.need[s->rank].hi);
    }
    for (int r = 0; r < s->world; ++r) { level[r].lo = st.cuts[r]; level[r].hi = st.cuts[r + 1]; }
    done += st.step;
    t->steps.push_back(st);
  }
  t->final = level;
  t->base = lo_hull;
  t->extent = hi_hull - lo_hull;
  t->row_bytes = p.elem_size[0];
  for (int d = 0; d < p.dim - 1; ++d) t->row_bytes *= s->dims[d];
  return 0;
}

// Super-step i, bands first (RecutPlan.pieces): the rows other ranks read in super-step
// i + 1 come first, the interior afterwards.  false: nothing to gain (the last super-step,
// no output rows, nobody waiting, or bands that meet).
bool recut_pieces(const RecutTable& t, const soda_hip_slab* s, size_t i, std::vector<Rows>* bands,
                  Rows* interior) {
  if (i + 1 >= t.steps.size()) return false;
  const RecutStep& st = t.steps[i];
  const RecutStep& next = t.steps[i + 1];
  const int64_t lo = st.cuts[s->rank], hi = st.cuts[s->rank + 1];
  if (hi <= lo) return false;
  int64_t b_lo = lo, b_hi = hi;
  for (int q = 0; q < s->rank; ++q)
    if (!next.need[q].empty() && next.need[q].hi > lo) b_lo = std::max(b_lo, next.need[q].hi);
  for (int q = s->rank + 1; q < s->world; ++q)
    if (!next.need[q].empty() && next.need[q].lo < hi) b_hi = std::min(b_hi, next.need[q].lo);
  b_lo = std::min(b_lo, hi);
  b_hi = std::max(b_hi, lo);
  if ((b_lo == lo && b_hi == hi) || b_lo >= b_hi) return false;
  bands->clear();
  if (b_lo > lo) bands->push_back(Rows{lo, b_lo});
  if (b_hi < hi) bands->push_back(Rows{b_hi, hi});
  interior->lo = b_lo;
  interior->hi = b_hi;
  return true;
}

}  // namespace

extern "C" {

int soda_hip_slab_exchange(int64_t rows, int world, int reach_lo, int reach_hi,
                           int wanted, int* exchange) {
  if (!exchange) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (rows < 1 || world < 1 || wanted < 1 || reach_lo < 0 || reach_hi < 0)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab figures out of range");
  const int64_t reach = std::max(1, std::max(reach_lo, reach_hi));
  const int64_t smallest = rows / world;
  if (world > 1 && smallest < reach)
    return fail(SODA_HIP_ERR_CONSTRAINT,
                "cannot cut %lld rows into %d slabs: the smallest slab (%lld rows) is "
                "thinner than the stencil reach (%lld)", (long long)rows, world,
                (long long)smallest, (long long)reach);
  *exchange = world > 1 ? (int)std::max<int64_t>(1, std::min<int64_t>(wanted, smallest / reach))
                        : wanted;
  return 0;
}

int soda_hip_slab_extent(const soda_hip_plan* plan, const soda_hip_slab* slab,
                         int64_t local_dims[SODA_HIP_MAX_DIMS], int64_t* ghost_lo,
                         int64_t* ghost_hi) {
  if (!plan || !slab || !local_dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC)
    return fail(SODA_HIP_ERR_CONSTRAINT, "soda_hip_slab_extent describes the static cut; a "
                "re-cut run's arrays depend on the iteration count: soda_hip_slab_layout");
  SlabGeometry g;
  int rc = slab_geometry(plan, slab, &g);
  if (rc) return rc;
  for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d)
    local_dims[d] = d < plan->prog.dim ? slab->dims[d] : 1;
  local_dims[plan->prog.dim - 1] = g.extent;
  if (ghost_lo) *ghost_lo = g.ghost_lo;
  if (ghost_hi) *ghost_hi = g.ghost_hi;
  return 0;
}

int soda_hip_slab_layout(const soda_hip_plan* plan, const soda_hip_slab* slab, int iterate,
                         int64_t local_dims[SODA_HIP_MAX_DIMS], int64_t* input_offset,
                         int64_t* result_first, int64_t* result_last,
                         int64_t* result_offset) {
  if (!plan || !slab || !local_dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC && slab->cut != SODA_HIP_SLAB_CUT_RECUT)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab cut %d", (int)slab->cut);
  for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d)
    local_dims[d] = d < plan->prog.dim ? slab->dims[d] : 1;
  if (slab->cut == SODA_HIP_SLAB_CUT_STATIC) {
    SlabGeometry g;
    int rc = slab_geometry(plan, slab, &g);
    if (rc) return rc;
    local_dims[plan->prog.dim - 1] = g.extent;
    if (input_offset) *input_offset = g.ghost_lo;
    if (result_first) *result_first = slab->own_first;
    if (result_last) *result_last = slab->own_last;
    if (result_offset) *result_offset = g.ghost_lo;
    return 0;
  }
  RecutTable t;
  int rc = recut_table(plan, slab, iterate, &t);
  if (rc) return rc;
  local_dims[plan->prog.dim - 1] = t.extent;
  if (input_offset) *input_offset = slab->own_first - t.base;
  if (result_first) *result_first = t.final[slab->rank].lo;
  if (result_last) *result_last = t.final[slab->rank].hi;
  if (result_offset) *result_offset = t.final[slab->rank].lo - t.base;
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
  if (slab->world > 1 && !comm)
    return fail(SODA_HIP_ERR_NULL_ARGUMENT, "world %d needs an RCCL communicator", slab->world);
  if (slab->world > 1 && !rccl().ok)
    return fail(SODA_HIP_ERR_NO_DEVICE, "librccl.so could not be loaded: %s", dlerror());
  // Everything that can be wrong with the call itself is found before the first message
  // is enqueued: such an error leaves the communicator alone (the peers have not been
  // promised anything yet - the caller's own rendezvous, or its next call, sees it).
  if (iterate < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "iterate must be >= 1");
  if (slab->order != SODA_HIP_SLAB_SERIAL && slab->order != SODA_HIP_SLAB_BANDS_FIRST)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab order %d", (int)slab->order);
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC && slab->cut != SODA_HIP_SLAB_CUT_RECUT)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab cut %d", (int)slab->cut);
  SlabGeometry g{};
  RecutTable table;
  const bool recut = slab->cut == SODA_HIP_SLAB_CUT_RECUT;
  int rc = recut ? recut_table(plan, slab, iterate, &table) : slab_geometry(plan, slab, &g);
  if (rc) return rc;
  const bool overlapped = slab->order == SODA_HIP_SLAB_BANDS_FIRST && slab->world > 1;
  if (overlapped) {
    // the stream and the two events of the bands-first order, each under its own check (the
    // clock probe creates the same stream; a half-built set must be completed, not skipped)
    if (!plan->side && hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking) != hipSuccess) {
      plan->side = nullptr;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "side stream for the exchange: %s",
                  hipGetErrorString(hipGetLastError()));
    }
    if (!plan->ev_main &&
        hipEventCreateWithFlags(&plan->ev_main, hipEventDisableTiming) != hipSuccess) {
      plan->ev_main = nullptr;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "event for the exchange stream: %s",
                  hipGetErrorString(hipGetLastError()));
    }
    if (!plan->ev_landed &&
        hipEventCreateWithFlags(&plan->ev_landed, hipEventDisableTiming) != hipSuccess) {
      plan->ev_landed = nullptr;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "event for the exchange stream: %s",
                  hipGetErrorString(hipGetLastError()));
    }
  }
  // From here on a failure of THIS rank may leave peers waiting in ncclRecv for rows it
  // will never send.  abort_on_error: after a failure of this rank's OWN (a launch, an
  // allocation - not an error RCCL reports, which may be somebody's abort of this very
  // communicator) the communicator is aborted before the error is returned (best effort -
  // ncclCommAbort is local to the rank, include/soda_hip.h); otherwise the communicator
  // is the caller's to abort, for every rank of its process.
  bool rccl_failed = false;     // the error came from RCCL itself (e.g. an aborted communicator)
  auto give_up = [&](int rc) {
    if (rc && !rccl_failed && slab->abort_on_error && slab->world > 1 && comm &&
        rccl().comm_abort) {
      const std::string keep = g_last_error;
      (void)rccl().comm_abort(comm);
      g_last_error = keep + " (communicator aborted)";
    }
    return rc;
  };
  const soda_hip_program& p = plan->prog;
  const int last = p.dim - 1;
  hipStream_t s = as_stream(stream);
  int64_t local_dims[SODA_HIP_MAX_DIMS] = {1, 1, 1, 1};
  for (int d = 0; d < p.dim; ++d) local_dims[d] = slab->dims[d];
  local_dims[last] = recut ? table.extent : g.extent;
  const int64_t row_bytes = recut ? table.row_bytes : g.row_bytes;
  const int64_t send_down = !recut && g.has_lo ? (int64_t)slab->exchange * slab->reach_hi : 0;
  const int64_t send_up = !recut && g.has_hi ? (int64_t)slab->exchange * slab->reach_lo : 0;
  // one message = rows [first, first + rows) of the LOCAL array, to or from a peer
  struct Message { bool send; int peer; int64_t first, rows; };
  auto static_messages = [&]() {
    std::vector<Message> m;
    const int64_t first_own = g.ghost_lo, last_own = g.ghost_lo + g.own;
    // lower neighbour: it needs our first rows, we need its last ones
    if (g.has_lo && send_down) m.push_back({true, slab->rank - 1, first_own, send_down});
    if (g.has_lo && g.ghost_lo) m.push_back({false, slab->rank - 1, 0, g.ghost_lo});
    if (g.has_hi && send_up) m.push_back({true, slab->rank + 1, last_own - send_up, send_up});
    if (g.has_hi && g.ghost_hi) m.push_back({false, slab->rank + 1, last_own, g.ghost_hi});
    return m;
  };
  // before super-step i of a re-cut run: to every rank the rows it reads and we hold, from
  // every rank the rows we read and it holds - ghost rows and rows changing owner alike
  // (both sides derive a pair's rows from the same table; ascending peers, sends first)
  auto recut_messages = [&](size_t i) {
    std::vector<Message> m;
    const RecutStep& st = table.steps[i];
    const Rows& mine = st.owned[slab->rank];
    for (int pass = 0; pass < 2; ++pass)
      for (int q = 0; q < slab->world; ++q) {
        if (q == slab->rank) continue;
        const Rows rows = pass == 0 ? intersect(st.need[q], mine)
                                    : intersect(st.need[slab->rank], st.owned[q]);
        const bool wanted = pass == 0 ? !st.need[q].empty() && !mine.empty()
                                      : !st.need[slab->rank].empty() && !st.owned[q].empty();
        if (wanted && !rows.empty())
          m.push_back({pass == 0, q, rows.lo - table.base, rows.hi - rows.lo});
      }
    return m;
  };
  auto exchange_rows = [&](char* array, const std::vector<Message>& messages,
                           hipStream_t on) -> int {
    if (slab->world == 1 || messages.empty()) return 0;
    const Rccl& r = rccl();
    int e = r.group_start();
    for (const Message& m : messages) {
      if (e) break;
      char* at = array + m.first * row_bytes;
      e = m.send ? r.send(at, (size_t)(m.rows * row_bytes), 0, m.peer, comm, on)
                 : r.recv(at, (size_t)(m.rows * row_bytes), 0, m.peer, comm, on);
    }
    const int e2 = r.group_end();
    if (e || e2) {
      rccl_failed = true;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "RCCL ghost exchange failed: %s",
                  r.error_string ? r.error_string(e ? e : e2) : "?");
    }
    return 0;
  };
  // Bands-first order (runtime/dist.py: StreamSchedule; band_plan / RecutPlan.pieces):
  // every super-step but the last first sweeps the bands of rows other ranks are waiting
  // for, hands them to the exchange of the NEXT super-step on a stream the plan owns, and
  // sweeps the interior meanwhile.  A piece's intermediate launches must not write rows of
  // `dst` another piece has finished (they are being sent): pieces run with out_final_only.
  bool landed_pending = false;      // an exchange on the side stream main has not waited for
  auto exchange = [&](char* array, const std::vector<Message>& messages) -> int {
    if (!overlapped) return exchange_rows(array, messages, s);
    // the rows to be sent were produced on the main stream: the side stream follows
    // everything enqueued there so far
    if (hipEventRecord(plan->ev_main, s) != hipSuccess ||
        hipStreamWaitEvent(plan->side, plan->ev_main, 0) != hipSuccess)
      return fail(SODA_HIP_ERR_DEVICE_RUN, "ordering the exchange stream failed");
    int e = exchange_rows(array, messages, plan->side);
    if (e) return e;
    if (hipEventRecord(plan->ev_landed, plan->side) != hipSuccess)
      return fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventRecord failed");
    landed_pending = true;
    return 0;
  };
  auto ghosts_have_landed = [&]() -> int {      // before a sweep reads ghost rows
    if (!landed_pending) return 0;
    landed_pending = false;
    if (hipStreamWaitEvent(s, plan->ev_landed, 0) != hipSuccess)
      return fail(SODA_HIP_ERR_DEVICE_RUN, "hipStreamWaitEvent failed");
    return 0;
  };
  const bool was_final_only = plan->out_final_only;
  // test hook (SODA_HIP_TUNING=1 only): rank R fails at its K-th super-step
  int fail_rank = -1, fail_at = -1;
  if (const char* env = tuning_env("SODA_HIP_FAIL_RANK")) fail_rank = atoi(env);
  if (const char* env = tuning_env("SODA_HIP_FAIL_SUPERSTEP")) fail_at = atoi(env);
  void* src = a;
  void* cycle[2] = {b, c};
  int done = 0, k = 0, count = 0;
  bool pending = false;            // src's ghost rows are (being) filled already
  // the sub-array of local rows [r0, r1) swept `step` iterations with the given outer
  // margins (0 = the side is cut inside valid rows)
  auto sweep_rows = [&](void* from, void* to, int64_t r0, int64_t r1, int step,
                        const int32_t* lo, const int32_t* hi, bool final_only) -> int {
    int64_t dims_piece[SODA_HIP_MAX_DIMS];
    for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) dims_piece[d] = local_dims[d];
    dims_piece[last] = r1 - r0;
    void* sp = (char*)from + r0 * row_bytes;
    void* dp = (char*)to + r0 * row_bytes;
    plan->out_final_only = final_only ? true : was_final_only;
    const int e = soda_hip_sweep(plan, &sp, &dp, dims_piece, step, lo, hi, stream);
    plan->out_final_only = was_final_only;
    return e;
  };
  while (done < iterate && !rc) {
    if (!pending) {
      rc = exchange((char*)src, recut ? recut_messages((size_t)k) : static_messages());
      count += slab->world > 1;
    }
    if (!rc) rc = ghosts_have_landed();
    if (rc) break;
    pending = false;
    const int step = std::min(slab->exchange, iterate - done);
    // valid region of the slab's input: sides cut inside valid rows are fully valid, the
    // global sides of a static slab carry the margin of the iterations done so far (a
    // re-cut rank's sub-array starts and ends at rows that are valid: every side is cut)
    int32_t lo[SODA_HIP_MAX_DIMS], hi[SODA_HIP_MAX_DIMS];
    output_margins(plan, done, lo, hi);
    if (recut || g.has_lo) lo[last] = 0;
    if (recut || g.has_hi) hi[last] = 0;
    void* dst = cycle[k % 2];
    if (slab->rank == fail_rank && k == fail_at) {
      rc = fail(SODA_HIP_ERR_DEVICE_RUN, "injected failure of rank %d at super-step %d",
                fail_rank, fail_at);
      break;
    }
    const bool more = done + step < iterate;
    if (recut) {
      const RecutStep& st = table.steps[(size_t)k];
      const int64_t reach_lo = (int64_t)step * slab->reach_lo,
                    reach_hi = (int64_t)step * slab->reach_hi;
      auto piece = [&](const Rows& out, bool final_only) -> int {
        return sweep_rows(src, dst, out.lo - reach_lo - table.base, out.hi + reach_hi - table.base,
                          step, lo, hi, final_only);
      };
      std::vector<Rows> bands;
      Rows interior;
      const Rows out{st.cuts[slab->rank], st.cuts[slab->rank + 1]};
      if (overlapped && recut_pieces(table, slab, (size_t)k, &bands, &interior)) {
        for (const Rows& band : bands)
          if (!rc) rc = piece(band, true);
        if (!rc) {
          rc = exchange((char*)dst, recut_messages((size_t)k + 1));   // beside the interior
          count += 1;
          pending = true;
        }
        if (!rc) rc = piece(interior, true);
      } else if (!out.empty()) {
        rc = piece(out, false);
      }
    } else if (overlapped && more && !(g.own < 2 * (send_down + send_up) + 1)) {
      const int64_t first_own = g.ghost_lo, last_own = g.ghost_lo + g.own;
      const int64_t reach_lo = (int64_t)step * slab->reach_lo,
                    reach_hi = (int64_t)step * slab->reach_hi;
      auto piece = [&](int64_t r0, int64_t r1, bool cut_lo, bool cut_hi) -> int {
        int32_t plo[SODA_HIP_MAX_DIMS], phi[SODA_HIP_MAX_DIMS];
        for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) { plo[d] = lo[d]; phi[d] = hi[d]; }
        if (cut_lo) plo[last] = 0;
        if (cut_hi) phi[last] = 0;
        return sweep_rows(src, dst, r0, r1, step, plo, phi, true);
      };
      int64_t lo_edge = first_own, hi_edge = last_own;
      if (g.has_lo) {    // the lower neighbour's ghost rows: our first send_down rows
        rc = piece(first_own - reach_lo, first_own + send_down + reach_hi, true, true);
        lo_edge = first_own + send_down;
      }
      if (!rc && g.has_hi) {
        rc = piece(last_own - send_up - reach_lo, last_own + reach_hi, true, true);
        hi_edge = last_own - send_up;
      }
      if (!rc) {
        rc = exchange((char*)dst, static_messages());        // beside the interior sweep
        count += 1;
        pending = true;
      }
      if (!rc)
        rc = piece(g.has_lo ? lo_edge - reach_lo : 0,
                   g.has_hi ? hi_edge + reach_hi : g.extent, g.has_lo, g.has_hi);
    } else {
      rc = soda_hip_sweep(plan, &src, &dst, local_dims, step, lo, hi, stream);
    }
    src = dst;
    done += step;
    ++k;
  }
  if (!rc) rc = ghosts_have_landed();
  if (rc) return give_up(rc);
  *result = src;
  if (exchanges) *exchanges = count;
  return 0;
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
  if (slab->world > 1 && !comm)
    return fail(SODA_HIP_ERR_NULL_ARGUMENT, "world %d needs an RCCL communicator", slab->world);
  if (slab->world > 1 && !rccl().ok)
    return fail(SODA_HIP_ERR_NO_DEVICE, "librccl.so could not be loaded: %s", dlerror());
  // as soda_hip_run_slab: whatever is wrong with the call itself is found before the
  // first message is enqueued and leaves the communicator alone
  if (iterate < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "iterate must be >= 1");
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: static cut only for programs over several "
                "fields");
  if (slab->order != SODA_HIP_SLAB_SERIAL)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: serial order only for programs over several "
                "fields");
  SlabGeometry g{};
  int rc = slab_geometry(plan, slab, &g);
  if (rc) return rc;
  const int last = p.dim - 1;
  int64_t row_bytes[SODA_HIP_MAX_IO];
  for (int j = 0; j < n; ++j) {
    // field j's three arrays hold input j and output j in turn
    if (p.elem_size[j] != p.elem_size[p.output_tensor[j]])
      return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: output %d (%d bytes per cell) cannot feed "
                  "input %d (%d)", j, p.elem_size[p.output_tensor[j]], j, p.elem_size[j]);
    row_bytes[j] = p.elem_size[j];
    for (int d = 0; d < last; ++d) row_bytes[j] *= slab->dims[d];
  }
  // the ghost rows must cover what ANY field reads in `exchange` iterations: the composed
  // margin of a field after k iterations is at most k x the hull of one iteration's
  {
    int32_t lo[SODA_HIP_MAX_DIMS], hi[SODA_HIP_MAX_DIMS];
    output_margins(plan, 1, lo, hi);
    if (slab->world > 1 && (slab->reach_lo < lo[last] || slab->reach_hi < hi[last]))
      return fail(SODA_HIP_ERR_CONSTRAINT, "slab reach %d / %d is below the program's %d / %d "
                  "(soda_hip_plan_margins(plan, 1))", slab->reach_lo, slab->reach_hi,
                  (int)lo[last], (int)hi[last]);
  }
  bool rccl_failed = false;
  auto give_up = [&](int e) {
    if (e && !rccl_failed && slab->abort_on_error && slab->world > 1 && comm &&
        rccl().comm_abort) {
      const std::string keep = g_last_error;
      (void)rccl().comm_abort(comm);
      g_last_error = keep + " (communicator aborted)";
    }
    return e;
  };
  hipStream_t s = as_stream(stream);
  int64_t local_dims[SODA_HIP_MAX_DIMS] = {1, 1, 1, 1};
  for (int d = 0; d < p.dim; ++d) local_dims[d] = slab->dims[d];
  local_dims[last] = g.extent;
  const int64_t send_down = g.has_lo ? (int64_t)slab->exchange * slab->reach_hi : 0;
  const int64_t send_up = g.has_hi ? (int64_t)slab->exchange * slab->reach_lo : 0;
  const int64_t first_own = g.ghost_lo, last_own = g.ghost_lo + g.own;
  // ONE group per super-step carries every field's ghost rows; the rows of one field are
  // contiguous, so nothing is packed: four messages per field at most, field by field
  // (both sides of a pair enumerate the fields in the same order)
  auto exchange = [&](void* const* arrays) -> int {
    if (slab->world == 1) return 0;
    const Rccl& r = rccl();
    int e = r.group_start();
    for (int j = 0; j < n && !e; ++j) {
      char* at = (char*)arrays[j];
      const int64_t rb = row_bytes[j];
      if (!e && g.has_lo && send_down)
        e = r.send(at + first_own * rb, (size_t)(send_down * rb), 0, slab->rank - 1, comm, s);
      if (!e && g.has_lo && g.ghost_lo)
        e = r.recv(at, (size_t)(g.ghost_lo * rb), 0, slab->rank - 1, comm, s);
      if (!e && g.has_hi && send_up)
        e = r.send(at + (last_own - send_up) * rb, (size_t)(send_up * rb), 0, slab->rank + 1,
                   comm, s);
      if (!e && g.has_hi && g.ghost_hi)
        e = r.recv(at + last_own * rb, (size_t)(g.ghost_hi * rb), 0, slab->rank + 1, comm, s);
    }
    const int e2 = r.group_end();
    if (e || e2) {
      rccl_failed = true;
      return fail(SODA_HIP_ERR_DEVICE_RUN, "RCCL ghost exchange failed: %s",
                  r.error_string ? r.error_string(e ? e : e2) : "?");
    }
    return 0;
  };
  int fail_rank = -1, fail_at = -1;      // test hook, as in soda_hip_run_slab
  if (const char* env = tuning_env("SODA_HIP_FAIL_RANK")) fail_rank = atoi(env);
  if (const char* env = tuning_env("SODA_HIP_FAIL_SUPERSTEP")) fail_at = atoi(env);
  void* src[SODA_HIP_MAX_IO];
  void* dst[SODA_HIP_MAX_IO];
  for (int j = 0; j < n; ++j) src[j] = a[j];
  int done = 0, k = 0, count = 0;
  while (done < iterate && !rc) {
    rc = exchange(src);
    count += slab->world > 1;
    if (rc) break;
    const int step = std::min(slab->exchange, iterate - done);
    // every field's own valid region: sides cut inside valid rows are fully valid, the
    // global sides - of every dimension - carry the field's own margin after `done`
    // iterations (output j fed input j)
    int32_t lo[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS], hi[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS];
    field_margins(plan, done, lo, hi);
    for (int j = 0; j < n; ++j) {
      if (g.has_lo) lo[j][last] = 0;
      if (g.has_hi) hi[j][last] = 0;
      dst[j] = k % 2 ? c[j] : b[j];
    }
    if (slab->rank == fail_rank && k == fail_at) {
      rc = fail(SODA_HIP_ERR_DEVICE_RUN, "injected failure of rank %d at super-step %d",
                fail_rank, fail_at);
      break;
    }
    rc = soda_hip_sweep_fields(plan, src, dst, local_dims, step, lo, hi, stream);
    for (int j = 0; j < n; ++j) src[j] = dst[j];
    done += step;
    ++k;
  }
  if (rc) return give_up(rc);
  for (int j = 0; j < n; ++j) result[j] = src[j];
  if (exchanges) *exchanges = count;
  return 0;
}

}  // extern "C"
