// The plan of a multi-GPU slab run (slab_plan.h), part of the library: who sends which rows
// to whom, which rows are swept in which order with which margins, where the result ends
// up.  The static cut and the re-cut are two constructions with one output type.
#include "slab_plan.h"

#include <algorithm>

namespace {

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

bool descriptor_in_range(const soda_hip_slab* s) {
  return s->world >= 1 && s->rank >= 0 && s->rank < s->world && s->exchange >= 1 &&
         s->reach_lo >= 0 && s->reach_hi >= 0;
}

// The margins the sweeps of a super-step start from: every field's own after `done`
// iterations on the global sides of every dimension (one output: the hull itself), 0 on
// the sides of the outermost dimension that are cut inside valid rows.
SlabPiece piece_of(Planner* plan, int done, int64_t r0, int64_t r1, bool cut_lo, bool cut_hi,
                   bool final_only) {
  SlabPiece piece{};
  piece.r0 = r0;
  piece.r1 = r1;
  piece.final_only = final_only;
  field_margins(plan, done, piece.valid_lo, piece.valid_hi);
  for (int j = 0; j < plan->prog.n_outputs; ++j) {
    if (cut_lo) piece.valid_lo[j][plan->prog.dim - 1] = 0;
    if (cut_hi) piece.valid_hi[j][plan->prog.dim - 1] = 0;
  }
  return piece;
}

// ---- the static cut (runtime/dist.py: SlabPlan, exchange_ghosts, band_plan, run_slab) ----
int plan_static(Planner* plan, const soda_hip_slab* s, int iterate, int fields, SlabRun* run) {
  const soda_hip_program& p = plan->prog;
  // the geometry is the same for every field of a program over several (output j feeds
  // input j); which driver runs it is the drivers' check
  if (p.n_inputs != p.n_outputs)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: programs with as many outputs as inputs");
  if (!descriptor_in_range(s))
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab descriptor out of range");
  const int64_t own = s->own_last - s->own_first;
  const bool has_lo = s->rank > 0, has_hi = s->rank < s->world - 1;
  const int64_t ghost_lo = has_lo ? (int64_t)s->exchange * s->reach_lo : 0;
  const int64_t ghost_hi = has_hi ? (int64_t)s->exchange * s->reach_hi : 0;
  // a ghost region deeper than a neighbour's own rows would send rows it does
  // not own (runtime/dist.py: SlabPlan raises for the same reason)
  if (own < 1 || (s->world > 1 && own < (int64_t)s->exchange *
                                            std::max(s->reach_lo, s->reach_hi)))
    return fail(SODA_HIP_ERR_CONSTRAINT,
                "slab of %lld own rows is thinner than its ghost regions (%d x %d)",
                (long long)own, s->exchange, std::max(s->reach_lo, s->reach_hi));
  run->local_extent = ghost_lo + own + ghost_hi;
  run->input_offset = run->result_offset = ghost_lo;
  run->result_first = s->own_first;
  run->result_last = s->own_last;
  if (!fields) return 0;
  // rows the neighbours need from us: our first rows go down, our last rows up
  const int64_t send_down = has_lo ? (int64_t)s->exchange * s->reach_hi : 0;
  const int64_t send_up = has_hi ? (int64_t)s->exchange * s->reach_lo : 0;
  const int64_t first_own = ghost_lo, last_own = ghost_lo + own;
  // the same group before every super-step (a one-sided window sends nothing one way)
  std::vector<SlabMessage> ghosts;
  if (has_lo && send_down) ghosts.push_back({true, s->rank - 1, first_own, send_down});
  if (has_lo && ghost_lo) ghosts.push_back({false, s->rank - 1, 0, ghost_lo});
  if (has_hi && send_up) ghosts.push_back({true, s->rank + 1, last_own - send_up, send_up});
  if (has_hi && ghost_hi) ghosts.push_back({false, s->rank + 1, last_own, ghost_hi});
  // Bands first: every super-step but the last first sweeps the bands of rows the
  // neighbours are waiting for, the interior afterwards - unless the slab is too thin for
  // bands.  (That test comes first: the band rows of a thin first rank start below 0.)
  const bool banded = s->order == SODA_HIP_SLAB_BANDS_FIRST && s->world > 1 &&
                      !(own < 2 * (send_down + send_up) + 1);
  for (int done = 0; done < iterate;) {
    SuperStep st;
    st.done = done;
    st.step = std::min(s->exchange, iterate - done);
    st.before = ghosts;
    if (banded && done + st.step < iterate) {
      const int64_t reach_lo = (int64_t)st.step * s->reach_lo,
                    reach_hi = (int64_t)st.step * s->reach_hi;
      if (has_lo)     // the lower neighbour's ghost rows: our first send_down rows
        st.pieces.push_back(piece_of(plan, done, first_own - reach_lo,
                                     first_own + send_down + reach_hi, true, true, true));
      if (has_hi)
        st.pieces.push_back(piece_of(plan, done, last_own - send_up - reach_lo,
                                     last_own + reach_hi, true, true, true));
      st.exchange_after = (int)st.pieces.size() - 1;
      st.pieces.push_back(piece_of(plan, done, has_lo ? first_own + send_down - reach_lo : 0,
                                   has_hi ? last_own - send_up + reach_hi : run->local_extent,
                                   has_lo, has_hi, true));
    } else {
      st.pieces.push_back(piece_of(plan, done, 0, run->local_extent, has_lo, has_hi, false));
    }
    done += st.step;
    run->steps.push_back(st);
  }
  return 0;
}

// ---- slabs re-cut to the shrinking valid box (runtime/dist.py: RecutPlan, run_recut) ----
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
};

int recut_table(const soda_hip_program& p, const soda_hip_slab* s, int iterate, RecutTable* t) {
  if (p.n_inputs != 1 || p.n_outputs != 1)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slabs: static cut only for programs over several "
                "fields");
  if (!descriptor_in_range(s) || iterate < 1)
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
  return 0;
}

// before super-step i: to every rank the rows it reads and we hold, from every rank the
// rows we read and it holds - ghost rows and rows changing owner alike (both sides derive
// a pair's rows from the same table; ascending peers, sends first)
std::vector<SlabMessage> recut_messages(const RecutTable& t, const soda_hip_slab* s, size_t i) {
  std::vector<SlabMessage> m;
  const RecutStep& st = t.steps[i];
  const Rows& mine = st.owned[s->rank];
  for (int pass = 0; pass < 2; ++pass)
    for (int q = 0; q < s->world; ++q) {
      if (q == s->rank) continue;
      const Rows rows = pass == 0 ? intersect(st.need[q], mine)
                                  : intersect(st.need[s->rank], st.owned[q]);
      const bool wanted = pass == 0 ? !st.need[q].empty() && !mine.empty()
                                    : !st.need[s->rank].empty() && !st.owned[q].empty();
      if (wanted && !rows.empty())
        m.push_back({pass == 0, q, rows.lo - t.base, rows.hi - rows.lo});
    }
  return m;
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
  if (b_lo > lo) bands->push_back(Rows{lo, b_lo});
  if (b_hi < hi) bands->push_back(Rows{b_hi, hi});
  interior->lo = b_lo;
  interior->hi = b_hi;
  return true;
}

int plan_recut(Planner* plan, const soda_hip_slab* s, int iterate, int fields, SlabRun* run) {
  RecutTable t;
  int rc = recut_table(plan->prog, s, iterate, &t);
  if (rc) return rc;
  run->local_extent = t.extent;
  run->input_offset = s->own_first - t.base;
  run->result_first = t.final[s->rank].lo;
  run->result_last = t.final[s->rank].hi;
  run->result_offset = t.final[s->rank].lo - t.base;
  if (!fields) return 0;
  const bool overlapped = s->order == SODA_HIP_SLAB_BANDS_FIRST && s->world > 1;
  for (size_t i = 0; i < t.steps.size(); ++i) {
    SuperStep st;
    st.done = t.steps[i].done;
    st.step = t.steps[i].step;
    st.before = recut_messages(t, s, i);
    // a piece is the sub-array of the rows it reads; those start and end at rows that are
    // valid (produced or received): every outer side is cut
    auto piece = [&](const Rows& out, bool final_only) {
      st.pieces.push_back(piece_of(plan, st.done,
                                   out.lo - (int64_t)st.step * s->reach_lo - t.base,
                                   out.hi + (int64_t)st.step * s->reach_hi - t.base, true, true,
                                   final_only));
    };
    const Rows out{t.steps[i].cuts[s->rank], t.steps[i].cuts[s->rank + 1]};
    std::vector<Rows> bands;
    Rows interior;
    if (overlapped && recut_pieces(t, s, i, &bands, &interior)) {
      for (const Rows& band : bands) piece(band, true);
      st.exchange_after = (int)bands.size() - 1;
      piece(interior, true);
    } else if (!out.empty()) {
      piece(out, false);
    }
    run->steps.push_back(st);
  }
  return 0;
}

}  // namespace

int plan_slab_run(Planner* plan, const soda_hip_slab* slab, int iterate, int fields,
                  SlabRun* run) {
  if (fields && iterate < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "iterate must be >= 1");
  if (fields && slab->order != SODA_HIP_SLAB_SERIAL && slab->order != SODA_HIP_SLAB_BANDS_FIRST)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab order %d", (int)slab->order);
  if (slab->cut != SODA_HIP_SLAB_CUT_STATIC && slab->cut != SODA_HIP_SLAB_CUT_RECUT)
    return fail(SODA_HIP_ERR_CONSTRAINT, "slab cut %d", (int)slab->cut);
  *run = SlabRun{};
  for (int j = 0; j < fields; ++j) {
    run->row_bytes[j] = plan->prog.elem_size[j];
    for (int d = 0; d < plan->prog.dim - 1; ++d) run->row_bytes[j] *= slab->dims[d];
  }
  return slab->cut == SODA_HIP_SLAB_CUT_RECUT ? plan_recut(plan, slab, iterate, fields, run)
                                              : plan_static(plan, slab, iterate, fields, run);
}

extern "C" int soda_hip_slab_exchange(int64_t rows, int world, int reach_lo, int reach_hi,
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
