// The launch planner of libsoda_hip.so: splits `iterate` into kernel depths, sizes
// every launch's box and grid, chooses chunk lengths and XCD placements and says which
// buffer each tensor of a launch is.  Nothing here calls the HIP runtime (schedule.h);
// soda_hip.cpp allocates, binds the buffers and launches.
#include "schedule.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

const char* tuning_env(const char* name) {
  const char* on = getenv("SODA_HIP_TUNING");
  return (on && on[0] == '1') ? getenv(name) : nullptr;
}

int n_tensors(const soda_hip_program& p) { return p.n_inputs + p.n_stages; }

bool is_output_tensor(const soda_hip_program& p, int t) {
  for (int j = 0; j < p.n_outputs; ++j)
    if (p.output_tensor[j] == t) return true;
  return false;
}

namespace {

// Composed read windows back to the sweep's inputs, one iteration at a time
// (reference core.py:794-835 on bounding boxes; output j feeds input j,
// core.py:342-360).  A fresh composition starts from the zero box for every input, a
// resumed one (Planner::resumed) from what each input's region lacks beyond the margins
// all inputs share.
void grow_boxes(Planner* plan, Growth* g, int iterations) {
  const soda_hip_program& p = plan->prog;
  const int nt = n_tensors(p);
  if (g->boxes.empty()) {
    g->feed = g->start;
    g->feed.resize(p.n_inputs, Box{});
    for (auto& b : g->feed) b.set = true;
  }
  while ((int)g->boxes.size() < iterations) {
    std::vector<Box> cur(nt, Box{});
    for (int i = 0; i < p.n_inputs; ++i) cur[i] = g->feed[i];
    for (int s = 0; s < p.n_stages; ++s) {
      const int t = p.n_inputs + s;
      Box acc{};
      for (int w = 0; w < p.n_windows; ++w) {
        const soda_hip_window& win = p.window[w];
        if (win.stage != t) continue;
        const Box& par = cur[win.parent];
        for (int d = 0; d < p.dim; ++d) {
          const int32_t lo = par.lo[d] + win.lo[d], hi = par.hi[d] + win.hi[d];
          acc.lo[d] = acc.set ? std::min(acc.lo[d], lo) : lo;
          acc.hi[d] = acc.set ? std::max(acc.hi[d], hi) : hi;
        }
        acc.set = true;
      }
      // the cell itself must lie inside the array: boxes contain the origin
      for (int d = 0; d < p.dim; ++d) {
        acc.lo[d] = std::min<int32_t>(acc.lo[d], 0);
        acc.hi[d] = std::max<int32_t>(acc.hi[d], 0);
      }
      cur[t] = acc;
    }
    if (p.n_inputs == p.n_outputs)
      for (int j = 0; j < p.n_inputs; ++j) g->feed[j] = cur[p.output_tensor[j]];
    g->boxes.push_back(cur);
  }
}

// hull over the outputs after `iterations` iterations of the composition `g`, as positive
// margins; level 0 = the hull over the inputs the composition starts from
void hull_margins(Planner* plan, Growth* g, int iterations, int32_t* lo, int32_t* hi) {
  const soda_hip_program& p = plan->prog;
  for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) lo[d] = hi[d] = 0;
  if (iterations <= 0) {
    for (const Box& b : g->start)
      for (int d = 0; d < p.dim; ++d) {
        lo[d] = std::max(lo[d], -b.lo[d]);
        hi[d] = std::max(hi[d], b.hi[d]);
      }
    return;
  }
  grow_boxes(plan, g, iterations);
  const std::vector<Box>& b = g->boxes[iterations - 1];
  for (int j = 0; j < p.n_outputs; ++j) {
    const Box& o = b[p.output_tensor[j]];
    for (int d = 0; d < p.dim; ++d) {
      lo[d] = std::max(lo[d], -o.lo[d]);
      hi[d] = std::max(hi[d], o.hi[d]);
    }
  }
}

}  // namespace

// hull over the outputs after `iterations` iterations of a fresh run, as positive margins
void output_margins(Planner* plan, int iterations, int32_t* lo, int32_t* hi) {
  hull_margins(plan, &plan->fresh, iterations, lo, hi);
}

// the same per output: output j of a fresh run lives on [lo[j][d], dims[d] - hi[j][d])
void field_margins(Planner* plan, int iterations, int32_t (*lo)[SODA_HIP_MAX_DIMS],
                   int32_t (*hi)[SODA_HIP_MAX_DIMS]) {
  const soda_hip_program& p = plan->prog;
  if (iterations > 0) grow_boxes(plan, &plan->fresh, iterations);
  for (int j = 0; j < p.n_outputs; ++j)
    for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) {
      const bool grown = iterations > 0 && d < p.dim;
      lo[j][d] = grown ? -plan->fresh.boxes[iterations - 1][p.output_tensor[j]].lo[d] : 0;
      hi[j][d] = grown ? plan->fresh.boxes[iterations - 1][p.output_tensor[j]].hi[d] : 0;
    }
}

namespace {

// Cost model of a streaming launch (what the scheduler compares depths with; it
// never has to be right in absolute terms).  A workgroup walks `steps` rows or
// planes; with R workgroups resident per CU one step of all of them takes
//   max( R * step_valu / 4 SIMDs / (clock * issue efficiency),
//        R * CUs * step_bytes / HBM rate this access pattern reaches ).
// Constants measured on MI355X with the jacobi2d kernels of every depth
// (tools/chunk_sweep.py, 16384^2): step_valu carries the arithmetic plus a fixed
// cost per streamed row (barrier, ring, hand-offs; kernel.py: annotate_cost) and
// is issued at the ~2.0 GHz the chip holds under that load; the shallow kernels
// move 4.5-4.7 TB/s.  Modelled vs measured us per step of a full chip: depth 12
// 0.91 / 0.89, 16 0.96 / 0.98, 20 0.84 / 0.84, 24 0.96 / 0.96.
const double kModelValuHz = 2.0e9;
const double kModelHbmBytesPerSec = 4.6e12;
const double kModelLaunchUs = 2.0;

// `footprint` = bytes of the arrays the launch streams (inputs + outputs of its box).
// With calibration figures in the descriptor (soda_hip_kernel.step_ns_*,
// stream_gbps): the kernel's own step time at the occupancy this grid reaches,
// interpolated between one workgroup per CU and a full chip, or - on arrays beyond
// the Infinity Cache - the time its HBM rate allows, whichever is longer.
// The HBM term fades in between arrays that live in the 256 MiB Infinity Cache and
// arrays several times its size (jacobi3d, one-level-per-wavefront kernel: 1.63 us per
// step at 304^3 = 215 MiB in + out, the step time of a cache-resident array; 2.03 us at
// 400^3 = 488 MiB; 2.41 us at 512^3).
// The two footprints are part of the kernel's calibration record (soda_hip_kernel.
// fade_lo_mib / fade_hi_mib, tools/calibrate.py); these are the defaults of kernels
// that carry none.
const double kCacheResidentMiB = 128.0;
const double kStreamingMiB = 512.0;
const int64_t kMaxGridYZ = 65535;      // workgroups along grid.y / grid.z

// `resident` = workgroups of this launch the chip holds at once (the kernel's occupancy,
// or less under a cap on workgroups per CU; 0 = the kernel's occupancy)
double step_seconds(const Planner* plan, int k, double blocks, double footprint = 0,
                    double resident = 0) {
  const soda_hip_kernel& desc = plan->kernels[k];
  const double cus = std::max(1, plan->cus);
  const double full = std::max(1, plan->resident_blocks[k]) / cus;
  const double held = resident > 0 ? std::min(full, resident / cus) : full;
  // a grid smaller than the chip holds: fewer workgroups share each CU
  const double per_cu = std::min(held, std::max(1.0, blocks / cus));
  if (desc.step_ns_full > 0 && desc.step_ns_one > 0) {
    const double share = full > 1 ? (per_cu - 1) / (full - 1) : 1.0;
    double t = (desc.step_ns_one + (desc.step_ns_full - desc.step_ns_one) * share) * 1e-9;
    const double mib = 1024.0 * 1024.0;
    const double fade_lo = (desc.fade_lo_mib > 0 ? desc.fade_lo_mib : kCacheResidentMiB) * mib;
    const double fade_hi = std::max(fade_lo + mib,
        (desc.fade_hi_mib > 0 ? desc.fade_hi_mib : kStreamingMiB) * mib);
    if (desc.stream_gbps > 0 && desc.step_bytes > 0 && footprint > fade_lo) {
      const double weight = std::min(1.0, (footprint - fade_lo) / (fade_hi - fade_lo));
      t = std::max(t, weight * std::min(blocks, held * cus) * desc.step_bytes /
                          (desc.stream_gbps * 1e9));
    }
    return t;
  }
  if (desc.step_valu <= 0 && desc.step_bytes <= 0) return 0;
  const double valu = per_cu * desc.step_valu / 4.0 / kModelValuHz;
  const double hbm = per_cu * cus * desc.step_bytes / kModelHbmBytesPerSec;
  return std::max(valu, hbm);
}

}  // namespace

double footprint_of(const Planner* plan, const soda_hip_args& args) {
  const soda_hip_program& p = plan->prog;
  double cells = 1;
  for (int e = 0; e < p.dim; ++e) cells *= (double)(args.box_hi[e] - args.box_lo[e]);
  double footprint = 0;
  for (int j = 0; j < p.n_inputs; ++j) footprint += cells * p.elem_size[j];
  for (int j = 0; j < p.n_outputs; ++j) footprint += cells * p.elem_size[p.output_tensor[j]];
  return footprint;
}

namespace {

// workgroups per CU a streaming launch of kernel k is capped at (0 = no cap):
// soda_hip_kernel.stream_wgs_per_cu for boxes beyond the Infinity Cache
// (tuning: SODA_HIP_WGS_PER_CU = N for every streaming kernel, -1 = never)
int streaming_cap(const Planner* plan, int k, double footprint) {
  if (plan->wgs_per_cu_cap != 0) return std::max(0, plan->wgs_per_cu_cap);
  if (footprint <= kBeyondCacheBytes) return 0;
  return std::max(0, (int)plan->kernels[k].stream_wgs_per_cu);
}

}  // namespace

std::array<int64_t, 5> stream_key(const Planner* plan, int k, const soda_hip_args& args) {
  std::array<int64_t, 5> key = {k, 1, 1, 1, 1};
  for (int d = 0; d < plan->prog.dim && d < 4; ++d) key[1 + d] = args.box_hi[d] - args.box_lo[d];
  return key;
}

std::array<int64_t, 5> split_key(const Planner* plan, const int64_t* dims, int iterate) {
  std::array<int64_t, 5> key;
  for (int d = 0; d < 4; ++d) key[d] = d < plan->prog.dim ? dims[d] : 1;
  key[4] = iterate;
  return key;
}

namespace {

// Fused kernels of programs with several outputs (kernel_fields2d.py, kernel_fields3d.py)
// store output j on a box of its own: the launch's box - the intersection of the outputs'
// boxes - widened by the extras of soda_hip_args.param[1..3] (include/soda_hip.h): 2-D four
// extras of 8 bits per output, two outputs to a word; 3-D six, one output to a word; 1-D
// (kernel_fields1d.py) two, four outputs to a word.
constexpr int kMaxExtra = 255;

int max_extra_outputs(int dim) { return dim == 3 ? 3 : 6; }

bool takes_output_extras(const Planner* plan, const soda_hip_kernel& desc) {
  return desc.kind == SODA_HIP_KERNEL_FUSED && plan->prog.dim >= 1 && plan->prog.dim <= 3 &&
         plan->prog.n_outputs > 1;
}

// extras of output j: {lo of dimension 0 .. dim - 1, hi of dimension 0 .. dim - 1}
void unpack_extras(int dim, const soda_hip_args& a, int j, int64_t* ex) {
  const uint64_t word = dim == 1   ? (uint64_t)a.param[1 + j / 4] >> (16 * (j % 4))
                        : dim == 2 ? (uint64_t)a.param[1 + j / 2] >> (32 * (j % 2))
                                   : (uint64_t)a.param[1 + j];
  for (int i = 0; i < 2 * dim; ++i) ex[i] = (word >> (8 * i)) & 0xff;
}

// the union of the outputs' boxes: what the tiles and chunks of such a launch cover
void widen_to_union(const Planner* plan, soda_hip_args* a) {
  const int dim = plan->prog.dim;
  int64_t most[6] = {0, 0, 0, 0, 0, 0};
  for (int j = 0; j < plan->prog.n_outputs; ++j) {
    int64_t ex[6];
    unpack_extras(dim, *a, j, ex);
    for (int i = 0; i < 2 * dim; ++i) most[i] = std::max(most[i], ex[i]);
  }
  for (int d = 0; d < dim; ++d) {
    a->box_lo[d] -= most[d];
    a->box_hi[d] += most[dim + d];
  }
}

// Streaming kernel: every workgroup walks `chunk + fill_rows` rows of the
// outer dimension.  Pick the chunk length that minimises
//   rounds(chunk) * (chunk + fill_rows),
// rounds = ceil(workgroups / workgroups resident on the chip): a grid
// that is 2.4 chip-fulls costs 3, so aim for whole rounds.
// `inner` = workgroups along the other dimensions, `extent` = rows (planes) of the box.
// Returns the chunk length; param[0], the LDS padding and the price go into `out`.
int64_t choose_stream_chunk(const Planner* plan, int k, const soda_hip_args& args,
                            int64_t inner, int64_t extent, Launch* out) {
  const soda_hip_kernel& desc = plan->kernels[k];
  const double footprint = footprint_of(plan, args);
  int64_t resident = std::max(1, plan->resident_blocks[k]);
  // A cap on the workgroups a CU holds at once (streaming launches of the
  // memory-bound kernels: fewer wavefronts walking longer chunks keep the set of
  // DRAM pages the chip touches at a time small - tools/copyceil.hip): enforced
  // with dynamic LDS the kernel never uses, 160 KiB / (cap + 1) + 1 KiB each
  int cap = streaming_cap(plan, k, footprint);
  int64_t tuned_chunk = 0;
  if (desc.stream_chunk > 0 && footprint > kBeyondCacheBytes &&
      plan->chunk_rows_override == 0 && plan->wgs_per_cu_cap == 0) {
    const auto tuned = plan->tuned_stream.find(stream_key(plan, k, args));
    if (tuned != plan->tuned_stream.end()) {
      tuned_chunk = tuned->second[0];
      cap = tuned->second[1];
    }
  }
  if (cap > 0 && resident > (int64_t)cap * plan->cus) {
    // each workgroup must take more than 1 / (cap + 1) of the CU's LDS and at most
    // 1 / cap of it, its static LDS included; a cap the padding cannot realise (the
    // static part alone already excludes `cap` workgroups) is not applied
    const int64_t lds_cu = plan->lds_per_cu, fixed = plan->static_lds[k];
    const int64_t granule = 1024;
    int64_t total = lds_cu / (cap + 1) / granule * granule + granule;   // > lds_cu / (cap + 1)
    total = std::max(total, (fixed + granule - 1) / granule * granule);
    if (total * cap <= lds_cu) {
      resident = (int64_t)cap * plan->cus;
      out->lds_bytes = (unsigned)std::max<int64_t>(0, total - fixed);
    }
  }
  int64_t best = desc.tile[plan->prog.dim - 1], best_cost = -1;
  const int64_t shortest = plan->chunk_rows_min;   // 8; SODA_HIP_CHUNK_MIN
  for (int64_t chunk = shortest;
       chunk <= std::max<int64_t>(shortest, std::min<int64_t>(extent, 4096));
       chunk += 4) {
    const int64_t blocks = inner * ((extent + chunk - 1) / chunk);
    const int64_t rounds = (blocks + resident - 1) / resident;
    const int64_t cost = rounds * (chunk + desc.fill_rows);
    // among equal step counts the LONGEST chunk: fewer workgroups, fewer fill rows
    // fetched (jacobi3d box 504^3: 5 chunks of 104 planes in one round and 11 of
    // 48 in two both walk 112 steps; the long ones read 8 % less).  (Round 3 also
    // measured the chunk by its PRICED time - cfg4 +16 %, cfg2 +7 % - and the shortest
    // chunk on ties - cfg5 +3 %: docs/DESIGN_HISTORY.md 4.3; both switches are gone.)
    if (best_cost < 0 || cost <= best_cost) {
      best_cost = cost;
      best = chunk;
    }
  }
  // the kernel's measured chunk for boxes beyond the cache (soda_hip_kernel.
  // stream_chunk): short chunks in dispatch order keep the rows in flight together
  // (tuning: SODA_HIP_CHUNK_ROWS = N forces N, -1 the rule above whatever the kernel says)
  if (desc.stream_chunk > 0 && footprint > kBeyondCacheBytes &&
      plan->chunk_rows_override == 0)
    best = std::max<int64_t>(1, std::min<int64_t>(
        tuned_chunk > 0 ? tuned_chunk : desc.stream_chunk, extent));
  if (plan->chunk_rows_override > 0) best = plan->chunk_rows_override;
  // ... but never so short that the chunks outnumber what one grid dimension takes
  // (a 256 x 1M box in chunks of 8 rows would be 125 000 workgroups along y)
  best = std::max<int64_t>(best, (extent + kMaxGridYZ - 1) / kMaxGridYZ);
  out->args.param[0] = best;
  const double blocks = (double)inner * (double)((extent + best - 1) / best);
  const double rounds = std::ceil(blocks / (double)resident);
  out->rounds = (long long)rounds;
  out->est_us = kModelLaunchUs + rounds * (double)(best + desc.fill_rows) *
                                     step_seconds(plan, k, blocks, footprint,
                                                  (double)resident) * 1e6;
  out->resident = (long long)resident;
  return best;
}

// Fused kernel of a 1-D program (kernel_stream1d.py): no streamed dimension, a workgroup
// does its whole tile in one go - step_valu and step_bytes are per workgroup per launch.
// The price is the launch constant plus, per chip-full of workgroups, the larger of a
// workgroup's VALU time and its bytes at the chip's streaming rate (step_seconds).
void price_segments(const Planner* plan, int k, const soda_hip_args& args, Launch* out) {
  const double resident = std::max(1, plan->resident_blocks[k]);
  const double blocks = out->grid[0];
  const double rounds = std::ceil(blocks / resident);
  out->rounds = (long long)rounds;
  out->resident = (long long)resident;
  out->est_us = kModelLaunchUs +
                rounds * step_seconds(plan, k, blocks, footprint_of(plan, args), resident) * 1e6;
}

// the first and the last tile of a row store the columns the alignment left over
// (include/soda_hip.h: edge_slack): tiles start up to `slack` columns inside the box.
// Returns the tiles along x; *origin = the column they start at.
int64_t edge_slack_tiles(const soda_hip_kernel& desc, const soda_hip_args& args,
                         int64_t* origin) {
  const int64_t slack = desc.edge_slack, tile = desc.tile[0];
  const int64_t lo = args.box_lo[0], hi = args.box_hi[0];
  int64_t x0 = (lo + slack) - (lo + slack) % desc.origin_align;
  if (x0 >= hi) x0 = lo - lo % desc.origin_align;     // a box narrower than the shift
  int64_t nx = std::max<int64_t>(1, (hi - x0 - slack + tile - 1) / tile);
  if (nx == 1 && hi > x0 + tile) {      // one tile cannot stretch both ways
    x0 = lo - lo % desc.origin_align;
    nx = std::max<int64_t>(1, (hi - x0 - slack + tile - 1) / tile);
  }
  *origin = x0;
  return nx;
}

// Per-stage kernels take one row (plane) per workgroup; past the 65535
// limit of grid.y / grid.z - and for every 4-D box - the rows and planes are
// folded into one index spread over grid.y x grid.z (kernel_stage.py;
// param[0] = 1 tells a 3-D kernel so).
int fold_rows(const Planner* plan, const soda_hip_kernel& desc, const soda_hip_args& args,
              Launch* out) {
  int64_t rows = 1;
  for (int d = 1; d < plan->prog.dim; ++d) rows *= args.box_hi[d] - args.box_lo[d];
  const int64_t gy = std::min<int64_t>(rows, 65535), gz = (rows + gy - 1) / gy;
  if (gz > 65535)
    return fail(SODA_HIP_ERR_EXTENTS_TOO_LARGE, "kernel %s: %lld rows", desc.name,
                (long long)rows);
  out->grid[1] = (unsigned)gy;
  out->grid[2] = (unsigned)gz;
  out->args.param[0] = 1;
  return 0;
}

// Runs (kernel_stream3d_blk.py, xcd_runs): XCD x (= workgroup id mod 8) takes the
// tiles [x P, (x + 1) P) of the x-fastest order, P = ceil(tiles / 8), so that a
// tile's x- and y-neighbours stream beside it on the same L2.
int place_runs(const soda_hip_kernel& desc, int64_t edge_origin, Launch* out) {
  const int64_t gx = out->grid[0], gy = out->grid[1], gz = out->grid[2];
  const int64_t per = (gx * gy * gz + 7) / 8;
  if (per * 8 > 2147483647LL || gx > 65535 || gy > 65535)
    return fail(SODA_HIP_ERR_EXTENTS_TOO_LARGE, "grid of kernel %s would be %lld",
                desc.name, (long long)(per * 8));
  out->args.param[1] = 1 | (1 << 16);
  if (edge_origin >= 0) out->args.param[1] |= edge_origin << 32;
  out->args.param[2] = gx | (gy << 16);
  out->args.param[3] = per;
  out->grid[0] = (unsigned)(per * 8);
  out->grid[1] = out->grid[2] = 1;
  return 0;
}

// XCD-aware placement (kernel_stream3d_wp.py, xcd_tiles): the plane of
// gx x gy tiles is cut into super-tiles of SX x SY tiles whose workgroups run
// together on one XCD and share its L2.  Pick the shape that fetches least:
// padding (tiles beyond the edge) x halo and cache-line slack amortised over
// the super-tile.
int place_super_tiles(const Planner* plan, int k, Launch* out) {
  const soda_hip_kernel& desc = plan->kernels[k];
  const int64_t gx = out->grid[0], gy = out->grid[1], gz = out->grid[2];
  const double w = desc.tile[0], r = desc.tile[1];
  const double line = 128.0 / std::max(1, plan->prog.elem_size[0]);
  const double hx = std::max(0, desc.min_extent[0] - desc.tile[0]) + 0.75 * line;
  const double hy = std::max(0, desc.min_extent[1] - desc.tile[1]);
  // Which shapes are eligible (jacobi3d, depth-4 wave-pipelined kernel, one call
  // each; `ids` = workgroup ids launched, padding included):
  //   512^3, 9 x 21 x 4 = 756 tiles on 768 slots: plain deal 378 us, 3 x 1 338,
  //     1 x 3 354, 2 x 1 (840 ids) 435, 1 x 2 (792 ids) 450, 3 x 7 (105 tiles on
  //     four XCDs, 84 on the others) 500
  //   440^3, 8 x 18 x 5 = 720: plain 223, 2 x 1 199, 4 x 1 189, 1 x 2 / 1 x 3 223
  //   392^3, 7 x 16 x 6 = 672: plain 162, 2 x 1 / 4 x 1 (768 ids) 150 / 140
  //   344^3, 6 x 14 x 9 = 756: plain 104, 3 x 1 97, 2 x 2 96, 4 x 1 (1008 ids) 140
  //   264^3, 5 x 11 x 13 = 715: plain 63, 2 x 1 / 3 x 1 (864 ids) 83 / 77;
  //     5 x 11 x 8 = 440: plain 56, 3 x 1 (66 tiles on the even XCDs, 44 on the odd) 67
  // So: (1) a partial super-tile is padded with workgroups that exit at once, and
  // that is harmless only while ALL ids fit the chip at once; (2) super-tiles are
  // dealt whole, so the busiest XCD must stay within 3 % of its even share;
  // (3) grouping along x is what pays (neighbours share 128-byte lines), along y
  // hardly at all.
  const int64_t real = gx * gy * gz;
  const int64_t slots = std::max<int64_t>(8, plan->resident_blocks[k] / 8 * 8);
  const int64_t even = (real + 7) / 8;
  const int64_t limit = even + std::max<int64_t>(1, even * 3 / 100);
  int best_sx = 1, best_sy = 1;
  double best = -1;
  // (the kernel names its largest group, soda_hip_kernel.xcd_tiles: 4 for
  // kernel_stream3d_wp, 1 = the plain deal for the block form.)  Groups of 16-24
  // tiles cut the PMC read bytes further (jacobi3d x200: reads 2.5x -> 1.7x the
  // written bytes) but every one measured ran SLOWER (cfg5 6.2 -> 7.0-7.4 ms)
  int max_group = std::max(1, (int)desc.xcd_tiles);   // the kernel's own limit
  if (const char* env = tuning_env("SODA_HIP_XCD_GROUP")) max_group = std::max(1, atoi(env));
  const std::array<int64_t, 4> key = {k, gx, gy, gz};
  const auto known = plan->xcd_shape.find(key);
  const bool cached = known != plan->xcd_shape.end() && !tuning_env("SODA_HIP_XCD_GROUP");
  if (cached) { best_sx = known->second.first; best_sy = known->second.second; }
  for (int sx = 1; sx <= 8 && !cached; ++sx)
    for (int sy = 1; sy <= 8; ++sy) {
      if (sx * sy > max_group) continue;
      const int64_t nsx = (gx + sx - 1) / sx, nsy = (gy + sy - 1) / sy;
      const int64_t ids = (nsx * nsy * gz + 7) / 8 * 8 * sx * sy;
      if (sx * sy > 1 && ids > (real <= slots ? slots : real + real * 3 / 100)) continue;
      // real tiles per XCD: super-tile g -> XCD g % 8; edge super-tiles are partial
      int64_t per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t g = 0; g < nsx * nsy * gz; ++g) {
        const int64_t tx = std::min<int64_t>(sx, gx - (g % nsx) * sx);
        const int64_t ty = std::min<int64_t>(sy, gy - ((g / nsx) % nsy) * sy);
        per_xcd[g % 8] += tx * ty;
      }
      if (sx * sy > 1 && *std::max_element(per_xcd, per_xcd + 8) > limit) continue;
      const double cost = (1 + hx / (std::min<int64_t>(sx, gx) * w)) *
                          (1 + 0.25 * hy / (std::min<int64_t>(sy, gy) * r));
      if (best < 0 || cost < best) { best = cost; best_sx = sx; best_sy = sy; }
    }
  if (!cached && !tuning_env("SODA_HIP_XCD_GROUP"))
    plan->xcd_shape[key] = std::make_pair(best_sx, best_sy);
  if (const char* env = tuning_env("SODA_HIP_XCD_TILES")) {   // tuning: "SX,SY"
    int sx = 0, sy = 0;
    if (sscanf(env, "%d,%d", &sx, &sy) == 2 && sx > 0 && sy > 0) { best_sx = sx; best_sy = sy; }
  }
  if (tuning_env("SODA_HIP_DEBUG"))
    fprintf(stderr, "soda_hip: %s: %lld x %lld x %lld tiles, super-tiles of %d x %d\n",
            desc.name, (long long)gx, (long long)gy, (long long)gz, best_sx, best_sy);
  const int64_t nsx = (gx + best_sx - 1) / best_sx, nsy = (gy + best_sy - 1) / best_sy;
  const int64_t supers = nsx * nsy * gz;
  const int64_t total = (supers + 7) / 8 * 8 * best_sx * best_sy;
  if (total > 2147483647LL || nsx > 65535 || nsy > 65535)
    return fail(SODA_HIP_ERR_EXTENTS_TOO_LARGE, "grid of kernel %s would be %lld",
                desc.name, (long long)total);
  out->args.param[1] = best_sx | (best_sy << 16);
  out->args.param[2] = nsx | (nsy << 16);
  out->grid[0] = (unsigned)total;
  out->grid[1] = out->grid[2] = 1;
  return 0;
}

// One launch of kernel k on the box of `launch_args`: the grid, dimension by dimension,
// then whatever the kernel's form asks for on top (chunks, folded rows, XCD placement).
int make_launch(const Planner* plan, int k, const soda_hip_args& launch_args,
                Launch* out, bool* empty) {
  const soda_hip_kernel& desc = plan->kernels[k];
  const int dim = plan->prog.dim;
  out->kernel = k;
  out->args = launch_args;
  // the grid is sized by `args`: the launch's box, or the union of the outputs' boxes
  soda_hip_args args = launch_args;
  if (takes_output_extras(plan, desc)) widen_to_union(plan, &args);
  out->est_us = 0;
  out->lds_bytes = 0;
  *empty = false;
  // never launch a box that sticks out of the array
  for (int d = 0; d < dim; ++d)
    if (args.box_hi[d] > args.box_lo[d] &&
        (args.box_lo[d] < 0 || args.box_hi[d] > args.dims[d]))
      return fail(SODA_HIP_ERR_OUT_OF_BOUNDS,
                  "kernel %s: box [%lld, %lld) outside dimension %d of extent %lld",
                  desc.name, (long long)args.box_lo[d], (long long)args.box_hi[d], d,
                  (long long)args.dims[d]);
  for (int d = 0; d < 3; ++d) out->grid[d] = 1;
  int64_t edge_origin = -1;      // soda_hip_kernel.edge_slack: where the tiles start along x
  if (dim > 3 && desc.kind != SODA_HIP_KERNEL_STAGE)
    return fail(SODA_HIP_ERR_INTERNAL, "kernel %s: only per-stage kernels take 4-D boxes",
                desc.name);
  bool folded = dim > 3;   // a 4-D box always goes as folded rows
  for (int d = 0; d < dim; ++d) {
    int64_t extent = args.box_hi[d] - args.box_lo[d];
    if (extent <= 0) { *empty = true; return 0; }
    if (d == 0 && desc.origin_align > 1)   // tiles start at an aligned column
      extent += args.box_lo[0] % desc.origin_align;
    if (desc.tile[d] <= 0)
      return fail(SODA_HIP_ERR_INTERNAL, "kernel %s has tile[%d]=%d", desc.name, d,
                  desc.tile[d]);
    int64_t tile = desc.tile[d];
    if (d == dim - 1 && desc.fill_rows > 0 && dim >= 2) {
      int64_t inner = 1;
      for (int e = 0; e < dim - 1; ++e) inner *= out->grid[e];
      tile = choose_stream_chunk(plan, k, args, inner, extent, out);
    }
    int64_t g = (extent + tile - 1) / tile;
    if (d == 0 && desc.edge_slack > 0 && desc.origin_align > 1 && desc.xcd_tiles < 0 && dim == 3)
      g = edge_slack_tiles(desc, args, &edge_origin);
    if (d > 0 && desc.kind == SODA_HIP_KERNEL_STAGE && (g > 65535 || dim > 3)) {
      // folded after the loop (fold_rows), once every extent is known
      folded = true;
      g = 1;
    }
    if (g > (d == 0 ? 2147483647LL : 65535LL))
      return fail(SODA_HIP_ERR_EXTENTS_TOO_LARGE,
                  "grid dimension %d of kernel %s would be %lld", d, desc.name,
                  (long long)g);
    if (d < 3) out->grid[d] = (unsigned)g;
  }
  if (folded) {
    int rc = fold_rows(plan, desc, args, out);
    if (rc) return rc;
  }
  if (dim == 1 && desc.kind == SODA_HIP_KERNEL_FUSED) price_segments(plan, k, args, out);
  if (desc.xcd_tiles < 0 && dim == 3) return place_runs(desc, edge_origin, out);
  if (desc.xcd_tiles && dim == 3) return place_super_tiles(plan, k, out);
  return 0;
}

int check_box_inside(const Planner* plan, const soda_hip_args& a,
                     const int32_t* reach_lo, const int32_t* reach_hi,
                     bool signed_window = false) {
  // every cell a launch may read must be inside the array: the kernels rely on
  // it.  reach_* are margins (>= 0) or, with signed_window, window offsets
  // (lo <= hi, either sign).
  for (int d = 0; d < plan->prog.dim; ++d) {
    if (a.box_hi[d] <= a.box_lo[d]) continue;
    const int64_t first = signed_window ? a.box_lo[d] + reach_lo[d] : a.box_lo[d] - reach_lo[d];
    if (first < 0 || a.box_hi[d] + reach_hi[d] > a.dims[d])
      return fail(SODA_HIP_ERR_OUT_OF_BOUNDS,
                  "launch would read [%lld, %lld) of dimension %d, extent %lld",
                  (long long)first,
                  (long long)(a.box_hi[d] + reach_hi[d]), d, (long long)a.dims[d]);
  }
  return 0;
}

// The fused kernels a sweep over arrays of these extents may use, deepest first.
// (single hull box => single-output programs, or outputs that share a window; the
// printer only emits them when that holds)
std::vector<int> eligible_fused(const Planner* plan, const int64_t* dims) {
  const soda_hip_program& p = plan->prog;
  std::vector<int> fused;
  for (size_t k = 0; k < plan->kernels.size(); ++k) {
    const soda_hip_kernel& kd = plan->kernels[k];
    if (kd.kind != SODA_HIP_KERNEL_FUSED ||
        (plan->max_depth > 0 && kd.depth > plan->max_depth))
      continue;
    // kernels without a guarded path: only arrays at least one tile large; the
    // 3-D ones index inside a plane with 32 bits (2-D ones are 64-bit throughout)
    if (kd.min_extent[0] > 0 &&
        (dims[0] < kd.min_extent[0] || (p.dim > 1 && dims[1] < kd.min_extent[1]) ||
         // (a lane that must not store gets byte offset 0xfffffff0 in the plane's
         // buffer resource: the plane must end below that, widest store included)
         (p.dim > 2 && dims[0] * dims[1] >= (int64_t(1) << 30) - 16)))
      continue;
    fused.push_back((int)k);
  }
  // (stable: same-depth alternatives keep the order of the table)
  std::stable_sort(fused.begin(), fused.end(), [&](int a, int b) {
    return plan->kernels[a].depth > plan->kernels[b].depth;
  });
  return fused;
}

// whether the sweep runs the fused kernels at all (otherwise: one launch per stage)
bool plans_fused(const Planner* plan, const std::vector<int>& fused, const int64_t* dims,
                 int iterate) {
  if (fused.empty() || plan->kernels[fused.back()].depth != 1) return false;
  if (plan->max_depth < 0) return false;  // force per-stage kernels
  if (plan->max_depth == 0 && !plan->tuning &&
      (takes_output_extras(plan, plan->kernels[fused.back()]) || plan->prog.dim == 1)) {
    // The fused kernels over several fields have not been timed on an MI355X yet
    // (profiles/r07_fields.txt, r07_fields3d.txt), so no depth of theirs has earned its place in the default
    // schedule: they run where the caller asks for them, with a depth limit
    // (soda_hip_plan_set_max_depth > 0) or a split (soda_hip_plan_set_split, _tune).
    // The same holds for the fused kernels of 1-D programs (kernel_stream1d.py;
    // profiles/r10_stream1d.txt): admitting a depth of theirs to the default schedule is a
    // change of its own.
    return plan->tuned_split.find(split_key(plan, dims, iterate)) != plan->tuned_split.end();
  }
  return true;
}

// the box of level `level` - the intersection of the outputs' boxes - on arrays whose inputs
// all carry the margins vlo / vhi and, beyond them, what the composition `g` starts from
soda_hip_args box_of_level(Planner* plan, Growth* g, const int64_t* dims, const int32_t* vlo,
                           const int32_t* vhi, int level, int32_t* mlo, int32_t* mhi) {
  const soda_hip_program& p = plan->prog;
  soda_hip_args a;
  memset(&a, 0, sizeof a);
  hull_margins(plan, g, level, mlo, mhi);
  for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) {
    a.dims[d] = d < p.dim ? dims[d] : 1;
    a.box_lo[d] = d < p.dim ? vlo[d] + mlo[d] : 0;
    a.box_hi[d] = d < p.dim ? dims[d] - vhi[d] - mhi[d] : 1;
  }
  return a;
}

// Split of `iterate` into the available depths: the cheapest one under the
// cost model (make_launch prices every depth on the first box it would run
// on; boxes shrink slowly, the ranking holds along the sweep), e.g. jacobi2d
// x100 = 5 x depth 20 rather than 4 x depth 24 + a memory-bound depth-4 tail.
// Kernels without cost figures: greedy, deepest first.  A split the tuner or the
// caller fixed for these arguments (Planner::tuned_split) goes before both.
int split_iterate(Planner* plan, Growth* g, const std::vector<int>& fused, const int64_t* dims,
                  int iterate, const int32_t* vlo, const int32_t* vhi, std::vector<int>* seq) {
  std::vector<int> usable;
  std::vector<double> price;
  bool priced = true;
  for (int k : fused) {
    if (plan->kernels[k].depth > iterate) continue;
    Launch l;
    bool empty = false;
    int32_t mlo[SODA_HIP_MAX_DIMS], mhi[SODA_HIP_MAX_DIMS];
    int rc = make_launch(plan, k, box_of_level(plan, g, dims, vlo, vhi, plan->kernels[k].depth,
                                               mlo, mhi), &l, &empty);
    if (rc) return rc;
    if (plan->bias_depth == plan->kernels[k].depth) l.est_us *= plan->bias;
    if (!empty && l.est_us <= 0) priced = false;
    usable.push_back(k);
    price.push_back(empty ? kModelLaunchUs : l.est_us);
  }
  if (usable.empty()) return fail(SODA_HIP_ERR_INTERNAL, "no fused kernel of depth 1");
  seq->clear();
  const auto tuned = plan->tuned_split.find(split_key(plan, dims, iterate));
  if (!plan->tuning && tuned != plan->tuned_split.end()) {
    // the split that ran fastest here (soda_hip_plan_tune): depth -> the first
    // usable kernel of that depth (same-depth alternatives are chosen per launch,
    // as always)
    for (int depth : tuned->second)
      for (int k : usable)
        if (plan->kernels[k].depth == depth) { seq->push_back(k); break; }
    int total = 0;
    for (int k : *seq) total += plan->kernels[k].depth;
    if (total != iterate) seq->clear();     // kernels changed since: fall back
  }
  if (!seq->empty()) {
  } else if (priced) {
    std::vector<double> best(iterate + 1, 1e300);
    std::vector<int> pick(iterate + 1, -1);
    best[0] = 0;
    for (int t = 1; t <= iterate; ++t)
      for (size_t i = 0; i < usable.size(); ++i) {
        const int d = plan->kernels[usable[i]].depth;
        // (<: among equal prices the deeper kernel, listed first, wins)
        if (d <= t && best[t - d] + price[i] < best[t]) {
          best[t] = best[t - d] + price[i];
          pick[t] = (int)i;
        }
      }
    for (int t = iterate; t > 0; t -= plan->kernels[usable[pick[t]]].depth) {
      if (pick[t] < 0) return fail(SODA_HIP_ERR_INTERNAL, "no fused kernel of depth 1");
      seq->push_back(usable[pick[t]]);
    }
    std::sort(seq->begin(), seq->end(), [&](int a, int b) {
      return plan->kernels[a].depth > plan->kernels[b].depth;
    });
  } else {
    for (int left = iterate; left > 0;) {
      int pick = -1;
      for (int k : usable)
        if (plan->kernels[k].depth <= left) { pick = k; break; }
      if (pick < 0) return fail(SODA_HIP_ERR_INTERNAL, "no fused kernel of depth 1");
      seq->push_back(pick);
      left -= plan->kernels[pick].depth;
    }
  }
  if (tuning_env("SODA_HIP_DEBUG")) {
    fprintf(stderr, "soda_hip: %d iteration(s) =", iterate);
    for (int k : *seq) fprintf(stderr, " %d", plan->kernels[k].depth);
    fprintf(stderr, "  (%s;", priced ? "cost model" : "greedy");
    for (size_t i = 0; i < usable.size(); ++i)
      fprintf(stderr, " k%d %.1f us", plan->kernels[usable[i]].depth, price[i]);
    fprintf(stderr, ")\n");
  }
  return 0;
}

// Where step i of a sweep's m steps writes its outputs.  Destinations alternate so
// that the last one is `out`; out_final_only: the m - 1 steps before the last alternate
// between the plan's two arrays and never touch `out` (two of them need the second one).
Buffer::Kind destination(const Planner* plan, int i, int m, ScratchNeeds* needs) {
  const bool even = ((m - 1 - i) % 2) == 0;     // steps left after this one
  Buffer::Kind to = even ? Buffer::OUTPUT : Buffer::ARRAY_A;
  if (plan->out_final_only)
    to = i == m - 1 ? Buffer::OUTPUT : m > 2 && even ? Buffer::ARRAY_B : Buffer::ARRAY_A;
  needs->pingpong |= to == Buffer::ARRAY_A;
  needs->second |= to == Buffer::ARRAY_B;
  return to;
}

// the tensors of step i of m: the inputs are what the step before wrote (`src`, which
// moves on to this step's outputs when the program feeds output j back into input j)
void route(const Planner* plan, int i, int m, std::vector<Buffer>* src, Buffer* tensor,
           ScratchNeeds* needs) {
  const soda_hip_program& p = plan->prog;
  const Buffer::Kind to = destination(plan, i, m, needs);
  for (int j = 0; j < p.n_inputs; ++j) tensor[j] = (*src)[j];
  for (int j = 0; j < p.n_outputs; ++j) {
    tensor[p.output_tensor[j]].kind = to;
    tensor[p.output_tensor[j]].index = (uint8_t)j;
    if (p.n_inputs == p.n_outputs) (*src)[j] = tensor[p.output_tensor[j]];
  }
}

std::vector<Buffer> sweep_inputs(const Planner* plan) {
  std::vector<Buffer> src(plan->prog.n_inputs);
  for (int j = 0; j < plan->prog.n_inputs; ++j) {
    src[j].kind = Buffer::INPUT;
    src[j].index = (uint8_t)j;
  }
  return src;
}

// every output on ITS box of level `level`, as extras against the hull `a`
int pack_output_extras(const Planner* plan, const Growth* g, const soda_hip_kernel& desc,
                       int level, const int32_t* mlo, const int32_t* mhi, soda_hip_args* a) {
  const soda_hip_program& p = plan->prog;
  const int dim = p.dim;
  if (p.n_outputs > max_extra_outputs(dim))
    return fail(SODA_HIP_ERR_INTERNAL, "kernel %s: %d outputs, the launch arguments "
                "carry the boxes of %d", desc.name, p.n_outputs, max_extra_outputs(dim));
  const std::vector<Box>& boxes = g->boxes[level - 1];
  for (int j = 0; j < p.n_outputs; ++j) {
    const Box& o = boxes[p.output_tensor[j]];
    int64_t ex[6];
    soda_hip_args own = *a;      // the widened box must lie inside the array as well
    for (int d = 0; d < dim; ++d) {
      ex[d] = mlo[d] + o.lo[d];
      ex[dim + d] = mhi[d] - o.hi[d];
      if (ex[d] < 0 || ex[d] > kMaxExtra || ex[dim + d] < 0 || ex[dim + d] > kMaxExtra)
        return fail(SODA_HIP_ERR_INTERNAL, "kernel %s: output %d is %lld / %lld cells "
                    "wider than the launch's box in dimension %d (limit %d)", desc.name,
                    j, (long long)ex[d], (long long)ex[dim + d], d, kMaxExtra);
      own.box_lo[d] -= ex[d];
      own.box_hi[d] += ex[dim + d];
    }
    const int32_t none[SODA_HIP_MAX_DIMS] = {0, 0, 0, 0};
    int rc = check_box_inside(plan, own, none, none);
    if (rc) return rc;
    uint64_t word = 0;
    for (int i = 0; i < 2 * dim; ++i) word |= (uint64_t)ex[i] << (8 * i);
    if (dim == 1) a->param[1 + j / 4] |= (int64_t)(word << (16 * (j % 4)));
    else if (dim == 2) a->param[1 + j / 2] |= (int64_t)(word << (32 * (j % 2)));
    else a->param[1 + j] = (int64_t)word;
  }
  return 0;
}

// the launches of the split `seq` (kernel indices, one per step)
int fused_list(Planner* plan, Growth* g, const std::vector<int>& fused, const std::vector<int>& seq,
               const int64_t* dims, const int32_t* vlo, const int32_t* vhi,
               std::vector<Launch>* list, int* max_depth_used, ScratchNeeds* needs) {
  const int m = (int)seq.size();
  int done = 0;
  int iterate = 0, form = 0;
  for (int k : seq) iterate += plan->kernels[k].depth;
  const auto tuned_form = plan->tuned_form.find(split_key(plan, dims, iterate));
  if (tuned_form != plan->tuned_form.end()) form = tuned_form->second;
  std::vector<Buffer> src = sweep_inputs(plan);
  for (int i = 0; i < m; ++i) {
    const soda_hip_kernel& desc = plan->kernels[seq[i]];
    Buffer tensor[SODA_HIP_MAX_TENSORS];
    route(plan, i, m, &src, tensor, needs);
    int32_t mlo[SODA_HIP_MAX_DIMS], mhi[SODA_HIP_MAX_DIMS];
    int32_t plo[SODA_HIP_MAX_DIMS], phi[SODA_HIP_MAX_DIMS];
    hull_margins(plan, g, done, plo, phi);
    soda_hip_args a = box_of_level(plan, g, dims, vlo, vhi, done + desc.depth, mlo, mhi);
    int32_t reach_lo[SODA_HIP_MAX_DIMS], reach_hi[SODA_HIP_MAX_DIMS];
    for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) {
      reach_lo[d] = mlo[d] - plo[d];
      reach_hi[d] = mhi[d] - phi[d];
    }
    int rc = check_box_inside(plan, a, reach_lo, reach_hi);
    if (rc) return rc;
    if (takes_output_extras(plan, desc)) {
      rc = pack_output_extras(plan, g, desc, done + desc.depth, mlo, mhi, &a);
      if (rc) return rc;
    }
    Launch l;
    bool empty;
    rc = make_launch(plan, seq[i], a, &l, &empty);
    if (rc) return rc;
    // several kernels of this depth (3-D: the wave-pipelined form with 64 x 32
    // tiles and the block form with 128 x 64 ones): the cheapest on THIS box -
    // large boxes favour the big tiles, small ones the many small ones
    if (!empty && l.est_us > 0) {
      // (tuning: SODA_HIP_PREFER=<suffix> takes the same-depth kernel whose name
      // ends in it whatever the estimates say - tools/ compare kernel forms with it)
      const char* prefer = tuning_env("SODA_HIP_PREFER");
      auto preferred = [&](int k) {
        if (!prefer) return false;
        const size_t n = strlen(plan->kernels[k].name), m = strlen(prefer);
        return n >= m && strcmp(plan->kernels[k].name + n - m, prefer) == 0;
      };
      // (a price from the model and one from measured step times do not compare: a kernel
      // without a calibration record never displaces one that has its own, and yields to it
      // - 2-D: the 12-column-lane kernels `k<d>w` next to the shipped `k<d>`)
      auto measured = [&](int k) {
        return plan->kernels[k].step_ns_full > 0 && plan->kernels[k].step_ns_one > 0;
      };
      // (soda_hip_plan_tune timed the sweep by price, with the first and with the last
      // kernel of every depth: Planner::tuned_form)
      int first = -1, last = -1;
      for (int k : fused)
        if (plan->kernels[k].depth == desc.depth) {
          if (first < 0) first = k;
          last = k;
        }
      const int forced = form == 1 ? first : form == 2 ? last : -1;
      for (int k : fused) {
        if (k == seq[i] || plan->kernels[k].depth != desc.depth) continue;
        Launch other;
        bool other_empty;
        if (make_launch(plan, k, a, &other, &other_empty) != 0 || other_empty ||
            other.est_us <= 0)
          continue;
        if (forced >= 0 && !prefer) {
          if (k == forced) l = other;
          continue;
        }
        const bool cheaper = measured(k) != measured(l.kernel) ? measured(k)
                                                               : other.est_us < l.est_us;
        if (preferred(k) || (cheaper && !preferred(l.kernel))) l = other;
      }
    }
    std::copy(tensor, tensor + SODA_HIP_MAX_TENSORS, l.buffer);
    if (!empty) list->push_back(l);
    *max_depth_used = std::max(*max_depth_used, (int)desc.depth);
    done += desc.depth;
  }
  return 0;
}

// per-stage kernels: one launch per stage per iteration, intermediates in HBM
int staged_list(Planner* plan, const Growth* g, const int64_t* dims, int iterate, const int32_t* vlo,
                const int32_t* vhi, std::vector<Launch>* list, int* max_depth_used,
                ScratchNeeds* needs) {
  const soda_hip_program& p = plan->prog;
  std::vector<int> stage_kernel(p.n_stages, -1);
  for (size_t k = 0; k < plan->kernels.size(); ++k)
    if (plan->kernels[k].kind == SODA_HIP_KERNEL_STAGE) {
      const int s = plan->kernels[k].stage - p.n_inputs;
      if (s >= 0 && s < p.n_stages) stage_kernel[s] = (int)k;
    }
  for (int s = 0; s < p.n_stages; ++s)
    if (stage_kernel[s] < 0)
      return fail(SODA_HIP_ERR_NO_KERNEL, "blob has no kernel for stage %d", s);
  std::vector<Buffer> src = sweep_inputs(plan);
  for (int it = 0; it < iterate; ++it) {
    Buffer tensor[SODA_HIP_MAX_TENSORS];
    for (int s = 0; s < p.n_stages; ++s) {
      if (is_output_tensor(p, p.n_inputs + s)) continue;
      tensor[p.n_inputs + s].kind = Buffer::LOCAL;
      tensor[p.n_inputs + s].index = (uint8_t)s;
      needs->locals = true;
    }
    route(plan, it, iterate, &src, tensor, needs);
    soda_hip_args a;
    memset(&a, 0, sizeof a);
    for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) a.dims[d] = d < p.dim ? dims[d] : 1;
    for (int s = 0; s < p.n_stages; ++s) {
      const Box& b = g->boxes[it][p.n_inputs + s];
      for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) {
        a.box_lo[d] = d < p.dim ? vlo[d] - b.lo[d] : 0;
        a.box_hi[d] = d < p.dim ? dims[d] - vhi[d] - b.hi[d] : 1;
      }
      // everything the stage reads must be inside the array
      for (int w = 0; w < p.n_windows; ++w) {
        if (p.window[w].stage != p.n_inputs + s) continue;
        int rc = check_box_inside(plan, a, p.window[w].lo, p.window[w].hi, true);
        if (rc) return rc;
      }
      Launch l;
      bool empty;
      int rc = make_launch(plan, stage_kernel[s], a, &l, &empty);
      if (rc) return rc;
      std::copy(tensor, tensor + SODA_HIP_MAX_TENSORS, l.buffer);
      if (!empty) list->push_back(l);
    }
  }
  *max_depth_used = 1;
  return 0;
}

}  // namespace

int build_schedule_fields(Planner* plan, const int64_t* dims, int iterate,
                          const int32_t (*valid_lo)[SODA_HIP_MAX_DIMS],
                          const int32_t (*valid_hi)[SODA_HIP_MAX_DIMS],
                          std::vector<Launch>* list, int* max_depth_used, ScratchNeeds* needs) {
  const soda_hip_program& p = plan->prog;
  if (iterate < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "iterate must be >= 1");
  if (iterate > 1 && p.n_inputs != p.n_outputs)
    return fail(SODA_HIP_ERR_CONSTRAINT,
                "iterate > 1 needs as many outputs as inputs (%d vs %d)",
                p.n_inputs, p.n_outputs);
  // The margins every input shares move the boxes as a whole (vlo / vhi: all there is
  // when one margin holds for every input); what an input's region lacks beyond them is
  // where the composition starts for it.
  int32_t vlo[SODA_HIP_MAX_DIMS] = {0, 0, 0, 0}, vhi[SODA_HIP_MAX_DIMS] = {0, 0, 0, 0};
  std::vector<int32_t> beyond;      // per input: lo of every dimension, then hi
  for (int d = 0; d < p.dim; ++d) {
    if (dims[d] <= 0) return fail(SODA_HIP_ERR_CONSTRAINT, "dims[%d] = %lld", d,
                                  (long long)dims[d]);
    for (int j = 0; j < p.n_inputs; ++j) {
      const int32_t lo = valid_lo ? valid_lo[j][d] : 0, hi = valid_hi ? valid_hi[j][d] : 0;
      vlo[d] = j ? std::min(vlo[d], lo) : lo;
      vhi[d] = j ? std::min(vhi[d], hi) : hi;
    }
  }
  bool uniform = true;
  for (int j = 0; j < p.n_inputs; ++j)
    for (int side = 0; side < 2; ++side)
      for (int d = 0; d < p.dim; ++d) {
        const int32_t* v = side ? (valid_hi ? valid_hi[j] : nullptr)
                                : (valid_lo ? valid_lo[j] : nullptr);
        beyond.push_back((v ? v[d] : 0) - (side ? vhi[d] : vlo[d]));
        uniform = uniform && beyond.back() == 0;
      }
  Growth* g = &plan->fresh;
  if (!uniform) {
    g = &plan->resumed[beyond];
    if (g->start.empty()) {
      g->start.assign(p.n_inputs, Box{});
      for (int j = 0; j < p.n_inputs; ++j)
        for (int d = 0; d < p.dim; ++d) {
          g->start[j].lo[d] = -beyond[(2 * j) * p.dim + d];
          g->start[j].hi[d] = beyond[(2 * j + 1) * p.dim + d];
        }
    }
  }
  grow_boxes(plan, g, iterate);
  list->clear();
  *max_depth_used = 0;
  *needs = ScratchNeeds{};
  const std::vector<int> fused = eligible_fused(plan, dims);
  if (!plans_fused(plan, fused, dims, iterate))
    return staged_list(plan, g, dims, iterate, vlo, vhi, list, max_depth_used, needs);
  std::vector<int> seq;
  int rc = split_iterate(plan, g, fused, dims, iterate, vlo, vhi, &seq);
  if (rc) return rc;
  return fused_list(plan, g, fused, seq, dims, vlo, vhi, list, max_depth_used, needs);
}

// one margin for every input
int build_schedule(Planner* plan, const int64_t* dims, int iterate, const int32_t* valid_lo,
                   const int32_t* valid_hi, std::vector<Launch>* list, int* max_depth_used,
                   ScratchNeeds* needs) {
  int32_t lo[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS], hi[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS];
  for (int j = 0; j < SODA_HIP_MAX_IO; ++j)
    for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d) {
      lo[j][d] = valid_lo && d < plan->prog.dim ? valid_lo[d] : 0;
      hi[j][d] = valid_hi && d < plan->prog.dim ? valid_hi[d] : 0;
    }
  return build_schedule_fields(plan, dims, iterate, lo, hi, list, max_depth_used, needs);
}
