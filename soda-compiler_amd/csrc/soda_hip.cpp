// libsoda_hip.so -- run-time of the SODA HIP back end for MI355X (gfx950).
//
// Thin and stateless per call apart from the handles it hands out: a module
// (one code object), a plan (program + kernels + scratch memory).  The stencil
// arithmetic lives in the generated kernels (soda_hip/codegen/kernel_*.py); this
// planner (schedule.cpp) decides which kernel runs on which box with which buffers;
// this file owns the modules and the plans' device memory, binds the buffers, launches
// on the caller's stream and times with hipEvents.  The multi-GPU driver is slab.cpp.
//
// Reference counterparts are cited per function in include/soda_hip.h.
#include "plan.h"

#include <hip/hiprtc.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

// a plan-owned array of at least `bytes`, zeroed when it is (re)allocated
int grow_zeroed(void** array, size_t* have, size_t bytes, hipStream_t stream) {
  if (*have >= bytes) return 0;
  if (*array) {
    HIP_TRY(SODA_HIP_ERR_DEVICE_FREE, hipFree(*array));
    *array = nullptr;
    *have = 0;
  }
  HIP_TRY(SODA_HIP_ERR_DEVICE_MALLOC, hipMalloc(array, bytes));
  // unspecified cells must at least be readable, finite-ish garbage: zero.
  // On the sweep's own stream: a null-stream memset is not ordered before
  // kernels on a non-blocking stream and could clobber their results.
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN, hipMemsetAsync(*array, 0, bytes, stream));
  *have = bytes;
  return 0;
}

int ensure_scratch(soda_hip_plan* plan, const int64_t* dims, const ScratchNeeds& needs,
                   hipStream_t stream) {
  const soda_hip_program& p = plan->prog;
  size_t cells = 1;
  for (int d = 0; d < p.dim; ++d) cells *= (size_t)dims[d];
  for (int j = 0; j < p.n_outputs && needs.pingpong; ++j) {
    int rc = grow_zeroed(&plan->scratch[j], &plan->scratch_bytes[j],
                         cells * p.elem_size[p.output_tensor[j]], stream);
    if (rc) return rc;
  }
  for (int j = 0; j < p.n_outputs && needs.second; ++j) {
    int rc = grow_zeroed(&plan->scratch_b[j], &plan->scratch_b_bytes[j],
                         cells * p.elem_size[p.output_tensor[j]], stream);
    if (rc) return rc;
  }
  for (int s = 0; s < p.n_stages && needs.locals; ++s) {
    const int t = p.n_inputs + s;
    if (is_output_tensor(p, t)) continue;
    int rc = grow_zeroed(&plan->scratch[p.n_outputs + s], &plan->scratch_bytes[p.n_outputs + s],
                         cells * p.elem_size[t], stream);
    if (rc) return rc;
  }
  return 0;
}

void* resolve(const soda_hip_plan* plan, Buffer b, void* const* in, void* const* out) {
  switch (b.kind) {
    case Buffer::INPUT: return in[b.index];
    case Buffer::OUTPUT: return out[b.index];
    case Buffer::ARRAY_A: return plan->scratch[b.index];
    case Buffer::ARRAY_B: return plan->scratch_b[b.index];
    case Buffer::LOCAL: return plan->scratch[plan->prog.n_outputs + b.index];
    case Buffer::NONE: break;
  }
  return nullptr;
}

// The launch list of one sweep over the caller's arrays, ready to launch: planned,
// the plan-owned arrays it names allocated (and zeroed on `stream`), buffers bound.
int bound_schedule(soda_hip_plan* plan, void* const* in, void* const* out,
                   const int64_t* dims, int iterate,
                   const int32_t (*valid_lo)[SODA_HIP_MAX_DIMS],
                   const int32_t (*valid_hi)[SODA_HIP_MAX_DIMS], std::vector<Launch>* list,
                   int* max_depth_used, hipStream_t stream) {
  const soda_hip_program& p = plan->prog;
  for (int j = 0; j < p.n_inputs; ++j)
    if (!in[j]) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "input %d is NULL", j);
  for (int j = 0; j < p.n_outputs; ++j)
    if (!out[j]) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "output %d is NULL", j);
  ScratchNeeds needs;
  int rc = build_schedule_fields(plan, dims, iterate, valid_lo, valid_hi, list, max_depth_used,
                                 &needs);
  if (rc) return rc;
  rc = ensure_scratch(plan, dims, needs, stream);
  if (rc) return rc;
  for (Launch& l : *list)
    for (int t = 0; t < n_tensors(p); ++t) l.args.tensor[t] = resolve(plan, l.buffer[t], in, out);
  return 0;
}

// one margin (NULL = none) as the margin of every input
struct Repeated {
  int32_t rows[SODA_HIP_MAX_IO][SODA_HIP_MAX_DIMS];
  Repeated(const soda_hip_plan* plan, const int32_t* margin) {
    for (int j = 0; j < SODA_HIP_MAX_IO; ++j)
      for (int d = 0; d < SODA_HIP_MAX_DIMS; ++d)
        rows[j][d] = margin && d < plan->prog.dim ? margin[d] : 0;
  }
};

int launch_one(const soda_hip_plan* plan, const Launch& l, hipStream_t stream) {
  const soda_hip_kernel& desc = plan->kernels[l.kernel];
  soda_hip_args args = l.args;
  size_t size = sizeof args;
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args,
                    HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN,
          hipModuleLaunchKernel(plan->funcs[l.kernel], l.grid[0], l.grid[1],
                                l.grid[2], desc.block[0], desc.block[1],
                                desc.block[2], l.lds_bytes, stream, nullptr, config));
  return 0;
}

// Streaming launches of the schedule (kernels that name a measured chunk, on boxes beyond
// the Infinity Cache): the calibrated (chunk, workgroups per CU) against the chunk's two
// neighbours on the calibration ladder and the other cap, each as a WHOLE sweep on this
// device; the fastest is kept per (kernel, box extents) when it beats the calibrated pair
// by more than 1 % (tools/calibrate.py measured those on one box; boxes differ).
template <typename TimeSweep>
int tune_streaming(soda_hip_plan* plan, const int64_t* dims, int iterate,
                   const int32_t* valid_lo, const int32_t* valid_hi, TimeSweep time_sweep) {
  if (plan->chunk_rows_override != 0 || plan->wgs_per_cu_cap != 0) return 0;
  std::vector<Launch> list;
  int depth = 0;
  ScratchNeeds needs;
  int rc = build_schedule(plan, dims, iterate, valid_lo, valid_hi, &list, &depth, &needs);
  if (rc) return rc;
  static const int ladder[] = {8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256};
  const int n_ladder = (int)(sizeof ladder / sizeof ladder[0]);
  std::vector<std::array<int64_t, 5>> seen;
  for (const Launch& l : list) {
    const soda_hip_kernel& desc = plan->kernels[l.kernel];
    if (desc.fill_rows <= 0 || desc.stream_chunk <= 0 ||
        footprint_of(plan, l.args) <= kBeyondCacheBytes)
      continue;
    const std::array<int64_t, 5> key = stream_key(plan, l.kernel, l.args);
    if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
    seen.push_back(key);
    plan->tuned_stream.erase(key);
    int at = 0;
    for (int i = 0; i < n_ladder; ++i)
      if (std::abs(ladder[i] - (int)desc.stream_chunk) < std::abs(ladder[at] - (int)desc.stream_chunk))
        at = i;
    const int cap0 = std::max(0, (int)desc.stream_wgs_per_cu);
    std::vector<std::array<int, 2>> candidates = {{(int)desc.stream_chunk, cap0}};
    for (int cap : {cap0, cap0 == 2 ? 0 : 2})
      for (int i : {at - 1, at, at + 1}) {
        if (i < 0 || i >= n_ladder) continue;
        const std::array<int, 2> c = {ladder[i], cap};
        if (std::find(candidates.begin(), candidates.end(), c) == candidates.end())
          candidates.push_back(c);
      }
    float incumbent = 0, best_ms = 0;
    size_t best = 0;
    for (size_t c = 0; c < candidates.size() && !rc; ++c) {
      if (c) plan->tuned_stream[key] = candidates[c];
      float ms = 0;
      rc = time_sweep(3, &ms);
      if (c == 0) incumbent = best_ms = ms;
      else if (ms < best_ms) { best_ms = ms; best = c; }
      if (tuning_env("SODA_HIP_DEBUG"))
        fprintf(stderr, "soda_hip: tune stream %s box %lld x %lld: chunk %d cap %d -> %.1f us\n",
                desc.name, (long long)key[1], (long long)key[2], candidates[c][0],
                candidates[c][1], ms * 1000.0);
    }
    if (!rc && best > 0 && best_ms < incumbent * 0.99f) plan->tuned_stream[key] = candidates[best];
    else plan->tuned_stream.erase(key);
  }
  return rc;
}

}  // namespace

extern "C" {

const char* soda_hip_error_name(int code) {
  switch (code) {
    case SODA_HIP_OK: return "ok";
    case SODA_HIP_ERR_GENERIC: return "generic_error";
    case SODA_HIP_ERR_BAD_ELEM_SIZE: return "bad_elem_size";
    case SODA_HIP_ERR_OUT_OF_BOUNDS: return "access_out_of_bounds";
    case SODA_HIP_ERR_EXTENTS_TOO_LARGE: return "buffer_extents_too_large";
    case SODA_HIP_ERR_CONSTRAINT: return "constraint_violated";
    case SODA_HIP_ERR_OUT_OF_MEMORY: return "out_of_memory";
    case SODA_HIP_ERR_NULL_ARGUMENT: return "buffer_argument_is_null";
    case SODA_HIP_ERR_COPY_TO_HOST: return "copy_to_host_failed";
    case SODA_HIP_ERR_COPY_TO_DEVICE: return "copy_to_device_failed";
    case SODA_HIP_ERR_DEVICE_MALLOC: return "device_malloc_failed";
    case SODA_HIP_ERR_DEVICE_SYNC: return "device_sync_failed";
    case SODA_HIP_ERR_DEVICE_FREE: return "device_free_failed";
    case SODA_HIP_ERR_NO_DEVICE: return "no_device_interface";
    case SODA_HIP_ERR_INTERNAL: return "internal_error";
    case SODA_HIP_ERR_DEVICE_RUN: return "device_run_failed";
    case SODA_HIP_ERR_COMPILE: return "kernel_compile_failed";
    case SODA_HIP_ERR_MODULE: return "bad_code_object";
    case SODA_HIP_ERR_NO_KERNEL: return "kernel_not_found";
    case SODA_HIP_ERR_MISMATCH: return "blob_program_mismatch";
    default: return "unknown_error";
  }
}

const char* soda_hip_last_error(void) { return g_last_error.c_str(); }
int soda_hip_abi_version(void) { return SODA_HIP_ABI_VERSION; }

int soda_hip_device_count(int* count) {
  if (!count) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(SODA_HIP_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return 0;
}

int soda_hip_set_device(int ordinal) {
  HIP_TRY(SODA_HIP_ERR_NO_DEVICE, hipSetDevice(ordinal));
  return 0;
}

int soda_hip_device_info(int ordinal, char* name, size_t name_cap, int* cu,
                         uint64_t* total_mem_bytes) {
  hipDeviceProp_t prop;
  HIP_TRY(SODA_HIP_ERR_NO_DEVICE, hipGetDeviceProperties(&prop, ordinal));
  if (name && name_cap) snprintf(name, name_cap, "%s", prop.gcnArchName);
  if (cu) *cu = prop.multiProcessorCount;
  if (total_mem_bytes) *total_mem_bytes = prop.totalGlobalMem;
  return 0;
}

int soda_hip_malloc(void** dev, size_t bytes) {
  if (!dev) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "dev is NULL");
  HIP_TRY(SODA_HIP_ERR_DEVICE_MALLOC, hipMalloc(dev, bytes ? bytes : 1));
  return 0;
}

int soda_hip_free(void* dev) {
  if (dev) HIP_TRY(SODA_HIP_ERR_DEVICE_FREE, hipFree(dev));
  return 0;
}

int soda_hip_memset(void* dev, int value, size_t bytes, void* stream) {
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN, hipMemsetAsync(dev, value, bytes, as_stream(stream)));
  return 0;
}

int soda_hip_memcpy_h2d(void* dev, const void* host, size_t bytes, void* stream) {
  HIP_TRY(SODA_HIP_ERR_COPY_TO_DEVICE,
          hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, as_stream(stream)));
  return 0;
}

int soda_hip_memcpy_d2h(void* host, const void* dev, size_t bytes, void* stream) {
  HIP_TRY(SODA_HIP_ERR_COPY_TO_HOST,
          hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
  return 0;
}

int soda_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN,
          hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
  return 0;
}

int soda_hip_stream_synchronize(void* stream) {
  HIP_TRY(SODA_HIP_ERR_DEVICE_SYNC, hipStreamSynchronize(as_stream(stream)));
  return 0;
}

// ---------------------------------------------------------------- modules
static int finish_module(soda_hip_module* m, soda_hip_module** out) {
  hipError_t e = hipModuleLoadData(&m->mod, m->image.data());
  if (e != hipSuccess) {
    delete m;
    return fail(SODA_HIP_ERR_MODULE, "hipModuleLoadData: %s", hipGetErrorString(e));
  }
  hipDeviceptr_t ptr = nullptr;
  size_t bytes = 0;
  if (hipModuleGetGlobal(&ptr, &bytes, m->mod, "soda_hip_meta") == hipSuccess && bytes) {
    m->meta.resize(bytes);
    if (hipMemcpyDtoH(&m->meta[0], ptr, bytes) != hipSuccess) m->meta.clear();
    const size_t z = m->meta.find('\0');
    if (z != std::string::npos) m->meta.resize(z);
  }
  (void)hipGetLastError();
  *out = m;
  return 0;
}

int soda_hip_module_load_data(const void* image, size_t bytes, soda_hip_module** module) {
  if (!image || !module) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  soda_hip_module* m = new soda_hip_module;
  m->image.assign((const char*)image, (const char*)image + bytes);
  return finish_module(m, module);
}

int soda_hip_module_load_file(const char* path, soda_hip_module** module) {
  if (!path || !module) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  FILE* f = fopen(path, "rb");
  if (!f) return fail(SODA_HIP_ERR_MODULE, "cannot open %s", path);
  std::vector<char> data;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  if (data.empty()) return fail(SODA_HIP_ERR_MODULE, "%s is empty", path);
  return soda_hip_module_load_data(data.data(), data.size(), module);
}

int soda_hip_module_compile(const char* source, const char* arch,
                            const char* const* options, int n_options,
                            soda_hip_module** module) {
  if (!source || !module) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  std::string arch_flag = "--offload-arch=";
  if (arch && *arch) {
    arch_flag += arch;
  } else {
    int dev = 0;
    hipDeviceProp_t prop;
    HIP_TRY(SODA_HIP_ERR_NO_DEVICE, hipGetDevice(&dev));
    HIP_TRY(SODA_HIP_ERR_NO_DEVICE, hipGetDeviceProperties(&prop, dev));
    arch_flag += prop.gcnArchName;
  }
  std::vector<const char*> opts = {arch_flag.c_str(), "-O3", "-ffp-contract=off",
                                   "-std=c++17"};
  for (int i = 0; i < n_options; ++i) opts.push_back(options[i]);
  hiprtcProgram prog;
  hiprtcResult r = hiprtcCreateProgram(&prog, source, "soda_kernel.hip", 0, nullptr, nullptr);
  if (r != HIPRTC_SUCCESS)
    return fail(SODA_HIP_ERR_COMPILE, "hiprtcCreateProgram: %s", hiprtcGetErrorString(r));
  r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
  if (r != HIPRTC_SUCCESS) {
    size_t log_size = 0;
    hiprtcGetProgramLogSize(prog, &log_size);
    std::string log(log_size, '\0');
    if (log_size) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    return fail(SODA_HIP_ERR_COMPILE, "hiprtc: %s\n%.900s", hiprtcGetErrorString(r),
                log.c_str());
  }
  size_t code_size = 0;
  hiprtcGetCodeSize(prog, &code_size);
  soda_hip_module* m = new soda_hip_module;
  m->image.resize(code_size);
  hiprtcGetCode(prog, m->image.data());
  hiprtcDestroyProgram(&prog);
  return finish_module(m, module);
}

int soda_hip_module_image(const soda_hip_module* module, const void** image, size_t* bytes) {
  if (!module || !image || !bytes) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  *image = module->image.data();
  *bytes = module->image.size();
  return 0;
}

int soda_hip_module_meta(const soda_hip_module* module, char* buf, size_t cap, size_t* length) {
  if (!module) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "module is NULL");
  if (length) *length = module->meta.size();
  if (buf && cap) {
    const size_t n = std::min(cap - 1, module->meta.size());
    memcpy(buf, module->meta.data(), n);
    buf[n] = '\0';
  }
  return 0;
}

int soda_hip_module_unload(soda_hip_module* module) {
  if (!module) return 0;
  if (module->mod) HIP_TRY(SODA_HIP_ERR_MODULE, hipModuleUnload(module->mod));
  delete module;
  return 0;
}

// ------------------------------------------------------------------ plans
int soda_hip_plan_create(soda_hip_module* module, const soda_hip_program* program,
                         const soda_hip_kernel* kernels, int n_kernels,
                         soda_hip_plan** plan) {
  if (!module || !program || !kernels || !plan)
    return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  const soda_hip_program& p = *program;
  if (p.dim < 1 || p.dim > SODA_HIP_MAX_DIMS)
    return fail(SODA_HIP_ERR_CONSTRAINT, "dim %d not supported (1..%d)", p.dim,
                SODA_HIP_MAX_DIMS);
  if (p.n_inputs < 1 || p.n_stages < 1 || p.n_outputs < 1 ||
      p.n_inputs + p.n_stages > SODA_HIP_MAX_TENSORS || p.n_outputs > SODA_HIP_MAX_IO ||
      p.n_inputs > SODA_HIP_MAX_IO || p.n_windows < 1 || p.n_windows > SODA_HIP_MAX_WINDOWS)
    return fail(SODA_HIP_ERR_CONSTRAINT, "program descriptor out of range");
  if (n_kernels < 1 || n_kernels > SODA_HIP_MAX_KERNELS)
    return fail(SODA_HIP_ERR_CONSTRAINT, "n_kernels %d out of range", n_kernels);
  for (int j = 0; j < p.n_outputs; ++j)
    if (p.output_tensor[j] < p.n_inputs || p.output_tensor[j] >= p.n_inputs + p.n_stages)
      return fail(SODA_HIP_ERR_CONSTRAINT, "output %d is not a stage", j);
  for (int w = 0; w < p.n_windows; ++w) {
    const soda_hip_window& win = p.window[w];
    if (win.stage < p.n_inputs || win.stage >= p.n_inputs + p.n_stages ||
        win.parent < 0 || win.parent >= win.stage)
      return fail(SODA_HIP_ERR_CONSTRAINT, "window %d breaks execution order", w);
  }
  soda_hip_plan* pl = new soda_hip_plan;
  pl->module = module;
  pl->prog = p;
  pl->kernels.assign(kernels, kernels + n_kernels);
  pl->funcs.resize(n_kernels);
  pl->scratch.assign(p.n_outputs + p.n_stages, nullptr);
  pl->scratch_bytes.assign(p.n_outputs + p.n_stages, 0);
  pl->scratch_b.assign(p.n_outputs, nullptr);
  pl->scratch_b_bytes.assign(p.n_outputs, 0);
  for (int k = 0; k < n_kernels; ++k) {
    pl->kernels[k].name[sizeof(pl->kernels[k].name) - 1] = '\0';
    hipError_t e = hipModuleGetFunction(&pl->funcs[k], module->mod, pl->kernels[k].name);
    if (e != hipSuccess) {
      std::string name = pl->kernels[k].name;
      delete pl;
      return fail(SODA_HIP_ERR_NO_KERNEL, "kernel `%s` is not in the blob: %s",
                  name.c_str(), hipGetErrorString(e));
    }
    {
      // occupancy of this kernel on this device (MI355X_MICROARCH.md, register
      // files: 512 VGPRs per lane per SIMD, granule 8, at most 8 waves per SIMD)
      int regs = 0, dev = 0, cus = 256;
      (void)hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, pl->funcs[k]);
      hipDeviceProp_t prop;
      memset(&prop, 0, sizeof prop);
      if (hipGetDevice(&dev) == hipSuccess &&
          hipGetDeviceProperties(&prop, dev) == hipSuccess)
        cus = prop.multiProcessorCount;
      const int alloc = std::max(8, (regs + 7) / 8 * 8);
      const int waves_per_simd = std::max(1, std::min(8, 512 / alloc));
      const int threads = pl->kernels[k].block[0] * pl->kernels[k].block[1] *
                          pl->kernels[k].block[2];
      const int waves_per_block = std::max(1, (threads + 63) / 64);
      int per_cu = 4 * waves_per_simd / waves_per_block;
      // the runtime's own answer also knows the kernel's LDS and SGPR use
      int api = 0;
      if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(
              &api, pl->funcs[k], threads, 0) == hipSuccess && api > 0)
        per_cu = api;
      if (tuning_env("SODA_HIP_DEBUG"))
        fprintf(stderr, "soda_hip: kernel %s: %d VGPRs, %d workgroup(s) of %d "
                "wavefronts per CU\n", pl->kernels[k].name, regs, per_cu,
                waves_per_block);
      pl->resident_blocks.push_back(std::max(1, cus * per_cu));
      pl->cus = cus;
      int lds = 0;
      (void)hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, pl->funcs[k]);
      pl->static_lds.push_back(std::max(0, lds));
      // (gfx950 has 160 KiB per CU; a runtime that reports the per-workgroup limit of
      // older parts here must not loosen the cap)
      pl->lds_per_cu = std::max<int64_t>(160 * 1024,
                                         (int64_t)prop.maxSharedMemoryPerMultiProcessor);
      if (tuning_env("SODA_HIP_DEBUG"))
        fprintf(stderr, "soda_hip: kernel %s: %d bytes of static LDS; device reports %lld "
                "bytes of LDS per CU\n", pl->kernels[k].name, lds,
                (long long)prop.maxSharedMemoryPerMultiProcessor);
    }
    const soda_hip_kernel& d = pl->kernels[k];
    if (d.block[0] < 1 || d.block[1] < 1 || d.block[2] < 1 ||
        (int64_t)d.block[0] * d.block[1] * d.block[2] > 1024) {
      delete pl;
      return fail(SODA_HIP_ERR_CONSTRAINT, "kernel %d has a bad block shape", k);
    }
  }
  if (const char* env = tuning_env("SODA_HIP_CHUNK_ROWS")) pl->chunk_rows_override = atoi(env);
  if (const char* env = tuning_env("SODA_HIP_WGS_PER_CU")) pl->wgs_per_cu_cap = atoi(env);
  if (const char* env = tuning_env("SODA_HIP_CHUNK_MIN"))
    pl->chunk_rows_min = std::max(4, atoi(env));
  *plan = pl;
  return 0;
}

int soda_hip_plan_destroy(soda_hip_plan* plan) {
  if (!plan) return 0;
  int rc = 0;
  for (void* ptr : plan->scratch)
    if (ptr && hipFree(ptr) != hipSuccess)
      rc = fail(SODA_HIP_ERR_DEVICE_FREE, "hipFree of plan scratch failed");
  for (void* ptr : plan->scratch_b)
    if (ptr && hipFree(ptr) != hipSuccess)
      rc = fail(SODA_HIP_ERR_DEVICE_FREE, "hipFree of plan scratch failed");
  if (plan->probe_buf) (void)hipFree(plan->probe_buf);
  if (plan->probe_t0) (void)hipEventDestroy(plan->probe_t0);
  if (plan->probe_t1) (void)hipEventDestroy(plan->probe_t1);
  if (plan->ev_main) (void)hipEventDestroy(plan->ev_main);
  if (plan->ev_landed) (void)hipEventDestroy(plan->ev_landed);
  if (plan->side) (void)hipStreamDestroy(plan->side);
  delete plan;
  return rc;
}

int soda_hip_plan_margins(const soda_hip_plan* plan, int iterations,
                          int32_t lo[SODA_HIP_MAX_DIMS], int32_t hi[SODA_HIP_MAX_DIMS]) {
  if (!plan || !lo || !hi) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (iterations < 0) return fail(SODA_HIP_ERR_CONSTRAINT, "iterations < 0");
  output_margins(const_cast<soda_hip_plan*>(plan), iterations, lo, hi);
  return 0;
}

int soda_hip_plan_field_margins(const soda_hip_plan* plan, int iterations,
                                int32_t (*lo)[SODA_HIP_MAX_DIMS],
                                int32_t (*hi)[SODA_HIP_MAX_DIMS]) {
  if (!plan || !lo || !hi) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (iterations < 0) return fail(SODA_HIP_ERR_CONSTRAINT, "iterations < 0");
  if (iterations > 1 && plan->prog.n_inputs != plan->prog.n_outputs)
    return fail(SODA_HIP_ERR_CONSTRAINT,
                "iterations > 1 need as many outputs as inputs (%d vs %d)",
                plan->prog.n_inputs, plan->prog.n_outputs);
  field_margins(const_cast<soda_hip_plan*>(plan), iterations, lo, hi);
  return 0;
}

int soda_hip_plan_set_max_depth(soda_hip_plan* plan, int max_depth) {
  if (!plan) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "plan is NULL");
  plan->max_depth = max_depth;
  return 0;
}

int soda_hip_plan_tune(soda_hip_plan* plan, void* const* in, void* const* out,
                       const int64_t dims[SODA_HIP_MAX_DIMS], int iterate,
                       const int32_t* valid_lo, const int32_t* valid_hi, void* stream) {
  if (!plan || !in || !out || !dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  hipStream_t s = as_stream(stream);
  const std::array<int64_t, 5> key = split_key(plan, dims, iterate);
  // candidate splits: the scheduler's own, and its answer when every deep kernel in
  // turn is made 12 % cheaper or dearer (the model ranks depths within a few percent
  // of each other; what really runs fastest depends on the device and the grid)
  std::vector<int> depths;
  for (const soda_hip_kernel& kd : plan->kernels)
    if (kd.kind == SODA_HIP_KERNEL_FUSED && kd.depth >= 4 && kd.depth <= iterate &&
        std::find(depths.begin(), depths.end(), kd.depth) == depths.end())
      depths.push_back(kd.depth);
  std::vector<std::vector<int>> candidates;
  plan->tuning = true;
  int rc = 0;
  for (int i = -1; i < 2 * (int)depths.size() && !rc; ++i) {
    plan->bias_depth = i < 0 ? 0 : depths[i / 2];
    plan->bias = i % 2 == 0 ? 0.88 : 1.12;
    std::vector<Launch> list;
    int depth = 0;
    ScratchNeeds needs;
    rc = build_schedule(plan, dims, iterate, valid_lo, valid_hi, &list, &depth, &needs);
    std::vector<int> split;
    for (const Launch& l : list)
      if (plan->kernels[l.kernel].kind == SODA_HIP_KERNEL_FUSED)
        split.push_back(plan->kernels[l.kernel].depth);
    int total = 0;
    for (int d : split) total += d;
    if (!rc && total == iterate &&
        std::find(candidates.begin(), candidates.end(), split) == candidates.end())
      candidates.push_back(split);
  }
  plan->bias_depth = 0;
  plan->bias = 1.0;
  plan->tuning = false;
  if (rc) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventCreate failed");
  // the fastest of `runs` whole sweeps after one untimed one, in milliseconds
  auto time_sweep = [&](int runs, float* fastest) -> int {
    int e = 0;
    for (int run = 0; run <= runs && !e; ++run) {
      if (hipEventRecord(e0, s) != hipSuccess) e = fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventRecord failed");
      if (!e) e = soda_hip_sweep(plan, in, out, dims, iterate, valid_lo, valid_hi, stream);
      if (!e && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess))
        e = fail(SODA_HIP_ERR_DEVICE_SYNC, "timing a tuning sweep failed");
      float ms = 0;
      if (!e) (void)hipEventElapsedTime(&ms, e0, e1);
      if (run == 1 || (run > 1 && ms < *fastest)) *fastest = ms;
    }
    return e;
  };
  // depths with several kernels in the blob (the run-time takes the cheaper by price per
  // launch): the sweep by price, with the table's first and with its last kernel of every
  // depth, one untimed run and the faster of two timed ones each - the fastest stays
  // (Planner::tuned_form).  Only where the sweep has such a launch.
  auto tune_forms = [&]() -> int {
    std::vector<Launch> list;
    int depth = 0;
    ScratchNeeds needs;
    int e = build_schedule(plan, dims, iterate, valid_lo, valid_hi, &list, &depth, &needs);
    bool several = false;
    for (const Launch& l : list) {
      const soda_hip_kernel& kd = plan->kernels[l.kernel];
      if (kd.kind != SODA_HIP_KERNEL_FUSED) continue;
      for (size_t k = 0; k < plan->kernels.size(); ++k)
        several = several || ((int)k != l.kernel && plan->kernels[k].depth == kd.depth &&
                              plan->kernels[k].kind == SODA_HIP_KERNEL_FUSED);
    }
    if (e || !several) return e;
    int best_form = 0;
    float best_form_ms = 0;
    for (int form = 0; form < 3 && !e; ++form) {
      plan->tuned_form[key] = form;
      float fastest = 0;
      e = time_sweep(2, &fastest);
      if (tuning_env("SODA_HIP_DEBUG"))
        fprintf(stderr, "soda_hip: tune %d iteration(s): form %d -> %.1f us\n", iterate, form,
                fastest * 1000.0);
      if (form == 0 || fastest < best_form_ms) { best_form = form; best_form_ms = fastest; }
    }
    if (e) plan->tuned_form.erase(key);
    else plan->tuned_form[key] = best_form;
    return e;
  };
  if (candidates.size() < 2) {      // one split only: the forms and the streaming launches remain
    rc = tune_forms();
    if (!rc) rc = tune_streaming(plan, dims, iterate, valid_lo, valid_hi, time_sweep);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
  }
  // every candidate as a whole sweep, in context: one untimed run, then the faster
  // of two timed ones
  size_t best = 0;
  float best_ms = 0;
  for (size_t c = 0; c < candidates.size() && !rc; ++c) {
    plan->tuned_split[key] = candidates[c];
    float fastest = 0;
    rc = time_sweep(2, &fastest);
    if (tuning_env("SODA_HIP_DEBUG")) {
      fprintf(stderr, "soda_hip: tune %d iteration(s):", iterate);
      for (int d : candidates[c]) fprintf(stderr, " %d", d);
      fprintf(stderr, "  -> %.1f us\n", fastest * 1000.0);
    }
    if (c == 0 || fastest < best_ms) { best = c; best_ms = fastest; }
  }
  if (rc) plan->tuned_split.erase(key);
  else plan->tuned_split[key] = candidates[best];
  if (!rc) rc = tune_forms();
  if (!rc) rc = tune_streaming(plan, dims, iterate, valid_lo, valid_hi, time_sweep);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

int soda_hip_plan_set_split(soda_hip_plan* plan, const int64_t dims[SODA_HIP_MAX_DIMS],
                            int iterate, const int32_t* depths, int n_depths) {
  if (!plan || !dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  const std::array<int64_t, 5> key = split_key(plan, dims, iterate);
  if (!depths || n_depths <= 0) {      // back to the scheduler's own choice
    plan->tuned_split.erase(key);
    return 0;
  }
  int total = 0;
  for (int i = 0; i < n_depths; ++i) {
    bool known = false;
    for (const soda_hip_kernel& kd : plan->kernels)
      known = known || (kd.kind == SODA_HIP_KERNEL_FUSED && kd.depth == depths[i]);
    if (!known)
      return fail(SODA_HIP_ERR_NO_KERNEL, "no fused kernel of depth %d in the blob",
                  (int)depths[i]);
    total += depths[i];
  }
  if (total != iterate)
    return fail(SODA_HIP_ERR_CONSTRAINT, "the depths add up to %d, not to iterate = %d",
                total, iterate);
  plan->tuned_split[key] = std::vector<int>(depths, depths + n_depths);
  return 0;
}

int soda_hip_plan_set_out_final_only(soda_hip_plan* plan, int on) {
  if (!plan) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "plan is NULL");
  plan->out_final_only = on != 0;
  return 0;
}

int soda_hip_plan_schedule_fields(soda_hip_plan* plan, const int64_t dims[SODA_HIP_MAX_DIMS],
                                  int iterate, const int32_t (*valid_lo)[SODA_HIP_MAX_DIMS],
                                  const int32_t (*valid_hi)[SODA_HIP_MAX_DIMS],
                                  int32_t* kernel_index, double* est_us, soda_hip_args* args,
                                  int capacity, int* n_launches) {
  if (!plan || !dims || !n_launches) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  std::vector<Launch> list;
  int depth = 0;
  ScratchNeeds needs;
  int rc = build_schedule_fields(plan, dims, iterate, valid_lo, valid_hi, &list, &depth, &needs);
  if (rc) return rc;
  *n_launches = (int)list.size();
  for (int i = 0; i < (int)list.size() && i < capacity; ++i) {
    if (kernel_index) kernel_index[i] = list[i].kernel;
    if (est_us) est_us[i] = list[i].est_us;
    if (args) args[i] = list[i].args;
  }
  return 0;
}

int soda_hip_plan_schedule(soda_hip_plan* plan, const int64_t dims[SODA_HIP_MAX_DIMS],
                           int iterate, const int32_t* valid_lo,
                           const int32_t* valid_hi, int32_t* kernel_index,
                           double* est_us, int capacity, int* n_launches) {
  if (!plan || !dims || !n_launches) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  const Repeated lo(plan, valid_lo), hi(plan, valid_hi);
  return soda_hip_plan_schedule_fields(plan, dims, iterate, lo.rows, hi.rows, kernel_index,
                                       est_us, nullptr, capacity, n_launches);
}

int soda_hip_sweep_fields(soda_hip_plan* plan, void* const* in, void* const* out,
                          const int64_t dims[SODA_HIP_MAX_DIMS], int iterate,
                          const int32_t (*valid_lo)[SODA_HIP_MAX_DIMS],
                          const int32_t (*valid_hi)[SODA_HIP_MAX_DIMS], void* stream) {
  if (!plan || !in || !out || !dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  std::vector<Launch> list;
  int depth = 0;
  int rc = bound_schedule(plan, in, out, dims, iterate, valid_lo, valid_hi, &list, &depth,
                          as_stream(stream));
  if (rc) return rc;
  for (const Launch& l : list) {
    rc = launch_one(plan, l, as_stream(stream));
    if (rc) return rc;
  }
  return 0;
}

int soda_hip_sweep(soda_hip_plan* plan, void* const* in, void* const* out,
                   const int64_t dims[SODA_HIP_MAX_DIMS], int iterate,
                   const int32_t* valid_lo, const int32_t* valid_hi, void* stream) {
  if (!plan || !in || !out || !dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  const Repeated lo(plan, valid_lo), hi(plan, valid_hi);
  return soda_hip_sweep_fields(plan, in, out, dims, iterate, lo.rows, hi.rows, stream);
}

int soda_hip_sweep_timed(soda_hip_plan* plan, void* const* in, void* const* out,
                         const int64_t dims[SODA_HIP_MAX_DIMS], int iterate,
                         int warmup, int repeats, void* stream,
                         soda_hip_timing* timing) {
  if (!plan || !in || !out || !dims) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (repeats < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "repeats must be >= 1");
  hipStream_t s = as_stream(stream);
  std::vector<Launch> list;
  int depth = 0;
  int rc = bound_schedule(plan, in, out, dims, iterate, nullptr, nullptr, &list, &depth, s);
  if (rc) return rc;
  for (int w = 0; w < warmup; ++w)
    for (const Launch& l : list)
      if ((rc = launch_one(plan, l, s))) return rc;
  // one event before every launch and one after the last, per repeat
  const size_t per = list.size() + 1;
  std::vector<hipEvent_t> ev(per * repeats, nullptr);
  for (auto& e : ev)
    if (!rc && hipEventCreate(&e) != hipSuccess) {
      e = nullptr;
      rc = fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventCreate failed");
    }
  for (int r = 0; r < repeats && !rc; ++r) {
    for (size_t i = 0; i < list.size() && !rc; ++i) {
      if (hipEventRecord(ev[r * per + i], s) != hipSuccess)
        rc = fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventRecord failed");
      else
        rc = launch_one(plan, list[i], s);
    }
    if (!rc && hipEventRecord(ev[r * per + list.size()], s) != hipSuccess)
      rc = fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventRecord failed");
  }
  if (!rc && hipStreamSynchronize(s) != hipSuccess)
    rc = fail(SODA_HIP_ERR_DEVICE_SYNC, "hipStreamSynchronize failed: %s",
              hipGetErrorString(hipGetLastError()));
  if (!rc && timing) {
    memset(timing, 0, sizeof *timing);
    double total_ms = 0;
    // every launch at its FASTEST repeat (events between launches add gaps and a
    // first repeat runs at other clocks: a mean over-states the kernels)
    std::vector<float> fastest(list.size(), 0.f);
    std::map<int, std::pair<double, int>> per_kernel;
    for (int r = 0; r < repeats; ++r) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ev[r * per], ev[r * per + list.size()]);
      total_ms += ms;
      for (size_t i = 0; i < list.size(); ++i) {
        float k_ms = 0;
        (void)hipEventElapsedTime(&k_ms, ev[r * per + i], ev[r * per + i + 1]);
        if (r == 0 || k_ms < fastest[i]) fastest[i] = k_ms;
      }
    }
    double fastest_ms = 0;
    for (size_t i = 0; i < list.size(); ++i) {
      auto& slot = per_kernel[list[i].kernel];
      slot.first += fastest[i];
      slot.second += 1;
      fastest_ms += fastest[i];
    }
    if (tuning_env("SODA_HIP_LAUNCH_TRACE"))   // tools/: every launch, fastest repeat
      for (size_t i = 0; i < list.size(); ++i) {
        const soda_hip_args& a = list[i].args;
        fprintf(stderr, "soda_hip: launch %3zu %-28s %8.1f us (model %7.1f)  box %lld x %lld x %lld  "
                "grid %u x %u x %u  chunk %lld  fill %d  resident %d  lds %u  rounds %lld\n", i,
                plan->kernels[list[i].kernel].name,
                fastest[i] * 1000.0, list[i].est_us, (long long)(a.box_hi[0] - a.box_lo[0]),
                (long long)(a.box_hi[1] - a.box_lo[1]), (long long)(a.box_hi[2] - a.box_lo[2]),
                list[i].grid[0], list[i].grid[1], list[i].grid[2], (long long)a.param[0],
                plan->kernels[list[i].kernel].fill_rows,
                list[i].resident > 0 ? (int)list[i].resident
                                     : plan->resident_blocks[list[i].kernel],
                list[i].lds_bytes, list[i].rounds);
      }
    timing->kernel_us = total_ms * 1000.0 / repeats;
    timing->fastest_us = fastest_ms * 1000.0;
    timing->launches = (int)list.size();
    timing->max_depth = depth;
    int best = -1;
    for (auto& kv : per_kernel)
      if (best < 0 || kv.second.first > per_kernel[best].first) best = kv.first;
    if (best >= 0) {
      timing->dominant_us = per_kernel[best].first * 1000.0;
      timing->dominant_launches = per_kernel[best].second;
      snprintf(timing->dominant_name, sizeof timing->dominant_name, "%s",
               plan->kernels[best].name);
    }
  }
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

// ------------------------------------------------------------- clock probe
int soda_hip_clock_probe_start(soda_hip_plan* plan, int spins) {
  if (!plan) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "plan is NULL");
  if (spins < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "spins must be >= 1");
  if (plan->probe_running) return fail(SODA_HIP_ERR_CONSTRAINT, "a clock probe is running");
  if (!plan->probe &&
      hipModuleGetFunction(&plan->probe, plan->module->mod, "soda_hip_clock_probe") != hipSuccess) {
    plan->probe = nullptr;
    (void)hipGetLastError();
    return fail(SODA_HIP_ERR_NO_KERNEL, "the blob holds no soda_hip_clock_probe (built "
                "before ABI 7)");
  }
  if (!plan->side &&
      hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking) != hipSuccess) {
    plan->side = nullptr;
    return fail(SODA_HIP_ERR_DEVICE_RUN, "hipStreamCreate failed");
  }
  if (!plan->probe_buf) HIP_TRY(SODA_HIP_ERR_DEVICE_MALLOC, hipMalloc(&plan->probe_buf, 16));
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN, hipMemsetAsync(plan->probe_buf, 0, 16, plan->side));
  struct { void* out; int spins; } args = {plan->probe_buf, spins};
  size_t size = sizeof args;
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE,
                    &size, HIP_LAUNCH_PARAM_END};
  // the wall time of the probe comes from events around it (the realtime counter it
  // reads is nominally 100 MHz; measured against events it is what calibrates it)
  if (!plan->probe_t0 && hipEventCreate(&plan->probe_t0) != hipSuccess) {
    plan->probe_t0 = nullptr;
    return fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventCreate failed");
  }
  if (!plan->probe_t1 && hipEventCreate(&plan->probe_t1) != hipSuccess) {
    plan->probe_t1 = nullptr;
    return fail(SODA_HIP_ERR_DEVICE_RUN, "hipEventCreate failed");
  }
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN, hipEventRecord(plan->probe_t0, plan->side));
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN,
          hipModuleLaunchKernel(plan->probe, 1, 1, 1, 64, 1, 1, 0, plan->side, nullptr, config));
  HIP_TRY(SODA_HIP_ERR_DEVICE_RUN, hipEventRecord(plan->probe_t1, plan->side));
  plan->probe_running = true;
  return 0;
}

int soda_hip_clock_probe_finish(soda_hip_plan* plan, double* shader_ghz, double* seconds) {
  if (!plan || !shader_ghz) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  if (!plan->probe_running) return fail(SODA_HIP_ERR_CONSTRAINT, "no clock probe is running");
  plan->probe_running = false;
  HIP_TRY(SODA_HIP_ERR_DEVICE_SYNC, hipStreamSynchronize(plan->side));
  unsigned long long got[2] = {0, 0};
  HIP_TRY(SODA_HIP_ERR_COPY_TO_HOST, hipMemcpy(got, plan->probe_buf, 16, hipMemcpyDeviceToHost));
  if (!got[1]) return fail(SODA_HIP_ERR_DEVICE_RUN, "the clock probe reported no time");
  // s_memrealtime ticks at a nominal 100 MHz; the events around the probe give the wall
  // time independently (the kernel is one wavefront that starts at once on the non-blocking
  // stream, so both spans agree to a few microseconds when the counter's rate is as named)
  double elapsed = (double)got[1] / 100.0e6;
  float ms = 0;
  if (hipEventElapsedTime(&ms, plan->probe_t0, plan->probe_t1) == hipSuccess && ms > 0) {
    const double by_events = ms * 1e-3;
    if (tuning_env("SODA_HIP_DEBUG"))
      fprintf(stderr, "soda_hip: clock probe: %llu shader cycles, %llu realtime ticks = %.3f ms "
              "at 100 MHz, events %.3f ms\n", got[0], got[1], elapsed * 1e3, by_events * 1e3);
    // a probe that waited for a wave slot makes the event span LONGER than its own count;
    // take the counter unless the two disagree by more than the realtime clock could
    if (by_events < elapsed * 0.97) elapsed = by_events;
  }
  *shader_ghz = (double)got[0] / elapsed / 1e9;
  if (seconds) *seconds = elapsed;
  return 0;
}

// how many (kernel, box) pairs of the plan run a MEASURED (chunk, workgroups per CU)
// instead of the kernel's calibrated one (soda_hip_plan_tune's streaming step)
int soda_hip_plan_tuned_streams(const soda_hip_plan* plan, int* n) {
  if (!plan || !n) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  *n = (int)plan->tuned_stream.size();
  return 0;
}

// ------------------------------------------------- host-buffer entry point
int soda_hip_run_buffers(soda_hip_plan* plan, soda_hip_buffer_t* const* inputs,
                         soda_hip_buffer_t* const* outputs, int iterate,
                         soda_hip_timing* timing) {
  if (!plan || !inputs || !outputs) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "NULL argument");
  const soda_hip_program& p = plan->prog;
  for (int j = 0; j < p.n_inputs; ++j)
    if (!inputs[j]) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "input buffer %d is NULL", j);
  for (int j = 0; j < p.n_outputs; ++j)
    if (!outputs[j]) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "output buffer %d is NULL", j);
  int32_t mlo[SODA_HIP_MAX_DIMS], mhi[SODA_HIP_MAX_DIMS];
  if (iterate < 1) return fail(SODA_HIP_ERR_CONSTRAINT, "iterate must be >= 1");
  output_margins(plan, iterate, mlo, mhi);

  // Bounds-query mode (host.py:204-252): a buffer with neither host nor device
  // memory only gets the shape it must have written into it, and nothing runs.
  // As the generated reference code (its halide_rewrite_buffer, host.py:100-113,
  // sets min / extent / stride of all four dimensions and leaves elem_size
  // alone): a null OUTPUT keeps its min and extents and gets dense strides; a
  // null INPUT gets the first output's min and that output's extents plus the
  // stencil window minus one, the window being the one between the FIRST input and
  // the first output (core.get_stencil_dim(get_overall_stencil_window(input 0,
  // output 0)), host.py:226-233) - for every null input, as in the reference.
  bool query = false;
  auto is_null = [](const soda_hip_buffer_t* b) { return b->host == nullptr && b->dev == 0; };
  for (int j = 0; j < p.n_outputs; ++j) query |= is_null(outputs[j]);
  for (int j = 0; j < p.n_inputs; ++j) query |= is_null(inputs[j]);
  if (query) {
    const soda_hip_buffer_t* o0 = outputs[0];
    // As the reference (host.py:226-233): the window between the FIRST input and the
    // first output, whichever input is asked about - for denoise2d / denoise3d, whose
    // first input `f` is read at the cell itself only, that is too small for `u`; it
    // is the reference's answer all the same.  The composed window of `iterate`
    // iterations with only input 0 as origin:
    Box window{};
    {
      const int nt = n_tensors(p);
      std::vector<Box> feed(p.n_inputs, Box{});
      feed[0].set = true;
      std::vector<Box> cur;
      for (int it = 0; it < iterate; ++it) {
        cur.assign(nt, Box{});
        for (int i = 0; i < p.n_inputs; ++i) cur[i] = feed[i];
        for (int st = 0; st < p.n_stages; ++st) {
          const int t = p.n_inputs + st;
          Box acc{};
          for (int w = 0; w < p.n_windows; ++w) {
            const soda_hip_window& win = p.window[w];
            if (win.stage != t || !cur[win.parent].set) continue;
            const Box& par = cur[win.parent];
            for (int d = 0; d < p.dim; ++d) {
              const int32_t lo = par.lo[d] + win.lo[d], hi = par.hi[d] + win.hi[d];
              acc.lo[d] = acc.set ? std::min(acc.lo[d], lo) : lo;
              acc.hi[d] = acc.set ? std::max(acc.hi[d], hi) : hi;
            }
            acc.set = true;
          }
          for (int d = 0; d < p.dim && acc.set; ++d) {   // boxes contain the cell itself
            acc.lo[d] = std::min<int32_t>(acc.lo[d], 0);
            acc.hi[d] = std::max<int32_t>(acc.hi[d], 0);
          }
          cur[t] = acc;
        }
        if (p.n_inputs == p.n_outputs)
          for (int j = 0; j < p.n_inputs; ++j) feed[j] = cur[p.output_tensor[j]];
      }
      window = cur[p.output_tensor[0]];
      if (!window.set)      // the first output does not depend on the first input
        window = plan->fresh.boxes[iterate - 1][p.output_tensor[0]];
    }
    for (int j = 0; j < p.n_outputs; ++j) {
      soda_hip_buffer_t* b = outputs[j];
      if (!is_null(b)) continue;
      int32_t stride = 1;
      for (int d = 0; d < 4; ++d) {
        if (d < p.dim) { b->stride[d] = stride; stride *= b->extent[d]; }
        else { b->min[d] = b->extent[d] = b->stride[d] = 0; }
      }
    }
    for (int j = 0; j < p.n_inputs; ++j) {
      soda_hip_buffer_t* b = inputs[j];
      if (!is_null(b)) continue;
      int32_t stride = 1;
      for (int d = 0; d < 4; ++d) {
        if (d < p.dim) {
          b->min[d] = o0->min[d];
          b->extent[d] = o0->extent[d] + window.hi[d] - window.lo[d];
          b->stride[d] = stride;
          stride *= b->extent[d];
        } else {
          b->min[d] = b->extent[d] = b->stride[d] = 0;
        }
      }
    }
    return 0;
  }

  // element-size checks (host.py:254-255, :969-982)
  for (int j = 0; j < p.n_outputs; ++j)
    if (outputs[j]->elem_size != p.elem_size[p.output_tensor[j]]) {
      fprintf(stderr, "Buffer output %d has elem_size %d instead of %d\n", j,
              outputs[j]->elem_size, p.elem_size[p.output_tensor[j]]);
      return fail(SODA_HIP_ERR_BAD_ELEM_SIZE, "output %d: elem_size %d, expected %d", j,
                  outputs[j]->elem_size, p.elem_size[p.output_tensor[j]]);
    }
  for (int j = 0; j < p.n_inputs; ++j)
    if (inputs[j]->elem_size != p.elem_size[j]) {
      fprintf(stderr, "Buffer input %d has elem_size %d instead of %d\n", j,
              inputs[j]->elem_size, p.elem_size[j]);
      return fail(SODA_HIP_ERR_BAD_ELEM_SIZE, "input %d: elem_size %d, expected %d", j,
                  inputs[j]->elem_size, p.elem_size[j]);
    }
  int64_t dims[SODA_HIP_MAX_DIMS] = {1, 1, 1, 1};
  size_t cells = 1;
  for (int d = 0; d < p.dim; ++d) {
    dims[d] = inputs[0]->extent[d];
    if (dims[d] <= 0) return fail(SODA_HIP_ERR_CONSTRAINT, "extent[%d] = %lld", d,
                                  (long long)dims[d]);
    cells *= (size_t)dims[d];
  }
  auto dense = [&](const soda_hip_buffer_t* b, const char* what, int j) -> int {
    int64_t stride = 1;
    for (int d = 0; d < p.dim; ++d) {
      if (b->extent[d] != dims[d])
        return fail(SODA_HIP_ERR_CONSTRAINT, "%s %d: extent[%d] = %d, expected %lld", what,
                    j, d, b->extent[d], (long long)dims[d]);
      if (b->stride[d] != stride)
        return fail(SODA_HIP_ERR_CONSTRAINT, "%s %d: stride[%d] = %d, expected %lld "
                    "(dense row-major arrays only)", what, j, d, b->stride[d],
                    (long long)stride);
      stride *= dims[d];
    }
    if (!b->host) return fail(SODA_HIP_ERR_NULL_ARGUMENT, "%s %d has no host memory", what, j);
    return 0;
  };
  for (int j = 0; j < p.n_inputs; ++j) { int rc = dense(inputs[j], "input", j); if (rc) return rc; }
  for (int j = 0; j < p.n_outputs; ++j) { int rc = dense(outputs[j], "output", j); if (rc) return rc; }

  std::vector<void*> din(p.n_inputs, nullptr), dout(p.n_outputs, nullptr);
  int rc = 0;
  auto cleanup = [&]() {
    for (void* q : din) if (q) (void)hipFree(q);
    for (void* q : dout) if (q) (void)hipFree(q);
  };
  for (int j = 0; j < p.n_inputs && !rc; ++j) {
    const size_t bytes = cells * p.elem_size[j];
    if (hipMalloc(&din[j], bytes) != hipSuccess)
      rc = fail(SODA_HIP_ERR_DEVICE_MALLOC, "hipMalloc(%zu) failed", bytes);
    else if (hipMemcpy(din[j], inputs[j]->host, bytes, hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(SODA_HIP_ERR_COPY_TO_DEVICE, "H2D copy of input %d failed", j);
  }
  for (int j = 0; j < p.n_outputs && !rc; ++j) {
    const size_t bytes = cells * p.elem_size[p.output_tensor[j]];
    if (hipMalloc(&dout[j], bytes) != hipSuccess)
      rc = fail(SODA_HIP_ERR_DEVICE_MALLOC, "hipMalloc(%zu) failed", bytes);
    else if (hipMemset(dout[j], 0, bytes) != hipSuccess)
      rc = fail(SODA_HIP_ERR_DEVICE_RUN, "hipMemset failed");
  }
  soda_hip_timing local;
  if (!rc) rc = soda_hip_sweep_timed(plan, din.data(), dout.data(), dims, iterate, 1, 1,
                                     nullptr, &local);
  if (!rc) {
    // host.py:796-800: pixels = product of input extents, not multiplied by iterate
    printf("Kernel execution time: %lf us\n", local.kernel_us);
    printf("Kernel throughput: %lf pixel/ns\n", (double)cells / local.kernel_us / 1e3);
    fflush(stdout);
    if (timing) *timing = local;
  }
  // only the valid interior goes back to the caller (host.py:838-899)
  for (int j = 0; j < p.n_outputs && !rc; ++j) {
    const int es = p.elem_size[p.output_tensor[j]];
    int64_t lo[4] = {0, 0, 0, 0}, hi[4] = {1, 1, 1, 1}, ext[4] = {1, 1, 1, 1};
    bool empty = false;
    // each output has its own composed window (host.py:1082-1091)
    const Box& ob = plan->fresh.boxes[iterate - 1][p.output_tensor[j]];
    for (int d = 0; d < p.dim; ++d) {
      lo[d] = -ob.lo[d]; hi[d] = dims[d] - ob.hi[d]; ext[d] = dims[d];
      if (hi[d] <= lo[d]) empty = true;
    }
    if (empty) continue;
    // one 3-D copy per index of the fourth dimension
    for (int64_t w = lo[3]; w < hi[3] && !rc; ++w) {
      const size_t skip = (size_t)w * ext[0] * ext[1] * ext[2] * es;
      hipMemcpy3DParms parms;
      memset(&parms, 0, sizeof parms);
      parms.srcPtr = make_hipPitchedPtr((char*)dout[j] + skip, ext[0] * es, ext[0] * es,
                                        ext[1]);
      parms.dstPtr = make_hipPitchedPtr((char*)outputs[j]->host + skip, ext[0] * es,
                                        ext[0] * es, ext[1]);
      parms.srcPos = make_hipPos(lo[0] * es, lo[1], lo[2]);
      parms.dstPos = make_hipPos(lo[0] * es, lo[1], lo[2]);
      parms.extent = make_hipExtent((hi[0] - lo[0]) * es, hi[1] - lo[1], hi[2] - lo[2]);
      parms.kind = hipMemcpyDeviceToHost;
      if (hipMemcpy3D(&parms) != hipSuccess)
        rc = fail(SODA_HIP_ERR_COPY_TO_HOST, "D2H copy of output %d failed: %s", j,
                  hipGetErrorString(hipGetLastError()));
    }
  }
  cleanup();
  return rc;
}

}  // extern "C"
