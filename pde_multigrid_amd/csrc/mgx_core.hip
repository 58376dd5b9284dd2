// mgx_core.hip -- context, its parameter table (mgx_ctx_set_param), memory, events, errors behind include/mgx.h.
#include "mgx_host3d.hpp"

namespace mgx {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// zero fill at streaming-store speed: hipMemsetAsync reaches about 2.8 TB/s on large arrays, 16-byte non-temporal
// stores about twice that (the coarse v of every level is zeroed once per cycle)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) fill_zero_kernel(u32x4* __restrict__ p, size_t n16) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) __builtin_nontemporal_store(z, &p[i]);
}

int fill_zero(mgx_ctx* ctx, void* dst, size_t bytes) {
    if (!bytes) return MGX_OK;
    if (bytes < ((size_t)4 << 20) || ((uintptr_t)dst & 15) || (bytes & 15)) {
        MGX_HIP(hipMemsetAsync(dst, 0, bytes, ctx->compute));
        return MGX_OK;
    }
    const size_t n16 = bytes >> 4;
    size_t blocks = (n16 + 256 * 8 - 1) / (256 * 8);  // 8 stores per thread
    const size_t cap = (size_t)ctx->num_cus * 32;
    if (blocks > cap) blocks = cap;
    MGX_LAUNCH(fill_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->compute, (u32x4*)dst, n16);
    MGX_HIP(hipGetLastError());
    return MGX_OK;
}

// ---- test hook: LDS poisoning (mgx_test_set_lds_poison) ----
// One workgroup claims all of a CU's LDS (160 KB), so no two of them share a CU; each stays ~10 us, far longer than the
// dispatcher needs to hand out the grid, so a grid of 2 x CUs workgroups on an idle GPU visits every CU.  The pattern is a
// NaN as fp64 and as two fp32 words.
int g_poison_lds = 0;
static constexpr int POISON_LDS_BYTES = 160 * 1024;
__global__ void __launch_bounds__(1024) poison_lds_kernel(unsigned long long pattern) {
    extern __shared__ unsigned long long poison_lds_[];
    volatile unsigned long long* p = poison_lds_;
    for (int i = threadIdx.x; i < POISON_LDS_BYTES / 8; i += 1024) p[i] = pattern;
    __syncthreads();
    const long long t0 = wall_clock64();  // 100 MHz
    for (int k = 0; k < 4096 && wall_clock64() - t0 < 1000; k++) __builtin_amdgcn_s_sleep(16);
}

void poison_lds_launch(hipStream_t stream) {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        cus = 256;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        (void)hipFuncSetAttribute((const void*)poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, POISON_LDS_BYTES);
    }
    hipLaunchKernelGGL(poison_lds_kernel, dim3(2 * cus), dim3(1024), POISON_LDS_BYTES, stream, 0x7FF4DEAD7FA0DEADull);
}

// counts, over every workgroup of the grid, the LDS words that carry `pattern` WITHOUT having written any: what the previous
// launch left behind (mgx_test_lds_probe: the self-test of the poisoning)
__global__ void __launch_bounds__(1024) probe_lds_kernel(unsigned long long pattern, unsigned long long* hits) {
    extern __shared__ unsigned long long poison_lds_[];
    volatile unsigned long long* p = poison_lds_;
    unsigned n = 0;
    for (int i = threadIdx.x; i < POISON_LDS_BYTES / 8; i += 1024) n += p[i] == pattern;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(hits, (unsigned long long)n);
    const long long t0 = wall_clock64();
    for (int k = 0; k < 4096 && wall_clock64() - t0 < 1000; k++) __builtin_amdgcn_s_sleep(16);
}

int workspace(mgx_ctx* ctx, size_t bytes, void** out) {
    if (ctx->scratch_bytes < bytes) {
        if (ctx->scratch) {
            MGX_HIP(hipStreamSynchronize(ctx->compute));
            MGX_HIP(hipFree(ctx->scratch));
            ctx->scratch = nullptr;
            ctx->scratch_bytes = 0;
        }
        size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
        MGX_HIP(hipMalloc(&ctx->scratch, want));
        ctx->scratch_bytes = want;
    }
    *out = ctx->scratch;
    return MGX_OK;
}

}  // namespace mgx

extern "C" {

const char* mgx_status_string(int s) {
    switch (s) {
        case MGX_OK: return "MGX_OK";
        case MGX_ERR_INVALID: return "MGX_ERR_INVALID";
        case MGX_ERR_SIZE: return "MGX_ERR_SIZE";
        case MGX_ERR_HIP: return "MGX_ERR_HIP";
        case MGX_ERR_NOMEM: return "MGX_ERR_NOMEM";
        case MGX_ERR_RCCL: return "MGX_ERR_RCCL";
        case MGX_ERR_NOGPU: return "MGX_ERR_NOGPU";
    }
    return "MGX_ERR_UNKNOWN";
}

const char* mgx_last_error(void) { return mgx::g_err; }
void mgx_set_last_error(const char* msg) { mgx::set_error("%s", msg ? msg : ""); }
const char* mgx_version(void) { return "mgx 0.1 (gfx950)"; }

int mgx_device_count(int* count) {
    MGX_REQUIRE(count, MGX_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        (void)hipGetLastError();
        return mgx::fail(MGX_ERR_NOGPU, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return MGX_OK;
}

int mgx_ctx_create(int device, mgx_ctx** out) {
    MGX_REQUIRE(out, MGX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return mgx::fail(MGX_ERR_NOGPU, "no HIP device visible: the HIP path cannot run (there is no CPU fallback)");
    }
    MGX_REQUIRE(device >= 0 && device < n, MGX_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    MGX_HIP(hipSetDevice(device));
    mgx_ctx* c = new mgx_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->comm, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_compute, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming)) != hipSuccess) {
        delete c;
        return mgx::fail(MGX_ERR_HIP, "stream/event creation failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return MGX_OK;
}

int mgx_ctx_destroy(mgx_ctx* ctx) {
    if (!ctx) return MGX_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->rccl_comm) mgx_comm_destroy(ctx);
    (void)hipStreamSynchronize(ctx->compute);
    (void)hipStreamSynchronize(ctx->comm);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->rehearse_buf) (void)hipFree(ctx->rehearse_buf);
    if (ctx->sweep_dev) (void)hipFree(ctx->sweep_dev);
    if (ctx->resident_buf) (void)hipFree(ctx->resident_buf);
    if (ctx->sweep_abort) (void)hipHostFree(ctx->sweep_abort);
    (void)hipEventDestroy(ctx->ev_compute);
    (void)hipEventDestroy(ctx->ev_comm);
    (void)hipStreamDestroy(ctx->compute);
    (void)hipStreamDestroy(ctx->comm);
    delete ctx;
    return MGX_OK;
}

int mgx_ctx_sync(mgx_ctx* ctx) {
    MGX_REQUIRE(ctx, MGX_ERR_INVALID, "ctx is NULL");
    MGX_USE(ctx);
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->comm));
    return mgx_ctx_check(ctx);
}

int mgx_ctx_device(const mgx_ctx* ctx, int* device) {
    MGX_REQUIRE(ctx && device, MGX_ERR_INVALID, "NULL argument");
    *device = ctx->device;
    return MGX_OK;
}

int mgx_ctx_stream(const mgx_ctx* ctx, void** hip_stream) {
    MGX_REQUIRE(ctx && hip_stream, MGX_ERR_INVALID, "NULL argument");
    *hip_stream = (void*)ctx->compute;
    return MGX_OK;
}

int mgx_malloc(mgx_ctx* ctx, size_t bytes, void** dptr) {
    MGX_REQUIRE(ctx && dptr, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    *dptr = nullptr;
    if (bytes == 0) return MGX_OK;
    hipError_t e = hipMalloc(dptr, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return mgx::fail(MGX_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    return MGX_OK;
}

int mgx_free(mgx_ctx* ctx, void* dptr) {
    MGX_REQUIRE(ctx, MGX_ERR_INVALID, "ctx is NULL");
    MGX_USE(ctx);
    if (!dptr) return MGX_OK;
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->comm));
    MGX_HIP(hipFree(dptr));
    return MGX_OK;
}

int mgx_memcpy_h2d(mgx_ctx* ctx, void* dst, const void* host_src, size_t bytes) {
    MGX_REQUIRE(ctx && (bytes == 0 || (dst && host_src)), MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    if (!bytes) return MGX_OK;
    MGX_HIP(hipMemcpyAsync(dst, host_src, bytes, hipMemcpyHostToDevice, ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    return MGX_OK;
}

int mgx_memcpy_d2h(mgx_ctx* ctx, void* host_dst, const void* src, size_t bytes) {
    MGX_REQUIRE(ctx && (bytes == 0 || (host_dst && src)), MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    if (!bytes) return MGX_OK;
    MGX_HIP(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    return MGX_OK;
}

int mgx_memcpy_d2d(mgx_ctx* ctx, void* dst, const void* src, size_t bytes) {
    MGX_REQUIRE(ctx && (bytes == 0 || (dst && src)), MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    if (!bytes) return MGX_OK;
    MGX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->compute));
    return MGX_OK;
}

int mgx_memset_zero(mgx_ctx* ctx, void* dst, size_t bytes) {
    MGX_REQUIRE(ctx && (bytes == 0 || dst), MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    return mgx::fill_zero(ctx, dst, bytes);
}

int mgx_test_set_lds_poison(int on) {
    mgx::g_poison_lds = on != 0;
    return MGX_OK;
}

int mgx_test_lds_probe(mgx_ctx* ctx, double* fraction) {
    MGX_REQUIRE(ctx && fraction, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    void* ws = nullptr;
    MGX_TRY_RET(mgx::workspace(ctx, 8, &ws));
    MGX_HIP(hipMemsetAsync(ws, 0, 8, ctx->compute));
    MGX_HIP(hipFuncSetAttribute((const void*)mgx::probe_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, mgx::POISON_LDS_BYTES));
    const int blocks = ctx->num_cus;
    MGX_LAUNCH(mgx::probe_lds_kernel, dim3(blocks), dim3(1024), mgx::POISON_LDS_BYTES, ctx->compute, 0x7FF4DEAD7FA0DEADull,
               (unsigned long long*)ws);
    unsigned long long hits = 0;
    MGX_HIP(hipMemcpyAsync(&hits, ws, 8, hipMemcpyDeviceToHost, ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    *fraction = (double)hits / ((double)blocks * (mgx::POISON_LDS_BYTES / 8));
    return MGX_OK;
}

int mgx_graph_begin(mgx_ctx* ctx) {
    MGX_REQUIRE(ctx, MGX_ERR_INVALID, "ctx is NULL");
    MGX_USE(ctx);
    MGX_HIP(hipStreamBeginCapture(ctx->compute, hipStreamCaptureModeThreadLocal));
    return MGX_OK;
}

int mgx_graph_end(mgx_ctx* ctx, void** graph_exec) {
    MGX_REQUIRE(ctx && graph_exec, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    *graph_exec = nullptr;
    hipGraph_t g = nullptr;
    MGX_HIP(hipStreamEndCapture(ctx->compute, &g));
    hipGraphExec_t e = nullptr;
    hipError_t r = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (r != hipSuccess) return mgx::fail(MGX_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(r));
    *graph_exec = (void*)e;
    return MGX_OK;
}

int mgx_graph_launch(mgx_ctx* ctx, void* graph_exec) {
    MGX_REQUIRE(ctx && graph_exec, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    MGX_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, ctx->compute));
    return MGX_OK;
}

int mgx_graph_destroy(mgx_ctx* ctx, void* graph_exec) {
    MGX_REQUIRE(ctx, MGX_ERR_INVALID, "ctx is NULL");
    MGX_USE(ctx);
    if (graph_exec) MGX_HIP(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return MGX_OK;
}

int mgx_event_create(mgx_ctx* ctx, mgx_event** out) {
    MGX_REQUIRE(ctx && out, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    mgx_event* e = new mgx_event();
    hipError_t r = hipEventCreate(&e->ev);
    if (r != hipSuccess) {
        delete e;
        return mgx::fail(MGX_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(r));
    }
    *out = e;
    return MGX_OK;
}

int mgx_event_destroy(mgx_ctx* ctx, mgx_event* ev) {
    (void)ctx;
    if (!ev) return MGX_OK;
    (void)hipEventDestroy(ev->ev);
    delete ev;
    return MGX_OK;
}

int mgx_event_record(mgx_ctx* ctx, mgx_event* ev) {
    MGX_REQUIRE(ctx && ev, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    MGX_HIP(hipEventRecord(ev->ev, ctx->compute));
    return MGX_OK;
}

int mgx_event_elapsed_ms(mgx_ctx* ctx, mgx_event* start, mgx_event* stop, float* ms) {
    MGX_REQUIRE(ctx && start && stop && ms, MGX_ERR_INVALID, "NULL argument");
    MGX_USE(ctx);
    MGX_HIP(hipEventSynchronize(stop->ev));
    MGX_HIP(hipEventElapsedTime(ms, start->ev, stop->ev));
    return MGX_OK;
}

const char* mgx_ctx_last_relax_kernel(const mgx_ctx* ctx) { return ctx ? ctx->last_relax_kernel : ""; }
const char* mgx_ctx_last_rr_kernel(const mgx_ctx* ctx) { return ctx ? ctx->last_rr_kernel : ""; }
const char* mgx_ctx_last_corr_kernel(const mgx_ctx* ctx) { return ctx ? ctx->last_corr_kernel : ""; }
const char* mgx_ctx_last_block3_kernel(const mgx_ctx* ctx) { return ctx ? ctx->last_block3_kernel : ""; }

int mgx_ctx_set_param(mgx_ctx* ctx, const char* name, int value) {
    MGX_REQUIRE(ctx && name, MGX_ERR_INVALID, "set_param: NULL argument");
    MGX_USE(ctx);
    ctx->generation++;  // also on a rejected value: a spurious re-capture is harmless
    if (!strcmp(name, "relax3d.ty")) {
        MGX_REQUIRE(value == 1 || value == 2 || value == 4 || value == 8, MGX_ERR_INVALID, "relax3d.ty (waves per block) must be 1, 2, 4 or 8");
        ctx->relax_ty = value;
    } else if (!strcmp(name, "relax3d.small")) {
        ctx->relax_small = value ? 1 : 0;  // one-workgroup LDS kernel for levels <= 17^3
    } else if (!strcmp(name, "relax3d.ablate")) {
#ifdef MGX_DIAGNOSTICS
        ctx->relax_ablate = value;  // diagnostic builds only: non-zero gives WRONG results (see relax3d_xs_kernel)
#else
        return mgx::fail(MGX_ERR_INVALID, "set_param: 'relax3d.ablate' exists only in diagnostic builds (make diag)");
#endif
    } else if (!strcmp(name, "relax3d.wave_planes")) {
        ctx->relax_wave_planes = value;  // < 0 automatic, 0 off (whole-grid passes), > 0 planes per slab
    } else if (!strcmp(name, "relax3d.rows")) {
        MGX_REQUIRE(value == 1 || value == 2 || value == 4 || value == 8, MGX_ERR_INVALID, "relax3d.rows must be 1, 2, 4 or 8");
        ctx->relax_rows = value;
    } else if (!strcmp(name, "residual_restrict3d.rows")) {
        MGX_REQUIRE(value == 0 || value == 2 || value == 4, MGX_ERR_INVALID, "residual_restrict3d.rows (fine rows per wave of the pipelined kernel) must be 0 (by level size), 2 or 4");
        ctx->rr_rows = value;
    } else if (!strcmp(name, "residual_restrict3d.rcp")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "residual_restrict3d.rcp must be 0 or 1");
        ctx->rr_rcp = value;
    } else if (!strcmp(name, "mixed3d.fused")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "mixed3d.fused must be 0 or 1");
        ctx->mixed_fused = value;
    } else if (!strcmp(name, "mixed3d.rows")) {
        MGX_REQUIRE(value == 2 || value == 4 || value == 8, MGX_ERR_INVALID, "mixed3d.rows must be 2, 4 or 8");
        ctx->mixed_rows = value;
    } else if (!strcmp(name, "mixed3d.zchunk")) {
        MGX_REQUIRE(value >= 0, MGX_ERR_INVALID, "mixed3d.zchunk must be >= 0 (0 = automatic)");
        ctx->mixed_zchunk = value;
    } else if (!strcmp(name, "residual_restrict3d.xcd")) {
        MGX_REQUIRE(value >= 0 && value <= 2, MGX_ERR_INVALID, "residual_restrict3d.xcd must be 0, 1 or 2");
        ctx->rr_xcd = value;
    } else if (!strcmp(name, "relax3d.xcd")) {
        MGX_REQUIRE(value >= 0 && value <= 2, MGX_ERR_INVALID, "relax3d.xcd must be 0, 1 or 2");
        ctx->relax_xcd = value;
    } else if (!strcmp(name, "relax3d.lds")) {
        // -1 = automatic (default), 0 = relax3d_xs_kernel, 1000 + 100*WX + 10*WY + R = relax3d_xs_pipe_kernel<WX, WY, R>,
        // 3282 = the 2 x 8 x 2 shape with non-temporal loads of f; below 1000 (no software pipeline): diagnostic builds
        bool ok = value == -1 || value == 0 || value == 3282 || (value >= 1000 && value < 2000 && mgx::relax3d_lds_shape_known(value - 1000));
#ifdef MGX_DIAGNOSTICS
        ok = ok || (value > 0 && value < 1000 && mgx::relax3d_lds_shape_known(value)) || (value >= 3000 && mgx::relax3d_lds_shape_known(value - 3000));
#endif
        MGX_REQUIRE(ok, MGX_ERR_INVALID, "relax3d.lds = %d is not a kernel shape of this build", value);
        ctx->relax_lds = value;
    } else if (!strcmp(name, "residual_restrict3d.cr")) {
        MGX_REQUIRE(value >= 0 && value <= 2, MGX_ERR_INVALID, "residual_restrict3d.cr must be 0 (by level size), 1 or 2");
        ctx->rr_cr = value;   // coarse rows per lane of the streaming kernel
    } else if (!strcmp(name, "residual_restrict3d.tyw")) {
        MGX_REQUIRE(value == 2 || value == 4 || value == 8, MGX_ERR_INVALID, "residual_restrict3d.tyw (waves per block) must be 2, 4 or 8");
        ctx->rr_tyw = value;
    } else if (!strcmp(name, "residual_restrict3d.stream")) {
        MGX_REQUIRE(value >= 0 && value <= 3, MGX_ERR_INVALID, "residual_restrict3d.stream must be 0 ... 3");
        ctx->rr_stream = value;  // 0 = LDS rolling-window kernel, 1 = streaming shuffle kernel,
                                                              // 2 = pipelined with halos through LDS (x-split), 3 = 2 on large levels, else 1 (default)
    } else if (!strcmp(name, "residual_restrict3d.pzchunk")) {
        MGX_REQUIRE(value >= 0, MGX_ERR_INVALID, "residual_restrict3d.pzchunk must be >= 0 (0 = automatic)");
        ctx->rr_pzchunk = value;
    } else if (!strcmp(name, "relax3d.zero_first")) {
        ctx->relax_zero_first = value ? 1 : 0;  // relax_from_zero: first red pass without reading v (1) or zero fill + generic passes (0)
    } else if (!strcmp(name, "relax3d.v2")) {
        ctx->relax_v2 = value ? 1 : 0;  // fp32, wide levels: two x-pairs per lane (relax3d_xs_pipe_v2_kernel) or one
    } else if (!strcmp(name, "relax3d.corr_fuse")) {
        ctx->corr_fuse = value ? 1 : 0;  // interpolate_correct_relax: first red pass reads the correction on the fly (1) or in-place correction first (0)
    } else if (!strcmp(name, "cycle2d.tile")) {
        MGX_REQUIRE(value == 0 || value == 16 || value == 32 || value == 64, MGX_ERR_INVALID, "cycle2d.tile must be 0 (automatic), 16, 32 or 64");
        ctx->cyc2_tile = value;
    } else if (!strcmp(name, "cycle2d.tail_points")) {
        MGX_REQUIRE(value >= 0 && value <= 5120, MGX_ERR_INVALID, "cycle2d.tail_points must be in [0, 5120]");
        ctx->cyc2_tail_points = value;
    } else if (!strcmp(name, "relax3d.fused")) {
        ctx->sweep_fused = value ? 1 : 0;  // levels of 513-point rows: one launch per red+black sweep (mgx_sweep3d.hip) or one per colour
    } else if (!strcmp(name, "relax3d.corr_v2")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: relax3d.corr_v2 = %d not in {0, 1}", value);
        ctx->corr_v2 = value;
    } else if (!strcmp(name, "relax3d.zero_sweep")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: relax3d.zero_sweep = %d not in {0, 1}", value);
        ctx->relax_zero_sweep = value;
    } else if (!strcmp(name, "relax3d.resident")) {
        MGX_REQUIRE(value >= 0 && value <= 2, MGX_ERR_INVALID, "set_param: relax3d.resident = %d not in {0, 1, 2}", value);
        ctx->relax_resident = value;
    } else if (!strcmp(name, "sync.spin_limit")) {
        MGX_REQUIRE(value >= 1, MGX_ERR_INVALID, "set_param: sync.spin_limit = %d < 1", value);
        ctx->sync_spin_limit = (unsigned)value;  // polls before a wait between workgroups gives up (mgx_sync.hpp)
    } else if (!strcmp(name, "test.handoff_fault")) {
        MGX_REQUIRE(value >= 0 && value < (1 << 20), MGX_ERR_INVALID, "set_param: test.handoff_fault = %d out of range", value);
        ctx->handoff_fault = (unsigned)value;  // TEST HOOK: != 0 makes workgroup 0 of those kernels wait for tags nobody writes
    } else if (!strcmp(name, "gpu.exclusive")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: gpu.exclusive = %d not in {0, 1}", value);
        ctx->gpu_exclusive = value;  // 0: the GPU is shared -> no kernel whose workgroups wait for each other is launched
    } else if (!strcmp(name, "relax3d.corr_low")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: relax3d.corr_low = %d not in {0, 1}", value);
        ctx->corr_low = value;  // the correcting red pass in 8-wave workgroups, two to a CU (fp64)
    } else if (!strcmp(name, "slab.edges_merged")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: slab.edges_merged = %d not in {0, 1}", value);
        ctx->slab_edges_merged = value;  // the two edge planes of a z-slab in one launch (mgx3dxs_relax_colour_slab2_*) or in two
    } else if (!strcmp(name, "relax3d.resident_tile")) {
        MGX_REQUIRE(value == 0 || value == 8, MGX_ERR_INVALID, "set_param: relax3d.resident_tile = %d not in {0, 8}", value);
        ctx->resident_tile = value;
    } else if (!strcmp(name, "relax3d.resident_min")) {
        MGX_REQUIRE(value >= 1, MGX_ERR_INVALID, "set_param: relax3d.resident_min = %d < 1", value);
        ctx->relax_resident_min = value;
    } else if (!strcmp(name, "rr3d.black")) {
        MGX_REQUIRE(value >= 0 && value <= 2, MGX_ERR_INVALID, "set_param: rr3d.black = %d not in {0, 1, 2}", value);
        ctx->rr_black = value;
    } else if (!strcmp(name, "rr3d.black_waves")) {
        MGX_REQUIRE(value == 0 || value == 8 || value == 12 || value == 16, MGX_ERR_INVALID, "set_param: rr3d.black_waves = %d not in {0, 8, 12, 16}", value);
        ctx->rr_black_waves = value;
    } else if (!strcmp(name, "rr3d.black_abl")) {
#ifdef MGX_DIAGNOSTICS
        ctx->rr_black_abl = value;  // ablation bits of relax_rr3d_xs_kernel: WRONG results
#else
        return mgx::fail(MGX_ERR_INVALID, "set_param: 'rr3d.black_abl' exists only in diagnostic builds (make diag)");
#endif
    } else if (!strcmp(name, "relax3d.fused_ilv")) {
        ctx->sweep_ilv = value ? 1 : 0;  // sweep3d_xs_kernel: memory instructions in groups between the rows of the arithmetic (1) or all first (0)
    } else if (!strcmp(name, "relax3d.fused_mid")) {
        MGX_REQUIRE(value >= 0 && value <= 2, MGX_ERR_INVALID, "set_param: relax3d.fused_mid = %d not in {0, 1, 2}", value);
        ctx->sweep_mid = value;  // 2: rows of 129 points too (slower there than two passes; tests).  cache-resident levels (33 ... 129 points per row): one launch per sweep (sweep3d_xs_mid_kernel)
    } else if (!strcmp(name, "relax3d.fused_dbg")) {
#ifdef MGX_DIAGNOSTICS
        ctx->sweep_dbg = value;  // 1 = cycle stamps, + 2 * ablation bits: WRONG results
#else
        return mgx::fail(MGX_ERR_INVALID, "set_param: 'relax3d.fused_dbg' exists only in diagnostic builds (make diag)");
#endif
    } else if (!strcmp(name, "relax3d.fused_lead")) {
        MGX_REQUIRE(value == 0 || (value >= 5 && value <= 7), MGX_ERR_INVALID, "relax3d.fused_lead (planes the red stage runs ahead) must be 0 (default), 5, 6 or 7");
        ctx->sweep_lead = value;
    } else if (!strcmp(name, "relax3d.unroll")) {
        // the pipelined smoother's step loop unrolled four times with fixed register roles (same loads, stores, arithmetic; measured:
        // tools/level_timing.py).  Bit 0: the correcting red pass, bit 1: the plain pass and the from-zero sweep (2 x 8 / 2 x 4 waves of
        // 2 rows), bit 2: the fp32 two-pair kernels; bits 0 and 1 apply to fp64 only (the fp32 one-pair kernels of the 257^3 level run
        // short runs in many workgroups and lose 10 % unrolled) unless bit 3 is set too (tests); bit 4: the plain pass requests its
        // column and f TWO steps ahead (six steps per loop trip; measured 2 % slower, kept for the record).  Default 7.
        MGX_REQUIRE(value >= 0 && value <= 31, MGX_ERR_INVALID, "set_param: relax3d.unroll = %d not in [0, 31]", value);
        ctx->pipe_unroll = value;
    } else if (!strcmp(name, "relax3d.block3")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: relax3d.block3 = %d not in {0, 1}", value);
        ctx->block3 = (ctx->block3 & ~1) | value;  // bit 0: the way down runs its last three colour passes in one launch (relax3d_xs_block3_kernel)
    } else if (!strcmp(name, "relax3d.block3_up")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: relax3d.block3_up = %d not in {0, 1}", value);
        ctx->block3 = (ctx->block3 & ~2) | (value << 1);  // bit 1: the way up runs its passes B, R, B after R' in one launch
    } else if (!strcmp(name, "relax3d.block3_corr")) {
        MGX_REQUIRE(value == 0 || value == 1, MGX_ERR_INVALID, "set_param: relax3d.block3_corr = %d not in {0, 1}", value);
        ctx->block3 = (ctx->block3 & ~4) | (value << 2);  // bit 2: the way up runs R', B, R as one in-place launch that stores red only
    } else if (!strcmp(name, "relax3d.zchunk")) {
        MGX_REQUIRE(value >= 0, MGX_ERR_INVALID, "relax3d.zchunk must be >= 0 (0 = automatic)");
        ctx->relax_zchunk = value;
    } else {
        return mgx::fail(MGX_ERR_INVALID, "set_param: unknown parameter '%s'", name);
    }
    return MGX_OK;
}

}  // extern "C"
