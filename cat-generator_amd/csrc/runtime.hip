// The library's runtime, no operator: the error string, the option table, the column reductions' scratch pool, the hardware-queue
// probe, and the device / memory / stream / event entry points of catgan.h.
#include "common.h"
#include <stdarg.h>
#include <stdlib.h>
#include <chrono>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace cg {
char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return 1;
}

namespace {
struct OptDef { const char* name; long dflt; };
// order = enum Opt (common.h)
const OptDef kOptDefs[OPT_COUNT] = {
    {"CG_SKINNY", 1}, {"CG_GEMM_BK32", 1}, {"CG_WINO_BK", 0}, {"CG_NN_TILE", 0}, {"CG_TN_TILE", 0}, {"CG_NN_SPLITS", 0}, {"CG_TN_SPLITS", 0},
    {"CG_XCD_SWIZZLE", 7}, {"CG_NN_GLDS", 1}, {"CG_TN_GLDS", 1}, {"CG_WINO_GLDS", 1}, {"CG_PAD_SKIP", 20}, {"CG_WINO3", 1},
    {"CG_WINO_DGRAD_FUSE", 1}, {"CG_WINO_DGRAD_FUSE_LAUNCHES", 0}, {"CG_WINO3_LAUNCHES", 0}, {"CG_PACK_WIDE", 1},
    {"CG_SAMPLER_ATOMIC_LAUNCHES", 0},
};
long g_opt_val[OPT_COUNT];
int g_opt_state[OPT_COUNT];   // 0 = not read yet, 1 = default / environment, 2 = set through the ABI
}  // namespace

void* col_scratch(hipStream_t stream) {
    // a pool of blocks allocated (and their ticket counters zeroed) in chunks of kPool, handed to streams as they appear.  A stream
    // that shows up inside a graph capture (torch.cuda.graph captures on a stream of its own) must find a free block - nothing can
    // be allocated then - so every hand-over outside a capture leaves at least kReserve blocks behind (a plan's side and
    // weight-gradient streams, several nets per process: streams are not scarce any more).
    constexpr int kPool = 8, kReserve = 4;
    static std::unordered_map<hipStream_t, void*> blocks;
    static std::vector<void*> pool;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    auto it = blocks.find(stream);
    if (it != blocks.end()) return it->second;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    const bool capturing = stream && hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
    if (capturing && pool.empty()) {
        cg::fail("column reduce: no scratch block left for a stream first used inside a graph capture (run one pass on it before cg_graph_begin)");
        return nullptr;
    }
    if (!capturing && (int)pool.size() <= kReserve) {
        char* p = nullptr;
        // ANOTHER stream of the process may be inside a graph capture right now (a plan's side / weight-gradient streams make
        // refills frequent): allocation, a memset and a synchronisation are "potentially unsafe" calls that a capture in global mode
        // forbids to every thread - so the refill runs with this thread's capture mode relaxed, and the memset is not on the null stream
        // (which would drag a capturing blocking stream in).  Nothing here touches the capturing stream's work; the blocks are handed
        // out only to streams that are not capturing.
        // No stream of its own for the memset: HIP maps streams onto a handful of hardware queues in creation order, and one more stream
        // moved the training host's side stream onto the main stream's queue (round 5: both generator forwards ran back to back, +2.7 %
        // per step).  The memset goes on the REQUESTING stream - not capturing, we checked - and only that stream is waited for.
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        const bool ok = hipMalloc((void**)&p, kColScratchBytes * kPool) == hipSuccess &&
                        hipMemsetAsync(p, 0, kColScratchBytes * kPool, stream) == hipSuccess &&   // finished before any kernel draws a ticket
                        hipStreamSynchronize(stream) == hipSuccess;
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        if (!ok) {
            (void)hipGetLastError();
            if (pool.empty()) { cg::fail("column reduce: cannot allocate %zu bytes of scratch", kColScratchBytes * kPool); return nullptr; }
        } else
            for (int i = kPool - 1; i >= 0; --i) pool.insert(pool.begin(), p + (size_t)i * kColScratchBytes);   // older blocks go first
    }
    void* blk = pool.back();
    pool.pop_back();
    blocks[stream] = blk;
    return blk;
}
namespace {
__global__ void queue_probe_spin_k(unsigned long long ticks, int* sink) {   // wall_clock64: 100 MHz, independent of the shader clock
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) { }
    if (ticks == ~0ull) *sink = 1;
}
struct QueuePool {
    std::vector<hipStream_t> s;
    std::unordered_map<hipStream_t, std::vector<int>> cls;   // per reference stream: class of every pool stream
    std::mutex mu;
};
QueuePool& qpool() { static QueuePool p; return p; }
constexpr int kQueuePool = 24;

// milliseconds for one spinning kernel on a (and one on b, if b != a's sentinel) to finish
double probe_pair(hipStream_t a, hipStream_t b, bool both, unsigned long long ticks) {
    (void)hipStreamSynchronize(a);
    if (both) (void)hipStreamSynchronize(b);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(queue_probe_spin_k, dim3(1), dim3(64), 0, a, ticks, (int*)nullptr);
    if (both) hipLaunchKernelGGL(queue_probe_spin_k, dim3(1), dim3(64), 0, b, ticks, (int*)nullptr);
    (void)hipStreamSynchronize(a);
    if (both) (void)hipStreamSynchronize(b);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
bool same_queue(hipStream_t a, hipStream_t b) {
    const unsigned long long ticks = 30000;   // 0.3 ms
    int votes = 0;
    for (int r = 0; r < 3; ++r) {
        const double one = probe_pair(a, a, false, ticks), two = probe_pair(a, b, true, ticks);
        if (two > 1.6 * one) ++votes;
    }
    return votes >= 2;
}
}  // namespace

int queue_classify(hipStream_t ref) {     // fills qpool().cls[ref]; caller holds the lock
    QueuePool& p = qpool();
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (ref && hipStreamIsCapturing(ref, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
        return cg::fail("queue_stream: a stream's hardware queue cannot be probed inside a graph capture (run one pass on it before cg_graph_begin)");
    while ((int)p.s.size() < kQueuePool) {
        hipStream_t q;
        if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) return cg::fail("queue_stream: hipStreamCreate failed");
        p.s.push_back(q);
    }
    std::vector<int> c(p.s.size(), -1);
    std::vector<hipStream_t> rep;           // representative of class 1, 2, 3
    for (size_t i = 0; i < p.s.size(); ++i) {
        if (same_queue(ref, p.s[i])) { c[i] = 0; continue; }
        for (size_t k = 0; k < rep.size() && c[i] < 0; ++k)
            if (same_queue(rep[k], p.s[i])) c[i] = (int)k + 1;
        if (c[i] < 0) { rep.push_back(p.s[i]); c[i] = (int)rep.size(); }
    }
    (void)hipGetLastError();
    p.cls[ref] = c;
    return 0;
}

hipStream_t queue_stream(hipStream_t ref, int cls, int slot) {
    QueuePool& p = qpool();
    std::lock_guard<std::mutex> lk(p.mu);
    if (!p.cls.count(ref) && queue_classify(ref)) return nullptr;
    const std::vector<int>& c = p.cls[ref];
    int nclass = 0;
    for (int v : c) nclass = std::max(nclass, v + 1);
    if (nclass < 2) {
        // GPU_MAX_HW_QUEUES=1, a serialising profiler / HIP_LAUNCH_BLOCKING, or a busy shared GPU that skewed the probe: results never
        // depend on the queue class (only the overlap does), so hand out distinct pool streams and say so once
        static bool warned = false;
        if (!warned) { warned = true; fprintf(stderr, "cg: the hardware-queue probe found one queue only - side streams are plain pool streams (overlap not guaranteed)\n"); }
        return p.s[(size_t)((cls & 3) * (kQueuePool / 4) + slot % (kQueuePool / 4)) % p.s.size()];
    }
    cls = cls % nclass;                     // fewer than four queues (GPU_MAX_HW_QUEUES < 4): wrap
    int seen = 0;
    hipStream_t last = nullptr;
    for (size_t i = 0; i < c.size(); ++i)
        if (c[i] == cls) { last = p.s[i]; if (seen++ == slot) return p.s[i]; }
    if (last) return last;                  // more roles than pool streams of this class: share the last one
    cg::fail("queue_stream: no pool stream on hardware queue class %d", cls);
    return nullptr;
}

int queue_class(hipStream_t ref, hipStream_t s) {
    if (s == ref) return 0;
    QueuePool& p = qpool();
    std::lock_guard<std::mutex> lk(p.mu);
    auto it = p.cls.find(ref);
    if (it == p.cls.end()) return -1;
    for (size_t i = 0; i < p.s.size(); ++i) if (p.s[i] == s) return it->second[i];
    return -1;
}

unsigned long g_opt_epoch = 1;   // bumped by cg_set_option: compiled plans (net.hip) re-derive workspace sizes / dispatch-dependent rows
long opt(Opt o) {
    if (g_opt_state[o] == 0) {
        const char* e = getenv(kOptDefs[o].name);
        g_opt_val[o] = e ? atol(e) : kOptDefs[o].dflt;
        g_opt_state[o] = 1;
    }
    return g_opt_val[o];
}
void opt_count(Opt o) { opt(o); ++g_opt_val[o]; }
}  // namespace cg

extern "C" {

int cg_abi_version(void) { return CG_TIMING_PROBE ? -1 : CG_ABI_VERSION; }   // a timing-only build (common.h) is refused by every host
int cg_set_option(const char* name, long value) {
    CG_REQUIRE(name, "cg_set_option: null name");
    for (int i = 0; i < cg::OPT_COUNT; ++i)
        if (strcmp(name, cg::kOptDefs[i].name) == 0) {
            ++cg::g_opt_epoch;
            if (value == -1) { cg::g_opt_state[i] = 0; return 0; }   // back to the environment / built-in default
            cg::g_opt_val[i] = value; cg::g_opt_state[i] = 2;
            return 0;
        }
    return cg::fail("cg_set_option: unknown option %s", name);
}
int cg_get_option(const char* name, long* value) {
    CG_REQUIRE(name && value, "cg_get_option: null pointer");
    for (int i = 0; i < cg::OPT_COUNT; ++i)
        if (strcmp(name, cg::kOptDefs[i].name) == 0) { *value = cg::opt((cg::Opt)i); return 0; }
    return cg::fail("cg_get_option: unknown option %s", name);
}
const char* cg_last_error(void) { return cg::err_buf(); }
int cg_device_count(int* count) { CG_REQUIRE(count, "null"); CG_HIP(hipGetDeviceCount(count)); return 0; }
int cg_set_device(int device) { CG_HIP(hipSetDevice(device)); return 0; }
int cg_malloc(void** dptr, size_t bytes) { CG_REQUIRE(dptr, "null"); CG_HIP(hipMalloc(dptr, bytes)); return 0; }
int cg_free(void* dptr) { CG_HIP(hipFree(dptr)); return 0; }
int cg_memcpy_h2d(void* stream, void* dst, const void* src, size_t bytes) {
    CG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cg::S(stream))); return 0;
}
int cg_memcpy_d2h(void* stream, void* dst, const void* src, size_t bytes) {
    CG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, cg::S(stream)));
    CG_HIP(hipStreamSynchronize(cg::S(stream)));
    return 0;
}
int cg_memcpy_d2d(void* stream, void* dst, const void* src, size_t bytes) {
    CG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, cg::S(stream))); return 0;
}
// 16 bytes per lane, grid-stride: the runtime's fill kernel (hipMemsetAsync -> __amd_rocclr_fillBufferAligned) takes 34 us for the
// 26.7 MB of D's flat gradient (0.8 TB/s) at the head of every fevalD (adversarial.lua:80 zeroes the gradients before the forward pass)
__global__ __launch_bounds__(256) void zero16_k(float4* __restrict__ p, long n16) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    CG_GRID_STRIDE(i, n16) p[i] = z;
}
int cg_memset_zero(void* stream, void* dst, size_t bytes) {
    if (bytes >= (1u << 20) && (uintptr_t)dst % 16 == 0) {     // large, aligned: our own kernel; the tail (< 16 bytes) and small buffers: the runtime
        const long n16 = (long)(bytes / 16);
        CG_EW_LAUNCH(zero16_k, n16, (float4*)dst, n16);
        const size_t done = (size_t)n16 * 16;
        if (done < bytes) CG_HIP(hipMemsetAsync((char*)dst + done, 0, bytes - done, cg::S(stream)));
        return 0;
    }
    CG_HIP(hipMemsetAsync(dst, 0, bytes, cg::S(stream))); return 0;
}
int cg_stream_create(void** stream) {
    CG_REQUIRE(stream, "null");
    hipStream_t s; CG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); *stream = (void*)s; return 0;
}
int cg_stream_on_queue(void* ref_stream, int queue_class, int slot, void** stream) {
    CG_REQUIRE(stream && queue_class >= 0 && slot >= 0, "cg_stream_on_queue: bad arguments");
    hipStream_t s = cg::queue_stream(cg::S(ref_stream), queue_class, slot);
    if (!s) return 1;
    *stream = (void*)s;
    return 0;
}
int cg_stream_destroy(void* stream) { CG_HIP(hipStreamDestroy(cg::S(stream))); return 0; }
int cg_stream_sync(void* stream) { CG_HIP(hipStreamSynchronize(cg::S(stream))); return 0; }

int cg_host_alloc(void** hptr, size_t bytes) {
    CG_REQUIRE(hptr && bytes > 0, "cg_host_alloc: bad arguments");
    CG_HIP(hipHostMalloc(hptr, bytes, hipHostMallocDefault));
    return 0;
}
int cg_host_free(void* hptr) { if (hptr) CG_HIP(hipHostFree(hptr)); return 0; }
int cg_event_create(void** event) {
    CG_REQUIRE(event, "cg_event_create: null pointer");
    hipEvent_t e; CG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); *event = (void*)e; return 0;
}
int cg_event_destroy(void* event) { if (event) CG_HIP(hipEventDestroy((hipEvent_t)event)); return 0; }
int cg_event_record(void* event, void* stream) {
    CG_REQUIRE(event, "cg_event_record: null event");
    CG_HIP(hipEventRecord((hipEvent_t)event, cg::S(stream))); return 0;
}
int cg_event_sync(void* event) {
    CG_REQUIRE(event, "cg_event_sync: null event");
    CG_HIP(hipEventSynchronize((hipEvent_t)event)); return 0;
}
int cg_stream_wait_event(void* stream, void* event) {
    CG_REQUIRE(event, "cg_stream_wait_event: null event");
    CG_HIP(hipStreamWaitEvent(cg::S(stream), (hipEvent_t)event, 0)); return 0;
}
}  // extern "C"
