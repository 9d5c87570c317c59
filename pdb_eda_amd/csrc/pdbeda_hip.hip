// pdbeda_hip.hip -- host side of libpdbeda_hip.so: contexts, device arenas, job setup and the
// extern "C" entry points declared in include/pdbeda.h.  gfx950 only, no CPU fallback.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>

#include <algorithm>
#include <chrono>
#include <thread>
#include <atomic>
#include <random>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "pdbeda_kernels.h"
#include "pdbeda_cloud.h"
#include "pdbeda_jobplan.h"
#include "pdbeda_stage.h"
#include "pdbeda_tile.h"
#include "pdbeda_upload.h"
// the feature headers, in alphabetical order: each one includes what it uses
#include "pdbeda_basins.h"
#include "pdbeda_blobnear.h"
#include "pdbeda_blobshape.h"
#include "pdbeda_contacts.h"
#include "pdbeda_filter.h"
#include "pdbeda_fourier.h"
#include "pdbeda_gradient.h"
#include "pdbeda_model.h"
#include "pdbeda_partition.h"
#include "pdbeda_peaks.h"
#include "pdbeda_pose.h"
#include "pdbeda_profiles.h"
#include "pdbeda_qscore.h"
#include "pdbeda_resample.h"
#include "pdbeda_spread.h"

using namespace pdbeda;

// ------------------------------------------------------------------------------------
// Handles
// ------------------------------------------------------------------------------------
struct pdbeda_ctx;
struct Block {      // a piece of device memory as the pool and the lent list keep it
    char *base = nullptr;
    size_t cap = 0;
};
// A block lent by a context's pool, and its ONE owner: it goes back to that pool when the owner dies, is assigned over, or put() says so -- in stream
// order, without a wait.  Whoever holds an Arena (a local, a map, a job record) releases it by going away: no path has to remember to.
struct Arena : Block {
    pdbeda_ctx *ctx = nullptr;
    Arena() = default;
    Arena(Arena &&o) noexcept : Block(o), ctx(o.ctx) { o.base = nullptr; o.cap = 0; }
    Arena &operator=(Arena &&o) noexcept {
        if (this != &o) { put(); base = o.base; cap = o.cap; ctx = o.ctx; o.base = nullptr; o.cap = 0; }
        return *this;
    }
    ~Arena() { put(); }
    void put();
};

struct pdbeda_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    std::multimap<size_t, Block> pool;  // free device arenas by capacity (reused: no hipMalloc in steady state)
    size_t pool_bytes = 0;              // bytes parked in the pool ...
    size_t pool_cap = (size_t)24 << 30; // ... trimmed (largest first) beyond this (PDBEDA_POOL_CAP_MB): streams x live lists x multi-GB
                                        // whole-map arenas must not creep up on the 288 GB until hipMalloc fails
    double *partials = nullptr;         // reduction partials (N_PARTIAL doubles) + 4 result slots
    char *dev_stage = nullptr;          // device staging block of d2h_many (results packed by k_pack, one copy to the host); handed out until the next ctx_sync
    size_t dev_stage_cap = 0, dev_stage_used = 0;
    // device -> host results are staged through pinned memory: the copies are truly asynchronous (a copy into pageable
    // memory blocks inside the runtime, where no watchdog can see it) and land in the caller's buffers when ctx_sync()
    // has seen the stream drain
    PinnedBlock pinned;
    // file -> device uploads (pdbeda_map_upload_file): the chunks of a map go through the process's upload engine (reader threads
    // with pinned chunks and copy streams of their own); what a context keeps is one event per reader, recorded
    // behind the reader's copies of the map and waited for by the context's stream
    static constexpr int MAX_READERS = 8;
    hipEvent_t reader_ev[MAX_READERS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int live_handles = 0;
    // optional per-kernel timing with HIP events on ctx->stream (bench.py's roofline leg)
    bool profiling = false;
    struct ProfRec { const char *name; hipEvent_t a, b; };
    std::vector<ProfRec> prof;
    std::vector<std::pair<const char *, double>> prof_host;   // host-side phases timed while profiling is on (name, ms): the ordering of a peak list
    // test hooks (environment, read once at creation): PDBEDA_DEBUG_POISON=1 fills every arena with 0xFF bytes when it
    // is handed out (a kernel that trusts recycled memory shows up at once); PDBEDA_DEBUG_EDGE_CAP=n shrinks the
    // cross-tile pair buffer so the shard-overflow path runs on small inputs.
    bool debug_poison = false;
    bool debug_shrink_totals = false;   // PDBEDA_DEBUG_SHRINK_TOTALS=1: the host sizes per-atom sphere batches for HALF their mask words -- what k_make_vols' check of the device's totals is there to catch (tests)
    int64_t debug_edge_cap = 0;
    bool debug_worst_case_arena = false;   // PDBEDA_DEBUG_WORST_CASE_ARENA=1: whole-map jobs are carved for the worst case at once (no second run)
    // per-entry watchdog (multipleStructures.py:359-377 wraps every entry in a SIGALRM timeout; threads cannot): when
    // timeout_s > 0 every wait on the stream is a timed hipStreamQuery loop; a wait that expires marks the context
    // abandoned: every later call fails at once with PDBEDA_ERR_TIMEOUT and destroy does not wait for the stream.
    double timeout_s = 0.0;
    std::chrono::steady_clock::time_point deadline;   // ONE deadline for every wait of the entry: set when the watchdog is (re-)armed
    bool timed_out = false;
    // the pool is touched by its own context's thread, and -- when another context of the process runs out of device memory --
    // by that context's thread, which trims its siblings' pools before it gives up
    std::mutex pool_mu;
    std::map<char *, size_t> lent;      // arenas handed out and not yet returned (maps, jobs): an abandoned context frees them too
    std::map<int, Arena> fft_tables;    // the twiddle table of every line length this context has transformed (pdbeda_fourier_line.h): made once, kept until destroy
};

// Contexts of this process: live ones (a context short of memory trims the arena pools of its siblings) and the ones the
// watchdog abandoned.  An abandoned context cannot be destroyed at once -- its stream may still run, hipFree would hang with
// it -- but leaking its arenas for the life of the process is not an option either: the entries that time out are the large
// ones.  So it is parked here and REAPED (normal destroy path, including the arenas its lost handles still hold) as soon as a
// query finds its stream drained: at every context creation and whenever an allocation fails.
static std::mutex g_ctx_mu;
static std::vector<pdbeda_ctx *> g_live, g_abandoned;

static void ctx_release_device(pdbeda_ctx *ctx, bool lent_too) {
    ctx->fft_tables.clear();      // (back to the pool, which goes next)
    for (auto &kv : ctx->pool) (void)hipFree(kv.second.base);
    ctx->pool.clear();
    ctx->pool_bytes = 0;
    if (lent_too) {
        for (auto &kv : ctx->lent) (void)hipFree(kv.first);
        ctx->lent.clear();
    }
    if (ctx->partials) (void)hipFree(ctx->partials);
    if (ctx->dev_stage) (void)hipFree(ctx->dev_stage);
    if (ctx->pinned.base) (void)hipHostFree(ctx->pinned.base);
    for (int k = 0; k < pdbeda_ctx::MAX_READERS; ++k)
        if (ctx->reader_ev[k]) (void)hipEventDestroy(ctx->reader_ev[k]);
    for (auto &r : ctx->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
}

// Destroy the abandoned contexts whose stream has drained meanwhile; returns how many are still parked.
static size_t reap_abandoned() {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    if (g_abandoned.empty()) return 0;
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;   // (the caller's current device is put back below)
    for (size_t i = 0; i < g_abandoned.size();) {
        pdbeda_ctx *ctx = g_abandoned[i];
        (void)hipSetDevice(ctx->device);
        // still running (or hung) on its stream, or the upload engine still copies into one of its maps: try again later
        bool busy = hipStreamQuery(ctx->stream) == hipErrorNotReady;
        for (int k = 0; k < pdbeda_ctx::MAX_READERS && !busy; ++k)      // (the readers' copies of its last map: behind these events)
            if (ctx->reader_ev[k] && hipEventQuery(ctx->reader_ev[k]) == hipErrorNotReady) busy = true;
        if (busy) { ++i; continue; }
        ctx_release_device(ctx, true);
        delete ctx;
        g_abandoned.erase(g_abandoned.begin() + i);
    }
    if (caller_device >= 0) (void)hipSetDevice(caller_device);
    return g_abandoned.size();
}

// Give the parked arenas of the OTHER live contexts of this device back to the driver (the caller is out of device memory).
static void trim_sibling_pools(pdbeda_ctx *self) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    for (pdbeda_ctx *other : g_live) {
        if (other == self || other->device != self->device) continue;
        std::lock_guard<std::mutex> p(other->pool_mu);
        for (auto &kv : other->pool) (void)hipFree(kv.second.base);
        other->pool.clear();
        other->pool_bytes = 0;
    }
}

struct ProfScope {
    pdbeda_ctx *ctx;
    hipEvent_t b = nullptr;
    ProfScope(pdbeda_ctx *c, const char *name) : ctx(c) {
        if (!ctx->profiling) return;
        hipEvent_t a = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { b = nullptr; return; }
        (void)hipEventRecord(a, ctx->stream);
        ctx->prof.push_back({name, a, b});
    }
    ~ProfScope() { if (b) (void)hipEventRecord(b, ctx->stream); }
};
#define PROF(ctx, name) ProfScope prof_scope_##__LINE__(ctx, name)

struct pdbeda_map {
    pdbeda_ctx *ctx = nullptr;
    const float *dens = nullptr;
    bool own_dens = false;
    Arena arena;                      // geometry (+ the grid when the library owns it): from the context's arena pool, recycled in
                                      // stream order -- a stream pool analysing entry after entry never calls hipMalloc / hipFree
    Geom geom;
    Geom *geom_dev = nullptr;
    int64_t n_vox = 0;
    double fix_mul = 0.0;             // 2^S of the order-independent blob sums (FixSums); 0 = not yet derived from the map's range
    bool fix_refused = false;         // the range pass found a NaN / infinity: labelling calls refuse the map (map_fix_mul)
    double max_abs = 0.0;             // the largest |rho| of the stored map, from the same range pass (valid while fix_mul != 0): pdbeda_atom_moments' quantum
};

// A blob list is a VIEW of a labelling job: the whole job, or one plane of a fused whole-map job (the handle is &job->view[p])
struct LabelJob;
struct pdbeda_bloblist {
    LabelJob *job = nullptr;
    int vol_lo = 0, vol_hi = 0;      // volumes of the job that belong to this list
    int sign = 1;
    bool freed = false;
    int64_t n_voxels = -1;
    // pdbeda_bloblist_moments: the rows of THIS list, made by the first call and kept until the list is freed
    bool shape_done = false;
    std::vector<int32_t> shape_i;      // [blobs][10]: box_lo, box_hi, extreme crs, bits of the extreme value
    std::vector<int64_t> shape_l;      // [blobs][9]: sum d, sum d d'
    std::vector<double> shape_d;       // [blobs][10]: sum w, sum w d, sum w d d'
};

// One record per labelling job, deleted (its arenas go back to the pool with it) when the last of its views is freed
struct LabelJob {
    pdbeda_ctx *ctx = nullptr;
    pdbeda_map *map = nullptr;
    Arena vox_arena;                   // the voxel lists of the job's blobs, made on demand (declared first: it goes back to the pool after the job's arena)
    Arena arena;
    Job job;
    TileDims td;
    bool whole_map = false;
    int32_t *labels_dev = nullptr;     // the signed label volume: inside arena when requested
    bool labels_done = false;
    int64_t *offsets_dev = nullptr;
    int32_t *crs_dev = nullptr;
    unsigned int *cursor_dev = nullptr;
    bool voxels_done = false;
    std::vector<AtomBox> host_boxes;   // a per-atom sphere batch whose boxes the host made: box of atom a (else empty)
    // whole-map jobs: what it takes to run the job again (a typical-size arena that turned out too small: see whole_map_enqueue)
    float cut_pos = 0.0f, cut_neg = 0.0f;
    bool want_pos = false, want_neg = false;
    uint32_t flags = 0;
    bool worst_case = false;           // the run on record has the second run's shape: the worst-case arena and the unit tiles' launches
    int reruns = 0;
    size_t bytes = 0;                  // bytes the job carved out of its arena (a recycled arena may be larger)
    // what the counters said, once read
    bool have_counts = false;
    int64_t n_blobs = 0, n_blobs_vol0 = 0;
    // whole-map jobs: the first rows of the job's blob table, fetched WITH the counters (round 5: the count and the table of
    // each of the two lists of a fused call were four waits; now one serves both)
    int64_t spec_rows = 0;
    std::vector<int64_t> spec_n, spec_key;
    std::vector<double> spec_total, spec_centroid, spec_center, spec_volume;
    std::vector<int32_t> spec_group;
    int live = 0;                      // views not yet freed
    pdbeda_bloblist view[2];
};

static const int N_PARTIAL = 2048;

static int fail(pdbeda_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    // results of a failed call are never delivered.  The staging regions are NOT handed out again here: copies queued by an
    // earlier call (a sphere batch's staged inputs) may still read them -- only ctx_sync(), which has drained the stream, rewinds
    if (ctx) ctx->pinned.drop_deliveries();
    if (ctx && ctx->timed_out) return PDBEDA_ERR_TIMEOUT;   // (the watchdog's message stays)
    if (ctx) ctx->err = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, PDBEDA_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Wait for the context's stream: plain hipStreamSynchronize, or (watchdog armed) a timed query loop; then deliver the
// staged device -> host results.
// (round 6, measured and dropped: polling the stream for the first 300 us of a wait without a watchdog instead of hipStreamSynchronize at once --
//  the analysis entry 3.07 against 3.02 ms, the pools inside their noise: the runtime's own wait is not where an entry's waits lose time)
static hipError_t ctx_wait(pdbeda_ctx *ctx) {
    if (ctx->timed_out) return hipErrorNotReady;
    if (ctx->timeout_s <= 0.0) return hipStreamSynchronize(ctx->stream);
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q != hipErrorNotReady) return q;
        if (spins > 256) {   // first ~0.3 ms: busy poll (the usual wait is tens of microseconds), then back off
            if (std::chrono::steady_clock::now() > ctx->deadline) {   // the entry's ONE deadline: an entry makes dozens of waits
                ctx->timed_out = true;
                ctx->err = "watchdog: the stream did not drain within the per-entry time-out; context abandoned";
                return hipErrorNotReady;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(spins > 4096 ? 200 : 20));
        }
    }
}

// The small staged copies of a call (inputs through the pinned block, results into it) are KERNELS that read / write the pinned block over the
// link, not hipMemcpyAsync (round 5).  A copy of a few hundred bytes is a packet on the SDMA engine, where it waits behind every 4-8 MiB chunk the
// upload engine has queued (up to 0.46 ms), and each hop between the compute queue and the copy engine is a semaphore: the analysis of a resident
// entry 0.48 -> 0.44 ms alone, 0.68-0.80 -> 0.60 beside two uploading threads; four workers 41.6 k -> 44.5 k entries/min.  PDBEDA_COPY_KERNELS=0: the
// runtime's copies (A/B).
// The two kinds of PDBEDA_* switch (a caller keeps the answer in a function-local static: read once per process, on first use): an A/B switch is on
// unless it is set to 0; a debug / trace hook is off unless it is set to something else than 0.
static bool env_unless_0(const char *name) { const char *e = getenv(name); return !(e && e[0] == '0'); }
static bool env_set(const char *name) { const char *e = getenv(name); return e && e[0] && e[0] != '0'; }
static bool copy_kernels() { static const bool v = env_unless_0("PDBEDA_COPY_KERNELS"); return v; }
static hipError_t copy_by_kernel(pdbeda_ctx *ctx, void *dst, const void *src, size_t bytes) {
    hipLaunchKernelGGL(k_copy_bytes, dim3((unsigned)std::min<size_t>((bytes >> 12) + 1, 64)), dim3(256), 0, ctx->stream, (const unsigned char *)src, (unsigned char *)dst,
                       (unsigned long long)bytes);
    return hipGetLastError();
}

static hipError_t ctx_sync(pdbeda_ctx *ctx) {
    const hipError_t e = ctx_wait(ctx);
    if (e == hipSuccess) ctx->pinned.rewind_delivering(); else ctx->pinned.rewind();
    ctx->dev_stage_used = 0;
    return e;
}

// The pinned block's allocator is PinnedBlock (pdbeda_stage.h); these forward to the context's block.
static inline size_t pinned_span(size_t bytes) { return PinnedBlock::span(bytes); }
static inline size_t pinned_room(const pdbeda_ctx *ctx) { return ctx->pinned.room(); }
static inline void pinned_deliver(pdbeda_ctx *ctx, const char *from, void *dst, size_t bytes) { ctx->pinned.deliver(from, dst, bytes); }
static inline char *pinned_take(pdbeda_ctx *ctx, size_t bytes, void *deliver_to = nullptr) { return ctx->pinned.take(bytes, deliver_to); }
static inline void pinned_untake(pdbeda_ctx *ctx, const char *first) { ctx->pinned.untake(first); }
// The copy between a take and device memory (by kernel, or PDBEDA_COPY_KERNELS=0: by the runtime); a take whose copy could not be launched is handed back.
static hipError_t stage_copy(pdbeda_ctx *ctx, char *stage, void *dev, size_t bytes, bool to_device) {
    void *dst = to_device ? dev : stage, *src = to_device ? stage : dev;
    const hipError_t e = copy_kernels() ? copy_by_kernel(ctx, dst, src, bytes) : hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) pinned_untake(ctx, stage);
    return e;
}

// Device -> host copy of a result, complete after the next ctx_sync(): staged through the pinned buffer when it fits,
// otherwise the stream is drained first (timed) so that the blocking copy into pageable memory has nothing to wait for.
static hipError_t d2h(pdbeda_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    if (char *stage = pinned_take(ctx, bytes, dst)) return stage_copy(ctx, stage, const_cast<void *>(src), bytes, false);
    hipError_t e = ctx_sync(ctx);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    return e;
}

static int arena_get_raw(pdbeda_ctx *ctx, size_t bytes, Arena *out);

static int arena_get(pdbeda_ctx *ctx, size_t bytes, Arena *out) {
    int rc = arena_get_raw(ctx, bytes, out);
    if (rc == 0 && ctx->debug_poison) HIP_TRY(ctx, hipMemsetAsync(out->base, 0xFF, out->cap, ctx->stream));
    return rc;
}

static int arena_get_raw(pdbeda_ctx *ctx, size_t bytes, Arena *out) {      // (*out is empty)
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    bytes = align_up(std::max<size_t>(bytes, 256));
    out->ctx = ctx;
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        auto it = ctx->pool.lower_bound(bytes);
        if (it != ctx->pool.end() && it->first <= bytes * 2 + (1u << 20)) {
            static_cast<Block &>(*out) = it->second;
            ctx->pool_bytes -= it->second.cap;
            ctx->pool.erase(it);
            ctx->lent[out->base] = out->cap;
            return 0;
        }
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        {   // drop the cache and retry
            std::lock_guard<std::mutex> g(ctx->pool_mu);
            for (auto &kv : ctx->pool) (void)hipFree(kv.second.base);
            ctx->pool.clear();
            ctx->pool_bytes = 0;
        }
        e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {   // then what abandoned contexts still hold, then what the sibling contexts have parked
            reap_abandoned();
            trim_sibling_pools(ctx);
            e = hipMalloc(&p, bytes);
        }
        if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_MEMORY, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    out->base = (char *)p;
    out->cap = bytes;
    std::lock_guard<std::mutex> g(ctx->pool_mu);
    ctx->lent[out->base] = out->cap;
    return 0;
}

// Back to the pool: recycled in stream order (whoever gets the block next is enqueued on the context's stream behind its last user), never a wait.
void Arena::put() {
    if (!base) return;
    std::lock_guard<std::mutex> g(ctx->pool_mu);
    ctx->lent.erase(base);
    ctx->pool.emplace(cap, Block{base, cap});
    ctx->pool_bytes += cap;
    base = nullptr;
    cap = 0;
    while (ctx->pool_bytes > ctx->pool_cap && !ctx->pool.empty() && !ctx->timed_out) {   // trim: the largest parked arena goes back to the
        auto last = std::prev(ctx->pool.end());                                            // driver (hipFree waits for the device: rare by design)
        ctx->pool_bytes -= last->second.cap;
        (void)hipFree(last->second.base);
        ctx->pool.erase(last);
    }
}

// An arena sized by `carve` and laid out by the same carve, moved into *out (what *out held goes back to the pool first).  A failure -- a second pass
// that does not end where the first did: the carve read something that changed in between -- leaves *out as it was and nothing behind.
// The ownership rule: an Arena is released by its owner going away.  An explicit put() stands only where the TIME of the release is the point, with a
// comment that says why.
template <typename Carve>
static int arena_carve(pdbeda_ctx *ctx, const char *site, Arena *out, Carve carve) {
    Carver size(nullptr);
    carve(size);
    Arena a;
    if (int rc = arena_get(ctx, size.off, &a)) return rc;
    Carver cv(a.base);
    carve(cv);
    if (cv.off != size.off || cv.off > a.cap) return fail(ctx, PDBEDA_ERR_STATE, "%s: scratch carve ends at %zu, sized %zu (arena of %zu)", site, cv.off, size.off, a.cap);
    *out = std::move(a);
    return 0;
}

static inline unsigned grid_for(int64_t n, int block, int64_t cap = 1 << 20) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// Several small inputs that sit in a row in device scratch (consecutive Carver takes), in ONE copy: laid out in the pinned
// staging block as on the device; one by one from the caller's memory when the block has no room (the caller waits before it
// returns either way).
struct H2DItem { void *dst; const void *src; size_t bytes; };
static hipError_t h2d_row(pdbeda_ctx *ctx, const H2DItem *items, int n, size_t max_span = H2D_ROW_SPAN) {
    char *lo = nullptr, *hi = nullptr;
    for (int k = 0; k < n; ++k) {
        if (items[k].bytes == 0) continue;
        char *d = (char *)items[k].dst;
        if (!lo || d < lo) lo = d;
        if (!hi || d + items[k].bytes > hi) hi = d + items[k].bytes;
    }
    if (!lo) return hipSuccess;
    const size_t span = (size_t)(hi - lo);
    if (char *stage = span <= max_span ? pinned_take(ctx, span) : nullptr) {
        const StagedRow row{stage, lo, span};
        for (int k = 0; k < n; ++k) row.put(items[k].dst, items[k].src, items[k].bytes);
        return stage_copy(ctx, stage, lo, span, true);
    }
    for (int k = 0; k < n; ++k) {
        if (items[k].bytes == 0) continue;
        const hipError_t e = hipMemcpyAsync(items[k].dst, items[k].src, items[k].bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

static hipError_t h2d_one(pdbeda_ctx *ctx, void *dst, const void *src, size_t bytes) {
    const H2DItem in[1] = {{dst, src, bytes}};
    return h2d_row(ctx, in, 1);
}

// Several results of one call, complete after the next ctx_sync(): packed on the device (k_pack) and brought over in ONE copy
// when they fit the staging blocks, else one by one (d2h).  Items with a null destination or no bytes are skipped.
struct D2HItem { void *dst; const void *src; size_t bytes; };
static hipError_t d2h_each(pdbeda_ctx *ctx, const D2HItem *items, int n) {      // (one by one)
    for (int k = 0; k < n; ++k)
        if (items[k].dst && items[k].bytes)
            if (const hipError_t e = d2h(ctx, items[k].dst, items[k].src, items[k].bytes)) return e;
    return hipSuccess;
}
static hipError_t d2h_many(pdbeda_ctx *ctx, const D2HItem *items, int n_items) {
    int live[8], n = 0;
    size_t total = 0;
    bool packable = (ctx->dev_stage != nullptr || copy_kernels()) && ctx->pinned.base != nullptr;
    for (int k = 0; k < n_items; ++k) {
        if (!items[k].dst || items[k].bytes == 0) continue;
        if (n == 8 || (items[k].bytes & 3u) || ((uintptr_t)items[k].src & 3u)) { packable = false; break; }
        live[n++] = k;
        total += pinned_span(items[k].bytes);
    }
    const bool via_dev_stage = !copy_kernels();      // (with copy kernels k_pack writes straight into the pinned block: nothing is staged on the device)
    if (packable && n >= 2 && (!via_dev_stage || ctx->dev_stage_used + total <= ctx->dev_stage_cap) && total <= pinned_room(ctx)) {
        PackArgs a;
        memset(&a, 0, sizeof a);
        a.n = n;
        size_t words = 0;
        char *pack = nullptr;      // (the items' takes lie in a row: `total` bytes from the first)
        for (int j = 0; j < n; ++j) {
            const D2HItem &it = items[live[j]];
            char *p = pinned_take(ctx, it.bytes, it.dst);
            if (j == 0) pack = p;
            a.seg[j].src = reinterpret_cast<const uint32_t *>(it.src);
            a.seg[j].words = it.bytes / 4;
            a.seg[j].dst_word = (size_t)(p - pack) / 4;
            words = std::max<size_t>(words, it.bytes / 4);
        }
        char *block = copy_kernels() ? pack : ctx->dev_stage + ctx->dev_stage_used;   // (packed straight into the pinned block)
        hipLaunchKernelGGL(k_pack, dim3(grid_for((int64_t)words, 256, 256)), dim3(256), 0, ctx->stream, a, reinterpret_cast<uint32_t *>(block));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && !copy_kernels()) e = hipMemcpyAsync(pack, block, total, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) { pinned_untake(ctx, pack); return e; }
        if (via_dev_stage) ctx->dev_stage_used += total;
        return hipSuccess;
    }
    return d2h_each(ctx, items, n_items);
}

// ------------------------------------------------------------------------------------
// Small batched helpers: stage host arrays through a scratch arena
// ------------------------------------------------------------------------------------
// Round 6: small results and single-touch inputs without copy launches.  pinned_out: a result array that a kernel writes STRAIGHT into the context's pinned
// block (delivered to `dst` by the next ctx_sync); pinned_in: an input that every thread reads once, staged in the pinned block and read by the kernel over the
// link.  nullptr: no room, or PDBEDA_COPY_KERNELS=0 (kernels do not touch host memory then) -- the caller stages on the device and copies as before.
// (An input that threads read many times -- the atoms of a nearest-atom search -- belongs in device memory: a copy launch is cheaper than the link.)
template <typename T>
static T *pinned_out(pdbeda_ctx *ctx, T *dst, size_t count) {
    const size_t bytes = sizeof(T) * count;
    if (!copy_kernels() || !dst || bytes == 0) return nullptr;
    return reinterpret_cast<T *>(pinned_take(ctx, bytes, dst));
}
template <typename T>
static const T *pinned_in(pdbeda_ctx *ctx, const T *src, size_t count) {
    const size_t bytes = sizeof(T) * count;
    if (!copy_kernels() || !src || bytes == 0) return nullptr;
    char *p = pinned_take(ctx, bytes);
    if (p) memcpy(p, src, bytes);
    return reinterpret_cast<const T *>(p);
}
// A result slot {host, count[, dev]}: `count` items for the caller's `host` array, and a device piece -- carve()d with the call's scratch, or given -- for
// when the block has no room.  at(): where the kernel writes -- the pinned take if pinned_out grants one, else the device piece; nullptr when the caller
// passed no array (the kernel skips that result).  finish(): the copy, queued only when the device piece was used.  Call at() in the order of the takes.
template <typename T>
struct Result {
    T *host;
    size_t count;
    T *dev = nullptr, *pin = nullptr;
    void carve(Carver &cv) { cv.take(dev, count); }
    T *at(pdbeda_ctx *ctx) { return !host ? nullptr : (pin = pinned_out(ctx, host, count)) ? pin : dev; }
    hipError_t finish(pdbeda_ctx *ctx) const { return host && !pin ? d2h(ctx, host, dev, sizeof(T) * count) : hipSuccess; }
};
// An input slot, the same way: send() stages the caller's array in the block when pinned_in grants a take, else copies it into the device piece; the kernel reads at `at`.
template <typename T>
struct Input {
    const T *host;
    size_t count;
    T *dev = nullptr;
    const T *at = nullptr;
    void carve(Carver &cv) { cv.take(dev, count); }
    hipError_t send(pdbeda_ctx *ctx) {
        if ((at = pinned_in(ctx, host, count)) != nullptr) return hipSuccess;
        at = dev;
        return h2d_one(ctx, dev, host, sizeof(T) * count);
    }
};

// Scratch for one call, laid out by `carve` (see Carver), which fills the caller's pointers; `fn` uses them; the stream is drained before the arena goes back.
template <typename Carve, typename Fn>
static int with_scratch(pdbeda_ctx *ctx, const char *site, Carve carve, Fn fn) {
    Arena a;
    int rc = arena_carve(ctx, site, &a, carve);
    if (rc) return rc;
    rc = fn();
    hipError_t e = ctx_sync(ctx);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "stream sync: %s", hipGetErrorString(e));
    return 0;
}
// One plain buffer of `bytes`: nothing to lay out.
template <typename Fn>
static int with_scratch(pdbeda_ctx *ctx, size_t bytes, Fn fn) {
    char *base = nullptr;
    return with_scratch(ctx, "scratch", [&](Carver &cv) { cv.take(base, bytes); }, [&]() -> int { return fn(base); });
}

// ------------------------------------------------------------------------------------
// Library / context
// ------------------------------------------------------------------------------------
extern "C" const char *pdbeda_version(void) { return "pdbeda-hip 0.1 (gfx950)"; }

extern "C" int pdbeda_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int pdbeda_device_pci_address(int device_id, char *out, int out_len) {
    if (!out || out_len < 16) return PDBEDA_ERR_ARGUMENT;
    out[0] = 0;
    if (hipDeviceGetPCIBusId(out, out_len, device_id) != hipSuccess) { (void)hipGetLastError(); return PDBEDA_ERR_DEVICE; }
    return PDBEDA_OK;
}

extern "C" int pdbeda_ctx_create_on_stream(int device_id, void *hip_stream, pdbeda_ctx **out) {
    if (!out) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return PDBEDA_ERR_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return PDBEDA_ERR_DEVICE;
    pdbeda_ctx *ctx = new pdbeda_ctx();
    ctx->device = device_id;
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
    } else {
        // (plain priority, like the upload engine's copy streams: r05 tried the contexts' streams above the copy streams -- with
        //  several PROCESSES on one GPU any mix of priorities took an entry from 1.4 to 9-15 ms)
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return PDBEDA_ERR_DEVICE; }
        ctx->own_stream = true;
    }
    if (hipMalloc((void **)&ctx->partials, sizeof(double) * (2 * N_PARTIAL + 8)) != hipSuccess) {
        if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return PDBEDA_ERR_MEMORY;
    }
    // (coherent + mapped, explicitly: with PDBEDA_COPY_KERNELS the staged results are WRITTEN BY KERNELS into this block and read by the host after the
    //  stream wait -- or after a hipStreamQuery poll under the watchdog --, which is only right for coherent host memory)
    if (hipHostMalloc((void **)&ctx->pinned.base, PINNED_BLOCK_BYTES, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess) ctx->pinned.cap = PINNED_BLOCK_BYTES;   // (without it results are copied directly)
    else (void)hipGetLastError();
    if (ctx->pinned.cap && hipMalloc((void **)&ctx->dev_stage, DEV_STAGE_BYTES) == hipSuccess) ctx->dev_stage_cap = DEV_STAGE_BYTES; else { ctx->dev_stage = nullptr; (void)hipGetLastError(); }
    ctx->debug_poison = env_set("PDBEDA_DEBUG_POISON");
    ctx->debug_shrink_totals = env_set("PDBEDA_DEBUG_SHRINK_TOTALS");
    if (const char *v = getenv("PDBEDA_DEBUG_EDGE_CAP")) ctx->debug_edge_cap = atoll(v);
    ctx->debug_worst_case_arena = env_set("PDBEDA_DEBUG_WORST_CASE_ARENA");
    if (const char *v = getenv("PDBEDA_POOL_CAP_MB")) ctx->pool_cap = (size_t)std::max<long long>(atoll(v), 0) << 20;
    reap_abandoned();   // (what the watchdog left behind earlier may have drained by now)
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_live.push_back(ctx);
    }
    *out = ctx;
    return PDBEDA_OK;
}

extern "C" int pdbeda_ctx_create(int device_id, pdbeda_ctx **out) { return pdbeda_ctx_create_on_stream(device_id, nullptr, out); }

extern "C" int pdbeda_ctx_destroy(pdbeda_ctx *ctx) {
    if (!ctx) return PDBEDA_ERR_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_live.erase(std::remove(g_live.begin(), g_live.end(), ctx), g_live.end());
        // abandoned by the watchdog: its stream may never drain, and hipFree would hang with it -- parked, and reaped (with the
        // arenas of the maps / jobs its entry left behind) once a query finds the stream empty; leaked only if it never drains
        if (ctx->timed_out) g_abandoned.push_back(ctx);
    }
    if (ctx->timed_out) {
        reap_abandoned();
        return PDBEDA_OK;
    }
    (void)ctx_sync(ctx);
    ctx->fft_tables.clear();      // (the context's own arenas are not a caller's lost handle)
    const bool lost = ctx->live_handles == 0 && !ctx->lent.empty();   // (no handle is alive and an arena is still out: the library itself lost it)
    ctx_release_device(ctx, false);   // (arenas still lent belong to live handles of the caller)
    delete ctx;
    return lost ? PDBEDA_ERR_STATE : PDBEDA_OK;
}

extern "C" int pdbeda_ctx_synchronize(pdbeda_ctx *ctx) {
    if (!ctx) return PDBEDA_ERR_ARGUMENT;
    HIP_TRY(ctx, ctx_sync(ctx));
    return PDBEDA_OK;
}

extern "C" int pdbeda_ctx_profile_begin(pdbeda_ctx *ctx) {
    if (!ctx) return PDBEDA_ERR_ARGUMENT;
    for (auto &r : ctx->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    ctx->prof.clear();
    ctx->prof_host.clear();
    ctx->profiling = true;
    return PDBEDA_OK;
}

// Stops profiling, synchronises, and writes "name calls total_ms\n" lines into buf.
extern "C" int pdbeda_ctx_profile_end(pdbeda_ctx *ctx, char *buf, int64_t cap) {
    if (!ctx || !buf || cap <= 0) return PDBEDA_ERR_ARGUMENT;
    ctx->profiling = false;
    HIP_TRY(ctx, ctx_sync(ctx));
    std::map<std::string, std::pair<int64_t, double>> agg;
    for (auto &r : ctx->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { auto &e = agg[r.name]; e.first++; e.second += ms; }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    ctx->prof.clear();
    for (auto &h : ctx->prof_host) { auto &e = agg[h.first]; e.first++; e.second += h.second; }
    ctx->prof_host.clear();
    std::string out;
    char line[160];
    for (auto &kv : agg) {
        snprintf(line, sizeof line, "%s %lld %.6f\n", kv.first.c_str(), (long long)kv.second.first, kv.second.second);
        out += line;
    }
    if ((int64_t)out.size() + 1 > cap) return fail(ctx, PDBEDA_ERR_CAPACITY, "profile buffer too small");
    memcpy(buf, out.c_str(), out.size() + 1);
    return PDBEDA_OK;
}

extern "C" int pdbeda_ctx_set_timeout(pdbeda_ctx *ctx, double seconds) {
    if (!ctx || !(seconds >= 0.0)) return PDBEDA_ERR_ARGUMENT;
    ctx->timeout_s = seconds;
    ctx->deadline = std::chrono::steady_clock::now() + std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(seconds));
    return PDBEDA_OK;
}

extern "C" int64_t pdbeda_reap_abandoned(void) { return (int64_t)reap_abandoned(); }

extern "C" void *pdbeda_ctx_stream(pdbeda_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" const char *pdbeda_last_error(pdbeda_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// ------------------------------------------------------------------------------------
// Maps
// ------------------------------------------------------------------------------------
static int fill_geom(pdbeda_ctx *ctx, const pdbeda_geometry *in, Geom *g) {
    for (int k = 0; k < 3; ++k) {
        g->ncrs[k] = in->ncrs[k];
        g->crs_start[k] = in->crs_start[k];
        g->xyz_interval[k] = in->xyz_interval[k];
        g->map2xyz[k] = in->map2xyz[k];
        g->map2crs[k] = in->map2crs[k];
        g->origin[k] = in->origin[k];
        g->grid_len[k] = in->grid_len[k];
        if (in->ncrs[k] <= 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "ncrs[%d] = %d", k, in->ncrs[k]);
        if (in->xyz_interval[k] <= 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "xyz_interval[%d] = %d", k, in->xyz_interval[k]);
        if (in->map2xyz[k] < 0 || in->map2xyz[k] > 2 || in->map2crs[k] < 0 || in->map2crs[k] > 2)
            return fail(ctx, PDBEDA_ERR_ARGUMENT, "axis map out of range");
    }
    for (int k = 0; k < 9; ++k) { g->ortho[k] = in->ortho[k]; g->deortho[k] = in->deortho[k]; }
    g->orthogonal = in->orthogonal;
    g->unit_volume = in->unit_volume;
    for (int k = 0; k < 3; ++k) {
        g->crs_interval[k] = g->xyz_interval[g->map2crs[k]];                  // ccp4.py:237
        g->unique_ncrs[k] = std::min(g->ncrs[k], g->crs_interval[k]);         // ccp4.py:262-269
    }
    return 0;
}

static int stats_enqueue(pdbeda_map *m, double *chunk_sums, double host[2], double range[2], bool want_range, bool with_geom = false);
// stats_enqueue's scratch: three doubles per numpy chunk of the map
static int stats_carve(pdbeda_map *m, Arena *out, double *&chunk_sums) {
    return arena_carve(m->ctx, "map statistics", out, [&](Carver &cv) { cv.take(chunk_sums, 3 * (size_t)std::max<int64_t>(m->n_vox / NP_CHUNK, 1)); });
}
static bool stats_carries_geom(const pdbeda_map *m) { return m->n_vox / NP_CHUNK > 0; }      // (the chain's first launch exists: it brings the geometry along when asked to)
static void range_apply(pdbeda_map *m, const double range[2]);

// A map the library makes, until it is the caller's: the record on a geometry and ONE arena that holds the device's copy of the geometry and (voxels)
// the grid, which the call then writes; make() sets dens and own_dens of a map with voxels (a borrowing maker sets dens itself).  geometry_up() queues
// the geometry's copy (it reads the record: a wait comes before the call returns); publish() counts the handle and writes *out, when nothing can fail
// any more.  A map that is never published goes back to the pool with its arena when the MadeMap goes away.
struct MadeMap {
    std::unique_ptr<pdbeda_map> m;
    float *dens = nullptr;
    double stats[2] = {0.0, 0.0}, range[2] = {0.0, 0.0};      // an uploaded map's mean / std and range, from the wait that completes the upload
    Arena stats_scratch;
    int make(pdbeda_ctx *ctx, const char *site, const Geom &geom, int64_t n_vox, bool voxels = true) {
        m.reset(new pdbeda_map());
        m->ctx = ctx;
        m->geom = geom;
        m->n_vox = n_vox;
        const int rc = arena_carve(ctx, site, &m->arena, [&](Carver &cv) { cv.take(m->geom_dev, 1); if (voxels) cv.take(dens, (size_t)n_vox); });
        if (rc == 0 && voxels) { m->dens = dens; m->own_dens = true; }
        return rc;
    }
    int make_like(const char *site, const pdbeda_map *like) { return make(like->ctx, site, like->geom, like->n_vox); }
    hipError_t geometry_up() { return h2d_one(m->ctx, m->geom_dev, &m->geom, sizeof(Geom)); }
    hipError_t stats_up(bool with_geom) {      // (queued behind the upload; filled by the next wait)
        double *chunk_sums = nullptr;
        if (stats_carve(m.get(), &stats_scratch, chunk_sums) != 0) return hipErrorOutOfMemory;
        return stats_enqueue(m.get(), chunk_sums, stats, range, true, with_geom) != 0 ? hipErrorUnknown : hipSuccess;
    }
    void stats_out(double *mean, double *std) { range_apply(m.get(), range); if (mean) *mean = stats[0]; if (std) *std = stats[1]; }
    void publish(pdbeda_map **out) { m->ctx->live_handles++; *out = m.release(); }
};

// A second map beside a grid (a first map's, or the one a call is about to make): of the call's context, and of the grid's shape (units: the unique
// boxes count too).  0, or the refusal; `what` words the refusal of the shape.
static int same_grid(pdbeda_ctx *ctx, const Geom &g, int64_t n_vox, const pdbeda_map *b, const char *what = "maps of different shapes", bool units = false) {
    if (b->ctx != ctx) return fail(ctx, PDBEDA_ERR_ARGUMENT, "maps of different contexts");
    if (b->n_vox != n_vox || memcmp(g.ncrs, b->geom.ncrs, sizeof g.ncrs) != 0 || (units && memcmp(g.unique_ncrs, b->geom.unique_ncrs, sizeof g.unique_ncrs) != 0))
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s", what);
    return 0;
}

static int map_create(pdbeda_ctx *ctx, const float *host, const float *dev, const pdbeda_geometry *geom, pdbeda_map **out, double *mean = nullptr, double *std = nullptr) {
    if (!ctx || !geom || !out || (!host && !dev)) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Geom g;
    int rc = fill_geom(ctx, geom, &g);
    if (rc) return rc;
    const int64_t n_vox = (int64_t)geom->ncrs[0] * geom->ncrs[1] * geom->ncrs[2];
    if (n_vox >= (1ll << 32)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "grids of 2^32 voxels or more are not supported");
    if (dev && ((uintptr_t)dev & 15u) != 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "device density pointer must be 16-byte aligned");
    MadeMap made;
    rc = made.make(ctx, "map_create", g, n_vox, host != nullptr);
    if (rc) return rc;
    pdbeda_map *m = made.m.get();
    hipError_t e = hipSuccess;
    if (host) {
        // (measured, round 5: the same grid through the upload engine -- readers memcpy chunks into their pinned slots -- takes twice as long as the runtime's
        //  own copy from pageable memory, which pins the caller's pages and lets the engine read them in place: 0.6 against 0.3 ms for 8 MB)
        e = hipMemcpyAsync(made.dens, host, sizeof(float) * (size_t)n_vox, hipMemcpyHostToDevice, ctx->stream);
    } else {
        m->dens = dev;      // (borrowed: the map owns its geometry alone)
    }
    // (an uploaded map with its statistics from the same wait: see upload_file_impl; the geometry rides in the statistics' first launch then)
    const bool with_stats = (mean || std) && host && e == hipSuccess;
    const bool geom_in_stats = with_stats && stats_carries_geom(m);
    if (e == hipSuccess && !geom_in_stats) e = made.geometry_up();
    if (with_stats && e == hipSuccess) e = made.stats_up(geom_in_stats);      // (a failed geometry copy stays the call's error)
    {
        const hipError_t e2 = ctx_sync(ctx);  // host buffers may be released on return
        if (e == hipSuccess) e = e2;
    }
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "map upload: %s", hipGetErrorString(e));
    if (with_stats) made.stats_out(mean, std);
    made.publish(out);
    return PDBEDA_OK;
}

extern "C" int pdbeda_map_upload(pdbeda_ctx *ctx, const float *density, const pdbeda_geometry *geom, pdbeda_map **out) {
    return map_create(ctx, density, nullptr, geom, out);
}
extern "C" int pdbeda_map_upload_stats(pdbeda_ctx *ctx, const float *density, const pdbeda_geometry *geom, pdbeda_map **out, double *mean, double *std) {
    return map_create(ctx, density, nullptr, geom, out, mean, std);
}
extern "C" int pdbeda_map_from_device(pdbeda_ctx *ctx, const float *density_dev, const pdbeda_geometry *geom, pdbeda_map **out) {
    return map_create(ctx, nullptr, density_dev, geom, out);
}

// Wait for an event of the context's stream with the watchdog's rules (see ctx_wait).
static hipError_t event_wait(pdbeda_ctx *ctx, hipEvent_t ev) {
    if (ctx->timed_out) return hipErrorNotReady;
    if (ctx->timeout_s <= 0.0) return hipEventSynchronize(ev);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        if (spins > 256) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > ctx->timeout_s) {
                ctx->timed_out = true;
                ctx->err = "watchdog: the stream did not drain within the per-entry time-out; context abandoned";
                return hipErrorNotReady;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
}

// The grid of a CCP4 file straight into HBM: pread() fills pinned chunks while earlier ones are on their way over PCIe, and
// no host copy of the map is ever made (ccp4.py:77-127 unpacks it into a Python tuple).  The readers are the PROCESS's (UploadEngine,
// pdbeda_upload.h: three threads, two pinned chunks and a copy stream each); rounds 3-4 gave every context a ring and two readers of its own.
// A thread copies out of the page cache at 20-40 GB/s (by host), one copy engine moves 54 GB/s: one 32 MB map alone arrives in 0.76-0.85 ms,
// four loads in flight move 50-53 GB/s (`tools/exp/single_load.py`, `trace_load.sh`; a pageable copy out of an mmap of the file runs at link
// speed only while its pages stay mapped -- a fresh mapping per file pays 0.6 ms of page faults per 32 MB before the first byte moves).
// byteswap: the file has the other endianness.
//
// Round 6: the engine itself lives in pdbeda_upload.h and reaches the runtime through a table of function pointers -- the HIP calls below
// here, a host stand-in in tests/upload_harness.cpp, where the engine runs under ThreadSanitizer and AddressSanitizer (tools/sanitize_cpu.sh).
using pdbeda_upload::UploadEngine;
using pdbeda_upload::UploadLoad;
using pdbeda_upload::now_s;
using pdbeda_upload::upload_trace;
static_assert(pdbeda_ctx::MAX_READERS == pdbeda_upload::MAX_READERS, "a context keeps one event per reader");
static int up_code(hipError_t e) { return e == hipSuccess ? pdbeda_upload::UP_OK : (e == hipErrorNotReady ? pdbeda_upload::UP_NOT_READY : (int)e); }
static hipError_t up_error(int code) { return code == pdbeda_upload::UP_OK ? hipSuccess : (code < 0 ? hipErrorUnknown : (hipError_t)code); }
static const pdbeda_upload::Backend g_hip_backend = {
    [](int device) { return up_code(hipSetDevice(device)); },
    [](pdbeda_upload::Stream *out) { hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); if (e != hipSuccess) (void)hipGetLastError(); *out = (void *)s; return up_code(e); },
    [](void **out, size_t bytes) { const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault); if (e != hipSuccess) (void)hipGetLastError(); return up_code(e); },
    [](pdbeda_upload::Event *out) { hipEvent_t ev = nullptr; const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); if (e != hipSuccess) (void)hipGetLastError(); *out = (void *)ev; return up_code(e); },
    [](pdbeda_upload::Event ev) { return up_code(hipEventQuery((hipEvent_t)ev)); },
    [](void *dst, const void *src, size_t bytes, pdbeda_upload::Stream s) { return up_code(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)s)); },
    [](pdbeda_upload::Event ev, pdbeda_upload::Stream s) { return up_code(hipEventRecord((hipEvent_t)ev, (hipStream_t)s)); },
};

static std::mutex g_engine_mu;
static std::map<int, UploadEngine *> g_engines;   // (never destroyed: the readers are parked on the queue when the process ends)

static UploadEngine *upload_engine(int device) {
    std::lock_guard<std::mutex> g(g_engine_mu);
    auto it = g_engines.find(device);
    if (it != g_engines.end()) return it->second;
    UploadEngine *en = UploadEngine::create(&g_hip_backend, device);
    g_engines[device] = en;
    return en;
}

static bool ensure_reader_events(pdbeda_ctx *ctx, UploadEngine *engine) {
    for (int r = 0; r < engine->n_readers; ++r)
        if (!ctx->reader_ev[r] && hipEventCreateWithFlags(&ctx->reader_ev[r], hipEventDisableTiming) != hipSuccess) {
            ctx->reader_ev[r] = nullptr;
            (void)hipGetLastError();
            return false;
        }
    return true;
}

// One map's bytes -- from a file (fd >= 0: pread at offset + position) or from the caller's memory (src) -- into HBM at dst through the process's
// upload engine; on return every chunk is queued on a reader's stream (or given up) and ctx->stream waits for them.  *why: a file-level reason.
static hipError_t engine_copy(pdbeda_ctx *ctx, UploadEngine *engine, int fd, int64_t offset, const char *src, char *dst, size_t need, const char **why) {
    hipError_t e = hipSuccess;
    // The arena may be a recycled one: the pool protects a recycled arena by STREAM ORDER on ctx->stream (maps and lists are
    // freed without a host sync while their kernels are still queued; the debug poison fill above is queued there too).  The
    // readers' copies go through their own streams, which know nothing of that order -- so the first chunk is handed out only
    // when everything queued on ctx->stream up to here has run (normally: nothing is pending, the query says so at once).
    if (e == hipSuccess) {
        hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipErrorNotReady) q = ctx_wait(ctx);     // (timed, under the watchdog)
        if (q != hipSuccess) e = q;
    }
    if (e == hipSuccess && !ctx->timed_out) {
        UploadLoad ld;
        ld.fd = fd; ld.offset = offset; ld.src = src; ld.dst = dst; ld.need = need;
        ld.timeout_s = ctx->timeout_s;
        ld.deadline = ctx->deadline;
        engine->submit(ld);      // (chunked, queued on the readers' streams or given up: pdbeda_upload.h)
        // the context's stream waits for the readers' copies of THIS map: an event behind whatever each reader has queued so far
        // (a little more than needed when it has gone on to another load's chunk -- never less)
        for (int r = 0; r < engine->n_readers; ++r) {
            if (!ld.used[r]) continue;
            hipError_t je = hipEventRecord(ctx->reader_ev[r], (hipStream_t)ld.stream_used[r]);      // (the stream this load's chunks went to: the reader may have taken a new one since)
            if (je == hipSuccess) je = hipStreamWaitEvent(ctx->stream, ctx->reader_ev[r], 0);
            if (je != hipSuccess && e == hipSuccess) e = je;
        }
        if (ld.e != pdbeda_upload::UP_OK && e == hipSuccess) e = up_error(ld.e);
        if (ld.stalled && e == hipSuccess) { e = hipErrorNotReady; if (!ld.why) ld.why = "a copy stream of the upload engine stalled behind another copy and was given up; the map is incomplete"; }
        *why = ld.why;
        if (ld.timed_out) {
            ctx->timed_out = true;
            ctx->err = "watchdog: the stream did not drain within the per-entry time-out; context abandoned";
            if (e == hipSuccess) e = hipErrorNotReady;
        }
    }
    return e;
}

static int upload_file_impl(pdbeda_ctx *ctx, const char *path, int64_t offset, int byteswap, const pdbeda_geometry *geom, pdbeda_map **out, double *mean, double *std) {
    if (!ctx || !path || !geom || !out || offset < 0) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n_vox = (int64_t)geom->ncrs[0] * geom->ncrs[1] * geom->ncrs[2];
    if (n_vox <= 0 || n_vox >= (1ll << 32)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "grid size out of range");
    const size_t need = sizeof(float) * (size_t)n_vox;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "cannot open %s: %s", path, strerror(errno));
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (int64_t)sb.st_size < offset + (int64_t)need) {
        close(fd);
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s holds fewer than %lld grid bytes after offset %lld", path, (long long)need, (long long)offset);
    }
    UploadEngine *engine = upload_engine(ctx->device);
    if (engine->n_readers < 1) { close(fd); return fail(ctx, PDBEDA_ERR_MEMORY, "no reader (pinned chunks, copy stream, thread) for the file upload"); }
    if (!ensure_reader_events(ctx, engine)) { close(fd); return fail(ctx, PDBEDA_ERR_MEMORY, "no event for the file upload"); }
    Geom g;
    MadeMap made;
    int rc = fill_geom(ctx, geom, &g);
    if (rc == 0) rc = made.make(ctx, "map upload from file", g, n_vox);
    if (rc) { close(fd); return rc; }
    pdbeda_map *m = made.m.get();
    float *d = made.dens;
    const char *why = nullptr;
    hipError_t e = engine_copy(ctx, engine, fd, offset, nullptr, (char *)d, need, &why);   // (first: the stream is idle, its query says so at once)
    const bool geom_in_stats = (mean || std) && stats_carries_geom(m);      // (the statistics' first launch brings the geometry along: a copy launch less)
    if (e == hipSuccess && !geom_in_stats) e = made.geometry_up();
    close(fd);
    if (e == hipSuccess && !why && byteswap) {
        PROF(ctx, "k_byteswap32");
        hipLaunchKernelGGL(k_byteswap32, dim3(grid_for(n_vox, 256, 8192)), dim3(256), 0, ctx->stream, (uint32_t *)d, n_vox);
        e = hipGetLastError();
    }
    // mean / std (and the range of the blob sums' quantum) queued behind the copies: ONE wait for the map and its statistics -- every
    // caller asks for them next (cutoffs are mean + k std), and a wait of their own was one of a pool entry's host round trips
    const bool with_stats = (mean || std) && e == hipSuccess && !why;
    if (with_stats) e = made.stats_up(geom_in_stats);
    const double t_s0 = now_s();
    const hipError_t e2 = ctx_sync(ctx);      // (&m->geom is free again)
    if (upload_trace()) fprintf(stderr, "upload: final wait %.3f ms\n", 1e3 * (now_s() - t_s0));
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess || why) return why ? fail(ctx, PDBEDA_ERR_ARGUMENT, "reading %s: %s", path, why) : fail(ctx, PDBEDA_ERR_DEVICE, "map upload from file: %s", hipGetErrorString(e));
    if (with_stats) made.stats_out(mean, std);
    made.publish(out);
    return PDBEDA_OK;
}

extern "C" int pdbeda_map_upload_file(pdbeda_ctx *ctx, const char *path, int64_t offset, int byteswap, const pdbeda_geometry *geom, pdbeda_map **out) {
    return upload_file_impl(ctx, path, offset, byteswap, geom, out, nullptr, nullptr);
}
extern "C" int pdbeda_map_upload_file_stats(pdbeda_ctx *ctx, const char *path, int64_t offset, int byteswap, const pdbeda_geometry *geom, pdbeda_map **out,
                                            double *mean, double *std) {
    return upload_file_impl(ctx, path, offset, byteswap, geom, out, mean, std);
}

extern "C" int pdbeda_map_combine(pdbeda_map *a, pdbeda_map *b, double alpha, pdbeda_map **out) {
    if (!a || !b || !out) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    pdbeda_ctx *ctx = a->ctx;
    if (int rc = same_grid(ctx, a->geom, a->n_vox, b)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MadeMap made;
    if (int rc = made.make_like("map combine", a)) return rc;
    hipError_t e = made.geometry_up();
    if (e == hipSuccess) {
        PROF(ctx, "k_map_combine");
        hipLaunchKernelGGL(k_map_combine, dim3(grid_for(a->n_vox / 4 + 1, 256, 4096)), dim3(256), 0, ctx->stream, a->dens, b->dens, alpha, a->n_vox, made.dens);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = ctx_sync(ctx);   // (the new map's geometry record is read by the copy above)
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "map combine: %s", hipGetErrorString(e));
    made.publish(out);
    return PDBEDA_OK;
}

extern "C" int pdbeda_map_download(pdbeda_map *m, float *density_out) {
    if (!m || !density_out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, d2h(ctx, density_out, m->dens, sizeof(float) * (size_t)m->n_vox));
    HIP_TRY(ctx, ctx_sync(ctx));
    return PDBEDA_OK;
}

extern "C" int pdbeda_map_free(pdbeda_map *m) {
    if (!m) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    // the arena goes back to the context's pool: whoever gets it next is enqueued on this stream behind the last kernel that
    // reads the map -- no wait, no hipFree (which would synchronise the whole device under the other streams of a pool)
    ctx->live_handles--;
    delete m;
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Whole-map reductions
// ------------------------------------------------------------------------------------
static int reduce_launch(pdbeda_map *m, int mode, const double *mean_dev, double cutoff, double scale, int take_sqrt, double *out_dev) {
    pdbeda_ctx *ctx = m->ctx;
    { PROF(ctx, "k_reduce_partials"); hipLaunchKernelGGL(k_reduce_partials, dim3(N_PARTIAL), dim3(256), 0, ctx->stream, m->dens, m->n_vox, mode, mean_dev, cutoff, ctx->partials); }
    hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(256), 0, ctx->stream, ctx->partials, N_PARTIAL, scale, take_sqrt, out_dev);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// The quantum of the order-independent blob sums of this map (see FixSums in pdbeda_kernels.h; the rule and the bounds it guarantees:
// map_quantum in pdbeda_jobplan.h).  Two deterministic reductions over the map, once per map (the result is cached; a borrowed device
// pointer is taken to hold the same grid for the life of the map).
// The quantum of a map's integer blob sums from its range (sum |x|, max |x|: fixed reduction order, so the quantum is the same in
// every run).  range_enqueue + range_apply: the pass rides in the same wait as the map's mean / std when those are asked for
// first (pdbeda_map_stats: every DensityMatrix asks at once) -- a wait of its own in front of the map's first labelling job was
// one of an entry's ~17 host round trips (round 4).
static int range_enqueue(pdbeda_map *m, double *range_host /* [2], filled at the next ctx_sync; nullptr: the caller copies the result slots itself */) {
    pdbeda_ctx *ctx = m->ctx;
    double *res = ctx->partials + 2 * N_PARTIAL + 4;
    { PROF(ctx, "k_range_partials"); hipLaunchKernelGGL(k_range_partials, dim3(N_PARTIAL), dim3(256), 0, ctx->stream, m->dens, m->n_vox, ctx->partials, ctx->partials + N_PARTIAL); }
    hipLaunchKernelGGL(k_range_final, dim3(1), dim3(256), 0, ctx->stream, ctx->partials, ctx->partials + N_PARTIAL, N_PARTIAL, res);
    HIP_TRY(ctx, hipGetLastError());
    if (range_host) HIP_TRY(ctx, d2h(ctx, range_host, res, 2 * sizeof(double)));
    return 0;
}
static void range_apply(pdbeda_map *m, const double range[2]) {
    bool refused = false;
    const double mul = map_quantum(range[0], range[1], &refused);
    if (refused) m->fix_refused = true;      // (NaN / infinite voxels: the labelling calls refuse the map)
    else { m->fix_mul = mul; m->max_abs = range[1]; }
}
static int map_fix_mul(pdbeda_map *m) {
    pdbeda_ctx *ctx = m->ctx;
    if (m->fix_mul == 0.0 && !m->fix_refused) {
        double range[2] = {0.0, 0.0};
        const int rc = range_enqueue(m, range);
        if (rc) return rc;
        HIP_TRY(ctx, ctx_sync(ctx));
        range_apply(m, range);
    }
    if (m->fix_refused) return fail(ctx, PDBEDA_ERR_ARGUMENT, "the map holds non-finite density values: blob sums are undefined");
    return 0;
}
// The quantum of sums over the unique box for a caller that leaves NaN / infinite voxels out of its sums (the partition, the basins): the map's
// own, or -- the map's was refused -- one from the largest finite |rho| of the box (box_quantum; k_partition_range and a wait).  d_range: a
// zeroed device word of the caller's.
static int box_fix_mul(pdbeda_map *m, int nc, int nr, int uc, int ur, int us, unsigned long long *d_range, double *fix_mul) {
    pdbeda_ctx *ctx = m->ctx;
    *fix_mul = m->fix_mul;
    if (!m->fix_refused) return 0;
    const int64_t nbox = (int64_t)uc * ur * us;
    unsigned long long bits = 0;
    { PROF(ctx, "k_partition_range"); hipLaunchKernelGGL(k_partition_range, dim3(grid_for(nbox, 256, 4096)), dim3(256), 0, ctx->stream, m->dens, nc, nr, uc, ur, us, d_range); }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, d2h(ctx, &bits, d_range, 8));
    HIP_TRY(ctx, ctx_sync(ctx));
    double top;
    memcpy(&top, &bits, 8);
    *fix_mul = box_quantum(top, nbox);
    return 0;
}

// A map made by pdbeda_map_from_device borrows the caller's buffer; what the library caches about its CONTENTS -- the quantum of
// the order-independent blob sums, derived from sum |rho| and max |rho| -- must be dropped when the caller rewrites the buffer
// in place (larger values would overflow the 62-bit sums silently).
extern "C" int pdbeda_map_invalidate(pdbeda_map *m) {
    if (!m) return PDBEDA_ERR_ARGUMENT;
    m->fix_mul = 0.0;
    m->max_abs = 0.0;
    m->fix_refused = false;
    return PDBEDA_OK;
}

// mean and std in numpy's own summation tree (k_np_chunk_sums / k_np_final): == np.mean / np.std, not merely close -- and, while
// the map's range is not known yet, the range pass behind them (range_enqueue): everything queued, nothing waited for.
// chunk_sums: 8 * max(n_vox / NP_CHUNK, 1) bytes of device scratch; host[2] / range[2] are filled at the next ctx_sync.
// chunk_sums: scratch of 3 x max(n_vox / NP_CHUNK, 1) doubles (the chunks' numpy sums; with want_range their range partials behind them).
// Round 6: with want_range the range rides in the mean's pass (k_np_chunk_sums / k_np_final, mode 0) and the LAST launch of the chain writes mean,
// std and range straight into the pinned block: four launches where there were seven (two range kernels and a copy), and one pass over the map less.
// with_geom: the first launch of the chain also writes the map's geometry struct to the device (a kernel argument by value; callers check stats_carries_geom)
static int stats_enqueue(pdbeda_map *m, double *chunk_sums, double host[2], double range[2], bool want_range, bool with_geom) {
    pdbeda_ctx *ctx = m->ctx;
    // (mean / std in the first two of the eight result slots behind the partial sums, the range in slots 4 / 5)
    double *res = ctx->partials + 2 * N_PARTIAL;
    const int64_t n_full = m->n_vox / NP_CHUNK;
    const int64_t n_chunks = std::max<int64_t>(n_full, 1);
    hipStream_t st = ctx->stream;
    // the results' place in the pinned block (kernels write host memory only with PDBEDA_COPY_KERNELS, the default)
    double *host_out = nullptr;
    if (want_range && copy_kernels()) host_out = reinterpret_cast<double *>(pinned_take(ctx, 6 * sizeof(double)));      // (the six doubles of res: one 64-byte line)
    if (host_out) {
        pinned_deliver(ctx, (char *)host_out, host, 2 * sizeof(double));
        pinned_deliver(ctx, (char *)(host_out + 4), range, 2 * sizeof(double));
    }
    double *r_sum = want_range ? chunk_sums + n_chunks : nullptr, *r_max = want_range ? chunk_sums + 2 * n_chunks : nullptr;
    for (int mode = 0; mode < 2; ++mode) {
        const bool with_range = want_range && mode == 0;
        if (n_full > 0) { PROF(ctx, "k_np_chunk_sums"); hipLaunchKernelGGL(k_np_chunk_sums, dim3((unsigned)std::min<int64_t>(n_full, 1 << 16)), dim3(256), 0, st, m->dens, n_full, mode, res, chunk_sums,
                                                                           with_range ? r_sum : (double *)nullptr, with_range ? r_max : (double *)nullptr,
                                                                           m->geom, with_geom && mode == 0 ? m->geom_dev : (Geom *)nullptr); }
        { PROF(ctx, "k_np_final"); hipLaunchKernelGGL(k_np_final, dim3(1), dim3(256), 0, st, m->dens, m->n_vox, n_full, mode, res, chunk_sums, mode, res + mode,
                                                      with_range && n_full > 0 ? r_sum : (const double *)nullptr, with_range && n_full > 0 ? r_max : (const double *)nullptr,
                                                      with_range ? res + 4 : (double *)nullptr, want_range && mode == 1 ? res + 4 : (const double *)nullptr, mode == 1 ? host_out : (double *)nullptr); }
    }
    HIP_TRY(ctx, hipGetLastError());
    if (host_out) return 0;
    if (!want_range) {
        HIP_TRY(ctx, d2h(ctx, host, res, 2 * sizeof(double)));
        return 0;
    }
    // (no room in the pinned block, or the runtime's copies asked for: one copy of the six doubles, or two)
    if (char *stage = pinned_take(ctx, 6 * sizeof(double))) {
        HIP_TRY(ctx, stage_copy(ctx, stage, res, 6 * sizeof(double), false));
        pinned_deliver(ctx, stage, host, 2 * sizeof(double));
        pinned_deliver(ctx, stage + 4 * sizeof(double), range, 2 * sizeof(double));
        return 0;
    }
    HIP_TRY(ctx, d2h(ctx, host, res, 2 * sizeof(double)));
    HIP_TRY(ctx, d2h(ctx, range, res + 4, 2 * sizeof(double)));
    return 0;
}

extern "C" int pdbeda_map_stats(pdbeda_map *m, double *mean, double *std) {
    if (!m) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n_full = m->n_vox / NP_CHUNK;
    double host[2], range[2] = {0.0, 0.0};
    const bool want_range = m->fix_mul == 0.0 && !m->fix_refused;   // the quantum of the map's blob sums, in the same wait
    int rc = with_scratch(ctx, 24 * (size_t)std::max<int64_t>(n_full, 1), [&](char *base) -> int {
        return stats_enqueue(m, reinterpret_cast<double *>(base), host, range, want_range);
    });
    if (rc) return rc;
    if (want_range) range_apply(m, range);
    if (mean) *mean = host[0];
    if (std) *std = host[1];
    return PDBEDA_OK;
}

extern "C" int pdbeda_sum_of_abs(pdbeda_map *m, float cutoff, double *out) {
    if (!m || !out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *res = ctx->partials + N_PARTIAL + 2;
    int rc = reduce_launch(m, 2, nullptr, (double)cutoff, 1.0, 0, res);
    if (rc) return rc;
    HIP_TRY(ctx, d2h(ctx, out, res, sizeof(double)));
    HIP_TRY(ctx, ctx_sync(ctx));
    return PDBEDA_OK;
}

extern "C" int pdbeda_abs_select_hist(pdbeda_map *a, pdbeda_map *b, double alpha, double cut_a, double cut_b, int which, int shift,
                                      unsigned long long prefix, unsigned long long prefix_mask, uint32_t *hist) {
    if (!a || !hist || shift < 0 || shift > 48 || (which != 0 && which != 1) || (which == 1 && !b)) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = a->ctx;
    if (b)
        if (int rc = same_grid(ctx, a->geom, a->n_vox, b)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n = (int64_t)a->geom.unique_ncrs[0] * a->geom.unique_ncrs[1] * a->geom.unique_ncrs[2];
    return with_scratch(ctx, 65536 * sizeof(uint32_t), [&](char *base) -> int {
        unsigned int *d_hist = reinterpret_cast<unsigned int *>(base);
        HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, 65536 * sizeof(uint32_t), ctx->stream));
        { PROF(ctx, "k_abs_select_hist");
          hipLaunchKernelGGL(k_abs_select_hist, dim3(grid_for(n, 256, 4096)), dim3(256), 0, ctx->stream, a->geom_dev, a->dens, b ? b->dens : nullptr,
                             alpha, cut_a, cut_b, which, shift, prefix, prefix_mask, d_hist); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, d2h(ctx, hist, d_hist, 65536 * sizeof(uint32_t)));
        return 0;
    });
}

// k_point_density writes the one of its two results that is asked for (the other has no array, and an empty piece of scratch).
static int point_lookup(pdbeda_map *m, const char *site, const int32_t *crs, int64_t n, double *out, uint8_t *valid) {
    if (!m || (n > 0 && (!crs || (!out && !valid))) || n < 0) return PDBEDA_ERR_ARGUMENT;
    if (n == 0) return PDBEDA_OK;
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Input<int32_t> in{crs, (size_t)(3 * n)};
    Result<double> r_out{out, out ? (size_t)n : 0};
    Result<uint8_t> r_valid{valid, valid ? (size_t)n : 0};
    return with_scratch(ctx, site, [&](Carver &cv) { in.carve(cv); r_out.carve(cv); r_valid.carve(cv); }, [&]() -> int {
        HIP_TRY(ctx, in.send(ctx));
        hipLaunchKernelGGL(k_point_density, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, m->geom_dev, m->dens, in.at, n, r_out.at(ctx), r_valid.at(ctx));      // (one of the two takes)
        HIP_TRY(ctx, r_out.finish(ctx));
        HIP_TRY(ctx, r_valid.finish(ctx));
        return 0;
    });
}
extern "C" int pdbeda_point_density(pdbeda_map *m, const int32_t *crs, int64_t n, double *out) { return point_lookup(m, "point density", crs, n, out, nullptr); }
extern "C" int pdbeda_valid_crs(pdbeda_map *m, const int32_t *crs, int64_t n, uint8_t *out) { return point_lookup(m, "valid crs", crs, n, nullptr, out); }

extern "C" int pdbeda_crs2xyz(pdbeda_map *m, const int32_t *crs, int64_t n, double *xyz) {
    if (!m || (n > 0 && (!crs || !xyz)) || n < 0) return PDBEDA_ERR_ARGUMENT;
    if (n == 0) return PDBEDA_OK;
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Input<int32_t> in{crs, (size_t)(3 * n)};
    Result<double> res{xyz, (size_t)(3 * n)};
    return with_scratch(ctx, "crs2xyz", [&](Carver &cv) { in.carve(cv); res.carve(cv); }, [&]() -> int {
        HIP_TRY(ctx, in.send(ctx));
        hipLaunchKernelGGL(k_crs2xyz, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, m->geom_dev, in.at, n, res.at(ctx));
        HIP_TRY(ctx, res.finish(ctx));
        return 0;
    });
}

extern "C" int pdbeda_xyz2crs(pdbeda_map *m, const double *xyz, int64_t n, int32_t *crs) {
    if (!m || (n > 0 && (!crs || !xyz)) || n < 0) return PDBEDA_ERR_ARGUMENT;
    if (n == 0) return PDBEDA_OK;
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Input<double> in{xyz, (size_t)(3 * n)};
    Result<int32_t> res{crs, (size_t)(3 * n)};
    return with_scratch(ctx, "xyz2crs", [&](Carver &cv) { in.carve(cv); res.carve(cv); }, [&]() -> int {
        HIP_TRY(ctx, in.send(ctx));
        hipLaunchKernelGGL(k_xyz2crs, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, m->geom_dev, in.at, n, res.at(ctx));
        HIP_TRY(ctx, res.finish(ctx));
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// Labelling jobs
// ------------------------------------------------------------------------------------
// Carve a job out of an arena.  max_runs / max_blobs are worst-case bounds (a run needs a
// gap: <= bits/2 + 1 per word; a blob owns >= one 2x2x2 cell... we simply bound blobs by runs).
// max_runs: run ids (comp_of_run); max_comps: component ids (every per-component array; generic jobs: == max_runs, a run is a component)
// The rank / key table's arithmetic is plan_key_table's (pdbeda_jobplan.h); the table is returned for the callers that size a clear by it.
static KeyTable job_carve(Job &job, Carver &cv, int n_vols, int64_t total_words, int64_t total_keys, int64_t max_runs,
                          int64_t max_blobs, size_t extra_labels, int32_t **labels_out, int64_t n_tiles = 0, int64_t max_comps = -1) {
    if (max_comps < 0) max_comps = max_runs;
    job.run_cap = (uint32_t)max_runs; job.comp_cap = (uint32_t)max_comps; job.blob_cap = (uint32_t)std::min<int64_t>(max_blobs, 0xffffffffll);
    job.n_vols = n_vols;
    job.total_words = total_words;
    const KeyTable kt = plan_key_table(total_keys, n_tiles);
    job.key_words = kt.key_words;
    job.n_fine = kt.n_fine; job.fine_shift = kt.fine_shift; job.fine_per_group = kt.fine_per_group; job.n_groups = kt.n_groups; job.n_fine_alloc = kt.n_fine_alloc;
    job.clear_bits = kt.clear_bits; job.clear_fine = kt.clear_fine; job.clear_mid = kt.clear_mid;   // (what a tile's k_face_merge workgroup clears)
    job.vols = cv.take<VolDesc>(std::max(n_vols, 1));
    // counters, masks, first-key bitmap and rank counters in a row: a sphere / list job clears them with ONE fill (grouped_job;
    // whole-map jobs clear theirs in kernels)
    job.ctr = cv.take<Counters>(1);
    job.mask = cv.take<uint64_t>(total_words);
    job.key_bits = cv.take<uint64_t>(kt.key_bits_elems);
    // the rank counters sit right behind the bitmap (ONE clear covers both)
    job.fine_count = cv.take<uint32_t>(kt.fine_count_elems);
    job.mid_count = cv.take<uint32_t>(kt.mid_count_elems);
    job.group_count = kt.has_group_count ? cv.take<uint32_t>(KEY_GROUPS) : nullptr;
    job.run_base = cv.take<uint32_t>(total_words);
    job.comps_are_runs = n_tiles ? 0 : 1;
    job.comp_of_run = n_tiles ? cv.take<uint32_t>(max_runs) : nullptr;
    job.label_of_comp = n_tiles ? cv.take<int32_t>(max_comps) : nullptr;
    job.word_comps = n_tiles ? cv.take<uint8_t>((size_t)n_tiles * 2 * 256 * 8) : nullptr;
    job.unit_done = n_tiles ? cv.take<uint32_t>((size_t)n_tiles) : nullptr;
    job.unit_flag = n_tiles ? cv.take<uint32_t>(4) : nullptr;
    job.tile_mode = n_tiles ? cv.take<uint8_t>(n_tiles) : nullptr;
    job.tile_runs = n_tiles ? cv.take<uint32_t>(n_tiles) : nullptr;
    job.root_mask = n_tiles ? cv.take<uint64_t>((size_t)n_tiles * 4) : nullptr;
    job.n_tiles = (int32_t)n_tiles;
    job.inbox = n_tiles ? cv.take<InboxEntry>((size_t)n_tiles * INBOX_CAP) : nullptr;
    job.inbox_count = n_tiles ? cv.take<uint32_t>((size_t)n_tiles * INBOX_STRIDE) : nullptr;
    job.vol_sign[0] = job.vol_sign[1] = 1;
    job.parent = cv.take<int32_t>(max_comps);
    job.kpar = n_tiles ? cv.take<unsigned long long>(max_comps) : nullptr;
    job.r_n = cv.take<uint32_t>(max_comps);
    job.r_sum = cv.take<long long>((size_t)7 * max_comps);
    job.r_sum_stride = max_comps;
    job.r_c = cv.take<long long>(max_comps);
    job.r_r = cv.take<long long>(max_comps);
    job.r_s = cv.take<long long>(max_comps);
    job.r_key = cv.take<unsigned long long>(max_comps);
    job.r_rank = cv.take<uint32_t>(max_comps);
    job.b_n = cv.take<int64_t>(max_blobs);
    job.b_key = cv.take<int64_t>(max_blobs);
    job.b_total = cv.take<double>(max_blobs);
    job.b_centroid = cv.take<double>(3 * max_blobs);
    job.b_center = cv.take<double>(3 * max_blobs);
    job.b_volume = cv.take<double>(max_blobs);
    job.b_group = cv.take<int32_t>(max_blobs);
    int32_t *lab = extra_labels ? cv.take<int32_t>(extra_labels) : nullptr;
    if (labels_out) *labels_out = lab;
    return kt;
}

// Enqueue the labelling engine on a job whose masks are already painted.
// labelled: k_atom_engine has done everything up to the painted keys.  unordered: the caller takes the roots' rows as they come (k_resolve hands them
// out) and writes its results itself (pdbeda_aggregate_cloud's union job: k_union_finish) -- no keys painted, no ranks, no blob table
static int engine_enqueue(pdbeda_ctx *ctx, pdbeda_map *m, Job &job, int64_t max_runs, bool labelled = false, bool unordered = false) {
    hipStream_t st = ctx->stream;
    // per-run kernels are grid-stride over the ACTUAL run count (read on the device)
    const unsigned run_grid = grid_for(max_runs, 256, 2048);
    if (job.total_words > 0 && !labelled) {
        {   // few words in large volumes: a quarter of the words a block, four times the blocks (the loop over a wave's words is
            // serial; the rows of many small volumes -- atom spheres -- are mostly narrow: a thread each, 256 to the block)
            PROF(ctx, "k_run_index");
            static const int force_wpb = [] { const char *e = getenv("PDBEDA_RUNINDEX_WPB"); return e ? atoi(e) : 0; }();   // (experiments: 64 / 256)
            if (force_wpb != 256 && (force_wpb == 64 || (job.total_words < 256ll * 2048 && job.total_words > 64ll * job.n_vols))) hipLaunchKernelGGL(k_run_index<64>, dim3(grid_for(job.total_words, 64, 1ll << 30)), dim3(256), 0, st, job, m->dens, m->geom_dev);
            else hipLaunchKernelGGL(k_run_index<256>, dim3(grid_for(job.total_words, 256, 1ll << 30)), dim3(256), 0, st, job, m->dens, m->geom_dev);
        }
        { PROF(ctx, "k_union"); hipLaunchKernelGGL(k_union, dim3(grid_for(job.total_words * 4, 256, 1ll << 30)), dim3(256), 0, st, job); }
        { PROF(ctx, "k_resolve"); hipLaunchKernelGGL(k_resolve, dim3(run_grid), dim3(256), 0, st, job, unordered ? 1 : 0); }
        if (!unordered) { PROF(ctx, "k_paint_keys"); hipLaunchKernelGGL(k_paint_keys, dim3(run_grid), dim3(256), 0, st, job); }
    }
    // (k_emit also runs for an empty job: its first block publishes the blob count)
    if (!unordered) { PROF(ctx, "k_emit"); hipLaunchKernelGGL(k_emit, dim3(job.total_words > 0 ? std::min(run_grid, 512u) : 1u), dim3(256), 0, st, job, m->geom_dev); }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

static LabelJob *new_label_job(pdbeda_ctx *ctx, pdbeda_map *m) {
    LabelJob *lj = new LabelJob();
    lj->ctx = ctx;
    lj->map = m;
    return lj;
}

// Hand out view p of an enqueued job: the volumes [vol_lo, vol_hi)
static pdbeda_bloblist *job_view(LabelJob *lj, int p, int vol_lo, int vol_hi, int sign) {
    pdbeda_bloblist *bl = &lj->view[p];
    bl->job = lj;
    bl->vol_lo = vol_lo;
    bl->vol_hi = vol_hi;
    bl->sign = sign;
    lj->live++;
    lj->ctx->live_handles++;
    return bl;
}

template <int CW>
static void launch_tile_label(pdbeda_ctx *ctx, unsigned n_tiles, const Job &job, const float *dens, const Geom *geom_dev, const TileDims &td,
                              const JobInit &init, int pair_slots) {
    { PROF(ctx, "k_tile_label"); hipLaunchKernelGGL((k_tile_label<CW>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(512), 0, ctx->stream, job, dens, geom_dev, td, init); }
    // cross-tile unions (and, when a tile overflowed LDS, every pair that has such a tile on either side)
    {   // (grids of one tile column have no c faces: two waves fewer per workgroup to dispatch)
        PROF(ctx, "k_face_merge");
        if (td.ctiles > 1) hipLaunchKernelGGL((k_face_merge<CW, FM_THREADS_WIDE>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(FM_THREADS_WIDE), 0, ctx->stream, job, dens, geom_dev, td, pair_slots);
        else hipLaunchKernelGGL((k_face_merge<CW, FM_THREADS>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(FM_THREADS), 0, ctx->stream, job, dens, geom_dev, td, pair_slots);
    }
    if (job.unit_form) {   // the job is known to have unit tiles (its first run said so): their labelling, then their pairs
        { PROF(ctx, "k_unit_label"); hipLaunchKernelGGL((k_unit_label<CW>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(512), 0, ctx->stream, job, dens, geom_dev, td); }
        { PROF(ctx, "k_unit_pairs"); hipLaunchKernelGGL((k_unit_pairs<CW>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(512), 0, ctx->stream, job, td); }
    }
}

// fused: the launch also ranks the roots and writes the blob table (k_emit_tiles is then not launched) -- see k_labels_tiles
// (a fused launch of a job whose rank counters come in groups of 16 -- maps up to 2^25 keys -- takes the instantiation that
//  builds the rank table under its second trip: UNDER in k_labels_tiles; every other launch is the kernel as it was)
template <bool FUSED, bool UNDER>
static void launch_labels_cw(pdbeda_ctx *ctx, const Job &job, const TileDims &td, int32_t *labels_dev, const Geom *geom_dev) {
    switch (td.cw) {
        case 1: hipLaunchKernelGGL((k_labels_tiles<1, FUSED, UNDER>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(PDBEDA_LABELS_NT_THREADS), 0, ctx->stream, job, td, labels_dev, geom_dev); break;
        case 2: hipLaunchKernelGGL((k_labels_tiles<2, FUSED, UNDER>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(PDBEDA_LABELS_NT_THREADS), 0, ctx->stream, job, td, labels_dev, geom_dev); break;
        case 3: hipLaunchKernelGGL((k_labels_tiles<3, FUSED, UNDER>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(PDBEDA_LABELS_NT_THREADS), 0, ctx->stream, job, td, labels_dev, geom_dev); break;
        default: hipLaunchKernelGGL((k_labels_tiles<4, FUSED, UNDER>), dim3(td.ctiles, td.rtiles, td.stiles), dim3(PDBEDA_LABELS_NT_THREADS), 0, ctx->stream, job, td, labels_dev, geom_dev); break;
    }
}
template <bool FUSED>
static void launch_labels(pdbeda_ctx *ctx, const Job &job, const TileDims &td, int32_t *labels_dev, const Geom *geom_dev) {
    if (FUSED && job.fine_shift == 4) launch_labels_cw<FUSED, FUSED>(ctx, job, td, labels_dev, geom_dev);
    else launch_labels_cw<FUSED, false>(ctx, job, td, labels_dev, geom_dev);
}
// A whole-map job's signed label volume: its own if it kept one (PDBEDA_FLAG_LABELS), else written into `scratch` now (a caller carves the scratch only
// when !job_keeps_labels).
static bool job_keeps_labels(const LabelJob *lj) { return lj->labels_dev && lj->labels_done; }
static const int32_t *job_signed_labels(const LabelJob *lj, int32_t *scratch) {
    if (job_keeps_labels(lj)) return lj->labels_dev;
    launch_labels<false>(lj->ctx, lj->job, lj->td, scratch, lj->map->geom_dev);
    return scratch;
}

// Enqueue a whole-map job.  The first run carves the arena for what maps need in practice instead of the worst case (2.9 GB at 256^3, of
// which a job touches a few hundred MB), and leaves out the unit tiles' two launches: the sizes are plan_whole_map's (pdbeda_jobplan.h).  A map
// that needs more raises Counters::overflow on the device, stays inside its arena, and is run again with worst_case set
// by the first accessor that reads the counters (list_resolve_counts): correct always, slower only where it was slow already.
// On success the job, its arena and the recipe of this run are written into *out (the record of a job's first run, or of the run it replaces).
static int whole_map_enqueue(pdbeda_map *m, float cut_pos, float cut_neg, bool want_pos, bool want_neg, uint32_t flags, bool worst_case, LabelJob *out) {
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Geom &g = m->geom;
    const int n_planes = (want_pos ? 1 : 0) + (want_neg ? 1 : 0);
    const int uc = g.unique_ncrs[0], ur = g.unique_ncrs[1], us = g.unique_ncrs[2];
    const bool labels = (flags & PDBEDA_FLAG_LABELS) != 0;
    const WholeMapPlan wp = plan_whole_map(uc, ur, us, n_planes, worst_case, labels);
    if (wp.refusal == PLAN_KEYS || wp.refusal == PLAN_AXIS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "grid too large");
    if (wp.refusal == PLAN_RUN_IDS)
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "grid too large for whole-map labelling: %d x %d x %d voxels need %lld run ids (limit 2^31: about 1100^3 for a fused job)",
                    uc, ur, us, (long long)wp.run_ids_needed);
    const int64_t tiles_pp = wp.tiles_pp;

    TileDims td;
    td.ctiles = wp.ctiles; td.cw = wp.cw; td.rtiles = wp.rtiles; td.stiles = wp.stiles;
    td.n_planes = n_planes;
    td.uc = uc; td.ur = ur; td.us = us; td.row_words = wp.row_words;
    td.nc = g.ncrs[0]; td.nr = g.ncrs[1];
    td.cut[0] = want_pos ? cut_pos : cut_neg;
    td.sign[0] = want_pos ? 1 : -1;
    td.cut[1] = cut_neg;
    td.sign[1] = -1;

    int rc_fix = map_fix_mul(m);
    if (rc_fix) return rc_fix;
    Job job;
    memset(&job, 0, sizeof job);
    job.fix_mul = m->fix_mul;
    size_t need = 0;
    Arena arena;
    int32_t *labels_dev = nullptr;
    int rc = arena_carve(ctx, "whole-map labelling", &arena, [&](Carver &cv) {
        job_carve(job, cv, n_planes, wp.total_words, wp.total_keys, wp.max_runs, wp.max_blobs, wp.lab_elems, &labels_dev, tiles_pp, wp.max_comps);
        need = cv.off;
    });
    if (rc) return rc;
    job.vol_sign[0] = td.sign[0];
    job.vol_sign[1] = td.sign[1];
    job.unit_form = worst_case ? 1 : 0;      // (the second run has both: the worst-case arena and the unit tiles' launches)
    // the job's number: unique in the process (contexts recycle each other's memory through the driver), started at a random value
    // (so is another process's); stale flags of an earlier job in recycled memory never match it.  Never 0 / the poison pattern.
    static std::atomic<uint32_t> g_epoch{[] {
        uint32_t seed;
        try { seed = (uint32_t)std::random_device{}(); }
        catch (...) { seed = (uint32_t)std::chrono::steady_clock::now().time_since_epoch().count() ^ ((uint32_t)getpid() * 2654435761u); }
        return seed | 1u;
    }()};
    do { job.epoch = g_epoch.fetch_add(1u); } while (job.epoch == 0u || job.epoch == 0xffffffffu);

    JobInit init;
    memset(&init, 0, sizeof init);
    for (int p = 0; p < n_planes; ++p) {
        VolDesc &v = init.v[p];
        v.dim[0] = uc; v.dim[1] = ur; v.dim[2] = us;
        v.org[0] = v.org[1] = v.org[2] = 0;
        v.row_words = wp.row_words;
        v.group = p;
        v.word_base = wp.words_pp * p;
        v.key_base = wp.keys_pp * p;
    }
    init.runs0 = (unsigned)wp.tile_runs;
    init.comps0 = (unsigned)wp.tile_comps;
    hipStream_t st = ctx->stream;
    int pair_slots = PAIR_SLOTS;   // test hook: a tiny LDS pair set overflows on small inputs (PDBEDA_DEBUG_EDGE_CAP = slots, a power of two)
    if (ctx->debug_edge_cap > 0) { pair_slots = 1; while (pair_slots * 2 <= std::min<int64_t>(ctx->debug_edge_cap, PAIR_SLOTS)) pair_slots *= 2; }
    switch (td.cw) {
        case 1: launch_tile_label<1>(ctx, (unsigned)tiles_pp, job, m->dens, m->geom_dev, td, init, pair_slots); break;
        case 2: launch_tile_label<2>(ctx, (unsigned)tiles_pp, job, m->dens, m->geom_dev, td, init, pair_slots); break;
        case 3: launch_tile_label<3>(ctx, (unsigned)tiles_pp, job, m->dens, m->geom_dev, td, init, pair_slots); break;
        default: launch_tile_label<4>(ctx, (unsigned)tiles_pp, job, m->dens, m->geom_dev, td, init, pair_slots); break;
    }
    { PROF(ctx, "k_resolve_tiles"); hipLaunchKernelGGL(k_resolve_tiles, dim3((unsigned)tiles_pp + 64u), dim3(256), 0, st, job, (int)tiles_pp); }
    if (job.group_count) { PROF(ctx, "k_group_counts"); hipLaunchKernelGGL(k_group_counts, dim3((unsigned)(job.n_groups + 255) / 256u), dim3(256), 0, st, job); }
    if (labels) {   // the label writer ranks the roots and writes the blob table itself: one launch
        PROF(ctx, "k_labels_tiles");
        launch_labels<true>(ctx, job, td, labels_dev, m->geom_dev);
    } else {
        PROF(ctx, "k_emit_tiles");
        hipLaunchKernelGGL(k_emit_tiles, dim3(std::min<unsigned>(512u, ((unsigned)tiles_pp + 1u) / 2u)), dim3(256), 0, st, job, m->geom_dev);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "whole-map labelling launch: %s", hipGetErrorString(e));
    out->job = job; out->arena = std::move(arena); out->td = td; out->labels_dev = labels_dev; out->labels_done = labels; out->bytes = need;
    out->cut_pos = cut_pos; out->cut_neg = cut_neg; out->want_pos = want_pos; out->want_neg = want_neg; out->flags = flags; out->worst_case = worst_case;
    return PDBEDA_OK;
}

static int full_blobs_impl(pdbeda_map *m, float cut_pos, float cut_neg, bool want_pos, bool want_neg, uint32_t flags,
                           pdbeda_bloblist **out_pos, pdbeda_bloblist **out_neg) {
    pdbeda_ctx *ctx = m->ctx;
    std::unique_ptr<LabelJob> lj(new_label_job(ctx, m));
    lj->whole_map = true;
    const bool worst_case = ctx->debug_worst_case_arena;   // (the debug hook: the second run's shape at once)
    int rc = whole_map_enqueue(m, cut_pos, cut_neg, want_pos, want_neg, flags, worst_case, lj.get());
    if (rc) return rc;
    for (int p = 0; p < lj->td.n_planes; ++p) {
        pdbeda_bloblist *bl = job_view(lj.get(), p, p, p + 1, lj->td.sign[p]);
        if (bl->sign > 0) *out_pos = bl; else *out_neg = bl;
    }
    lj.release();      // (the views own the job now: pdbeda_bloblist_free)
    return PDBEDA_OK;
}

extern "C" int pdbeda_full_blobs(pdbeda_map *m, float cutoff, uint32_t flags, pdbeda_bloblist **out) {
    if (!m || !out) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    if (cutoff == 0.0f || cutoff != cutoff) return fail(m->ctx, PDBEDA_ERR_ARGUMENT, "cutoff must be non-zero (the reference returns None)");
    pdbeda_bloblist *dummy = nullptr;
    if (cutoff > 0) return full_blobs_impl(m, cutoff, 0.0f, true, false, flags, out, &dummy);
    return full_blobs_impl(m, 0.0f, cutoff, false, true, flags, &dummy, out);
}

extern "C" int pdbeda_full_blobs_pm(pdbeda_map *m, float cutoff_pos, float cutoff_neg, uint32_t flags, pdbeda_bloblist **green,
                                    pdbeda_bloblist **red) {
    if (!m || !green || !red) return PDBEDA_ERR_ARGUMENT;
    *green = *red = nullptr;
    if (!(cutoff_pos > 0.0f) || !(cutoff_neg < 0.0f)) return fail(m->ctx, PDBEDA_ERR_ARGUMENT, "need cutoff_pos > 0 > cutoff_neg");
    return full_blobs_impl(m, cutoff_pos, cutoff_neg, true, true, flags, green, red);
}

// ---- accessors ------------------------------------------------------------------------
static const int64_t SPEC_ROWS = 2048;      // rows of a whole-map job's blob table fetched with its counters (84 B each: 172 KB; the analysis entry's 128^3 map has ~1 400 blobs)

// What the counters of a job said: recorded once, for every view of the job
static void job_record_counts(LabelJob *lj, const Counters &ctr) {
    lj->n_blobs = ctr.n_blobs;
    lj->n_blobs_vol0 = ctr.n_blobs_vol0;
    lj->have_counts = true;
}

// Rank range of a list inside its job's blob table (the counters have been read): a list is the whole job, or one plane of a
// fused whole-map job (k_emit published the split)
struct RankRange { int64_t lo, hi; };
static RankRange list_ranks(const pdbeda_bloblist *bl) {
    const LabelJob *lj = bl->job;
    if (bl->vol_lo == 0 && bl->vol_hi == lj->job.n_vols) return {0, lj->n_blobs};
    return bl->vol_lo == 0 ? RankRange{0, lj->n_blobs_vol0} : RankRange{lj->n_blobs_vol0, lj->n_blobs};
}

static int list_resolve_counts(pdbeda_bloblist *bl) {
    LabelJob *lj = bl->job;
    if (lj->have_counts) return 0;
    pdbeda_ctx *ctx = lj->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Counters ctr;
    // a whole-map job: the first rows of its blob table ride along with the counters (rows beyond the blob count are stale bytes: never served)
    auto fetch = [&]() -> int {
        const Job &job = lj->job;
        const int64_t g = lj->whole_map ? std::min<int64_t>((int64_t)job.blob_cap, SPEC_ROWS) : 0;
        if (g > 0) {
            lj->spec_rows = 0;
            lj->spec_n.resize((size_t)g); lj->spec_key.resize((size_t)g); lj->spec_total.resize((size_t)g); lj->spec_centroid.resize(3 * (size_t)g);
            lj->spec_center.resize(3 * (size_t)g); lj->spec_volume.resize((size_t)g); lj->spec_group.resize((size_t)g);
            const D2HItem parts[8] = {{&ctr, job.ctr, sizeof ctr}, {lj->spec_n.data(), job.b_n, (size_t)(8 * g)}, {lj->spec_total.data(), job.b_total, (size_t)(8 * g)},
                                      {lj->spec_centroid.data(), job.b_centroid, (size_t)(24 * g)}, {lj->spec_center.data(), job.b_center, (size_t)(24 * g)},
                                      {lj->spec_volume.data(), job.b_volume, (size_t)(8 * g)}, {lj->spec_key.data(), job.b_key, (size_t)(8 * g)},
                                      {lj->spec_group.data(), job.b_group, (size_t)(4 * g)}};
            HIP_TRY(ctx, d2h_many(ctx, parts, 8));
            HIP_TRY(ctx, ctx_sync(ctx));
            lj->spec_rows = g;
            return 0;
        }
        HIP_TRY(ctx, d2h(ctx, &ctr, job.ctr, sizeof ctr));
        HIP_TRY(ctx, ctx_sync(ctx));
        return 0;
    };
    {
        const int rc_fetch = fetch();
        if (rc_fetch) return rc_fetch;
    }
    while (lj->whole_map && ctr.overflow != 0u) {
        // The job is run again, ONCE (every list of the job reads the new run), when the typical-size arena was too small
        // for this map (bits 0 / 1), or when the map has unit tiles and the job was enqueued without their two launches (bit 2,
        // Job::unit_form).  The second run has both: the worst-case arena and the unit launches -- a first run without the unit
        // launches does not know how many ids its unit tiles would have asked for.
        if (lj->worst_case) return fail(ctx, PDBEDA_ERR_STATE, "whole-map labelling overflowed its worst-case arena");
        if (lj->voxels_done) return fail(ctx, PDBEDA_ERR_STATE, "whole-map labelling: overflow noticed after the voxel lists were made");
        lj->arena.put();      // the first run's arena goes back BEFORE the larger one is carved: the job's peak is the larger of the two, not their sum (stream order: the first run's kernels are done -- ctx_sync above)
        int rc = whole_map_enqueue(lj->map, lj->cut_pos, lj->cut_neg, lj->want_pos, lj->want_neg, lj->flags, true, lj);
        if (rc) return rc;      // (the record holds no arena now)
        lj->reruns += 1;
        const int rc_fetch = fetch();
        if (rc_fetch) return rc_fetch;
    }
    if (!lj->whole_map && ctr.unit_wait_failed) return fail(ctx, PDBEDA_ERR_DEVICE, "sphere batch: the device's volumes outgrew what the host sized the job for");
    job_record_counts(lj, ctr);
    return 0;
}

// Diagnostic: device counters of the labelling job behind a list:
// out[0..7] = run ids, component ids, runs of the job (1 = the typical-size arena overflowed and the job ran again), blobs,
// unit tiles by cause (run slots, -, component table), bytes of the job's arena.
extern "C" int pdbeda_bloblist_counters(pdbeda_bloblist *bl, int64_t *out) {
    if (!bl || bl->freed || !out) return PDBEDA_ERR_ARGUMENT;
    const LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Counters c;
    HIP_TRY(ctx, d2h(ctx, &c, lj->job.ctr, sizeof c));
    HIP_TRY(ctx, ctx_sync(ctx));
    out[0] = c.n_runs; out[1] = c.n_comps; out[2] = lj->reruns; out[3] = c.n_blobs;
    out[4] = out[5] = out[6] = 0;
    out[7] = (int64_t)(lj->bytes ? lj->bytes : lj->arena.cap);   // bytes of device memory the job needs (its arena, if recycled, may be up to twice that)
    if (lj->whole_map && lj->job.tile_mode) {   // tiles off the fast path by kind: tile_mode 1 = unit tile (run slots / values), 2 = wide tile (more than CCAP components, united in LDS all the same), 3 = unit tile (no ids left for a wide tile's components)
        const int64_t n_tiles = (int64_t)lj->td.ctiles * lj->td.rtiles * lj->td.stiles;
        std::vector<uint8_t> mode(n_tiles);
        HIP_TRY(ctx, d2h(ctx, mode.data(), lj->job.tile_mode, n_tiles));
        HIP_TRY(ctx, ctx_sync(ctx));
        for (uint8_t v : mode) { if (v == 1) ++out[4]; else if (v == 2) ++out[5]; else if (v == 3) ++out[6]; }
    }
    return PDBEDA_OK;
}


extern "C" int64_t pdbeda_bloblist_count(pdbeda_bloblist *bl) {
    if (!bl || bl->freed) return PDBEDA_ERR_ARGUMENT;
    int rc = list_resolve_counts(bl);
    if (rc) return rc;
    const RankRange r = list_ranks(bl);
    return r.hi - r.lo;
}

extern "C" int pdbeda_bloblist_stats(pdbeda_bloblist *bl, int64_t *n, double *total_density, double *centroid, double *coord_center,
                                     double *volume, int64_t *first_key, int32_t *group) {
    if (!bl || bl->freed) return PDBEDA_ERR_ARGUMENT;
    int rc = list_resolve_counts(bl);
    if (rc) return rc;
    const LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    const Job &job = lj->job;
    const int64_t lo = list_ranks(bl).lo, cnt = list_ranks(bl).hi - lo;
    if (cnt == 0) return PDBEDA_OK;
    if (lj->whole_map && lj->spec_rows >= lo + cnt) {      // the rows that came with the counters
        if (n) memcpy(n, lj->spec_n.data() + lo, (size_t)(8 * cnt));
        if (total_density) memcpy(total_density, lj->spec_total.data() + lo, (size_t)(8 * cnt));
        if (centroid) memcpy(centroid, lj->spec_centroid.data() + 3 * lo, (size_t)(24 * cnt));
        if (coord_center) memcpy(coord_center, lj->spec_center.data() + 3 * lo, (size_t)(24 * cnt));
        if (volume) memcpy(volume, lj->spec_volume.data() + lo, (size_t)(8 * cnt));
        if (first_key) memcpy(first_key, lj->spec_key.data() + lo, (size_t)(8 * cnt));
        if (group) memcpy(group, lj->spec_group.data() + lo, (size_t)(4 * cnt));
        return PDBEDA_OK;
    }
    const D2HItem columns[7] = {{n, job.b_n + lo, (size_t)(8 * cnt)}, {total_density, job.b_total + lo, (size_t)(8 * cnt)},
                                {centroid, job.b_centroid + 3 * lo, (size_t)(24 * cnt)}, {coord_center, job.b_center + 3 * lo, (size_t)(24 * cnt)},
                                {volume, job.b_volume + lo, (size_t)(8 * cnt)}, {first_key, job.b_key + lo, (size_t)(8 * cnt)},
                                {group, job.b_group + lo, (size_t)(4 * cnt)}};
    HIP_TRY(ctx, d2h_many(ctx, columns, 7));      // (packed on the device: one copy instead of seven)
    HIP_TRY(ctx, ctx_sync(ctx));
    return PDBEDA_OK;
}

// Counters AND the first `guess` rows of a batch job's blob table in ONE host round trip (the batches of pdbeda_aggregate_cloud:
// a count and then the table were two waits each; under four workers on one GPU a wait costs a quarter of a millisecond).
// Rows beyond the blob count are stale arena bytes, copied and dropped.  Falls back to the two-step path when the guess was
// too small (or the list is not a whole batch job).
static int list_stats_one_trip(pdbeda_bloblist *bl, int64_t guess, std::vector<int64_t> &n, std::vector<double> &tot, std::vector<double> &cen,
                               std::vector<int32_t> &grp, const D2HItem *extra = nullptr) {      // (extra: one more result of the caller's, in the same pack and wait)
    LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    const Job &job = lj->job;
    guess = std::min<int64_t>(guess, (int64_t)job.blob_cap);
    const bool whole_job = !lj->whole_map && bl->vol_lo == 0 && bl->vol_hi == job.n_vols;
    const int64_t extra_bytes = extra ? (int64_t)extra->bytes + 64 : 0;
    if (!lj->have_counts && whole_job && guess > 0 && 44 * guess + 4096 + extra_bytes < (int64_t)pinned_room(ctx)) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        n.resize((size_t)guess); tot.resize((size_t)guess); cen.resize(3 * (size_t)guess); grp.resize((size_t)guess);
        Counters ctr;
        const D2HItem parts[6] = {{&ctr, job.ctr, sizeof ctr}, {n.data(), job.b_n, (size_t)(8 * guess)}, {tot.data(), job.b_total, (size_t)(8 * guess)},
                                  {cen.data(), job.b_centroid, (size_t)(24 * guess)}, {grp.data(), job.b_group, (size_t)(4 * guess)},
                                  extra ? *extra : D2HItem{nullptr, nullptr, 0}};
        HIP_TRY(ctx, d2h_many(ctx, parts, 6));
        HIP_TRY(ctx, ctx_sync(ctx));
        if (ctr.unit_wait_failed) return fail(ctx, PDBEDA_ERR_DEVICE, "sphere batch: the device's volumes outgrew what the host sized the job for");
        job_record_counts(lj, ctr);
        if ((int64_t)ctr.n_blobs <= guess) {
            const size_t nb = ctr.n_blobs;
            n.resize(nb); tot.resize(nb); cen.resize(3 * nb); grp.resize(nb);
            return PDBEDA_OK;
        }
        extra = nullptr;      // (the guess was too small for the table; the caller's extra result has arrived with this first wait all the same)
    }
    if (extra) HIP_TRY(ctx, d2h_each(ctx, extra, 1));      // (delivered by the waits below)
    const int64_t nb = pdbeda_bloblist_count(bl);
    if (nb < 0) return (int)nb;
    n.resize((size_t)nb); tot.resize((size_t)nb); cen.resize(3 * (size_t)nb); grp.resize((size_t)nb);
    return pdbeda_bloblist_stats(bl, n.data(), tot.data(), cen.data(), nullptr, nullptr, nullptr, grp.data());
}

// Voxel lists are materialised once per JOB (every list of a fused call reads its part of them).
static int list_materialise_voxels(pdbeda_bloblist *bl) {
    LabelJob *lj = bl->job;
    if (lj->voxels_done) return 0;
    pdbeda_ctx *ctx = lj->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {   // the job's blob count: one read of the counters per job, not one more here (every caller has resolved its counts;
        // a whole-map job that overflowed its typical-size arena has been run again by then)
        const int rc_counts = list_resolve_counts(bl);
        if (rc_counts) return rc_counts;
    }
    const Job &job = lj->job;
    const int64_t nb = lj->n_blobs;
    // total voxels unknown until the offsets scan; bound by key bits
    const int64_t max_vox = job.key_words * 64;
    Arena lists;      // (the job's only once the launches are queued: a failed call leaves the record without lists, and nothing lent)
    int rc = arena_carve(ctx, "voxel lists", &lists, [&](Carver &cv) {
        cv.take(lj->offsets_dev, nb + 1);
        cv.take(lj->cursor_dev, std::max<int64_t>(nb, 1));
        cv.take(lj->crs_dev, 3 * std::max<int64_t>(max_vox, 1));
    });
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_blob_offsets, dim3(1), dim3(1024), 0, st, job, lj->offsets_dev, lj->cursor_dev);
    if (job.total_words > 0)
        hipLaunchKernelGGL(k_voxel_lists, dim3(grid_for(job.total_words * 64, 256, 8192)), dim3(256), 0, st, job, lj->offsets_dev,
                           lj->cursor_dev, lj->crs_dev);
    HIP_TRY(ctx, hipGetLastError());
    lj->vox_arena = std::move(lists);
    lj->voxels_done = true;      // (enqueued: whatever reads the lists is ordered behind them on the stream, and waits there)
    return 0;
}

extern "C" int64_t pdbeda_bloblist_num_voxels(pdbeda_bloblist *bl) {
    if (!bl || bl->freed) return PDBEDA_ERR_ARGUMENT;
    int rc = list_resolve_counts(bl);
    if (rc) return rc;
    if (bl->n_voxels >= 0) return bl->n_voxels;
    rc = list_materialise_voxels(bl);
    if (rc) return rc;
    const LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    const RankRange r = list_ranks(bl);
    int64_t off[2] = {0, 0};
    HIP_TRY(ctx, d2h(ctx, &off[0], lj->offsets_dev + r.lo, 8));
    HIP_TRY(ctx, d2h(ctx, &off[1], lj->offsets_dev + r.hi, 8));
    HIP_TRY(ctx, ctx_sync(ctx));
    bl->n_voxels = off[1] - off[0];
    return bl->n_voxels;
}

extern "C" int pdbeda_bloblist_voxels(pdbeda_bloblist *bl, int32_t *crs, int64_t *blob_offsets) {
    if (!bl || bl->freed) return PDBEDA_ERR_ARGUMENT;
    int64_t nv = pdbeda_bloblist_num_voxels(bl);
    if (nv < 0) return (int)nv;
    const LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    const RankRange r = list_ranks(bl);
    const int64_t cnt = r.hi - r.lo;
    std::vector<int64_t> off(cnt + 1);
    HIP_TRY(ctx, d2h(ctx, off.data(), lj->offsets_dev + r.lo, 8 * (cnt + 1))); HIP_TRY(ctx, ctx_sync(ctx));
    const int64_t base = off[0];
    if (blob_offsets)
        for (int64_t i = 0; i <= cnt; ++i) blob_offsets[i] = off[i] - base;
    if (crs && nv > 0) HIP_TRY(ctx, d2h(ctx, crs, lj->crs_dev + 3 * base, 12 * nv)); HIP_TRY(ctx, ctx_sync(ctx));
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Blob shape descriptors (pdbeda_blobshape.h; no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// The launch graph of a list's FIRST call: two fills (box records INT_MIN, sums records 0), k_blobshape_box, k_blobshape_widths and a wait
// for the widest box (a list with a box of 2^15 voxels or more is refused here, in front of the moment launches); k_blobshape_sums,
// k_blobshape_finish, and the three row tables in one pack and one wait.  The scratch arena goes back to the pool in stream order whatever
// happens; results are registered for delivery (d2h_many) only behind the last launch.
static int list_moments_compute(pdbeda_bloblist *bl) {
    const int64_t nv = pdbeda_bloblist_num_voxels(bl);      // (resolves the counts and materialises the voxel lists)
    if (nv < 0) return (int)nv;
    const LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    const RankRange ranks = list_ranks(bl);
    const int64_t cnt = ranks.hi - ranks.lo;
    if (cnt == 0 || nv == 0) { bl->shape_done = true; return PDBEDA_OK; }
    // What the accumulators hold: F = fix_of(|rho|), bounded per voxel and per map by the quantum's rule (map_quantum in pdbeda_jobplan.h).  The low
    // limbs of the two-limb sums are below 2^32 per voxel and are read as signed 64-bit: fewer than 2^31 voxels in the list.  sum F is ONE 64-bit word,
    // and the high limb of F d d' is F * 2^30 / 2^32 at the most: a whole-map blob counts every stored voxel at most once (nothing wraps in the unique
    // box), so the map's bound holds for sum F and a quarter of it for the high limbs; a sphere / list batch may meet a stored voxel again through the
    // periodic wrap, so only its voxel count bounds it: the rule's wrapped-batch limit, refused below.
    if (cnt >= (1ll << 31) || nv >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "blob moments: a list of 2^31 blobs or voxels, or more");
    if (!lj->whole_map && nv >= (1ll << 24)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "blob moments: a sphere / list batch of 2^24 voxels or more");
    pdbeda_map *m = lj->map;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = map_fix_mul(m)) return rc;      // (known since the labelling call, unless the map was invalidated meanwhile)
    const size_t nb = (size_t)cnt;
    BlobShapeArgs a;
    unsigned long long *d_widest = nullptr;
    int32_t *d_i = nullptr;
    long long *d_l = nullptr;
    double *d_d = nullptr;
    Arena arena;
    const int rc_arena = arena_carve(ctx, "blob moments", &arena, [&](Carver &cv) {      // (back to the pool on every way out, in stream order: whatever a failed call left queued runs before the arena's next user)
        cv.take(a.park_rho, (size_t)nv); cv.take(a.park_blob, (size_t)nv);
        cv.take(a.box, BS_BOX * nb); cv.take(a.rec, BS_REC * nb);
        cv.take(d_widest, 8);      // (right behind the sums records: ONE fill clears both)
        cv.take(d_i, 10 * nb);
        cv.take(d_l, 9 * nb);
        cv.take(d_d, 10 * nb);
    });
    if (rc_arena) return rc_arena;
    a.geom = m->geom_dev; a.dens = m->dens;
    a.crs = lj->crs_dev; a.off = lj->offsets_dev + ranks.lo; a.cnt = cnt;
    a.fix_mul = m->fix_mul;
    hipStream_t st = ctx->stream;
    const unsigned chunks = (unsigned)((nv + BS_CHUNK - 1) / BS_CHUNK);
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)a.box, (int)0x80000000u, BS_BOX * nb, st));
    HIP_TRY(ctx, hipMemsetAsync(a.rec, 0, (size_t)((char *)(d_widest + 8) - (char *)a.rec), st));      // (the sums records and the widest box behind them)
    { PROF(ctx, "k_blobshape_box"); hipLaunchKernelGGL(k_blobshape_box, dim3(chunks), dim3(256), 0, st, a); }
    { PROF(ctx, "k_blobshape_widths"); hipLaunchKernelGGL(k_blobshape_widths, dim3(grid_for(cnt, 256, 1024)), dim3(256), 0, st, a.box, cnt, d_widest); }
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long widest = 0;
    HIP_TRY(ctx, d2h(ctx, &widest, d_widest, 8));
    HIP_TRY(ctx, ctx_sync(ctx));
    if (widest >= (unsigned long long)BS_MAX_WIDTH)
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "blob moments: a blob's box is %llu voxels wide (the limit is %d)", widest, BS_MAX_WIDTH - 1);
    { PROF(ctx, "k_blobshape_sums"); hipLaunchKernelGGL(k_blobshape_sums, dim3(chunks), dim3(256), 0, st, a); }
    { PROF(ctx, "k_blobshape_finish"); hipLaunchKernelGGL(k_blobshape_finish, dim3(grid_for(cnt, 256)), dim3(256), 0, st, a.box, a.rec, cnt, 1.0 / m->fix_mul, d_i, d_l, d_d); }
    HIP_TRY(ctx, hipGetLastError());
    bl->shape_i.resize(10 * nb); bl->shape_l.resize(9 * nb); bl->shape_d.resize(10 * nb);
    const D2HItem rows[3] = {{bl->shape_i.data(), d_i, sizeof(int32_t) * 10 * nb}, {bl->shape_l.data(), d_l, sizeof(long long) * 9 * nb}, {bl->shape_d.data(), d_d, sizeof(double) * 10 * nb}};
    HIP_TRY(ctx, d2h_many(ctx, rows, 3));
    HIP_TRY(ctx, ctx_sync(ctx));
    bl->shape_done = true;
    return PDBEDA_OK;
}

extern "C" int pdbeda_bloblist_moments(pdbeda_bloblist *bl, int32_t *box_lo, int32_t *box_hi, int32_t *extreme_crs, float *extreme, int64_t *s1, int64_t *s2,
                                       double *sw, double *sw1, double *sw2) {
    if (!bl || bl->freed) return PDBEDA_ERR_ARGUMENT;
    if (bl->job->ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    if (!bl->shape_done)
        if (int rc = list_moments_compute(bl)) return rc;
    const size_t cnt = bl->shape_l.size() / 9;
    for (size_t b = 0; b < cnt; ++b) {
        const int32_t *ri = bl->shape_i.data() + 10 * b;
        const int64_t *rl = bl->shape_l.data() + 9 * b;
        const double *rd = bl->shape_d.data() + 10 * b;
        if (box_lo) memcpy(box_lo + 3 * b, ri, 12);
        if (box_hi) memcpy(box_hi + 3 * b, ri + 3, 12);
        if (extreme_crs) memcpy(extreme_crs + 3 * b, ri + 6, 12);
        if (extreme) memcpy(extreme + b, ri + 9, 4);
        if (s1) memcpy(s1 + 3 * b, rl, 24);
        if (s2) memcpy(s2 + 6 * b, rl + 3, 48);
        if (sw) sw[b] = rd[0];
        if (sw1) memcpy(sw1 + 3 * b, rd + 1, 24);
        if (sw2) memcpy(sw2 + 6 * b, rd + 4, 48);
    }
    return PDBEDA_OK;
}

extern "C" int pdbeda_bloblist_labels(pdbeda_bloblist *bl, int32_t *labels_host) {
    if (!bl || bl->freed || !labels_host) return PDBEDA_ERR_ARGUMENT;
    const LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    if (!lj->whole_map) return fail(ctx, PDBEDA_ERR_STATE, "dense labels exist only for whole-map blob lists");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {   // a job whose unit tiles waited in vain (k_face_merge) has no valid labels either: the same check the blob table makes
        const int rc_counts = list_resolve_counts(bl);
        if (rc_counts) return rc_counts;
    }
    const Geom &g = lj->map->geom;
    const int uc = g.unique_ncrs[0], ur = g.unique_ncrs[1], us = g.unique_ncrs[2];
    const int64_t nvox = (int64_t)uc * ur * us;
    // scratch: [signed volume if it was not requested at labelling time] + decoded volume
    Arena a;
    int32_t *decoded = nullptr, *tmp = nullptr;
    int rc = arena_carve(ctx, "labels", &a, [&](Carver &cv) { cv.take(decoded, nvox); if (!job_keeps_labels(lj)) cv.take(tmp, nvox); });
    if (rc) return rc;
    const int32_t *signed_vol = job_signed_labels(lj, tmp);
    hipLaunchKernelGGL(k_labels_decode, dim3(grid_for(nvox, 256, 4096)), dim3(256), 0, ctx->stream, signed_vol, nvox, bl->sign, decoded);
    hipError_t e = d2h(ctx, labels_host, decoded, 4 * nvox);
    if (e == hipSuccess) e = ctx_sync(ctx);
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "labels: %s", hipGetErrorString(e));
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Nearest blob of another list (pdbeda_blobnear.h; no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// The launch graph: the packed table to the device (one staged copy), one fill (the records start as "no pair"), b's signed volume by
// launch_labels when its job kept none, k_blobnear_scan over the chunks of a's voxel lists, k_blobnear_finish, and the rows in one copy and
// one wait.  Every refusal comes before the first launch; the scratch arena goes back to the pool in stream order whatever happens; the
// rows are registered for delivery only behind the last launch.
extern "C" int pdbeda_bloblist_nearest(pdbeda_bloblist *a, pdbeda_bloblist *b, const int32_t *offsets, int64_t n_offsets, int32_t *index, int32_t *partner,
                                       int32_t *voxel, int32_t *partner_voxel) {
    if (!a || !b || a->freed || b->freed) return PDBEDA_ERR_ARGUMENT;
    const LabelJob *ja = a->job, *jb = b->job;
    pdbeda_ctx *ctx = ja->ctx;
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    if (a == b) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: a list against itself");
    if (jb->ctx != ctx) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: the lists belong to different contexts");
    if (!ja->whole_map || !jb->whole_map) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: both lists must be whole-map lists");
    const Geom &g = ja->map->geom, &gb = jb->map->geom;
    for (int k = 0; k < 3; ++k)
        if (g.unique_ncrs[k] != gb.unique_ncrs[k]) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: the maps of the two lists have different uniqueNcrs");
    if (n_offsets < 0 || n_offsets > BN_MAX_OFFSETS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: a table of %lld offsets (the limit is %d)", (long long)n_offsets, BN_MAX_OFFSETS);
    if (n_offsets > 0 && !offsets) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: no offsets table");
    std::vector<uint32_t> packed((size_t)n_offsets);
    for (int64_t t = 0; t < n_offsets; ++t) {
        const int32_t *o = offsets + 3 * t;
        for (int k = 0; k < 3; ++k)
            if (o[k] < -BN_MAX_COMPONENT || o[k] > BN_MAX_COMPONENT)
                return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: offset %lld has the component %d (the limit is +-%d)", (long long)t, o[k], BN_MAX_COMPONENT);
        packed[(size_t)t] = blobnear_pack(o[0], o[1], o[2]);
    }
    // the counts of both lists first: a job that overflowed its typical-size arena runs again now
    if (int rc = list_resolve_counts(a)) return rc;
    if (int rc = list_resolve_counts(b)) return rc;
    const RankRange ra = list_ranks(a), rb = list_ranks(b);
    const int64_t cnt = ra.hi - ra.lo, cnt_b = rb.hi - rb.lo;
    auto no_pairs = [&]() {
        for (int64_t i = 0; i < cnt; ++i) {
            if (index) index[i] = -1;
            if (partner) partner[i] = -1;
            for (int k = 0; k < 3; ++k) { if (voxel) voxel[3 * i + k] = 0; if (partner_voxel) partner_voxel[3 * i + k] = 0; }
        }
        return PDBEDA_OK;
    };
    if (cnt == 0 || cnt_b == 0 || n_offsets == 0) return no_pairs();
    const int64_t nv = pdbeda_bloblist_num_voxels(a);      // (materialises a's voxel lists)
    if (nv < 0) return (int)nv;
    if (nv == 0) return no_pairs();
    if (cnt >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "nearest blobs: a list of 2^31 blobs or more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nvox = (int64_t)g.unique_ncrs[0] * g.unique_ncrs[1] * g.unique_ncrs[2];
    const size_t nb = (size_t)cnt;
    BlobNearArgs args;
    uint32_t *d_table = nullptr;
    int32_t *d_rows = nullptr, *tmp = nullptr;
    Arena arena;
    const int rc_arena = arena_carve(ctx, "nearest blobs", &arena, [&](Carver &cv) {
        cv.take(args.best, nb);
        cv.take(d_table, (size_t)n_offsets);
        cv.take(d_rows, 8 * nb);
        if (!job_keeps_labels(jb)) cv.take(tmp, (size_t)nvox);
    });
    if (rc_arena) return rc_arena;
    std::vector<int32_t> rows(8 * nb);
    auto run = [&]() -> int {
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, h2d_one(ctx, d_table, packed.data(), sizeof(uint32_t) * (size_t)n_offsets));
        HIP_TRY(ctx, hipMemsetAsync(args.best, 0xFF, sizeof(unsigned long long) * nb, st));
        args.crs = ja->crs_dev; args.off = ja->offsets_dev + ra.lo; args.cnt = cnt;
        args.labels = job_signed_labels(jb, tmp); args.sign = b->sign;
        args.uc = g.unique_ncrs[0]; args.ur = g.unique_ncrs[1]; args.us = g.unique_ncrs[2];
        args.table = d_table; args.n_off = (int32_t)n_offsets;
        // positions per thread: one while that gives fewer than BN_MIN_GROUPS workgroups (a walk is a chain of read latencies: a short list
        // wants its walks side by side, not eight in a row in one thread), then the power of two that keeps about that many
        args.per_thread = 1;
        while (args.per_thread < BN_PER_THREAD && nv > (int64_t)256 * args.per_thread * BN_MIN_GROUPS) args.per_thread *= 2;
        const int64_t chunk = (int64_t)256 * args.per_thread;
        const unsigned chunks = (unsigned)((nv + chunk - 1) / chunk);
        { PROF(ctx, "k_blobnear_scan"); hipLaunchKernelGGL(k_blobnear_scan, dim3(chunks), dim3(256), 0, st, args); }
        { PROF(ctx, "k_blobnear_finish"); hipLaunchKernelGGL(k_blobnear_finish, dim3(grid_for(cnt, 256)), dim3(256), 0, st, args, d_rows); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, d2h(ctx, rows.data(), d_rows, sizeof(int32_t) * 8 * nb));
        HIP_TRY(ctx, ctx_sync(ctx));
        return PDBEDA_OK;
    };
    if (const int rc = run()) {
        (void)ctx_sync(ctx);      // (`packed` is freed on return and the table's copy may be a hipMemcpyAsync out of it: nothing of a failed call may still read it)
        return rc;
    }
    for (size_t i = 0; i < nb; ++i) {
        const int32_t *r = rows.data() + 8 * i;
        if (index) index[i] = r[0];
        if (partner) partner[i] = r[1];
        if (voxel) memcpy(voxel + 3 * i, r + 2, 12);
        if (partner_voxel) memcpy(partner_voxel + 3 * i, r + 5, 12);
    }
    return PDBEDA_OK;
}

extern "C" int pdbeda_bloblist_free(pdbeda_bloblist *bl) {
    if (!bl) return PDBEDA_ERR_ARGUMENT;
    if (bl->freed) return PDBEDA_ERR_STATE;
    LabelJob *lj = bl->job;
    pdbeda_ctx *ctx = lj->ctx;
    bl->freed = true;
    ctx->live_handles--;
    bl->shape_done = false;      // (the rows go with the list, also while another list keeps the job alive)
    std::vector<int32_t>().swap(bl->shape_i); std::vector<int64_t>().swap(bl->shape_l); std::vector<double>().swap(bl->shape_d);
    if (--lj->live == 0) {
        // last list of the job.  Arenas are recycled only inside this context, i.e. by work that
        // is enqueued later on the SAME stream, so stream order protects them: no host sync.
        delete lj;
    }
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Density peaks (pdbeda_peaks.h): local extrema of a map, tied to the blobs of a whole-map list
// ------------------------------------------------------------------------------------
// One job serves one list, or the two lists of a fused call.  The call enqueues the stencil and the finish kernel and returns;
// the first accessor reads the counters (one wait), runs the job again in an arena of the size the counters ask for when the
// typical-size one was too small, and brings the keys over to order them: the list order is the ascending order of the keys
// (std::sort on the host -- DESIGN.md 4.5 has the measurement behind that choice), applied to the columns as they are fetched.
struct PeakJob {
    pdbeda_ctx *ctx = nullptr;
    pdbeda_map *map = nullptr;
    Arena arena;
    PeakJobArgs args;
    pdbeda_bloblist *blobs[2] = {nullptr, nullptr};   // the caller's lists (alive until the first accessor has returned: include/pdbeda.h)
    int refs = 0, reruns = 0;
    size_t bytes = 0;
    bool resolved = false;
    int64_t n[2] = {0, 0}, tested[2] = {0, 0};
    std::vector<uint32_t> order[2];                   // list position -> arena slot
    std::vector<uint32_t> pos[2];                     // list position -> c-major position of the peak's voxel (the low word of its key)
    // pdbeda_peaklist_basins: the rows of each list, made by the first call and kept until the job goes
    struct BasinRows {
        bool done = false;
        std::vector<int64_t> n, s1;
        std::vector<double> sum, sw1;
        std::vector<float> saddle;
        std::vector<int32_t> neighbour;
        int64_t counters[4] = {0, 0, 0, 0};
    } basins[2];
};
struct pdbeda_peaklist {
    PeakJob *job = nullptr;
    int plane = 0;
    bool freed = false;
};

// Carve and enqueue.  seg[p]: keys a tile's segment of plane p holds; cap[p]: peaks its compact list holds.  The label volumes of lists that were made without PDBEDA_FLAG_LABELS
// are written into the job's own arena (two lists of one fused labelling job share one signed volume).
static int peaks_enqueue(PeakJob *pj, const int64_t cap[2], const int64_t seg[2]) {
    pdbeda_ctx *ctx = pj->ctx;
    pdbeda_map *m = pj->map;
    PeakJobArgs &a = pj->args;
    const int64_t nvox = (int64_t)a.uc * a.ur * a.us;
    const int32_t *have[2] = {nullptr, nullptr};
    bool need_own[2] = {false, false};
    for (int p = 0; p < a.n_planes; ++p) {
        pdbeda_bloblist *bl = pj->blobs[p];
        if (!bl) continue;
        if (job_keeps_labels(bl->job)) have[p] = bl->job->labels_dev;
        else need_own[p] = true;
    }
    // (the two lists of ONE fused labelling job: one signed volume serves both planes)
    const bool shared = need_own[0] && need_own[1] && pj->blobs[0]->job == pj->blobs[1]->job;
    if (shared) need_own[1] = false;
    Arena arena;      // (the job's only once the launches are queued: a failed run leaves the record without an arena)
    const int rc = arena_carve(ctx, "peak search", &arena, [&](Carver &cv) {
        a.ctr = cv.take<PeakCounters>(1);
        int32_t *own[2] = {nullptr, nullptr};
        for (int p = 0; p < a.n_planes; ++p) {
            PeakPlane &pl = a.plane[p];
            const size_t k = (size_t)cap[p];
            pl.cap = (unsigned long long)cap[p];
            pl.seg = (uint32_t)seg[p];
            pl.seg_keys = cv.take<unsigned long long>((size_t)a.n_tiles * (size_t)seg[p]);
            pl.tile_count = cv.take<uint32_t>((size_t)a.n_tiles);
            pl.tile_tested = cv.take<uint32_t>((size_t)a.n_tiles);
            pl.tile_off = cv.take<uint32_t>((size_t)a.n_tiles);
            pl.keys = cv.take<unsigned long long>(k);
            pl.xyz = cv.take<double>(3 * k);
            pl.refined = cv.take<double>(k);
            pl.crs = cv.take<int32_t>(3 * k);
            pl.height = cv.take<float>(k);
            pl.blob = cv.take<int32_t>(k);
            pl.border = cv.take<uint8_t>(k);
            if (need_own[p]) own[p] = cv.take<int32_t>((size_t)nvox);
            pl.labels = have[p] ? have[p] : (need_own[p] ? own[p] : ((p == 1 && shared) ? own[0] : nullptr));
        }
        pj->bytes = cv.off;
    });
    if (rc) return rc;
    hipError_t e = hipSuccess;
    {   // (nothing to clear: the stencil stores every tile's counts, the scan every counter)
        for (int p = 0; p < a.n_planes; ++p)
            if (need_own[p]) (void)job_signed_labels(pj->blobs[p]->job, const_cast<int32_t *>(a.plane[p].labels));      // (written into the piece carved above: the list's job is one of this map)
        const dim3 grid((unsigned)((a.uc + PK_C - 1) / PK_C), (unsigned)((a.ur + PK_R - 1) / PK_R), (unsigned)((a.us + PK_S - 1) / PK_S));
        { PROF(ctx, "k_peak_stencil"); hipLaunchKernelGGL(k_peak_stencil, grid, dim3(PK_THREADS), 0, ctx->stream, a, m->dens); }
        { PROF(ctx, "k_peak_scan"); hipLaunchKernelGGL(k_peak_scan, dim3(1), dim3(PK_SCAN_THREADS), 0, ctx->stream, a); }
        const int64_t most = (int64_t)a.n_tiles * std::max<int64_t>(seg[0], a.n_planes > 1 ? seg[1] : 0);
        { PROF(ctx, "k_peak_finish"); hipLaunchKernelGGL(k_peak_finish, dim3(grid_for(most, 256, 2048)), dim3(256), 0, ctx->stream, a, m->dens, m->geom_dev); }
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "peak search launch: %s", hipGetErrorString(e));
    pj->arena = std::move(arena);
    return PDBEDA_OK;
}

// A blob list handed to a peak call: a live whole-map list of the same map, sign and float32 cutoff.  Its counters are read
// here (a wait; a labelling job whose typical-size arena overflowed runs again now), so that its label volume is final.
static int peaks_check_blobs(pdbeda_map *m, pdbeda_bloblist *bl, int sign, float cutoff) {
    if (!bl) return PDBEDA_OK;
    pdbeda_ctx *ctx = m->ctx;
    const LabelJob *lj = bl->job;
    if (bl->freed || !lj->whole_map || lj->map != m || lj->ctx != ctx) return fail(ctx, PDBEDA_ERR_ARGUMENT, "peaks: the blob list is not a whole-map list of this map");
    if (bl->sign != sign || (sign > 0 ? lj->cut_pos : lj->cut_neg) != cutoff)
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "peaks: the blob list was made with another cutoff (%g, asked for %g)", (double)(bl->sign > 0 ? lj->cut_pos : lj->cut_neg), (double)cutoff);
    return list_resolve_counts(bl);
}

static int peaks_impl(pdbeda_map *m, int n_planes, const float cut[2], const int sign[2], pdbeda_bloblist *const blobs[2], pdbeda_peaklist **out[2]) {
    pdbeda_ctx *ctx = m->ctx;
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Geom &g = m->geom;
    const int64_t nvox = (int64_t)g.unique_ncrs[0] * g.unique_ncrs[1] * g.unique_ncrs[2];
    if (nvox >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "grid too large");       // (the c-major position is the low word of a key)
    const TileGrid tg = tile_grid(g.unique_ncrs, PK_C, PK_R, PK_S);
    const int64_t n_tiles = tg.n;
    if ((tg.refusal & TILES_AXIS) || n_tiles * 512 >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "grid too large");      // (a tile holds at most 512 peaks: no two are neighbours)
    for (int p = 0; p < n_planes; ++p) {
        const int rc = peaks_check_blobs(m, blobs[p], sign[p], cut[p]);
        if (rc) return rc;
    }
    std::unique_ptr<PeakJob> pj(new PeakJob());
    pj->ctx = ctx;
    pj->map = m;
    memset(&pj->args, 0, sizeof pj->args);
    PeakJobArgs &a = pj->args;
    a.n_planes = n_planes;
    a.uc = g.unique_ncrs[0]; a.ur = g.unique_ncrs[1]; a.us = g.unique_ncrs[2];
    a.nc = g.ncrs[0]; a.nr = g.ncrs[1];
    a.n_tiles = (int32_t)n_tiles;
    // typical size: a peak per 64 voxels of a tile (a smooth map at 1.5 sigma has one per several hundred; white noise, one per 27, runs twice)
    int64_t cap[2] = {0, 0}, seg[2] = {0, 0};
    for (int p = 0; p < n_planes; ++p) {
        a.plane[p].cut = cut[p];
        a.plane[p].sign = sign[p];
        pj->blobs[p] = blobs[p];
        seg[p] = PK_C * PK_R * PK_S / 64;
        cap[p] = n_tiles * seg[p];
    }
    const int rc = peaks_enqueue(pj.get(), cap, seg);
    if (rc) return rc;
    for (int p = 0; p < n_planes; ++p) {
        pdbeda_peaklist *pl = new pdbeda_peaklist();
        pl->job = pj.get();
        pl->plane = p;
        pj->refs++;
        ctx->live_handles++;
        *out[p] = pl;
    }
    pj.release();      // (the lists own the job now: pdbeda_peaklist_free)
    return PDBEDA_OK;
}

extern "C" int pdbeda_map_peaks(pdbeda_map *m, float cutoff, pdbeda_bloblist *blobs, pdbeda_peaklist **out) {
    if (!m || !out) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    if (cutoff == 0.0f || cutoff != cutoff) return fail(m->ctx, PDBEDA_ERR_ARGUMENT, "cutoff must be non-zero");
    const float cut[2] = {cutoff, 0.0f};
    const int sign[2] = {cutoff > 0 ? 1 : -1, 0};
    pdbeda_bloblist *const bl[2] = {blobs, nullptr};
    pdbeda_peaklist **outs[2] = {out, nullptr};
    return peaks_impl(m, 1, cut, sign, bl, outs);
}

extern "C" int pdbeda_map_peaks_pm(pdbeda_map *m, float cutoff_pos, float cutoff_neg, pdbeda_bloblist *green, pdbeda_bloblist *red,
                                   pdbeda_peaklist **pos, pdbeda_peaklist **neg) {
    if (!m || !pos || !neg) return PDBEDA_ERR_ARGUMENT;
    *pos = *neg = nullptr;
    if (!(cutoff_pos > 0.0f) || !(cutoff_neg < 0.0f)) return fail(m->ctx, PDBEDA_ERR_ARGUMENT, "need cutoff_pos > 0 > cutoff_neg");
    const float cut[2] = {cutoff_pos, cutoff_neg};
    const int sign[2] = {1, -1};
    pdbeda_bloblist *const bl[2] = {green, red};
    pdbeda_peaklist **outs[2] = {pos, neg};
    return peaks_impl(m, 2, cut, sign, bl, outs);
}

static int peaks_resolve(PeakJob *pj) {
    if (pj->resolved) return 0;
    pdbeda_ctx *ctx = pj->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int np = pj->args.n_planes;
    PeakCounters c;
    for (;;) {
        HIP_TRY(ctx, d2h(ctx, &c, pj->args.ctr, sizeof c));
        HIP_TRY(ctx, ctx_sync(ctx));
        bool over = false;
        for (int p = 0; p < np; ++p) over = over || c.max_tile[p] > pj->args.plane[p].seg || c.peaks[p] > pj->args.plane[p].cap;
        if (!over) break;
        // the typical-size arena was too small for this map: once more, in one of the size the counters name
        if (pj->reruns) return fail(ctx, PDBEDA_ERR_STATE, "peak search overflowed an arena sized from its own count");
        int64_t cap[2] = {0, 0}, seg[2] = {0, 0};
        for (int p = 0; p < np; ++p) {
            seg[p] = std::max<int64_t>((int64_t)pj->args.plane[p].seg, (int64_t)c.max_tile[p]);
            cap[p] = std::max<int64_t>(1, (int64_t)c.peaks[p]);
        }
        pj->arena.put();      // the first run's arena goes back BEFORE the one of the counters' size is carved: the peak is the larger of the two, not their sum (stream order: the first run is done -- ctx_sync above)
        const int rc = peaks_enqueue(pj, cap, seg);
        if (rc) return rc;      // (the record holds no arena now)
        pj->reruns = 1;
    }
    std::vector<unsigned long long> keys[2];
    for (int p = 0; p < np; ++p) {
        pj->n[p] = (int64_t)c.peaks[p];
        pj->tested[p] = (int64_t)c.tested[p];
        keys[p].resize((size_t)pj->n[p]);
        HIP_TRY(ctx, d2h(ctx, keys[p].data(), pj->args.plane[p].keys, 8 * (size_t)pj->n[p]));
    }
    HIP_TRY(ctx, ctx_sync(ctx));
    const auto sort_t0 = std::chrono::steady_clock::now();
    for (int p = 0; p < np; ++p) {
        std::vector<uint32_t> &ord = pj->order[p];
        std::vector<std::pair<unsigned long long, uint32_t>> kv(keys[p].size());      // (sorted in place: no indirection in the comparisons)
        for (size_t i = 0; i < kv.size(); ++i) kv[i] = {keys[p][i], (uint32_t)i};
        std::sort(kv.begin(), kv.end());                                              // (keys are unique: one order)
        ord.resize(kv.size());
        pj->pos[p].resize(kv.size());
        for (size_t i = 0; i < kv.size(); ++i) { ord[i] = kv[i].second; pj->pos[p][i] = (uint32_t)(kv[i].first & 0xffffffffull); }
    }
    if (ctx->profiling) ctx->prof_host.push_back({"host_peak_sort", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - sort_t0).count()});
    pj->resolved = true;
    return 0;
}

extern "C" int64_t pdbeda_peaklist_count(pdbeda_peaklist *pl) {
    if (!pl || pl->freed) return PDBEDA_ERR_ARGUMENT;
    const int rc = peaks_resolve(pl->job);
    if (rc) return rc;
    return pl->job->n[pl->plane];
}

template <typename T>
static void peaks_permute(const std::vector<uint32_t> &ord, const std::vector<T> &src, T *dst, int width) {
    for (size_t i = 0; i < ord.size(); ++i)
        for (int k = 0; k < width; ++k) dst[width * i + k] = src[(size_t)width * ord[i] + k];
}

extern "C" int pdbeda_peaklist_rows(pdbeda_peaklist *pl, int32_t *crs, float *height, double *refined_xyz, double *refined_height,
                                    int32_t *blob, uint8_t *on_border) {
    if (!pl || pl->freed) return PDBEDA_ERR_ARGUMENT;
    PeakJob *pj = pl->job;
    const int rc = peaks_resolve(pj);
    if (rc) return rc;
    pdbeda_ctx *ctx = pj->ctx;
    const PeakPlane &dp = pj->args.plane[pl->plane];
    const size_t n = (size_t)pj->n[pl->plane];
    if (n == 0) return PDBEDA_OK;
    std::vector<int32_t> h_crs(crs ? 3 * n : 0), h_blob(blob ? n : 0);
    std::vector<float> h_height(height ? n : 0);
    std::vector<double> h_xyz(refined_xyz ? 3 * n : 0), h_ref(refined_height ? n : 0);
    std::vector<uint8_t> h_border(on_border ? n : 0);
    if (crs) HIP_TRY(ctx, d2h(ctx, h_crs.data(), dp.crs, 12 * n));
    if (height) HIP_TRY(ctx, d2h(ctx, h_height.data(), dp.height, 4 * n));
    if (refined_xyz) HIP_TRY(ctx, d2h(ctx, h_xyz.data(), dp.xyz, 24 * n));
    if (refined_height) HIP_TRY(ctx, d2h(ctx, h_ref.data(), dp.refined, 8 * n));
    if (blob) HIP_TRY(ctx, d2h(ctx, h_blob.data(), dp.blob, 4 * n));
    if (on_border) HIP_TRY(ctx, d2h(ctx, h_border.data(), dp.border, n));
    HIP_TRY(ctx, ctx_sync(ctx));
    const std::vector<uint32_t> &ord = pj->order[pl->plane];
    if (crs) peaks_permute(ord, h_crs, crs, 3);
    if (height) peaks_permute(ord, h_height, height, 1);
    if (refined_xyz) peaks_permute(ord, h_xyz, refined_xyz, 3);
    if (refined_height) peaks_permute(ord, h_ref, refined_height, 1);
    if (blob) peaks_permute(ord, h_blob, blob, 1);
    if (on_border) peaks_permute(ord, h_border, on_border, 1);
    return PDBEDA_OK;
}

extern "C" int pdbeda_peaklist_counters(pdbeda_peaklist *pl, int64_t *out) {
    if (!pl || pl->freed || !out) return PDBEDA_ERR_ARGUMENT;
    const int rc = peaks_resolve(pl->job);
    if (rc) return rc;
    out[0] = pl->job->tested[pl->plane];
    out[1] = pl->job->n[pl->plane];
    out[2] = pl->job->reruns;
    out[3] = (int64_t)pl->job->bytes;
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Peak basins (pdbeda_basins.h; no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// The launch graph of a call that computes: (a map with NaN / infinite voxels only: k_partition_range and a wait for the quantum;) one fill
// of the accumulators and flags, the peaks' box positions up, k_basin_parent, then batches of BN_BATCH k_basin_jump rounds with ONE wait per
// batch for the batch's changed-flags (a bounded loop: BN_MAX_ROUNDS rounds at the most, then an error; a round behind one that changed
// nothing reads that round's flag and returns), k_basin_mark, k_basin_resolve,
// k_basin_sums, k_basin_decode when the volume is asked for, and one wait for the accumulators (and the volume).  The integers become the
// rows on the host.  The scratch arena goes back to the pool in stream order whatever happens.
static int basins_compute(pdbeda_peaklist *pl, int32_t *basin_host) {
    PeakJob *pj = pl->job;
    pdbeda_ctx *ctx = pj->ctx;
    pdbeda_map *m = pj->map;
    const int p = pl->plane;
    const PeakJobArgs &pa = pj->args;
    const PeakPlane &pp = pa.plane[p];
    const int uc = pa.uc, ur = pa.ur, us = pa.us;
    const int64_t nbox = (int64_t)uc * ur * us;      // (< 2^31: peaks_impl)
    const size_t np = (size_t)pj->n[p];
    PeakJob::BasinRows &br = pj->basins[p];
    if (np == 0) {      // no peak: every significant voxel (there are some only beside NaNs) is an orphan
        if (basin_host) std::fill(basin_host, basin_host + nbox, (int32_t)-1);
        br.counters[0] = br.counters[1] = pj->tested[p];
        br.counters[2] = br.counters[3] = 0;
        br.done = true;
        return PDBEDA_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (m->fix_mul == 0.0 && !m->fix_refused) {      // (a wait when the map's range is not known yet: before anything is staged)
        const int rc = map_fix_mul(m);
        if (rc && !m->fix_refused) return rc;
    }
    // the peaks' voxels in list order, as box positions
    std::vector<int32_t> peak_box(np);
    for (size_t i = 0; i < np; ++i) {
        const uint32_t pos = pj->pos[p][i];
        const int64_t s = pos % (uint32_t)us, cr = pos / (uint32_t)us, r = cr % ur, c = cr / ur;
        peak_box[i] = (int32_t)((s * ur + r) * uc + c);
    }
    BasinArgs a;
    memset(&a, 0, sizeof a);
    int32_t *d_peak_box = nullptr;
    uint32_t *d_flags = nullptr;
    unsigned long long *d_range = nullptr;
    size_t bytes = 0;
    Arena arena;
    const int rc_arena = arena_carve(ctx, "peak basins", &arena, [&](Carver &cv) {
        cv.take(a.up, (size_t)nbox);
        cv.take(d_peak_box, np);
        cv.take(a.acc, BN_ACC * np);      // (the accumulators and everything behind them: ONE fill clears all)
        cv.take(a.orphans, 1);
        cv.take(d_flags, 32);
        cv.take(d_range, 1);
        bytes = cv.off;
    });
    if (rc_arena) return rc_arena;
    std::vector<unsigned long long> acc(BN_ACC * np);
    unsigned long long orphans = 0;
    int rounds = 0;
    double fix_mul = 0.0;
    auto run = [&]() -> int {
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemsetAsync(a.acc, 0, (size_t)((char *)(d_range + 1) - (char *)a.acc), st));
        if (int rc = box_fix_mul(m, pa.nc, pa.nr, uc, ur, us, d_range, &fix_mul)) return rc;
        HIP_TRY(ctx, h2d_one(ctx, d_peak_box, peak_box.data(), 4 * np));
        a.dens = m->dens;
        a.uc = uc; a.ur = ur; a.us = us; a.nc = pa.nc; a.nr = pa.nr;
        a.cut = pp.cut; a.sign = pp.sign;
        a.peak_box = d_peak_box; a.n_peaks = (int64_t)np;
        a.fix_mul = fix_mul;
        const dim3 tiles((unsigned)((uc + PK_C - 1) / PK_C), (unsigned)((ur + PK_R - 1) / PK_R), (unsigned)((us + PK_S - 1) / PK_S));
        const dim3 flat(grid_for(nbox, 256, 2048));      // (grid-stride loops: eight workgroups per CU, and a jump round that returns at once costs a small launch)
        { PROF(ctx, "k_basin_parent"); hipLaunchKernelGGL(k_basin_parent, tiles, dim3(PK_THREADS), 0, st, a); }
        HIP_TRY(ctx, hipGetLastError());
        for (;;) {
            if (rounds >= BN_MAX_ROUNDS) return fail(ctx, PDBEDA_ERR_STATE, "peak basins: the ascent did not settle in %d doubling rounds", BN_MAX_ROUNDS);
            const int batch = std::min(BN_BATCH, BN_MAX_ROUNDS - rounds);
            uint32_t changed[BN_BATCH];
            for (int k = 0; k < batch; ++k) {      // (a round behind one that changed nothing returns at once: the rest of a batch costs its launches)
                PROF(ctx, "k_basin_jump");
                hipLaunchKernelGGL(k_basin_jump, flat, dim3(256), 0, st, a.up, nbox, rounds + k > 0 ? d_flags + rounds + k - 1 : (const uint32_t *)nullptr, d_flags + rounds + k);
            }
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, d2h(ctx, changed, d_flags + rounds, 4 * (size_t)batch));
            HIP_TRY(ctx, ctx_sync(ctx));
            int settled = -1;
            for (int k = 0; k < batch && settled < 0; ++k)
                if (changed[k] == 0u) settled = k;
            rounds += settled < 0 ? batch : settled + 1;      // (rounds that ran: up to and with the first that changed nothing)
            if (settled >= 0) break;
        }
        { PROF(ctx, "k_basin_mark"); hipLaunchKernelGGL(k_basin_mark, dim3(grid_for((int64_t)np, 256, 1024)), dim3(256), 0, st, a.up, d_peak_box, (int64_t)np); }
        { PROF(ctx, "k_basin_resolve"); hipLaunchKernelGGL(k_basin_resolve, flat, dim3(256), 0, st, a.up, nbox, a.orphans); }
        { PROF(ctx, "k_basin_sums"); hipLaunchKernelGGL(k_basin_sums, tiles, dim3(PK_THREADS), 0, st, a); }
        if (basin_host) { PROF(ctx, "k_basin_decode"); hipLaunchKernelGGL(k_basin_decode, flat, dim3(256), 0, st, a.up, nbox); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, d2h(ctx, acc.data(), a.acc, 8 * BN_ACC * np));
        HIP_TRY(ctx, d2h(ctx, &orphans, a.orphans, 8));
        if (basin_host) HIP_TRY(ctx, d2h(ctx, basin_host, a.up, 4 * (size_t)nbox));
        HIP_TRY(ctx, ctx_sync(ctx));
        return PDBEDA_OK;
    };
    if (const int rc = run()) {
        (void)ctx_sync(ctx);      // (`peak_box` is freed on return and its copy may be a hipMemcpyAsync out of it: nothing of a failed call may still read it)
        return rc;
    }
    const double fix_inv = 1.0 / fix_mul;      // (a power of two: the products below are exact)
    br.n.resize(np); br.sum.resize(np); br.s1.resize(3 * np); br.sw1.resize(3 * np); br.saddle.resize(np); br.neighbour.resize(np);
    for (size_t i = 0; i < np; ++i) {
        br.n[i] = (int64_t)acc[i];
        br.sum[i] = (double)((long long)acc[np + i] * pp.sign) * fix_inv;
        for (int k = 0; k < 3; ++k) {
            br.s1[3 * i + k] = (int64_t)acc[(2 + k) * np + i];
            const __int128 v = (__int128)(long long)acc[(6 + 2 * k) * np + i] * ((__int128)1 << 32) + (__int128)(long long)acc[(5 + 2 * k) * np + i];
            br.sw1[3 * i + k] = (double)v * fix_inv;
        }
        const unsigned long long key = acc[11 * np + i];
        uint32_t bits = (uint32_t)(key >> 32);
        if (key != 0ull && pp.sign < 0) bits |= 0x80000000u;
        memcpy(&br.saddle[i], &bits, 4);
        br.neighbour[i] = key != 0ull ? (int32_t)(~(uint32_t)(key & 0xffffffffull)) : -1;
    }
    br.counters[0] = pj->tested[p];
    br.counters[1] = (int64_t)orphans;
    br.counters[2] = rounds;
    br.counters[3] = (int64_t)bytes;
    br.done = true;
    return PDBEDA_OK;
}

extern "C" int pdbeda_peaklist_basins(pdbeda_peaklist *pl, int64_t *n, double *sum, int64_t *s1, double *sw1, float *saddle, int32_t *neighbour,
                                      int32_t *basin, int64_t counters[4]) {
    if (!pl || pl->freed) return PDBEDA_ERR_ARGUMENT;
    PeakJob *pj = pl->job;
    if (pj->ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    if (int rc = peaks_resolve(pj)) return rc;
    PeakJob::BasinRows &br = pj->basins[pl->plane];
    if (!br.done || basin)      // (the volume is not kept: a call that asks for it runs the job, and gets the same rows)
        if (int rc = basins_compute(pl, basin)) return rc;
    const size_t np = br.n.size();
    if (n && np) memcpy(n, br.n.data(), 8 * np);
    if (sum && np) memcpy(sum, br.sum.data(), 8 * np);
    if (s1 && np) memcpy(s1, br.s1.data(), 24 * np);
    if (sw1 && np) memcpy(sw1, br.sw1.data(), 24 * np);
    if (saddle && np) memcpy(saddle, br.saddle.data(), 4 * np);
    if (neighbour && np) memcpy(neighbour, br.neighbour.data(), 4 * np);
    if (counters) memcpy(counters, br.counters, sizeof br.counters);
    return PDBEDA_OK;
}

extern "C" int pdbeda_peaklist_free(pdbeda_peaklist *pl) {
    if (!pl) return PDBEDA_ERR_ARGUMENT;
    if (pl->freed) return PDBEDA_ERR_STATE;
    PeakJob *pj = pl->job;
    pl->freed = true;
    pj->ctx->live_handles--;
    if (--pj->refs == 0) delete pj;   // last list of the job: the arena is recycled in stream order, as a blob list's
    delete pl;
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Sphere / list batches
// ------------------------------------------------------------------------------------
struct GroupSetup {
    Arena in_arena;          // inputs + boxes + bounds (scratch: grouped_job releases it behind the painting, any other way out with the setup)
    double *d_xyz = nullptr;
    float *d_radii = nullptr;
    int32_t *d_item_group = nullptr;
    AtomBox *d_boxes = nullptr;
    int32_t *d_crs = nullptr;
    int32_t *g_lo = nullptr, *g_hi = nullptr;
    VolDesc *d_vols = nullptr;
    Counters *d_ctr = nullptr;
    int64_t total_words = 0, total_keys = 0;
    bool host_totals = false;   // the totals are the host's (per-atom spheres): nobody waited for the device's -- k_make_vols checks them
    std::vector<AtomBox> host_boxes;   // per-atom spheres: the boxes the host made (kept on the list: aggregateCloud's union volumes are boxes around them)
    int64_t largest_box = 0;    // a batch the host planned: voxels of its largest volume
    bool atom_engine = false;   // per-atom spheres whose boxes the host made, every box one mask word a row and at most ATOM_WORDS rows: ONE launch labels the batch (k_atom_engine)
    // staged inputs whose copy into the device scratch has not been launched yet: grouped_job's k_job_init does it (one launch less), flush_pending for everybody else
    PendingCopy pend;
};

static hipError_t flush_pending(pdbeda_ctx *ctx, GroupSetup *gs) {
    const PendingCopy p = gs->pend.take();
    return p.bytes ? copy_by_kernel(ctx, p.dst, p.src, p.bytes) : hipSuccess;
}

static int expand_groups(const int64_t *group_offsets, int64_t n_groups, int64_t n_items, std::vector<int32_t> &item_group) {
    item_group.assign((size_t)n_items, 0);
    if (group_offsets[0] != 0 || group_offsets[n_groups] != n_items) return -1;
    for (int64_t g = 0; g < n_groups; ++g) {
        if (group_offsets[g + 1] < group_offsets[g]) return -1;
        for (int64_t i = group_offsets[g]; i < group_offsets[g + 1]; ++i) item_group[(size_t)i] = (int32_t)g;
    }
    return 0;
}

// Scratch of a sphere / list batch: inputs, boxes, group bounds, volume descriptors.
static int group_alloc(pdbeda_ctx *ctx, int64_t n_items, int64_t n_groups, GroupSetup *gs) {
    if (n_groups >= (1ll << 31) || n_items >= (1ll << 40)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "batch too large");
    const int64_t ni = std::max<int64_t>(n_items, 1), ng = std::max<int64_t>(n_groups, 1);
    return arena_carve(ctx, "sphere / list batch", &gs->in_arena, [&](Carver &cv) {
        cv.take(gs->d_xyz, 3 * ni);
        cv.take(gs->d_radii, ni);
        cv.take(gs->d_item_group, ni);
        cv.take(gs->d_boxes, ni);
        cv.take(gs->d_vols, ng);       // (boxes, volumes and counters follow the inputs: a per-atom sphere batch whose bounds the host makes sends all six in one row)
        cv.take(gs->d_ctr, 1);
        cv.take(gs->d_crs, 3 * ni);
        cv.take(gs->g_lo, 3 * ng);
        cv.take(gs->g_hi, 3 * ng);
    });
}

// Every path that sizes a sphere / list batch ends here -- the device's totals after their round trip, the host's without one: the totals onto the
// setup, and the one limit on them.
static int group_sized(pdbeda_ctx *ctx, GroupSetup *gs, int64_t words, int64_t keys, bool by_host) {
    gs->total_words = words;
    gs->total_keys = keys;
    gs->host_totals = by_host;
    if (words >= (1ll << 31) * 2) return fail(ctx, PDBEDA_ERR_ARGUMENT, "sphere batch too large (%lld mask words)", (long long)words);
    return 0;
}

// Inputs are on the device (d_xyz + d_radii, or d_crs; d_item_group): group bounding volumes, volume descriptors, and the
// totals read back (the one host round trip of a sphere / list batch).
static int group_bounds(pdbeda_map *m, GroupSetup *gs, int64_t n_items, int64_t n_groups, bool spheres, const int64_t *host_totals = nullptr) {
    pdbeda_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const int64_t ng = std::max<int64_t>(n_groups, 1);
    { PROF(ctx, "k_init_bounds"); hipLaunchKernelGGL(k_init_bounds, dim3(grid_for(3 * ng, 256)), dim3(256), 0, st, gs->g_lo, gs->g_hi, 3 * ng, gs->d_ctr); }
    if (n_items > 0) {
        if (spheres)
            { PROF(ctx, "k_atom_boxes"); hipLaunchKernelGGL(k_atom_boxes, dim3(grid_for(n_items, 256)), dim3(256), 0, st, m->geom_dev, gs->d_xyz, gs->d_radii,
                               gs->d_item_group, n_items, gs->d_boxes, gs->g_lo, gs->g_hi); }
        else
            { PROF(ctx, "k_list_boxes"); hipLaunchKernelGGL(k_list_boxes, dim3(grid_for(n_items, 256 * 4, 256)), dim3(256), 0, st, gs->d_crs, gs->d_item_group, n_items,
                               gs->g_lo, gs->g_hi); }
    }
    { PROF(ctx, "k_make_vols"); hipLaunchKernelGGL(k_make_vols, dim3(1), dim3(1024), 0, st, gs->g_lo, gs->g_hi, (int)n_groups, gs->d_vols, gs->d_ctr,
                                                   host_totals ? (long long)host_totals[0] : LLONG_MAX, host_totals ? (long long)host_totals[1] : LLONG_MAX); }
    HIP_TRY(ctx, hipGetLastError());
    if (host_totals) return group_sized(ctx, gs, host_totals[0], host_totals[1], true);   // sized by the host: no round trip (the kernel holds the device's totals against these)
    Counters ctr;
    HIP_TRY(ctx, d2h(ctx, &ctr, gs->d_ctr, sizeof ctr));
    HIP_TRY(ctx, ctx_sync(ctx));  // (host-side staging vectors of the caller are also safe to drop now)
    return group_sized(ctx, gs, ctr.total_words, ctr.total_keys, false);
}

// A sphere / list batch onto the device, sized.  It validates, chooses ONE of four plans, and ships that plan:
//   the row, left to the job    inputs, boxes, volumes and counters as they sit at the head of the scratch arena (group_alloc), made by the host
//                               (plan_spheres: pdbeda_spherebox.h) in the pinned block; the job's first launch copies the row (pend_*)
//   the row, copied now         the same row without copy kernels, whose launches cannot read host memory
//   inputs only                 coordinates, radii and groups; the device makes boxes and volumes, and nobody waits for its totals: k_make_vols holds
//                               them against the host's, which follow from the radii alone (plan_radii_totals)
//   the device's own sizing     k_init_bounds, k_atom_boxes / k_list_boxes, k_make_vols and the WAIT for their totals: voxel lists, what the range test
//                               or the one limit declines, what finds no room in the block
// Per-atom spheres (a group per atom: the clouds of aggregateCloud, the per-atom region tables) and grouped spheres (a residue's atoms: the residue
// region tables, RSCC / RSR) take the row -- three launches, the copy of the totals and one of an entry's waits less per call, and a launch costs
// several times its 5 us when other processes' uploads hold the link.  PDBEDA_HOST_BOXES=0: the device makes boxes and volumes (A/B, and what the test of
// the paths' equality runs against).  The inputs go through the pinned block, so nothing here needs the caller's arrays after the call returns.
static int group_setup(pdbeda_map *m, const double *xyz, const float *radii, const int32_t *crs, int64_t n_items,
                       const int64_t *group_offsets, int64_t n_groups, GroupSetup *gs) {
    static const bool host_boxes_on = env_unless_0("PDBEDA_HOST_BOXES");
    static const bool atom_engine_on = env_unless_0("PDBEDA_ATOM_ENGINE");   // (A/B switch)
    pdbeda_ctx *ctx = m->ctx;
    const bool spheres = xyz != nullptr;
    // ---- validate ----
    std::vector<int32_t> item_group;
    if (expand_groups(group_offsets, n_groups, n_items, item_group)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "bad group_offsets");
    for (int64_t a = 0; spheres && a < n_items; ++a) {
        if (!std::isfinite(xyz[3 * a]) || !std::isfinite(xyz[3 * a + 1]) || !std::isfinite(xyz[3 * a + 2]) || !std::isfinite(radii[a]))
            return fail(ctx, PDBEDA_ERR_ARGUMENT, "sphere batch: atom %lld has a non-finite coordinate or radius", (long long)a);
    }
    int rc = group_alloc(ctx, n_items, n_groups, gs);
    if (rc) return rc;
    bool per_atom = spheres && n_items > 0 && n_groups == n_items;
    for (int64_t g = 0; g <= n_groups && per_atom; ++g) per_atom = group_offsets[g] == g;
    const bool grouped = spheres && n_items > 0 && n_groups > 0 && n_groups < n_items;
    // (a staged block mirrors the head of the scratch arena, where group_alloc carves the inputs first: a StagedRow over it)
    char *const base = gs->in_arena.base;
    const size_t inputs = (size_t)((char *)(gs->d_item_group + n_items) - base), row = (size_t)((char *)(gs->d_ctr + 1) - base);
    // ---- decide: each plan is sized once, by the planner ----
    enum { ROW_TO_JOB, ROW_NOW, INPUTS_ONLY, DEVICE_SIZED } ship = DEVICE_SIZED;
    StagedRow sr;
    SpherePlan plan;
    const bool row_allowed = (per_atom || (grouped && copy_kernels())) && host_boxes_on && !ctx->debug_shrink_totals && row <= STAGED_ROW_LIMIT;
    if (row_allowed && (sr = StagedRow{pinned_take(ctx, row), base, row}).stage) {      // (boxes and volumes straight into the staged row)
        plan = plan_spheres(m->geom, xyz, radii, per_atom ? nullptr : item_group.data(), n_items, n_groups, sr.twin(gs->d_boxes), sr.twin(gs->d_vols), ATOM_WORDS);
        if (plan.fits) ship = copy_kernels() ? ROW_TO_JOB : ROW_NOW;
        else { pinned_untake(ctx, sr.stage); sr = StagedRow(); }
    }
    if (ship == DEVICE_SIZED && per_atom && plan.plannable) {      // (a coordinate the host may not cast: the device's boxes are its own business, and so are its totals)
        plan = plan_radii_totals(m->geom, radii, n_items, ATOM_WORDS);
        if (plan.fits && (sr = StagedRow{pinned_take(ctx, inputs), base, inputs}).stage) ship = INPUTS_ONLY;
    }
    // ---- ship ----
    if (ship != DEVICE_SIZED) {      // coordinates, radii and groups at their arena offsets
        sr.put(gs->d_xyz, xyz, 24 * (size_t)n_items);
        sr.put(gs->d_radii, radii, 4 * (size_t)n_items);
        sr.put(gs->d_item_group, item_group.data(), 4 * (size_t)n_items);
    }
    if (ship == ROW_TO_JOB || ship == ROW_NOW) {
        Counters *ctr0 = sr.twin(gs->d_ctr);
        memset(ctr0, 0, sizeof *ctr0);
        ctr0->total_words = plan.words;
        ctr0->total_keys = plan.keys;
        gs->largest_box = plan.largest;
        if (per_atom) {
            const AtomBox *boxes = sr.twin(gs->d_boxes);
            gs->host_boxes.assign(boxes, boxes + n_items);
            gs->atom_engine = plan.small_boxes && atom_engine_on && n_items < (1ll << 31);
        }
        if (ship == ROW_NOW) HIP_TRY(ctx, stage_copy(ctx, sr.stage, base, row, true));
        else gs->pend = {sr.stage, base, sr.bytes16()};   // (copied by the job's first launch; whole 16-byte units: the stage and the carve are padded)
        return group_sized(ctx, gs, plan.words, plan.keys, true);
    }
    if (ship == INPUTS_ONLY) {
        const int64_t totals[2] = {plan.words / (ctx->debug_shrink_totals ? 2 : 1), plan.keys / (ctx->debug_shrink_totals ? 2 : 1)};
        HIP_TRY(ctx, stage_copy(ctx, sr.stage, base, inputs, true));      // (a row at the head of the scratch arena: one staged block, one copy)
        return group_bounds(m, gs, n_items, n_groups, true, totals);
    }
    if (n_items > 0) {
        if (spheres) {
            const H2DItem in[3] = {{gs->d_xyz, xyz, (size_t)(24 * n_items)}, {gs->d_radii, radii, (size_t)(4 * n_items)}, {gs->d_item_group, item_group.data(), (size_t)(4 * n_items)}};
            HIP_TRY(ctx, h2d_row(ctx, in, 3));       // (a row at the head of the scratch arena: one copy)
        } else {
            HIP_TRY(ctx, h2d_one(ctx, gs->d_crs, crs, (size_t)(12 * n_items)));
            HIP_TRY(ctx, h2d_one(ctx, gs->d_item_group, item_group.data(), (size_t)(4 * n_items)));
        }
    }
    return group_bounds(m, gs, n_items, n_groups, spheres);   // (synchronises: item_group may go)
}

// Paint the group volumes and enqueue the labelling engine on them; the input scratch is recycled in stream order.
static int grouped_job(pdbeda_map *m, GroupSetup &gs, int64_t n_items, int64_t n_groups, bool spheres, float cutoff, pdbeda_bloblist **out, const PoolPaint *pool = nullptr,
                       bool unordered = false) {
    // (PDBEDA_DEBUG_ATOM_CAPS="runs,comps": tests shrink the LDS tables' use so that small inputs run k_atom_engine's global-table path)
    static const std::pair<int, int> atom_caps = [] {
        int r = ATOM_RUNS, c = ATOM_COMPS;
        if (const char *e = getenv("PDBEDA_DEBUG_ATOM_CAPS")) { int x = 0, y = 0; if (sscanf(e, "%d,%d", &x, &y) == 2) { r = std::max(0, std::min(x, ATOM_RUNS)); c = std::max(0, std::min(y, ATOM_COMPS)); } }
        return std::make_pair(r, c);
    }();
    pdbeda_ctx *ctx = m->ctx;
    const int64_t max_runs = gs.total_keys / 2 + gs.total_words + 1;
    if (gs.pend.bytes && m->fix_mul == 0.0 && !m->fix_refused) {
        // map_fix_mul is about to WAIT (a map whose range is not known yet), and a wait hands the pinned block out afresh: inputs staged there must be on
        // their way before it, not left to k_job_init behind it
        const hipError_t ep = flush_pending(ctx, &gs);
        if (ep != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "grouped blobs: %s", hipGetErrorString(ep));
    }
    int rc_fix = map_fix_mul(m);
    if (rc_fix) return rc_fix;
    std::unique_ptr<LabelJob> lj(new_label_job(ctx, m));
    Job &job = lj->job;
    memset(&job, 0, sizeof job);
    job.fix_mul = m->fix_mul;
    KeyTable kt;
    int rc = arena_carve(ctx, "grouped blobs", &lj->arena, [&](Carver &cv) { kt = job_carve(job, cv, (int)n_groups, gs.total_words, gs.total_keys, max_runs, max_runs, 0, nullptr); });
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    {   // volume descriptors into the job + zeroes over counters, masks, first-key bitmap and both levels of rank counters (adjacent in the arena: job_carve): one launch
        static_assert(sizeof(VolDesc) % 16 == 0, "VolDesc is copied in 16-byte units");
        const size_t zero_bytes = ((size_t)((char *)(job.mid_count + kt.mid_count_elems) - (char *)job.ctr) + 15) & ~(size_t)15;   // (into the carve's own padding)
        const PendingCopy pend = gs.pend.take();      // (the staged inputs, when their copy was left to this launch)
        const size_t vol16 = sizeof(VolDesc) * (size_t)n_groups / 16, in16 = pend.bytes / 16;
        // (volume descriptors that are part of the inputs still to be copied come straight from the staged block)
        const char *vol_src = reinterpret_cast<const char *>(gs.d_vols);
        if (pend.bytes && vol_src >= pend.dst && vol_src < pend.dst + pend.bytes) vol_src = StagedRow{pend.src, pend.dst, pend.bytes}.twin(vol_src);
        hipLaunchKernelGGL(k_job_init, dim3((unsigned)std::min<size_t>((std::max(std::max(zero_bytes / 16, vol16), in16) + 255) / 256, 2048)), dim3(256), 0, st,
                           reinterpret_cast<const uint4 *>(pend.src), reinterpret_cast<uint4 *>(pend.dst), (unsigned long long)in16,
                           reinterpret_cast<const uint4 *>(vol_src), reinterpret_cast<uint4 *>(job.vols), (unsigned long long)vol16,
                           reinterpret_cast<uint4 *>(job.ctr), (unsigned long long)(zero_bytes / 16));
        e = hipGetLastError();
    }
    const bool fused_atoms = spheres && gs.atom_engine && n_items > 0 && n_items == n_groups;
    if (e == hipSuccess && fused_atoms) {   // a per-atom batch of small boxes: paint, run index, unions, resolve and key painting in one launch
        PROF(ctx, "k_atom_engine");
        hipLaunchKernelGGL(k_atom_engine, dim3((unsigned)n_items), dim3(256), 0, st, job, m->geom_dev, m->dens, gs.d_xyz, gs.d_radii, gs.d_boxes, cutoff, atom_caps.first, atom_caps.second);
        e = hipGetLastError();
    } else if (e == hipSuccess && n_items > 0) {
        if (spheres)
            { PROF(ctx, "k_sphere_paint"); hipLaunchKernelGGL(k_sphere_paint, dim3((unsigned)n_items), dim3(256), 0, st, m->geom_dev, m->dens, gs.d_xyz, gs.d_radii,
                               gs.d_item_group, gs.d_boxes, job.vols, job.mask, cutoff, gs.d_ctr, job.ctr); }
        else if (pool)      // (aggregateCloud's union job: the pooled voxels painted straight from the clouds' lists, the bonded pairs tested by the same launch)
            { PoolPaint pp = *pool; pp.ctr = job.ctr; PROF(ctx, "k_pool_paint"); hipLaunchKernelGGL(k_pool_paint, dim3(pp.paint_blocks + (unsigned)pp.n_pairs), dim3(256), 0, st, pp, job.vols, job.mask); }
        else
            { PROF(ctx, "k_list_paint"); hipLaunchKernelGGL(k_list_paint, dim3(grid_for(n_items, 256)), dim3(256), 0, st, gs.d_crs, gs.d_item_group, n_items, job.vols, job.mask); }
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = engine_enqueue(ctx, m, job, max_runs, fused_atoms, unordered);
    // The inputs go back NOW, not with the caller's setup: the paint kernel has consumed them (whoever gets their arena next is enqueued behind it on
    // this stream), and the union job of the same pdbeda_aggregate_cloud call takes this very block for its own inputs
    gs.in_arena.put();
    if (e != hipSuccess || rc) return rc ? rc : fail(ctx, PDBEDA_ERR_DEVICE, "grouped blobs: %s", hipGetErrorString(e));
    lj->host_boxes.swap(gs.host_boxes);
    *out = job_view(lj.release(), 0, 0, (int)n_groups, 1);      // (one list over all the volumes)
    return PDBEDA_OK;
}

static int grouped_blobs(pdbeda_map *m, const double *xyz, const float *radii, const int32_t *crs, int64_t n_items,
                         const int64_t *group_offsets, int64_t n_groups, float cutoff, pdbeda_bloblist **out) {
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GroupSetup gs;
    int rc = group_setup(m, xyz, radii, crs, n_items, group_offsets, n_groups, &gs);
    if (rc) return rc;
    return grouped_job(m, gs, n_items, n_groups, xyz != nullptr, cutoff, out);
}

extern "C" int pdbeda_sphere_blobs(pdbeda_map *m, const double *xyz, const float *radii, int64_t n_atoms, const int64_t *group_offsets,
                                   int64_t n_groups, float density_cutoff, pdbeda_bloblist **out) {
    if (!m || !out || n_atoms < 0 || n_groups < 0 || !group_offsets || (n_atoms > 0 && (!xyz || !radii))) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    return grouped_blobs(m, xyz, radii, nullptr, n_atoms, group_offsets, n_groups, density_cutoff, out);
}

extern "C" int pdbeda_list_blobs(pdbeda_map *m, const int32_t *crs, int64_t n, const int64_t *group_offsets, int64_t n_groups,
                                 pdbeda_bloblist **out) {
    if (!m || !out || n < 0 || n_groups < 0 || !group_offsets || (n > 0 && !crs)) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    return grouped_blobs(m, nullptr, nullptr, crs, n, group_offsets, n_groups, 0.0f, out);
}

extern "C" int pdbeda_region_sums(pdbeda_map *m, const double *xyz, const float *radii, int64_t n_atoms, const int64_t *group_offsets,
                                  int64_t n_groups, float cutoff, double *pos, double *neg, int64_t *n_region, uint8_t *valid) {
    if (!m || n_atoms < 0 || n_groups < 0 || !group_offsets || (n_atoms > 0 && (!xyz || !radii))) return PDBEDA_ERR_ARGUMENT;
    static const bool atom_region_on = env_unless_0("PDBEDA_ATOM_REGION");      // (A/B switch)
    pdbeda_ctx *ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_groups == 0) return PDBEDA_OK;
    GroupSetup gs;
    int rc = group_setup(m, xyz, radii, nullptr, n_atoms, group_offsets, n_groups, &gs);
    if (rc) return rc;
    std::vector<unsigned long long> h_cnt(n_groups);
    std::vector<unsigned int> h_inv(n_groups);
    auto deliver_counts = [&] {      // (both paths end here, behind their wait)
        for (int64_t g = 0; g < n_groups; ++g) {
            if (n_region) n_region[g] = (int64_t)h_cnt[g];
            if (valid) valid[g] = h_inv[g] ? 0 : 1;
        }
        return PDBEDA_OK;
    };
    {   // a group per atom whose inputs the host staged (coordinates, radii, host-made volumes in the pinned block): ONE launch, no mask (k_atom_region).
        // The kernel counts a box's voxels in 32 bits and does not ask for small boxes, so the gate does: the plan's largest box has fewer than 2^31.
        const size_t out_bytes = 3 * pinned_span(8 * (size_t)n_groups) + pinned_span(4 * (size_t)n_groups);
        if (atom_region_on && n_groups == n_atoms && gs.pend.bytes && !gs.host_boxes.empty() && gs.largest_box < (1ll << 31) && copy_kernels() && out_bytes <= pinned_room(ctx)) {
            // (n_groups > 0: no take is empty.  As before a failed launch below keeps the takes until the next wait and, through fail(), delivers nothing)
            double *o_pos = reinterpret_cast<double *>(pinned_take(ctx, 8 * (size_t)n_groups, pos));
            double *o_neg = reinterpret_cast<double *>(pinned_take(ctx, 8 * (size_t)n_groups, neg));
            unsigned long long *o_cnt = reinterpret_cast<unsigned long long *>(pinned_take(ctx, 8 * (size_t)n_groups, h_cnt.data()));
            unsigned int *o_inv = reinterpret_cast<unsigned int *>(pinned_take(ctx, 4 * (size_t)n_groups, h_inv.data()));
            // (the kernel reads the staged row where it lies: its copy into the scratch arena is never launched)
            const PendingCopy pend = gs.pend.take();
            const StagedRow sr{pend.src, pend.dst, pend.bytes};
            { PROF(ctx, "k_atom_region"); hipLaunchKernelGGL(k_atom_region, dim3((unsigned)std::min<int64_t>(n_groups, 65536)), dim3(256), 0, ctx->stream, m->geom_dev, m->dens, sr.twin(gs.d_xyz), sr.twin(gs.d_radii),
                                                            sr.twin(gs.d_vols), (int)n_groups, cutoff, o_pos, o_neg, o_cnt, o_inv); }
            hipError_t e1 = hipGetLastError();
            if (e1 == hipSuccess) e1 = ctx_sync(ctx);
            if (e1 != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "region sums: %s", hipGetErrorString(e1));
            return deliver_counts();
        }
    }
    const int64_t tw = std::max<int64_t>(gs.total_words, 1);
    Arena a;
    uint64_t *mask = nullptr;
    double *d_pos = nullptr, *d_neg = nullptr;
    unsigned long long *d_cnt = nullptr;
    unsigned int *d_inv = nullptr;
    size_t zero_bytes = 0;
    rc = arena_carve(ctx, "region sums", &a, [&](Carver &cv) {
        cv.take(mask, tw);
        cv.take(d_pos, n_groups);
        cv.take(d_neg, n_groups);
        cv.take(d_cnt, n_groups);
        cv.take(d_inv, n_groups);
        zero_bytes = cv.off;      // (all of it)
    });
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    hipError_t e;
    {   // the staged inputs into the scratch (when group_setup left their copy to us) and zeroes over masks and sums: one launch
        const PendingCopy pend = gs.pend.take();
        const size_t in16 = pend.bytes / 16, zero16 = zero_bytes / 16;
        hipLaunchKernelGGL(k_job_init, dim3((unsigned)std::min<size_t>((std::max(zero16, in16) + 255) / 256, 2048)), dim3(256), 0, st,
                           reinterpret_cast<const uint4 *>(pend.src), reinterpret_cast<uint4 *>(pend.dst), (unsigned long long)in16,
                           (const uint4 *)nullptr, (uint4 *)nullptr, 0ull, reinterpret_cast<uint4 *>(a.base), (unsigned long long)zero16);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_atoms > 0) {
        { PROF(ctx, "k_sphere_paint"); hipLaunchKernelGGL(k_sphere_paint, dim3((unsigned)n_atoms), dim3(256), 0, st, m->geom_dev, m->dens, gs.d_xyz, gs.d_radii,
                           gs.d_item_group, gs.d_boxes, gs.d_vols, mask, 0.0f, gs.d_ctr, (Counters *)nullptr); }
        { PROF(ctx, "k_region_reduce"); hipLaunchKernelGGL(k_region_reduce, dim3((unsigned)std::min<int64_t>(n_groups, 65536)), dim3(256), 0, st, m->geom_dev, m->dens, gs.d_vols,
                           (int)n_groups, mask, gs.total_words, cutoff, d_pos, d_neg, d_cnt, d_inv); }
        e = hipGetLastError();
    }
    Counters setup;
    memset(&setup, 0, sizeof setup);
    if (e == hipSuccess) {
        const D2HItem parts[5] = {{pos, d_pos, (size_t)(8 * n_groups)}, {neg, d_neg, (size_t)(8 * n_groups)}, {h_cnt.data(), d_cnt, (size_t)(8 * n_groups)},
                                  {h_inv.data(), d_inv, (size_t)(4 * n_groups)}, {gs.host_totals ? &setup : nullptr, gs.d_ctr, sizeof setup}};
        e = d2h_many(ctx, parts, 5);
    }
    if (e == hipSuccess) e = ctx_sync(ctx);
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "region sums: %s", hipGetErrorString(e));
    if (setup.overflow != 0u) return fail(ctx, PDBEDA_ERR_DEVICE, "region sums: the device's volumes outgrew what the host sized the batch for");
    return deliver_counts();
}

// ------------------------------------------------------------------------------------
// Radial profiles (no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// One launch per chunk of atoms, and a chunk is every atom whenever the pinned block holds the batch (48 bytes of inputs and 32 n_shells + 1 of
// results an atom: 2 000 atoms x 20 shells are 1.4 MB of its 4 MiB).  The host makes the boxes -- the library's one sphere-box rule, as for the
// per-atom region sums -- and refuses what the contract refuses before anything is launched; the kernel reads coordinates and boxes where the host
// staged them and writes the rows straight into the block (pinned_take: delivered by the wait).  Without copy kernels, or without a block, the same
// launch runs on device scratch and the runtime copies.
extern "C" int pdbeda_radial_profiles(pdbeda_map *m, const double *xyz, int64_t n_atoms, float radius, int32_t n_shells, float cutoff,
                                      int64_t *n, double *sum, int64_t *n_sig, double *sum_sig, uint8_t *valid) {
    if (!m || n_atoms < 0 || (n_atoms > 0 && !xyz)) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    if (n_shells < 1 || n_shells > PDBEDA_MAX_SHELLS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: n_shells %d outside [1, %d]", (int)n_shells, PDBEDA_MAX_SHELLS);
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: the radius must be finite and > 0");
    if (std::isnan(cutoff)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: the cutoff is NaN");
    if (n_atoms == 0) return PDBEDA_OK;
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    if (n_atoms >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: batch too large");
    std::vector<AtomBox> boxes((size_t)n_atoms);
    int64_t largest = 0;
    {
        // (the planner's range test and box function.  There is no device sizing to fall back on here: what the host may not cast is refused)
        int32_t R[3];
        if (!plan_half_widths(m->geom, radius, R)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: the radius is 2^29 grid steps or more");
        for (int64_t a = 0; a < n_atoms; ++a) {
            const double *p = xyz + 3 * a;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: atom %lld has a non-finite coordinate", (long long)a);
            if (!plan_atom_box(m->geom, p, R, &boxes[(size_t)a])) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: atom %lld lies 2^29 grid steps or more from the map's origin", (long long)a);
            SpherePlan one;      // (the box as a plan of its own: what does not fit the planner's limit has 2^32 voxels or more -- every width of a box is even)
            one.push(boxes[(size_t)a].lo, boxes[(size_t)a].hi, 0);
            if (!one.fits || one.largest >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "radial profiles: the sphere box of atom %lld has 2^31 voxels or more", (long long)a);
            largest = std::max(largest, one.largest);
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc_fix = map_fix_mul(m);      // (a wait when the map's range is not known yet: before anything is staged)
    if (rc_fix) return rc_fix;
    const double fix_mul = coarsened_for(m->fix_mul, largest);      // (a shell's sum inside 64 bits: the quantum's rule in pdbeda_jobplan.h)
    const double fix_inv = 1.0 / fix_mul;      // (powers of two: exact)
    const size_t cells = (size_t)n_shells, per_atom = 48 + 32 * cells + 1, slack = 7 * 64;
    const bool direct = copy_kernels() && ctx->pinned.base && pinned_room(ctx) >= per_atom + slack;
    const int64_t chunk = std::max<int64_t>(1, direct ? (int64_t)((pinned_room(ctx) - slack) / per_atom) : (int64_t)(((size_t)8 << 20) / per_atom));
    Arena scratch;
    for (int64_t a0 = 0; a0 < n_atoms; a0 += chunk) {
        const size_t na = (size_t)std::min<int64_t>(chunk, n_atoms - a0), rows = na * cells;
        const double *k_xyz;
        const AtomBox *k_box;
        long long *k_n, *k_nsig;
        double *k_sum, *k_sumsig;
        uint8_t *k_valid;
        const char *first = nullptr;
        hipError_t e = hipSuccess;
        if (direct) {      // (the chunk was sized to fit: no take fails)
            k_xyz = pinned_in(ctx, xyz + 3 * a0, 3 * na);
            k_box = pinned_in(ctx, &boxes[(size_t)a0], na);
            first = reinterpret_cast<const char *>(k_xyz);
            k_n = reinterpret_cast<long long *>(pinned_take(ctx, 8 * rows, n ? n + (size_t)a0 * cells : nullptr));
            k_sum = reinterpret_cast<double *>(pinned_take(ctx, 8 * rows, sum ? sum + (size_t)a0 * cells : nullptr));
            k_nsig = reinterpret_cast<long long *>(pinned_take(ctx, 8 * rows, n_sig ? n_sig + (size_t)a0 * cells : nullptr));
            k_sumsig = reinterpret_cast<double *>(pinned_take(ctx, 8 * rows, sum_sig ? sum_sig + (size_t)a0 * cells : nullptr));
            k_valid = reinterpret_cast<uint8_t *>(pinned_take(ctx, na, valid ? valid + a0 : nullptr));
        } else {
            double *d_xyz = nullptr;
            AtomBox *d_box = nullptr;
            auto carve = [&](Carver &cv, size_t atoms) {      // (sized once for the largest chunk, laid out for each chunk's own count)
                cv.take(d_xyz, 3 * atoms);
                cv.take(d_box, atoms);
                cv.take(k_n, atoms * cells); cv.take(k_sum, atoms * cells); cv.take(k_nsig, atoms * cells); cv.take(k_sumsig, atoms * cells);
                cv.take(k_valid, atoms);
            };
            if (!scratch.base) {
                const size_t nc = (size_t)std::min<int64_t>(chunk, n_atoms);
                const int rc = arena_carve(ctx, "radial profiles", &scratch, [&](Carver &cv) { carve(cv, nc); });
                if (rc) return rc;
            }
            Carver cv(scratch.base);
            carve(cv, na);
            k_xyz = d_xyz;
            k_box = d_box;
            const H2DItem in[2] = {{d_xyz, xyz + 3 * a0, 24 * na}, {d_box, &boxes[(size_t)a0], sizeof(AtomBox) * na}};
            e = h2d_row(ctx, in, 2, STAGED_ROW_LIMIT);
        }
        if (e == hipSuccess) {
            PROF(ctx, "k_atom_shells");
            const dim3 grid((unsigned)std::min<size_t>(na, 65536)), block(256);
            hipLaunchKernelGGL(k_atom_shells, grid, block, 0, ctx->stream, m->geom_dev, m->dens, k_xyz, k_box, (int)na, radius, (int)n_shells, cutoff, fix_mul, fix_inv, k_n, k_sum, k_nsig, k_sumsig, k_valid);
            e = hipGetLastError();
            if (e != hipSuccess && first) pinned_untake(ctx, first);      // (nothing was queued that reads or writes the takes: the block and the deliveries are as before)
        }
        if (e == hipSuccess && !direct) {
            const D2HItem parts[5] = {{n ? n + (size_t)a0 * cells : nullptr, k_n, 8 * rows}, {sum ? sum + (size_t)a0 * cells : nullptr, k_sum, 8 * rows},
                                      {n_sig ? n_sig + (size_t)a0 * cells : nullptr, k_nsig, 8 * rows}, {sum_sig ? sum_sig + (size_t)a0 * cells : nullptr, k_sumsig, 8 * rows},
                                      {valid ? valid + a0 : nullptr, k_valid, na}};
            e = d2h_each(ctx, parts, 5);
        }
        if (e == hipSuccess) e = ctx_sync(ctx);      // (delivers the chunk's rows and rewinds the block for the next chunk)
        if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "radial profiles: %s", hipGetErrorString(e));
    }
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Voxel-set adjacency, symmetry atoms, nearest atom
// ------------------------------------------------------------------------------------
extern "C" int pdbeda_test_overlap(pdbeda_ctx *ctx, const int32_t *crs, const int64_t *set_offsets, int64_t n_sets, const int32_t *a_idx,
                                   const int32_t *b_idx, int64_t n_pairs, uint8_t *out) {
    if (!ctx || n_sets < 0 || n_pairs < 0 || !set_offsets || (n_pairs > 0 && (!a_idx || !b_idx || !out))) return PDBEDA_ERR_ARGUMENT;
    if (n_pairs == 0) return PDBEDA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nv = set_offsets[n_sets];
    for (int64_t p = 0; p < n_pairs; ++p)
        if (a_idx[p] < 0 || a_idx[p] >= n_sets || b_idx[p] < 0 || b_idx[p] >= n_sets) return fail(ctx, PDBEDA_ERR_ARGUMENT, "pair index out of range");
    std::vector<unsigned int> h_out(n_pairs);
    int32_t *d_crs = nullptr, *d_a = nullptr, *d_b = nullptr;
    int64_t *d_off = nullptr;
    unsigned int *d_out = nullptr;
    int rc = with_scratch(ctx, "test overlap", [&](Carver &cv) {
        cv.take(d_crs, 3 * std::max<int64_t>(nv, 1));
        cv.take(d_off, n_sets + 1);
        cv.take(d_a, n_pairs);
        cv.take(d_b, n_pairs);
        cv.take(d_out, n_pairs);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        if (nv > 0) HIP_TRY(ctx, h2d_one(ctx, d_crs, crs, (size_t)(12 * nv)));
        {
            const H2DItem in[3] = {{d_off, set_offsets, (size_t)(8 * (n_sets + 1))}, {d_a, a_idx, (size_t)(4 * n_pairs)}, {d_b, b_idx, (size_t)(4 * n_pairs)}};
            HIP_TRY(ctx, h2d_row(ctx, in, 3));      // (consecutive takes: one copy)
        }
        HIP_TRY(ctx, hipMemsetAsync(d_out, 0, 4 * n_pairs, st));
        hipLaunchKernelGGL(k_test_overlap, dim3((unsigned)n_pairs), dim3(256), 0, st, d_crs, d_off, d_a, d_b, d_out);
        HIP_TRY(ctx, d2h(ctx, h_out.data(), d_out, 4 * n_pairs));
        return 0;
    });
    if (rc) return rc;
    for (int64_t p = 0; p < n_pairs; ++p) out[p] = h_out[p] ? 1 : 0;
    return PDBEDA_OK;
}

extern "C" int pdbeda_symmetry_atoms(pdbeda_ctx *ctx, const double *xyz, int64_t n_atoms, const double *rot, int32_t n_ops,
                                     const double ortho[9], const double bbox_lo[3], const double bbox_hi[3], int32_t *atom_index,
                                     int32_t *symmetry, double *out_xyz, int64_t cap, int64_t *n_out) {
    if (!ctx || n_atoms < 0 || n_ops < 0 || (n_ops > 0 && !rot) || !ortho || !bbox_lo || !bbox_hi || !n_out || (n_atoms > 0 && !xyz)) return PDBEDA_ERR_ARGUMENT;
    *n_out = 0;
    // no operators (a file without REMARK 290): the reference's loop over them runs zero times and builds an empty list
    // (densityAnalysis.py:896-912) -- not an error
    if (n_atoms == 0 || n_ops == 0) return PDBEDA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t total = 27ll * n_ops * n_atoms, n_words = (total + 63) / 64;
    std::vector<unsigned long long> h_keep((size_t)n_words);
    std::vector<int64_t> picked;
    std::vector<double> h_xyz;
    double *d_xyz = nullptr, *d_rot = nullptr, *d_ortho = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_out = nullptr;
    unsigned long long *d_keep = nullptr;
    int64_t *d_picked = nullptr;
    int rc = with_scratch(ctx, "symmetry atoms", [&](Carver &cv) {
        cv.take(d_xyz, 3 * n_atoms);
        cv.take(d_rot, 12 * n_ops);
        cv.take(d_ortho, 9);
        cv.take(d_lo, 3);
        cv.take(d_hi, 3);
        cv.take(d_keep, n_words);
        cv.take(d_picked, total);
        cv.take(d_out, 3 * total);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        {
            const H2DItem in[5] = {{d_xyz, xyz, (size_t)(24 * n_atoms)}, {d_rot, rot, (size_t)(96 * n_ops)}, {d_ortho, ortho, 72}, {d_lo, bbox_lo, 24}, {d_hi, bbox_hi, 24}};
            HIP_TRY(ctx, h2d_row(ctx, in, 5));      // (one copy: the five sit in a row)
        }
        Result<unsigned long long> keep{h_keep.data(), (size_t)n_words, d_keep};
        { PROF(ctx, "k_symmetry_keep"); hipLaunchKernelGGL(k_symmetry_keep, dim3(grid_for(total, 256)), dim3(256), 0, st, d_xyz, n_atoms, d_rot, (int)n_ops, d_ortho, d_lo, d_hi, keep.at(ctx)); }
        HIP_TRY(ctx, keep.finish(ctx));
        HIP_TRY(ctx, ctx_sync(ctx));
        for (int64_t w = 0; w < n_words; ++w)
            for (unsigned long long bits = h_keep[(size_t)w]; bits; bits &= bits - 1) picked.push_back(64 * w + __builtin_ctzll(bits));
        const int64_t n = (int64_t)picked.size();
        if (n == 0 || n > cap || !out_xyz) return 0;
        h_xyz.resize(3 * (size_t)n);
        Input<int64_t> in_picked{picked.data(), (size_t)n, d_picked};      // (a survivor's number is read by its own thread, once)
        Result<double> out{h_xyz.data(), 3 * (size_t)n, d_out};
        HIP_TRY(ctx, in_picked.send(ctx));
        { PROF(ctx, "k_symmetry_pick"); hipLaunchKernelGGL(k_symmetry_pick, dim3(grid_for(n, 256)), dim3(256), 0, st, d_xyz, n_atoms, d_rot, (int)n_ops, d_ortho, d_lo, d_hi, in_picked.at, n, out.at(ctx)); }
        HIP_TRY(ctx, out.finish(ctx));
        return 0;
    });
    if (rc) return rc;
    const int64_t n = (int64_t)picked.size();
    *n_out = n;
    if (n > cap && (atom_index || symmetry || out_xyz)) return fail(ctx, PDBEDA_ERR_CAPACITY, "need capacity %lld", (long long)n);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t t = picked[(size_t)k], a = t % n_atoms, cell_op = t / n_atoms;
        const int op = (int)(cell_op % n_ops), cell = (int)(cell_op / n_ops);
        if (atom_index) atom_index[k] = (int32_t)a;
        if (symmetry) { symmetry[4 * k] = cell / 9 - 1; symmetry[4 * k + 1] = (cell / 3) % 3 - 1; symmetry[4 * k + 2] = cell % 3 - 1; symmetry[4 * k + 3] = op; }
    }
    if (out_xyz && n > 0) memcpy(out_xyz, h_xyz.data(), 24 * (size_t)n);
    return PDBEDA_OK;
}

extern "C" int pdbeda_nearest_atom(pdbeda_ctx *ctx, const double *centroids, int64_t n_centroids, const double *atom_xyz, int64_t n_atoms,
                                   int64_t *index, double *distance) {
    if (!ctx || n_centroids < 0 || n_atoms <= 0 || !atom_xyz || (n_centroids > 0 && (!centroids || !index || !distance))) return PDBEDA_ERR_ARGUMENT;
    if (n_centroids == 0) return PDBEDA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *d_c = nullptr, *d_a = nullptr, *d_d = nullptr;
    int64_t *d_i = nullptr;
    return with_scratch(ctx, "nearest atom", [&](Carver &cv) {
        cv.take(d_c, 3 * n_centroids);
        cv.take(d_a, 3 * n_atoms);
        cv.take(d_i, n_centroids);
        cv.take(d_d, n_centroids);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        {
            const H2DItem in[2] = {{d_c, centroids, (size_t)(24 * n_centroids)}, {d_a, atom_xyz, (size_t)(24 * n_atoms)}};
            HIP_TRY(ctx, h2d_row(ctx, in, 2));
        }
        int64_t *r_i = pinned_out(ctx, index, (size_t)n_centroids);
        double *r_d = pinned_out(ctx, distance, (size_t)n_centroids);
        hipLaunchKernelGGL(k_nearest_atom, dim3((unsigned)n_centroids), dim3(256), 0, st, d_c, d_a, n_atoms, r_i ? r_i : d_i, r_d ? r_d : d_d);
        if (!r_i) HIP_TRY(ctx, d2h(ctx, index, d_i, 8 * n_centroids));
        if (!r_d) HIP_TRY(ctx, d2h(ctx, distance, d_d, 8 * n_centroids));
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// Crystal contacts (crystalContacts.py): cell grids, symmetry images, minimum distances
// ------------------------------------------------------------------------------------
// How large a staged input may be so that `results` bytes of pinned_out results still fit in the pinned block behind it (a result without
// room there costs a wait of its own).
static size_t pinned_room_beside(const pdbeda_ctx *ctx, size_t results) {
    const size_t reserve = results + (size_t)(4 << 10);
    return pinned_room(ctx) > reserve ? pinned_room(ctx) - reserve : 0;
}

static bool all_finite(const double *v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// The device side of one cell grid (the host plans it: pdbeda_cellgrid.h): the arrays of its counting sort in a carve, and the sort itself.  The counts are
// carved apart from the rest where a call zeroes them with zeros that ride in its one input copy, in a row with those inputs.  sorted_index: when kept.
struct GridBuild {
    unsigned *count = nullptr, *cursor = nullptr, *start = nullptr;
    double *sorted = nullptr;
    int *sorted_index = nullptr;
    void carve_counts(Carver &cv, int64_t cells) { cv.take(count, cells); }
    void carve_rest(Carver &cv, int64_t cells, int64_t n_points, bool indexed) {
        cv.take(cursor, cells); cv.take(start, cells + 1); cv.take(sorted, 3 * n_points);
        if (indexed) cv.take(sorted_index, n_points);
    }
    void carve(Carver &cv, int64_t cells, int64_t n_points, bool indexed) { carve_counts(cv, cells); carve_rest(cv, cells, n_points, indexed); }
    void scan(pdbeda_ctx *ctx, const CellGrid &g, unsigned *total_out) const {      // (the total also into the pinned block when given)
        PROF(ctx, "k_grid_scan");
        hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(1024), 0, ctx->stream, count, g.n_cells, start, cursor, total_out);
    }
    void sort_points(pdbeda_ctx *ctx, const CellGrid &g, const double *d_xyz, int64_t n) const {
        hipStream_t st = ctx->stream;
        { PROF(ctx, "k_grid_count_points"); hipLaunchKernelGGL(k_grid_count_points, dim3(grid_for(n, 256)), dim3(256), 0, st, d_xyz, n, g, count); }
        scan(ctx, g, nullptr);
        if (sorted_index) { PROF(ctx, "k_grid_scatter_indexed"); hipLaunchKernelGGL(k_grid_scatter_indexed, dim3(grid_for(n, 256)), dim3(256), 0, st, d_xyz, n, g, cursor, sorted, sorted_index, n); }
        else { PROF(ctx, "k_grid_scatter_points"); hipLaunchKernelGGL(k_grid_scatter_points, dim3(grid_for(n, 256)), dim3(256), 0, st, d_xyz, n, g, cursor, sorted, n); }
    }
};

// The contacts entry points accept any finite coordinate, so the extent of a point set may overflow fp64: such a box has no grid (make_cell_grid).
static int refuse_extent(pdbeda_ctx *ctx, const char *set, const double lo[3], const double hi[3]) {
    const int q = std::max(bad_extent(lo, hi), 0);
    return fail(ctx, PDBEDA_ERR_ARGUMENT, "the extent of the %s along %c, %g .. %g, overflows fp64: no cell grid can be laid over it", set, "xyz"[q], lo[q], hi[q]);
}
static int contacts_query_grid(pdbeda_ctx *ctx, const double *q_xyz, int64_t n_q, double cutoff, int64_t n_points, CellGrid *out) {
    double lo[3], hi[3];
    return query_grid(q_xyz, n_q, cutoff, n_points, out, lo, hi) ? PDBEDA_OK : refuse_extent(ctx, "query points (grown by twice the cutoff)", lo, hi);
}

static int check_images(pdbeda_ctx *ctx, const double *rot, int32_t n_ops, const double *ortho, const int32_t *cand, int64_t n_cand) {
    if (n_cand == 0) return PDBEDA_OK;
    if (!cand || !rot || !ortho || n_ops < 1) return fail(ctx, PDBEDA_ERR_ARGUMENT, "images need operators, a cell and a candidate list");
    if (!all_finite(rot, 12 * (int64_t)n_ops) || !all_finite(ortho, 9)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "non-finite operator or cell");
    for (int64_t c = 0; c < n_cand; ++c) {
        const int32_t *k = cand + 4 * c;
        if (k[0] < 0 || k[0] >= n_ops) return fail(ctx, PDBEDA_ERR_ARGUMENT, "candidate %lld: operator %d out of range", (long long)c, k[0]);
        for (int q = 1; q < 4; ++q)
            if (k[q] < -(1 << 20) || k[q] > (1 << 20)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "candidate %lld: cell shift out of range", (long long)c);
        if (k[0] == 0 && k[1] == 0 && k[2] == 0 && k[3] == 0)
            return fail(ctx, PDBEDA_ERR_ARGUMENT, "candidate %lld is (op 0, n = 0): the asymmetric unit, not an image", (long long)c);
    }
    return PDBEDA_OK;
}

static int check_contacts_args(pdbeda_ctx *ctx, const double *q_xyz, int64_t n_q, const double *p_xyz, int64_t n_p, double cutoff,
                               const int64_t *out_index, const double *out_distance, int64_t cap) {
    if ((n_q > 0 && !q_xyz) || (n_p > 0 && !p_xyz) || (cap > 0 && (!out_index || !out_distance))) return fail(ctx, PDBEDA_ERR_ARGUMENT, "null array");
    if (!std::isfinite(cutoff) || !(cutoff > 0.0)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "cutoff must be finite and > 0");
    if (n_q >= (1ll << 31) || n_p >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "more than 2^31 points");
    if (!all_finite(q_xyz, 3 * n_q) || !all_finite(p_xyz, 3 * n_p)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "non-finite coordinate");
    return PDBEDA_OK;
}

// The compaction of k_contact_min's distances into the caller's (index, distance) rows and their count: written by k_contact_compact straight
// into the pinned block when it has room, else on the device and copied.  Complete after the next ctx_sync.
static int enqueue_compact(pdbeda_ctx *ctx, const double *d_dist, int64_t n_q, double cutoff, int64_t *out_index, double *out_distance, int64_t cap,
                           int64_t *n_out, int64_t *d_idx, double *d_odist, int64_t *d_nout) {
    const int64_t rows = std::min(cap, n_q);
    int64_t *r_i = pinned_out(ctx, out_index, (size_t)rows);
    double *r_d = pinned_out(ctx, out_distance, (size_t)rows);
    int64_t *r_n = pinned_out(ctx, n_out, 1);
    { PROF(ctx, "k_contact_compact"); hipLaunchKernelGGL(k_contact_compact, dim3(1), dim3(1024), 0, ctx->stream, d_dist, n_q, cutoff, r_i ? r_i : d_idx, r_d ? r_d : d_odist, rows, r_n ? r_n : d_nout); }
    HIP_TRY(ctx, hipGetLastError());
    if (!r_i && rows > 0) HIP_TRY(ctx, d2h(ctx, out_index, d_idx, 8 * rows));
    if (!r_d && rows > 0) HIP_TRY(ctx, d2h(ctx, out_distance, d_odist, 8 * rows));
    if (!r_n) HIP_TRY(ctx, d2h(ctx, n_out, d_nout, 8));
    return 0;
}

extern "C" int pdbeda_coord_contacts(pdbeda_ctx *ctx, const double *q_xyz, int64_t n_q, const double *p_xyz, int64_t n_p, double cutoff,
                                     int64_t *out_index, double *out_distance, int64_t cap, int64_t *n_out) {
    if (!ctx || !n_out || n_q < 0 || n_p < 0 || cap < 0) return PDBEDA_ERR_ARGUMENT;
    *n_out = 0;
    if (int rc = check_contacts_args(ctx, q_xyz, n_q, p_xyz, n_p, cutoff, out_index, out_distance, cap)) return rc;
    if (n_q == 0 || n_p == 0) return PDBEDA_OK;      // nothing to be near to: no rows (cdist + np.min would raise on an empty list)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CellGrid g;
    if (int rc = contacts_query_grid(ctx, q_xyz, n_q, cutoff, n_q + n_p, &g)) return rc;
    const int64_t cells = g.n_cells;
    std::vector<unsigned> zeros((size_t)cells, 0u);
    int64_t total = 0;
    double *d_q = nullptr, *d_p = nullptr, *d_dist = nullptr, *d_odist = nullptr;
    GridBuild gb;
    int64_t *d_idx = nullptr, *d_nout = nullptr;
    int rc = with_scratch(ctx, "coord contacts", [&](Carver &cv) {
        cv.take(d_q, 3 * n_q);
        cv.take(d_p, 3 * n_p);
        gb.carve(cv, cells, n_p, false);
        cv.take(d_dist, n_q);
        cv.take(d_idx, n_q);
        cv.take(d_odist, n_q);
        cv.take(d_nout, 1);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        {
            const H2DItem in[3] = {{d_q, q_xyz, (size_t)(24 * n_q)}, {d_p, p_xyz, (size_t)(24 * n_p)}, {gb.count, zeros.data(), (size_t)(4 * cells)}};
            // ONE copy whenever the pinned block holds it beside the rows (else one per item); the cell counts start from the zeros that ride in it
            HIP_TRY(ctx, h2d_row(ctx, in, 3, pinned_room_beside(ctx, 16 * (size_t)n_q + 64)));
        }
        gb.sort_points(ctx, g, d_p, n_p);
        { PROF(ctx, "k_contact_min"); hipLaunchKernelGGL(k_contact_min, dim3(grid_for(n_q, 256)), dim3(256), 0, st, d_q, n_q, gb.sorted, gb.start, g, d_dist); }
        HIP_TRY(ctx, hipGetLastError());
        return enqueue_compact(ctx, d_dist, n_q, cutoff, out_index, out_distance, cap, &total, d_idx, d_odist, d_nout);
    });
    if (rc) return rc;
    *n_out = total;
    if (total > cap) return fail(ctx, PDBEDA_ERR_CAPACITY, "need capacity %lld", (long long)total);
    return PDBEDA_OK;
}

extern "C" int pdbeda_crystal_contacts(pdbeda_ctx *ctx, const double *q_xyz, int64_t n_q, const double *poly_xyz, int64_t n_poly, const double *rot,
                                       int32_t n_ops, const double ortho[9], const int32_t *cand, int64_t n_cand, double cutoff, uint8_t *kept_out,
                                       int64_t *out_index, double *out_distance, int64_t cap, int64_t *n_out) {
    if (!ctx || !n_out || n_q < 0 || n_poly < 0 || n_cand < 0 || n_ops < 0 || cap < 0) return PDBEDA_ERR_ARGUMENT;
    *n_out = 0;
    if (int rc = check_contacts_args(ctx, q_xyz, n_q, poly_xyz, n_poly, cutoff, out_index, out_distance, cap)) return rc;
    if (int rc = check_images(ctx, rot, n_ops, ortho, cand, n_cand)) return rc;
    if (n_cand > 0 && n_poly > 0 && n_cand * n_poly >= (1ll << 32) - 1) return fail(ctx, PDBEDA_ERR_ARGUMENT, "more than 2^32 image atoms");
    if (kept_out && n_cand > 0) memset(kept_out, 0, (size_t)n_cand);
    if (n_cand == 0 || n_poly == 0) return PDBEDA_OK;   // no image: no neighbours, no rows (the reference's np.min of an empty array would raise)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double plo[3], phi[3];
    bbox3(poly_xyz, n_poly, plo, phi);
    const double inf_lo[3] = {-INFINITY, -INFINITY, -INFINITY}, inf_hi[3] = {INFINITY, INFINITY, INFINITY};
    CellGrid gp, gn = {};      // (no query: no neighbour grid)
    if (!make_cell_grid(plo, phi, cutoff, n_poly, inf_lo, inf_hi, &gp)) return refuse_extent(ctx, "polymer atoms", plo, phi);
    if (int rc = n_q > 0 ? contacts_query_grid(ctx, q_xyz, n_q, cutoff, n_q + n_poly, &gn) : 0) return rc;
    const int64_t cells_p = gp.n_cells, cells_n = n_q > 0 ? gn.n_cells : 0;
    std::vector<unsigned> zeros((size_t)std::max({cells_p, cells_n, n_cand}), 0u);
    std::vector<unsigned> h_keep((size_t)n_cand);
    unsigned h_total = 0;
    int64_t rows = 0;
    double *d_poly = nullptr, *d_q = nullptr, *d_rot = nullptr, *d_ortho = nullptr, *d_dist = nullptr, *d_odist = nullptr;
    int32_t *d_cand = nullptr;
    unsigned *d_keep = nullptr;
    GridBuild bp, bn;      // over the polymer; over the neighbours (counted and scattered by the image kernels: its points come in a second arena)
    int64_t *d_idx = nullptr, *d_nout = nullptr;
    Arena A, B;
    int rc = arena_carve(ctx, "crystal contacts", &A, [&](Carver &cv) {
        cv.take(d_poly, 3 * n_poly);
        cv.take(d_q, 3 * n_q);
        cv.take(d_rot, 12 * n_ops);
        cv.take(d_ortho, 9);
        cv.take(d_cand, 4 * n_cand);
        bp.carve_counts(cv, cells_p);
        cv.take(d_keep, n_cand);
        bn.carve_counts(cv, cells_n);
        bp.carve_rest(cv, cells_p, n_poly, false);
        bn.carve_rest(cv, cells_n, 0, false);
        cv.take(d_dist, n_q);
        cv.take(d_idx, n_q);
        cv.take(d_odist, n_q);
        cv.take(d_nout, 1);
    });
    if (rc) return rc;
    rc = [&]() -> int {
        hipStream_t st = ctx->stream;
        {   // inputs and the zeroed counters and flags in a row: ONE copy whenever the pinned block holds them (up to ~80 000 atoms), else one per item
            const H2DItem in[8] = {{d_poly, poly_xyz, (size_t)(24 * n_poly)}, {d_q, q_xyz, (size_t)(24 * n_q)}, {d_rot, rot, (size_t)(96 * n_ops)},
                                   {d_ortho, ortho, 72}, {d_cand, cand, (size_t)(16 * n_cand)}, {bp.count, zeros.data(), (size_t)(4 * cells_p)},
                                   {d_keep, zeros.data(), (size_t)(4 * n_cand)}, {bn.count, zeros.data(), (size_t)(4 * cells_n)}};
            HIP_TRY(ctx, h2d_row(ctx, in, 8, pinned_room_beside(ctx, 4 * (size_t)n_cand + 64)));
        }
        const int64_t lanes = n_cand * n_poly;
        bp.sort_points(ctx, gp, d_poly, n_poly);
        { PROF(ctx, "k_image_select"); hipLaunchKernelGGL(k_image_select, dim3(grid_for(lanes, 256)), dim3(256), 0, st, d_poly, n_poly, d_rot, d_ortho, d_cand, n_cand, bp.sorted, bp.start, gp, cutoff, d_keep); }
        if (n_q > 0) {      // (the keep flags and the neighbour count go to the host from inside these two launches: no copy launch)
            unsigned *r_keep = pinned_out(ctx, h_keep.data(), (size_t)n_cand);
            unsigned *r_total = pinned_out(ctx, &h_total, 1);
            { PROF(ctx, "k_image_count"); hipLaunchKernelGGL(k_image_count, dim3(grid_for(lanes, 256)), dim3(256), 0, st, d_poly, n_poly, d_rot, d_ortho, d_cand, n_cand, d_keep, gn, bn.count, r_keep); }
            bn.scan(ctx, gn, r_total);
            HIP_TRY(ctx, hipGetLastError());
            if (!r_keep) HIP_TRY(ctx, d2h(ctx, h_keep.data(), d_keep, 4 * (size_t)n_cand));
            if (!r_total) HIP_TRY(ctx, d2h(ctx, &h_total, bn.start + cells_n, 4));
        } else {
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, d2h(ctx, h_keep.data(), d_keep, 4 * (size_t)n_cand));
        }
        HIP_TRY(ctx, ctx_sync(ctx));                 // wait 1: the kept images and the size of the neighbour grid
        if (kept_out)
            for (int64_t c = 0; c < n_cand; ++c) kept_out[c] = h_keep[(size_t)c] ? 1 : 0;
        if (n_q == 0 || h_total == 0) return 0;
        if ((int64_t)h_total > lanes) return fail(ctx, PDBEDA_ERR_DEVICE, "neighbour grid holds %u points of at most %lld", h_total, (long long)lanes);
        if (int e = arena_carve(ctx, "crystal contacts: neighbours", &B, [&](Carver &cv) { cv.take(bn.sorted, 3 * (size_t)h_total); })) return e;
        { PROF(ctx, "k_image_scatter"); hipLaunchKernelGGL(k_image_scatter, dim3(grid_for(lanes, 256)), dim3(256), 0, st, d_poly, n_poly, d_rot, d_ortho, d_cand, n_cand, d_keep, gn, bn.cursor, bn.sorted, (int64_t)h_total); }
        { PROF(ctx, "k_contact_min"); hipLaunchKernelGGL(k_contact_min, dim3(grid_for(n_q, 256)), dim3(256), 0, st, d_q, n_q, bn.sorted, bn.start, gn, d_dist); }
        HIP_TRY(ctx, hipGetLastError());
        if (int e = enqueue_compact(ctx, d_dist, n_q, cutoff, out_index, out_distance, cap, &rows, d_idx, d_odist, d_nout)) return e;
        HIP_TRY(ctx, ctx_sync(ctx));                 // wait 2: the rows
        return 0;
    }();
    if (rc) {
        (void)ctx_sync(ctx);                         // (a failed call drains the stream before its arenas go back to the pool)
        return rc;
    }
    *n_out = rows;
    if (rows > cap) return fail(ctx, PDBEDA_ERR_CAPACITY, "need capacity %lld", (long long)rows);
    return PDBEDA_OK;
}

extern "C" int pdbeda_image_coords(pdbeda_ctx *ctx, const double *poly_xyz, int64_t n_poly, const double *rot, int32_t n_ops, const double ortho[9],
                                   const int32_t *cand, int64_t n_cand, double *out_xyz) {
    if (!ctx || n_poly < 0 || n_cand < 0 || n_ops < 0 || (n_poly > 0 && !poly_xyz) || (n_poly > 0 && n_cand > 0 && !out_xyz)) return PDBEDA_ERR_ARGUMENT;
    if (n_poly >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "more than 2^31 points");
    if (!all_finite(poly_xyz, 3 * n_poly)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "non-finite coordinate");
    if (int rc = check_images(ctx, rot, n_ops, ortho, cand, n_cand)) return rc;
    if (n_cand == 0 || n_poly == 0) return PDBEDA_OK;
    if (n_cand * n_poly >= (1ll << 32) - 1) return fail(ctx, PDBEDA_ERR_ARGUMENT, "more than 2^32 image atoms");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t total = n_cand * n_poly;
    double *d_poly = nullptr, *d_rot = nullptr, *d_ortho = nullptr;
    int32_t *d_cand = nullptr;
    Result<double> out{out_xyz, 3 * (size_t)total};
    return with_scratch(ctx, "image coords", [&](Carver &cv) {
        cv.take(d_poly, 3 * n_poly);
        cv.take(d_rot, 12 * n_ops);
        cv.take(d_ortho, 9);
        cv.take(d_cand, 4 * n_cand);
        out.carve(cv);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        {
            const H2DItem in[4] = {{d_poly, poly_xyz, (size_t)(24 * n_poly)}, {d_rot, rot, (size_t)(96 * n_ops)}, {d_ortho, ortho, 72}, {d_cand, cand, (size_t)(16 * n_cand)}};
            HIP_TRY(ctx, h2d_row(ctx, in, 4));
        }
        { PROF(ctx, "k_image_emit"); hipLaunchKernelGGL(k_image_emit, dim3(grid_for(total, 256)), dim3(256), 0, st, d_poly, n_poly, d_rot, d_ortho, d_cand, n_cand, out.at(ctx)); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, out.finish(ctx));
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// Nearest-atom partition of a map (no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// The launch graph: memset of the cell counts and the integer tables; the grid build (GridBuild, with each atom's original index) over the atoms
// inside the crop box -- the xyz bounding box of the map's box grown by the maximum distance (crop_cell_grid): an atom outside it owns nothing, and
// the grid never grows with atoms that lie far from the map; k_partition_tile, a workgroup per voxel tile; k_partition_finish.  One wait.
// Measured and removed: the same tile walking the 27 cells around every voxel in global memory instead of staging.
extern "C" int pdbeda_map_partition(pdbeda_map *m, const double *xyz, int64_t n_atoms, float max_distance, float cutoff,
                                    int64_t *n, double *sum, int64_t *n_pos, double *sum_pos, int64_t *n_neg, double *sum_neg,
                                    int64_t unowned_n[3], double unowned_sum[4], int32_t *owner) {
    if (!m || n_atoms < 0 || (n_atoms > 0 && !xyz)) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    if (!std::isfinite(max_distance) || !(max_distance > 0.0f)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map partition: the maximum distance must be finite and > 0");
    if (std::isnan(cutoff) || cutoff < 0.0f) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map partition: the cutoff must be >= 0");
    if (n_atoms >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map partition: 2^31 atoms or more");
    if (!all_finite(xyz, 3 * n_atoms)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map partition: non-finite coordinate");
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    const Geom &g = m->geom;
    const int uc = g.unique_ncrs[0], ur = g.unique_ncrs[1], us = g.unique_ncrs[2];
    const int64_t nbox = (int64_t)uc * ur * us;
    const TileGrid tg = tile_grid(g.unique_ncrs, PT_C, PT_R, PT_S);      // (a 1-D grid of tiles: only their number is limited)
    const int tiles_c = tg.nc, tiles_r = tg.nr;
    const int64_t n_tiles = tg.n;
    if (tg.refusal & (TILES_EMPTY | TILES_2P31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map partition: the box is empty or has 2^31 tiles or more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (m->fix_mul == 0.0 && !m->fix_refused) {      // (a wait when the map's range is not known yet: before anything is staged)
        const int rc = map_fix_mul(m);
        if (rc && !m->fix_refused) return rc;
    }
    const double maxd = (double)max_distance;
    const int32_t first[3] = {0, 0, 0}, last[3] = {uc - 1, ur - 1, us - 1};      // the grid of the atoms within the maximum distance of the box
    double blo[3], bhi[3];
    crs_box_xyz(g, first, last, blo, bhi);
    CellGrid grid;
    if (!crop_cell_grid(blo, bhi, maxd, xyz, n_atoms, &grid)) return fail(ctx, PDBEDA_ERR_STATE, "map partition: no cell grid over a finite box");
    const int64_t cells = grid.n_cells;
    const size_t na = (size_t)n_atoms, tables = 6 * na + 8;
    double *d_xyz = nullptr, *d_tsq = nullptr, *d_os = nullptr;
    GridBuild gb;
    unsigned long long *d_tab = nullptr;
    long long *d_on = nullptr, *d_un = nullptr;
    int32_t *d_owner = nullptr;
    return with_scratch(ctx, "map partition", [&](Carver &cv) {
        cv.take(d_xyz, 3 * na);
        gb.carve(cv, cells, n_atoms, true);
        cv.take(d_tab, tables);      // atom_n [3][n] | atom_sum [3][n] | unowned [6] | range [1]
        cv.take(d_tsq, n_tiles);
        cv.take(d_on, 3 * na);
        cv.take(d_os, 3 * na);
        cv.take(d_un, 8);      // unowned_n [3] | (as doubles) unowned_sum [4]
        if (owner) cv.take(d_owner, nbox);
    }, [&]() -> int {
        double *d_us = reinterpret_cast<double *>(d_un + 3);
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemsetAsync(gb.count, 0, 4 * (size_t)cells, st));
        HIP_TRY(ctx, hipMemsetAsync(d_tab, 0, 8 * tables, st));
        double fix_mul = 0.0;
        if (int rc = box_fix_mul(m, g.ncrs[0], g.ncrs[1], uc, ur, us, d_tab + tables - 1, &fix_mul)) return rc;
        if (n_atoms > 0) HIP_TRY(ctx, h2d_one(ctx, d_xyz, xyz, 24 * na));
        gb.sort_points(ctx, grid, d_xyz, n_atoms);
        PartitionArgs a;
        a.geom = m->geom_dev; a.dens = m->dens;
        a.uc = uc; a.ur = ur; a.us = us; a.tiles_c = tiles_c; a.tiles_r = tiles_r;
        a.grid = grid; a.sorted = gb.sorted; a.sorted_index = gb.sorted_index; a.start = gb.start;
        a.max_distance = maxd; a.cutoff = (double)cutoff; a.fix_mul = fix_mul;
        a.atom_n = d_tab; a.atom_sum = d_tab + 3 * na; a.n_atoms = n_atoms; a.unowned = d_tab + 6 * na;
        a.tile_sq = d_tsq; a.owner = d_owner;
        { PROF(ctx, "k_partition_tile"); hipLaunchKernelGGL(k_partition_tile, dim3((unsigned)n_tiles), dim3(256), 0, st, a); }
        { PROF(ctx, "k_partition_finish"); hipLaunchKernelGGL(k_partition_finish, dim3(grid_for(3 * n_atoms, 256, 1024) + 1), dim3(256), 0, st, a.atom_n, a.atom_sum, n_atoms, a.unowned, d_tsq, n_tiles, 1.0 / fix_mul, d_on, d_os, d_un, d_us); }
        HIP_TRY(ctx, hipGetLastError());
        const D2HItem parts[9] = {{n, d_on, 8 * na}, {n_pos, d_on + na, 8 * na}, {n_neg, d_on + 2 * na, 8 * na}, {sum, d_os, 8 * na}, {sum_pos, d_os + na, 8 * na},
                                  {sum_neg, d_os + 2 * na, 8 * na}, {unowned_n, d_un, 24}, {unowned_sum, d_us, 32}, {owner, d_owner, 4 * (size_t)nbox}};
        HIP_TRY(ctx, d2h_each(ctx, parts, 9));
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// The map between voxels: trilinear density and atom Q-scores (no reference counterpart; the contracts: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// A point the kernels may convert: finite, and every grid position below 2^29 in magnitude (the floor is cast to int32 and its neighbour is one more).
static bool frac_castable(const Geom &g, const double p[3]) {
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) return false;
    double f[3];
    xyz2frac(g, p, f);
    for (int q = 0; q < 3; ++q)
        if (!(std::fabs(f[q]) < (double)(1ll << 29))) return false;
    return true;
}

// The launch graph: the points (through the pinned block when they fit, else a copy), k_interp_density, the results.  One wait.
extern "C" int pdbeda_interp_density(pdbeda_map *m, const double *xyz, int64_t n, double *out, uint8_t *valid) {
    if (!m || n < 0 || (n > 0 && !xyz)) return PDBEDA_ERR_ARGUMENT;
    if (n == 0) return PDBEDA_OK;
    pdbeda_ctx *ctx = m->ctx;
    if (n >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "interpolated density: 2^31 points or more");
    for (int64_t i = 0; i < n; ++i)
        if (!frac_castable(m->geom, xyz + 3 * i))
            return fail(ctx, PDBEDA_ERR_ARGUMENT, "interpolated density: point %lld is not finite or lies 2^29 grid steps or more from the map's origin", (long long)i);
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Input<double> in{xyz, (size_t)(3 * n)};
    Result<double> r_out{out, (size_t)n};
    Result<uint8_t> r_valid{valid, (size_t)n};
    return with_scratch(ctx, "interpolated density", [&](Carver &cv) { in.carve(cv); r_out.carve(cv); r_valid.carve(cv); }, [&]() -> int {
        HIP_TRY(ctx, in.send(ctx));
        double *k_out = r_out.at(ctx);
        uint8_t *k_valid = r_valid.at(ctx);
        { PROF(ctx, "k_interp_density"); hipLaunchKernelGGL(k_interp_density, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, m->geom_dev, m->dens, in.at, n, k_out, k_valid); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, r_out.finish(ctx));
        HIP_TRY(ctx, r_valid.finish(ctx));
        return 0;
    });
}

// The launch graph: memset of the cell counts and the two counters; the atoms, the scored indices and the host's tables (reference profile,
// candidate directions); the grid build (GridBuild) over the atoms inside the crop box -- the scored atoms' bounding box grown by the reach,
// 2 R_max (crop_cell_grid): an atom outside it wins no sample point --; k_atom_qscores, a wave per scored atom; the results.  One wait.
extern "C" int pdbeda_atom_qscores(pdbeda_map *m, const double *xyz, int64_t n_all, const int32_t *scored, int64_t n_scored, float step, int32_t n_shells,
                                   const double *ref, const double *unit_pts, const int32_t *level_offsets, int32_t n_levels, int32_t min_points,
                                   double *q, int32_t *n_points, int32_t *shell_n, double *shell_mean, uint8_t *valid, int64_t counters[2]) {
    if (!m || n_all < 0 || n_scored < 0 || (n_all > 0 && !xyz)) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = m->ctx;
    if (!scored) n_scored = n_all;
    if (n_scored == 0) return PDBEDA_OK;
    if (n_all >= (1ll << 31) || n_scored >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: 2^31 atoms or more");
    if (!ref || !unit_pts || !level_offsets) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: null table");
    if (n_shells < 2 || n_shells > PDBEDA_MAX_SHELLS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: n_shells must be 2 .. %d", PDBEDA_MAX_SHELLS);
    if (n_levels < 1 || n_levels > PDBEDA_QSCORE_MAX_LEVELS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: n_levels must be 1 .. %d", PDBEDA_QSCORE_MAX_LEVELS);
    if (level_offsets[0] != 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: level_offsets must start at 0");
    for (int l = 0; l < n_levels; ++l) {
        const int64_t rows = (int64_t)level_offsets[l + 1] - level_offsets[l];
        if (rows < 1 || rows > PDBEDA_QSCORE_MAX_LEVEL_POINTS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: level %d has %lld candidates (1 .. %d)", l, (long long)rows, PDBEDA_QSCORE_MAX_LEVEL_POINTS);
    }
    if (min_points < 1 || min_points > level_offsets[1]) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: min_points must be 1 .. the size of level 0");
    if (!std::isfinite(step) || !(step > 0.0f)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: the step must be finite and > 0");
    const int64_t n_unit = level_offsets[n_levels];
    if (!all_finite(ref, n_shells) || !all_finite(unit_pts, 3 * n_unit)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: non-finite reference profile or direction");
    if (!all_finite(xyz, 3 * n_all)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: non-finite coordinate");
    const Geom &g = m->geom;
    const double r_max = (double)(n_shells - 1) * (double)step;
    // every sample point stays castable: |f(atom)| < 2^29 and the sphere of R_max spans fewer than 2^29 steps of every grid axis
    if (!reach_below_2p29_steps(g, r_max)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: the largest shell spans 2^29 grid steps or more");
    double slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n_scored; ++i) {
        const int64_t at = scored ? (int64_t)scored[i] : i;
        if (at < 0 || at >= n_all) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: scored[%lld] = %lld is outside the %lld atoms", (long long)i, (long long)at, (long long)n_all);
        const double *p = xyz + 3 * at;
        if (!frac_castable(g, p)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom Q-scores: atom %lld lies 2^29 grid steps or more from the map's origin", (long long)at);
        for (int k = 0; k < 3; ++k) { slo[k] = std::min(slo[k], p[k]); shi[k] = std::max(shi[k], p[k]); }
    }
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the grid of the atoms that can matter to a scored atom: those within the reach, 2 R_max, of the scored atoms' bounding box
    const double reach = 2.0 * r_max * (1.0 + 1e-6);
    CellGrid grid;
    if (!crop_cell_grid(slo, shi, reach, xyz, n_all, &grid)) return fail(ctx, PDBEDA_ERR_STATE, "atom Q-scores: no cell grid over a finite box");
    const int64_t cells = grid.n_cells;
    const size_t na = (size_t)n_all, ns = (size_t)n_scored, rows = ns * (size_t)n_shells;
    double *d_xyz = nullptr, *d_tab = nullptr, *d_q = nullptr, *d_mean = nullptr;
    GridBuild gb;
    int32_t *d_scored = nullptr, *d_np = nullptr, *d_sn = nullptr;
    uint8_t *d_valid = nullptr;
    unsigned long long *d_ctr = nullptr;
    return with_scratch(ctx, "atom Q-scores", [&](Carver &cv) {
        cv.take(d_xyz, 3 * na);
        cv.take(d_scored, scored ? ns : 0);
        cv.take(d_tab, (size_t)n_shells + 3 * (size_t)n_unit);      // ref [n_shells] | unit_pts [n_unit][3]
        gb.carve(cv, cells, n_all, true);
        cv.take(d_ctr, 2);
        cv.take(d_q, ns);
        cv.take(d_np, ns);
        cv.take(d_sn, rows);
        cv.take(d_mean, rows);
        cv.take(d_valid, ns);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemsetAsync(gb.count, 0, 4 * (size_t)cells, st));
        HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, 16, st));
        HIP_TRY(ctx, h2d_one(ctx, d_xyz, xyz, 24 * na));
        if (scored) HIP_TRY(ctx, h2d_one(ctx, d_scored, scored, 4 * ns));
        {
            const H2DItem in[2] = {{d_tab, ref, 8 * (size_t)n_shells}, {d_tab + n_shells, unit_pts, 24 * (size_t)n_unit}};
            HIP_TRY(ctx, h2d_row(ctx, in, 2));
        }
        gb.sort_points(ctx, grid, d_xyz, n_all);
        QScoreArgs a;
        a.geom = m->geom_dev; a.dens = m->dens; a.xyz = d_xyz; a.scored = scored ? d_scored : nullptr; a.n_scored = n_scored;
        a.grid = grid; a.sorted = gb.sorted; a.sorted_index = gb.sorted_index; a.start = gb.start;
        a.step = (double)step; a.reach2 = reach * reach;
        a.n_shells = n_shells; a.n_levels = n_levels; a.min_points = min_points;
        for (int l = 0; l <= PDBEDA_QSCORE_MAX_LEVELS; ++l) a.level_off[l] = level_offsets[std::min(l, n_levels)];
        a.ref = d_tab; a.unit = d_tab + n_shells;
        a.q = d_q; a.n_points = d_np; a.shell_n = d_sn; a.shell_mean = d_mean; a.valid = d_valid; a.counters = d_ctr;
        { PROF(ctx, "k_atom_qscores"); hipLaunchKernelGGL(k_atom_qscores, dim3((unsigned)((n_scored + 3) / 4)), dim3(256), 0, st, a); }
        HIP_TRY(ctx, hipGetLastError());
        const D2HItem parts[6] = {{q, d_q, 8 * ns}, {n_points, d_np, 4 * ns}, {shell_n, d_sn, 4 * rows}, {shell_mean, d_mean, 8 * rows}, {valid, d_valid, ns}, {counters, d_ctr, 16}};
        HIP_TRY(ctx, d2h_each(ctx, parts, 6));
        return 0;
    });
}

// ------------------------------------------------------------------------------------
// From the model to a map: the density of Gaussian atoms, the sums that correlate two maps (no reference counterpart; the contracts: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// The launch graph: memset of the cell counts and the two counters; the atoms' coordinates, amplitudes, exponents and radii in one row of scratch;
// the grid build (GridBuild) over the atoms inside the crop box -- the xyz bounding box of the STORED box grown by the largest radius
// (crop_cell_grid): an atom outside it reaches no voxel, and the grid never grows with atoms that lie far from the map --; k_model_tile, a workgroup per
// tile of stored voxels, which writes the float32 voxels itself; the counters.  One wait.  The new map's arena is taken first and goes back to the pool
// with the half-made map when anything fails: *out is written last.
extern "C" int pdbeda_model_density(pdbeda_map *like, const double *xyz, int64_t n_atoms, int32_t n_terms, const double *amp, const double *expo, const float *radii,
                                    pdbeda_map **out, int64_t counters[3]) {
    if (!like || !out || n_atoms < 0 || (n_atoms > 0 && (!xyz || !amp || !expo || !radii))) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = like->ctx;
    if (n_terms < 1 || n_terms > PDBEDA_MODEL_MAX_TERMS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: n_terms must be 1 .. %d", PDBEDA_MODEL_MAX_TERMS);
    if (n_atoms >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: 2^31 atoms or more");
    if (!all_finite(xyz, 3 * n_atoms)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: non-finite coordinate");
    const int64_t n_pairs = n_atoms * n_terms;
    if (!all_finite(amp, n_pairs) || !all_finite(expo, n_pairs)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: non-finite amplitude or exponent");
    for (int64_t i = 0; i < n_pairs; ++i)
        if (expo[i] < 0.0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: the exponent of atom %lld is negative", (long long)(i / n_terms));
    float r_top = 0.0f;
    for (int64_t i = 0; i < n_atoms; ++i) {
        if (!std::isfinite(radii[i]) || !(radii[i] > 0.0f)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: the radius of atom %lld is not finite or <= 0", (long long)i);
        r_top = std::max(r_top, radii[i]);
    }
    const Geom &g = like->geom;
    const double r_max = n_atoms > 0 ? (double)r_top : 1.0;      // (no atom: any cell edge will do)
    if (!reach_below_2p29_steps(g, r_max)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: the largest radius spans 2^29 grid steps or more");
    const int nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2];
    const TileGrid tg = tile_grid(g.ncrs, PT_C, PT_R, PT_S);      // (a 1-D grid of tiles: only their number is limited)
    const int tiles_c = tg.nc, tiles_r = tg.nr;
    const int64_t n_tiles = tg.n;
    if (tg.refusal & (TILES_EMPTY | TILES_2P31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: the map is empty or has 2^31 tiles or more");
    const int32_t first[3] = {0, 0, 0}, last[3] = {nc - 1, nr - 1, ns - 1};      // the grid of the atoms within the largest radius of the STORED box
    double blo[3], bhi[3];
    crs_box_xyz(g, first, last, blo, bhi);
    CellGrid grid;
    if (!crop_cell_grid(blo, bhi, r_max, xyz, n_atoms, &grid)) return fail(ctx, PDBEDA_ERR_STATE, "model density: no cell grid over a finite box");
    // S: from the atoms the grid will hold and the largest sum of |amplitudes| of ANY atom
    int64_t n_gridded = 0;
    double a_max = 0.0;
    for (int64_t i = 0; i < n_atoms; ++i) {
        if (!grid_cropped(grid, xyz + 3 * i)) ++n_gridded;
        double t = 0.0;
        for (int j = 0; j < n_terms; ++j) t += std::fabs(amp[i * n_terms + j]);
        a_max = std::max(a_max, t);
    }
    if (!std::isfinite((double)std::max<int64_t>(n_gridded, 1) * a_max)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "model density: the amplitudes of an atom add up beyond fp64");
    const int S = model_shift(n_gridded, a_max);      // (pdbeda_jobplan.h)
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t cells = grid.n_cells;
    const size_t na = (size_t)n_atoms, np = (size_t)n_pairs;
    MadeMap made;
    if (int rc = made.make_like("model density", like)) return rc;
    double *d_xyz = nullptr, *d_amp = nullptr, *d_expo = nullptr;
    float *d_radii = nullptr;
    GridBuild gb;
    unsigned long long *d_ctr = nullptr;
    int64_t seen[2] = {0, 0};
    const int rc = with_scratch(ctx, "model density", [&](Carver &cv) {
        cv.take(d_xyz, 3 * na);
        cv.take(d_amp, np);
        cv.take(d_expo, np);
        cv.take(d_radii, na);
        gb.carve(cv, cells, n_atoms, true);
        cv.take(d_ctr, 2);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemsetAsync(gb.count, 0, 4 * (size_t)cells, st));
        HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, 16, st));
        HIP_TRY(ctx, made.geometry_up());
        if (n_atoms > 0) {
            const H2DItem in[4] = {{d_xyz, xyz, 24 * na}, {d_amp, amp, 8 * np}, {d_expo, expo, 8 * np}, {d_radii, radii, 4 * na}};
            HIP_TRY(ctx, h2d_row(ctx, in, 4));
        }
        gb.sort_points(ctx, grid, d_xyz, n_atoms);
        ModelArgs a;
        a.geom = made.m->geom_dev; a.tiles_c = tiles_c; a.tiles_r = tiles_r;
        a.grid = grid; a.sorted = gb.sorted; a.sorted_index = gb.sorted_index; a.start = gb.start;
        a.amp = d_amp; a.expo = d_expo; a.radii = d_radii; a.n_terms = n_terms;
        a.r_max = r_max; a.fix_mul = ldexp(1.0, S); a.fix_inv = ldexp(1.0, -S);
        a.out = made.dens; a.counters = d_ctr;
        { PROF(ctx, "k_model_tile"); hipLaunchKernelGGL(k_model_tile, dim3((unsigned)n_tiles), dim3(256), 0, st, a); }
        HIP_TRY(ctx, hipGetLastError());
        if (counters) HIP_TRY(ctx, d2h(ctx, seen, d_ctr, 16));
        return 0;
    });
    if (rc) return rc;
    if (counters) { counters[0] = S; counters[1] = seen[0]; counters[2] = seen[1]; }
    made.publish(out);
    return PDBEDA_OK;
}

// The launch graph: k_pair_moments over a number of workgroups fixed by the box, k_pair_moments_fold, the six results.  One wait.
extern "C" int pdbeda_map_pair_moments(pdbeda_map *a, pdbeda_map *b, float b_floor, int64_t *n, double sums[5]) {
    if (!a || !b) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = a->ctx;
    if (int rc = same_grid(ctx, a->geom, a->n_vox, b, "maps of different shapes", true)) return rc;
    if (std::isnan(b_floor)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "pair moments: the floor is NaN");
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    const Geom &g = a->geom;
    const int uc = g.unique_ncrs[0], ur = g.unique_ncrs[1], us = g.unique_ncrs[2];
    const int64_t nbox = (int64_t)uc * ur * us;
    if (nbox <= 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "pair moments: the box is empty");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned blocks = grid_for(nbox, 256, PM_BLOCKS);
    double *d_part = nullptr, *d_res = nullptr;
    double res[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int rc = with_scratch(ctx, "pair moments", [&](Carver &cv) { cv.take(d_part, 6 * (size_t)blocks); cv.take(d_res, 6); }, [&]() -> int {
        { PROF(ctx, "k_pair_moments"); hipLaunchKernelGGL(k_pair_moments, dim3(blocks), dim3(256), 0, ctx->stream, a->dens, b->dens, g.ncrs[0], g.ncrs[1], uc, ur, us, (double)b_floor, d_part); }
        { PROF(ctx, "k_pair_moments_fold"); hipLaunchKernelGGL(k_pair_moments_fold, dim3(1), dim3(256), 0, ctx->stream, d_part, (int)blocks, d_res); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, d2h(ctx, res, d_res, 48));
        return 0;
    });
    if (rc) return rc;
    if (n) *n = (int64_t)res[0];
    if (sums) memcpy(sums, res + 1, 40);
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// From a map back to the atoms: the adjoint of the model density (no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// The xyz -> crs map of a geometry as the plan takes it (xyz2frac's arithmetic, row by row) and the domain.
static GradGrid grad_grid_of(const Geom &g, bool unique_box) {
    GradGrid gg = GradGrid();
    for (int k = 0; k < 3; ++k) {
        const int a = g.map2crs[k];
        if (g.orthogonal) {
            gg.rows[3 * k + a] = 1.0 / g.grid_len[a];
            gg.off[k] = -(g.origin[a] / g.grid_len[a]);
        } else {
            for (int i = 0; i < 3; ++i) gg.rows[3 * k + i] = g.deortho[3 * a + i] * (double)g.xyz_interval[a];
            gg.off[k] = -(double)sel3(g.crs_start, g.map2xyz[a]);
        }
        gg.dom[k] = unique_box ? std::min(g.unique_ncrs[k], g.ncrs[k]) : g.ncrs[k];
    }
    grad_grid_norms(&gg);
    return gg;
}

template <int NT>
static void atom_moments_launch(pdbeda_ctx *ctx, unsigned blocks, const GradArgs &a) {
    PROF(ctx, "k_atom_moments");
    hipLaunchKernelGGL(k_atom_moments<NT>, dim3(blocks), dim3(256), 0, ctx->stream, a);
}

// The launch graph: the host's checks and boxes (pdbeda_gradplan.h); the range pass when the map's max |w| is not cached yet (a wait); the atoms'
// coordinates, exponents, radii and boxes in one row of scratch; k_atom_moments<n_terms>, a wave per atom; the results.  One wait.
extern "C" int pdbeda_atom_moments(pdbeda_map *weight, const double *xyz, int64_t n_atoms, int32_t n_terms, const double *expo, const float *radii, uint32_t flags,
                                   double *moments, int32_t *n_voxels, int64_t counters[3]) {
    if (!weight || (n_atoms > 0 && (!xyz || !expo || !radii))) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = weight->ctx;
    int64_t bad = -1;
    float r_top = 0.0f;
    switch (grad_check(xyz, n_atoms, n_terms, expo, radii, flags, PDBEDA_MOMENTS_UNIQUE_BOX, &bad, &r_top)) {
    case GRAD_TERMS: return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: n_terms must be 1 .. %d", PDBEDA_MODEL_MAX_TERMS);
    case GRAD_FLAG: return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: unknown flag 0x%x", flags);
    case GRAD_COUNT: return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: a negative number of atoms, or 2^31 or more");
    case GRAD_XYZ: return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: a coordinate of atom %lld is not finite", (long long)bad);
    case GRAD_EXPO: return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: an exponent of atom %lld is not finite or negative", (long long)bad);
    case GRAD_RADIUS: return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: the radius of atom %lld is not finite or <= 0", (long long)bad);
    default: break;
    }
    if (n_atoms == 0) return PDBEDA_OK;
    const Geom &g = weight->geom;
    const GradGrid gg = grad_grid_of(g, (flags & PDBEDA_MOMENTS_UNIQUE_BOX) != 0);
    const double r_max = (double)r_top;
    if (!grad_reach_ok(gg, r_max)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: the largest radius spans 2^29 grid steps or more");
    std::vector<GradBox> boxes((size_t)n_atoms);
    int64_t v_max = 0, n_clipped = 0;
    for (int64_t i = 0; i < n_atoms; ++i) {
        bool clipped = false;
        const int64_t vox = grad_box(gg, xyz + 3 * i, (double)radii[i], &boxes[(size_t)i], &clipped);
        if (grad_box_too_large(vox)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom moments: the box of atom %lld holds 2^31 voxels or more", (long long)i);
        v_max = std::max(v_max, vox);
        n_clipped += clipped ? 1 : 0;
    }
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = map_fix_mul(weight)) return rc;      // (a wait when the map's range is not known yet; a map with non-finite voxels is refused here)
    const int S = grad_shift(weight->max_abs, r_max, v_max);
    const size_t na = (size_t)n_atoms, np = na * (size_t)n_terms;
    double *d_xyz = nullptr, *d_expo = nullptr, *d_mom = nullptr;
    float *d_radii = nullptr;
    GradBox *d_box = nullptr;
    int32_t *d_nv = nullptr;
    const int rc = with_scratch(ctx, "atom moments", [&](Carver &cv) {
        cv.take(d_xyz, 3 * na);
        cv.take(d_expo, np);
        cv.take(d_radii, na);
        cv.take(d_box, na);
        cv.take(d_mom, 5 * np);
        cv.take(d_nv, na);
    }, [&]() -> int {
        const H2DItem in[4] = {{d_xyz, xyz, 24 * na}, {d_expo, expo, 8 * np}, {d_radii, radii, 4 * na}, {d_box, boxes.data(), sizeof(GradBox) * na}};
        HIP_TRY(ctx, h2d_row(ctx, in, 4));
        GradArgs a;
        a.geom = weight->geom_dev; a.w = weight->dens;
        a.xyz = d_xyz; a.expo = d_expo; a.radii = d_radii; a.box = d_box; a.n_atoms = (int)n_atoms;
        a.fix_mul = ldexp(1.0, S); a.fix_inv = ldexp(1.0, -S);
        a.moments = d_mom; a.n_voxels = d_nv;
        const unsigned blocks = grid_for(n_atoms, GP_WAVES, 8192);
        switch (n_terms) {
        case 1: atom_moments_launch<1>(ctx, blocks, a); break;
        case 2: atom_moments_launch<2>(ctx, blocks, a); break;
        case 3: atom_moments_launch<3>(ctx, blocks, a); break;
        case 4: atom_moments_launch<4>(ctx, blocks, a); break;
        case 5: atom_moments_launch<5>(ctx, blocks, a); break;
        default: atom_moments_launch<6>(ctx, blocks, a); break;
        }
        HIP_TRY(ctx, hipGetLastError());
        const D2HItem parts[2] = {{moments, d_mom, 40 * np}, {n_voxels, d_nv, 4 * na}};
        HIP_TRY(ctx, d2h_each(ctx, parts, 2));
        return 0;
    });
    if (rc) return rc;
    if (counters) { counters[0] = S; counters[1] = v_max; counters[2] = n_clipped; }
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// What fits in a blob: rigid-fragment poses scored on a map (no reference counterpart; the contract: include/pdbeda.h, the plan: pdbeda_poseplan.h)
// ------------------------------------------------------------------------------------
// A staged box may take more dynamic LDS than the 64 KiB a kernel gets unasked: told to the runtime once per process.
static hipError_t pose_lds_allowance() {
    static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pose_scores), hipFuncAttributeMaxDynamicSharedMemorySize, POSE_LDS_BUDGET);
    return e;
}

// The launch graph: the host's checks and boxes (pdbeda_poseplan.h); the fragment, its weights and the rotations in one row of scratch, once; then per chunk
// of centres (pose_chunk: the score table stays within POSE_TABLE_BYTES) the chunk's centres and boxes, k_pose_scores -- a workgroup per centre, dynamic LDS
// for the chunk's largest staged box --, the requested rows and tables, and a wait.
extern "C" int pdbeda_pose_scores(pdbeda_map *map, const double *frag_xyz, const double *frag_w, int32_t n_frag, const double *rot, int64_t n_rot, const double *centres,
                                  int64_t n_centres, float floor, int32_t max_low, int32_t top_k, uint32_t flags, int32_t *best_rot, double *best_score, int32_t *best_low,
                                  int32_t *n_kept, double *all_score, int32_t *all_low, uint8_t *all_kept, int64_t counters[3]) {
    if (!map || !frag_xyz || !frag_w || !rot || (n_centres > 0 && !centres)) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = map->ctx;
    int64_t bad = -1;
    double radius = 0.0;
    switch (pose_check(frag_xyz, frag_w, n_frag, rot, n_rot, centres, n_centres, top_k, flags, PDBEDA_POSE_ALLOW_OUTSIDE | PDBEDA_POSE_GLOBAL_ONLY, &bad, &radius)) {
    case POSE_ATOMS: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: n_frag must be 1 .. %d", PDBEDA_POSE_MAX_ATOMS);
    case POSE_ROTATIONS: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: n_rot must be 1 .. %d", PDBEDA_POSE_MAX_ROTATIONS);
    case POSE_TOP: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: top_k must be 1 .. %d", PDBEDA_POSE_MAX_TOP);
    case POSE_FLAG: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: unknown flag 0x%x", flags);
    case POSE_COUNT: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: a negative number of centres, or n_centres * n_rot is 2^31 or more");
    case POSE_FRAG_VALUE: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: a coordinate or the weight of fragment atom %lld is not finite", (long long)bad);
    case POSE_ROT_VALUE: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: an entry of rotation %lld is not finite", (long long)bad);
    case POSE_CENTRE_VALUE: return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: a coordinate of centre %lld is not finite", (long long)bad);
    default: break;
    }
    if (n_centres == 0) return PDBEDA_OK;
    const Geom &g = map->geom;
    const GradGrid gg = grad_grid_of(g, false);
    if (!grad_reach_ok(gg, radius)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: the fragment's radius spans 2^29 grid steps or more");
    for (int64_t i = 0; i < n_centres; ++i)
        if (!pose_centre_ok(gg, centres + 3 * i)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "pose scores: centre %lld lies 2^29 grid steps or more from the map's origin", (long long)i);
    const bool global_only = (flags & PDBEDA_POSE_GLOBAL_ONLY) != 0;
    std::vector<PoseBox> boxes((size_t)n_centres);
    int64_t n_global = 0, top_box = 0;
    for (int64_t i = 0; i < n_centres; ++i) {
        const int64_t vox = pose_box(gg, centres + 3 * i, radius, global_only, &boxes[(size_t)i]);
        if (boxes[(size_t)i].staged) top_box = std::max(top_box, vox); else ++n_global;
    }
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (pose_lds_bytes(top_box) > 64 * 1024) HIP_TRY(ctx, pose_lds_allowance());
    const int64_t chunk = pose_chunk(n_centres, n_rot);
    const size_t nf = (size_t)n_frag, nr = (size_t)n_rot, k = (size_t)top_k;
    std::vector<int32_t> kept_of((size_t)n_centres);
    PoseScratch sc;
    const int rc = with_scratch(ctx, "pose scores", [&](Carver &cv) { sc.carve(cv, n_frag, n_rot, chunk, top_k); }, [&]() -> int {
        const H2DItem in[3] = {{sc.frag, frag_xyz, 24 * nf}, {sc.w, frag_w, 8 * nf}, {sc.rot, rot, 72 * nr}};
        HIP_TRY(ctx, h2d_row(ctx, in, 3));
        for (int64_t c0 = 0; c0 < n_centres; c0 += chunk) {
            const size_t ch = (size_t)std::min(chunk, n_centres - c0), at = (size_t)c0;
            const H2DItem per[2] = {{sc.centres, centres + 3 * c0, 24 * ch}, {sc.box, boxes.data() + c0, sizeof(PoseBox) * ch}};
            HIP_TRY(ctx, h2d_row(ctx, per, 2));
            int64_t lds_box = 0;
            for (size_t i = 0; i < ch; ++i)
                if (boxes[at + i].staged) lds_box = std::max<int64_t>(lds_box, (int64_t)boxes[at + i].n[0] * boxes[at + i].n[1] * boxes[at + i].n[2]);
            PoseArgs a;
            a.geom = map->geom_dev; a.dens = map->dens;
            a.frag = sc.frag; a.w = sc.w; a.rot = sc.rot; a.centres = sc.centres; a.box = sc.box;
            a.n_frag = n_frag; a.n_rot = (int)n_rot; a.top_k = top_k;
            a.floor_d = (double)floor; a.max_low = max_low; a.allow_outside = (flags & PDBEDA_POSE_ALLOW_OUTSIDE) ? 1 : 0;
            a.score = sc.score; a.low = sc.low; a.kept = sc.kept;
            a.best_rot = sc.best_rot; a.best_score = sc.best_score; a.best_low = sc.best_low; a.n_kept = sc.n_kept;
            { PROF(ctx, "k_pose_scores"); hipLaunchKernelGGL(k_pose_scores, dim3((unsigned)ch), dim3(256), (size_t)pose_lds_bytes(lds_box), ctx->stream, a); }
            HIP_TRY(ctx, hipGetLastError());
            const D2HItem parts[7] = {{best_rot ? best_rot + at * k : nullptr, sc.best_rot, 4 * ch * k}, {best_score ? best_score + at * k : nullptr, sc.best_score, 8 * ch * k},
                                      {best_low ? best_low + at * k : nullptr, sc.best_low, 4 * ch * k}, {kept_of.data() + at, sc.n_kept, 4 * ch},
                                      {all_score ? all_score + at * nr : nullptr, sc.score, 8 * ch * nr}, {all_low ? all_low + at * nr : nullptr, sc.low, 4 * ch * nr},
                                      {all_kept ? all_kept + at * nr : nullptr, sc.kept, ch * nr}};
            HIP_TRY(ctx, d2h_each(ctx, parts, 7));
            if (c0 + chunk < n_centres) HIP_TRY(ctx, ctx_sync(ctx));      // (the next chunk writes the same table: this one's copies are done first)
        }
        return 0;
    });
    if (rc) return rc;
    int64_t rejected = 0;
    for (int64_t i = 0; i < n_centres; ++i) rejected += n_rot - kept_of[(size_t)i];
    if (n_kept) memcpy(n_kept, kept_of.data(), 4 * (size_t)n_centres);
    if (counters) { counters[0] = n_global; counters[1] = top_box; counters[2] = rejected; }
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// From a map to a map through a neighbourhood: the separable filter and the windowed moments (no reference counterpart; the contracts: include/pdbeda.h)
// ------------------------------------------------------------------------------------
struct FilterAxes {
    FilterTaps taps[3];
    std::vector<double> weight[3];      // W_axis[i] = sum_k w[k + R] * present(i + k), the kernels' order and arithmetic
};

// The checks both entry points share, then the taps and (want_w) the W arrays.  0, or the failure's status.
static int filter_axes(pdbeda_ctx *ctx, const char *what, const Geom &g, const double *const taps[3], const int32_t radius[3], bool nonneg, bool want_w, FilterAxes *fa) {
    static const char axis_name[3] = {'c', 'r', 's'};
    for (int ax = 0; ax < 3; ++ax) {
        const int R = radius[ax];
        if (R < 0 || R > PDBEDA_FILTER_MAX_RADIUS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s: radius %d along %c is outside 0 .. %d", what, R, axis_name[ax], PDBEDA_FILTER_MAX_RADIUS);
        if (!taps[ax]) return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s: no taps along %c", what, axis_name[ax]);
        if (!all_finite(taps[ax], 2 * R + 1)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s: a non-finite tap along %c", what, axis_name[ax]);
        if (nonneg)
            for (int k = 0; k <= 2 * R; ++k)
                if (taps[ax][k] < 0.0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s: tap %d along %c is negative", what, k, axis_name[ax]);
        if (g.ncrs[ax] <= 0 || g.ncrs[ax] >= (1 << 30) || g.crs_interval[ax] <= 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "%s: the map is empty, or an axis has 2^30 indices or more", what);
    }
    for (int ax = 0; ax < 3; ++ax) {
        FilterTaps &t = fa->taps[ax];
        memset(&t, 0, sizeof t);
        t.radius = radius[ax];
        memcpy(t.w, taps[ax], sizeof(double) * (size_t)(2 * radius[ax] + 1));
        if (!want_w) continue;
        const int n = g.ncrs[ax], I = g.crs_interval[ax], R = radius[ax];
        fa->weight[ax].resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int k = 0; k <= 2 * R; ++k) acc += t.w[k] * (wrap_axis(i - R + k, n, I) >= 0 ? 1.0 : 0.0);
            fa->weight[ax][(size_t)i] = acc;
        }
    }
    return 0;
}

// A pass of k_filter_line along r (axis 1) or s (axis 2).
template <typename OUT>
static void filter_line_launch(pdbeda_ctx *ctx, const Geom &g, int axis, const FilterTaps &t, const double *in, OUT *out, const double *w_c, const double *w_f, const double *w_o) {
    const int nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2];
    const int n = axis == 1 ? nr : ns, n_other = axis == 1 ? ns : nr;
    const int64_t stride = axis == 1 ? (int64_t)nc : (int64_t)nc * nr, other_stride = axis == 1 ? (int64_t)nc * nr : (int64_t)nc;
    const int col_tiles = (nc + FL_LANES - 1) / FL_LANES, chunks = (n + FL_CHUNK - 1) / FL_CHUNK;
    const size_t lds = sizeof(double) * (size_t)(FL_CHUNK + 2 * t.radius) * FL_LANES;
    PROF(ctx, axis == 1 ? "k_filter_line_r" : "k_filter_line_s");
    hipLaunchKernelGGL(k_filter_line<OUT>, dim3((unsigned)((int64_t)col_tiles * chunks * n_other)), dim3(256), lds, ctx->stream, in, nc, n, g.crs_interval[axis], stride, n_other,
                       other_stride, col_tiles, chunks, t, out, w_c, w_f, w_o, axis == 1 ? 1 : 0);
}

// The workgroups of the widest pass stay below 2^31.
static bool filter_grid_fits(const Geom &g) {
    const int64_t nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2];
    const int64_t col = (nc + FL_LANES - 1) / FL_LANES, run = (nc + FC_RUN - 1) / FC_RUN;
    const int64_t lim = 1ll << 31;
    return run * ((nr * ns + FC_ROWS - 1) / FC_ROWS) < lim && col * ((nr + FL_CHUNK - 1) / FL_CHUNK) * ns < lim && col * ((ns + FL_CHUNK - 1) / FL_CHUNK) * nr < lim;
}

// The launch graph: the W arrays (under renormalisation) in one row of scratch; k_filter_c<1> from the map into fp64 volume 0; k_filter_line<double> along r
// into volume 1; k_filter_line<float> along s into the new map.  One wait.  Scratch: two fp64 volumes.
extern "C" int pdbeda_map_filter(pdbeda_map *map, const double *taps_c, int32_t radius_c, const double *taps_r, int32_t radius_r, const double *taps_s, int32_t radius_s,
                                 uint32_t flags, pdbeda_map **out) {
    if (!map || !out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = map->ctx;
    if (flags & ~PDBEDA_FILTER_RENORMALIZE) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map filter: unknown flag 0x%x", flags);
    const bool renorm = (flags & PDBEDA_FILTER_RENORMALIZE) != 0;
    const Geom &g = map->geom;
    const double *const taps[3] = {taps_c, taps_r, taps_s};
    const int32_t radius[3] = {radius_c, radius_r, radius_s};
    FilterAxes fa;
    if (int rc = filter_axes(ctx, "map filter", g, taps, radius, renorm, renorm, &fa)) return rc;
    if (map->n_vox <= 0 || !filter_grid_fits(g)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map filter: the map is empty or too large for one launch");
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2];
    const size_t nv = (size_t)map->n_vox;
    MadeMap made;
    if (int rc = made.make_like("map filter", map)) return rc;
    double *d_vol = nullptr, *d_wc = nullptr, *d_wr = nullptr, *d_ws = nullptr;
    const int rc = with_scratch(ctx, "map filter", [&](Carver &cv) {
        cv.take(d_vol, 2 * nv);
        cv.take(d_wc, renorm ? (size_t)nc : 0);
        cv.take(d_wr, renorm ? (size_t)nr : 0);
        cv.take(d_ws, renorm ? (size_t)ns : 0);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, made.geometry_up());
        if (renorm) {
            const H2DItem in[3] = {{d_wc, fa.weight[0].data(), 8 * (size_t)nc}, {d_wr, fa.weight[1].data(), 8 * (size_t)nr}, {d_ws, fa.weight[2].data(), 8 * (size_t)ns}};
            HIP_TRY(ctx, h2d_row(ctx, in, 3));
        }
        const int64_t rows = (int64_t)nr * ns;
        const int runs = (nc + FC_RUN - 1) / FC_RUN;
        { PROF(ctx, "k_filter_c"); hipLaunchKernelGGL(k_filter_c<1>, dim3((unsigned)(runs * ((rows + FC_ROWS - 1) / FC_ROWS))), dim3(256), 0, st, map->dens, (const float *)nullptr, nc,
                                                       g.crs_interval[0], rows, runs, fa.taps[0], d_vol, (int64_t)nv); }
        filter_line_launch<double>(ctx, g, 1, fa.taps[1], d_vol, d_vol + nv, nullptr, nullptr, nullptr);
        filter_line_launch<float>(ctx, g, 2, fa.taps[2], d_vol + nv, made.dens, renorm ? d_wc : nullptr, renorm ? d_ws : nullptr, renorm ? d_wr : nullptr);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    made.publish(out);
    return PDBEDA_OK;
}

// The launch graph: the W arrays in one row of scratch; k_filter_c<2 or 5> reads a (and b) ONCE and writes every channel; per channel a pass along r and one
// along s, through ONE spare volume -- channel k goes from volume k to volume k - 1 along r (channel 0 to the spare one, in ascending k) and back to volume k
// along s (in descending k); k_local_finish writes the requested maps.  One wait.  Scratch: channels + 1 fp64 volumes, 3 for one map and 6 for a pair.
extern "C" int pdbeda_map_local_stats(pdbeda_map *a, pdbeda_map *b, const double *taps_c, int32_t radius_c, const double *taps_r, int32_t radius_r, const double *taps_s,
                                      int32_t radius_s, double std_floor, pdbeda_map **mean_a, pdbeda_map **std_a, pdbeda_map **z_a, pdbeda_map **mean_b, pdbeda_map **std_b,
                                      pdbeda_map **cc) {
    if (!a) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = a->ctx;
    if (b) {
        if (int rc = same_grid(ctx, a->geom, a->n_vox, b)) return rc;
    } else if (mean_b || std_b || cc) {
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "local stats: an output of the second map is requested without a second map");
    }
    if (!(std_floor >= 0.0)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "local stats: std_floor is negative or NaN");
    const Geom &g = a->geom;
    const double *const taps[3] = {taps_c, taps_r, taps_s};
    const int32_t radius[3] = {radius_c, radius_r, radius_s};
    FilterAxes fa;
    if (int rc = filter_axes(ctx, "local stats", g, taps, radius, true, true, &fa)) return rc;
    if (a->n_vox <= 0 || !filter_grid_fits(g)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "local stats: the map is empty or too large for one launch");
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2];
    const size_t nv = (size_t)a->n_vox;
    const int n_ch = b ? 5 : 2;
    pdbeda_map **const want[6] = {mean_a, std_a, z_a, mean_b, std_b, cc};
    MadeMap made[6];
    for (int k = 0; k < 6; ++k)
        if (want[k])
            if (int rc = made[k].make_like("local stats", a)) return rc;
    double *d_vol = nullptr, *d_wc = nullptr, *d_wr = nullptr, *d_ws = nullptr;
    const int rc = with_scratch(ctx, "local stats", [&](Carver &cv) {
        cv.take(d_vol, (size_t)(n_ch + 1) * nv);
        cv.take(d_wc, (size_t)nc);
        cv.take(d_wr, (size_t)nr);
        cv.take(d_ws, (size_t)ns);
    }, [&]() -> int {
        hipStream_t st = ctx->stream;
        for (int k = 0; k < 6; ++k)
            if (made[k].m) HIP_TRY(ctx, made[k].geometry_up());
        const H2DItem in[3] = {{d_wc, fa.weight[0].data(), 8 * (size_t)nc}, {d_wr, fa.weight[1].data(), 8 * (size_t)nr}, {d_ws, fa.weight[2].data(), 8 * (size_t)ns}};
        HIP_TRY(ctx, h2d_row(ctx, in, 3));
        const int64_t rows = (int64_t)nr * ns;
        const int runs = (nc + FC_RUN - 1) / FC_RUN;
        const dim3 grid_c((unsigned)(runs * ((rows + FC_ROWS - 1) / FC_ROWS)));
        {
            PROF(ctx, "k_filter_c");
            if (b) hipLaunchKernelGGL(k_filter_c<5>, grid_c, dim3(256), 0, st, a->dens, b->dens, nc, g.crs_interval[0], rows, runs, fa.taps[0], d_vol, (int64_t)nv);
            else hipLaunchKernelGGL(k_filter_c<2>, grid_c, dim3(256), 0, st, a->dens, (const float *)nullptr, nc, g.crs_interval[0], rows, runs, fa.taps[0], d_vol, (int64_t)nv);
        }
        auto vol = [&](int slot) { return d_vol + (size_t)(slot < 0 ? n_ch : slot) * nv; };
        for (int k = 0; k < n_ch; ++k) filter_line_launch<double>(ctx, g, 1, fa.taps[1], vol(k), vol(k - 1), nullptr, nullptr, nullptr);
        for (int k = n_ch - 1; k >= 0; --k) filter_line_launch<double>(ctx, g, 2, fa.taps[2], vol(k - 1), vol(k), nullptr, nullptr, nullptr);
        LocalFinishArgs p;
        p.a = a->dens; p.b = b ? b->dens : nullptr;
        p.ch = d_vol; p.vol_stride = (int64_t)nv; p.n_vox = a->n_vox;
        p.nc = nc; p.nr = nr;
        p.w_c = d_wc; p.w_r = d_wr; p.w_s = d_ws;
        p.std_floor = std_floor;
        p.mean_a = made[0].dens; p.std_a = made[1].dens; p.z_a = made[2].dens; p.mean_b = made[3].dens; p.std_b = made[4].dens; p.cc = made[5].dens;
        { PROF(ctx, "k_local_finish"); hipLaunchKernelGGL(k_local_finish, dim3(grid_for(a->n_vox, 256, 8192)), dim3(256), 0, st, p); }
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    for (int k = 0; k < 6; ++k)
        if (made[k].m) made[k].publish(want[k]);
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// From a region of a map to a map: the ordered spread of a mask (no reference counterpart; the contract: include/pdbeda.h, the plan: pdbeda_spreadplan.h)
// ------------------------------------------------------------------------------------
// A workgroup may take more dynamic LDS than the 64 KiB a kernel gets unasked: told to the runtime once per kernel and process.
template <bool ROWS>
static hipError_t spread_lds_allowance() {
    static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_spread<ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS_BUDGET);
    return e;
}

// The launch graph: the table (row records and ranks, or packed offsets) and the values in one row of scratch; k_spread<rows or walk> over the tiles into the
// new map and the tiles' count slots; k_spread_fold; the two counts.  One wait.  PDBEDA_SPREAD_ROWS=0 (A/B switch, read at every call): the ordered walk for
// every table.  Equal results to the bit.
extern "C" int pdbeda_map_spread(pdbeda_map *map, float threshold, uint32_t flags, const int32_t *offsets, int64_t n_offsets, const float *values, pdbeda_map *base,
                                 pdbeda_map **out, int64_t counters[3]) {
    if (!map || !offsets || !values || !out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = map->ctx;
    const Geom &g = map->geom;
    int reach[3];
    switch (spread_check(offsets, n_offsets, std::isnan(threshold), flags, PDBEDA_SPREAD_BELOW, g.ncrs, g.crs_interval, reach)) {
    case SPREAD_COUNT: return fail(ctx, PDBEDA_ERR_ARGUMENT, "map spread: %lld offsets are outside 1 .. %d", (long long)n_offsets, PDBEDA_SPREAD_MAX_OFFSETS);
    case SPREAD_REACH: return fail(ctx, PDBEDA_ERR_ARGUMENT, "map spread: an offset reaches beyond +-%d voxels", PDBEDA_SPREAD_MAX_REACH);
    case SPREAD_THRESHOLD: return fail(ctx, PDBEDA_ERR_ARGUMENT, "map spread: the threshold is NaN");
    case SPREAD_FLAG: return fail(ctx, PDBEDA_ERR_ARGUMENT, "map spread: unknown flag 0x%x", flags);
    case SPREAD_AXIS: return fail(ctx, PDBEDA_ERR_ARGUMENT, "map spread: the map is empty, or an axis has 2^30 indices or more");
    default: break;
    }
    if (base)
        if (int rc = same_grid(ctx, g, map->n_vox, base)) return rc;
    std::vector<SpreadRow> rows;
    std::vector<uint16_t> ranks;
    std::vector<uint32_t> packed;
    const bool by_rows = env_unless_0("PDBEDA_SPREAD_ROWS") && spread_compile_rows(offsets, n_offsets, &rows, &ranks);
    if (!by_rows) {
        rows.clear(); ranks.clear();
        packed.resize((size_t)n_offsets);
        for (int64_t t = 0; t < n_offsets; ++t) packed[(size_t)t] = spread_pack(offsets[3 * t], offsets[3 * t + 1], offsets[3 * t + 2]);
    }
    const SpreadPlan plan = plan_spread(g.ncrs, reach, (int)ranks.size());
    if (plan.refusal != SPREAD_OK || plan.lds_total > SP_LDS_BUDGET || map->n_vox <= 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map spread: the map is empty or too large for one launch");
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (plan.lds_total > 64 * 1024) HIP_TRY(ctx, by_rows ? spread_lds_allowance<true>() : spread_lds_allowance<false>());
    MadeMap made;
    if (int rc = made.make_like("map spread", map)) return rc;
    SpreadRow *d_rows = nullptr;
    uint16_t *d_ranks = nullptr;
    uint32_t *d_packed = nullptr, *d_counts = nullptr;
    float *d_values = nullptr;
    int64_t *d_res = nullptr;
    int64_t res[2] = {0, 0};
    const int rc = with_scratch(ctx, "map spread", [&](Carver &cv) {
        cv.take(d_rows, rows.size());
        cv.take(d_ranks, ranks.size());
        cv.take(d_packed, packed.size());
        cv.take(d_values, (size_t)n_offsets + 1);
        cv.take(d_counts, 2 * (size_t)plan.n_tiles);
        cv.take(d_res, 2);
    }, [&]() -> int {
        HIP_TRY(ctx, made.geometry_up());
        const H2DItem in[4] = {{d_rows, rows.data(), sizeof(SpreadRow) * rows.size()}, {d_ranks, ranks.data(), 2 * ranks.size()}, {d_packed, packed.data(), 4 * packed.size()},
                               {d_values, values, 4 * ((size_t)n_offsets + 1)}};
        HIP_TRY(ctx, h2d_row(ctx, in, 4));
        SpreadArgs a;
        memset(&a, 0, sizeof a);
        a.x = map->dens; a.base = base ? base->dens : nullptr; a.out = made.dens;
        a.nc = g.ncrs[0]; a.nr = g.ncrs[1]; a.ns = g.ncrs[2];
        a.ic = g.crs_interval[0]; a.ir = g.crs_interval[1]; a.is = g.crs_interval[2];
        a.threshold = threshold; a.below = (flags & PDBEDA_SPREAD_BELOW) ? 1 : 0;
        a.reach_c = reach[0]; a.reach_r = reach[1]; a.reach_s = reach[2];
        a.tile_r = plan.tile_r; a.tile_s = plan.tile_s; a.words = plan.words; a.box_r = plan.box_r; a.box_s = plan.box_s; a.n_words = plan.n_words;
        a.tiles_c = plan.tiles_c; a.tiles_r = plan.tiles_r;
        a.rows = d_rows; a.n_rows = (int32_t)rows.size(); a.ranks = d_ranks; a.n_ranks = (int32_t)ranks.size();
        a.packed = d_packed; a.n_off = (int32_t)n_offsets; a.values = d_values; a.counts = d_counts;
        {
            PROF(ctx, by_rows ? "k_spread_rows" : "k_spread_walk");
            if (by_rows) hipLaunchKernelGGL(k_spread<true>, dim3((unsigned)plan.n_tiles), dim3(256), (size_t)plan.lds_total, ctx->stream, a);
            else hipLaunchKernelGGL(k_spread<false>, dim3((unsigned)plan.n_tiles), dim3(256), (size_t)plan.lds_total, ctx->stream, a);
        }
        { PROF(ctx, "k_spread_fold"); hipLaunchKernelGGL(k_spread_fold, dim3(1), dim3(256), 0, ctx->stream, d_counts, plan.n_tiles, d_res); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, d2h(ctx, res, d_res, 16));
        return 0;
    });
    if (rc) return rc;
    if (counters) { counters[0] = res[0]; counters[1] = res[1]; counters[2] = by_rows ? 1 : 0; }
    made.publish(out);
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// From a map to a map on ANOTHER grid through coordinate operators (no reference counterpart; the contract: include/pdbeda.h)
// ------------------------------------------------------------------------------------
// PDBEDA_RESAMPLE_STAGE (A/B switch, read at every call so that one process can compare the paths): 0 -- every tap is a direct load; 2 -- the staged
// boxes are not grown, so that lanes at a tile's rim leave them (a test's hook); anything else -- staged boxes.  Equal results to the bit.
static int resample_stage_mode() {
    const char *e = getenv("PDBEDA_RESAMPLE_STAGE");
    return (e && e[0] == '0') ? 0 : ((e && e[0] == '2') ? 2 : 1);
}

// The launch graph: the host's checks; the arenas of the new maps; the operators, the two geometries and the zeroed counters in one row of scratch;
// k_map_resample<order>, a workgroup per destination tile; the rows of counters, which the host adds up.  One wait.  *out and *coverage are written last.
extern "C" int pdbeda_map_resample(pdbeda_map *src, const pdbeda_geometry *dst_geom, const double *ops, int32_t n_ops, int32_t order, uint32_t flags, float fill,
                                   pdbeda_map *base, double alpha, pdbeda_map **out, pdbeda_map **coverage, int64_t counters[4]) {
    if (!src || !dst_geom || !out || !ops) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = src->ctx;
    if (n_ops < 1 || n_ops > PDBEDA_RESAMPLE_MAX_OPS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: n_ops must be 1 .. %d", PDBEDA_RESAMPLE_MAX_OPS);
    if (order != 0 && order != 1 && order != 3) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: order %d is not 0, 1 or 3", order);
    if (flags & ~PDBEDA_RESAMPLE_MEAN) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: unknown flag 0x%x", flags);
    if (!all_finite(ops, 12 * (int64_t)n_ops)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: a non-finite operator entry");
    if (!std::isfinite(alpha)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: alpha is not finite");
    for (int k = 0; k < 3; ++k)
        if (dst_geom->ncrs[k] < 1 || dst_geom->ncrs[k] >= (1 << 30)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: destination axis %d has %d indices (1 .. 2^30 - 1)", k, dst_geom->ncrs[k]);
    Geom gd;
    if (int rc = fill_geom(ctx, dst_geom, &gd)) return rc;
    const int64_t n_vox = (int64_t)gd.ncrs[0] * gd.ncrs[1] * gd.ncrs[2];
    const int tiles_c = (gd.ncrs[0] + RS_C - 1) / RS_C, tiles_r = (gd.ncrs[1] + RS_R - 1) / RS_R, tiles_s = (gd.ncrs[2] + RS_S - 1) / RS_S;
    const int64_t n_tiles = (int64_t)tiles_c * tiles_r * tiles_s;
    if (n_vox >= (1ll << 32) || n_tiles >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: a destination of 2^32 voxels or 2^31 tiles or more");
    if (base)
        if (int rc = same_grid(ctx, gd, n_vox, base, "map resample: base is not of the destination's shape")) return rc;
    // every source grid position the kernel will cast: the map is affine, so its extreme over the destination box (grown by a voxel) sits at a corner
    const Geom &gs = src->geom;
    for (int k = 0; k < n_ops; ++k)
        for (int j = 0; j < 8; ++j) {
            double p[3], x[3], f[3];
            crs2xyz(gd, (j & 1) ? gd.ncrs[0] : -1, (j & 2) ? gd.ncrs[1] : -1, (j & 4) ? gd.ncrs[2] : -1, p);
            resample_apply(ops + 12 * k, p, x);
            bool ok = std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]);
            if (ok) {
                xyz2frac(gs, x, f);
                for (int q = 0; q < 3; ++q) ok = ok && std::fabs(f[q]) < (double)(1ll << 29);
            }
            if (!ok) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map resample: operator %d carries the destination 2^29 grid steps or more from the source map's origin", k);
        }
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MadeMap made, cov;
    if (int rc = made.make(ctx, "map resample", gd, n_vox)) return rc;
    if (coverage)
        if (int rc = cov.make(ctx, "map resample", gd, n_vox)) return rc;
    double *d_ops = nullptr;
    unsigned long long *d_ctr = nullptr;
    std::vector<unsigned long long> seen(4 * (size_t)RS_CTR_SLOTS, 0ull);
    const int stage = resample_stage_mode();
    const int rc = with_scratch(ctx, "map resample", [&](Carver &cv) { cv.take(d_ops, 12 * (size_t)n_ops); cv.take(d_ctr, 4 * (size_t)RS_CTR_SLOTS); }, [&]() -> int {
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, 32 * (size_t)RS_CTR_SLOTS, st));
        HIP_TRY(ctx, made.geometry_up());
        if (cov.m) HIP_TRY(ctx, cov.geometry_up());
        HIP_TRY(ctx, h2d_one(ctx, d_ops, ops, 96 * (size_t)n_ops));
        ResampleArgs a;
        a.src_geom = src->geom_dev; a.src = src->dens; a.dst_geom = made.m->geom_dev;
        a.tiles_c = tiles_c; a.tiles_r = tiles_r;
        a.ops = d_ops; a.n_ops = n_ops;
        a.mean = (flags & PDBEDA_RESAMPLE_MEAN) ? 1 : 0; a.stage = stage;
        a.fill = fill; a.base = base ? base->dens : nullptr; a.alpha = alpha;
        a.out = made.dens; a.coverage = cov.dens; a.counters = d_ctr;
        {
            PROF(ctx, "k_map_resample");
            if (order == 0) hipLaunchKernelGGL(k_map_resample<0>, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
            else if (order == 1) hipLaunchKernelGGL(k_map_resample<1>, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(k_map_resample<3>, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
        }
        HIP_TRY(ctx, hipGetLastError());
        if (counters) HIP_TRY(ctx, d2h(ctx, seen.data(), d_ctr, 32 * (size_t)RS_CTR_SLOTS));
        return 0;
    });
    if (rc) return rc;
    if (counters)
        for (int k = 0; k < 4; ++k) {
            counters[k] = 0;
            for (int slot = 0; slot < RS_CTR_SLOTS; ++slot) counters[k] += (int64_t)seen[4 * (size_t)slot + k];
        }
    made.publish(out);
    if (cov.m) cov.publish(coverage);
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// Reciprocal space: the transform of a resident map and the calls on a resident spectrum (no reference counterpart; the contracts: include/pdbeda.h)
// ------------------------------------------------------------------------------------
struct pdbeda_spectrum {
    pdbeda_ctx *ctx = nullptr;
    Arena arena;                      // the half spectrum: goes back to the context's pool with the handle
    FftCplx *data = nullptr;
    int32_t ncrs[3] = {0, 0, 0};      // of the map it was made from
    int32_t nh = 0;
    int64_t n_coef = 0;
};

// The plan and the device's twiddle table of one line length; the table is made on first use (one upload, one wait) and cached in the context.
static int fft_line_setup(pdbeda_ctx *ctx, int n, FftPlan *plan, const FftCplx **table) {
    if (!pdbeda_fft_plan(n, plan)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "fft: a line of %d is not plannable", n);
    auto it = ctx->fft_tables.find(n);
    if (it == ctx->fft_tables.end()) {
        std::vector<FftCplx> host((size_t)n);
        pdbeda_fft_twiddles(n, host.data());
        Arena a;
        FftCplx *dev = nullptr;
        if (int rc = arena_carve(ctx, "fft table", &a, [&](Carver &cv) { cv.take(dev, (size_t)n); })) return rc;
        hipError_t e = h2d_one(ctx, dev, host.data(), sizeof(FftCplx) * (size_t)n);
        const hipError_t e2 = ctx_sync(ctx);      // (the host's table may be read until here)
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "fft table: %s", hipGetErrorString(e));
        it = ctx->fft_tables.emplace(n, std::move(a)).first;
    }
    *table = reinterpret_cast<const FftCplx *>(it->second.base);
    return 0;
}

// The kernels are instantiated per class of line length (their LDS is static): the smallest class that holds n.
#define FFT_BY_LENGTH(n, LAUNCH)                                                                                         \
    do {                                                                                                                 \
        if ((n) <= 64) { LAUNCH(64); } else if ((n) <= 128) { LAUNCH(128); } else if ((n) <= 256) { LAUNCH(256); }       \
        else if ((n) <= 512) { LAUNCH(512); } else { LAUNCH(1024); }                                                     \
    } while (0)

struct FftAxes {
    FftPlan plan[3];
    const FftCplx *table[3];
};

static void fft_rows_launch(pdbeda_ctx *ctx, const float *in, int64_t rows, const FftAxes &ax, FftCplx *out) {
    PROF(ctx, "k_fft_rows");
    const dim3 grid((unsigned)((rows + FFT_ROWS - 1) / FFT_ROWS));
#define LAUNCH(NMAX) hipLaunchKernelGGL(k_fft_rows<NMAX>, grid, dim3(256), 0, ctx->stream, in, rows, ax.plan[0], ax.table[0], out)
    FFT_BY_LENGTH(ax.plan[0].n, LAUNCH);
#undef LAUNCH
}
static void ifft_rows_launch(pdbeda_ctx *ctx, const FftCplx *in, int64_t rows, const FftAxes &ax, double n_total, float *out) {
    PROF(ctx, "k_ifft_rows");
    const dim3 grid((unsigned)((rows + FFT_ROWS - 1) / FFT_ROWS));
#define LAUNCH(NMAX) hipLaunchKernelGGL(k_ifft_rows<NMAX>, grid, dim3(256), 0, ctx->stream, in, rows, ax.plan[0], ax.table[0], n_total, out)
    FFT_BY_LENGTH(ax.plan[0].n, LAUNCH);
#undef LAUNCH
}
// A pass along r (axis 1) or s (axis 2) of a [ns][nr][nh] volume; in == out runs in place.
static void fft_cols_launch(pdbeda_ctx *ctx, const FftCplx *in, int nh, int nr, int ns, int axis, const FftAxes &ax, int inverse, FftCplx *out) {
    PROF(ctx, axis == 1 ? "k_fft_cols_r" : "k_fft_cols_s");
    const int col_tiles = (nh + FFT_COLS - 1) / FFT_COLS, n_other = axis == 1 ? ns : nr;
    const int64_t stride = axis == 1 ? (int64_t)nh : (int64_t)nh * nr, other_stride = axis == 1 ? (int64_t)nh * nr : (int64_t)nh;
    const dim3 grid((unsigned)((int64_t)col_tiles * n_other));
#define LAUNCH(NMAX) hipLaunchKernelGGL(k_fft_cols<NMAX>, grid, dim3(256), 0, ctx->stream, in, nh, col_tiles, stride, other_stride, ax.plan[axis], ax.table[axis], inverse, out)
    FFT_BY_LENGTH(ax.plan[axis].n, LAUNCH);
#undef LAUNCH
}

// The launch graph: the three tables (made on first use); k_fft_rows from the map into the new spectrum; k_fft_cols along r, then along s, in place.  One wait.
extern "C" int pdbeda_map_fft(pdbeda_map *map, pdbeda_spectrum **out) {
    if (!map || !out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = map->ctx;
    static const char axis_name[3] = {'c', 'r', 's'};
    const Geom &g = map->geom;
    for (int k = 0; k < 3; ++k)
        if (!pdbeda_fft_plannable(g.ncrs[k])) {
            const int next = pdbeda_fft_next(g.ncrs[k]);
            if (next) return fail(ctx, PDBEDA_ERR_ARGUMENT, "map fft: axis %c has %d indices, which is not 2^a 3^b 5^c 7^d; the next plannable length is %d", axis_name[k], g.ncrs[k], next);
            return fail(ctx, PDBEDA_ERR_ARGUMENT, "map fft: axis %c has %d indices, above the longest plannable line of %d; there is no next plannable length", axis_name[k], g.ncrs[k], PDBEDA_FFT_MAX_AXIS);
        }
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2], nh = nc / 2 + 1;
    FftAxes ax;
    for (int k = 0; k < 3; ++k)
        if (int rc = fft_line_setup(ctx, g.ncrs[k], &ax.plan[k], &ax.table[k])) return rc;
    std::unique_ptr<pdbeda_spectrum> sp(new pdbeda_spectrum());
    sp->ctx = ctx;
    sp->ncrs[0] = nc; sp->ncrs[1] = nr; sp->ncrs[2] = ns;
    sp->nh = nh;
    sp->n_coef = (int64_t)nh * nr * ns;
    if (int rc = arena_carve(ctx, "map fft", &sp->arena, [&](Carver &cv) { cv.take(sp->data, (size_t)sp->n_coef); })) return rc;
    fft_rows_launch(ctx, map->dens, (int64_t)nr * ns, ax, sp->data);
    fft_cols_launch(ctx, sp->data, nh, nr, ns, 1, ax, 0, sp->data);
    fft_cols_launch(ctx, sp->data, nh, nr, ns, 2, ax, 0, sp->data);
    hipError_t e = hipGetLastError();
    const hipError_t e2 = ctx_sync(ctx);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(ctx, PDBEDA_ERR_DEVICE, "map fft: %s", hipGetErrorString(e));
    ctx->live_handles++;
    *out = sp.release();
    return PDBEDA_OK;
}

// The launch graph: k_fft_cols along s from the spectrum into the spare volume; along r in place there; k_ifft_rows into the new map.  One wait.
extern "C" int pdbeda_spectrum_inverse(pdbeda_spectrum *spec, pdbeda_map *like, pdbeda_map **out) {
    if (!spec || !like || !out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = spec->ctx;
    if (like->ctx != ctx) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum inverse: the map belongs to another context");
    if (memcmp(like->geom.ncrs, spec->ncrs, sizeof spec->ncrs) != 0)
        return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum inverse: the map is %d x %d x %d, the spectrum was made from %d x %d x %d", like->geom.ncrs[0], like->geom.ncrs[1], like->geom.ncrs[2],
                    spec->ncrs[0], spec->ncrs[1], spec->ncrs[2]);
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int nc = spec->ncrs[0], nr = spec->ncrs[1], ns = spec->ncrs[2], nh = spec->nh;
    FftAxes ax;
    for (int k = 0; k < 3; ++k)
        if (int rc = fft_line_setup(ctx, spec->ncrs[k], &ax.plan[k], &ax.table[k])) return rc;
    MadeMap made;
    if (int rc = made.make_like("spectrum inverse", like)) return rc;
    FftCplx *d_vol = nullptr;
    const int rc = with_scratch(ctx, "spectrum inverse", [&](Carver &cv) { cv.take(d_vol, (size_t)spec->n_coef); }, [&]() -> int {
        HIP_TRY(ctx, made.geometry_up());
        fft_cols_launch(ctx, spec->data, nh, nr, ns, 2, ax, 1, d_vol);
        fft_cols_launch(ctx, d_vol, nh, nr, ns, 1, ax, 1, d_vol);
        ifft_rows_launch(ctx, d_vol, (int64_t)nr * ns, ax, (double)((int64_t)nc * nr * ns), made.dens);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    made.publish(out);
    return PDBEDA_OK;
}

extern "C" int pdbeda_spectrum_shape(pdbeda_spectrum *spec, int32_t ncrs[3]) {
    if (!spec || !ncrs) return PDBEDA_ERR_ARGUMENT;
    memcpy(ncrs, spec->ncrs, sizeof spec->ncrs);
    return PDBEDA_OK;
}

extern "C" int pdbeda_spectrum_download(pdbeda_spectrum *spec, double *out) {
    if (!spec || !out) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = spec->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, d2h(ctx, out, spec->data, sizeof(FftCplx) * (size_t)spec->n_coef));
    HIP_TRY(ctx, ctx_sync(ctx));
    return PDBEDA_OK;
}

extern "C" int pdbeda_spectrum_free(pdbeda_spectrum *spec) {
    if (!spec) return PDBEDA_ERR_ARGUMENT;
    spec->ctx->live_handles--;      // (the arena goes back to the pool in stream order, as a map's)
    delete spec;
    return PDBEDA_OK;
}

static SpectrumShape spectrum_shape_of(const pdbeda_spectrum *spec, const double metric[6]) {
    SpectrumShape sh;
    sh.nc = spec->ncrs[0]; sh.nr = spec->ncrs[1]; sh.ns = spec->ncrs[2]; sh.nh = spec->nh;
    sh.n_coef = spec->n_coef;
    for (int k = 0; k < 6; ++k) sh.m[k] = metric ? metric[k] : 0.0;
    return sh;
}

extern "C" int pdbeda_spectrum_values(pdbeda_spectrum *spec, const int32_t *idx, int64_t n, double *out) {
    if (!spec || n < 0 || (n > 0 && (!idx || !out))) return PDBEDA_ERR_ARGUMENT;
    if (n == 0) return PDBEDA_OK;
    pdbeda_ctx *ctx = spec->ctx;
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Input<int32_t> in{idx, (size_t)(3 * n)};
    Result<double> res{out, (size_t)(2 * n)};
    const SpectrumShape sh = spectrum_shape_of(spec, nullptr);
    return with_scratch(ctx, "spectrum values", [&](Carver &cv) { in.carve(cv); res.carve(cv); }, [&]() -> int {
        HIP_TRY(ctx, in.send(ctx));
        hipLaunchKernelGGL(k_spectrum_values, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, spec->data, sh, in.at, n, res.at(ctx));
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, res.finish(ctx));
        return 0;
    });
}

extern "C" int pdbeda_spectrum_scale(pdbeda_spectrum *spec, const double metric[6], const double *table, int32_t n_table, double s2_max, double beyond) {
    if (!spec) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = spec->ctx;
    if (!metric || !table) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum scale: no metric or no table");
    if (n_table < 2 || n_table > PDBEDA_SPECTRUM_MAX_TABLE) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum scale: a table of %d entries is outside 2 .. %d", n_table, PDBEDA_SPECTRUM_MAX_TABLE);
    if (!all_finite(metric, 6)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum scale: a non-finite metric entry");
    if (!all_finite(table, n_table)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum scale: a non-finite table entry");
    if (!std::isfinite(beyond)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum scale: `beyond` is not finite");
    if (!(std::isfinite(s2_max) && s2_max > 0.0)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum scale: s2_max is not a finite number above 0");
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SpectrumShape sh = spectrum_shape_of(spec, metric);
    const double t_scale = (double)(n_table - 1) / s2_max;
    double *d_table = nullptr;
    return with_scratch(ctx, "spectrum scale", [&](Carver &cv) { cv.take(d_table, (size_t)n_table); }, [&]() -> int {
        HIP_TRY(ctx, h2d_one(ctx, d_table, table, 8 * (size_t)n_table));
        { PROF(ctx, "k_spectrum_scale"); hipLaunchKernelGGL(k_spectrum_scale, dim3(grid_for(sh.n_coef, 256, 4096)), dim3(256), 0, ctx->stream, spec->data, sh, d_table, n_table, t_scale, beyond); }
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    });
}

// The launch graph: the edges in scratch; k_spectrum_shells over a number of workgroups fixed by the shape; k_spectrum_shells_fold; the rows.  One wait.
extern "C" int pdbeda_spectrum_shells(pdbeda_spectrum *a, pdbeda_spectrum *b, const double metric[6], const double *edges, int32_t n_shells, int64_t *count, double *sums) {
    if (!a) return PDBEDA_ERR_ARGUMENT;
    pdbeda_ctx *ctx = a->ctx;
    if (!metric || !edges) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: no metric or no edges");
    if (n_shells < 1 || n_shells > PDBEDA_SPECTRUM_MAX_SHELLS) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: %d shells are outside 1 .. %d", n_shells, PDBEDA_SPECTRUM_MAX_SHELLS);
    if (!all_finite(metric, 6)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: a non-finite metric entry");
    if (!all_finite(edges, (int64_t)n_shells + 1)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: a non-finite edge");
    for (int k = 0; k < n_shells; ++k)
        if (!(edges[k] < edges[k + 1])) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: edge %d does not lie above edge %d", k + 1, k);
    if (b) {
        if (b->ctx != ctx) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: spectra of different contexts");
        if (memcmp(a->ncrs, b->ncrs, sizeof a->ncrs) != 0) return fail(ctx, PDBEDA_ERR_ARGUMENT, "spectrum shells: spectra of different shapes");
    }
    if (ctx->timed_out) return PDBEDA_ERR_TIMEOUT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SpectrumShape sh = spectrum_shape_of(a, metric);
    const int64_t rounds = (sh.n_coef + 255) / 256;
    const unsigned blocks = (unsigned)std::min<int64_t>(rounds, FFT_SHELL_BLOCKS);
    const int64_t chunk = (rounds + blocks - 1) / blocks * 256;
    int parts = 1;      // lanes that share a shell's scan of the 256 staged coefficients
    while (2 * parts * n_shells <= 256) parts *= 2;
    std::vector<double> rows(5 * (size_t)n_shells, 0.0);
    double *d_edges = nullptr, *d_part = nullptr, *d_res = nullptr;
    const int rc = with_scratch(ctx, "spectrum shells", [&](Carver &cv) { cv.take(d_edges, (size_t)n_shells + 1); cv.take(d_part, 5 * (size_t)n_shells * blocks); cv.take(d_res, 5 * (size_t)n_shells); },
                                [&]() -> int {
        HIP_TRY(ctx, h2d_one(ctx, d_edges, edges, 8 * ((size_t)n_shells + 1)));
        { PROF(ctx, "k_spectrum_shells"); hipLaunchKernelGGL(k_spectrum_shells, dim3(blocks), dim3(256), 0, ctx->stream, a->data, b ? b->data : (const FftCplx *)nullptr, sh, d_edges, n_shells, parts, chunk, d_part); }
        { PROF(ctx, "k_spectrum_shells_fold"); hipLaunchKernelGGL(k_spectrum_shells_fold, dim3((unsigned)n_shells), dim3(256), 0, ctx->stream, d_part, (int)blocks, n_shells, d_res); }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, d2h(ctx, rows.data(), d_res, 40 * (size_t)n_shells));
        return 0;
    });
    if (rc) return rc;
    for (int j = 0; j < n_shells; ++j) {
        if (count) count[j] = (int64_t)rows[5 * (size_t)j];
        if (sums) memcpy(sums + 4 * (size_t)j, rows.data() + 5 * (size_t)j + 1, 32);
    }
    return PDBEDA_OK;
}

// ------------------------------------------------------------------------------------
// aggregateCloud (densityAnalysis.py:571-731) behind one call
// ------------------------------------------------------------------------------------
struct pdbeda_cloud : CloudTables {      // (the tables: pdbeda_cloud.h)
    pdbeda_ctx *ctx = nullptr;
};
// A blob list that pdbeda_aggregate_cloud makes for itself: freed when the call returns, however it returns
struct ScopedList {
    pdbeda_bloblist *bl = nullptr;
    ~ScopedList() { if (bl) pdbeda_bloblist_free(bl); }
};

extern "C" int pdbeda_aggregate_cloud(pdbeda_map *m, const pdbeda_cloud_atoms *at, float density_cutoff, double min_cloud_electrons,
                                      pdbeda_cloud **out) {
    if (!m || !at || !out || at->n < 0 || at->n_keys < 0 || at->n_owners < 0) return PDBEDA_ERR_ARGUMENT;
    *out = nullptr;
    pdbeda_ctx *ctx = m->ctx;
    const int64_t n = at->n;
    if (n > 0 && (!at->xyz || !at->radius || !at->weight || !at->residue || !at->alias || !at->key)) return PDBEDA_ERR_ARGUMENT;
    if (at->n_keys > 0 && !at->bonded_off) return PDBEDA_ERR_ARGUMENT;
    if (at->n_owners > 0 && !at->owner_key) return PDBEDA_ERR_ARGUMENT;
    if (n >= (1ll << 31)) return fail(ctx, PDBEDA_ERR_ARGUMENT, "too many atoms");
    for (int64_t i = 0; i < n; ++i) {
        if (at->alias[i] < 0 || at->alias[i] >= n || at->key[i] < 0 || at->key[i] >= at->n_keys || (i > 0 && at->residue[i] < at->residue[i - 1]))
            return fail(ctx, PDBEDA_ERR_ARGUMENT, "atom %lld: alias / key out of range or residues not in order", (long long)i);
    }
    for (int64_t o = 0; o < at->n_owners; ++o)
        if (at->owner_key[o] < 0 || at->owner_key[o] >= at->n_keys) return fail(ctx, PDBEDA_ERR_ARGUMENT, "owner key out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<pdbeda_cloud> res(new pdbeda_cloud());      // (the caller's on success: *out = res.release())
    res->ctx = ctx;
    res->owner_state.assign((size_t)at->n_owners, 0);
    res->totals[3] = NAN;
    if (n == 0) { *out = res.release(); return PDBEDA_OK; }
    hipStream_t st = ctx->stream;
    // PDBEDA_CLOUD_TRACE=1 (experiments): the sizes of the two jobs and the host-side phases of this call on stderr
    static const bool cloud_trace = env_set("PDBEDA_CLOUD_TRACE");
    const double t_call = now_s();
    double t_wait1 = 0.0, t_pooled = 0.0, t_marks[6] = {0, 0, 0, 0, 0, 0};

    // ---- 1. the clouds of every atom: one sphere batch, a group per atom (findAberrantBlobs, 603) ----
    ScopedList clouds_list, uni_list;      // (in this order: the union job's list is freed first, as it is made last)
    pdbeda_bloblist *&clouds = clouds_list.bl, *&uni = uni_list.bl;
    {
        std::vector<int64_t> goff((size_t)n + 1);
        for (int64_t i = 0; i <= n; ++i) goff[(size_t)i] = i;
        int rc = grouped_blobs(m, at->xyz, at->radius, nullptr, n, goff.data(), n, density_cutoff, &clouds);
        if (rc) return rc;
    }
    std::vector<int64_t> c_n;
    std::vector<double> c_tot, c_cen;
    std::vector<int32_t> c_grp;
    int rc = list_stats_one_trip(clouds, 4 * n + 64, c_n, c_tot, c_cen, c_grp);   // (an atom has one to three clouds: the count and the table in one wait)
    if (rc) return rc;
    const int64_t nb = (int64_t)c_n.size();
    t_wait1 = now_s();
    // the voxel lists of the clouds (what the pooled voxels and the overlap tests are gathered from) are made by the device
    // while the host decides what to pool
    rc = list_materialise_voxels(clouds);
    if (rc) return rc;

    t_marks[0] = now_s();
    // ---- 2. host: centroid-distance cut-off, best cloud, pool (604-642), and the residue groups, voxel offsets and bonded pairs of the pool (pdbeda_cloud.h) ----
    CloudPool pool;
    if (cloud_pool(*at, c_n, c_tot, c_cen, c_grp, pool, *res, t_marks + 1) != CLOUD_OK) return fail(ctx, PDBEDA_ERR_ARGUMENT, "bonded key out of range");
    const int64_t n_pool = pool.n_pool();
    if (n_pool == 0) { *out = res.release(); return PDBEDA_OK; }
    t_marks[3] = now_s();

    // ---- 3. device: pooled voxels -> union job (a group per residue + the domain group) ----
    const LabelJob *cj = clouds->job;
    const std::vector<int32_t> &pool_cloud = pool.pool_cloud, &pool_atom = pool.pool_atom, &pool_group = pool.pool_group, &pair_a = pool.pair_a, &pair_b = pool.pair_b;
    const std::vector<int64_t> &pool_voff = pool.pool_voff, &set_off = pool.set_off;
    const int n_rg = (int)pool.group_res.size(), n_groups = n_rg + 1;
    const int64_t V = pool.V(), n_pairs = (int64_t)pair_a.size();

    GroupSetup gs;
    rc = group_alloc(ctx, 2 * V, n_groups, &gs);
    if (rc) return rc;
    // what the device needs of the host's decisions, in ONE copy: pooled clouds, their groups, voxel offsets, the atoms' voxel
    // slices, the bonded pairs and the pairs' (zeroed) touch flags sit in a row in the scratch arena and in one host block
    // (six copies and a fill were seven launches on the stream, 6-8 us apart each: round 4, tools/exp/trace_cloud.sh)
    Arena aux;
    const int64_t np1 = std::max<int64_t>(n_pairs, 1);
    VolDesc *d_union_vols = nullptr;
    int32_t *d_pool_cloud = nullptr, *d_pool_group = nullptr, *d_pa = nullptr, *d_pb = nullptr, *d_comp = nullptr;
    int64_t *d_pool_voff = nullptr, *d_set_off = nullptr;
    unsigned int *d_touch = nullptr;
    size_t upload_bytes = 0;
    rc = arena_carve(ctx, "aggregate cloud", &aux, [&](Carver &cv) {
        cv.take(d_union_vols, n_groups);      // (the union job's volume descriptors ride in the same block: round 5)
        cv.take(d_pool_cloud, n_pool); cv.take(d_pool_group, n_pool);
        cv.take(d_pool_voff, n_pool + 1);
        cv.take(d_set_off, n + 1);
        cv.take(d_pa, np1); cv.take(d_pb, np1);
        cv.take(d_touch, np1);
        upload_bytes = cv.off;      // (the row that is uploaded ends here)
        cv.take(d_comp, 2 * n_pool);
    });
    if (rc) return rc;
    auto fail_dev = [&](hipError_t e) { return fail(ctx, PDBEDA_ERR_DEVICE, "aggregate cloud: %s", hipGetErrorString(e)); };
    // The union job's volumes are made by the HOST (round 5; three launches -- k_init_bounds, k_list_boxes, k_make_vols -- and a
    // wait for their totals before): the voxels of a pooled cloud lie inside its atom's sphere box [C - R - 1, C + R], so the box
    // around the boxes of a residue's pooled atoms -- around all of them for the domain group -- holds the group's voxels.  A
    // volume a little larger than its voxels' own bounds changes nothing in the result: keys are lexicographic in (c, r, s)
    // whatever the box, so the blobs come out in the same order with the same sums.
    std::vector<VolDesc> union_vols((size_t)n_groups);
    SpherePlan union_plan{union_vols.data(), ATOM_WORDS};
    {
        GroupBounds bounds(n_groups);
        const bool have_boxes = (int64_t)cj->host_boxes.size() == n;      // (the sphere job's own boxes, made by the planner: two xyz2crs per pooled cloud were 0.06 ms here)
        int64_t last_a = -1;
        AtomBox bx = {{0, 0, 0}, {-1, -1, -1}};
        for (int64_t p = 0; p < n_pool; ++p) {
            const int64_t a = at->alias[pool_atom[(size_t)p]];          // (the clouds are those of the coordinate's last atom: its coordinate, its radius)
            if (a != last_a) {
                int32_t R[3];
                if (have_boxes) bx = cj->host_boxes[(size_t)a];
                else if (!plan_half_widths(m->geom, at->radius[a], R) || !plan_atom_box(m->geom, at->xyz + 3 * a, R, &bx)) union_plan.plannable = union_plan.fits = false;
                last_a = a;
            }
            bounds.add(bx, pool_group[(size_t)p]);      // (an empty box holds no voxel: it has no cloud, it is not pooled -- unreachable, and ignored)
            bounds.add(bx, n_rg);
        }
        bounds.finish(union_plan);
    }
    t_marks[4] = now_s();
    const bool host_sized = union_plan.fits && !ctx->debug_shrink_totals;   // (what the planner declines, or the debug hook that wants the device's own sizing: the waiting path sizes and reports)
    hipError_t e;
    // The row is written straight into the pinned block when it fits there -- copied by the union job's first launch (k_job_init) --, else into one pageable
    // block that h2d_row has finished reading when it returns.  What no put covers is zero: the pairs' touch flags, and the padding.
    std::vector<char> block;
    {
        StagedRow row{nullptr, aux.base, upload_bytes};      // (upload_bytes is a carve boundary: a multiple of 256, and so is bytes16())
        char *const stage = copy_kernels() && row.bytes16() <= STAGED_ROW_LIMIT ? pinned_take(ctx, row.bytes16()) : nullptr;
        if (stage) memset(stage, 0, upload_bytes);
        else block.assign(upload_bytes, 0);
        row.stage = stage ? stage : block.data();
        row.put(d_pool_cloud, pool_cloud.data(), 4 * (size_t)n_pool);
        row.put(d_pool_group, pool_group.data(), 4 * (size_t)n_pool);
        row.put(d_pool_voff, pool_voff.data(), 8 * (size_t)(n_pool + 1));
        row.put(d_set_off, set_off.data(), 8 * (size_t)(n + 1));
        row.put(d_pa, pair_a.data(), 4 * (size_t)n_pairs);
        row.put(d_pb, pair_b.data(), 4 * (size_t)n_pairs);
        if (host_sized) row.put(d_union_vols, union_vols.data(), sizeof(VolDesc) * (size_t)n_groups);
        if (stage) {
            gs.pend = {stage, aux.base, row.bytes16()};
            e = hipSuccess;
        } else {
            const H2DItem in[1] = {{aux.base, block.data(), upload_bytes}};
            e = h2d_row(ctx, in, 1);
        }
    }
    if (e != hipSuccess) return fail_dev(e);
    PoolPaint paint;
    memset(&paint, 0, sizeof paint);
    paint.src_crs = cj->crs_dev; paint.src_off = cj->offsets_dev;
    paint.pool_cloud = d_pool_cloud; paint.pool_voff = d_pool_voff; paint.pool_group = d_pool_group;
    paint.n_pool = (int)n_pool; paint.domain_group = n_rg; paint.V = V;
    paint.set_off = d_set_off; paint.pair_a = d_pa; paint.pair_b = d_pb; paint.touch = d_touch; paint.n_pairs = (int)n_pairs;
    paint.paint_blocks = grid_for(2 * V, 256, 1ll << 30);
    const bool fused_paint = host_sized && 2 * V <= (1ll << 30) * 256 && n_pairs < (1ll << 30);      // (the device-sized path needs the gathered list for its boxes)
    if (!fused_paint) {
        e = flush_pending(ctx, &gs);      // (these two read the aux block)
        if (e != hipSuccess) return fail_dev(e);
        { PROF(ctx, "k_pool_gather"); hipLaunchKernelGGL(k_pool_gather, dim3(grid_for(2 * V, 256)), dim3(256), 0, st, cj->crs_dev, cj->offsets_dev, d_pool_cloud, d_pool_voff,
                                                         d_pool_group, (int)n_pool, V, n_rg, gs.d_crs, gs.d_item_group); }
        if (n_pairs > 0) { PROF(ctx, "k_test_overlap"); hipLaunchKernelGGL(k_test_overlap, dim3((unsigned)n_pairs), dim3(256), 0, st, cj->crs_dev, d_set_off, d_pa, d_pb, d_touch); }
    }
    if (host_sized) {
        gs.d_vols = d_union_vols;          // (in the aux block, which outlives the job's enqueue)
        rc = group_sized(ctx, &gs, union_plan.words, union_plan.keys, true);
    } else {
        rc = group_bounds(m, &gs, 2 * V, n_groups, false);      // (synchronises)
    }
    if (rc) return rc;
    t_pooled = now_s();
    // The union job's results: rows of its blobs, the row of the component that holds each pooled cloud, the pairs' touch flags.  The
    // host orders the rows by the pooled clouds they hold (below), not by key: the job runs UNORDERED (no k_paint_keys, no k_emit) and its
    // last launch writes the results straight into the pinned block (k_union_finish; four launches -- keys, ranks, components, pack --
    // before).  Without room in the block (or with PDBEDA_COPY_KERNELS=0: kernels do not write host memory then) the ordered form serves.
    const int64_t u_cap = 2 * n_pool + 64;      // (a union component holds at least one pooled cloud, per kind)
    std::vector<int32_t> comp(2 * (size_t)n_pool);
    std::vector<unsigned int> touch((size_t)n_pairs);
    std::vector<int64_t> u_n;
    std::vector<double> u_tot, u_cen;
    std::vector<int32_t> u_grp;
    const size_t fin_bytes = pinned_span(sizeof(Counters)) + pinned_span(8 * (size_t)u_cap) * 2 + pinned_span(24 * (size_t)u_cap) + pinned_span(4 * (size_t)u_cap) +
                             pinned_span(4 * (size_t)np1) + pinned_span(8 * (size_t)n_pool);
    static const bool unordered_on = env_unless_0("PDBEDA_UNORDERED_UNION");      // (A/B switch)
    const bool unordered = unordered_on && fused_paint && copy_kernels() && fin_bytes <= pinned_room(ctx);
    rc = grouped_job(m, gs, 2 * V, n_groups, false, 0.0f, &uni, fused_paint ? &paint : nullptr, unordered);
    if (rc) return rc;
    if (unordered) {
        u_n.resize((size_t)u_cap); u_tot.resize((size_t)u_cap); u_cen.resize(3 * (size_t)u_cap); u_grp.resize((size_t)u_cap);
        Counters u_ctr;
        memset(&u_ctr, 0, sizeof u_ctr);
        UnionFinish fin;
        memset(&fin, 0, sizeof fin);
        fin.src_crs = cj->crs_dev; fin.src_off = cj->offsets_dev; fin.pool_cloud = d_pool_cloud; fin.pool_group = d_pool_group;
        fin.n_pool = (int)n_pool; fin.domain_group = n_rg; fin.touch = d_touch; fin.n_pairs = (int)n_pairs; fin.cap = (unsigned int)u_cap;
        // (the takes fin_bytes made room for; as before a failed launch below keeps them until the next wait and, through fail(), delivers nothing)
        fin.out_ctr = reinterpret_cast<Counters *>(pinned_take(ctx, sizeof u_ctr, &u_ctr));
        fin.out_n = reinterpret_cast<long long *>(pinned_take(ctx, 8 * (size_t)u_cap, u_n.data()));
        fin.out_total = reinterpret_cast<double *>(pinned_take(ctx, 8 * (size_t)u_cap, u_tot.data()));
        fin.out_centroid = reinterpret_cast<double *>(pinned_take(ctx, 24 * (size_t)u_cap, u_cen.data()));
        fin.out_group = reinterpret_cast<int32_t *>(pinned_take(ctx, 4 * (size_t)u_cap, u_grp.data()));
        fin.out_touch = reinterpret_cast<unsigned int *>(pinned_take(ctx, 4 * (size_t)np1, n_pairs ? touch.data() : nullptr));      // (no pair: a line of its own all the same, nothing delivered)
        fin.out_comp = reinterpret_cast<int32_t *>(pinned_take(ctx, 8 * (size_t)n_pool, comp.data()));
        const int64_t fin_threads = std::max<int64_t>(std::max<int64_t>(uni->job->job.run_cap, 2 * n_pool), n_pairs);
        { PROF(ctx, "k_union_finish"); hipLaunchKernelGGL(k_union_finish, dim3(grid_for(fin_threads, 256, 1024)), dim3(256), 0, st, uni->job->job, m->geom_dev, fin); }
        e = hipGetLastError();
        if (e != hipSuccess) return fail_dev(e);
        e = ctx_sync(ctx);      // (the one wait of the union job: everything above lands in the host's arrays)
        if (e != hipSuccess) return fail(ctx, ctx->timed_out ? PDBEDA_ERR_TIMEOUT : PDBEDA_ERR_DEVICE, "aggregate cloud: %s", ctx->timed_out ? ctx->err.c_str() : hipGetErrorString(e));
        if (u_ctr.unit_wait_failed) return fail(ctx, PDBEDA_ERR_DEVICE, "aggregate cloud: a pooled voxel lies outside its group's volume");
        if ((int64_t)u_ctr.n_blobs > u_cap) return fail(ctx, PDBEDA_ERR_STATE, "aggregate cloud: more union components than pooled clouds");
        const size_t nb_u = u_ctr.n_blobs;
        u_n.resize(nb_u); u_tot.resize(nb_u); u_cen.resize(3 * nb_u); u_grp.resize(nb_u);
    } else {
        { PROF(ctx, "k_pool_component"); hipLaunchKernelGGL(k_pool_component, dim3(grid_for(2 * n_pool, 256)), dim3(256), 0, st, uni->job->job, cj->crs_dev, cj->offsets_dev, d_pool_cloud,
                                                            d_pool_group, (int)n_pool, n_rg, d_comp); }
        e = hipGetLastError();
        if (e != hipSuccess) return fail_dev(e);
        // (the pairs' touch flags and the pooled clouds' components are neighbours in the aux arena: one copy brings both)
        const size_t tail_bytes = (size_t)((char *)(d_comp + 2 * n_pool) - (char *)d_touch);
        std::vector<char> tail((tail_bytes + 3) & ~(size_t)3);
        const D2HItem tail_item = {tail.data(), d_touch, tail.size()};      // (whole words: the pack kernel copies words; the carve's padding covers the round-up)
        rc = list_stats_one_trip(uni, u_cap, u_n, u_tot, u_cen, u_grp, &tail_item);   // (synchronises: comp / touch land with the statistics)
        if (rc) return rc;
        if (n_pairs > 0) memcpy(touch.data(), tail.data(), 4 * (size_t)n_pairs);
        memcpy(comp.data(), tail.data() + ((char *)d_comp - (char *)d_touch), 8 * (size_t)n_pool);
    }
    const int64_t nu = (int64_t)u_n.size();
    if (cloud_trace)
        fprintf(stderr, "aggregate_cloud: %lld atoms, %lld clouds, %lld pooled clouds (%lld voxels), %d residue groups + the domain group: %lld mask words, %lld keys, %lld union blobs; "
                        "ms: clouds enqueued + waited %.3f, host pooling %.3f (voxel lists enqueued %.3f, distances + cut-off %.3f, pool loop %.3f, groups + pairs %.3f, arenas + volumes %.3f, block + staging %.3f), union job enqueued + waited %.3f\n",
                (long long)n, (long long)nb, (long long)n_pool, (long long)V, n_rg, (long long)union_plan.words, (long long)union_plan.keys, (long long)nu,
                1e3 * (t_wait1 - t_call), 1e3 * (t_pooled - t_wait1), 1e3 * (t_marks[0] - t_wait1), 1e3 * (t_marks[1] - t_marks[0]), 1e3 * (t_marks[2] - t_marks[1]),
                1e3 * (t_marks[3] - t_marks[2]), 1e3 * (t_marks[4] - t_marks[3]), 1e3 * (t_pooled - t_marks[4]), 1e3 * (now_s() - t_pooled));

    // ---- 4. host: overlap completeness, electrons per union component, emission order, totals (652-731: pdbeda_cloud.h) ----
    if (cloud_finish(*at, pool, u_n, u_tot, u_cen, u_grp, comp, touch, min_cloud_electrons, *res) != CLOUD_OK)
        return fail(ctx, PDBEDA_ERR_STATE, "aggregate cloud: component rank out of range");
    *out = res.release();
    return PDBEDA_OK;
}

extern "C" int pdbeda_cloud_counts(pdbeda_cloud *c, int64_t counts[4], double totals[4]) {
    if (!c) return PDBEDA_ERR_ARGUMENT;
    if (counts) { counts[0] = (int64_t)c->atom_idx.size(); counts[1] = (int64_t)c->res_rows.size(); counts[2] = (int64_t)c->dom_rows.size(); counts[3] = (int64_t)c->owner_state.size(); }
    if (totals) for (int k = 0; k < 4; ++k) totals[k] = c->totals[k];
    return PDBEDA_OK;
}

extern "C" int pdbeda_cloud_atom_rows(pdbeda_cloud *c, int32_t *atom, double *total_density, int64_t *n_voxels, double *centroid, double *distance) {
    if (!c) return PDBEDA_ERR_ARGUMENT;
    const size_t n = c->atom_idx.size();
    if (atom) memcpy(atom, c->atom_idx.data(), 4 * n);
    if (total_density) memcpy(total_density, c->atom_total.data(), 8 * n);
    if (n_voxels) memcpy(n_voxels, c->atom_nvox.data(), 8 * n);
    if (centroid) memcpy(centroid, c->atom_centroid.data(), 24 * n);
    if (distance) memcpy(distance, c->atom_dist.data(), 8 * n);
    return PDBEDA_OK;
}

static int cloud_rows_out(const std::vector<CloudRow> &rows, int32_t *residue, double *total_density, int64_t *n_voxels, double *electrons, double *centroid) {
    for (size_t i = 0; i < rows.size(); ++i) {
        if (residue) residue[i] = rows[i].residue;
        if (total_density) total_density[i] = rows[i].total;
        if (n_voxels) n_voxels[i] = rows[i].n;
        if (electrons) electrons[i] = rows[i].electrons;
        if (centroid) for (int q = 0; q < 3; ++q) centroid[3 * i + q] = rows[i].cen[q];
    }
    return PDBEDA_OK;
}
extern "C" int pdbeda_cloud_residue_rows(pdbeda_cloud *c, int32_t *residue, double *total_density, int64_t *n_voxels, double *electrons, double *centroid) {
    if (!c) return PDBEDA_ERR_ARGUMENT;
    return cloud_rows_out(c->res_rows, residue, total_density, n_voxels, electrons, centroid);
}
extern "C" int pdbeda_cloud_domain_rows(pdbeda_cloud *c, int32_t *residue, double *total_density, int64_t *n_voxels, double *electrons, double *centroid) {
    if (!c) return PDBEDA_ERR_ARGUMENT;
    return cloud_rows_out(c->dom_rows, residue, total_density, n_voxels, electrons, centroid);
}
extern "C" int pdbeda_cloud_owner_states(pdbeda_cloud *c, uint8_t *state) {
    if (!c || (!state && !c->owner_state.empty())) return PDBEDA_ERR_ARGUMENT;
    if (!c->owner_state.empty()) memcpy(state, c->owner_state.data(), c->owner_state.size());
    return PDBEDA_OK;
}
extern "C" int pdbeda_cloud_free(pdbeda_cloud *c) {
    if (!c) return PDBEDA_ERR_ARGUMENT;
    delete c;
    return PDBEDA_OK;
}
