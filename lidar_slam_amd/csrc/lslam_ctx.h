// Host side, part 1 (included by lidarslam.hip after the kernels): the context -- streams, events,
// timers, grow-only device buffers -- its create / destroy, and the small ABI utilities (version,
// errors, memory, copies, timers, parameter defaults).  The launchers are in lslam_launch.h and lslam_launch_map.h.
#pragma once
#include "lslam_hazards.h"

constexpr int LSLAM_EV_RING = 64;
constexpr int NSLOTS = 2;  // producer slots in the ring

static thread_local std::string g_err;

static size_t default_steps_budget() { return (size_t)2 << 30; }  // lslam_set_steps_budget

// lslam_set_reloc_budget: the score volume of a 4096-robot map match at its defaults, or the environment's
static size_t default_reloc_budget() {
    if (const char *e = getenv("LSLAM_RELOC_BUDGET")) {
        const long long v = atoll(e);
        if (v > 0) return (size_t)v;
    }
    return (size_t)4096 * 41 * 21 * 21 * 4;
}

static int set_err(int code, const char *msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            g_err = std::string(#expr) + ": " + hipGetErrorString(_e);                \
            return LSLAM_ERR_HIP;                                                     \
        }                                                                             \
    } while (0)

// A grow-only device buffer of the context.  Growing frees the old allocation, which work in
// flight may still use.  The rule: a grow first synchronises all four streams of the context,
// whichever of them use the buffer (it happens only when a shape first grows).  A failed grow
// leaves the buffer empty.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    template <typename T>
    T *as() const { return (T *)p; }
    hipError_t release() {
        void *q = p;
        p = nullptr;
        bytes = 0;
        return q ? hipFree(q) : hipSuccess;
    }
    static bool fits(const DevBuf *b, int n, size_t need) {
        for (int i = 0; i < n; i++)
            if (b[i].bytes < need) return false;
        return true;
    }
    // b[0..n) grow as a group: all are freed before any is allocated
    static int ensure(lslam_ctx *c, DevBuf *b, int n, size_t need, const char *what);
    int ensure(lslam_ctx *c, size_t need, const char *what) { return ensure(c, this, 1, need, what); }
};

struct lslam_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    // per kernel id: a ring of (start, stop) event pairs harvested lazily, so
    // timing never blocks the host between back-to-back launches
    hipEvent_t ev0[LSLAM_K_COUNT][LSLAM_EV_RING] = {}, ev1[LSLAM_K_COUNT][LSLAM_EV_RING] = {};
    int head[LSLAM_K_COUNT] = {}, npend[LSLAM_K_COUNT] = {};
    double total_ms[LSLAM_K_COUNT] = {};
    int64_t launches[LSLAM_K_COUNT] = {};
    DevBuf scr;   // main-stream scratch: resolved draws (when the caller gives no draws_out)
    DevBuf escr;  // express-scan revolution builder scratch (per-packet flags/ranks, per-revolution info)
    DevBuf cscr;  // large-chunk consensus scratch: per-trial counts (+ Philox draws)
    DevBuf mscr;  // score volume of a scan-match or scan-to-map call (when the caller gives no scores)
    DevBuf rscr;  // relocalisation: a chunk's coarse volume (when the caller gives no coarse_scores) and peak keys
    size_t reloc_budget = default_reloc_budget();  // bytes of coarse volume per chunk (lslam_set_reloc_budget)
    int resolve_beside = 0;  // this call's resolves will likely run beside the next call's producer
    int n_cus = 1;           // compute units of the device
    uint32_t timing_mask = 0xffffffffu;  // kernel ids timed when timing is on (lslam_set_timing_mask)
    // reject tables of the table-mode parser, K = 2..127 (lslam_rng_pipe.h)
    uint32_t *rt_all = nullptr;
    // seed_kernel -> rng_kernel: initial MT states [n_scans][624].  [0], [1]: the pipeline's, by
    // call parity, seeded on sstream ahead of their producers (seed_beside); [2]: producers on the
    // ctx stream (lslam_hyp_mt19937), seeded in stream order
    DevBuf seedst[3];
    hipStream_t sstream = nullptr;
    hipEvent_t ev_seeded[2] = {};     // on sstream, after seed_kernel into seedst[i]
    hipEvent_t ev_seed_read[2] = {};  // on pstream, after the producer that read seedst[i]
    int seed_next = 0;                // the pipeline's next seed buffer
    // cut_lane_kernel -> chunk_kernel: [n_chunks] ChunkCut, a ring of four by seeded call: the
    // buffer of call n is written after the producer of seeded call n - 2 (ev_seed_read), which
    // waited for its slot, released by the fix-up of the mt call two before it -- after the
    // consensus of seeded call n - 4, the buffer's previous reader
    DevBuf cutb[4];
    int cut_next = 0;
    size_t steps_budget = default_steps_budget();  // producer slot budget (prepare_steps)
    // The MT producer of call k+1 runs on its own stream while call k's
    // consumers finish on `stream`: two producer slots (Fisher-Yates steps +
    // end-of-scan MT state), each released by an event once its consumers ran.
    // (Measured and dropped at r04: a third slot, 0.79-0.86 vs 0.76 ms per C3 step; the resolve
    // on a stream of its own after its producer, 0.871 vs 0.763 ms.)
    hipStream_t pstream = nullptr;
    DevBuf pslot[NSLOTS];  // (one size: they grow together)
    int next_slot = 0;
    hipEvent_t ev_slot_free[NSLOTS] = {};  // on stream, after the slot's resolve + fix-up
    hipEvent_t ev_produced = nullptr;      // on pstream, after rng_kernel
    hipEvent_t ev_copy = nullptr;          // on stream, after the latest lslam_h2d / lslam_memset
    hipEvent_t ev_call = nullptr;          // on stream, at the end of the latest pipeline call
    // A UKF step that does not read the call's RANSAC results runs on its own
    // stream beside the RANSAC chain; the main stream joins it before ev_call.
    hipStream_t ustream = nullptr;
    hipEvent_t ev_ukf = nullptr;  // on ustream, after the side UKF
    // what the producer's waits are decided from (lslam_hazards.h); hz.prev_state_out is complete
    // once ev_slot_free[prev_slot] fired
    HazardState hz;
    int prev_slot = 0;
    DevBuf spec_dirty[2];  // [n_scans] replayed-by-fix-up flags, by call parity (they grow together)
    int spec_cur = 0;      // the buffer the latest fix-up wrote
};

int DevBuf::ensure(lslam_ctx *c, DevBuf *b, int n, size_t need, const char *what) {
    if (fits(b, n, need)) return LSLAM_OK;
    for (hipStream_t s : {c->stream, c->pstream, c->ustream, c->sstream}) HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < n; i++) HIPCHK(b[i].release());
    for (int i = 0; i < n; i++) {
        const hipError_t e = hipMalloc(&b[i].p, need);
        if (e == hipErrorOutOfMemory) {
            g_err = std::string("hipMalloc: out of memory (") + what + ")";
            return LSLAM_ERR_NOMEM;
        }
        HIPCHK(e);
        b[i].bytes = need;
    }
    return LSLAM_OK;
}

// rows v = 0..127 of every K = 2..127, built once per process (rt_word, lslam_rng_pipe.h)
static const std::vector<uint32_t> &reject_tables() {
    static const std::vector<uint32_t> t = [] {
        std::vector<uint32_t> v((size_t)(RT_KMAX - 1) * RT_DWORDS);
        for (uint32_t K = 2; K <= RT_KMAX; K++)
            for (uint32_t r = 0; r < (uint32_t)RT_ROWS; r++)
                for (uint32_t q = 0; q < (uint32_t)RT_ST; q++)
                    v[(size_t)(K - 2) * RT_DWORDS + r * RT_ST + q] = rt_word(K, r, q);
        return v;
    }();
    return t;
}

// streams, events and the reject tables of a new context; on a failure lslam_ctx_create
// destroys whatever exists by then
static int ctx_init(lslam_ctx *c, int device) {
    c->device = device;
    HIPCHK(hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, device));
    if (c->n_cus < 1) c->n_cus = 1;
    if (const char *e = getenv("LSLAM_MT_SPECULATE")) c->hz.speculate = atoi(e) != 0;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (int k = 0; k < LSLAM_K_COUNT; k++)
        for (int r = 0; r < LSLAM_EV_RING; r++) {
            HIPCHK(hipEventCreate(&c->ev0[k][r]));
            HIPCHK(hipEventCreate(&c->ev1[k][r]));
        }
    // the producer's chains are the critical path: its stream gets the highest
    // priority so that its workgroups are dispatched ahead of the previous call's
    // consumers (resolve / consensus / post) that run beside it
    {
        int lo_pri = 0, hi_pri = 0;
        if (hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri) != hipSuccess) hi_pri = 0;
        HIPCHK(hipStreamCreateWithPriority(&c->pstream, hipStreamNonBlocking, hi_pri));
    }
    HIPCHK(hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipEventCreateWithFlags(&c->ev_seeded[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->ev_seed_read[i], hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_seed_read[i], c->stream));
    }
    for (int i = 0; i < NSLOTS; i++) HIPCHK(hipEventCreateWithFlags(&c->ev_slot_free[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_produced, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&c->ustream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_ukf, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_call, hipEventDisableTiming));
    for (int i = 0; i < NSLOTS; i++) HIPCHK(hipEventRecord(c->ev_slot_free[i], c->stream));
    HIPCHK(hipEventRecord(c->ev_copy, c->stream));
    HIPCHK(hipEventRecord(c->ev_call, c->stream));
    const std::vector<uint32_t> &t = reject_tables();
    HIPCHK(hipMalloc(&c->rt_all, t.size() * 4));
    HIPCHK(hipMemcpy(c->rt_all, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    return LSLAM_OK;
}

extern "C" {

#define LSLAM_STR_(x) #x
#define LSLAM_STR(x) LSLAM_STR_(x)
#ifndef LSLAM_SRC_HASH
#define LSLAM_SRC_HASH "0000000000000000"  // lidar_slam_amd/build.py passes the sources' sha256 prefix
#endif
const char *lslam_version(void) {
    return "lidarslam-mi355x 0.3.0 (abi " LSLAM_STR(LSLAM_ABI_VERSION) ", src " LSLAM_SRC_HASH ", gfx950)";
}

const char *lslam_status_string(int st) {
    switch (st) {
        case LSLAM_OK: return "ok";
        case LSLAM_ERR_ARG: return "invalid argument";
        case LSLAM_ERR_HIP: return "HIP runtime error";
        case LSLAM_ERR_NOMEM: return "out of memory";
        case LSLAM_ERR_CAPACITY: return "capacity exceeded";
        case LSLAM_ERR_UNSUPPORTED: return "unsupported";
        default: return "unknown status";
    }
}

const char *lslam_last_error(void) { return g_err.c_str(); }

int lslam_device_count(int *n) {
    if (!n) return LSLAM_ERR_ARG;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    *n = c;
    return LSLAM_OK;
}

int lslam_ctx_create(int device, lslam_ctx **out) {
    if (!out) return LSLAM_ERR_ARG;
    *out = nullptr;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_err(LSLAM_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    lslam_ctx *c = new (std::nothrow) lslam_ctx();
    if (!c) return LSLAM_ERR_NOMEM;
    const int st = ctx_init(c, device);
    if (st) {
        lslam_ctx_destroy(c);  // (leaves g_err as ctx_init set it)
        return st;
    }
    *out = c;
    return LSLAM_OK;
}

// safe on a partially built context (lslam_ctx_create's failure path): every handle may be null
int lslam_ctx_destroy(lslam_ctx *c) {
    if (!c) return LSLAM_OK;
    (void)hipSetDevice(c->device);
    hipStream_t streams[4] = {c->stream, c->pstream, c->ustream, c->sstream};
    for (hipStream_t s : streams)
        if (s) (void)hipStreamSynchronize(s);
    for (int k = 0; k < LSLAM_K_COUNT; k++)
        for (int r = 0; r < LSLAM_EV_RING; r++) {
            if (c->ev0[k][r]) (void)hipEventDestroy(c->ev0[k][r]);
            if (c->ev1[k][r]) (void)hipEventDestroy(c->ev1[k][r]);
        }
    for (DevBuf *b : {&c->scr, &c->escr, &c->cscr, &c->mscr, &c->rscr}) (void)b->release();
    for (DevBuf &b : c->seedst) (void)b.release();
    for (DevBuf &b : c->cutb) (void)b.release();
    for (DevBuf &b : c->pslot) (void)b.release();
    for (DevBuf &b : c->spec_dirty) (void)b.release();
    if (c->rt_all) (void)hipFree(c->rt_all);
    hipEvent_t evs[10] = {c->ev_seeded[0], c->ev_seeded[1], c->ev_seed_read[0], c->ev_seed_read[1], c->ev_slot_free[0],
                          c->ev_slot_free[1], c->ev_produced, c->ev_copy, c->ev_call, c->ev_ukf};
    for (hipEvent_t e : evs)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : streams)
        if (s) (void)hipStreamDestroy(s);
    delete c;
    return LSLAM_OK;
}

int lslam_sync(lslam_ctx *c) {
    if (!c) return LSLAM_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->pstream));
    HIPCHK(hipStreamSynchronize(c->ustream));
    HIPCHK(hipStreamSynchronize(c->sstream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LSLAM_OK;
}

int lslam_malloc(lslam_ctx *c, size_t bytes, void **p) {
    if (!c || !p) return LSLAM_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) return set_err(LSLAM_ERR_NOMEM, "hipMalloc: out of memory");
    HIPCHK(e);
    return LSLAM_OK;
}

int lslam_free(lslam_ctx *c, void *p) {
    if (!c) return LSLAM_ERR_ARG;
    if (!p) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipFree(p));
    return LSLAM_OK;
}

int lslam_host_alloc(size_t bytes, void **p) {
    if (!p) return LSLAM_ERR_ARG;
    HIPCHK(hipHostMalloc(p, bytes ? bytes : 16, hipHostMallocDefault));
    return LSLAM_OK;
}

int lslam_host_free(void *p) {
    if (p) HIPCHK(hipHostFree(p));
    return LSLAM_OK;
}

int lslam_h2d(lslam_ctx *c, void *dst, const void *src, size_t n) {
    if (!c || (!dst && n) || (!src && n)) return LSLAM_ERR_ARG;
    if (!n) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    // (the previous calls, which may still read dst, are ahead of this on the ctx stream)
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_copy, c->stream));
    c->hz.copies.add(dst, n);
    return LSLAM_OK;
}

int lslam_d2h(lslam_ctx *c, void *dst, const void *src, size_t n) {
    if (!c || (!dst && n) || (!src && n)) return LSLAM_ERR_ARG;
    if (!n) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    // (the previous calls, which may still read dst, are ahead of this on the ctx stream)
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream));
    return LSLAM_OK;
}

int lslam_d2d(lslam_ctx *c, void *dst, const void *src, size_t n) {
    if (!c || (!dst && n) || (!src && n)) return LSLAM_ERR_ARG;
    if (!n) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    // (the previous calls, which may still read dst, are ahead of this on the ctx stream)
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_copy, c->stream));
    c->hz.copies.add(dst, n);
    return LSLAM_OK;
}

int lslam_host_register(void *p, size_t n) {
    if (!p || !n) return LSLAM_ERR_ARG;
    const hipError_t e = hipHostRegister(p, n, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // not sticky: the caller falls back to pageable copies
        return set_err(LSLAM_ERR_HIP, hipGetErrorString(e));
    }
    return LSLAM_OK;
}

int lslam_host_unregister(void *p) {
    if (!p) return LSLAM_ERR_ARG;
    HIPCHK(hipHostUnregister(p));
    return LSLAM_OK;
}

int lslam_ctx_stream(lslam_ctx *c, void **stream) {
    if (!c || !stream) return LSLAM_ERR_ARG;
    *stream = (void *)c->stream;
    return LSLAM_OK;
}

int lslam_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[9] = {(int64_t)sizeof(lslam_chunk_model), (int64_t)sizeof(lslam_landmark),
                          (int64_t)sizeof(lslam_ransac_params), (int64_t)sizeof(lslam_ukf_params),
                          (int64_t)sizeof(lslam_scan_batch), (int64_t)sizeof(lslam_express_measures),
                          (int64_t)sizeof(lslam_express_revs), (int64_t)sizeof(lslam_match_params),
                          (int64_t)sizeof(lslam_match_batch)};
    for (int i = 0; i < n && i < 9 && sizes; i++) sizes[i] = s[i];
    return 9;
}

int lslam_grid_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_grid_params), (int64_t)sizeof(lslam_grid_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_mapmatch_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_mapmatch_params), (int64_t)sizeof(lslam_mapmatch_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_mapfuse_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_mapfuse_params), (int64_t)sizeof(lslam_mapfuse_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_reloc_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_reloc_params), (int64_t)sizeof(lslam_reloc_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_raycast_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_raycast_params), (int64_t)sizeof(lslam_raycast_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_recentre_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_recentre_params), (int64_t)sizeof(lslam_recentre_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_dist_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[4] = {(int64_t)sizeof(lslam_dist_params), (int64_t)sizeof(lslam_dist_batch),
                          (int64_t)sizeof(lslam_fieldscore_params), (int64_t)sizeof(lslam_fieldscore_batch)};
    for (int i = 0; i < n && i < 4 && sizes; i++) sizes[i] = s[i];
    return 4;
}

int lslam_fieldalign_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_fieldalign_params), (int64_t)sizeof(lslam_fieldalign_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_fieldfuse_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_fieldfuse_params), (int64_t)sizeof(lslam_fieldfuse_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_relocprior_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_relocprior_params), (int64_t)sizeof(lslam_relocprior_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_page_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_page_params), (int64_t)sizeof(lslam_page_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_gridmerge_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_gridmerge_params), (int64_t)sizeof(lslam_gridmerge_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_gridpoints_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_gridpoints_params), (int64_t)sizeof(lslam_gridpoints_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_posegraph_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_posegraph_params), (int64_t)sizeof(lslam_posegraph_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_posegate_abi_sizes(int64_t *sizes, int n) {
    const int64_t s[2] = {(int64_t)sizeof(lslam_posegate_params), (int64_t)sizeof(lslam_posegate_batch)};
    for (int i = 0; i < n && i < 2 && sizes; i++) sizes[i] = s[i];
    return 2;
}

int lslam_memset(lslam_ctx *c, void *dst, int v, size_t n) {
    if (!c || (!dst && n)) return LSLAM_ERR_ARG;
    if (!n) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    // (the previous calls, which may still read dst, are ahead of this on the ctx stream)
    HIPCHK(hipMemsetAsync(dst, v, n, c->stream));
    HIPCHK(hipEventRecord(c->ev_copy, c->stream));
    c->hz.copies.add(dst, n);
    return LSLAM_OK;
}

// fold the oldest `keep_free` pending event pairs (all of them if < 0) into the totals
static int harvest(lslam_ctx *c, int k, int upto_free = -1) {
    while (c->npend[k] > 0 && (upto_free < 0 || LSLAM_EV_RING - c->npend[k] < upto_free)) {
        const int r = (c->head[k] - c->npend[k] + LSLAM_EV_RING) % LSLAM_EV_RING;
        HIPCHK(hipEventSynchronize(c->ev1[k][r]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0[k][r], c->ev1[k][r]));
        c->total_ms[k] += ms;
        c->launches[k] += 1;
        c->npend[k] -= 1;
    }
    return LSLAM_OK;
}

static int timer_begin(lslam_ctx *c, int k, hipStream_t st_ = nullptr) {
    if (!c->timing || !((c->timing_mask >> k) & 1u)) return LSLAM_OK;
    int st = harvest(c, k, 1);
    if (st) return st;
    HIPCHK(hipEventRecord(c->ev0[k][c->head[k]], st_ ? st_ : c->stream));
    return LSLAM_OK;
}

static int timer_end(lslam_ctx *c, int k, hipStream_t st_ = nullptr) {
    if (!c->timing || !((c->timing_mask >> k) & 1u)) return LSLAM_OK;
    HIPCHK(hipEventRecord(c->ev1[k][c->head[k]], st_ ? st_ : c->stream));
    c->head[k] = (c->head[k] + 1) % LSLAM_EV_RING;
    c->npend[k] += 1;
    return LSLAM_OK;
}

int lslam_set_timing(lslam_ctx *c, int en) {
    if (!c) return LSLAM_ERR_ARG;
    c->timing = en != 0;
    return LSLAM_OK;
}

int lslam_set_timing_mask(lslam_ctx *c, uint32_t mask) {
    if (!c) return LSLAM_ERR_ARG;
    c->timing_mask = mask;
    return LSLAM_OK;
}

int lslam_timing(lslam_ctx *c, int k, double *ms, int64_t *n) {
    if (!c || k < 0 || k >= LSLAM_K_COUNT) return LSLAM_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    int st = harvest(c, k);
    if (st) return st;
    if (ms) *ms = c->total_ms[k];
    if (n) *n = c->launches[k];
    return LSLAM_OK;
}

int lslam_timing_reset(lslam_ctx *c) {
    if (!c) return LSLAM_ERR_ARG;
    for (int k = 0; k < LSLAM_K_COUNT; k++) {
        int st = harvest(c, k);
        if (st) return st;
        c->total_ms[k] = 0;
        c->launches[k] = 0;
    }
    return LSLAM_OK;
}

int lslam_ransac_params_default(lslam_ransac_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->residual_threshold = 20.0;  // ransac_functions.py:9
    p->max_trials = 100;           // :10
    p->min_samples = 2;            // :11
    p->hyp_source = LSLAM_HYP_MT19937;
    p->life = 40;                  // landmarking.py:3
    p->tol_a = 0.1;                // :4
    p->tol_b = 10.0;               // :5
    p->tol_dist = 100.0;           // :6
    p->philox_seed = 0x5eed5eedull;
    return LSLAM_OK;
}

int lslam_ukf_params_default(lslam_ukf_params *p, int32_t L) {
    if (!p || L < 0) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->n_landmarks = L;
    p->flags = LSLAM_UKF_PREDICT | LSLAM_UKF_UPDATE;
    p->dt = 0.005;          // systemClass.py:10
    p->wheel_radius = 50;   // UKFMethods.py:6
    p->wheel_base = 200;    // UKFMethods.py:7
    p->alpha = 1e-4;        // systemClass.py:20
    p->beta = 2.0;
    p->kappa = 0.0;
    for (int i = 0; i < 9; i++) p->Q[i] = (i % 4 == 0) ? 0.001 : 0.0;  // systemClass.py:29
    return LSLAM_OK;
}

int lslam_match_params_default(lslam_match_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->cell = 20.0;                  // mm: a 512-cell grid spans +-5.12 m
    p->theta_step = LS_PI / 360.0;   // half a degree
    p->grid_w = 512;
    p->smear = 2;
    p->k_trans = 10;                 // +-200 mm
    p->k_theta = 20;                 // +-10 degrees
    return LSLAM_OK;
}

int lslam_grid_params_default(lslam_grid_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->cell = 20.0;         // mm: a 512-cell grid spans 10.24 m
    p->max_range = 8000.0;  // mm
    p->grid_w = 512;
    p->l_hit = 85;          // ln(0.7 / 0.3), 0.01 nat
    p->l_miss = -41;        // ln(0.4 / 0.6)
    p->l_min = -200;        // p ~ 0.12
    p->l_max = 350;         // p ~ 0.97
    return LSLAM_OK;
}

int lslam_mapmatch_params_default(lslam_mapmatch_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->theta_step = LS_PI / 360.0;  // half a degree
    p->win_w = 512;
    p->smear = 2;
    p->k_trans = 10;        // +-200 mm at 20 mm cells
    p->k_theta = 20;        // +-10 degrees
    p->occ_min = 85;        // one hit's worth of log-odds (lslam_grid_params.l_hit)
    p->min_permille = 500;  // half of a perfect overlay
    return LSLAM_OK;
}

int lslam_mapfuse_params_default(lslam_mapfuse_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->r_scale = 1.0;
    p->nis_max = 16.27;      // the 99.9 % point of chi-square with 3 degrees of freedom
    p->cut_permille = 900;   // the candidates within a tenth of the winner's score
    return LSLAM_OK;
}

int lslam_reloc_params_default(lslam_reloc_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->head_step = 2.0 * LS_PI / 180.0;  // two degrees: the fine window's +-10 covers it five times
    p->n_head = 180;                     // the whole turn
    p->factor = 4;                       // 80 mm coarse cells at 20 mm: the fine window's +-200 mm covers them
    p->n_cand = 8;
    p->ambig_permille = 900;
    p->dup_mm = 100.0;                   // half the fine translation window
    p->dup_rad = 0.0873;                 // five degrees
    p->reset_sigma_xy = 50.0;            // mm
    p->reset_sigma_theta = 0.05;         // rad
    return LSLAM_OK;
}

int lslam_raycast_params_default(lslam_raycast_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    // a cell with any net evidence is read: p > 0.5 occupied, p < 0.5 free, L = 0 (never seen) unknown.  The
    // matchers' 85 with one pass's -41 calls the cells beside a wall (one hit, a few passes) unknown, and
    // they stop 28 % of a room's beams in front of the wall
    p->occ_min = 1;
    p->free_max = -1;
    p->tol = 3;         // steps: the map's walls are one to two cells thick
    return LSLAM_OK;
}

int lslam_recentre_params_default(lslam_recentre_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->margin = 128;  // cells: a quarter of the default map; the grid moves before max_range reaches far past the edge
    p->quantum = 8;   // cells: 16 bytes of a row, the group every reader of the grid loads
    return LSLAM_OK;
}

int lslam_dist_params_default(lslam_dist_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->mode = LSLAM_DIST_OCC;
    p->occ_min = 85;    // the matchers' threshold: one hit's worth
    p->free_max = -1;   // the ray caster's: p < 0.5
    p->d_max = 64;      // cells: 1.28 m at the default cell, beyond any clearance a stop acts on
    return LSLAM_OK;
}

int lslam_fieldscore_params_default(lslam_fieldscore_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->trunc2 = 625;    // 25 cells: an outlier costs no more
    p->near2 = 4;       // two cells: the map's walls are one to two cells thick
    p->off2 = 4096;     // the default d_max squared
    return LSLAM_OK;
}

int lslam_fieldalign_params_default(lslam_fieldalign_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->trunc = 25.0;       // cells: the square root of the score's trunc2; an outlier costs nothing
    p->damp_t = 1.0;       // one point's worth of gradient: a corridor's free direction stays put
    p->damp_r = 100.0;     // one point's worth at a lever arm of ten cells
    p->eps_t = 0.01;       // cells: 0.2 mm at the default cell, far below the range noise
    p->eps_r = 1e-4;       // rad: 0.01 cell at a lever arm of 100 cells
    p->max_shift = 200.0;  // mm: ten default cells, inside the basin that trunc leaves
    p->max_turn = 0.1;     // rad: beyond it the guess was lost, which is the matchers' case
    p->n_iter = 10;
    p->min_points = 16;    // three unknowns, with room for the outliers among them
    p->min_permille = 500;
    return LSLAM_OK;
}

int lslam_fieldfuse_params_default(lslam_fieldfuse_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->sigma_min = 0.5;                             // cells: the field cannot resolve less than half a cell
    p->r_scale = 1.0;
    p->floor_t = 1.0 / sqrt(12.0);                  // cells: one cell's quantum, as lslam_map_fuse's search quantum
    p->floor_r = (LS_PI / 360.0) / sqrt(12.0);      // rad: the matcher's heading quantum, so the two measurements floor alike
    p->nis_max = 16.27;                             // the 99.9 % point of chi-square with 3 degrees of freedom
    return LSLAM_OK;
}

int lslam_relocprior_params_default(lslam_relocprior_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->half_xy = 1000.0;   // mm: a filter that has drifted a metre ...
    p->half_theta = 0.5;   // ... and twenty-odd degrees still has its pose inside the window
    p->clear_min2 = 16;    // four fine cells: one coarse cell at the default factor
    return LSLAM_OK;
}

int lslam_page_params_default(lslam_page_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->canvas_w = 2048;  // cells: 40.96 m a side at 20 mm, sixteen default windows; 8 MiB a robot
    return LSLAM_OK;
}

int lslam_gridmerge_params_default(lslam_gridmerge_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->src_w = 512;
    p->n_src = 1;
    p->occ_min = 85;                // one hit: the matchers' and the distance field's threshold
    p->mode = LSLAM_MERGE_ADD;
    p->min_support = 64;            // cells: 1.28 m of common wall at 20 mm
    p->max_contra_permille = 100;   // measured in the L-shaped room (tests/test_gridmerge_ref.py)
    return LSLAM_OK;
}

int lslam_gridpoints_params_default(lslam_gridpoints_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->radius = 8000.0;  // the grid's default max_range: the matchers drop what lies further
    p->occ_min = 85;     // one hit: the matchers' and the merge's threshold
    p->cap = 1024;       // slots: the L-shaped room's 827 cells in range fit (tests/test_gridpoints_ref.py)
    return LSLAM_OK;
}

int lslam_posegraph_params_default(lslam_posegraph_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->damp_t = 1e-6;    // 1/mm^2: a prior of one metre on a node that no edge holds
    p->damp_r = 1e-3;    // 1/rad^2: some thirty radians, likewise
    p->eps_t = 0.01;     // mm: far below a keyframe's own uncertainty
    p->eps_r = 1e-5;     // rad: 0.01 mm at a lever arm of one metre
    p->max_nodes = 48;   // keyframes a graph: 20 KiB ... 81 KiB of LDS, one to several workgroups a CU
    p->max_edges = 256;
    p->n_iter = 10;
    return LSLAM_OK;
}

int lslam_posegate_params_default(lslam_posegate_params *p) {
    if (!p) return LSLAM_ERR_ARG;
    memset(p, 0, sizeof(*p));
    p->damp_t = 1e-6;    // lslam_posegraph_params' defaults: the solve that follows uses the same H
    p->damp_r = 1e-3;
    p->nis_max = 16.27;  // chi-square, 3 dof, 0.1 %: lslam_fieldfuse_params' gate
    p->max_nodes = 48;
    p->max_edges = 256;
    p->max_cand = 16;    // closures proposed between two solves
    p->append = 0;
    return LSLAM_OK;
}

double lslam_inlier_cutoff(double thr) {
    if (isnan(thr)) return NAN;
    if (!(thr > 0)) return 0.0;
    if (isinf(thr)) return INFINITY;
    double e = thr * thr;
    while (e > 0 && sqrt(e) >= thr) e = nextafter(e, 0.0);
    while (sqrt(e) < thr) e = nextafter(e, INFINITY);
    return e;
}

int lslam_ukf_weights(const lslam_ukf_params *p, double *Wm, double *Wc, double *lpn) {
    if (!p || !Wm || !Wc) return LSLAM_ERR_ARG;
    // filterpy MerweScaledSigmaPoints._compute_weights, n = 3
    const double n = 3.0;
    const double lambda_ = p->alpha * p->alpha * (n + p->kappa) - n;
    const double c = .5 / (n + lambda_);
    for (int i = 0; i < 7; i++) Wm[i] = Wc[i] = c;
    Wc[0] = lambda_ / (n + lambda_) + (1 - p->alpha * p->alpha + p->beta);
    Wm[0] = lambda_ / (n + lambda_);
    if (lpn) *lpn = lambda_ + n;
    return LSLAM_OK;
}

int lslam_mt_seed_state(uint32_t seed, uint32_t *st) {
    if (!st) return LSLAM_ERR_ARG;
    for (int i = 0; i < 624; i++) {
        st[i] = seed;
        seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)(i + 1);
    }
    st[624] = 624;
    return LSLAM_OK;
}

}  // extern "C"

