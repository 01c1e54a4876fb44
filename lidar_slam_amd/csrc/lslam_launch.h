// Host side, part 2 (included by lidarslam.hip after lslam_ctx.h): kernel arguments and LDS
// layouts, the launchers, run_split (the pipeline call: the producer's waits come from
// plan_producer, lslam_hazards.h) and the entry points that launch kernels: the scan pipeline, the UKF
// and the express codec.  The map side is lslam_launch_map.h, included below run_split.
#pragma once
#include <type_traits>

static inline int align16(int x) { return (x + 15) & ~15; }

// f(std::integral_constant<int, H>) for the hypothesis source H: the one place where the run-time
// hyp_source picks a kernel instantiation
template <typename F>
static void with_hyp_source(int hyp_source, F &&f) {
    switch (hyp_source) {
        case LSLAM_HYP_PHILOX: f(std::integral_constant<int, LSLAM_HYP_PHILOX>{}); break;
        case LSLAM_HYP_EXPLICIT: f(std::integral_constant<int, LSLAM_HYP_EXPLICIT>{}); break;
        default: f(std::integral_constant<int, LSLAM_HYP_MT19937>{}); break;
    }
}

static int validate_batch(const lslam_scan_batch *b, bool need_points) {
    if (!b) return set_err(LSLAM_ERR_ARG, "batch is NULL");
    if (b->n_scans < 0 || b->n_chunks < 0 || b->n_points < 0) return set_err(LSLAM_ERR_ARG, "negative sizes");
    if (b->n_scans == 0) return LSLAM_OK;
    if (!b->scan_chunk_off || !b->chunk_pt_off) return set_err(LSLAM_ERR_ARG, "missing CSR offsets");
    if (need_points && !b->xy && (!b->theta_deg || !b->dist_mm) && b->n_points > 0)
        return set_err(LSLAM_ERR_ARG, "missing points (xy, or theta_deg + dist_mm)");
    if (b->max_chunk_points < 0 || b->max_scan_chunks < 0) return set_err(LSLAM_ERR_ARG, "bad maxima");
    return LSLAM_OK;
}

#if defined(LSLAM_STAMPS) || defined(LSLAM_CENSUS)
static unsigned long long *g_wcen = nullptr;  // wave census (diagnostic builds)
static unsigned int *g_wcen_n = nullptr;
static unsigned int g_wcen_cap = 0;
static unsigned int g_call_seq = 0;
extern "C" int lslam_debug_set_census(unsigned long long *dev_buf, unsigned int *dev_count, unsigned int cap) {
    g_wcen = dev_buf;
    g_wcen_n = dev_count;
    g_wcen_cap = cap;
    return LSLAM_OK;
}
#endif
#ifdef LSLAM_STAMPS
static unsigned long long *g_dbg = nullptr;
extern "C" int lslam_debug_set_stamps(unsigned long long *dev_buf) {
    g_dbg = dev_buf;
    return LSLAM_OK;
}
#endif

// The fused scan kernel (the MT19937 fix-up) runs every chunk of a replayed scan through mt_draws
// with the chunk's OWN mt_nslot(n), and mt_nslot is not monotonic in n: 64 slots at n = 3, 8 from 17
// to 512 points, 2 above.  Its draw-resolution tables (j1s: one word per slot; nxt: n words per slot)
// must hold the worst chunk size up to the batch's largest, not the largest's own.
struct MtTables {
    int slots;    // max mt_nslot(n)
    int entries;  // max mt_nslot(n) * n
};
static MtTables mt_tables_upto(int N) {
    constexpr int SMALL = 512;  // mt_resolve_batch's threshold: above it mt_nslot(n) = 2
    static const std::vector<MtTables> pre = [] {
        std::vector<MtTables> v(SMALL + 1, MtTables{1, 1});
        for (int n = 1; n <= SMALL; n++) {
            const int s = mt_nslot(n);
            v[n].slots = std::max(v[n - 1].slots, s);
            v[n].entries = std::max(v[n - 1].entries, s * n);
        }
        return v;
    }();
    MtTables m = pre[std::min(std::max(N, 1), SMALL)];
    if (N > SMALL) {
        m.slots = std::max(m.slots, mt_nslot(N));
        m.entries = std::max(m.entries, mt_nslot(N) * N);
    }
    return m;
}

static int build_args(KArgs &k, const lslam_scan_batch *b, const lslam_ransac_params *p, const lslam_ukf_params *u,
                      int mode, int &lds) {
    memset(&k, 0, sizeof(k));
#ifdef LSLAM_STAMPS
    k.dbg = g_dbg;
#endif
#if defined(LSLAM_STAMPS) || defined(LSLAM_CENSUS)
    k.wcen = g_wcen;
    k.wcen_n = g_wcen_n;
    k.wcen_cap = g_wcen_cap;
    k.call_seq = g_call_seq;
#endif
    k.b = *b;
    if (p) {
        if (p->min_samples != 2) return set_err(LSLAM_ERR_UNSUPPORTED, "only min_samples == 2 (ransac_functions.py:11)");
        if (p->residual_threshold < 0) return set_err(LSLAM_ERR_ARG, "`residual_threshold` must be greater than zero");
        if (p->max_trials < 0) return set_err(LSLAM_ERR_ARG, "`max_trials` must be greater than zero");
        if (p->max_trials > 65533) return set_err(LSLAM_ERR_UNSUPPORTED, "max_trials > 65533");
        if (p->hyp_source < 0 || p->hyp_source > 2) return set_err(LSLAM_ERR_ARG, "bad hyp_source");
        if (p->hyp_source == LSLAM_HYP_EXPLICIT && !b->hyp) return set_err(LSLAM_ERR_ARG, "explicit hyp without hyp");
        k.thr = p->residual_threshold;
        k.ecut = lslam_inlier_cutoff(p->residual_threshold);
        k.ecut_q = std::sqrt(k.ecut) * 1.01 + 1.0;
        k.tol_a = p->tol_a;
        k.tol_b = p->tol_b;
        k.tol_dist = p->tol_dist;
        k.tol_dist_sq = sqrt_le_bound(p->tol_dist);
        k.philox_seed = p->philox_seed;
        k.T = p->max_trials;
        k.hyp_source = p->hyp_source;
        k.life = p->life;
    }
    if ((mode & MODE_ASSOC) && b->landmarks && !b->lmk_count) return set_err(LSLAM_ERR_ARG, "landmarks without lmk_count");
    const int N = b->max_chunk_points > 0 ? b->max_chunk_points : 1;
    const int T = k.T;
    int off = 0;
    if (mode & (MODE_RANSAC | MODE_HYP_ONLY)) {
        k.off_pts = off; off += align16(16 * N);
        k.off_key = off; off += align16(4 * 624);
        // phase-exclusive scratch shares one region: the draw-resolution tables
        // (draw generation), then the tie sums (selection)
        const MtTables mtt = mt_tables_upto(N);
        const int nxt_bytes = 4 * mtt.entries;
        const int uni_bytes = max(nxt_bytes, 8 * (T > 0 ? T : 1));
        k.off_ring = off;
        k.off_tsum = off;
        off += align16(uni_bytes);
        k.off_j1 = off;
        off += align16(4 * mtt.slots);
        k.off_draws = off; off += align16(8 * (T + 1));
        k.off_cnt = off; off += align16(4 * (T > 0 ? T : 1));
        k.off_tied = off; off += align16(4 * (T > 0 ? T : 1));
        k.off_mask = off; off += align16(N);
        k.off_vstack = off; off += (N > 128) ? align16(8 * 64 * 24) : 0;
        k.off_nstack = off; off += (N > 128) ? align16(4 * 72) : 0;
        k.off_recs = -1;
    } else {
        // post pass (association / UKF over fitted models): only the chunk's mask
        k.off_mask = off; off += align16(N);
        // and the scan's chunk records + offsets, staged up front (post_assoc_fast)
        const int msc = b->max_scan_chunks > 0 ? b->max_scan_chunks : 1;
        if (msc <= 256) {
            k.off_recs = off;
            off += align16((int)sizeof(lslam_chunk_model) * msc) + align16(4 * (msc + 1));
        } else {
            k.off_recs = -1;
        }
    }
    // the UKF runs after the last chunk: its scratch aliases the RANSAC scratch
    // above (offset 0); only the persistent region below (chunk history, chunk
    // origins, landmark list) is live across both
    if (u && u->n_landmarks > 0) {
        k.off_ukf = 0;
        off = max(off, align16(8 * UkfLds::doubles(u->n_landmarks)));
    }
    k.hist_cap = b->max_scan_chunks > 0 ? b->max_scan_chunks : 1;
    k.off_snap = off; off += (mode & MODE_RANSAC) ? align16(4 * MT_N) : 0;
    k.corg_cap = k.hist_cap;
    k.off_corg = off; off += align16(16 * k.corg_cap);
    k.off_zobs = off; off += (u && (u->flags & LSLAM_UKF_MAP)) ? align16(16 * k.corg_cap) : 0;
    k.lmk_cap = (mode & MODE_ASSOC) ? b->lmk_capacity : 0;
    if ((mode & MODE_ASSOC) && k.lmk_cap <= 0) return set_err(LSLAM_ERR_ARG, "lmk_capacity must be > 0");
    // the association-only post pass keeps a list of at most 64 entries in registers
    k.lmk_reg = (mode == MODE_ASSOC && k.lmk_cap > 0 && k.lmk_cap <= 64 && k.off_recs >= 0 &&
                 !(u && (u->flags & LSLAM_UKF_MAP)) && b->landmarks) ? 1 : 0;
    k.off_lmk = off; off += k.lmk_reg ? 0 : align16((int)sizeof(lslam_landmark) * (k.lmk_cap > 0 ? k.lmk_cap : 1));
    k.off_vis = off; off += k.lmk_reg ? 0 : align16(8 * ((k.lmk_cap + 63) / 64 + 1));
    k.pts_cap = N;
    if (u) {
        if (u->n_landmarks <= 0) return set_err(LSLAM_ERR_ARG, "n_landmarks must be > 0");
        const bool map = (u->flags & LSLAM_UKF_MAP) != 0;
        if (!b->ukf_x || !b->ukf_P || !b->ukf_u || !b->ukf_R_diag || (!map && (!b->ukf_z || !b->ukf_lmk)))
            return set_err(LSLAM_ERR_ARG, "UKF buffers missing");
        if (map && (!(mode & MODE_ASSOC) || !b->landmarks))
            return set_err(LSLAM_ERR_ARG, "LSLAM_UKF_MAP needs the landmark lists (the map) in lslam_scan_pipeline");
        if (map && u->n_landmarks < b->max_scan_chunks)
            return set_err(LSLAM_ERR_CAPACITY, "LSLAM_UKF_MAP: n_landmarks (measurement slots) < max_scan_chunks");
        double lpn = 0;
        lslam_ukf_weights(u, k.ukf.Wm, k.ukf.Wc, &lpn);
        for (int i = 0; i < 7; i++)
            if (k.ukf.Wc[i] == 0.0) return set_err(LSLAM_ERR_UNSUPPORTED, "zero covariance weight");
        k.ukf.cfac = lpn;
        k.ukf.dt = u->dt;
        k.ukf.wr = u->wheel_radius;
        k.ukf.wb = u->wheel_base;
        for (int i = 0; i < 9; i++) k.ukf.Q[i] = u->Q[i];
        k.ukf.L = u->n_landmarks;
        k.ukf.flags = u->flags;
    }
    lds = off;
    // The MODE_RANSAC layout is the MT19937 fix-up kernel's (run_split).  With Philox or explicit
    // hypotheses no kernel is launched with it: the consensus kernels lay out and check their own LDS
    // (layout_chunk, layout_select), so its size refuses nothing there beyond the points themselves.
    const bool unused = mode == MODE_RANSAC && p && p->hyp_source != LSLAM_HYP_MT19937 &&
                        (int64_t)16 * N <= 160 * 1024;
    if (lds > 160 * 1024 && !unused)
        return set_err(LSLAM_ERR_CAPACITY, "chunk/trial/landmark sizes exceed the 160 KiB LDS");
    return LSLAM_OK;
}

template <int MODE>
static hipError_t launch_mode(const KArgs &k, int lds, hipStream_t st) {
    const dim3 grid((unsigned)k.b.n_scans), block(64);
    with_hyp_source(k.hyp_source, [&](auto H) {
        hipLaunchKernelGGL((scan_kernel<decltype(H)::value, MODE>), grid, block, lds, st, k);
    });
    return hipGetLastError();
}

template <int MODE>
static int run_scan_kernel(lslam_ctx *c, const KArgs &k, int lds, int timer) {
    HIPCHK(hipSetDevice(c->device));
    if (k.b.n_scans == 0) return LSLAM_OK;
    static std::once_flag once;
    std::call_once(once, [] {
        const int mx = 160 * 1024;
        (void)hipFuncSetAttribute((const void *)scan_kernel<0, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
        (void)hipFuncSetAttribute((const void *)scan_kernel<1, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
        (void)hipFuncSetAttribute((const void *)scan_kernel<2, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, mx);
        set_max_lds(scan_kernel_w4<LSLAM_HYP_EXPLICIT, MODE>);
    });
    int st = timer_begin(c, timer);
    if (st) return st;
    if (MODE == MODE_UKF && !(k.ukf.flags & LSLAM_UKF_MAP)) {  // stand-alone UKF: lane groups
        launch_ukf_group(k, k.ukf.L, c->stream, false);
        HIPCHK(hipGetLastError());
    } else if (MODE == MODE_ASSOC || MODE == MODE_UKF) {  // stand-alone association / UKF: no producer beside them
        hipLaunchKernelGGL((scan_kernel_w4<LSLAM_HYP_EXPLICIT, MODE>), dim3((unsigned)k.b.n_scans), dim3(64), lds,
                           c->stream, k);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(launch_mode<MODE>(k, lds, c->stream));
    }
    st = timer_end(c, timer);
    if (st) return st;
    return LSLAM_OK;
}


// chunk_kernel LDS: one chunk's points, draws and consensus scratch
static int layout_chunk(KArgs &k, const lslam_scan_batch *b, int &lds) {
    const int N = b->max_chunk_points > 0 ? b->max_chunk_points : 1;
    const int T = k.T;
    int off = 0;
    k.off_pts = off; off += align16(16 * N);
    k.off_draws = off; off += (k.hyp_source == LSLAM_HYP_PHILOX) ? align16(8 * (T + 1)) : 0;  // else read in place
    k.off_cnt = off; off += align16(4 * (T > 0 ? T : 1));
    k.off_tied = off; off += align16(4 * (T > 0 ? T : 1));
    k.off_tsum = off; off += align16(8 * (T > 0 ? T : 1));  // tie sums
    k.off_mask = off; off += align16(N);
    k.off_vstack = off; off += (N > 128) ? align16(8 * 64 * 24) : 0;
    k.off_nstack = off; off += (N > 128) ? align16(4 * 72) : 0;
    k.off_vtmp = off;  // (pairwise sums from registers: pw_sum_regs)
    lds = off;
    if (lds > 160 * 1024) return set_err(LSLAM_ERR_CAPACITY, "chunk/trial sizes exceed the 160 KiB LDS");
    return LSLAM_OK;
}

// rng_kernel LDS: two raw MT blocks + flags
static int layout_rng(KArgs &k, const lslam_scan_batch *b, int &lds) {
    const int N = b->max_chunk_points > 3 ? b->max_chunk_points : 3;
    if (N > 65536) return set_err(LSLAM_ERR_UNSUPPORTED, "chunks of more than 65536 points");
    int off = 0;
    k.off_blk = off; off += align16(4 * (2 * 624 + 64));  // two block slots + the head pad
    k.rng_pipe_bytes = off;
    lds = off * RNG_PPW;
    // two K claims (16 B) + two reject tables shared by the workgroup's parsers, after the
    // pipes: table mode is chosen per chunk (N - 1 <= RT_KMAX), so a batch whose largest chunk
    // is bigger may still parse its small chunks with them
    k.off_stbl = lds;
    lds += 16 + 2 * 4 * RT_DWORDS;
    return LSLAM_OK;
}

// consumer grids: one workgroup per item, at most 2^30 (kernels loop over their items)
static inline unsigned launch_cap(int64_t n) { return (unsigned)(n < (1 << 30) ? (n > 0 ? n : 1) : (1 << 30)); }

// allow up to 160 KiB of LDS per workgroup (static + dynamic); a failure here must
// not linger as the runtime's last error for the next launch check
template <typename F>
static void set_max_lds(F *fn) {
    hipFuncAttributes at;
    size_t stat = 0;
    if (hipFuncGetAttributes(&at, (const void *)fn) == hipSuccess) stat = at.sharedSizeBytes;
    (void)hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - stat));
    (void)hipGetLastError();
}

// Producer slot: one j per Fisher-Yates step (D * n_points entries; chunk c at
// D * chunk_pt_off[c]; + slack for 16-byte staging loads) and the end-of-scan
// MT state.  The resolved draws live in the main-stream scratch unless the
// caller asked for draws_out.
// Epochs: when every scan is one chunk (C5) and the steps of all T + 1 draws
// exceed the slot budget (lslam_set_steps_budget, default 2 GiB), the producer
// runs in launches of ep_nd draws, each resolved before its slot is reused; the
// MT state chains through the slots' state areas.  k.ep_count launches.
static int prepare_steps(lslam_ctx *c, KArgs &k, int slot) {
    const int N = k.b.max_chunk_points;
    k.j8 = N <= 256 ? 1 : 0;
    const size_t per_draw = (size_t)(k.b.n_points > 0 ? k.b.n_points : 1) * (k.j8 ? 1 : 2);
    const size_t budget = c->steps_budget;
    const int D = k.T + 1;
    int De = D;
    if (k.b.max_scan_chunks == 1 && (size_t)D * per_draw > budget) {
        const size_t fit = budget / per_draw;
        De = fit < 1 ? 1 : (fit < (size_t)D ? (int)fit : D);
    }
    k.ep_nd = De < D ? De : 0;
    k.ep_d0 = 0;
    k.ep_count = (D + De - 1) / De;
    const size_t jbytes = ((size_t)De * per_draw + JBUF_FRONT + 64 + 255) & ~(size_t)255;
    const size_t sbytes = ((size_t)(k.b.n_scans > 0 ? k.b.n_scans : 1) * 625 * 4 + 255) & ~(size_t)255;
    if (!DevBuf::fits(c->pslot, NSLOTS, jbytes + sbytes)) c->hz.spec_ok = 0;  // the previous producer's end state goes with the old slots
    int st = DevBuf::ensure(c, c->pslot, NSLOTS, jbytes + sbytes, "producer slot");
    if (st) return st;
    k.jbuf = c->pslot[slot].as<unsigned char>() + JBUF_FRONT;
    k.state_scr = (uint32_t *)(c->pslot[slot].as<unsigned char>() + jbytes);
    k.slot_jbytes = jbytes;
    if (k.b.draws_out) {
        k.draws_scr = k.b.draws_out;
    } else {
        st = c->scr.ensure(c, (size_t)(k.b.n_chunks > 0 ? k.b.n_chunks : 1) * 2 * (k.T + 1) * 4, "step scratch");
        if (st) return st;
        k.draws_scr = c->scr.as<int32_t>();
    }
    return LSLAM_OK;
}

// resolve_kernel LDS: the chunk's staged steps (if they fit)
static int launch_resolve(lslam_ctx *c, const KArgs &base, hipStream_t rs) {
    if (base.b.n_chunks == 0) return LSLAM_OK;
    KArgs k = base;
    const int N = k.b.max_chunk_points > 3 ? k.b.max_chunk_points : 3;
    const int esz = k.j8 ? 1 : 2;
    // stage a chunk's steps in LDS when they fit 16 KiB (C3: 101 x 99 B), else stream them from HBM
    const int De = k.ep_nd > 0 ? k.ep_nd : k.T + 1;  // draws of this launch
    const int64_t need = ((int64_t)De * (N - 1) * esz + 46) & ~(int64_t)15;  // + alignment skew
    const int lds = need <= 16 * 1024 ? (int)need : 0;
    k.res_g = lds;  // staging capacity in bytes
    if (lds == 0) {  // steps streamed from HBM, waves over (chunk, draw)
        const int64_t items = (int64_t)k.b.n_chunks * De;
        // beside the next epoch's producer (produce_draws): four waves per SIMD beside its four
        // parsers.  The epoch loop is max(producer, resolve beside it): with the double-buffered
        // walk, three waves per SIMD measured 65.7-66.1 vs 68.9-69.3 ms per C5 call at two (r06d,
        // four: 66.0-66.3); once mask-mode runs crossed block ends (r06f: a 9 % faster producer)
        // the resolve was the longer again, and four gave 61.4-61.6 vs 63.5-63.6 ms at three.
        // (At r02, with five producer waves per SIMD, three displaced parser workgroups: 107 vs
        // 78 ms.  Measured and dropped: LDS tiles of [64 draws][128 steps], 1.0 vs 0.43 ms per
        // epoch.)
        const int64_t cap = k.ep_count > 1 ? 16 * (int64_t)c->n_cus : (1 << 20);
        const dim3 grid(launch_cap(items > cap ? cap : items)), block(64);
        if (k.j8) hipLaunchKernelGGL((resolve_walk_kernel<uint8_t, 16>), grid, block, 0, rs, k);
        else hipLaunchKernelGGL((resolve_walk_kernel<uint16_t, 16>), grid, block, 0, rs, k);
        HIPCHK(hipGetLastError());
        return LSLAM_OK;
    }
    if (k.j8 && c->resolve_beside) {  // no LDS: the producer's workgroups hold most of it
        if (N - 1 <= 16 * RR_GROUPS - 1) {
            // draws of this launch to resolve per chunk: all but draw T (never read by the
            // consensus) unless the caller wants the draws
            const bool has_last = k.ep_d0 + De == k.T + 1;
            const int Dres = (has_last && !k.b.draws_out && De > 1) ? De - 1 : De;
            if ((int64_t)k.b.n_chunks * Dres >= ((int64_t)1 << 31) - 64)
                return set_err(LSLAM_ERR_UNSUPPORTED, "more than 2^31 chunk draws in one call");
            const dim3 grid(launch_cap(((int64_t)k.b.n_chunks * Dres + 63) / 64)), block(64);
            hipLaunchKernelGGL(resolve_reg8_kernel, grid, block, 0, rs, k, Dres);
        } else {
            const dim3 grid(launch_cap(k.b.n_chunks)), block(64);
            hipLaunchKernelGGL(resolve_reg_kernel, grid, block, 0, rs, k);
        }
        HIPCHK(hipGetLastError());
        return LSLAM_OK;
    }
    static std::once_flag once;
    std::call_once(once, [] {
        set_max_lds(resolve_kernel<uint8_t>);
        set_max_lds(resolve_kernel<uint16_t>);
    });
    const dim3 grid(launch_cap(k.b.n_chunks)), block(64);
    if (k.j8) hipLaunchKernelGGL(resolve_kernel<uint8_t>, grid, block, lds, rs, k);
    else hipLaunchKernelGGL(resolve_kernel<uint16_t>, grid, block, lds, rs, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// Fresh streams (np.random.seed per scan, no mt_state_in): seed_kernel on `ss` fills seed buffer
// i and k.seed_state points the producer at it.
static int launch_seed(lslam_ctx *c, KArgs &k, hipStream_t ss, int i) {
    int st = c->seedst[i].ensure(c, (size_t)k.b.n_scans * MT_N * 4, "seed states");
    if (st) return st;
    hipLaunchKernelGGL(seed_kernel, dim3((unsigned)((k.b.n_scans + 63) / 64)), dim3(64), 0, ss, k.b.seeds,
                       (int)k.b.n_scans, c->seedst[i].as<uint32_t>());
    HIPCHK(hipGetLastError());
    k.seed_state = c->seedst[i].as<uint32_t>();
    return LSLAM_OK;
}

// chunk_kernel's chunks (at most 128 points): cut_lane_kernel on `ss` fills the next buffer of the
// cut ring and k.cuts points the consensus at it.  `ss` makes the producer's waits only, so a call
// whose points a pending copy or an earlier call wrote (pl.skip_cuts) launches none: the
// consensus, ordered after both on the ctx stream, computes the cuts itself.
static int launch_cuts(lslam_ctx *c, KArgs &k, const ProducerPlan &pl, hipStream_t ss) {
    k.cuts = nullptr;
    if (!precomputes_cuts(&k.b) || pl.skip_cuts) return LSLAM_OK;
    DevBuf &cb = c->cutb[c->cut_next];
    int st = cb.ensure(c, (size_t)k.b.n_chunks * sizeof(ChunkCut), "chunk cutoffs");
    if (st) return st;
    hipLaunchKernelGGL(cut_lane_kernel, dim3((unsigned)((k.b.n_chunks + 63) / 64)), dim3(64), 0, ss, k, cb.as<ChunkCut>());
    HIPCHK(hipGetLastError());
    k.cuts = cb.as<ChunkCut>();
    c->cut_next = (c->cut_next + 1) & 3;
    return LSLAM_OK;
}

// The pipeline seeds a fresh-stream call on a stream of its own as soon as the call is enqueued
// -- after the input waits the producer would make (copies into the seeds, a previous call
// writing them) and after the producer that last read its buffer (two buffers by call parity)
// -- so the seeding overlaps the previous call's producer, and the producer only waits for its
// event.  Measured and dropped: seed_kernel in the producer's stream order, right before
// rng_kernel (every producer launch 40 us later, moved onto the next resolve's launch: 0.917 vs
// 0.715 ms per C3 step) or before its slot wait (0.786 vs 0.716 ms: the producers no longer run
// back to back).  buf: the seed buffer used (-1: a chained state, nothing seeded).
static int seed_beside(lslam_ctx *c, KArgs &k, const ProducerPlan &pl, int &buf) {
    buf = -1;
    if (k.b.mt_state_in) return LSLAM_OK;
    const int i = c->seed_next;
    hipStream_t ss = c->sstream;
    HIPCHK(hipStreamWaitEvent(ss, c->ev_seed_read[i], 0));
    if (pl.wait_copy) HIPCHK(hipStreamWaitEvent(ss, c->ev_copy, 0));
    if (pl.hazard == 2) HIPCHK(hipStreamWaitEvent(ss, c->ev_call, 0));
    int st = launch_seed(c, k, ss, i);
    if (st) return st;
    if ((st = launch_cuts(c, k, pl, ss))) return st;
    HIPCHK(hipEventRecord(c->ev_seeded[i], ss));
    HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_seeded[i], 0));
    c->seed_next ^= 1;
    buf = i;
    return LSLAM_OK;
}

static int launch_rng(lslam_ctx *c, const KArgs &base, hipStream_t stream) {
    KArgs k = base;
    k.rt_all = c->rt_all;
    if (k.b.mt_state_in || k.ep_d0 != 0) k.seed_state = nullptr;  // a chained state, or a later epoch
    int lds = 0;
    int st = layout_rng(k, &k.b, lds);
    if (st) return st;
    static std::once_flag once;
    std::call_once(once, [] {
        set_max_lds(rng_kernel<uint8_t>);
        set_max_lds(rng_kernel<uint16_t>);
    });
    st = timer_begin(c, LSLAM_K_RNG, stream);
    if (st) return st;
    const dim3 grid((unsigned)((k.b.n_scans + RNG_PPW - 1) / RNG_PPW)), block(64 * RNG_PPW);
    if (k.j8) hipLaunchKernelGGL((rng_kernel<uint8_t>), grid, block, lds, stream, k);
    else hipLaunchKernelGGL((rng_kernel<uint16_t>), grid, block, lds, stream, k);
    HIPCHK(hipGetLastError());
    return timer_end(c, LSLAM_K_RNG, stream);
}

// Producer + resolve of a call: one launch, or k.ep_count epochs in alternating
// slots (prepare_steps).  rng_kernel runs on `ps` (after the previous epoch's
// resolve released its slot), the resolve on the ctx stream.  final_out: where
// the last launch writes the end state (null: the slot's state area).  On return
// k.state_scr is the end state's area and last_slot the slot the caller releases.
static int produce_draws(lslam_ctx *c, KArgs &k, int slot, hipStream_t ps, uint32_t *final_out, int &last_slot) {
    const int D = k.T + 1;
    // An epoch's resolve (the lane walk on a grid of two waves per SIMD) runs on the ctx
    // stream beside the next epoch's producer on ps, the slots alternating (C5: 78 vs 89 ms
    // per call with the epochs one after the other).
    const uint32_t *prev_state = nullptr;
    int sl = slot;
    for (int e = 0; e < k.ep_count; e++) {
        KArgs ke = k;
        if (k.ep_count > 1) {
            ke.ep_d0 = e * k.ep_nd;
            ke.ep_nd = std::min(k.ep_nd, D - ke.ep_d0);
            ke.jbuf = c->pslot[sl].as<unsigned char>() + JBUF_FRONT;
            ke.state_scr = (uint32_t *)(c->pslot[sl].as<unsigned char>() + k.slot_jbytes);
            if (e > 0) {
                if (ps != c->stream) HIPCHK(hipStreamWaitEvent(ps, c->ev_slot_free[sl], 0));
                ke.b.mt_state_in = prev_state;  // the previous epoch's end state (same parser, draw boundary)
            }
        }
        const bool last = e == k.ep_count - 1;
        ke.b.mt_state_out = (last && final_out) ? final_out : ke.state_scr;
        int st = launch_rng(c, ke, ps);
        if (st) return st;
        if (ps != c->stream) {
            HIPCHK(hipEventRecord(c->ev_produced, ps));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ev_produced, 0));
        }
        st = launch_resolve(c, ke, c->stream);
        if (st) return st;
        if (!last) HIPCHK(hipEventRecord(c->ev_slot_free[sl], c->stream));
        prev_state = ke.state_scr;
        last_slot = sl;
        sl = (sl + 1) % NSLOTS;
    }
    k.state_scr = const_cast<uint32_t *>(prev_state);
    c->next_slot = sl;
    return LSLAM_OK;
}

static void remember_outputs(lslam_ctx *c, const lslam_scan_batch *b, int T, int L) {
    const size_t S = (size_t)b->n_scans, C = (size_t)b->n_chunks, P = (size_t)b->n_points;
    const void *p[11] = {b->inlier_mask, b->models, b->y_proj, b->draws_out, b->trial_cnt_out, b->mt_state_out,
                         b->landmarks, b->lmk_count, b->lmk_walk, b->ukf_x, b->ukf_P};
    const size_t n[11] = {P, C * sizeof(lslam_chunk_model), P * 8, C * 2 * (T + 1) * 4, C * T * 4, S * 625 * 4,
                          S * b->lmk_capacity * sizeof(lslam_landmark), S * 4, S * b->lmk_capacity * 4,
                          L ? S * 24 : 0, L ? S * 72 : 0};
    for (int i = 0; i < 11; i++) c->hz.outs.add(p[i], n[i]);
}

// No event is recorded at the end of an entry point.  Each call's work on the producer and side
// streams joins the ctx stream before the call returns, so "every call so far" is the ctx
// stream's tail: copies on the ctx stream follow it by stream order, and another stream that
// must wait for it records ev_call at that moment (here) and waits on that.  An event recorded
// at every call's end would be a marker packet inside the pipelined ctx chain (~7 us between
// two kernels on the MI355X).
static int mark_calls(lslam_ctx *c) {
    HIPCHK(hipEventRecord(c->ev_call, c->stream));
    return LSLAM_OK;
}

// select_kernel LDS: the chunk's points, tied trials, tie sums, mask, sum scratch
static int layout_select(KArgs &k, const lslam_scan_batch *b, int &lds) {
    const int N = b->max_chunk_points > 0 ? b->max_chunk_points : 1;
    const int T = k.T > 0 ? k.T : 1;
    int off = 0;
    k.off_pts = off; off += align16(16 * N);
    k.off_tied = off; off += align16(4 * T);
    k.off_cnt = off; off += align16(4 * T);
    k.off_tsum = off; off += align16(8 * T);
    k.off_mask = off; off += align16(N);
    k.off_vstack = off; off += align16(8 * 24);
    k.off_nstack = off; off += align16(4 * 72);
    k.off_vtmp = off; off += align16(8 * 128);
    lds = off;
    if (lds > 160 * 1024) return set_err(LSLAM_ERR_CAPACITY, "chunk/trial sizes exceed the 160 KiB LDS");
    return LSLAM_OK;
}

// chunks of more than 128 points: count_kernel (many waves per chunk) + select_kernel
static int launch_chunks_large(lslam_ctx *c, KArgs &k) {
    const int T = k.T;
    const size_t nc = (size_t)k.b.n_chunks;
    const size_t cnt_bytes = (k.b.trial_cnt_out || T == 0) ? 0 : ((nc * T * 4 + 255) & ~(size_t)255);
    const bool philox = k.hyp_source == LSLAM_HYP_PHILOX;
    const size_t drw_bytes = (philox && !k.b.draws_out) ? ((nc * 2 * (size_t)(T + 1) * 4 + 255) & ~(size_t)255) : 0;
    const size_t mdl_bytes = nc * (size_t)(T > 0 ? T : 1) * 32;
    int st = c->cscr.ensure(c, cnt_bytes + drw_bytes + mdl_bytes, "consensus scratch");
    if (st) return st;
    unsigned char *base = c->cscr.as<unsigned char>();
    k.cnt_scr = k.b.trial_cnt_out ? k.b.trial_cnt_out : (int32_t *)base;
    if (philox) k.draws_scr = k.b.draws_out ? k.b.draws_out : (int32_t *)(base + cnt_bytes);
    k.models = (double *)(base + cnt_bytes + drw_bytes);
    const int N = k.b.max_chunk_points;
    int lds_sel = 0;
    st = layout_select(k, &k.b, lds_sel);
    if (st) return st;
    k.cnt_blocks = T > 0 ? (T + CNT_HYP_BLOCK - 1) / CNT_HYP_BLOCK : 0;
    static std::once_flag once;
    std::call_once(once, [] {
        set_max_lds(select_kernel<LSLAM_HYP_MT19937>);
        set_max_lds(select_kernel<LSLAM_HYP_PHILOX>);
        set_max_lds(select_kernel<LSLAM_HYP_EXPLICIT>);
    });
    const size_t nmod = nc * (size_t)(T + 1);
    const dim3 mgrid((unsigned)((nmod + 255) / 256)), block(256);
    with_hyp_source(k.hyp_source, [&](auto H) {
        hipLaunchKernelGGL(model_kernel<decltype(H)::value>, mgrid, block, 0, c->stream, k);
    });
    HIPCHK(hipGetLastError());
    if (k.cnt_blocks > 0) {
        const dim3 grid((unsigned)(nc * k.cnt_blocks)), cblock(CNT_TPB);
        // points per lane: the smallest power of two covering the chunk, at most 16 (then tiles)
        if (N <= 256) hipLaunchKernelGGL(count_kernel<1>, grid, cblock, 0, c->stream, k);
        else if (N <= 512) hipLaunchKernelGGL(count_kernel<2>, grid, cblock, 0, c->stream, k);
        else if (N <= 1024) hipLaunchKernelGGL(count_kernel<4>, grid, cblock, 0, c->stream, k);
        else if (N <= 2048) hipLaunchKernelGGL(count_kernel<8>, grid, cblock, 0, c->stream, k);
        else hipLaunchKernelGGL(count_kernel<16>, grid, cblock, 0, c->stream, k);
        HIPCHK(hipGetLastError());
    }
    const dim3 grid((unsigned)nc), sblock(64);
    with_hyp_source(k.hyp_source, [&](auto H) {
        hipLaunchKernelGGL(select_kernel<decltype(H)::value>, grid, sblock, lds_sel, c->stream, k);
    });
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

static int launch_chunks(lslam_ctx *c, const KArgs &base, bool write_yproj) {
    if (base.b.n_chunks == 0) return LSLAM_OK;
    KArgs k = base;
    k.write_yproj = write_yproj ? 1 : 0;
    int st = timer_begin(c, LSLAM_K_CONSENSUS);
    if (st) return st;
    if (k.b.max_chunk_points > 128) {
        st = launch_chunks_large(c, k);
        if (st) return st;
        return timer_end(c, LSLAM_K_CONSENSUS);
    }
    int lds = 0;
    st = layout_chunk(k, &k.b, lds);
    if (st) return st;
    static std::once_flag once;
    std::call_once(once, [] {
        set_max_lds(chunk_kernel<LSLAM_HYP_MT19937>);
        set_max_lds(chunk_kernel<LSLAM_HYP_PHILOX>);
        set_max_lds(chunk_kernel<LSLAM_HYP_EXPLICIT>);
    });
    const dim3 grid(launch_cap(k.b.n_chunks)), block(64);
    with_hyp_source(k.hyp_source, [&](auto H) {
        hipLaunchKernelGGL(chunk_kernel<decltype(H)::value>, grid, block, lds, c->stream, k);
    });
    HIPCHK(hipGetLastError());
    return timer_end(c, LSLAM_K_CONSENSUS);
}

template <int MODE>
static int launch_post(lslam_ctx *c, const KArgs &k, int lds) {
    static std::once_flag once;
    std::call_once(once, [] {
        set_max_lds(scan_kernel<LSLAM_HYP_EXPLICIT, MODE>);
        set_max_lds(scan_kernel_w4<LSLAM_HYP_EXPLICIT, MODE>);
    });
    const dim3 grid(launch_cap(k.b.n_scans));
    if (MODE == MODE_ASSOC && k.lmk_reg) {
        static std::once_flag once_reg;
        std::call_once(once_reg, [] { set_max_lds(post_reg_kernel); });
        hipLaunchKernelGGL(post_reg_kernel, grid, dim3(64), lds, c->stream, k);
    } else if (k.hyp_source == LSLAM_HYP_MT19937)  // beside the next call's producer
        hipLaunchKernelGGL((scan_kernel<LSLAM_HYP_EXPLICIT, MODE>), grid, dim3(64), lds, c->stream, k);
    else
        hipLaunchKernelGGL((scan_kernel_w4<LSLAM_HYP_EXPLICIT, MODE>), grid, dim3(64), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// rng_kernel -> chunk_kernel -> fix-up -> association/UKF post pass, all on the ctx stream
static int run_split(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ransac_params *p,
                     const lslam_ukf_params *u) {
    HIPCHK(hipSetDevice(c->device));
    if (b->n_scans == 0) return LSLAM_OK;
#if defined(LSLAM_STAMPS) || defined(LSLAM_CENSUS)
    g_call_seq += 1;
#endif
    const bool assoc = b->landmarks != nullptr;
    KArgs k;
    int lds_fix = 0;
    int st = build_args(k, b, p, nullptr, MODE_RANSAC, lds_fix);
    if (st) return st;
    const bool mt = k.hyp_source == LSLAM_HYP_MT19937;
    bool spec = false;
    int seed_buf = -1;  // the seed buffer this call's producer reads (seed_beside)
    int slot = c->next_slot;
    if (mt) {
        st = prepare_steps(c, k, slot);
        if (st) return st;
        c->next_slot = (c->next_slot + 1) % NSLOTS;
    }
    KArgs kp;
    int lds_post = 0;
    // a UKF step that reads nothing of this call's RANSAC (no LMK_FROM_RANSAC / MAP) runs
    // on the side stream, off the resolve -> consensus -> association chain
    // (Philox / explicit hypotheses only: beside the MT producer a third stream of UKF waves
    // slows the resolve -> consensus chain more than it saves, 1.23 -> 1.27-1.32 ms on C3, and
    // made the step bimodal)
    const bool ukf_side = p->hyp_source != LSLAM_HYP_MT19937 && u &&
                          !(u->flags & (LSLAM_UKF_LMK_FROM_RANSAC | LSLAM_UKF_MAP));
    // the UKF of the fused call on lane groups after the association pass (not in MAP mode,
    // whose measurements come out of the association walk itself)
    const bool ukf_lane = u && !ukf_side && !(u->flags & LSLAM_UKF_MAP);
    const int pmode = (assoc ? MODE_ASSOC : MODE_POST) | (u && !ukf_side && !ukf_lane ? MODE_UKF : 0);
    if ((pmode & MODE_UKF) && !(u->flags & LSLAM_UKF_MAP))  // scan_body's one-wave UKF fuses no origins
        return set_err(LSLAM_ERR_UNSUPPORTED, "post pass given a non-map UKF step");
    if (assoc || (u && !ukf_side && !ukf_lane)) {
        st = build_args(kp, b, p, (ukf_side || ukf_lane) ? nullptr : u, pmode, lds_post);
        if (st) return st;
    }
    KArgs kl;
    if (ukf_lane) {
        int lds_l = 0;
        st = build_args(kl, b, p, u, MODE_UKF, lds_l);
        if (st) return st;
        if ((u->flags & LSLAM_UKF_LMK_FROM_RANSAC) && !b->models)
            return set_err(LSLAM_ERR_ARG, "LSLAM_UKF_LMK_FROM_RANSAC needs the chunk models");
    }
    KArgs ku;
    int lds_u = 0;
    if (ukf_side) {
        st = build_args(ku, b, nullptr, u, MODE_UKF, lds_u);
        if (st) return st;
    }
    st = timer_begin(c, LSLAM_K_PIPELINE);
    if (st) return st;
    if (ukf_side) {
        // after the previous call (its outputs may be this step's inputs) and the latest copies
        if ((st = mark_calls(c))) return st;
        HIPCHK(hipStreamWaitEvent(c->ustream, c->ev_call, 0));
        HIPCHK(hipStreamWaitEvent(c->ustream, c->ev_copy, 0));
        launch_ukf_group(ku, u->n_landmarks, c->ustream, false);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev_ukf, c->ustream));
    }
    if (mt) {
        // producer on its own stream: it waits for input copies, (on a hazard) for the previous
        // call, and for its slot's previous consumers; the consumers wait for it.  A fresh
        // stream's seed_kernel goes between the input waits and the slot wait (seed_beside).
        const ProducerPlan pl = plan_producer(c->hz, b, k.ep_count);
        if (pl.wait_copy) HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_copy, 0));
        if (pl.hazard == 2) {
            if ((st = mark_calls(c))) return st;
            HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_call, 0));
        }
        if ((st = seed_beside(c, k, pl, seed_buf))) return st;
        HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_slot_free[slot], 0));
        // speculation (a chained stream, e.g. LandmarkMap steps): parse from the previous
        // producer's end state, which precedes this producer on pstream, instead of waiting for
        // the previous fix-up; this call's fix-up replays the scans that one replayed
        spec = pl.spec;
        if (pl.wait_prev_slot) HIPCHK(hipStreamWaitEvent(c->pstream, c->ev_slot_free[c->prev_slot], 0));
        c->resolve_beside = pl.resolve_beside;
        const uint32_t *true_in = k.b.mt_state_in;
        if (spec) k.b.mt_state_in = c->hz.prev_state_scr;
        st = produce_draws(c, k, slot, c->pstream, nullptr, slot);  // slot <- the last epoch's
        k.b.mt_state_in = true_in;  // the fix-up's replays start from the true state
        if (st) return st;
        if (seed_buf >= 0) HIPCHK(hipEventRecord(c->ev_seed_read[seed_buf], c->pstream));
    }
    // A UKF that reads nothing of this call's RANSAC runs between the fix-up and the post pass.
    // The fix-up releases this call's steps slot; the next producer starts ~40 us after that
    // event, so a UKF placed right behind the fix-up runs alone (35 us) instead of beside the
    // parsers (~180 us): C3 0.893 -> 0.858 ms per step, the producer 0.79 -> 0.71 ms in the
    // pipeline.  (Measured and dropped, DESIGN.md §8: the UKF before the fix-up, +2.7 %, or
    // before the consensus, +0.8 %; the slot released after the post pass or at the call's end.)
    const bool ukf_indep = ukf_lane && !(u->flags & (LSLAM_UKF_LMK_FROM_RANSAC | LSLAM_UKF_MAP));
    st = launch_chunks(c, k, !assoc);
    if (st) return st;
    if (mt) {
        KArgs kf = k;
        kf.fixup = 1;
        // replay flags: this call's, for the next call's speculation (one epoch only: the
        // end state is then the slot's state area)
        if (k.ep_count == 1 && b->mt_state_out) {
            if (spec && !DevBuf::fits(c->spec_dirty, 2, (size_t)b->n_scans))
                return set_err(LSLAM_ERR_HIP, "speculation without replay flags");  // unreachable
            if ((st = DevBuf::ensure(c, c->spec_dirty, 2, (size_t)b->n_scans, "flags"))) return st;
            kf.spec_dirty_in = spec ? c->spec_dirty[c->spec_cur].as<uint8_t>() : nullptr;
            kf.spec_dirty_out = c->spec_dirty[c->spec_cur ^ 1].as<uint8_t>();
        }
        static std::once_flag once;
        std::call_once(once, [] { set_max_lds(scan_kernel<LSLAM_HYP_MT19937, MODE_RANSAC>); });
        hipLaunchKernelGGL((scan_kernel<LSLAM_HYP_MT19937, MODE_RANSAC>), dim3(launch_cap(b->n_scans)), dim3(64), lds_fix,
                           c->stream, kf);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev_slot_free[slot], c->stream));
    }
    if (ukf_indep) {
        launch_ukf_group(kl, u->n_landmarks, c->stream, true);
        HIPCHK(hipGetLastError());
    }
    // (mt_state_out is final after the fix-up: the next call's producer may chain from it early)
    c->hz.prev_state_out = mt ? b->mt_state_out : nullptr;
    c->prev_slot = slot;
    c->hz.prev_fixed = mt ? 1 : 0;
    c->hz.spec_ok = (mt && k.ep_count == 1 && b->mt_state_out) ? 1 : 0;
    if (c->hz.spec_ok) {
        c->spec_cur ^= 1;  // the buffer this call's fix-up writes
        c->hz.prev_state_scr = k.state_scr;
        c->hz.prev_spec_scans = b->n_scans;
    }
    switch (pmode) {
        case MODE_ASSOC | MODE_UKF: st = launch_post<MODE_ASSOC | MODE_UKF>(c, kp, lds_post); break;
        case MODE_POST | MODE_UKF: st = launch_post<MODE_POST | MODE_UKF>(c, kp, lds_post); break;
        case MODE_ASSOC: st = launch_post<MODE_ASSOC>(c, kp, lds_post); break;
        default: break;
    }
    if (st) return st;
    if (ukf_lane && !ukf_indep) {  // reads this call's chunk models (LMK_FROM_RANSAC)
        launch_ukf_group(kl, u->n_landmarks, c->stream, true);
        HIPCHK(hipGetLastError());
    }
    if (ukf_side) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_ukf, 0));
    remember_outputs(c, b, k.T, u ? u->n_landmarks : 0);
    return timer_end(c, LSLAM_K_PIPELINE);
}

// The map side: its launchers and entry points.  Why here, between the launchers above and the entry
// points below: a kernel template is emitted into the code object where the translation unit first
// uses it, and a host template's kernels where that host template is first used.  The map launchers
// have always stood behind run_split and ahead of lslam_landmarks and lslam_ukf_step, whose
// run_scan_kernel<MODE> bring the last scan_kernel instantiations; included behind this file instead,
// the map side's kernel templates would land behind those.  Only fieldfuse_kernel belongs behind them,
// as the code object's last: lslam_launch_map.h names the two run_scan_kernel<MODE> ahead of
// launch_fieldfuse.  A new kernel goes behind every other first use, so that no kernel moves against
// another.
#include "lslam_launch_map.h"

// ---- express-scan codec (lslam_express.h) ----

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// packet streams are read as dwords: 4-byte alignment, and every rank fits int32
static int express_check(const uint8_t *packets, int64_t n) {
    if (n < 0 || (n > 0 && !packets)) return set_err(LSLAM_ERR_ARG, "express: bad packet stream");
    if (((uintptr_t)packets & 3) != 0) return set_err(LSLAM_ERR_ARG, "express: packet stream must be 4-byte aligned");
    if (n > ((int64_t)1 << 26)) return set_err(LSLAM_ERR_ARG, "express: more than 2^26 packets per call");
    return LSLAM_OK;
}

extern "C" {

int lslam_polar_to_xy(lslam_ctx *c, const double *th, const double *d, double *xy, int64_t n) {
    if (!c || n < 0 || (n > 0 && (!th || !d || !xy))) return LSLAM_ERR_ARG;
    if (n == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    int st = timer_begin(c, LSLAM_K_POLAR);
    if (st) return st;
    hipLaunchKernelGGL(polar_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, th, d, (double2 *)xy, n);
    HIPCHK(hipGetLastError());
    st = timer_end(c, LSLAM_K_POLAR);
    if (st) return st;
    c->hz.outs.add(xy, (size_t)n * 16);
    return LSLAM_OK;
}

int lslam_set_steps_budget(lslam_ctx *c, int64_t bytes) {
    if (!c) return LSLAM_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->pstream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->steps_budget = bytes > 0 ? (size_t)bytes : default_steps_budget();
    return LSLAM_OK;
}

int lslam_hyp_mt19937(lslam_ctx *c, const lslam_scan_batch *b, int32_t max_trials) {
    if (!c) return LSLAM_ERR_ARG;
    int st = validate_batch(b, false);
    if (st) return st;
    if (!b->draws_out) return set_err(LSLAM_ERR_ARG, "draws_out required");
    lslam_ransac_params p;
    lslam_ransac_params_default(&p);
    p.max_trials = max_trials;
    KArgs k;
    int lds = 0;
    st = build_args(k, b, &p, nullptr, MODE_HYP_ONLY, lds);
    if (st) return st;
    HIPCHK(hipSetDevice(c->device));
    if (b->n_scans == 0) return LSLAM_OK;
    k.hyp_source = LSLAM_HYP_MT19937;
    const int slot = c->next_slot;
    st = prepare_steps(c, k, slot);
    if (st) return st;
    c->next_slot = (c->next_slot + 1) % NSLOTS;
    st = timer_begin(c, LSLAM_K_HYP);
    if (st) return st;
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_slot_free[slot], 0));
    int last = slot;
    // on the main stream; the end state goes straight to mt_state_out
    c->resolve_beside = 0;  // alone on the ctx stream
    if (!b->mt_state_in && (st = launch_seed(c, k, c->stream, 2))) return st;  // fresh streams, seeded in stream order
    st = produce_draws(c, k, slot, c->stream, b->mt_state_out, last);
    if (st) return st;
    HIPCHK(hipEventRecord(c->ev_slot_free[last], c->stream));
    // the end state is written by the rng kernel itself, final at ev_slot_free[slot]: a
    // pipeline call chaining from it waits for that event, anything else for ev_call
    c->hz.outs.add(b->draws_out, (size_t)b->n_chunks * 2 * (size_t)(max_trials + 1) * 4);
    c->hz.outs.add(b->mt_state_out, (size_t)b->n_scans * 625 * 4);
    c->hz.prev_state_out = b->mt_state_out;
    c->prev_slot = last;
    c->hz.prev_fixed = b->mt_state_out ? 1 : 0;
    c->hz.spec_ok = 0;
    c->hz.spec_run = 0;
    return timer_end(c, LSLAM_K_HYP);
}

int lslam_ransac(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ransac_params *p) {
    if (!c || !p) return LSLAM_ERR_ARG;
    int st = validate_batch(b, true);
    if (st) return st;
    return run_split(c, b, p, nullptr);
}

int lslam_landmarks(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ransac_params *p) {
    if (!c || !p) return LSLAM_ERR_ARG;
    int st = validate_batch(b, true);
    if (st) return st;
    if (!b->models || !b->landmarks || !b->inlier_mask) return set_err(LSLAM_ERR_ARG, "models/landmarks/mask required");
    KArgs k;
    int lds = 0;
    st = build_args(k, b, p, nullptr, MODE_ASSOC, lds);
    if (st) return st;
    if ((st = run_scan_kernel<MODE_ASSOC>(c, k, lds, LSLAM_K_LANDMARK))) return st;
    remember_outputs(c, b, k.T, 0);
    return LSLAM_OK;
}

static int ukf_step_impl(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ukf_params *u, double *trace) {
    if (!c || !u || !b) return LSLAM_ERR_ARG;
    if (b->n_scans < 0) return LSLAM_ERR_ARG;
    lslam_scan_batch bb = *b;
    // UKF-only: no chunks are touched; give the kernel an empty CSR if absent
    KArgs k;
    int lds = 0;
    if (!bb.scan_chunk_off) return set_err(LSLAM_ERR_ARG, "scan_chunk_off required (may describe 0 chunks)");
    int st = build_args(k, &bb, nullptr, u, MODE_UKF, lds);
    if (st) return st;
    // always true here: build_args refuses LSLAM_UKF_MAP without the association pass (LSLAM_ERR_ARG
    // above), so the stand-alone step is the lane-group form and the one-wave form runs only as map
    // mode's post pass (tests/test_gpu_ukf_edges.py pins the refusal)
    const bool lanes = !(u->flags & LSLAM_UKF_MAP);
    if ((u->flags & LSLAM_UKF_SIGMAS_IN) && !b->ukf_sigmas)
        return set_err(LSLAM_ERR_ARG, "LSLAM_UKF_SIGMAS_IN without ukf_sigmas");
    if ((b->ukf_sigmas || trace) && !lanes)
        return set_err(LSLAM_ERR_UNSUPPORTED, "ukf_sigmas / trace need the lane-group UKF (not LSLAM_UKF_MAP)");
    if (trace && !(u->flags & LSLAM_UKF_UPDATE)) return set_err(LSLAM_ERR_ARG, "lslam_ukf_trace needs LSLAM_UKF_UPDATE");
    if (trace || b->ukf_sigmas) {
        HIPCHK(hipSetDevice(c->device));
        if (k.b.n_scans > 0) {
            if ((st = timer_begin(c, LSLAM_K_UKF))) return st;
            launch_ukf_group(k, k.ukf.L, c->stream, false, trace);
            HIPCHK(hipGetLastError());
            if ((st = timer_end(c, LSLAM_K_UKF))) return st;
        }
    } else if ((st = run_scan_kernel<MODE_UKF>(c, k, lds, LSLAM_K_UKF))) {
        return st;
    }
    c->hz.outs.add(b->ukf_x, (size_t)b->n_scans * 24);
    c->hz.outs.add(b->ukf_P, (size_t)b->n_scans * 72);
    c->hz.outs.add(b->ukf_sigmas, (size_t)b->n_scans * 168);
    if (trace) c->hz.outs.add(trace,(size_t)b->n_scans * 8 * ukf_tr_doubles(u->n_landmarks));
    return LSLAM_OK;
}

int lslam_ukf_step(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ukf_params *u) {
    return ukf_step_impl(c, b, u, nullptr);
}

int lslam_ukf_trace(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ukf_params *u, double *trace) {
    if (!trace) return set_err(LSLAM_ERR_ARG, "trace buffer required");
    return ukf_step_impl(c, b, u, trace);
}

int lslam_scan_pipeline(lslam_ctx *c, const lslam_scan_batch *b, const lslam_ransac_params *p,
                        const lslam_ukf_params *u) {
    if (!c || !p) return LSLAM_ERR_ARG;
    int st = validate_batch(b, true);
    if (st) return st;
    if (u && ((u->flags & LSLAM_UKF_SIGMAS_IN) || b->ukf_sigmas))
        return set_err(LSLAM_ERR_UNSUPPORTED, "ukf_sigmas / LSLAM_UKF_SIGMAS_IN are lslam_ukf_step's (filterpy's cache)");
    return run_split(c, b, p, u);
}

int lslam_express_decode(lslam_ctx *c, const uint8_t *packets, int64_t n_packets, const lslam_express_measures *out) {
    if (!c || !out) return LSLAM_ERR_ARG;
    int st = express_check(packets, n_packets);
    if (st) return st;
    if (n_packets == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    ExpressOut o{out->angle_deg, out->dist_mm, out->new_scan, out->valid, (double2 *)out->xy, out->pkt_valid};
    if ((st = timer_begin(c, LSLAM_K_EXPRESS))) return st;
    const int64_t blocks = (n_packets + EXP_DEC_PER_WG - 1) / EXP_DEC_PER_WG;
    hipLaunchKernelGGL(express_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, packets, n_packets, o);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_EXPRESS))) return st;
    const size_t nm = (size_t)(n_packets > 1 ? n_packets - 1 : 0) * 32;
    c->hz.outs.add(out->angle_deg, nm * 8);
    c->hz.outs.add(out->dist_mm, nm * 8);
    c->hz.outs.add(out->new_scan, nm);
    c->hz.outs.add(out->valid, nm);
    c->hz.outs.add(out->xy, nm * 16);
    c->hz.outs.add(out->pkt_valid, (size_t)n_packets);
    return LSLAM_OK;
}

int lslam_express_scans(lslam_ctx *c, const uint8_t *packets, int64_t n_packets, int32_t skip,
                        const lslam_express_revs *out) {
    if (!c || !out || !out->counts || !out->scan_chunk_off || !out->chunk_pt_off) return LSLAM_ERR_ARG;
    if (out->cap_scans < 0 || out->cap_chunks < 0 || out->cap_points < 0 || (out->cap_points > 0 && !out->xy))
        return set_err(LSLAM_ERR_ARG, "express: bad output capacities");
    int st = express_check(packets, n_packets);
    if (st) return st;
    if (skip < 0 || skip > 31) return set_err(LSLAM_ERR_ARG, "express: skip must be in [0, 31]");
    HIPCHK(hipSetDevice(c->device));
    const int64_t np = n_packets > 1 ? n_packets - 1 : 0;  // packets that carry measures
    const int64_t tiles = (np + EXP_TILE - 1) / EXP_TILE;
    size_t off = 0;
    const size_t o_flags = off;
    off = align256(off + (size_t)np);
    const size_t o_tile = off;
    off = align256(off + (size_t)tiles * sizeof(int2));
    const size_t o_rank = off;
    off = align256(off + (size_t)np * sizeof(int2));
    const size_t o_rend = off;
    off = align256(off + (size_t)np * sizeof(int2));
    const size_t o_rinfo = off;
    off = align256(off + (size_t)np * sizeof(int4));
    if ((st = c->escr.ensure(c, off > 0 ? off : 256, "express scratch"))) return st;
    uint8_t *base = c->escr.as<uint8_t>();
    ExpressScratch s{base + o_flags, (int2 *)(base + o_tile), (int2 *)(base + o_rank), (int2 *)(base + o_rend),
                     (int4 *)(base + o_rinfo), out->counts};
    ExpressScans o{(double2 *)out->xy, out->scan_chunk_off, out->chunk_pt_off, out->cap_points, out->cap_scans,
                   out->cap_chunks};
    if ((st = timer_begin(c, LSLAM_K_EXPRESS))) return st;
    if (tiles > 0) {
        hipLaunchKernelGGL(express_flags_kernel, dim3((unsigned)tiles), dim3(256), 0, c->stream, packets, n_packets,
                           (int)skip, s);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(express_rank_kernel, dim3((unsigned)tiles), dim3(256), 0, c->stream, n_packets, (int)skip, s);
        HIPCHK(hipGetLastError());
    }
    // revolutions <= packets with measures: one 256-revolution workgroup per packet tile
    hipLaunchKernelGGL(express_revs_kernel, dim3((unsigned)(tiles > 0 ? tiles : 1)), dim3(256), 0, c->stream,
                       (int)tiles, s, o);
    HIPCHK(hipGetLastError());
    if (np > 0) {
        if ((st = timer_begin(c, LSLAM_K_EXPRESS_SCATTER))) return st;
        const int64_t blocks = (np + EXP_DEC_PER_WG - 1) / EXP_DEC_PER_WG;
        hipLaunchKernelGGL(express_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, packets, n_packets,
                           (int)skip, s, o);
        HIPCHK(hipGetLastError());
        if ((st = timer_end(c, LSLAM_K_EXPRESS_SCATTER))) return st;
    }
    if ((st = timer_end(c, LSLAM_K_EXPRESS))) return st;
    // the outputs may feed a pipeline call whose MT producer runs on the other stream
    HIPCHK(hipEventRecord(c->ev_copy, c->stream));
    c->hz.copies.add(out->xy, (size_t)out->cap_points * 16);
    c->hz.copies.add(out->scan_chunk_off, ((size_t)out->cap_scans + 1) * 4);
    c->hz.copies.add(out->chunk_pt_off, ((size_t)out->cap_chunks + 1) * 4);
    c->hz.copies.add(out->counts, 16);
    return LSLAM_OK;
}

}  // extern "C"
