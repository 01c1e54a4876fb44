// Host side, part 2 (included by lidarslam.hip after lslam_ctx.h): kernel arguments and LDS
// layouts, the launchers, run_split (the pipeline call: the producer's waits come from
// plan_producer, lslam_hazards.h) and the entry points that launch kernels.
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
        const int nxt_bytes = 4 * mt_nslot(N) * N;
        const int uni_bytes = max(nxt_bytes, 8 * (T > 0 ? T : 1));
        k.off_ring = off;
        k.off_tsum = off;
        off += align16(uni_bytes);
        k.off_j1 = off;
        off += align16(4 * mt_nslot(N));
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
    if (lds > 160 * 1024) return set_err(LSLAM_ERR_CAPACITY, "chunk/trial/landmark sizes exceed the 160 KiB LDS");
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


// ---- the correlative search (lslam_corr.h): what the scan matcher and the scan-to-map matcher share ----

// The range checks of both matchers' params; who: the errors' prefix, width_name: the width field's name.
static int corr_check_params(const char *who, const char *width_name, double theta_step, int width, int smear, int k_trans,
                             int k_theta) {
    const std::string p = std::string(who) + ": ";
    if (!(theta_step > 0) || !std::isfinite(theta_step)) return set_err(LSLAM_ERR_ARG, (p + "theta_step must be > 0").c_str());
    if (width < 16 || width > 512 || (width & 1))
        return set_err(LSLAM_ERR_ARG, (p + width_name + " must be even, in [16, 512]").c_str());
    if (smear < 0 || smear > 2) return set_err(LSLAM_ERR_ARG, (p + "smear must be in [0, 2]").c_str());
    if (k_trans < 0 || k_trans > 15) return set_err(LSLAM_ERR_ARG, (p + "k_trans must be in [0, 15]").c_str());
    if (k_theta < 0 || k_theta > 31) return set_err(LSLAM_ERR_ARG, (p + "k_theta must be in [0, 31]").c_str());
    return LSLAM_OK;
}

// The geometry of a search over n robots, the slice rule and the score volume (the caller's `scores`
// or the context's scratch; vol = its bytes).  Slices: enough for two workgroups per CU (what the
// LDS allows) when the robots alone do not give them, at most one per rotation; each slice rebuilds G.
static int corr_geometry(lslam_ctx *c, const char *who, int n, double cell, double theta_step, int width, int smear,
                         int k_trans, int k_theta, int32_t *scores, CorrGeom &g, size_t &vol) {
    g.cell = cell;
    g.inv = 1.0 / cell;
    g.theta_step = theta_step;
    g.n = n;
    g.win_w = width;
    g.half = width / 2;
    g.smear = smear;
    g.kt = k_trans;
    g.kth = k_theta;
    g.Nt = 2 * k_trans + 1;
    g.Nth = 2 * k_theta + 1;
    g.W = width + 2 * k_trans;
    g.Sd = match_row_dwords(g.W);
    const int64_t want = 2 * (int64_t)c->n_cus;
    int64_t ns = (want + n - 1) / n;
    ns = std::min<int64_t>(std::max<int64_t>(ns, 1), g.Nth);
    g.per_slice = (int)((g.Nth + ns - 1) / ns);
    g.n_slices = (g.Nth + g.per_slice - 1) / g.per_slice;
    if ((int64_t)n * g.n_slices >= ((int64_t)1 << 31))
        return set_err(LSLAM_ERR_UNSUPPORTED, (std::string(who) + ": too many robots in one call").c_str());
    vol = (size_t)n * g.Nth * g.Nt * g.Nt * 4;
    g.scores = scores;
    if (!scores) {
        int st = c->mscr.ensure(c, vol, (std::string(who) + " scores").c_str());
        if (st) return st;
        g.scores = c->mscr.as<int32_t>();
    }
    return LSLAM_OK;
}

// ---- scan matcher (lslam_match.h) ----

static int match_check_params(const lslam_match_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "match: params is NULL");
    if (!(p->cell > 0) || !std::isfinite(p->cell)) return set_err(LSLAM_ERR_ARG, "match: cell must be > 0");
    return corr_check_params("match", "grid_w", p->theta_step, p->grid_w, p->smear, p->k_trans, p->k_theta);
}

// match_search_kernel on a grid of (robots x rotation slices), then match_pick_kernel per robot.
static int launch_match(lslam_ctx *c, const lslam_match_batch *b, const lslam_match_params *p,
                        const lslam_ukf_params *u) {
    MatchArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    size_t vol;
    int st = corr_geometry(c, "match", b->n_scans, p->cell, p->theta_step, p->grid_w, p->smear, p->k_trans, p->k_theta,
                           b->scores, k.g, vol);
    if (st) return st;
    k.write_u = (u && b->ukf_u) ? 1 : 0;
    if (k.write_u) {
        k.dt = u->dt;
        k.wr = u->wheel_radius;
        k.wb = u->wheel_base;
    }
    const int lds = match_lds_bytes(k.g.W, k.g.Sd, k.g.Nt);
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(match_search_kernel); });
    if ((st = timer_begin(c, LSLAM_K_MATCH))) return st;
    hipLaunchKernelGGL(match_search_kernel, dim3((unsigned)(k.g.n * k.g.n_slices)), dim3(MATCH_TPB), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(match_pick_kernel, dim3((unsigned)k.g.n), dim3(MATCH_PICK_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_MATCH))) return st;
    const size_t S = (size_t)b->n_scans;
    c->hz.outs.add(b->delta, S * 24);
    c->hz.outs.add(b->best, S * 16);
    c->hz.outs.add(b->n_valid, S * 8);
    c->hz.outs.add(b->flags, S * 4);
    c->hz.outs.add(b->scores, vol);
    if (k.write_u) c->hz.outs.add(b->ukf_u, S * 16);
    return LSLAM_OK;
}

// ---- occupancy grid (lslam_grid.h) ----

static int grid_check_params(const lslam_grid_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "grid: params is NULL");
    if (!(p->cell > 0) || !std::isfinite(p->cell)) return set_err(LSLAM_ERR_ARG, "grid: cell must be > 0");
    if (!(p->max_range > 0) || !std::isfinite(p->max_range) || !(p->max_range / p->cell <= 4096.0))
        return set_err(LSLAM_ERR_ARG, "grid: max_range must be > 0, finite and at most 4096 cells");
    if (p->grid_w < 16 || p->grid_w > 2048) return set_err(LSLAM_ERR_ARG, "grid: grid_w must be in [16, 2048]");
    if (p->l_hit < 1 || p->l_hit > 1024) return set_err(LSLAM_ERR_ARG, "grid: l_hit must be in [1, 1024]");
    if (p->l_miss < -1024 || p->l_miss > -1) return set_err(LSLAM_ERR_ARG, "grid: l_miss must be in [-1024, -1]");
    if (p->l_min < -32768 || p->l_min >= 0) return set_err(LSLAM_ERR_ARG, "grid: l_min must be in [-32768, -1]");
    if (p->l_max <= 0 || p->l_max > 32767) return set_err(LSLAM_ERR_ARG, "grid: l_max must be in [1, 32767]");
    return LSLAM_OK;
}

template <int T, int WAVE_RAY>
static int launch_grid_form(lslam_ctx *c, GridArgs &k) {
    k.ntile = (k.grid_w + T - 1) / T;
    const int64_t blocks = (int64_t)k.b.n_robots * k.ntile * k.ntile;
    if (blocks >= ((int64_t)1 << 31)) return set_err(LSLAM_ERR_UNSUPPORTED, "grid: too many robots in one call");
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(grid_update_kernel<T, WAVE_RAY>); });
    hipLaunchKernelGGL((grid_update_kernel<T, WAVE_RAY>), dim3((unsigned)blocks), dim3(GRID_TPB), grid_lds_bytes(T),
                       c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// One workgroup per (robot, tile).  LSLAM_GRID_FORM (tools/gridbench.py) selects the forms that were
// measured and dropped: "128l", "64w", "128w" (tile side; a lane or a wave per ray); default "64l".
static int launch_grid(lslam_ctx *c, const lslam_grid_batch *b, const lslam_grid_params *p) {
    GridArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.inv = 1.0 / p->cell;
    k.max_r2 = p->max_range * p->max_range;
    k.grid_w = p->grid_w;
    k.l_hit = p->l_hit;
    k.l_miss = p->l_miss;
    k.l_min = p->l_min;
    k.l_max = p->l_max;
    k.vec = (p->grid_w % 8 == 0 && ((uintptr_t)b->logodds & 15) == 0) ? 1 : 0;
    int T = GRID_T, wave_ray = GRID_WAVE_RAY;
    if (const char *e = getenv("LSLAM_GRID_FORM")) {
        if (atoi(e) == 64 || atoi(e) == 128) T = atoi(e);
        if (strchr(e, 'l')) wave_ray = 0;
        if (strchr(e, 'w')) wave_ray = 1;
    }
    int st = timer_begin(c, LSLAM_K_GRID);
    if (st) return st;
    if (T == 128) st = wave_ray ? launch_grid_form<128, 1>(c, k) : launch_grid_form<128, 0>(c, k);
    else st = wave_ray ? launch_grid_form<64, 1>(c, k) : launch_grid_form<64, 0>(c, k);
    if (st) return st;
    if ((st = timer_end(c, LSLAM_K_GRID))) return st;
    const size_t R = (size_t)b->n_robots;
    c->hz.outs.add(b->logodds, R * (size_t)p->grid_w * (size_t)p->grid_w * 2);
    c->hz.outs.add(b->rot, R * 16);
    c->hz.outs.add(b->n_used, R * 8);
    c->hz.outs.add(b->flags, R * 4);
    return LSLAM_OK;
}

// ---- scan-to-map matcher (lslam_mapmatch.h) ----

static int mapmatch_check_params(const lslam_mapmatch_params *m) {
    if (!m) return set_err(LSLAM_ERR_ARG, "mapmatch: params is NULL");
    int st = corr_check_params("mapmatch", "win_w", m->theta_step, m->win_w, m->smear, m->k_trans, m->k_theta);
    if (st) return st;
    if (m->occ_min < -32768 || m->occ_min > 32767)
        return set_err(LSLAM_ERR_ARG, "mapmatch: occ_min must be in [-32768, 32767]");
    if (m->min_permille < 0 || m->min_permille > 1000)
        return set_err(LSLAM_ERR_ARG, "mapmatch: min_permille must be in [0, 1000]");
    return LSLAM_OK;
}

// The matcher's pointers of a scan-to-map batch: 0 all there, 1 an input missing, 2 an output missing.
// (The callers keep their own texts: lslam_map_fuse names more pointers.)
static int mapmatch_missing(const lslam_mapmatch_batch *b) {
    if (!b->xy || !b->pt_off || !b->pose || !b->origin || !b->logodds || !b->rot) return 1;
    if (!b->pose_out || !b->delta || !b->best || !b->n_valid || !b->rot0 || !b->flags) return 2;
    return 0;
}

// The kernels' arguments of a scan-to-map search (launch_mapmatch, launch_mapfuse and the fine stage
// of launch_reloc); vol = the score volume's bytes.
static int mapmatch_args(lslam_ctx *c, const lslam_mapmatch_batch *b, const lslam_grid_params *g,
                         const lslam_mapmatch_params *m, MapMatchArgs &k, size_t &vol) {
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.map_w = g->grid_w;
    k.occ_min = m->occ_min;
    k.min_permille = m->min_permille;
    k.vec = (g->grid_w % 8 == 0 && ((uintptr_t)b->logodds & 15) == 0) ? 1 : 0;
    // LSLAM_MAPMATCH_FORM=cell (tools/mapmatchbench.py): the lane-per-cell window load on every map
    if (const char *e = getenv("LSLAM_MAPMATCH_FORM"))
        if (!strcmp(e, "cell")) k.vec = 0;
    return corr_geometry(c, "mapmatch", b->n_robots, g->cell, m->theta_step, m->win_w, m->smear, m->k_trans, m->k_theta,
                         b->scores, k.g, vol);
}

static int launch_mapmatch_search(lslam_ctx *c, const MapMatchArgs &k) {
    const int lds = mapmatch_lds_bytes(k.g.W, k.g.Sd, k.g.Nt);
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(mapmatch_search_kernel); });
    hipLaunchKernelGGL(mapmatch_search_kernel, dim3((unsigned)(k.g.n * k.g.n_slices)), dim3(MATCH_TPB), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// mapmatch_search_kernel on a grid of (robots x rotation slices), each slice reading the window and
// rebuilding G, then mapmatch_pick_kernel per robot.
static int launch_mapmatch_kernels(lslam_ctx *c, const MapMatchArgs &k) {
    int st = launch_mapmatch_search(c, k);
    if (st) return st;
    hipLaunchKernelGGL(mapmatch_pick_kernel, dim3((unsigned)k.g.n), dim3(MATCH_PICK_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// the matcher's outputs, for the hazard planner
static void mapmatch_outs(lslam_ctx *c, const lslam_mapmatch_batch *b, size_t vol) {
    const size_t R = (size_t)b->n_robots;
    c->hz.outs.add(b->pose_out, R * 24);
    c->hz.outs.add(b->delta, R * 24);
    c->hz.outs.add(b->best, R * 16);
    c->hz.outs.add(b->n_valid, R * 8);
    c->hz.outs.add(b->rot0, R * 16);
    c->hz.outs.add(b->flags, R * 4);
    c->hz.outs.add(b->scores, vol);
}

static int launch_mapmatch(lslam_ctx *c, const lslam_mapmatch_batch *b, const lslam_grid_params *g,
                           const lslam_mapmatch_params *m) {
    MapMatchArgs k;
    size_t vol;
    int st = mapmatch_args(c, b, g, m, k, vol);
    if (st) return st;
    if ((st = timer_begin(c, LSLAM_K_MAPMATCH))) return st;
    if ((st = launch_mapmatch_kernels(c, k))) return st;
    if ((st = timer_end(c, LSLAM_K_MAPMATCH))) return st;
    mapmatch_outs(c, b, vol);
    return LSLAM_OK;
}

// ---- match fusion (lslam_mapfuse.h) ----

static int mapfuse_check_params(const lslam_mapfuse_params *f) {
    if (!f) return set_err(LSLAM_ERR_ARG, "mapfuse: params is NULL");
    if (!(f->r_scale > 0) || !std::isfinite(f->r_scale))
        return set_err(LSLAM_ERR_ARG, "mapfuse: r_scale must be > 0 and finite");
    if (!(f->nis_max > 0)) return set_err(LSLAM_ERR_ARG, "mapfuse: nis_max must be > 0 (+inf: no gate)");
    if (f->cut_permille < 0 || f->cut_permille > 999)
        return set_err(LSLAM_ERR_ARG, "mapfuse: cut_permille must be in [0, 999]");
    return LSLAM_OK;
}

// launch_mapmatch with mapfuse_pick_kernel in the place of mapmatch_pick_kernel.
static int launch_mapfuse(lslam_ctx *c, const lslam_mapfuse_batch *b, const lslam_grid_params *g,
                          const lslam_mapmatch_params *m, const lslam_mapfuse_params *f) {
    MapFuseArgs k;
    memset(&k, 0, sizeof(k));
    size_t vol;
    int st = mapmatch_args(c, &b->m, g, m, k.m, vol);
    if (st) return st;
    k.P = b->P;
    k.P_out = b->P_out;
    k.z = b->z;
    k.Rm = b->Rm;
    k.nis = b->nis;
    k.moments = b->moments;
    k.r_scale = f->r_scale;
    k.nis_max = f->nis_max;
    k.cut_permille = f->cut_permille;
    if ((st = timer_begin(c, LSLAM_K_MAPFUSE))) return st;
    if ((st = launch_mapmatch_search(c, k.m))) return st;
    hipLaunchKernelGGL(mapfuse_pick_kernel<0>, dim3((unsigned)k.m.g.n), dim3(MATCH_PICK_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_MAPFUSE))) return st;
    const size_t R = (size_t)b->m.n_robots;
    mapmatch_outs(c, &b->m, vol);
    c->hz.outs.add(b->P_out, R * 72);
    c->hz.outs.add(b->z, R * 24);
    c->hz.outs.add(b->Rm, R * 72);
    c->hz.outs.add(b->nis, R * 8);
    c->hz.outs.add(b->moments, R * 80);
    return LSLAM_OK;
}

// ---- relocalisation (lslam_reloc.h) ----

static int reloc_check_params(const lslam_reloc_params *q, const lslam_grid_params *g, const lslam_mapmatch_params *m) {
    if (!q) return set_err(LSLAM_ERR_ARG, "reloc: params is NULL");
    if (!(q->head_step > 0) || !std::isfinite(q->head_step))
        return set_err(LSLAM_ERR_ARG, "reloc: head_step must be > 0");
    if (q->n_head < 4 || q->n_head > 1024) return set_err(LSLAM_ERR_ARG, "reloc: n_head must be in [4, 1024]");
    if (q->factor != 2 && q->factor != 4 && q->factor != 8)
        return set_err(LSLAM_ERR_ARG, "reloc: factor must be 2, 4 or 8");
    if (g->grid_w % q->factor != 0 || g->grid_w / q->factor < 4 || g->grid_w / q->factor > 256)
        return set_err(LSLAM_ERR_ARG, "reloc: factor must divide grid_w, with grid_w / factor in [4, 256]");
    if (q->n_cand < 1 || q->n_cand > RELOC_KMAX) return set_err(LSLAM_ERR_ARG, "reloc: n_cand must be in [1, 16]");
    if (q->ambig_permille < 0 || q->ambig_permille > 1000)
        return set_err(LSLAM_ERR_ARG, "reloc: ambig_permille must be in [0, 1000]");
    if (!(q->dup_mm >= 0)) return set_err(LSLAM_ERR_ARG, "reloc: dup_mm must be >= 0");
    if (!(q->dup_rad >= 0)) return set_err(LSLAM_ERR_ARG, "reloc: dup_rad must be >= 0");
    if (!(q->reset_sigma_xy > 0) || !std::isfinite(q->reset_sigma_xy))
        return set_err(LSLAM_ERR_ARG, "reloc: reset_sigma_xy must be > 0 and finite");
    if (!(q->reset_sigma_theta > 0) || !std::isfinite(q->reset_sigma_theta))
        return set_err(LSLAM_ERR_ARG, "reloc: reset_sigma_theta must be > 0 and finite");
    if (2 * m->k_trans < q->factor)
        return set_err(LSLAM_ERR_ARG, "reloc: the fine window must cover a coarse cell: 2 k_trans >= factor");
    if (!(2.0 * (double)m->k_theta * m->theta_step >= q->head_step))
        return set_err(LSLAM_ERR_ARG, "reloc: the fine window must cover a heading step: 2 k_theta theta_step >= head_step");
    return LSLAM_OK;
}

template <int FORM>
static int launch_reloc_search(lslam_ctx *c, const RelocArgs &k, int nr) {
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(reloc_search_kernel<FORM>); });
    hipLaunchKernelGGL(reloc_search_kernel<FORM>, dim3((unsigned)(nr * k.n_slices)), dim3(RELOC_TPB),
                       reloc_lds_bytes(k.Wc, k.RW), c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// The coarse stage in chunks of robots under the context's byte budget (search, peaks, the K best),
// then K times the scan-to-map matcher (launch_mapmatch_kernels), rank j's arrays in the place of
// the batch's, then the selection.  LSLAM_RELOC_FORM=add (tools/relocbench.py) selects the search
// form that was measured and dropped.
static int launch_reloc(lslam_ctx *c, const lslam_reloc_batch *b, const lslam_grid_params *g,
                        const lslam_mapmatch_params *m, const lslam_reloc_params *q) {
    const int R = b->n_robots, K = q->n_cand;
    RelocArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.f = q->factor;
    k.Wc = g->grid_w / q->factor;
    k.cellc = g->cell * (double)q->factor;
    k.invc = 1.0 / k.cellc;
    k.head_step = q->head_step;
    k.max_r2 = g->max_range * g->max_range;
    k.dup_mm = q->dup_mm;
    k.dup_rad = q->dup_rad;
    k.pxy = q->reset_sigma_xy * q->reset_sigma_xy;
    k.pth = q->reset_sigma_theta * q->reset_sigma_theta;
    k.map_w = g->grid_w;
    k.n_head = q->n_head;
    k.K = K;
    k.occ_min = m->occ_min;
    k.ambig = q->ambig_permille;
    k.nspan = (k.Wc + 31) / 32;
    k.RW = reloc_row_dwords(k.Wc, k.nspan);
    k.vec = (g->grid_w % 8 == 0 && ((uintptr_t)b->logodds & 15) == 0) ? 1 : 0;
    if (const char *e = getenv("LSLAM_RELOC_FORM"))
        if (!strcmp(e, "add")) k.form = 1;
    const size_t cells = (size_t)k.n_head * k.Wc * k.Wc;
    k.nbh = (k.Wc * k.Wc + RELOC_PEAK_BLOCK - 1) / RELOC_PEAK_BLOCK;
    k.nblk = k.n_head * k.nbh;
    const int nc = (int)std::min<size_t>((size_t)R, std::max<size_t>(1, c->reloc_budget / (cells * 4)));
    const int64_t want = 2 * (int64_t)c->n_cus;
    int64_t ns = (want + nc - 1) / nc;
    ns = std::min<int64_t>(std::max<int64_t>(ns, 1), k.n_head);
    k.per_slice = (int)((k.n_head + ns - 1) / ns);
    k.n_slices = (k.n_head + k.per_slice - 1) / k.per_slice;
    if ((int64_t)nc * k.nblk >= ((int64_t)1 << 31)) return set_err(LSLAM_ERR_UNSUPPORTED, "reloc: too many robots in one call");
    const size_t keys_bytes = ((size_t)nc * k.nblk * K * 8 + 255) & ~(size_t)255;
    int st = c->rscr.ensure(c, keys_bytes + (b->coarse_scores ? 0 : (size_t)nc * cells * 4), "reloc scratch");
    if (st) return st;
    k.keys = c->rscr.as<unsigned long long>();
    // the fine stage's batch of rank 0: its scratch is grown here, before the timer and the first launch
    lslam_mapmatch_batch mb;
    memset(&mb, 0, sizeof(mb));
    mb.n_robots = R;
    mb.xy = b->xy;
    mb.pt_off = b->pt_off;
    mb.origin = b->origin;
    mb.logodds = b->logodds;
    mb.rot = b->rot;
    MapMatchArgs mk;
    size_t mvol;
    if ((st = mapmatch_args(c, &mb, g, m, mk, mvol))) return st;
    if ((st = timer_begin(c, LSLAM_K_RELOC))) return st;
    for (int r0 = 0; r0 < R; r0 += nc) {
        const int nr = std::min(nc, R - r0);
        k.r0 = r0;
        k.vol = b->coarse_scores ? b->coarse_scores + (size_t)r0 * cells : (int32_t *)(c->rscr.as<char>() + keys_bytes);
        if ((st = k.form ? launch_reloc_search<1>(c, k, nr) : launch_reloc_search<0>(c, k, nr))) return st;
        hipLaunchKernelGGL(reloc_peak_kernel, dim3((unsigned)(nr * k.nblk)), dim3(RELOC_PEAK_TPB), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(reloc_topk_kernel, dim3((unsigned)nr), dim3(RELOC_PEAK_TPB), 0, c->stream, k);
        HIPCHK(hipGetLastError());
    }
    const size_t Rz = (size_t)R;
    // LSLAM_RELOC_STAGES=coarse (tools/relocbench.py): the coarse stage alone; the fine outputs, result, flags
    // and pose_out are not written
    const char *stages = getenv("LSLAM_RELOC_STAGES");
    if (stages && !strcmp(stages, "coarse")) return timer_end(c, LSLAM_K_RELOC);
    for (int j = 0; j < K; j++) {
        mb.pose = b->cand_pose + (size_t)j * Rz * 3;
        mb.pose_out = b->fine_pose + (size_t)j * Rz * 3;
        mb.delta = b->fine_delta + (size_t)j * Rz * 3;
        mb.best = b->fine_best + (size_t)j * Rz * 4;
        mb.n_valid = b->fine_nvalid + (size_t)j * Rz * 2;
        mb.rot0 = b->fine_rot0 + (size_t)j * Rz * 2;
        mb.flags = b->fine_flags + (size_t)j * Rz;
        if ((st = mapmatch_args(c, &mb, g, m, mk, mvol))) return st;  // (the stream orders the reuse of its scratch)
        if ((st = launch_mapmatch_kernels(c, mk))) return st;
    }
    hipLaunchKernelGGL(reloc_select_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_RELOC))) return st;
    const size_t KR = (size_t)K * Rz;
    c->hz.outs.add(b->n_occ, Rz * 4);
    c->hz.outs.add(b->n_used, Rz * 4);
    c->hz.outs.add(b->cand, KR * 16);
    c->hz.outs.add(b->cand_pose, KR * 24);
    c->hz.outs.add(b->fine_pose, KR * 24);
    c->hz.outs.add(b->fine_delta, KR * 24);
    c->hz.outs.add(b->fine_best, KR * 16);
    c->hz.outs.add(b->fine_nvalid, KR * 8);
    c->hz.outs.add(b->fine_rot0, KR * 16);
    c->hz.outs.add(b->fine_flags, KR * 4);
    c->hz.outs.add(b->result, Rz * 32);
    c->hz.outs.add(b->flags, Rz * 4);
    c->hz.outs.add(b->pose_out, Rz * 24);
    c->hz.outs.add(b->P_out, Rz * 72);
    c->hz.outs.add(b->coarse_scores, Rz * cells * 4);
    return LSLAM_OK;
}

// ---- grid ray casting (lslam_raycast.h) ----

static int raycast_check_params(const lslam_raycast_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "raycast: params is NULL");
    if (p->occ_min < -32768 || p->occ_min > 32767)
        return set_err(LSLAM_ERR_ARG, "raycast: occ_min must be in [-32768, 32767]");
    if (p->free_max < -32768 || p->free_max > 32766 || p->free_max >= p->occ_min)
        return set_err(LSLAM_ERR_ARG, "raycast: free_max must be in [-32768, 32766] and below occ_min");
    if (p->tol < 0 || p->tol > 64) return set_err(LSLAM_ERR_ARG, "raycast: tol must be in [0, 64]");
    return LSLAM_OK;
}

template <int FORM>
static int launch_raycast_form(lslam_ctx *c, const RaycastArgs &k, int lds) {
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(raycast_kernel<FORM>); });
    hipLaunchKernelGGL(raycast_kernel<FORM>, dim3((unsigned)((int64_t)k.b.n_robots * k.n_slices)), dim3(RAYCAST_TPB), lds,
                       c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// One workgroup per (robot, slice of its points), by launch_mapmatch's rule: slices exist so that a
// few robots still fill the chip.  The HBM form ships: in the bench room's grids it is the faster one
// at 4096 robots.  LSLAM_RAYCAST_FORM=lds (tools/raycastbench.py, the tests) selects
// the LDS form where the largest window's codes fit its budget.
static int launch_raycast(lslam_ctx *c, const lslam_raycast_batch *b, const lslam_grid_params *g,
                          const lslam_raycast_params *p) {
    RaycastArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.inv = 1.0 / g->cell;
    k.max_r2 = g->max_range * g->max_range;
    k.far = g->max_range + 2.0 * g->cell;
    k.grid_w = g->grid_w;
    k.Rc = (int)floor(g->max_range * k.inv);
    k.occ_min = p->occ_min;
    k.free_max = p->free_max;
    k.tol = p->tol;
    k.vec = (g->grid_w % 8 == 0 && ((uintptr_t)b->logodds & 15) == 0) ? 1 : 0;
    const int win = raycast_window(k.Rc, k.grid_w);
    k.Sd = raycast_row_dwords(win);
    int hbm = 1;
    if (const char *e = getenv("LSLAM_RAYCAST_FORM"))
        if (!strcmp(e, "lds") && raycast_lds_bytes(win) <= RAYCAST_LDS_BUDGET) hbm = 0;
    const int64_t n = b->n_robots, want = 2 * (int64_t)c->n_cus;
    k.n_slices = (int)std::min<int64_t>(std::max<int64_t>((want + n - 1) / n, 1), RAYCAST_MAX_SLICES);
    if (n * k.n_slices >= ((int64_t)1 << 31)) return set_err(LSLAM_ERR_UNSUPPORTED, "raycast: too many robots in one call");
    int st = timer_begin(c, LSLAM_K_RAYCAST);
    if (st) return st;
    HIPCHK(hipMemsetAsync(b->counts, 0, (size_t)n * 32, c->stream));
    st = hbm ? launch_raycast_form<1>(c, k, 32) : launch_raycast_form<0>(c, k, raycast_lds_bytes(win));
    if (st) return st;
    if ((st = timer_end(c, LSLAM_K_RAYCAST))) return st;
    // (cls and stop are as long as pt_off, on the device, says: per-point outputs that no producer reads)
    c->hz.outs.add(b->counts, (size_t)n * 32);
    c->hz.outs.add(b->rot, (size_t)n * 16);
    c->hz.outs.add(b->flags, (size_t)n * 4);
    return LSLAM_OK;
}

// ---- grid recentre (lslam_recentre.h) ----

static int recentre_check_params(const lslam_recentre_params *p, const lslam_grid_params *g) {
    if (!p) return set_err(LSLAM_ERR_ARG, "recentre: params is NULL");
    if (p->margin < 0 || p->margin > g->grid_w / 2)
        return set_err(LSLAM_ERR_ARG, "recentre: margin must be in [0, grid_w / 2]");
    if (p->quantum < 1 || p->quantum > 64) return set_err(LSLAM_ERR_ARG, "recentre: quantum must be in [1, 64]");
    return LSLAM_OK;
}

// One workgroup per robot (two on one robot would race: lslam_recentre.h).  With grid_w and quantum
// multiples of 8 every shift lies on 16-byte groups and the instantiation without the lane-per-cell
// path, and without its LDS, is launched.
static int launch_recentre(lslam_ctx *c, const lslam_recentre_batch *b, const lslam_grid_params *g,
                           const lslam_recentre_params *p) {
    RecentreArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.cell = g->cell;
    k.inv = 1.0 / g->cell;
    k.grid_w = g->grid_w;
    k.margin = p->margin;
    k.quantum = p->quantum;
    k.band_rows = recentre_band_rows(g->grid_w);
    k.vec = (g->grid_w % 8 == 0 && ((uintptr_t)b->logodds & 15) == 0) ? 1 : 0;
    if (b->n_robots > (1 << 30)) return set_err(LSLAM_ERR_UNSUPPORTED, "recentre: too many robots in one call");
    int st = timer_begin(c, LSLAM_K_RECENTRE);
    if (st) return st;
    if (k.vec && p->quantum % 8 == 0)
        hipLaunchKernelGGL(recentre_kernel<0>, dim3((unsigned)recentre_blocks(b->n_robots)), dim3(RECENTRE_TPB), 0, c->stream, k);
    else
        hipLaunchKernelGGL(recentre_kernel<1>, dim3((unsigned)recentre_blocks(b->n_robots)), dim3(RECENTRE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_RECENTRE))) return st;
    const size_t R = (size_t)b->n_robots;
    c->hz.outs.add(b->logodds, R * (size_t)g->grid_w * (size_t)g->grid_w * 2);
    c->hz.outs.add(b->origin, R * 16);
    c->hz.outs.add(b->shift, R * 8);
    c->hz.outs.add(b->flags, R * 4);
    return LSLAM_OK;
}

// ---- distance field and its read (lslam_dist.h) ----

static int dist_check_params(const lslam_dist_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "dist: params is NULL");
    if (p->mode != LSLAM_DIST_OCC && p->mode != LSLAM_DIST_NOT_FREE)
        return set_err(LSLAM_ERR_ARG, "dist: mode must be LSLAM_DIST_OCC or LSLAM_DIST_NOT_FREE");
    if (p->occ_min < -32768 || p->occ_min > 32767) return set_err(LSLAM_ERR_ARG, "dist: occ_min must be in [-32768, 32767]");
    if (p->free_max < -32768 || p->free_max > 32767)
        return set_err(LSLAM_ERR_ARG, "dist: free_max must be in [-32768, 32767]");
    if (p->d_max < 1 || p->d_max > DIST_D_MAX) return set_err(LSLAM_ERR_ARG, "dist: d_max must be in [1, 255]");
    return LSLAM_OK;
}

// The band of rows of a workgroup: all of a robot's rows when the robots alone fill the chip, else so
// many bands that there are two workgroups to a CU (at most DIST_MAX_SLICES per robot), in whole
// groups of DIST_NW rows; then shrunk until the workgroup's LDS leaves room for two on a CU, or at
// least fits one.  0: not even a band of DIST_NW rows fits.
static int dist_band_rows(int W, int hal, int64_t n_robots, int n_cus) {
    const int64_t want = std::min<int64_t>(std::max<int64_t>((2 * (int64_t)n_cus + n_robots - 1) / n_robots, 1), DIST_MAX_SLICES);
    int band = (int)((W + want - 1) / want);
    band = (band + DIST_NW - 1) / DIST_NW * DIST_NW;
    while (band > DIST_NW && dist_lds_bytes(W, dist_blocks(W, band, hal)) > DIST_LDS_TWO) band -= DIST_NW;
    if (dist_lds_bytes(W, dist_blocks(W, band, hal)) <= DIST_LDS_TWO) return band;
    // (no band leaves room for two: the largest that fits one)
    band = (int)((W + want - 1) / want);
    band = (band + DIST_NW - 1) / DIST_NW * DIST_NW;
    while (band > DIST_NW && dist_lds_bytes(W, dist_blocks(W, band, hal)) > DIST_LDS_MAX) band -= DIST_NW;
    return dist_lds_bytes(W, dist_blocks(W, band, hal)) <= DIST_LDS_MAX ? band : 0;
}

static int launch_dist(lslam_ctx *c, const lslam_dist_batch *b, const lslam_grid_params *g, const lslam_dist_params *p) {
    static std::once_flag once;
    std::call_once(once, [] {
        set_max_lds(dist_kernel<8>);
        set_max_lds(dist_kernel<1>);
    });
    DistArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.grid_w = g->grid_w;
    k.d_max = p->d_max;
    k.not_free = p->mode == LSLAM_DIST_NOT_FREE ? 1 : 0;
    k.thr = k.not_free ? p->free_max + 1 : p->occ_min;
    k.hal = std::min(p->d_max, g->grid_w) - 1;
    k.band = dist_band_rows(k.grid_w, k.hal, b->n_robots, c->n_cus);
    if (!k.band) return set_err(LSLAM_ERR_UNSUPPORTED, "dist: the bitmap of 2 d_max rows of this grid_w does not fit LDS");
    k.n_slices = (k.grid_w + k.band - 1) / k.band;
    k.nblk = dist_blocks(k.grid_w, k.band, k.hal);
    const int lds = dist_lds_bytes(k.grid_w, k.nblk);
    const int64_t n = b->n_robots;
    if (n * k.n_slices >= ((int64_t)1 << 31)) return set_err(LSLAM_ERR_UNSUPPORTED, "dist: too many robots in one call");
    const bool vec = g->grid_w % 8 == 0 && (((uintptr_t)b->logodds | (uintptr_t)b->d2) & 15) == 0;
    HIPCHK(hipMemsetAsync(b->n_src, 0, (size_t)n * 4, c->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b->flags, LSLAM_DIST_EMPTY, (size_t)n, c->stream));
    if (vec) hipLaunchKernelGGL(dist_kernel<8>, dim3((unsigned)(n * k.n_slices)), dim3(DIST_TPB), lds, c->stream, k);
    else hipLaunchKernelGGL(dist_kernel<1>, dim3((unsigned)(n * k.n_slices)), dim3(DIST_TPB), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    c->hz.outs.add(b->d2, (size_t)n * (size_t)g->grid_w * (size_t)g->grid_w * 2);
    c->hz.outs.add(b->n_src, (size_t)n * 4);
    c->hz.outs.add(b->flags, (size_t)n * 4);
    return LSLAM_OK;
}

static int fieldscore_check_params(const lslam_fieldscore_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "fieldscore: params is NULL");
    if (p->trunc2 < 1 || p->trunc2 > 65025) return set_err(LSLAM_ERR_ARG, "fieldscore: trunc2 must be in [1, 65025]");
    if (p->near2 < 0 || p->near2 > 65025) return set_err(LSLAM_ERR_ARG, "fieldscore: near2 must be in [0, 65025]");
    if (p->off2 < 0 || p->off2 > 65025) return set_err(LSLAM_ERR_ARG, "fieldscore: off2 must be in [0, 65025]");
    return LSLAM_OK;
}

// One workgroup per (robot, slice of its points), by launch_raycast's rule.
static int launch_fieldscore(lslam_ctx *c, const lslam_fieldscore_batch *b, const lslam_grid_params *g,
                             const lslam_fieldscore_params *p) {
    FieldScoreArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.inv = 1.0 / g->cell;
    k.max_r2 = g->max_range * g->max_range;
    k.grid_w = g->grid_w;
    k.trunc2 = p->trunc2;
    k.near2 = p->near2;
    k.off2 = p->off2;
    const int64_t n = b->n_robots, want = 2 * (int64_t)c->n_cus;
    k.n_slices = (int)std::min<int64_t>(std::max<int64_t>((want + n - 1) / n, 1), FIELDSCORE_MAX_SLICES);
    if (n * k.n_slices >= ((int64_t)1 << 31)) return set_err(LSLAM_ERR_UNSUPPORTED, "fieldscore: too many robots in one call");
    HIPCHK(hipMemsetAsync(b->stats, 0, (size_t)n * 32, c->stream));
    hipLaunchKernelGGL(fieldscore_kernel, dim3((unsigned)(n * k.n_slices)), dim3(FIELDSCORE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    c->hz.outs.add(b->rot, (size_t)n * 16);
    c->hz.outs.add(b->stats, (size_t)n * 32);
    c->hz.outs.add(b->clear2, (size_t)n * 4);
    c->hz.outs.add(b->flags, (size_t)n * 4);
    return LSLAM_OK;
}

// ---- alignment in the field (lslam_fieldalign.h) ----

static int fieldalign_check_params(const lslam_fieldalign_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "fieldalign: params is NULL");
    if (!(p->trunc >= 0.0 && p->trunc <= 255.0)) return set_err(LSLAM_ERR_ARG, "fieldalign: trunc must be in [0, 255]");
    if (!(p->damp_t >= 0.0) || !std::isfinite(p->damp_t)) return set_err(LSLAM_ERR_ARG, "fieldalign: damp_t must be >= 0 and finite");
    if (!(p->damp_r >= 0.0) || !std::isfinite(p->damp_r)) return set_err(LSLAM_ERR_ARG, "fieldalign: damp_r must be >= 0 and finite");
    if (!(p->eps_t >= 0.0) || !std::isfinite(p->eps_t)) return set_err(LSLAM_ERR_ARG, "fieldalign: eps_t must be >= 0 and finite");
    if (!(p->eps_r >= 0.0) || !std::isfinite(p->eps_r)) return set_err(LSLAM_ERR_ARG, "fieldalign: eps_r must be >= 0 and finite");
    if (!(p->max_shift >= 0.0)) return set_err(LSLAM_ERR_ARG, "fieldalign: max_shift must be >= 0");
    if (!(p->max_turn >= 0.0)) return set_err(LSLAM_ERR_ARG, "fieldalign: max_turn must be >= 0");
    if (p->n_iter < 1 || p->n_iter > FIELDALIGN_MAX_ITER) return set_err(LSLAM_ERR_ARG, "fieldalign: n_iter must be in [1, 32]");
    if (p->min_points < 0) return set_err(LSLAM_ERR_ARG, "fieldalign: min_points must be >= 0");
    if (p->min_permille < 0 || p->min_permille > 1000) return set_err(LSLAM_ERR_ARG, "fieldalign: min_permille must be in [0, 1000]");
    return LSLAM_OK;
}

// One wave per robot, FIELDALIGN_RPB robots to a workgroup.
static int launch_fieldalign(lslam_ctx *c, const lslam_fieldalign_batch *b, const lslam_grid_params *g,
                             const lslam_fieldalign_params *p) {
    FieldAlignArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.p = *p;
    k.cell = g->cell;
    k.inv = 1.0 / g->cell;
    k.max_r2 = g->max_range * g->max_range;
    k.grid_w = g->grid_w;
    const size_t n = (size_t)b->n_robots, rows = (size_t)p->n_iter + 1;
    // (pose_out is written for every robot; the rest is zeros where the kernel writes nothing)
    HIPCHK(hipMemsetAsync(b->trace, 0, n * rows * 40, c->stream));
    HIPCHK(hipMemsetAsync(b->normal, 0, n * 80, c->stream));
    HIPCHK(hipMemsetAsync(b->n_used, 0, n * 12, c->stream));
    HIPCHK(hipMemsetAsync(b->iters, 0, n * 4, c->stream));
    const unsigned blocks = (unsigned)((n + FIELDALIGN_RPB - 1) / FIELDALIGN_RPB);
    hipLaunchKernelGGL(fieldalign_kernel, dim3(blocks), dim3(FIELDALIGN_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    c->hz.outs.add(b->pose_out, n * 24);
    c->hz.outs.add(b->trace, n * rows * 40);
    c->hz.outs.add(b->normal, n * 80);
    c->hz.outs.add(b->n_used, n * 12);
    c->hz.outs.add(b->iters, n * 4);
    c->hz.outs.add(b->flags, n * 4);
    return LSLAM_OK;
}

// ---- field fusion (lslam_fieldfuse.h) ----

static int fieldfuse_check_params(const lslam_fieldfuse_params *f) {
    if (!f) return set_err(LSLAM_ERR_ARG, "fieldfuse: params is NULL");
    if (!(f->sigma_min > 0) || !std::isfinite(f->sigma_min)) return set_err(LSLAM_ERR_ARG, "fieldfuse: sigma_min must be > 0 and finite");
    if (!(f->r_scale > 0) || !std::isfinite(f->r_scale)) return set_err(LSLAM_ERR_ARG, "fieldfuse: r_scale must be > 0 and finite");
    if (!(f->floor_t > 0) || !std::isfinite(f->floor_t)) return set_err(LSLAM_ERR_ARG, "fieldfuse: floor_t must be > 0 and finite");
    if (!(f->floor_r > 0) || !std::isfinite(f->floor_r)) return set_err(LSLAM_ERR_ARG, "fieldfuse: floor_r must be > 0 and finite");
    if (!(f->nis_max > 0)) return set_err(LSLAM_ERR_ARG, "fieldfuse: nis_max must be > 0 (+inf: no gate)");
    return LSLAM_OK;
}

// true iff [a, a + na) and [b, b + nb) share a byte
static bool fieldfuse_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// (launch_fieldfuse stands above lslam_field_fuse, behind every other launch: see there)

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

// (the checks that need no device come first, the context last: tests/test_scanmatch_ref.py)
int lslam_scan_match(lslam_ctx *c, const lslam_match_batch *b, const lslam_match_params *p,
                     const lslam_ukf_params *u) {
    int st = match_check_params(p);
    if (st) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "match: batch is NULL");
    if (b->n_scans < 0) return set_err(LSLAM_ERR_ARG, "match: negative n_scans");
    if (b->n_scans > 0) {
        if (!b->ref_xy || !b->ref_off || !b->cur_xy || !b->cur_off || !b->rot)
            return set_err(LSLAM_ERR_ARG, "match: missing input (ref_xy, ref_off, cur_xy, cur_off, rot)");
        if (!b->delta || !b->best || !b->n_valid || !b->flags)
            return set_err(LSLAM_ERR_ARG, "match: missing output (delta, best, n_valid, flags)");
        if (u && b->ukf_u && (!(u->dt > 0) || !(u->wheel_radius > 0)))
            return set_err(LSLAM_ERR_ARG, "match: wheel speeds need dt > 0 and wheel_radius > 0");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "match: ctx is NULL");
    if (b->n_scans == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_match(c, b, p, u);
}

// On the main stream: every pipeline call ends there (its post pass and lane-group UKF run on it,
// and it waits for ev_ukf when the UKF ran on the side stream), so a ukf_x given as pose is final.
int lslam_grid_update(lslam_ctx *c, const lslam_grid_batch *b, const lslam_grid_params *p) {
    int st = grid_check_params(p);
    if (st) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "grid: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "grid: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->xy || !b->pt_off || !b->pose || !b->origin)
            return set_err(LSLAM_ERR_ARG, "grid: missing input (xy, pt_off, pose, origin)");
        if (!b->logodds || !b->rot || !b->n_used || !b->flags)
            return set_err(LSLAM_ERR_ARG, "grid: missing output (logodds, rot, n_used, flags)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "grid: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_grid(c, b, p);
}

// On the main stream, as lslam_grid_update: a ukf_x given as pose is final, and so is the grid that
// a preceding lslam_grid_update wrote.
int lslam_map_match(lslam_ctx *c, const lslam_mapmatch_batch *b, const lslam_grid_params *g,
                    const lslam_mapmatch_params *m) {
    int st = mapmatch_check_params(m);
    if (st) return st;
    if ((st = grid_check_params(g))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "mapmatch: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "mapmatch: negative n_robots");
    if (b->n_robots > 0) {
        const int miss = mapmatch_missing(b);
        if (miss == 1) return set_err(LSLAM_ERR_ARG, "mapmatch: missing input (xy, pt_off, pose, origin, logodds, rot)");
        if (miss == 2)
            return set_err(LSLAM_ERR_ARG, "mapmatch: missing output (pose_out, delta, best, n_valid, rot0, flags)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "mapmatch: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_mapmatch(c, b, g, m);
}

// On the main stream, as lslam_map_match.
int lslam_map_fuse(lslam_ctx *c, const lslam_mapfuse_batch *b, const lslam_grid_params *g,
                   const lslam_mapmatch_params *m, const lslam_mapfuse_params *f) {
    int st = mapmatch_check_params(m);
    if (st) return st;
    if ((st = grid_check_params(g))) return st;
    if ((st = mapfuse_check_params(f))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "mapfuse: batch is NULL");
    if (b->m.n_robots < 0) return set_err(LSLAM_ERR_ARG, "mapfuse: negative n_robots");
    if (b->m.n_robots > 0) {
        const int miss = mapmatch_missing(&b->m);
        if (miss == 1 || !b->P)
            return set_err(LSLAM_ERR_ARG, "mapfuse: missing input (xy, pt_off, pose, origin, logodds, rot, P)");
        if (miss == 2 || !b->P_out || !b->z || !b->Rm || !b->nis)
            return set_err(LSLAM_ERR_ARG,
                           "mapfuse: missing output (pose_out, delta, best, n_valid, rot0, flags, P_out, z, Rm, nis)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "mapfuse: ctx is NULL");
    if (b->m.n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_mapfuse(c, b, g, m, f);
}

// On the main stream, as lslam_map_match.
int lslam_map_relocalize(lslam_ctx *c, const lslam_reloc_batch *b, const lslam_grid_params *g,
                         const lslam_mapmatch_params *m, const lslam_reloc_params *q) {
    int st = mapmatch_check_params(m);
    if (st) return st;
    if ((st = grid_check_params(g))) return st;
    if ((st = reloc_check_params(q, g, m))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "reloc: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "reloc: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->xy || !b->pt_off || !b->origin || !b->logodds || !b->rot || !b->head_rot)
            return set_err(LSLAM_ERR_ARG, "reloc: missing input (xy, pt_off, origin, logodds, rot, head_rot)");
        if (!b->n_occ || !b->n_used || !b->cand || !b->cand_pose || !b->fine_pose || !b->fine_delta || !b->fine_best ||
            !b->fine_nvalid || !b->fine_rot0 || !b->fine_flags || !b->result || !b->flags || !b->pose_out)
            return set_err(LSLAM_ERR_ARG,
                           "reloc: missing output (n_occ, n_used, cand, cand_pose, fine_pose, fine_delta, fine_best, "
                           "fine_nvalid, fine_rot0, fine_flags, result, flags, pose_out)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "reloc: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_reloc(c, b, g, m, q);
}

// On the main stream, as lslam_map_match.
int lslam_grid_raycast(lslam_ctx *c, const lslam_raycast_batch *b, const lslam_grid_params *g,
                       const lslam_raycast_params *p) {
    int st = raycast_check_params(p);
    if (st) return st;
    if ((st = grid_check_params(g))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "raycast: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "raycast: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->xy || !b->pt_off || !b->pose || !b->origin || !b->logodds)
            return set_err(LSLAM_ERR_ARG, "raycast: missing input (xy, pt_off, pose, origin, logodds)");
        if (!b->cls || !b->counts || !b->rot || !b->flags)
            return set_err(LSLAM_ERR_ARG, "raycast: missing output (cls, counts, rot, flags)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "raycast: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_raycast(c, b, g, p);
}

// On the main stream, as lslam_grid_update: ordered after the calls that read the grid where it was and
// before the calls that read it where it is.
int lslam_grid_recentre(lslam_ctx *c, const lslam_recentre_batch *b, const lslam_grid_params *g,
                        const lslam_recentre_params *p) {
    int st = grid_check_params(g);
    if (st) return st;
    if ((st = recentre_check_params(p, g))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "recentre: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "recentre: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->pose || !b->origin || !b->logodds)
            return set_err(LSLAM_ERR_ARG, "recentre: missing input (pose, origin, logodds)");
        if (!b->shift || !b->flags) return set_err(LSLAM_ERR_ARG, "recentre: missing output (shift, flags)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "recentre: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_recentre(c, b, g, p);
}

// On the main stream, as lslam_grid_raycast: after the calls that wrote the grid.
int lslam_grid_distance(lslam_ctx *c, const lslam_dist_batch *b, const lslam_grid_params *g, const lslam_dist_params *p) {
    int st = grid_check_params(g);
    if (st) return st;
    if ((st = dist_check_params(p))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "dist: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "dist: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->logodds) return set_err(LSLAM_ERR_ARG, "dist: missing input (logodds)");
        if (!b->d2 || !b->n_src || !b->flags) return set_err(LSLAM_ERR_ARG, "dist: missing output (d2, n_src, flags)");
        const uintptr_t bytes = (uintptr_t)b->n_robots * (uintptr_t)g->grid_w * (uintptr_t)g->grid_w * 2;
        const uintptr_t l0 = (uintptr_t)b->logodds, d0 = (uintptr_t)b->d2;
        if (l0 < d0 + bytes && d0 < l0 + bytes) return set_err(LSLAM_ERR_ARG, "dist: d2 overlaps logodds");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "dist: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_dist(c, b, g, p);
}

// On the main stream, as lslam_grid_raycast.
int lslam_field_score(lslam_ctx *c, const lslam_fieldscore_batch *b, const lslam_grid_params *g,
                      const lslam_fieldscore_params *p) {
    int st = grid_check_params(g);
    if (st) return st;
    if ((st = fieldscore_check_params(p))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "fieldscore: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "fieldscore: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->xy || !b->pt_off || !b->pose || !b->origin || !b->d2)
            return set_err(LSLAM_ERR_ARG, "fieldscore: missing input (xy, pt_off, pose, origin, d2)");
        if (!b->rot || !b->stats || !b->clear2 || !b->flags)
            return set_err(LSLAM_ERR_ARG, "fieldscore: missing output (rot, stats, clear2, flags)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "fieldscore: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_fieldscore(c, b, g, p);
}

// On the main stream, as lslam_field_score.
int lslam_field_align(lslam_ctx *c, const lslam_fieldalign_batch *b, const lslam_grid_params *g,
                      const lslam_fieldalign_params *p) {
    int st = grid_check_params(g);
    if (st) return st;
    if ((st = fieldalign_check_params(p))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "fieldalign: batch is NULL");
    if (b->n_robots < 0) return set_err(LSLAM_ERR_ARG, "fieldalign: negative n_robots");
    if (b->n_robots > 0) {
        if (!b->xy || !b->pt_off || !b->pose || !b->origin || !b->d2)
            return set_err(LSLAM_ERR_ARG, "fieldalign: missing input (xy, pt_off, pose, origin, d2)");
        if (!b->pose_out || !b->trace || !b->normal || !b->n_used || !b->iters || !b->flags)
            return set_err(LSLAM_ERR_ARG, "fieldalign: missing output (pose_out, trace, normal, n_used, iters, flags)");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "fieldalign: ctx is NULL");
    if (b->n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_fieldalign(c, b, g, p);
}

// launch_fieldalign with pose_out := z, then one thread per robot for steps 5-11.  It stands here, behind
// every other launch of the file, for fieldfuse_kernel's place in the code object: a kernel template is
// emitted where it is first launched, and from here it lands behind the last scan_kernel instantiation,
// so that no existing kernel moves against another.
static int launch_fieldfuse(lslam_ctx *c, const lslam_fieldfuse_batch *b, const lslam_grid_params *g,
                            const lslam_fieldalign_params *p, const lslam_fieldfuse_params *f) {
    lslam_fieldalign_batch a = b->a;
    a.pose_out = b->z;
    int st = launch_fieldalign(c, &a, g, p);
    if (st) return st;
    FieldFuseArgs k;
    memset(&k, 0, sizeof(k));
    k.n_robots = b->a.n_robots;
    k.pose = b->a.pose;
    k.P = b->P;
    k.z = b->z;
    k.normal = b->a.normal;
    k.n_used = b->a.n_used;
    k.flags = b->a.flags;
    k.pose_out = b->a.pose_out;
    k.P_out = b->P_out;
    k.info = b->info;
    k.info_f = b->info_f;
    k.s2 = b->s2;
    k.nis = b->nis;
    k.k = fieldfuse_consts(g->cell, f->sigma_min, f->r_scale, f->floor_t, f->floor_r, f->nis_max);
    const size_t n = (size_t)b->a.n_robots;
    const unsigned blocks = (unsigned)((n + FIELDFUSE_TPB - 1) / FIELDFUSE_TPB);
    hipLaunchKernelGGL(fieldfuse_kernel<0>, dim3(blocks), dim3(FIELDFUSE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    c->hz.outs.add(b->a.pose_out, n * 24);
    c->hz.outs.add(b->P_out, n * 72);
    c->hz.outs.add(b->info, n * 72);
    c->hz.outs.add(b->info_f, n * 72);
    c->hz.outs.add(b->s2, n * 8);
    c->hz.outs.add(b->nis, n * 8);
    return LSLAM_OK;
}

// On the main stream, as lslam_field_align.
int lslam_field_fuse(lslam_ctx *c, const lslam_fieldfuse_batch *b, const lslam_grid_params *g,
                     const lslam_fieldalign_params *p, const lslam_fieldfuse_params *f) {
    int st = grid_check_params(g);
    if (st) return st;
    if ((st = fieldalign_check_params(p))) return st;
    if ((st = fieldfuse_check_params(f))) return st;
    if (!b) return set_err(LSLAM_ERR_ARG, "fieldfuse: batch is NULL");
    if (b->a.n_robots < 0) return set_err(LSLAM_ERR_ARG, "fieldfuse: negative n_robots");
    if (b->a.n_robots > 0) {
        const lslam_fieldalign_batch &a = b->a;
        if (!a.xy || !a.pt_off || !a.pose || !a.origin || !a.d2 || !b->P)
            return set_err(LSLAM_ERR_ARG, "fieldfuse: missing input (xy, pt_off, pose, origin, d2, P)");
        if (!a.pose_out || !a.trace || !a.normal || !a.n_used || !a.iters || !a.flags || !b->P_out || !b->z || !b->info ||
            !b->info_f || !b->s2 || !b->nis)
            return set_err(LSLAM_ERR_ARG, "fieldfuse: missing output (pose_out, trace, normal, n_used, iters, flags, P_out, "
                                          "z, info, info_f, s2, nis)");
        const size_t n = (size_t)a.n_robots;
        if (fieldfuse_overlap(b->z, n * 24, a.pose, n * 24) || fieldfuse_overlap(b->z, n * 24, a.pose_out, n * 24) ||
            fieldfuse_overlap(b->z, n * 24, b->P, n * 72) || fieldfuse_overlap(b->z, n * 24, b->P_out, n * 72))
            return set_err(LSLAM_ERR_ARG, "fieldfuse: z must not overlap pose, pose_out, P or P_out");
    }
    if (!c) return set_err(LSLAM_ERR_ARG, "fieldfuse: ctx is NULL");
    if (b->a.n_robots == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch_fieldfuse(c, b, g, p, f);
}

// (the scratch is sized per call: a call in flight keeps the chunking it was launched with)
int lslam_set_reloc_budget(lslam_ctx *c, int64_t bytes) {
    if (!c) return LSLAM_ERR_ARG;
    c->reloc_budget = bytes > 0 ? (size_t)bytes : default_reloc_budget();
    return LSLAM_OK;
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
