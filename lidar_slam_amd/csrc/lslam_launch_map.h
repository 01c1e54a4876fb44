// Host side, part 3 (included by lslam_launch.h between the scan pipeline's launchers and its entry
// points: see there for why it stands at that place): the map side.  What its entry points share (the
// entry frame, the outputs' registration, the small rules), then per feature the params check, the
// launcher and the required pointers, from the correlative search to the field fusion, then the entry
// points.
#pragma once

// ---- what the map-side entry points share ----

static int map_err(int code, const char *who, const char *what) {
    return set_err(code, (std::string(who) + ": " + what).c_str());
}

// A batch's required pointers, inputs then outputs, each list ending at its first empty slot (so at
// most 11 and 15 names), with the batch's size.  Optional pointers stay out.  The entry frame tests the
// pointers and names them in its message from this one list.
struct Req {
    const char *name;
    const void *p;
};
struct Reqs {
    Req in[12], out[16];
    int n = 0;
    const char *n_name = "n_robots";
};

// a's lists with b's behind them: a batch that embeds another one's (lslam_map_fuse, lslam_field_fuse)
static Reqs reqs_join(Reqs a, const Reqs &b) {
    const Req *from[2] = {b.in, b.out};
    Req *to[2] = {a.in, a.out};
    for (int i = 0; i < 2; i++) {
        while (to[i]->name) to[i]++;
        while (from[i]->name) *to[i]++ = *from[i]++;
    }
    return a;
}

// "who: missing <kind> (every name of the list)" when one of the list's pointers is NULL
static int reqs_missing(const char *who, const char *kind, const Req *list) {
    bool missing = false;
    for (const Req *r = list; r->name; r++) missing |= !r->p;
    if (!missing) return LSLAM_OK;
    std::string s = std::string("missing ") + kind + " (";
    for (const Req *r = list; r->name; r++) s += std::string(r == list ? "" : ", ") + r->name;
    return map_err(LSLAM_ERR_ARG, who, (s + ")").c_str());
}

// The frame of every map-side entry point, behind its params checks.  The order is an interface: what
// needs no device comes first, the context behind it (the tests call without one and read the message),
// and the context is asked for before an empty batch returns.  extra: the entry's own checks of a batch
// that is not empty.  launch: a lambda written in the entry point that calls its plain launcher (a kernel
// launched from inside a template would take another place in the code object).
template <typename B, typename Extra, typename Launch>
static int map_entry(const char *who, lslam_ctx *c, const B *b, Reqs (*reqs)(const B &), Extra extra, Launch launch) {
    if (!b) return map_err(LSLAM_ERR_ARG, who, "batch is NULL");
    const Reqs r = reqs(*b);
    if (r.n < 0) return map_err(LSLAM_ERR_ARG, who, (std::string("negative ") + r.n_name).c_str());
    if (r.n > 0) {
        int st = reqs_missing(who, "input", r.in);
        if (st || (st = reqs_missing(who, "output", r.out)) || (st = extra())) return st;
    }
    if (!c) return map_err(LSLAM_ERR_ARG, who, "ctx is NULL");
    if (r.n == 0) return LSLAM_OK;
    HIPCHK(hipSetDevice(c->device));
    return launch();
}
template <typename B, typename Launch>
static int map_entry(const char *who, lslam_ctx *c, const B *b, Reqs (*reqs)(const B &), Launch launch) {
    return map_entry(who, c, b, reqs, [] { return (int)LSLAM_OK; }, launch);
}

// A launcher's outputs, for the hazard planner (a NULL optional adds nothing); one marked `zero` is
// first cleared on the ctx stream, so a launcher that zeroes calls this before its kernel.
struct Out {
    const void *p;
    size_t bytes;
    bool zero = false;
};
static int note_outs(lslam_ctx *c, std::initializer_list<Out> outs) {
    for (const Out &o : outs) {
        if (o.zero) HIPCHK(hipMemsetAsync(const_cast<void *>(o.p), 0, o.bytes, c->stream));
        c->hz.outs.add(o.p, o.bytes);
    }
    return LSLAM_OK;
}

// rows of w int16 cells at a (and at b) lie on 16-byte groups: the kernels' 8-cell loads and stores
static bool groups16(int w, const void *a, const void *b = nullptr) {
    return w % 8 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

// Slices of a robot's work: enough for two workgroups per CU when the n robots alone do not give them,
// at most cap.
static int64_t slices_for(const lslam_ctx *c, int64_t n, int64_t cap) {
    return std::min<int64_t>(std::max<int64_t>((2 * (int64_t)c->n_cus + n - 1) / n, 1), cap);
}

// a launch's workgroups must fit the grid's 31 bits
static int check_blocks(const char *who, int64_t blocks) {
    if (blocks >= ((int64_t)1 << 31)) return map_err(LSLAM_ERR_UNSUPPORTED, who, "too many robots in one call");
    return LSLAM_OK;
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
// or the context's scratch; vol = its bytes).  Slices: by slices_for (what the LDS allows), at most one
// per rotation; each slice rebuilds G.
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
    const int64_t ns = slices_for(c, n, g.Nth);
    g.per_slice = (int)((g.Nth + ns - 1) / ns);
    g.n_slices = (g.Nth + g.per_slice - 1) / g.per_slice;
    int st = check_blocks(who, (int64_t)n * g.n_slices);
    if (st) return st;
    vol = (size_t)n * g.Nth * g.Nt * g.Nt * 4;
    g.scores = scores;
    if (!scores) {
        if ((st = c->mscr.ensure(c, vol, (std::string(who) + " scores").c_str()))) return st;
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

static Reqs match_reqs(const lslam_match_batch &b) {
    return {{{"ref_xy", b.ref_xy}, {"ref_off", b.ref_off}, {"cur_xy", b.cur_xy}, {"cur_off", b.cur_off}, {"rot", b.rot}},
            {{"delta", b.delta}, {"best", b.best}, {"n_valid", b.n_valid}, {"flags", b.flags}},
            b.n_scans,
            "n_scans"};
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
    return note_outs(c, {{b->delta, S * 24}, {b->best, S * 16}, {b->n_valid, S * 8}, {b->flags, S * 4}, {b->scores, vol},
                         {k.write_u ? b->ukf_u : nullptr, S * 16}});
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

static Reqs grid_reqs(const lslam_grid_batch &b) {
    return {{{"xy", b.xy}, {"pt_off", b.pt_off}, {"pose", b.pose}, {"origin", b.origin}},
            {{"logodds", b.logodds}, {"rot", b.rot}, {"n_used", b.n_used}, {"flags", b.flags}},
            b.n_robots};
}

template <int T, int WAVE_RAY>
static int launch_grid_form(lslam_ctx *c, GridArgs &k) {
    k.ntile = (k.grid_w + T - 1) / T;
    const int64_t blocks = (int64_t)k.b.n_robots * k.ntile * k.ntile;
    int st = check_blocks("grid", blocks);
    if (st) return st;
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
    k.vec = groups16(p->grid_w, b->logodds);
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
    return note_outs(c, {{b->logodds, R * (size_t)p->grid_w * (size_t)p->grid_w * 2}, {b->rot, R * 16}, {b->n_used, R * 8},
                         {b->flags, R * 4}});
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

static Reqs mapmatch_reqs(const lslam_mapmatch_batch &b) {
    return {{{"xy", b.xy}, {"pt_off", b.pt_off}, {"pose", b.pose}, {"origin", b.origin}, {"logodds", b.logodds}, {"rot", b.rot}},
            {{"pose_out", b.pose_out}, {"delta", b.delta}, {"best", b.best}, {"n_valid", b.n_valid}, {"rot0", b.rot0},
             {"flags", b.flags}},
            b.n_robots};
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
    k.vec = groups16(g->grid_w, b->logodds);
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
static int mapmatch_outs(lslam_ctx *c, const lslam_mapmatch_batch *b, size_t vol) {
    const size_t R = (size_t)b->n_robots;
    return note_outs(c, {{b->pose_out, R * 24}, {b->delta, R * 24}, {b->best, R * 16}, {b->n_valid, R * 8}, {b->rot0, R * 16},
                         {b->flags, R * 4}, {b->scores, vol}});
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
    return mapmatch_outs(c, b, vol);
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

static Reqs mapfuse_reqs(const lslam_mapfuse_batch &b) {
    return reqs_join(mapmatch_reqs(b.m), {{{"P", b.P}}, {{"P_out", b.P_out}, {"z", b.z}, {"Rm", b.Rm}, {"nis", b.nis}}});
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
    if ((st = mapmatch_outs(c, &b->m, vol))) return st;
    return note_outs(c, {{b->P_out, R * 72}, {b->z, R * 24}, {b->Rm, R * 72}, {b->nis, R * 8}, {b->moments, R * 80}});
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

static Reqs reloc_reqs(const lslam_reloc_batch &b) {
    return {{{"xy", b.xy}, {"pt_off", b.pt_off}, {"origin", b.origin}, {"logodds", b.logodds}, {"rot", b.rot},
             {"head_rot", b.head_rot}},
            {{"n_occ", b.n_occ}, {"n_used", b.n_used}, {"cand", b.cand}, {"cand_pose", b.cand_pose}, {"fine_pose", b.fine_pose},
             {"fine_delta", b.fine_delta}, {"fine_best", b.fine_best}, {"fine_nvalid", b.fine_nvalid},
             {"fine_rot0", b.fine_rot0}, {"fine_flags", b.fine_flags}, {"result", b.result}, {"flags", b.flags},
             {"pose_out", b.pose_out}},
            b.n_robots};
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

// The kernels' arguments of a relocalisation but for the chunk's (r0, vol, keys) and the slicing; returns
// the cells of one robot's coarse volume.
static size_t reloc_args(const lslam_reloc_batch *b, const lslam_grid_params *g, const lslam_mapmatch_params *m,
                         const lslam_reloc_params *q, RelocArgs &k) {
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
    k.K = q->n_cand;
    k.occ_min = m->occ_min;
    k.ambig = q->ambig_permille;
    k.nspan = (k.Wc + 31) / 32;
    k.RW = reloc_row_dwords(k.Wc, k.nspan);
    k.vec = groups16(g->grid_w, b->logodds);
    k.nbh = (k.Wc * k.Wc + RELOC_PEAK_BLOCK - 1) / RELOC_PEAK_BLOCK;
    k.nblk = k.n_head * k.nbh;
    return (size_t)k.n_head * k.Wc * k.Wc;
}

// the fine stage's batch but for the rank's arrays
static void reloc_fine_batch(const lslam_reloc_batch *b, lslam_mapmatch_batch &mb) {
    memset(&mb, 0, sizeof(mb));
    mb.n_robots = b->n_robots;
    mb.xy = b->xy;
    mb.pt_off = b->pt_off;
    mb.origin = b->origin;
    mb.logodds = b->logodds;
    mb.rot = b->rot;
}

// K times the scan-to-map matcher (launch_mapmatch_kernels), rank j's arrays in the place of the batch's
static int launch_reloc_fine(lslam_ctx *c, const lslam_reloc_batch *b, const lslam_grid_params *g,
                             const lslam_mapmatch_params *m, int K, lslam_mapmatch_batch &mb) {
    const size_t Rz = (size_t)b->n_robots;
    MapMatchArgs mk;
    size_t mvol;
    for (int j = 0; j < K; j++) {
        mb.pose = b->cand_pose + (size_t)j * Rz * 3;
        mb.pose_out = b->fine_pose + (size_t)j * Rz * 3;
        mb.delta = b->fine_delta + (size_t)j * Rz * 3;
        mb.best = b->fine_best + (size_t)j * Rz * 4;
        mb.n_valid = b->fine_nvalid + (size_t)j * Rz * 2;
        mb.rot0 = b->fine_rot0 + (size_t)j * Rz * 2;
        mb.flags = b->fine_flags + (size_t)j * Rz;
        int st = mapmatch_args(c, &mb, g, m, mk, mvol);  // (the stream orders the reuse of its scratch)
        if (st || (st = launch_mapmatch_kernels(c, mk))) return st;
    }
    return LSLAM_OK;
}

// a relocalisation's outputs, for the hazard planner
static int reloc_outs(lslam_ctx *c, const lslam_reloc_batch *b, int K, size_t cells) {
    const size_t Rz = (size_t)b->n_robots, KR = (size_t)K * Rz;
    return note_outs(c, {{b->n_occ, Rz * 4}, {b->n_used, Rz * 4}, {b->cand, KR * 16}, {b->cand_pose, KR * 24},
                         {b->fine_pose, KR * 24}, {b->fine_delta, KR * 24}, {b->fine_best, KR * 16}, {b->fine_nvalid, KR * 8},
                         {b->fine_rot0, KR * 16}, {b->fine_flags, KR * 4}, {b->result, Rz * 32}, {b->flags, Rz * 4},
                         {b->pose_out, Rz * 24}, {b->P_out, Rz * 72}, {b->coarse_scores, Rz * cells * 4}});
}

// LSLAM_RELOC_STAGES=coarse (tools/relocbench.py): the coarse stage alone; the fine outputs, result, flags
// and pose_out are not written
static bool reloc_coarse_only() {
    const char *stages = getenv("LSLAM_RELOC_STAGES");
    return stages && !strcmp(stages, "coarse");
}

// The coarse stage in chunks of robots under the context's byte budget (search, peaks, the K best),
// then the fine stage, then the selection.  LSLAM_RELOC_FORM=add (tools/relocbench.py) selects the search
// form that was measured and dropped.
static int launch_reloc(lslam_ctx *c, const lslam_reloc_batch *b, const lslam_grid_params *g,
                        const lslam_mapmatch_params *m, const lslam_reloc_params *q) {
    const int R = b->n_robots, K = q->n_cand;
    RelocArgs k;
    const size_t cells = reloc_args(b, g, m, q, k);
    if (const char *e = getenv("LSLAM_RELOC_FORM"))
        if (!strcmp(e, "add")) k.form = 1;
    const int nc = (int)std::min<size_t>((size_t)R, std::max<size_t>(1, c->reloc_budget / (cells * 4)));
    const int64_t ns = slices_for(c, nc, k.n_head);
    k.per_slice = (int)((k.n_head + ns - 1) / ns);
    k.n_slices = (k.n_head + k.per_slice - 1) / k.per_slice;
    int st = check_blocks("reloc", (int64_t)nc * k.nblk);
    if (st) return st;
    const size_t keys_bytes = ((size_t)nc * k.nblk * K * 8 + 255) & ~(size_t)255;
    if ((st = c->rscr.ensure(c, keys_bytes + (b->coarse_scores ? 0 : (size_t)nc * cells * 4), "reloc scratch"))) return st;
    k.keys = c->rscr.as<unsigned long long>();
    // the fine stage's batch of rank 0: its scratch is grown here, before the timer and the first launch
    lslam_mapmatch_batch mb;
    reloc_fine_batch(b, mb);
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
    if (reloc_coarse_only()) return timer_end(c, LSLAM_K_RELOC);
    if ((st = launch_reloc_fine(c, b, g, m, K, mb))) return st;
    hipLaunchKernelGGL(reloc_select_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_RELOC))) return st;
    return reloc_outs(c, b, K, cells);
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

static Reqs raycast_reqs(const lslam_raycast_batch &b) {
    return {{{"xy", b.xy}, {"pt_off", b.pt_off}, {"pose", b.pose}, {"origin", b.origin}, {"logodds", b.logodds}},
            {{"cls", b.cls}, {"counts", b.counts}, {"rot", b.rot}, {"flags", b.flags}},
            b.n_robots};
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

// One workgroup per (robot, slice of its points), by slices_for: slices exist so that a few robots
// still fill the chip.  The HBM form ships: in the bench room's grids it is the faster one at 4096
// robots.  LSLAM_RAYCAST_FORM=lds (tools/raycastbench.py, the tests) selects the LDS
// form where the largest window's codes fit its budget.
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
    k.vec = groups16(g->grid_w, b->logodds);
    const int win = raycast_window(k.Rc, k.grid_w);
    k.Sd = raycast_row_dwords(win);
    int hbm = 1;
    if (const char *e = getenv("LSLAM_RAYCAST_FORM"))
        if (!strcmp(e, "lds") && raycast_lds_bytes(win) <= RAYCAST_LDS_BUDGET) hbm = 0;
    const int64_t n = b->n_robots;
    k.n_slices = (int)slices_for(c, n, RAYCAST_MAX_SLICES);
    int st = check_blocks("raycast", n * k.n_slices);
    if (st) return st;
    if ((st = timer_begin(c, LSLAM_K_RAYCAST))) return st;
    // (cls and stop are as long as pt_off, on the device, says: per-point outputs that no producer reads)
    if ((st = note_outs(c, {{b->counts, (size_t)n * 32, true}, {b->rot, (size_t)n * 16}, {b->flags, (size_t)n * 4}})))
        return st;
    st = hbm ? launch_raycast_form<1>(c, k, 32) : launch_raycast_form<0>(c, k, raycast_lds_bytes(win));
    if (st) return st;
    return timer_end(c, LSLAM_K_RAYCAST);
}

// ---- grid recentre (lslam_recentre.h) ----

static int recentre_check_params(const lslam_recentre_params *p, const lslam_grid_params *g) {
    if (!p) return set_err(LSLAM_ERR_ARG, "recentre: params is NULL");
    if (p->margin < 0 || p->margin > g->grid_w / 2)
        return set_err(LSLAM_ERR_ARG, "recentre: margin must be in [0, grid_w / 2]");
    if (p->quantum < 1 || p->quantum > 64) return set_err(LSLAM_ERR_ARG, "recentre: quantum must be in [1, 64]");
    return LSLAM_OK;
}

static Reqs recentre_reqs(const lslam_recentre_batch &b) {
    return {{{"pose", b.pose}, {"origin", b.origin}, {"logodds", b.logodds}}, {{"shift", b.shift}, {"flags", b.flags}}, b.n_robots};
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
    k.vec = groups16(g->grid_w, b->logodds);
    // (its own bound, below check_blocks': recentre_blocks rounds the robots up)
    if (b->n_robots > (1 << 30)) return map_err(LSLAM_ERR_UNSUPPORTED, "recentre", "too many robots in one call");
    int st = timer_begin(c, LSLAM_K_RECENTRE);
    if (st) return st;
    if (k.vec && p->quantum % 8 == 0)
        hipLaunchKernelGGL(recentre_kernel<0>, dim3((unsigned)recentre_blocks(b->n_robots)), dim3(RECENTRE_TPB), 0, c->stream, k);
    else
        hipLaunchKernelGGL(recentre_kernel<1>, dim3((unsigned)recentre_blocks(b->n_robots)), dim3(RECENTRE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_RECENTRE))) return st;
    const size_t R = (size_t)b->n_robots;
    return note_outs(c, {{b->logodds, R * (size_t)g->grid_w * (size_t)g->grid_w * 2}, {b->origin, R * 16}, {b->shift, R * 8},
                         {b->flags, R * 4}});
}

// ---- the paged rolling grid (lslam_page.h) ----

static int page_check_params(const lslam_page_params *pp) {
    if (!pp) return set_err(LSLAM_ERR_ARG, "page: params is NULL");
    if (pp->canvas_w < 16 || pp->canvas_w > 2048) return set_err(LSLAM_ERR_ARG, "page: canvas_w must be in [16, 2048]");
    return LSLAM_OK;
}

// the two batches of a paged recentre, and the window of a flush or a load with its page batch: what
// the entry frame takes as one batch
struct PagedBatch {
    lslam_recentre_batch b;
    lslam_page_batch pg;
};
struct PageWindowBatch {
    lslam_page_batch pg;
    const int16_t *logodds;
    bool store;  // flush: the window is the input and the canvas the output
};

static Reqs paged_reqs(const PagedBatch &x) {
    const Reqs pg = {{{"win", x.pg.win}, {"canvas", x.pg.canvas}}, {{"moved", x.pg.moved}, {"page flags", x.pg.flags}}, x.pg.n_robots};
    Reqs r = reqs_join(recentre_reqs(x.b), pg);
    // (one size rules both: a negative one of either is reported, and an empty call is empty in both)
    r.n = x.b.n_robots < 0 || x.pg.n_robots < 0 ? -1 : std::max(x.b.n_robots, x.pg.n_robots);
    return r;
}

static Reqs page_window_reqs(const PageWindowBatch &x) {
    if (x.store) return {{{"logodds", x.logodds}, {"win", x.pg.win}}, {{"canvas", x.pg.canvas}, {"moved", x.pg.moved}}, x.pg.n_robots};
    return {{{"canvas", x.pg.canvas}, {"win", x.pg.win}}, {{"logodds", x.logodds}, {"moved", x.pg.moved}}, x.pg.n_robots};
}

static int page_check_overlap(const lslam_page_batch &pg, const void *logodds, const lslam_grid_params *g, const lslam_page_params *pp) {
    const size_t R = (size_t)pg.n_robots;
    if (ranges_overlap(logodds, R * (size_t)g->grid_w * (size_t)g->grid_w * 2, pg.canvas, R * (size_t)pp->canvas_w * (size_t)pp->canvas_w * 2))
        return set_err(LSLAM_ERR_ARG, "page: canvas overlaps logodds");
    return LSLAM_OK;
}

// One workgroup per robot, as launch_recentre and under its timing slot: the call is a whole recentre.
static int launch_recentre_paged(lslam_ctx *c, const PagedBatch &x, const lslam_grid_params *g, const lslam_recentre_params *p,
                                 const lslam_page_params *pp) {
    PageArgs k;
    memset(&k, 0, sizeof(k));
    k.pose = x.b.pose, k.origin = x.b.origin, k.logodds = x.b.logodds, k.shift = x.b.shift, k.flags = x.b.flags;
    k.canvas = x.pg.canvas, k.win = x.pg.win, k.moved = x.pg.moved, k.pflags = x.pg.flags;
    k.cell = g->cell;
    k.inv = 1.0 / g->cell;
    k.n_robots = x.b.n_robots;
    k.grid_w = g->grid_w;
    k.margin = p->margin;
    k.quantum = p->quantum;
    k.band_rows = recentre_band_rows(g->grid_w);
    k.vec = groups16(g->grid_w, x.b.logodds);
    k.canvas_w = pp->canvas_w;
    k.pvec = k.vec && groups16(pp->canvas_w, x.pg.canvas);
    if (x.b.n_robots > (1 << 30)) return map_err(LSLAM_ERR_UNSUPPORTED, "page", "too many robots in one call");
    int st = timer_begin(c, LSLAM_K_RECENTRE);
    if (st) return st;
    const dim3 blocks((unsigned)recentre_blocks(x.b.n_robots));
    if (k.vec && p->quantum % 8 == 0) hipLaunchKernelGGL(page_recentre_kernel<0>, blocks, dim3(PAGE_TPB), 0, c->stream, k);
    else hipLaunchKernelGGL(page_recentre_kernel<1>, blocks, dim3(PAGE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_RECENTRE))) return st;
    const size_t R = (size_t)x.b.n_robots, W = (size_t)g->grid_w, Cw = (size_t)pp->canvas_w;
    return note_outs(c, {{x.b.logodds, R * W * W * 2}, {x.b.origin, R * 16}, {x.b.shift, R * 8}, {x.b.flags, R * 4},
                         {x.pg.canvas, R * Cw * Cw * 2}, {x.pg.win, R * 8}, {x.pg.moved, R * 8}, {x.pg.flags, R * 4}});
}

// A robot's rows in slices (slices_for), each of whole rows.
static int launch_page_window(lslam_ctx *c, const PageWindowBatch &x, const lslam_grid_params *g, const lslam_page_params *pp) {
    PageWindowArgs k;
    memset(&k, 0, sizeof(k));
    k.pg = x.pg;
    k.logodds = const_cast<int16_t *>(x.logodds);
    k.grid_w = g->grid_w;
    k.canvas_w = pp->canvas_w;
    k.vec = groups16(g->grid_w, x.logodds) && groups16(pp->canvas_w, x.pg.canvas);
    const int64_t n = x.pg.n_robots;
    const int want = (int)slices_for(c, n, g->grid_w);
    k.rows = (g->grid_w + want - 1) / want;
    k.n_slices = (g->grid_w + k.rows - 1) / k.rows;
    int st = check_blocks("page", n * k.n_slices);
    if (st) return st;
    const dim3 blocks((unsigned)(n * k.n_slices));
    if (x.store) hipLaunchKernelGGL(page_window_kernel<true>, blocks, dim3(PAGE_TPB), 0, c->stream, k);
    else hipLaunchKernelGGL(page_window_kernel<false>, blocks, dim3(PAGE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
    const size_t R = (size_t)n, W = (size_t)g->grid_w, Cw = (size_t)pp->canvas_w;
    if (x.store) return note_outs(c, {{x.pg.canvas, R * Cw * Cw * 2}, {x.pg.moved, R * 8}});
    return note_outs(c, {{x.logodds, R * W * W * 2}, {x.pg.moved, R * 8}});
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

static Reqs dist_reqs(const lslam_dist_batch &b) {
    return {{{"logodds", b.logodds}}, {{"d2", b.d2}, {"n_src", b.n_src}, {"flags", b.flags}}, b.n_robots};
}

// The band of rows of a workgroup: all of a robot's rows when the robots alone fill the chip, else so
// many bands as slices_for gives (at most DIST_MAX_SLICES per robot), in whole groups of DIST_NW rows;
// then shrunk until the workgroup's LDS leaves room for two on a CU, or at least fits one.  0: not
// even a band of DIST_NW rows fits.
static int dist_band_rows(const lslam_ctx *c, int W, int hal, int64_t n_robots) {
    const int64_t want = slices_for(c, n_robots, DIST_MAX_SLICES);
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
    k.band = dist_band_rows(c, k.grid_w, k.hal, b->n_robots);
    if (!k.band) return set_err(LSLAM_ERR_UNSUPPORTED, "dist: the bitmap of 2 d_max rows of this grid_w does not fit LDS");
    k.n_slices = (k.grid_w + k.band - 1) / k.band;
    k.nblk = dist_blocks(k.grid_w, k.band, k.hal);
    const int lds = dist_lds_bytes(k.grid_w, k.nblk);
    const int64_t n = b->n_robots;
    int st = check_blocks("dist", n * k.n_slices);
    if (st) return st;
    if ((st = note_outs(c, {{b->d2, (size_t)n * (size_t)g->grid_w * (size_t)g->grid_w * 2}, {b->n_src, (size_t)n * 4, true},
                            {b->flags, (size_t)n * 4}})))
        return st;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)b->flags, LSLAM_DIST_EMPTY, (size_t)n, c->stream));
    if (groups16(g->grid_w, b->logodds, b->d2))
        hipLaunchKernelGGL(dist_kernel<8>, dim3((unsigned)(n * k.n_slices)), dim3(DIST_TPB), lds, c->stream, k);
    else hipLaunchKernelGGL(dist_kernel<1>, dim3((unsigned)(n * k.n_slices)), dim3(DIST_TPB), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

static int fieldscore_check_params(const lslam_fieldscore_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "fieldscore: params is NULL");
    if (p->trunc2 < 1 || p->trunc2 > 65025) return set_err(LSLAM_ERR_ARG, "fieldscore: trunc2 must be in [1, 65025]");
    if (p->near2 < 0 || p->near2 > 65025) return set_err(LSLAM_ERR_ARG, "fieldscore: near2 must be in [0, 65025]");
    if (p->off2 < 0 || p->off2 > 65025) return set_err(LSLAM_ERR_ARG, "fieldscore: off2 must be in [0, 65025]");
    return LSLAM_OK;
}

static Reqs fieldscore_reqs(const lslam_fieldscore_batch &b) {
    return {{{"xy", b.xy}, {"pt_off", b.pt_off}, {"pose", b.pose}, {"origin", b.origin}, {"d2", b.d2}},
            {{"rot", b.rot}, {"stats", b.stats}, {"clear2", b.clear2}, {"flags", b.flags}},
            b.n_robots};
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
    const int64_t n = b->n_robots;
    k.n_slices = (int)slices_for(c, n, FIELDSCORE_MAX_SLICES);
    int st = check_blocks("fieldscore", n * k.n_slices);
    if (st) return st;
    if ((st = note_outs(c, {{b->rot, (size_t)n * 16}, {b->stats, (size_t)n * 32, true}, {b->clear2, (size_t)n * 4},
                            {b->flags, (size_t)n * 4}})))
        return st;
    hipLaunchKernelGGL(fieldscore_kernel, dim3((unsigned)(n * k.n_slices)), dim3(FIELDSCORE_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
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

static Reqs fieldalign_reqs(const lslam_fieldalign_batch &b) {
    return {{{"xy", b.xy}, {"pt_off", b.pt_off}, {"pose", b.pose}, {"origin", b.origin}, {"d2", b.d2}},
            {{"pose_out", b.pose_out}, {"trace", b.trace}, {"normal", b.normal}, {"n_used", b.n_used}, {"iters", b.iters},
             {"flags", b.flags}},
            b.n_robots};
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
    int st = note_outs(c, {{b->pose_out, n * 24}, {b->trace, n * rows * 40, true}, {b->normal, n * 80, true},
                           {b->n_used, n * 12, true}, {b->iters, n * 4, true}, {b->flags, n * 4}});
    if (st) return st;
    const unsigned blocks = (unsigned)((n + FIELDALIGN_RPB - 1) / FIELDALIGN_RPB);
    hipLaunchKernelGGL(fieldalign_kernel, dim3(blocks), dim3(FIELDALIGN_TPB), 0, c->stream, k);
    HIPCHK(hipGetLastError());
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

static Reqs fieldfuse_reqs(const lslam_fieldfuse_batch &b) {
    return reqs_join(fieldalign_reqs(b.a), {{{"P", b.P}}, {{"P_out", b.P_out}, {"z", b.z}, {"info", b.info}, {"info_f", b.info_f},
                                                            {"s2", b.s2}, {"nis", b.nis}}});
}

// fieldfuse_kernel's place in the code object (lslam_launch.h, at this file's include): the scan entry
// points' instantiations, named here, take theirs ahead of launch_fieldfuse's launch.
static int (*const scan_entries_first[])(lslam_ctx *, const KArgs &, int, int) = {run_scan_kernel<MODE_ASSOC>,
                                                                                  run_scan_kernel<MODE_UKF>};

// launch_fieldalign with pose_out := z, then one thread per robot for steps 5-11.
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
    return note_outs(c, {{b->a.pose_out, n * 24}, {b->P_out, n * 72}, {b->info, n * 72}, {b->info_f, n * 72}, {b->s2, n * 8},
                         {b->nis, n * 8}});
}

// ---- closure gating (lslam_posegate.h) ----
// Between launch_fieldfuse and launch_posegraph: a kernel template is emitted where it is first used, and
// tests/test_posegraph_budget.py holds the pose-graph kernel to the place -12 of the code object.  Here the one
// instantiation stands directly ahead of it; the kernels behind it keep their bytes.

static int posegate_check_params(const lslam_posegate_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "posegate: params is NULL");
    if (p->max_nodes < 2 || p->max_nodes > POSEGRAPH_MAX_NODES) return set_err(LSLAM_ERR_ARG, "posegate: max_nodes must be in [2, 64]");
    if (p->max_edges < 1 || p->max_edges > POSEGRAPH_MAX_EDGES) return set_err(LSLAM_ERR_ARG, "posegate: max_edges must be in [1, 1024]");
    if (p->max_cand < 1 || p->max_cand > POSEGATE_MAX_CAND) return set_err(LSLAM_ERR_ARG, "posegate: max_cand must be in [1, 64]");
    if (!(p->damp_t >= 0.0) || !std::isfinite(p->damp_t)) return set_err(LSLAM_ERR_ARG, "posegate: damp_t must be >= 0 and finite");
    if (!(p->damp_r >= 0.0) || !std::isfinite(p->damp_r)) return set_err(LSLAM_ERR_ARG, "posegate: damp_r must be >= 0 and finite");
    if (!(p->nis_max > 0)) return set_err(LSLAM_ERR_ARG, "posegate: nis_max must be > 0 (+inf: no gate)");
    if (p->append != 0 && p->append != 1) return set_err(LSLAM_ERR_ARG, "posegate: append must be 0 or 1");
    return LSLAM_OK;
}

static Reqs posegate_reqs(const lslam_posegate_batch &b) {
    return {{{"n_nodes", b.n_nodes}, {"n_edges", b.n_edges}, {"pose", b.pose}, {"edge_ij", b.edge_ij}, {"edge_z", b.edge_z},
             {"edge_info", b.edge_info}, {"n_cand", b.n_cand}, {"cand_ij", b.cand_ij}, {"cand_z", b.cand_z},
             {"cand_info", b.cand_info}},
            {{"trace", b.trace}, {"chi2", b.chi2}, {"cand_nis", b.cand_nis}, {"cand_err", b.cand_err}, {"cand_cov", b.cand_cov},
             {"cand_flags", b.cand_flags}, {"flags", b.flags}},
            b.n_graphs,
            "n_graphs"};
}

// One workgroup per graph; the LDS is sized from max_nodes, max_edges, max_cand and the candidates of a block.
static int launch_posegate(lslam_ctx *c, const lslam_posegate_batch *b, const lslam_posegate_params *p) {
    PoseGateArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.p = *p;
    k.slots = posegate_slots(p->max_nodes, p->max_edges, p->max_cand);
    const int lds = posegate_lds_bytes(p->max_nodes, p->max_edges, p->max_cand, k.slots);
    if (lds > POSEGRAPH_LDS_MAX) return set_err(LSLAM_ERR_UNSUPPORTED, "posegate: max_nodes, max_edges and max_cand do not fit LDS");
    const size_t n = (size_t)b->n_graphs, Nc = (size_t)p->max_nodes, Ec = (size_t)p->max_edges, Cc = (size_t)p->max_cand;
    int st = check_blocks("posegate", (int64_t)b->n_graphs);
    if (st) return st;
    // (flags is written for every graph; the rest is zeros where the kernel writes nothing.  Without append the edge
    // arrays and n_edges are only read; with it they are outputs too.)
    if ((st = note_outs(c, {{b->trace, n * Nc * 16, true}, {b->chi2, n * 8, true}, {b->cand_nis, n * Cc * 8, true},
                            {b->cand_err, n * Cc * 24, true}, {b->cand_cov, n * Cc * 48, true}, {b->cand_flags, n * Cc * 4, true},
                            {b->flags, n * 4}})))
        return st;
    if (p->append && (st = note_outs(c, {{b->n_edges, n * 4}, {b->edge_ij, n * Ec * 8}, {b->edge_z, n * Ec * 24},
                                         {b->edge_info, n * Ec * 48}})))
        return st;
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(posegate_kernel<0>); });
    hipLaunchKernelGGL(posegate_kernel<0>, dim3((unsigned)n), dim3(POSEGATE_TPB), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// ---- pose-graph optimisation (lslam_posegraph.h) ----
// Between launch_fieldfuse and launch_gridpoints: a kernel template is emitted where it is first used, and
// tests/test_gridpoints_budget.py holds the four gridpoints kernels to the places -11..-8 of the code object.  Here
// the one instantiation stands directly ahead of those four; the kernels behind it keep their bytes.

static int posegraph_check_params(const lslam_posegraph_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "posegraph: params is NULL");
    if (p->max_nodes < 2 || p->max_nodes > POSEGRAPH_MAX_NODES) return set_err(LSLAM_ERR_ARG, "posegraph: max_nodes must be in [2, 64]");
    if (p->max_edges < 1 || p->max_edges > POSEGRAPH_MAX_EDGES) return set_err(LSLAM_ERR_ARG, "posegraph: max_edges must be in [1, 1024]");
    if (p->n_iter < 0 || p->n_iter > POSEGRAPH_MAX_ITER) return set_err(LSLAM_ERR_ARG, "posegraph: n_iter must be in [0, 32]");
    if (!(p->damp_t >= 0.0) || !std::isfinite(p->damp_t)) return set_err(LSLAM_ERR_ARG, "posegraph: damp_t must be >= 0 and finite");
    if (!(p->damp_r >= 0.0) || !std::isfinite(p->damp_r)) return set_err(LSLAM_ERR_ARG, "posegraph: damp_r must be >= 0 and finite");
    if (!(p->eps_t >= 0.0) || !std::isfinite(p->eps_t)) return set_err(LSLAM_ERR_ARG, "posegraph: eps_t must be >= 0 and finite");
    if (!(p->eps_r >= 0.0) || !std::isfinite(p->eps_r)) return set_err(LSLAM_ERR_ARG, "posegraph: eps_r must be >= 0 and finite");
    return LSLAM_OK;
}

static Reqs posegraph_reqs(const lslam_posegraph_batch &b) {
    return {{{"n_nodes", b.n_nodes}, {"n_edges", b.n_edges}, {"pose", b.pose}, {"edge_ij", b.edge_ij}, {"edge_z", b.edge_z},
             {"edge_info", b.edge_info}},
            {{"pose_out", b.pose_out}, {"trace", b.trace}, {"chi2", b.chi2}, {"edge_chi2", b.edge_chi2}, {"iters", b.iters},
             {"flags", b.flags}},
            b.n_graphs,
            "n_graphs"};
}

// One workgroup per graph; the LDS is sized from max_nodes and max_edges.
static int launch_posegraph(lslam_ctx *c, const lslam_posegraph_batch *b, const lslam_posegraph_params *p) {
    PoseGraphArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.p = *p;
    const int lds = posegraph_lds_bytes(p->max_nodes, p->max_edges);
    if (lds > POSEGRAPH_LDS_MAX) return set_err(LSLAM_ERR_UNSUPPORTED, "posegraph: max_nodes and max_edges do not fit LDS");
    const size_t n = (size_t)b->n_graphs, Nc = (size_t)p->max_nodes, Ec = (size_t)p->max_edges, rows = (size_t)p->n_iter + 1;
    int st = check_blocks("posegraph", (int64_t)b->n_graphs);
    if (st) return st;
    // (pose_out and flags are written for every graph; the rest is zeros where the kernel writes nothing)
    if ((st = note_outs(c, {{b->pose_out, Nc * n * 24}, {b->trace, n * rows * Nc * 16, true}, {b->chi2, n * 16, true},
                            {b->edge_chi2, n * Ec * 8, true}, {b->iters, n * 4, true}, {b->flags, n * 4}})))
        return st;
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(posegraph_kernel<0>); });
    hipLaunchKernelGGL(posegraph_kernel<0>, dim3((unsigned)n), dim3(POSEGRAPH_TPB), lds, c->stream, k);
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// ---- a map as a revolution (lslam_gridpoints.h) ----
// Between launch_fieldfuse and launch_gridmerge: a kernel template is emitted where it is first used, and
// tests/test_gridmerge_budget.py holds the merge's four kernels to the places -7..-4 of the code object.  Here the
// four instantiations stand directly ahead of those four: every other kernel keeps its bytes and its place.

static int gridpoints_check_params(const lslam_gridpoints_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "gridpoints: params is NULL");
    if (!(p->radius > 0) || !std::isfinite(p->radius)) return set_err(LSLAM_ERR_ARG, "gridpoints: radius must be > 0 and finite");
    if (p->occ_min < -32768 || p->occ_min > 32767) return set_err(LSLAM_ERR_ARG, "gridpoints: occ_min must be in [-32768, 32767]");
    if (p->cap < 1 || p->cap > 65536) return set_err(LSLAM_ERR_ARG, "gridpoints: cap must be in [1, 65536]");
    return LSLAM_OK;
}

static Reqs gridpoints_reqs(const lslam_gridpoints_batch &b) {
    return {{{"logodds", b.logodds}, {"origin", b.origin}, {"anchor", b.anchor}},
            {{"xy", b.xy}, {"pt_off", b.pt_off}, {"counts", b.counts}, {"flags", b.flags}, {"band_counts", b.band_counts}},
            b.n_robots};
}

// One wave per (robot, band of rows): eight waves a SIMD when the robots alone do not give them, at most
// GP_BANDS bands.  The memset of xy, the count pass, the write pass.
static int launch_gridpoints(lslam_ctx *c, const lslam_gridpoints_batch *b, const lslam_grid_params *g,
                             const lslam_gridpoints_params *p) {
    GridPointsArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.cell = g->cell;
    k.r2 = p->radius * p->radius;
    k.grid_w = g->grid_w;
    k.occ_min = p->occ_min;
    k.cap = p->cap;
    k.n_robots = b->n_robots;
    const int64_t n = b->n_robots;
    k.rows = gp_band_rows(g->grid_w, (int)std::min<int64_t>((32 * (int64_t)c->n_cus + n - 1) / n, GP_BANDS));
    k.n_bands = gp_bands(g->grid_w, k.rows);
    int st = check_blocks("gridpoints", n * k.n_bands);
    if (st) return st;
    if ((st = note_outs(c, {{b->xy, (size_t)n * (size_t)p->cap * 16, true}, {b->pt_off, ((size_t)n + 1) * 4}, {b->counts, (size_t)n * 16},
                            {b->flags, (size_t)n * 4}, {b->band_counts, (size_t)n * GP_BANDS * 8}})))
        return st;
    const dim3 blocks((unsigned)(n * k.n_bands));
    if (groups16(g->grid_w, b->logodds)) {
        hipLaunchKernelGGL((gridpoints_kernel<8, false>), blocks, dim3(GP_WAVE), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((gridpoints_kernel<8, true>), blocks, dim3(GP_WAVE), 0, c->stream, k);
    } else {
        hipLaunchKernelGGL((gridpoints_kernel<1, false>), blocks, dim3(GP_WAVE), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((gridpoints_kernel<1, true>), blocks, dim3(GP_WAVE), 0, c->stream, k);
    }
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// ---- map merge (lslam_gridmerge.h) ----
// Between launch_gridpoints and the relocalisation priors: a kernel template is emitted where it is first used
// (lslam_launch.h, at this file's include), and tests/test_relocprior_budget.py holds the priors' three kernels
// to the code object's end.  Here the four instantiations stand directly ahead of those three: every other kernel
// keeps its bytes and its place, and the three keep their bytes.

static int gridmerge_check_params(const lslam_gridmerge_params *p) {
    if (!p) return set_err(LSLAM_ERR_ARG, "gridmerge: params is NULL");
    if (p->src_w < 16 || p->src_w > 2048) return set_err(LSLAM_ERR_ARG, "gridmerge: src_w must be in [16, 2048]");
    if (p->n_src < 1) return set_err(LSLAM_ERR_ARG, "gridmerge: n_src must be >= 1");
    if (p->occ_min < -32768 || p->occ_min > 32767) return set_err(LSLAM_ERR_ARG, "gridmerge: occ_min must be in [-32768, 32767]");
    if (p->mode != LSLAM_MERGE_ADD && p->mode != LSLAM_MERGE_FILL)
        return set_err(LSLAM_ERR_ARG, "gridmerge: mode must be LSLAM_MERGE_ADD or LSLAM_MERGE_FILL");
    if (p->dry_run != 0 && p->dry_run != 1) return set_err(LSLAM_ERR_ARG, "gridmerge: dry_run must be 0 or 1");
    if (p->min_support < 0) return set_err(LSLAM_ERR_ARG, "gridmerge: min_support must be >= 0");
    if (p->max_contra_permille < 0 || p->max_contra_permille > 1000)
        return set_err(LSLAM_ERR_ARG, "gridmerge: max_contra_permille must be in [0, 1000]");
    return LSLAM_OK;
}

static Reqs gridmerge_reqs(const lslam_gridmerge_batch &b) {
    return {{{"src", b.src}, {"src_origin", b.src_origin}, {"dst_origin", b.dst_origin}, {"xform", b.xform}},
            {{"dst", b.dst}, {"stats", b.stats}, {"flags", b.flags}},
            b.n_pairs,
            "n_pairs"};
}

// One workgroup per (pair, slice of its tiles), by slices_for; the statistics, then the merge.
static int launch_gridmerge(lslam_ctx *c, const lslam_gridmerge_batch *b, const lslam_grid_params *g,
                            const lslam_gridmerge_params *p) {
    MergeArgs k;
    memset(&k, 0, sizeof(k));
    k.b = *b;
    k.cell = g->cell;
    k.inv = 1.0 / g->cell;
    k.grid_w = g->grid_w;
    k.src_w = p->src_w;
    k.n_src = p->n_src;
    k.occ_min = p->occ_min;
    k.l_min = g->l_min;
    k.l_max = g->l_max;
    k.fill = p->mode == LSLAM_MERGE_FILL ? 1 : 0;
    k.dry_run = p->dry_run;
    k.min_support = p->min_support;
    k.max_permille = p->max_contra_permille;
    const int64_t n = b->n_pairs;
    const int nt = merge_tiles(g->grid_w);
    k.per = merge_slice_tiles(nt, (int)slices_for(c, n, nt));
    k.n_slices = merge_slices(nt, k.per);
    int st = check_blocks("gridmerge", n * k.n_slices);
    if (st) return st;
    if ((st = note_outs(c, {{b->dst, (size_t)n * (size_t)g->grid_w * (size_t)g->grid_w * 2}, {b->stats, (size_t)n * 32, true},
                            {b->flags, (size_t)n * 4}})))
        return st;
    const dim3 blocks((unsigned)(n * k.n_slices));
    if (groups16(g->grid_w, b->dst)) {
        hipLaunchKernelGGL((gridmerge_kernel<8, false>), blocks, dim3(MERGE_TPB), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((gridmerge_kernel<8, true>), blocks, dim3(MERGE_TPB), 0, c->stream, k);
    } else {
        hipLaunchKernelGGL((gridmerge_kernel<1, false>), blocks, dim3(MERGE_TPB), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((gridmerge_kernel<1, true>), blocks, dim3(MERGE_TPB), 0, c->stream, k);
    }
    HIPCHK(hipGetLastError());
    return LSLAM_OK;
}

// ---- relocalisation priors (lslam_relocprior.h) ----
// Behind launch_fieldfuse: its three kernel templates are the newest, so they take the code object's end
// (lslam_launch.h, at this file's include).

static int relocprior_check_params(const lslam_relocprior_params *pp) {
    if (!pp) return set_err(LSLAM_ERR_ARG, "relocprior: params is NULL");
    if (!(pp->half_xy >= 0)) return set_err(LSLAM_ERR_ARG, "relocprior: half_xy must be >= 0 (+inf: no box)");
    if (!(pp->half_theta >= 0)) return set_err(LSLAM_ERR_ARG, "relocprior: half_theta must be >= 0 (+inf: every heading)");
    if (pp->clear_min2 < 0 || pp->clear_min2 > 65025) return set_err(LSLAM_ERR_ARG, "relocprior: clear_min2 must be in [0, 65025]");
    return LSLAM_OK;
}

static Reqs relocprior_reqs(const lslam_relocprior_batch &b) {
    return reqs_join(reloc_reqs(b.r), {{}, {{"n_admit", b.n_admit}, {"fine_clear2", b.fine_clear2}}});
}

// clear_d2 overlaps no output
static int relocprior_check_overlap(const lslam_relocprior_batch *b, const lslam_grid_params *g, const lslam_reloc_params *q) {
    if (!b->clear_d2) return LSLAM_OK;
    const lslam_reloc_batch &r = b->r;
    const size_t Rz = (size_t)r.n_robots, KR = (size_t)q->n_cand * Rz, Wc = (size_t)(g->grid_w / q->factor);
    const size_t bytes = Rz * (size_t)g->grid_w * (size_t)g->grid_w * 2;
    const Out outs[] = {{r.n_occ, Rz * 4}, {r.n_used, Rz * 4}, {r.cand, KR * 16}, {r.cand_pose, KR * 24}, {r.fine_pose, KR * 24},
                        {r.fine_delta, KR * 24}, {r.fine_best, KR * 16}, {r.fine_nvalid, KR * 8}, {r.fine_rot0, KR * 16},
                        {r.fine_flags, KR * 4}, {r.result, Rz * 32}, {r.flags, Rz * 4}, {r.pose_out, Rz * 24}, {r.P_out, Rz * 72},
                        {r.coarse_scores, Rz * (size_t)q->n_head * Wc * Wc * 4}, {b->n_admit, Rz * 8}, {b->fine_clear2, KR * 4}};
    for (const Out &o : outs)
        if (o.p && ranges_overlap(b->clear_d2, bytes, o.p, o.bytes)) return set_err(LSLAM_ERR_ARG, "relocprior: clear_d2 overlaps an output");
    return LSLAM_OK;
}

// launch_reloc over the admissible set: the admissible bits and headings of every robot once, then per
// chunk the volume cleared (the search leaves dead spans and skipped headings alone), the search over
// the live spans, lslam_map_relocalize's own peak and top-K kernels, its fine stage, and the selection
// with the clearance test.  With neither prior the set is everything: the plain search kernel runs, with
// no clear, between the same admissibility pass (n_admit) and selection (fine_clear2).
static int launch_relocprior(lslam_ctx *c, const lslam_relocprior_batch *pb, const lslam_grid_params *g,
                             const lslam_mapmatch_params *m, const lslam_reloc_params *q, const lslam_relocprior_params *pp) {
    const lslam_reloc_batch *b = &pb->r;
    const int R = b->n_robots, K = q->n_cand;
    RelocPriorArgs pa;
    memset(&pa, 0, sizeof(pa));
    RelocArgs &k = pa.r;
    const size_t cells = reloc_args(b, g, m, q, k);
    pa.clear_d2 = pb->clear_d2;
    pa.win_pose = pb->win_pose;
    pa.n_admit = pb->n_admit;
    pa.fine_clear2 = pb->fine_clear2;
    pa.half_xy = pp->half_xy;
    pa.half_theta = pp->half_theta;
    pa.inv = 1.0 / g->cell;
    pa.clear_min2 = pp->clear_min2;
    pa.vec_d = groups16(g->grid_w, pb->clear_d2);
    const bool prior = pb->clear_d2 || pb->win_pose;
    const int nc = (int)std::min<size_t>((size_t)R, std::max<size_t>(1, c->reloc_budget / (cells * 4)));
    const int64_t ns = slices_for(c, nc, k.n_head);
    if (prior) {
        k.n_slices = (int)ns;  // of the robot's admissible headings: the kernel divides them
    } else {  // every cell and heading is admissible: the plain search, sliced as launch_reloc slices it
        k.per_slice = (int)((k.n_head + ns - 1) / ns);
        k.n_slices = (k.n_head + k.per_slice - 1) / k.per_slice;
    }
    int st = check_blocks("relocprior", (int64_t)nc * k.nblk);
    if (st) return st;
    // the scratch: the chunk's keys, every robot's bits and headings, the chunk's volume
    const size_t ntask = (size_t)k.Wc * k.nspan;
    const size_t keys_bytes = ((size_t)nc * k.nblk * K * 8 + 255) & ~(size_t)255;
    const size_t bits_bytes = ((size_t)R * ntask * 4 + 255) & ~(size_t)255;
    const size_t heads_bytes = ((size_t)R * (k.n_head + 1) * 4 + 255) & ~(size_t)255;
    const size_t vol_off = keys_bytes + bits_bytes + heads_bytes;
    if ((st = c->rscr.ensure(c, vol_off + (b->coarse_scores ? 0 : (size_t)nc * cells * 4), "reloc scratch"))) return st;
    k.keys = c->rscr.as<unsigned long long>();
    pa.bits = (uint32_t *)(c->rscr.as<char>() + keys_bytes);
    pa.heads = (int32_t *)(c->rscr.as<char>() + keys_bytes + bits_bytes);
    lslam_mapmatch_batch mb;
    reloc_fine_batch(b, mb);
    MapMatchArgs mk;
    size_t mvol;
    if ((st = mapmatch_args(c, &mb, g, m, mk, mvol))) return st;
    static std::once_flag once;
    std::call_once(once, [] { set_max_lds(relocprior_search_kernel<0>); });
    if ((st = timer_begin(c, LSLAM_K_RELOC))) return st;
    hipLaunchKernelGGL(relocprior_admit_kernel<0>, dim3((unsigned)R), dim3(RELOCPRIOR_ADMIT_TPB), 0, c->stream, pa);
    HIPCHK(hipGetLastError());
    for (int r0 = 0; r0 < R; r0 += nc) {
        const int nr = std::min(nc, R - r0);
        k.r0 = r0;
        k.vol = b->coarse_scores ? b->coarse_scores + (size_t)r0 * cells : (int32_t *)(c->rscr.as<char>() + vol_off);
        if (prior) {
            HIPCHK(hipMemsetAsync(k.vol, 0, (size_t)nr * cells * 4, c->stream));
            hipLaunchKernelGGL(relocprior_search_kernel<0>, dim3((unsigned)(nr * k.n_slices)), dim3(RELOC_TPB),
                               relocprior_lds_bytes(k.Wc, k.RW, k.nspan), c->stream, pa);
            HIPCHK(hipGetLastError());
        } else if ((st = launch_reloc_search<0>(c, k, nr))) {
            return st;
        }
        hipLaunchKernelGGL(reloc_peak_kernel, dim3((unsigned)(nr * k.nblk)), dim3(RELOC_PEAK_TPB), 0, c->stream, k);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(reloc_topk_kernel, dim3((unsigned)nr), dim3(RELOC_PEAK_TPB), 0, c->stream, k);
        HIPCHK(hipGetLastError());
    }
    const size_t Rz = (size_t)R;
    if (reloc_coarse_only()) return timer_end(c, LSLAM_K_RELOC);
    if ((st = launch_reloc_fine(c, b, g, m, K, mb))) return st;
    hipLaunchKernelGGL(relocprior_select_kernel<0>, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, c->stream, pa);
    HIPCHK(hipGetLastError());
    if ((st = timer_end(c, LSLAM_K_RELOC))) return st;
    if ((st = reloc_outs(c, b, K, cells))) return st;
    return note_outs(c, {{pb->n_admit, Rz * 8}, {pb->fine_clear2, (size_t)K * Rz * 4}});
}

// ---- the entry points: the params checks (which of two wrong ones wins is their order), then the frame ----

extern "C" {

int lslam_scan_match(lslam_ctx *c, const lslam_match_batch *b, const lslam_match_params *p,
                     const lslam_ukf_params *u) {
    int st = match_check_params(p);
    if (st) return st;
    return map_entry(
        "match", c, b, match_reqs,
        [&]() -> int {
            if (u && b->ukf_u && (!(u->dt > 0) || !(u->wheel_radius > 0)))
                return set_err(LSLAM_ERR_ARG, "match: wheel speeds need dt > 0 and wheel_radius > 0");
            return LSLAM_OK;
        },
        [&] { return launch_match(c, b, p, u); });
}

// On the main stream: every pipeline call ends there (its post pass and lane-group UKF run on it,
// and it waits for ev_ukf when the UKF ran on the side stream), so a ukf_x given as pose is final.
int lslam_grid_update(lslam_ctx *c, const lslam_grid_batch *b, const lslam_grid_params *p) {
    int st = grid_check_params(p);
    if (st) return st;
    return map_entry("grid", c, b, grid_reqs, [&] { return launch_grid(c, b, p); });
}

// On the main stream, as lslam_grid_update: a ukf_x given as pose is final, and so is the grid that
// a preceding lslam_grid_update wrote.
int lslam_map_match(lslam_ctx *c, const lslam_mapmatch_batch *b, const lslam_grid_params *g,
                    const lslam_mapmatch_params *m) {
    int st = mapmatch_check_params(m);
    if (st || (st = grid_check_params(g))) return st;
    return map_entry("mapmatch", c, b, mapmatch_reqs, [&] { return launch_mapmatch(c, b, g, m); });
}

// On the main stream, as lslam_map_match.
int lslam_map_fuse(lslam_ctx *c, const lslam_mapfuse_batch *b, const lslam_grid_params *g,
                   const lslam_mapmatch_params *m, const lslam_mapfuse_params *f) {
    int st = mapmatch_check_params(m);
    if (st || (st = grid_check_params(g)) || (st = mapfuse_check_params(f))) return st;
    return map_entry("mapfuse", c, b, mapfuse_reqs, [&] { return launch_mapfuse(c, b, g, m, f); });
}

// On the main stream, as lslam_map_match.
int lslam_map_relocalize(lslam_ctx *c, const lslam_reloc_batch *b, const lslam_grid_params *g,
                         const lslam_mapmatch_params *m, const lslam_reloc_params *q) {
    int st = mapmatch_check_params(m);
    if (st || (st = grid_check_params(g)) || (st = reloc_check_params(q, g, m))) return st;
    return map_entry("reloc", c, b, reloc_reqs, [&] { return launch_reloc(c, b, g, m, q); });
}

// On the main stream, as lslam_map_match.
int lslam_grid_raycast(lslam_ctx *c, const lslam_raycast_batch *b, const lslam_grid_params *g,
                       const lslam_raycast_params *p) {
    int st = raycast_check_params(p);
    if (st || (st = grid_check_params(g))) return st;
    return map_entry("raycast", c, b, raycast_reqs, [&] { return launch_raycast(c, b, g, p); });
}

// On the main stream, as lslam_grid_update: ordered after the calls that read the grid where it was and
// before the calls that read it where it is.
int lslam_grid_recentre(lslam_ctx *c, const lslam_recentre_batch *b, const lslam_grid_params *g,
                        const lslam_recentre_params *p) {
    int st = grid_check_params(g);
    if (st || (st = recentre_check_params(p, g))) return st;
    return map_entry("recentre", c, b, recentre_reqs, [&] { return launch_recentre(c, b, g, p); });
}

// On the main stream, as lslam_grid_recentre.
int lslam_grid_recentre_paged(lslam_ctx *c, const lslam_recentre_batch *b, const lslam_page_batch *pg, const lslam_grid_params *g,
                              const lslam_recentre_params *p, const lslam_page_params *pp) {
    int st = grid_check_params(g);
    if (st || (st = recentre_check_params(p, g)) || (st = page_check_params(pp))) return st;
    PagedBatch x;
    if (b && pg) x = {*b, *pg};
    return map_entry(
        "page", c, b && pg ? &x : nullptr, paged_reqs,
        [&]() -> int {
            if (b->n_robots != pg->n_robots) return set_err(LSLAM_ERR_ARG, "page: n_robots of the two batches differ");
            return page_check_overlap(*pg, b->logodds, g, pp);
        },
        [&] { return launch_recentre_paged(c, x, g, p, pp); });
}

// On the main stream: a flush after the calls that wrote the window, a load before the calls that read it.
static int page_window_entry(lslam_ctx *c, const lslam_page_batch *pg, const int16_t *logodds, bool store,
                             const lslam_grid_params *g, const lslam_page_params *pp) {
    int st = grid_check_params(g);
    if (st || (st = page_check_params(pp))) return st;
    PageWindowBatch x;
    if (pg) x = {*pg, logodds, store};
    return map_entry(
        "page", c, pg ? &x : nullptr, page_window_reqs, [&] { return page_check_overlap(*pg, logodds, g, pp); },
        [&] { return launch_page_window(c, x, g, pp); });
}

int lslam_grid_page_flush(lslam_ctx *c, const lslam_page_batch *pg, const int16_t *logodds, const lslam_grid_params *g,
                          const lslam_page_params *pp) {
    return page_window_entry(c, pg, logodds, true, g, pp);
}

int lslam_grid_page_load(lslam_ctx *c, const lslam_page_batch *pg, int16_t *logodds, const lslam_grid_params *g,
                         const lslam_page_params *pp) {
    return page_window_entry(c, pg, logodds, false, g, pp);
}

// On the main stream, as lslam_grid_raycast: after the calls that wrote the grid.
int lslam_grid_distance(lslam_ctx *c, const lslam_dist_batch *b, const lslam_grid_params *g, const lslam_dist_params *p) {
    int st = grid_check_params(g);
    if (st || (st = dist_check_params(p))) return st;
    return map_entry(
        "dist", c, b, dist_reqs,
        [&]() -> int {
            const size_t bytes = (size_t)b->n_robots * (size_t)g->grid_w * (size_t)g->grid_w * 2;
            if (ranges_overlap(b->logodds, bytes, b->d2, bytes)) return set_err(LSLAM_ERR_ARG, "dist: d2 overlaps logodds");
            return LSLAM_OK;
        },
        [&] { return launch_dist(c, b, g, p); });
}

// On the main stream, as lslam_grid_raycast.
int lslam_field_score(lslam_ctx *c, const lslam_fieldscore_batch *b, const lslam_grid_params *g,
                      const lslam_fieldscore_params *p) {
    int st = grid_check_params(g);
    if (st || (st = fieldscore_check_params(p))) return st;
    return map_entry("fieldscore", c, b, fieldscore_reqs, [&] { return launch_fieldscore(c, b, g, p); });
}

// On the main stream, as lslam_field_score.
int lslam_field_align(lslam_ctx *c, const lslam_fieldalign_batch *b, const lslam_grid_params *g,
                      const lslam_fieldalign_params *p) {
    int st = grid_check_params(g);
    if (st || (st = fieldalign_check_params(p))) return st;
    return map_entry("fieldalign", c, b, fieldalign_reqs, [&] { return launch_fieldalign(c, b, g, p); });
}

// On the main stream, as lslam_field_align.
int lslam_field_fuse(lslam_ctx *c, const lslam_fieldfuse_batch *b, const lslam_grid_params *g,
                     const lslam_fieldalign_params *p, const lslam_fieldfuse_params *f) {
    int st = grid_check_params(g);
    if (st || (st = fieldalign_check_params(p)) || (st = fieldfuse_check_params(f))) return st;
    return map_entry(
        "fieldfuse", c, b, fieldfuse_reqs,
        [&]() -> int {
            const size_t n = (size_t)b->a.n_robots;
            if (ranges_overlap(b->z, n * 24, b->a.pose, n * 24) || ranges_overlap(b->z, n * 24, b->a.pose_out, n * 24) ||
                ranges_overlap(b->z, n * 24, b->P, n * 72) || ranges_overlap(b->z, n * 24, b->P_out, n * 72))
                return set_err(LSLAM_ERR_ARG, "fieldfuse: z must not overlap pose, pose_out, P or P_out");
            return LSLAM_OK;
        },
        [&] { return launch_fieldfuse(c, b, g, p, f); });
}

// On the main stream, as lslam_map_relocalize.
int lslam_map_relocalize_prior(lslam_ctx *c, const lslam_relocprior_batch *b, const lslam_grid_params *g,
                               const lslam_mapmatch_params *m, const lslam_reloc_params *q,
                               const lslam_relocprior_params *pp) {
    int st = mapmatch_check_params(m);
    if (st || (st = grid_check_params(g)) || (st = reloc_check_params(q, g, m)) || (st = relocprior_check_params(pp))) return st;
    return map_entry(
        "relocprior", c, b, relocprior_reqs, [&] { return relocprior_check_overlap(b, g, q); },
        [&] { return launch_relocprior(c, b, g, m, q, pp); });
}

// On the main stream, as lslam_grid_update: after the calls that wrote either grid, before the calls that
// read the destination.
int lslam_grid_merge(lslam_ctx *c, const lslam_gridmerge_batch *b, const lslam_grid_params *g, const lslam_gridmerge_params *p) {
    int st = grid_check_params(g);
    if (st || (st = gridmerge_check_params(p))) return st;
    return map_entry(
        "gridmerge", c, b, gridmerge_reqs,
        [&]() -> int {
            const size_t sb = (size_t)p->n_src * (size_t)p->src_w * (size_t)p->src_w * 2;
            const size_t db = (size_t)b->n_pairs * (size_t)g->grid_w * (size_t)g->grid_w * 2;
            if (ranges_overlap(b->src, sb, b->dst, db)) return set_err(LSLAM_ERR_ARG, "gridmerge: src overlaps dst");
            return LSLAM_OK;
        },
        [&] { return launch_gridmerge(c, b, g, p); });
}

// On the main stream, as lslam_grid_update: after the calls that wrote the grids, before the calls that read
// the points.
int lslam_grid_points(lslam_ctx *c, const lslam_gridpoints_batch *b, const lslam_grid_params *g, const lslam_gridpoints_params *p) {
    int st = grid_check_params(g);
    if (st || (st = gridpoints_check_params(p))) return st;
    return map_entry(
        "gridpoints", c, b, gridpoints_reqs,
        [&]() -> int {
            // pt_off is 32 bits wide
            if ((int64_t)b->n_robots * (int64_t)p->cap >= ((int64_t)1 << 31))
                return set_err(LSLAM_ERR_ARG, "gridpoints: n_robots * cap must be below 2^31");
            return LSLAM_OK;
        },
        [&] { return launch_gridpoints(c, b, g, p); });
}

// On the main stream: after the calls that wrote the poses and the edges, before the calls that read pose_out
// (a slab of it is a pose of lslam_grid_update and of the matchers).
int lslam_pose_graph(lslam_ctx *c, const lslam_posegraph_batch *b, const lslam_posegraph_params *p) {
    int st = posegraph_check_params(p);
    if (st) return st;
    return map_entry("posegraph", c, b, posegraph_reqs, [&] { return launch_posegraph(c, b, p); });
}

// On the main stream, as lslam_pose_graph: after the calls that wrote the poses, the edges and the candidates,
// before the calls that read the verdicts or, with append, the edges (lslam_pose_graph among them).
int lslam_pose_graph_gate(lslam_ctx *c, const lslam_posegate_batch *b, const lslam_posegate_params *p) {
    int st = posegate_check_params(p);
    if (st) return st;
    return map_entry("posegate", c, b, posegate_reqs, [&] { return launch_posegate(c, b, p); });
}

// (the scratch is sized per call: a call in flight keeps the chunking it was launched with)
int lslam_set_reloc_budget(lslam_ctx *c, int64_t bytes) {
    if (!c) return LSLAM_ERR_ARG;
    c->reloc_budget = bytes > 0 ? (size_t)bytes : default_reloc_budget();
    return LSLAM_OK;
}

}  // extern "C"
