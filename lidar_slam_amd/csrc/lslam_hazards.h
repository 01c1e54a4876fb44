// Which waits the MT producer of a pipeline call needs: bookkeeping over pointers and integers,
// nothing dereferenced (plain C++, no HIP; also compiled by tests/test_hazards.py).  plan_producer
// decides, run_split (lslam_launch.h) turns the plan into hipStreamWaitEvent calls.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lidarslam.h"

constexpr int LSLAM_MAX_COPIES = 32;
constexpr int LSLAM_MAX_OUTS = 48;
// a scan replayed by a speculative call stays dirty in every later one (its producer state is
// never repaired): every SPEC_RESYNC-th chained call waits for the previous
// fix-up instead, which clears the flags (test_gpu_speculate.py runs past it)
constexpr int SPEC_RESYNC = 32;

// a null pointer or a zero length overlaps nothing
static inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// Address ranges written since the producer last waited for the event that covers them.  Past
// CAP distinct ranges the set no longer knows what was written: everything hits until clear().
template <int CAP>
struct RangeSet {
    struct { const void *p; size_t n; } r[CAP];
    int n = 0;
    bool overflow = false;
    void add(const void *p, size_t len) {
        if (!p || !len) return;
        for (int i = 0; i < n; i++)
            if (r[i].p == p && r[i].n == len) return;
        if (n == CAP) {
            overflow = true;
            return;
        }
        r[n].p = p;
        r[n].n = len;
        n++;
    }
    bool hits(const void *p, size_t len) const {
        if (overflow) return true;
        for (int i = 0; i < n; i++)
            if (ranges_overlap(p, len, r[i].p, r[i].n)) return true;
        return false;
    }
    void clear() {
        n = 0;
        overflow = false;
    }
};

// What the producer (seed_kernel, rng_kernel) reads of a batch.
struct ProducerInputs {
    const void *p[4];
    size_t n[4];
    enum { SEEDS, SCAN_CHUNK_OFF, CHUNK_PT_OFF, MT_STATE_IN };
};
static inline ProducerInputs producer_inputs(const lslam_scan_batch *b) {
    return {{b->seeds, b->scan_chunk_off, b->chunk_pt_off, b->mt_state_in},
            {(size_t)b->n_scans * 4, (size_t)(b->n_scans + 1) * 4, (size_t)(b->n_chunks + 1) * 4,
             (size_t)b->n_scans * 625 * 4}};
}

// What cut_lane_kernel reads of a batch besides the CSR arrays: the points, xy or (xy == NULL) the
// polar pair.  It runs on the seeding stream, which makes the producer's waits and no others.
struct PointInputs {
    const void *p[2];
    size_t n[2];
};
static inline PointInputs point_inputs(const lslam_scan_batch *b) {
    const size_t P = (size_t)b->n_points;
    if (b->xy) return {{b->xy, nullptr}, {P * 16, 0}};
    return {{b->theta_deg, b->dist_mm}, {P * 8, P * 8}};
}
// does the call launch cut_lane_kernel (launch_cuts)?  A fresh-stream call (only those seed, and
// the cut kernel goes with seed_kernel) whose chunks fit chunk_kernel.
static inline bool precomputes_cuts(const lslam_scan_batch *b) {
    return !b->mt_state_in && b->n_chunks > 0 && b->max_chunk_points <= 128;
}

struct HazardState {
    // destinations written by copies since the producer last waited for ev_copy: the producer
    // waits only if one of them is its input (seeds, CSR, MT state), so an xy upload per call
    // overlaps the stream parse
    RangeSet<LSLAM_MAX_COPIES> copies;
    // Every buffer written by a call since the producer last waited for ev_call: the union
    // over calls, not only the latest (the producer of call k may start once call k-2's
    // fix-up has run).  A producer input that overlaps one of them makes it wait.
    RangeSet<LSLAM_MAX_OUTS> outs;
    // the latest call's mt_state_out, complete once ev_slot_free[prev_slot] (after its fix-up) fired
    const void *prev_state_out = nullptr;
    int prev_fixed = 0;
    // speculative producer (map mode): a call whose only producer hazard is the previous call's
    // mt_state_out parses from the previous producer's end state (its slot's state area) without
    // waiting for that call's fix-up; the fix-up replays the scans it replayed (spec_dirty)
    int speculate = 1;  // env LSLAM_MT_SPECULATE=0: wait for the fix-up (test_gpu_speculate.py)
    int spec_ok = 0;    // the previous call was a one-epoch pipeline call with dirty flags
    int spec_run = 0;   // consecutive speculative calls (bounded by SPEC_RESYNC)
    const uint32_t *prev_state_scr = nullptr;
    int prev_spec_scans = 0;
};

struct ProducerPlan {
    bool wait_copy;  // a copy wrote one of the producer's inputs: wait for ev_copy
    // does the producer read anything an earlier call wrote?  0: no; 1: only the previous call's
    // mt_state_out (final once that call's fix-up ran: a chained stream, e.g. LandmarkMap steps);
    // 2: something else (wait for ev_call, recorded after every call so far)
    int hazard;
    bool spec;            // parse from the previous producer's end state (level 1 only)
    bool wait_prev_slot;  // level 1 without speculation: wait for the previous call's fix-up
    // a producer that waited on the previous call will most likely wait on this one too, so
    // this call's resolve runs alone: the LDS-staged form is faster there (map mode 1.48 vs
    // 1.39 ms per step); otherwise the next call's producer runs beside it and holds the LDS
    // (C3 0.93 vs 1.03 ms)
    bool resolve_beside;
    // A copy or an earlier call wrote the points and no wait of this plan covers it: launch no
    // cut kernel, the stream-ordered consensus computes its cuts itself (byte-identical,
    // test_gpu_cuts.py).  Asks for no wait and clears no set, so the producer still overlaps an
    // upload of the points; false in a call that launches no cut kernel anyway.
    bool skip_cuts;
};

// The waits of this call's producer; a wait that the plan asks for empties the set it covers.
// ep_count: the call's producer launches (prepare_steps).
static inline ProducerPlan plan_producer(HazardState &h, const lslam_scan_batch *b, int ep_count) {
    const ProducerInputs in = producer_inputs(b);
    ProducerPlan pl;
    // a copy into this call's MT state (e.g. a caller's upload into the previous call's
    // mt_state_out) invalidates speculating from the previous producer's end state
    const bool state_copied = h.copies.hits(in.p[ProducerInputs::MT_STATE_IN], in.n[ProducerInputs::MT_STATE_IN]);
    pl.wait_copy = false;
    for (int i = 0; i < 4; i++) pl.wait_copy |= h.copies.hits(in.p[i], in.n[i]);
    if (pl.wait_copy) h.copies.clear();
    pl.hazard = h.outs.overflow ? 2 : 0;
    for (int i = 0; i < 4 && !h.outs.overflow; i++)
        for (int j = 0; j < h.outs.n; j++)
            if (ranges_overlap(in.p[i], in.n[i], h.outs.r[j].p, h.outs.r[j].n)) {
                const bool chained = i == ProducerInputs::MT_STATE_IN && h.outs.r[j].p == h.prev_state_out && h.prev_fixed;
                if (pl.hazard < 2) pl.hazard = chained ? 1 : 2;
            }
    if (pl.hazard == 2) h.outs.clear();  // ev_call follows every call enqueued so far: the union starts afresh
    pl.spec = pl.hazard == 1 && h.speculate && h.spec_ok && ep_count == 1 && h.prev_state_scr &&
              h.prev_spec_scans == b->n_scans && b->mt_state_in == h.prev_state_out && !state_copied;
    if (pl.spec && ++h.spec_run >= SPEC_RESYNC) pl.spec = false;
    if (!pl.spec) h.spec_run = 0;
    pl.wait_prev_slot = pl.hazard == 1 && !pl.spec;
    pl.resolve_beside = pl.hazard == 0 || pl.spec;
    // after the clears above: a set that this plan's waits emptied no longer hits, and the seeding
    // stream makes those waits ahead of the cut kernel (seed_beside)
    pl.skip_cuts = false;
    if (precomputes_cuts(b)) {
        const PointInputs pt = point_inputs(b);
        for (int i = 0; i < 2; i++)
            if (pt.p[i] && pt.n[i]) pl.skip_cuts |= h.copies.hits(pt.p[i], pt.n[i]) || h.outs.hits(pt.p[i], pt.n[i]);
    }
    return pl;
}
