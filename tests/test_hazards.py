"""The producer's wait decisions (lidar_slam_amd/csrc/lslam_hazards.h), compiled with g++ on the CPU:
the range sets of copies and call outputs, and plan_producer, which run_split turns into stream
waits -- and, for the points that the cut kernel reads on the seeding stream, into launching no
cut kernel (points_copied, points_written).  Addresses are integers cast to pointers; nothing is dereferenced.  The program is built
with -fsanitize=address,undefined when the compiler here can link an empty program with them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_hazards.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

static int bad = 0;
#define CHECK(x) do { if (!(x)) { bad++; std::printf("line %d: %s\n", __LINE__, #x); } } while (0)

static const uintptr_t SEEDS = 0x10000, SCO = 0x20000, CPO = 0x30000, X = 0x40000, Y = 0x50000, SCR = 0x60000,
                       FAR = 0x900000;
enum { S = 4, C = 8 };
static const size_t LEN[4] = {S * 4, (S + 1) * 4, (C + 1) * 4, S * 625 * 4};
static const void *A(uintptr_t a) { return (const void *)a; }

static lslam_scan_batch batch(uintptr_t state_in, uintptr_t state_out = 0) {
    lslam_scan_batch b;
    std::memset(&b, 0, sizeof(b));
    b.n_scans = S;
    b.n_chunks = C;
    b.seeds = (const uint32_t *)SEEDS;
    b.scan_chunk_off = (const int32_t *)SCO;
    b.chunk_pt_off = (const int32_t *)CPO;
    b.mt_state_in = (const uint32_t *)state_in;
    b.mt_state_out = (uint32_t *)state_out;
    return b;
}
// what run_split notes once a one-epoch MT pipeline call with mt_state_out is enqueued
static void mt_call_done(HazardState &h, const lslam_scan_batch &b) {
    h.outs.add(b.mt_state_out, LEN[3]);
    h.prev_state_out = b.mt_state_out;
    h.prev_fixed = 1;
    h.spec_ok = 1;
    h.prev_state_scr = (const uint32_t *)SCR;
    h.prev_spec_scans = b.n_scans;
}
// a context whose latest call was an MT call that wrote its end state to X
static HazardState chained() {
    HazardState h;
    mt_call_done(h, batch(0, X));
    return h;
}

static void copies() {
    const uintptr_t in[4] = {SEEDS, SCO, CPO, X};
    const lslam_scan_batch b = batch(X);
    const ProducerInputs pi = producer_inputs(&b);
    for (int i = 0; i < 4; i++) {
        CHECK(pi.p[i] == A(in[i]) && pi.n[i] == LEN[i]);
        // the whole input; a copy whose last byte is the input's first; one whose first is its last
        const uintptr_t lo[3] = {in[i], in[i] - 8, in[i] + LEN[i] - 1};
        const size_t n[3] = {LEN[i], 9, 100};
        for (int v = 0; v < 3; v++) {
            HazardState h;
            h.copies.add(A(FAR), 64);
            h.copies.add(A(lo[v]), n[v]);
            const ProducerPlan pl = plan_producer(h, &b, 1);
            CHECK(pl.wait_copy);
            CHECK(h.copies.n == 0 && !h.copies.overflow);
            CHECK(pl.hazard == 0 && !pl.spec && !pl.wait_prev_slot && pl.resolve_beside);
            CHECK(!plan_producer(h, &b, 1).wait_copy);
        }
        // adjacent on either side: no wait, and the set is kept
        HazardState h;
        h.copies.add(A(in[i] - 8), 8);
        h.copies.add(A(in[i] + LEN[i]), 8);
        CHECK(!plan_producer(h, &b, 1).wait_copy);
        CHECK(h.copies.n == 2);
    }
    HazardState h;
    h.copies.add(nullptr, 64);
    h.copies.add(A(SEEDS), 0);
    CHECK(h.copies.n == 0);
    CHECK(!plan_producer(h, &b, 1).wait_copy);
    // an absent input overlaps nothing, whatever was copied
    h.copies.add(A(1), (size_t)X - 1);  // [1, X): everything below X but the state
    lslam_scan_batch nb = batch(0);
    nb.seeds = nullptr;
    nb.scan_chunk_off = nullptr;
    nb.chunk_pt_off = nullptr;
    CHECK(!plan_producer(h, &nb, 1).wait_copy);
    CHECK(!ranges_overlap(nullptr, 8, nullptr, 8) && !ranges_overlap(A(8), 0, A(8), 8) && ranges_overlap(A(8), 1, A(8), 1));
}

static void duplicates() {
    RangeSet<4> r;
    r.add(A(X), 100);
    r.add(A(X), 100);
    CHECK(r.n == 1);
    r.add(A(X), 101);
    r.add(A(X + 1), 100);
    CHECK(r.n == 3 && !r.overflow);
    CHECK(r.hits(A(X + 100), 1) && !r.hits(A(X + 101), 1) && !r.hits(A(X - 1), 1));
    r.clear();
    CHECK(r.n == 0 && !r.hits(A(X), 100));
}

static void overflow() {
    const lslam_scan_batch b = batch(0);
    HazardState h;
    for (int i = 0; i < LSLAM_MAX_COPIES; i++) h.copies.add(A(FAR + 256 * i), 64);
    h.copies.add(A(FAR), 64);  // known already: takes no slot
    CHECK(h.copies.n == LSLAM_MAX_COPIES && LSLAM_MAX_COPIES == 32 && !h.copies.overflow);
    CHECK(!plan_producer(h, &b, 1).wait_copy);
    h.copies.add(A(FAR + 256 * LSLAM_MAX_COPIES), 64);  // the 33rd distinct range
    CHECK(h.copies.overflow && h.copies.hits(A(8), 1));
    h.copies.add(A(FAR + 256 * (LSLAM_MAX_COPIES + 1)), 64);
    CHECK(plan_producer(h, &b, 1).wait_copy);
    CHECK(!h.copies.overflow && h.copies.n == 0);
    CHECK(!plan_producer(h, &b, 1).wait_copy);

    for (int i = 0; i < LSLAM_MAX_OUTS; i++) h.outs.add(A(FAR + 256 * i), 64);
    h.outs.add(A(FAR), 64);
    CHECK(h.outs.n == LSLAM_MAX_OUTS && !h.outs.overflow);
    CHECK(plan_producer(h, &b, 1).hazard == 0);
    h.outs.add(A(FAR + 256 * LSLAM_MAX_OUTS), 64);
    CHECK(h.outs.overflow);
    const ProducerPlan pl = plan_producer(h, &b, 1);
    CHECK(pl.hazard == 2 && !pl.spec && !pl.wait_prev_slot && !pl.resolve_beside && !pl.wait_copy);
    CHECK(!h.outs.overflow && h.outs.n == 0);
    CHECK(plan_producer(h, &b, 1).hazard == 0);
}

// MT (state -> X), Philox (other outputs), MT chaining from X: the producer waits for every call
static void output_union() {
    for (int other_state = 0; other_state < 2; other_state++) {
        HazardState h = chained();
        h.outs.add(A(FAR), 4096);  // the unrelated call's outputs
        h.prev_state_out = other_state ? A(Y) : nullptr;
        h.prev_fixed = other_state;
        h.spec_ok = 0;
        const lslam_scan_batch b = batch(X, Y);
        const ProducerPlan pl = plan_producer(h, &b, 1);
        CHECK(pl.hazard == 2 && !pl.spec && !pl.wait_prev_slot && !pl.resolve_beside && !pl.wait_copy);
        CHECK(h.outs.n == 0 && h.spec_run == 0);
    }
    // an output over a CSR array or the seeds is level 2 even when the state chains
    const uintptr_t in[3] = {SEEDS, SCO, CPO};
    for (int i = 0; i < 3; i++) {
        HazardState h = chained();
        h.outs.add(A(in[i] + LEN[i] - 1), 64);
        const lslam_scan_batch b = batch(X, Y);
        CHECK(plan_producer(h, &b, 1).hazard == 2 && h.outs.n == 0);
    }
}

static void chaining() {
    const lslam_scan_batch b = batch(X, Y);
    {
        HazardState h;
        const ProducerPlan pl = plan_producer(h, &b, 1);  // nothing written yet
        CHECK(pl.hazard == 0 && !pl.spec && !pl.wait_prev_slot && pl.resolve_beside && !pl.wait_copy);
    }
    {
        HazardState h = chained();
        const ProducerPlan pl = plan_producer(h, &b, 1);
        CHECK(pl.hazard == 1 && pl.spec && pl.resolve_beside && !pl.wait_prev_slot && !pl.wait_copy);
        CHECK(h.outs.n == 1 && h.spec_run == 1);
    }
    for (int flip = 0; flip < 5; flip++) {
        HazardState h = chained();
        h.spec_run = 3;
        int ep = 1;
        if (flip == 0) h.spec_ok = 0;
        if (flip == 1) h.prev_spec_scans = S + 1;
        if (flip == 2) ep = 2;
        if (flip == 3) h.prev_state_scr = nullptr;
        if (flip == 4) h.speculate = 0;
        const ProducerPlan pl = plan_producer(h, &b, ep);
        CHECK(pl.hazard == 1 && !pl.spec && pl.wait_prev_slot && !pl.resolve_beside);
        CHECK(h.outs.n == 1 && h.spec_run == 0);
    }
    {
        HazardState h = chained();
        h.prev_fixed = 0;  // the state is not final at the slot's event
        const ProducerPlan pl = plan_producer(h, &b, 1);
        CHECK(pl.hazard == 2 && !pl.spec && !pl.wait_prev_slot);
    }
}

// a copy into the chained state between two calls: the set is cleared by the same plan, and the
// call still must not speculate
static void copy_between() {
    const lslam_scan_batch b = batch(X, Y);
    HazardState h = chained();
    h.copies.add(A(X), LEN[3]);
    ProducerPlan pl = plan_producer(h, &b, 1);
    CHECK(pl.wait_copy && pl.hazard == 1 && !pl.spec && pl.wait_prev_slot && !pl.resolve_beside);
    CHECK(h.copies.n == 0 && h.spec_run == 0);
    h = chained();
    for (int i = 0; i <= LSLAM_MAX_COPIES; i++) h.copies.add(A(FAR + 256 * i), 64);  // unknown copies
    pl = plan_producer(h, &b, 1);
    CHECK(pl.wait_copy && pl.hazard == 1 && !pl.spec && pl.wait_prev_slot);
    h = chained();
    h.copies.add(A(FAR), 64);  // a copy elsewhere (an xy upload) leaves the speculation alone
    pl = plan_producer(h, &b, 1);
    CHECK(!pl.wait_copy && pl.spec && h.copies.n == 1);
}

static void resync() {
    HazardState h = chained();
    uintptr_t in = X, out = Y;
    int waits = 0;
    for (int call = 1; call <= 70; call++) {
        const lslam_scan_batch b = batch(in, out);
        const ProducerPlan pl = plan_producer(h, &b, 1);
        const bool resync_call = call == 32 || call == 64;
        CHECK(pl.hazard == 1 && pl.spec == !resync_call && pl.wait_prev_slot == resync_call);
        if (!pl.spec) {
            waits++;
            CHECK(h.spec_run == 0);
        }
        mt_call_done(h, b);
        const uintptr_t t = in;
        in = out;
        out = t;
    }
    CHECK(waits == 2 && SPEC_RESYNC == 32 && h.spec_run == 6);
}

// The points that cut_lane_kernel reads on the seeding stream: xy [P][2] doubles, or theta_deg and
// dist_mm [P] doubles each.  kind 0: xy (the polar pointers set too: xy wins); 1: polar.
enum { P = 800 };
static const uintptr_t PXY = 0x100000, PTH = 0x200000, PDD = 0x300000;
static lslam_scan_batch pbatch(int kind, uintptr_t state_in = 0, uintptr_t state_out = 0) {
    lslam_scan_batch b = batch(state_in, state_out);
    b.n_points = P;
    b.max_chunk_points = 128;
    b.xy = kind == 0 ? (const double *)PXY : nullptr;
    b.theta_deg = (const double *)PTH;
    b.dist_mm = (const double *)PDD;
    return b;
}
static const struct { int kind; uintptr_t at; size_t len; } PT[3] = {{0, PXY, P * 16}, {1, PTH, P * 8}, {1, PDD, P * 8}};

// via: 0 a pending copy, 1 an earlier call's output
static void note(HazardState &h, int via, uintptr_t at, size_t n) {
    if (via) h.outs.add(A(at), n);
    else h.copies.add(A(at), n);
}
static int noted(const HazardState &h, int via) { return via ? h.outs.n : h.copies.n; }
// the cut kernel may not run ahead of the write: skipped, or behind a wait the seeding stream makes
static bool cuts_safe(const ProducerPlan &pl, int via) { return pl.skip_cuts || (via ? pl.hazard == 2 : pl.wait_copy); }

static void points_case(int via) {
    for (int i = 0; i < 3; i++) {
        const lslam_scan_batch b = pbatch(PT[i].kind);
        const uintptr_t at = PT[i].at;
        const size_t len = PT[i].len;
        const uintptr_t lo[3] = {at, at - 8, at + len - 1};
        const size_t n[3] = {len, 9, 100};
        for (int v = 0; v < 3; v++) {
            HazardState h;
            note(h, via, FAR, 64);
            note(h, via, lo[v], n[v]);
            ProducerPlan pl = plan_producer(h, &b, 1);
            CHECK(cuts_safe(pl, via));
            // the points alone: the producer gains no wait, so nothing may be cleared
            CHECK(pl.skip_cuts && !pl.wait_copy && pl.hazard == 0 && !pl.spec && !pl.wait_prev_slot && pl.resolve_beside);
            CHECK(noted(h, via) == 2);
            pl = plan_producer(h, &b, 1);  // still pending for the next call
            CHECK(pl.skip_cuts && !pl.wait_copy && pl.hazard == 0);
            // the seeds written as well: the seeding stream waits, the set is cleared, the cuts run
            note(h, via, SEEDS, 4);
            pl = plan_producer(h, &b, 1);
            CHECK(cuts_safe(pl, via) && !pl.skip_cuts && noted(h, via) == 0);
            CHECK(via ? (pl.hazard == 2 && !pl.wait_copy) : (pl.wait_copy && pl.hazard == 0));
            CHECK(!plan_producer(h, &b, 1).skip_cuts);
        }
        // adjacent on either side: nothing asked
        HazardState h;
        note(h, via, at - 8, 8);
        note(h, via, at + len, 8);
        ProducerPlan pl = plan_producer(h, &b, 1);
        CHECK(!pl.skip_cuts && !pl.wait_copy && pl.hazard == 0 && noted(h, via) == 2);
        // a call that launches no cut kernel: a hit asks for nothing, the plan is the one without points
        for (int why = 0; why < 3; why++) {
            HazardState h1 = chained(), h2 = chained();
            note(h1, via, at, len);
            lslam_scan_batch nb = pbatch(PT[i].kind, why == 0 ? X : 0, Y);
            if (why == 1) nb.max_chunk_points = 129;
            if (why == 2) nb.n_chunks = 0;
            lslam_scan_batch ref = nb;
            ref.xy = nullptr;
            ref.theta_deg = nullptr;
            ref.dist_mm = nullptr;
            const ProducerPlan a = plan_producer(h1, &nb, 1), r = plan_producer(h2, &ref, 1);
            CHECK(!a.skip_cuts && !r.skip_cuts);
            CHECK(a.wait_copy == r.wait_copy && a.hazard == r.hazard && a.spec == r.spec &&
                  a.wait_prev_slot == r.wait_prev_slot && a.resolve_beside == r.resolve_beside);
            CHECK(!a.wait_copy && a.hazard == (why == 0 ? 1 : 0) && a.spec == (why == 0));
            CHECK(noted(h1, via) == 1 + via);  // (chained() holds one output)
        }
        // max_chunk_points = 128 is the last size with a cut kernel
        {
            HazardState h1;
            note(h1, via, at, len);
            lslam_scan_batch nb = pbatch(PT[i].kind);
            nb.max_chunk_points = 1;
            CHECK(plan_producer(h1, &nb, 1).skip_cuts);
        }
    }
    // xy given: what lies where the polar arrays would be is not read, and the other way round
    {
        HazardState h;
        note(h, via, PTH, P * 8);
        note(h, via, PDD, P * 8);
        const lslam_scan_batch b = pbatch(0);
        CHECK(!plan_producer(h, &b, 1).skip_cuts);
        const lslam_scan_batch pb = pbatch(1);
        CHECK(plan_producer(h, &pb, 1).skip_cuts);
    }
    {
        HazardState h;
        note(h, via, PXY, P * 16);
        const lslam_scan_batch pb = pbatch(1);
        CHECK(!plan_producer(h, &pb, 1).skip_cuts);
        const lslam_scan_batch b = pbatch(0);
        CHECK(plan_producer(h, &b, 1).skip_cuts);
    }
    // absent points overlap nothing
    {
        HazardState h;
        note(h, via, PXY, 0x300000);
        lslam_scan_batch b = pbatch(1);
        b.theta_deg = nullptr;
        b.dist_mm = nullptr;
        CHECK(!plan_producer(h, &b, 1).skip_cuts);
        b = pbatch(0);
        b.n_points = 0;
        CHECK(!plan_producer(h, &b, 1).skip_cuts);
    }
    // a set that no longer knows what was written hits the points too
    for (int kind = 0; kind < 2; kind++) {
        HazardState h;
        const int cap = via ? LSLAM_MAX_OUTS : LSLAM_MAX_COPIES;
        for (int i = 0; i <= cap; i++) note(h, via, FAR + 256 * i, 64);
        CHECK(via ? h.outs.overflow : h.copies.overflow);
        lslam_scan_batch b = pbatch(kind);
        const ProducerPlan pl = plan_producer(h, &b, 1);
        CHECK(cuts_safe(pl, via));
        // and in a call without a cut kernel it asks for what it asked before, no more
        HazardState h2;
        for (int i = 0; i <= cap; i++) note(h2, via, FAR + 256 * i, 64);
        b.max_chunk_points = 129;
        const ProducerPlan p2 = plan_producer(h2, &b, 1);
        CHECK(!p2.skip_cuts && p2.wait_copy == !via && p2.hazard == (via ? 2 : 0));
    }
}
static void points_copied() { points_case(0); }
static void points_written() { points_case(1); }

int main(int argc, char **argv) {
    const struct { const char *name; void (*fn)(); } cases[] = {
        {"copies", copies},       {"duplicates", duplicates},     {"overflow", overflow}, {"output_union", output_union},
        {"chaining", chaining},   {"copy_between", copy_between}, {"resync", resync},     {"points_copied", points_copied},
        {"points_written", points_written}};
    int ran = 0;
    for (const auto &c : cases)
        if (argc < 2 || !std::strcmp(argv[1], c.name)) {
            c.fn();
            ran++;
        }
    std::printf("%d %d\n", ran, bad);
    return bad != 0 || ran == 0;
}
"""

CASES = ["copies", "duplicates", "overflow", "output_union", "chaining", "copy_between", "resync", "points_copied",
         "points_written"]


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def hazards_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("hazards")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_plan_producer(hazards_exe, case):
    out = subprocess.run([hazards_exe, case], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    ran, bad = map(int, out.stdout.split()[-2:])
    assert ran == 1 and bad == 0, out.stdout
