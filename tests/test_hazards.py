"""The producer's wait decisions (lidar_slam_amd/csrc/lslam_hazards.h), compiled with g++ on the CPU:
the range sets of copies and call outputs, and plan_producer, which run_split turns into stream
waits.  Addresses are integers cast to pointers; nothing is dereferenced.  The program is built
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

int main(int argc, char **argv) {
    const struct { const char *name; void (*fn)(); } cases[] = {
        {"copies", copies},       {"duplicates", duplicates},     {"overflow", overflow}, {"output_union", output_union},
        {"chaining", chaining},   {"copy_between", copy_between}, {"resync", resync}};
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

CASES = ["copies", "duplicates", "overflow", "output_union", "chaining", "copy_between", "resync"]


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
