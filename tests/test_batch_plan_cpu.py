"""csrc/client/batch_plan.h on its own (CPU, a host compiler only): the batch
worker's decisions — which job slices share a launch, when a shared buffer
forces a new one, which slices run one by one, which pieces a failed launch
fails, what the injected failing thread's slice does, and that no table
passes the cap — are otherwise reached only end to end on a GPU
(test_batch_gpu.py, test_half_batch_gpu.py).

A stand-alone program (its own main) includes the planner header and plans
rounds over made-up addresses, which the planner compares and never
dereferences.  Every plan goes through one structural check (pieces follow
FifoSliceGeometry, the tables hold exactly the slices the rules put there, in
order, every launch's fail range covers its own jobs' pieces and the ranges
are disjoint); the cases then pin the shape of each plan.  Built with the
host compiler, plain and once more with the address and undefined-behaviour
sanitizers, and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIENT = os.path.join(ROOT, "p4app-switchml_amd", "csrc", "client")
# FifoSliceGeometry's definition and what it links against; no HIP in either
SOURCES = [os.path.join(CLIENT, f) for f in ("fifo_scheduler.cc", "job.cc")]

PROGRAM = r"""
#include "batch_plan.h"

#include <stdio.h>

#include <string>

using namespace switchml;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) { printf("line %d (%s): %s\n", __LINE__, g_case, #cond); failures++; } \
    } while (0)
static const char* g_case = "";

static PlanJob J(uintptr_t in, uintptr_t out, Numel n, DataType t = FLOAT32) {
    return PlanJob{(const void*)in, (void*)out, n, t};
}
// T, P, bmax 8, no injected fault, not instant, a pre/post-processor, cap 64
static PlanParams PP(int T, uint64_t P) { return PlanParams{T, P, 8, -1, false, true, 64}; }

static std::string order(const BatchPlan& pl) {
    std::string s;
    for (const PlanStep& st : pl.steps) s += st.kind == PlanStep::kLaunch ? 'L' : 'S';
    return s;
}
static std::vector<size_t> tables(const BatchPlan& pl) {
    std::vector<size_t> v;
    for (const PlanStep& st : pl.steps)
        if (st.kind == PlanStep::kLaunch) v.push_back(st.count);
    return v;
}

// What holds for every plan.  The rules are restated here from the batch
// worker's contract, not taken from the planner.
static BatchPlan plan_checked(const std::vector<PlanJob>& jobs, const PlanParams& p) {
    const BatchPlan pl = PlanBatch(jobs, p);
    const size_t T = (size_t)p.T;
    CHECK(pl.pieces.size() == jobs.size() * T);
    if (pl.pieces.size() != jobs.size() * T) return pl;
    // the pieces: T per job in job, tid order, cut by FifoSliceGeometry; which of
    // them sit in a table (in order: slice k belongs to piece slice_piece[k]),
    // which run alone
    std::vector<size_t> slice_piece, single_piece;
    std::vector<bool> job_batched(jobs.size());
    for (size_t j = 0; j < jobs.size(); j++) {
        const PlanJob& job = jobs[j];
        const bool work = job.numel > 0 && !p.instant;
        const bool flt = job.data_type == FLOAT32 || job.data_type == FLOAT16 || job.data_type == BFLOAT16;
        job_batched[j] = work && p.has_ppp && flt && job.in_d && job.out_d;
        for (size_t t = 0; t < T; t++) {
            const PlanPiece& pc = pl.pieces[j * T + t];
            Numel off, n;
            FifoSliceGeometry(job.numel, p.T, (int)t, &off, &n);
            CHECK(pc.job == j && pc.tid == (WorkerTid)t && pc.offset == off && pc.numel == n);
            const bool touched = work && n > 0 && p.has_ppp && (int)t != p.fail_tid;
            CHECK(pc.ok == (!work || n == 0 || touched));
            if (touched && job_batched[j]) slice_piece.push_back(j * T + t);
            if (touched && !job_batched[j]) single_piece.push_back(j * T + t);
            if (!(touched && job_batched[j])) CHECK(pc.packets == 0);
        }
    }
    CHECK(pl.slices.size() == slice_piece.size());
    if (pl.slices.size() != slice_piece.size()) return pl;
    for (size_t k = 0; k < pl.slices.size(); k++) {
        const PlanPiece& pc = pl.pieces[slice_piece[k]];
        const PlanJob& job = jobs[pc.job];
        const size_t esz = job.data_type == FLOAT32 ? 4 : 2;
        CHECK((uintptr_t)pl.slices[k].in == (uintptr_t)job.in_d + pc.offset * esz);
        CHECK((uintptr_t)pl.slices[k].out == (uintptr_t)job.out_d + pc.offset * esz);
        CHECK(pl.slices[k].numel == pc.numel && pl.slices[k].data_type == job.data_type);
        const uint64_t B = (pc.numel + p.P - 1) / p.P;
        CHECK(pc.packets == B + std::min<uint64_t>(B, p.bmax));
    }
    // the steps: the tables partition the slices in order, none is empty or over
    // the cap; single slices come in piece order; steps are in FIFO order
    size_t next_slice = 0, next_single = 0, last_fail_end = 0;
    long last_piece = -1;
    for (const PlanStep& st : pl.steps) {
        if (st.kind == PlanStep::kSingle) {
            CHECK(next_single < single_piece.size() && st.first == single_piece[next_single]);
            CHECK(st.count == 1 && st.fail_first == st.first && st.fail_end == st.first + 1);
            CHECK((long)st.first > last_piece);
            last_piece = (long)st.first;
            next_single++;
        } else {
            CHECK(st.first == next_slice && st.count > 0 && st.count <= p.max_table_slices);
            CHECK(st.first + st.count <= pl.slices.size());
            if (st.count == 0 || st.first + st.count > pl.slices.size()) return pl;
            next_slice = st.first + st.count;
            CHECK((long)slice_piece[st.first] > last_piece);
            last_piece = (long)slice_piece[next_slice - 1];
            // (l) the fail range holds every piece with a slice in this table ...
            CHECK(st.fail_first <= slice_piece[st.first] && slice_piece[next_slice - 1] < st.fail_end);
            CHECK(st.fail_end <= pl.pieces.size());
            // ... every piece of a job that is wholly in this table ...
            for (size_t k = st.first; k < next_slice; k++) {
                const size_t j = pl.pieces[slice_piece[k]].job;
                bool whole = true;
                for (size_t k2 = 0; k2 < pl.slices.size(); k2++)
                    if (pl.pieces[slice_piece[k2]].job == j && (k2 < st.first || k2 >= next_slice)) whole = false;
                if (whole) CHECK(st.fail_first <= j * T && (j + 1) * T <= st.fail_end);
            }
            // ... and nothing that another step touches
            for (size_t k = 0; k < pl.slices.size(); k++)
                if (k < st.first || k >= next_slice)
                    CHECK(slice_piece[k] < st.fail_first || slice_piece[k] >= st.fail_end);
            for (size_t s : single_piece) CHECK(s < st.fail_first || s >= st.fail_end);
        }
        // disjoint ranges, in order
        CHECK(st.fail_first >= last_fail_end && st.fail_first < st.fail_end);
        last_fail_end = st.fail_end;
    }
    CHECK(next_slice == pl.slices.size() && next_single == single_piece.size());
    return pl;
}

int main() {
    const int Ts[] = {1, 3, 4};
    const uint64_t Ps[] = {64, 256, 1024};
    // made-up, well separated addresses
    const uintptr_t A = 0x10000000, B = 0x20000000, C = 0x30000000, D = 0x40000000, E = 0x50000000;
    for (int T : Ts)
        for (uint64_t P : Ps) {
            const PlanParams p = PP(T, P);
            const size_t uT = (size_t)T;
            {
                g_case = "a: five distinct fp32 buckets";
                const Numel n[5] = {100003, 7, 4097, 65536, 777};
                std::vector<PlanJob> jobs;
                for (int j = 0; j < 5; j++) jobs.push_back(J(A + j * 0x1000000, B + j * 0x1000000, n[j]));
                const BatchPlan pl = plan_checked(jobs, p);
                CHECK(order(pl) == "L" && pl.slices.size() == 5 * uT);
                CHECK(pl.steps[0].fail_first == 0 && pl.steps[0].fail_end == 5 * uT);
                for (int j = 0; j < 5; j++)
                    for (int t = 0; t < T; t++) {
                        Numel off, cnt;
                        FifoSliceGeometry(n[j], T, t, &off, &cnt);
                        const PlanSlice& s = pl.slices[j * uT + t];
                        CHECK((uintptr_t)s.in == A + j * 0x1000000 + off * 4 && s.numel == cnt);
                        CHECK((uintptr_t)s.out == B + j * 0x1000000 + off * 4);
                    }
            }
            {
                g_case = "b: the same in-place job twice";
                const BatchPlan pl = plan_checked({J(A, A, 4097), J(A, A, 4097)}, p);
                CHECK(order(pl) == "LL" && tables(pl) == std::vector<size_t>({uT, uT}));
                CHECK(pl.steps[1].fail_first == uT && pl.steps[1].fail_end == 2 * uT);
                CHECK(pl.steps[0].fail_first == 0 && pl.steps[0].fail_end == uT);
            }
            {
                g_case = "c: job 2 reads what job 1 writes";
                CHECK(order(plan_checked({J(A, B, 4097), J(B, C, 4097)}, p)) == "LL");
                // the last byte of job 1's output alone
                CHECK(order(plan_checked({J(A, B, 4097), J(B + 4097 * 4 - 1, C, 100)}, p)) == "LL");
                // adjacent is not shared
                CHECK(order(plan_checked({J(A, B, 4097), J(B + 4097 * 4, C, 100)}, p)) == "L");
                g_case = "d: job 2 writes what job 1 reads";
                CHECK(order(plan_checked({J(A, B, 4097), J(C, A, 4097)}, p)) == "LL");
                CHECK(order(plan_checked({J(A, B, 4097), J(C, A - 100 * 4 + 1, 100)}, p)) == "LL");
                CHECK(order(plan_checked({J(A, B, 4097), J(C, A - 100 * 4, 100)}, p)) == "L");
                g_case = "d': job 2 writes what job 1 writes";
                CHECK(order(plan_checked({J(A, B, 4097), J(C, B, 4097)}, p)) == "LL");
                g_case = "e: two jobs read one input";
                const BatchPlan pl = plan_checked({J(A, B, 4097), J(A, C, 4097)}, p);
                CHECK(order(pl) == "L" && pl.slices.size() == 2 * uT);
                // the split starts afresh: job 3 shares nothing with job 2's table
                CHECK(tables(plan_checked({J(A, A, 4097), J(A, A, 4097), J(C, D, 4097)}, p)) ==
                      std::vector<size_t>({uT, 2 * uT}));
            }
            {
                g_case = "f: bf16 + fp16 + fp32 in one table";
                const BatchPlan pl =
                    plan_checked({J(A, B, 100003, BFLOAT16), J(C, C, 4097, FLOAT16), J(D, E, 777, FLOAT32)}, p);
                CHECK(order(pl) == "L" && pl.slices.size() == 3 * uT);
                const PlanPiece& last16 = pl.pieces[uT - 1];
                CHECK((uintptr_t)pl.slices[uT - 1].in == A + last16.offset * 2);
                CHECK((uintptr_t)pl.slices[2 * uT - 1].out == C + pl.pieces[2 * uT - 1].offset * 2);
                CHECK((uintptr_t)pl.slices[3 * uT - 1].out == E + pl.pieces[3 * uT - 1].offset * 4);
                CHECK(pl.slices[0].data_type == BFLOAT16 && pl.slices[uT].data_type == FLOAT16 &&
                      pl.slices[2 * uT].data_type == FLOAT32);
            }
            {
                g_case = "g: a job that cannot be batched between float jobs";
                const PlanJob mid[] = {J(C, C, 4097, INT32), J(0, C, 4097), J(C, 0, 4097), J(0, 0, 4097, FLOAT16)};
                for (const PlanJob& m : mid) {
                    const BatchPlan pl = plan_checked({J(A, A, 4097), m, J(B, B, 4097)}, p);
                    CHECK(order(pl) == "L" + std::string(uT, 'S') + "L");
                    CHECK(tables(pl) == std::vector<size_t>({uT, uT}));
                    for (size_t t = 0; t < uT; t++) CHECK(pl.steps[1 + t].first == uT + t && pl.pieces[uT + t].ok);
                    CHECK(pl.steps[0].fail_end == uT && pl.steps[uT + 1].fail_first == 2 * uT);
                }
            }
            {
                g_case = "h: numel < T";
                const BatchPlan pl = plan_checked({J(A, B, 2), J(C, D, 4097)}, p);
                const size_t filled = std::min<size_t>(2, uT);
                CHECK(order(pl) == "L" && pl.slices.size() == filled + uT);
                for (size_t t = 0; t < uT; t++) CHECK(pl.pieces[t].ok && (pl.pieces[t].numel == 0) == (t >= filled));
                g_case = "i: numel == 0";
                const BatchPlan none = plan_checked({J(A, B, 0)}, p);
                CHECK(none.steps.empty() && none.slices.empty() && none.pieces.size() == uT);
                for (const PlanPiece& pc : none.pieces) CHECK(pc.ok && pc.numel == 0);
                // between two jobs of one table it neither splits nor hides them from the fail range
                const BatchPlan mid = plan_checked({J(A, B, 4097), J(0, 0, 0), J(C, D, 4097)}, p);
                CHECK(order(mid) == "L" && mid.steps[0].fail_first == 0 && mid.steps[0].fail_end == 3 * uT);
                PlanParams inst = p;
                inst.instant = true;
                const BatchPlan ip = plan_checked({J(A, B, 4097), J(C, C, 4097, INT32)}, inst);
                CHECK(ip.steps.empty() && ip.slices.empty());
                for (const PlanPiece& pc : ip.pieces) CHECK(pc.ok);
            }
            for (int f = 0; f < T; f++) {
                g_case = "j: the fail-injection tid";
                PlanParams pf = p;
                pf.fail_tid = f;
                const BatchPlan pl = plan_checked({J(A, B, 4097), J(C, C, 4097, INT32), J(D, E, 2)}, pf);
                CHECK(!pl.pieces[f].ok && !pl.pieces[uT + f].ok);
                CHECK(pl.pieces[2 * uT + f].ok == (pl.pieces[2 * uT + f].numel == 0));   // an empty slice has nothing to fail
                for (const PlanSlice& s : pl.slices) CHECK((uintptr_t)s.in != A + pl.pieces[f].offset * 4);
                for (const PlanStep& st : pl.steps) CHECK(st.kind == PlanStep::kLaunch || st.first != uT + f);
                size_t ok = 0;
                for (size_t t = 0; t < uT; t++) ok += pl.pieces[t].ok;
                CHECK(ok == uT - 1);
                if (T > 1) CHECK(tables(pl)[0] == uT - 1);   // job 1's table, closed by the INT32 job
            }
            {
                g_case = "k: no pre/post-processor";
                PlanParams pn = p;
                pn.has_ppp = false;
                const BatchPlan pl = plan_checked({J(A, B, 2), J(C, D, 1000), J(0, 0, 0), J(E, E, 100, INT32)}, pn);
                CHECK(pl.steps.empty() && pl.slices.empty());
                for (const PlanPiece& pc : pl.pieces) CHECK(pc.ok == (pc.numel == 0));
            }
            for (const uint64_t bmax : {1, 8}) {
                g_case = "n: packets";
                PlanParams pb = PP(1, P);
                pb.bmax = bmax;
                const BatchPlan pl = plan_checked({J(A, A, P - 1), J(B, B, P), J(C, C, P + 1), J(D, D, 9 * P + 1)}, pb);
                CHECK(pl.pieces[0].packets == 2 && pl.pieces[1].packets == 2);
                CHECK(pl.pieces[2].packets == (bmax == 1 ? 3u : 4u));
                CHECK(pl.pieces[3].packets == 10 + bmax);
            }
        }
    {
        g_case = "m: the table cap";
        PlanParams p = PP(4, 256);
        p.max_table_slices = 8;
        const std::vector<PlanJob> three = {J(A, A, 4097), J(B, B, 100003), J(C, D, 777)};
        CHECK(tables(plan_checked(three, p)) == std::vector<size_t>({8, 4}));
        p.max_table_slices = 6;   // the cut falls inside job 2
        const BatchPlan pl = plan_checked(three, p);
        CHECK(tables(pl) == std::vector<size_t>({6, 6}));
        CHECK(pl.steps[0].fail_end == 6 && pl.steps[1].fail_first == 6 && pl.steps[1].fail_end == 12);
        // a job cut by the cap still splits a later job that shares its buffer
        CHECK(tables(plan_checked({J(A, A, 4097), J(B, C, 4097), J(C, D, 4097)}, p)) == std::vector<size_t>({6, 2, 4}));
        p.max_table_slices = 64;
        std::vector<PlanJob> many;
        for (int j = 0; j < 16; j++) many.push_back(J(A + j * 0x100000, B + j * 0x100000, 4097));
        CHECK(tables(plan_checked(many, p)) == std::vector<size_t>({64}));
    }
    if (failures) return 1;
    printf("batch plan ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("batch_plan")
    src = d / "batch_plan_check.cc"
    src.write_text(PROGRAM)
    return cxx, d, src


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_batch_plan_standalone(source, sanitize):
    cxx, d, src = source
    exe = d / ("check_san" if sanitize else "check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else ["-O2"]
    # the client's own headers only: no HIP include path, no kernel C-ABI header
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CLIENT,
                            "-o", str(exe), str(src), *SOURCES, "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "batch plan ok"


def test_batch_plan_header_needs_no_hip():
    with open(os.path.join(CLIENT, "batch_plan.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(includes) == ['"common.h"', '"fifo_scheduler.h"', "<algorithm>", "<cstdint>", "<utility>",
                                "<vector>"]
    # and what those two pull in stays inside the client, HIP-free
    for header in ("common.h", "fifo_scheduler.h", "config.h", "job.h"):
        with open(os.path.join(CLIENT, header)) as f:
            for ln in f:
                if ln.startswith("#include"):
                    assert "hip" not in ln.lower(), (header, ln)
