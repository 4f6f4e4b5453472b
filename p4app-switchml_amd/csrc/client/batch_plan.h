// batch_plan.h — what the batch worker (LoopbackBackend::BatchMain) does with
// the jobs it took in one round, decided without touching them: which FIFO
// slices share a launch of sml_roundtrip_loopback_batch_typed, where a shared
// buffer forces a new launch, which slices run one by one through run_slice,
// and which pieces a failed launch fails.  No HIP in here: addresses are
// numbers that are compared, never dereferenced, so the plan is tested on a
// CPU (tests/test_batch_plan_cpu.py).
#ifndef SWITCHML_AMD_BATCH_PLAN_H_
#define SWITCHML_AMD_BATCH_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "common.h"
#include "fifo_scheduler.h"

namespace switchml {

struct PlanJob {
    const void* in_d;   // the addresses a kernel can use for the job's tensors,
    void* out_d;        // null where the device cannot address them
    Numel numel;
    DataType data_type;
};

struct PlanParams {
    int T;                    // general.num_worker_threads: slices per job
    uint64_t P;               // general.packet_numel
    uint64_t bmax;            // max_outstanding_packets / T
    int fail_tid;             // backend.dummy.fail_worker_thread, -1: none
    bool instant;             // general.instant_job_completion
    bool has_ppp;             // a pre/post-processor exists: without one, work fails
    size_t max_table_slices;  // SML_MAX_BATCH_SLICES
};

// One entry of a launch's table (sml_typed_slice, converted where it is launched).
struct PlanSlice {
    const void* in;
    void* out;
    uint64_t numel;
    DataType data_type;
};

// One FIFO slice of one job, reported under its worker thread id.
struct PlanPiece {
    size_t job;         // index into the round's jobs
    WorkerTid tid;
    Numel offset, numel;
    uint64_t packets;   // batched pieces; a single slice's count comes from run_slice
    bool ok;            // false: published FAILED whatever the round's event says
};

struct PlanStep {
    enum Kind { kLaunch, kSingle } kind;
    // kLaunch: slices [first, first + count) of BatchPlan::slices as one table,
    //          which if it fails fails pieces [fail_first, fail_end);
    // kSingle: piece `first` through run_slice (count == 1), which if it fails
    //          fails that piece alone.
    size_t first, count;
    size_t fail_first, fail_end;
};

struct BatchPlan {
    std::vector<PlanPiece> pieces;   // T per job, in job then tid order
    std::vector<PlanSlice> slices;
    std::vector<PlanStep> steps;     // in stream (FIFO) order
};

inline BatchPlan PlanBatch(const std::vector<PlanJob>& jobs, const PlanParams& p) {
    typedef std::vector<std::pair<uintptr_t, uintptr_t>> Ranges;
    BatchPlan plan;
    Ranges reads, writes;     // kernel address ranges of the pending table
    size_t table_first = 0;   // its first slice
    size_t fail_first = 0;    // the first piece of its jobs
    auto overlaps = [](const Ranges& v, uintptr_t a, uintptr_t b) {
        for (const auto& r : v)
            if (a < r.second && r.first < b) return true;
        return false;
    };
    // Close the pending table: one launch, whose failure fails the pieces
    // collected since the table was opened.
    auto flush = [&] {
        if (plan.slices.size() > table_first)
            plan.steps.push_back(PlanStep{PlanStep::kLaunch, table_first, plan.slices.size() - table_first,
                                          fail_first, plan.pieces.size()});
        table_first = plan.slices.size();
        fail_first = plan.pieces.size();
        reads.clear();
        writes.clear();
    };
    for (size_t j = 0; j < jobs.size(); j++) {
        const PlanJob& job = jobs[j];
        const size_t esz = DataTypeSize(job.data_type);
        // empty jobs and instant_job_completion never touch the buffers
        const bool work = job.numel > 0 && !p.instant;
        // all three float types share one table
        const bool batched = work && p.has_ppp && IsFloatType(job.data_type) && job.in_d && job.out_d;
        const uintptr_t i0 = (uintptr_t)job.in_d, i1 = i0 + job.numel * esz;
        const uintptr_t o0 = (uintptr_t)job.out_d, o1 = o0 + job.numel * esz;
        if (batched) {
            // a buffer shared with an earlier job of the table: a new launch,
            // stream order keeps FIFO order (two reads of one buffer may share)
            if (overlaps(writes, i0, i1) || overlaps(writes, o0, o1) || overlaps(reads, o0, o1)) flush();
            reads.emplace_back(i0, i1);
            writes.emplace_back(o0, o1);
        } else if (work && p.has_ppp) {
            flush();   // keep FIFO order on the stream
        }
        // The first job with work opens an empty table's fail range.  (A job
        // without work between two jobs of one table lies inside the range,
        // which is contiguous.)
        if (work && plan.slices.size() == table_first) fail_first = plan.pieces.size();
        for (int tid = 0; tid < p.T; tid++) {
            PlanPiece pc{j, (WorkerTid)tid, 0, 0, 0, true};
            FifoSliceGeometry(job.numel, p.T, tid, &pc.offset, &pc.numel);
            if (!work || pc.numel == 0) {
                // an empty slice: published ok, nothing touched
            } else if (!p.has_ppp) {
                pc.ok = false;   // no pre/post-processor
            } else if (tid == p.fail_tid) {
                pc.ok = false;   // injected fault: this slice's buffers are not touched
            } else if (batched) {
                if (plan.slices.size() - table_first >= p.max_table_slices) {
                    flush();   // a table never exceeds the cap; the job goes on in the next one
                    reads.emplace_back(i0, i1);
                    writes.emplace_back(o0, o1);
                }
                const uint64_t B = pc.numel / p.P + (pc.numel % p.P != 0);
                pc.packets = B + std::min<uint64_t>(B, p.bmax);
                plan.slices.push_back(PlanSlice{static_cast<const char*>(job.in_d) + pc.offset * esz,
                                                static_cast<char*>(job.out_d) + pc.offset * esz, pc.numel,
                                                job.data_type});
            } else {
                plan.steps.push_back(PlanStep{PlanStep::kSingle, plan.pieces.size(), 1, plan.pieces.size(),
                                              plan.pieces.size() + 1});
            }
            plan.pieces.push_back(pc);
        }
    }
    flush();
    return plan;
}

}  // namespace switchml

#endif  // SWITCHML_AMD_BATCH_PLAN_H_
