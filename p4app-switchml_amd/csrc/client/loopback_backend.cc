// loopback_backend.cc — see loopback_backend.h.
#include "loopback_backend.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <vector>
#include <cstdio>
#include <memory>
#include <string>

#include "batch_plan.h"
#include "context.h"
#include "hip_exponent_quantizer_ppp.h"
#include "hip_util.h"
#include "prepostprocessor.h"
#include "xgmi_switch.h"

namespace switchml {

namespace {

// Wait for the worker's stream: poll for a short while (a slice's kernels
// usually finish within it), then block in hipStreamSynchronize.
void stream_wait(hipStream_t st) {
    const bool done = SpinUntil([st] {
        const hipError_t q = hipStreamQuery(st);
        if (q != hipSuccess && q != hipErrorNotReady) hip_ok(q, "hipStreamQuery");
        return q == hipSuccess;
    });
    if (!done) hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
}

// Grow-only device buffer owned by one worker thread, used only on that
// worker's stream.  Stream-ordered (hipFreeAsync / hipMallocAsync on the
// stream): the old buffer is released after the work already queued on it,
// and no device-wide synchronisation happens on the worker thread — hipFree
// waits for every stream of the device, which a worker serving RCCL's
// CollNet proxy must not do while RCCL's kernels wait on that proxy.
struct DeviceBuffer {
    void* p = nullptr;
    size_t cap = 0;
    hipStream_t owner = nullptr;
    void Abandon() { p = nullptr; cap = 0; }   // the owner stream is wedged: leak, never free
    void* get(size_t bytes, hipStream_t st) {
        if (bytes > cap) {
            if (p) hip_ok(hipFreeAsync(p, owner), "hipFreeAsync");
            p = nullptr;
            cap = std::max<size_t>(bytes, 4096);
            hip_ok(hipMallocAsync(&p, cap, st), "hipMallocAsync");
            owner = st;
        }
        return p;
    }
    ~DeviceBuffer() {
        if (p) (void)hipFreeAsync(p, owner);
    }
};

// Grow-only host buffer: page-locked (hipHostMalloc) or pageable (malloc).
struct HostBuffer {
    void* p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    void* get(size_t bytes, bool pin) {
        if (bytes > cap || pin != pinned) {
            release();
            cap = std::max<size_t>(bytes, 4096);
            pinned = pin;
            if (pin) hip_ok(hipHostMalloc(&p, cap, hipHostMallocDefault), "hipHostMalloc");
            else if (!(p = std::malloc(cap))) throw SwitchMLFatal("malloc failed");
        }
        return p;
    }
    void release() {
        if (!p) return;
        if (pinned) (void)hipHostFree(p);
        else std::free(p);
        p = nullptr;
        cap = 0;
    }
    ~HostBuffer() { release(); }
};

struct WorkerState {
    DeviceBuffer in, out, payload, exps, ring, ring_extra;
    HostBuffer hring, hring_extra;
    // the worker's stream is wedged (XgmiSwitch::Wedged): its unfinished work
    // may still use these buffers, so they are leaked, not freed
    void Abandon() {
        for (DeviceBuffer* b : {&in, &out, &payload, &exps, &ring, &ring_extra}) b->Abandon();
        hring.p = hring_extra.p = nullptr;
        hring.cap = hring_extra.cap = 0;
    }
};

// DummyWorkerThread's per-packet loop (dummy_worker_thread.cc:86-177) with
// in-order delivery over a device-resident ring of b packets.  The ring holds
// wire words, whatever the slice's element type (FLOAT16 / BFLOAT16 slices
// under backend.hip.half_packets: the PPP's hooks convert).
void run_packet_loop(HipExponentQuantizerPPP& ppp, const Config& cfg, WorkerState& ws, bool extra_batch) {
    const uint64_t P = ppp.ltu_numel();
    const uint64_t B = ppp.total_main_num_ltus();
    const uint64_t b = ppp.batch_num_ltus();
    const uint64_t total = B + (extra_batch ? b : 0);
    const std::string& where = cfg.backend_.hip.packet_ring;
    int32_t* ring;
    uint8_t* extra;
    if (where == "device") {
        ring = static_cast<int32_t*>(ws.ring.get(b * P * 4, ppp.stream()));
        extra = static_cast<uint8_t*>(ws.ring_extra.get(b * 2, ppp.stream()));
        hip_ok(hipMemsetAsync(ring, 0, b * P * 4, ppp.stream()), "hipMemsetAsync");
    } else {
        const bool pin = where == "pinned";
        ring = static_cast<int32_t*>(ws.hring.get(b * P * 4, pin));
        extra = static_cast<uint8_t*>(ws.hring_extra.get(b * 2, pin));
        std::memset(ring, 0, b * P * 4);
    }
    // ProcessPacket (every entry of the packet x W, dummy_backend.cc:72-84) on
    // the device for a device-addressable ring (HBM or pinned host memory, in
    // the same launch as the PPP's calls), on the CPU for a pageable one.
    //
    // The reference handles one packet per loop trip: packet p comes back,
    // ProcessPacket, PostprocessSingle(p), PreprocessSingle(p + b) into the
    // same ring slot.  Slots are independent, so the packets of one pass over
    // the ring (slots s0 .. s0 + w - 1, w <= b) go as one burst — the way a
    // DPDK worker handles an rx burst and refills its mbufs — with the same
    // calls per slot in the same order: PostprocessReuseBurst (post of p, pre
    // of p + b into the slot).  A device-addressable ring runs the whole trip,
    // ProcessPacket included, as ONE launch per pass; the HBM ring stays
    // stream-ordered (no host sync), a host ring completes each burst before
    // the call returns (the packets would go to the NIC next).
    const uint16_t W = cfg.general_.num_workers;
    const bool dev_ring = where == "device";
    const bool proc = cfg.backend_.dummy.process_packets;
    ppp.SetStreamOrdered(dev_ring);
    std::vector<uint64_t> ids(b);
    std::vector<void*> ents(b), exs(b);
    for (uint64_t p = 0; p < b; p++) {
        ids[p] = p;
        ents[p] = ring + p * P;
        exs[p] = extra + p * 2;
    }
    ppp.PreprocessBurst((uint32_t)b, ids.data(), ents.data(), exs.data());
    for (uint64_t p0 = 0; p0 < total; p0 += b) {
        const uint64_t w = std::min<uint64_t>(b, total - p0);   // p0 % b == 0: slots 0 .. w - 1
        for (uint64_t s = 0; s < w; s++) ids[s] = p0 + s;
        if (proc && where != "pageable") {
            ppp.ProcessPostprocessReuseBurst((uint32_t)w, ids.data(), ents.data(), exs.data());
            continue;
        }
        if (proc)
            for (uint64_t i = 0; i < w * P; i++)
                ring[i] = (int32_t)__builtin_bswap32(__builtin_bswap32((uint32_t)ring[i]) * (uint32_t)W);
        ppp.PostprocessReuseBurst((uint32_t)w, ids.data(), ents.data(), exs.data(), b, total);
    }
    ppp.SetStreamOrdered(false);
}

uint64_t run_slice(PrePostProcessor& base, const Config& cfg, WorkerState& ws, JobSlice& js, XgmiSwitch* xs,
                   WorkerTid tid) {
    auto* ppp = dynamic_cast<HipExponentQuantizerPPP*>(&base);
    if (!ppp) {  // bypass: count packets, move nothing (bypass_ppp.h)
        const uint64_t B = base.SetupJobSlice(&js);
        base.CleanupJobSlice();
        return B;
    }
    hipStream_t st = ppp->stream();
    Tensor& t = js.slice;
    const std::string& mode = cfg.backend_.hip.mode;
    // FLOAT16 / BFLOAT16: the bulk hooks and the fused round trip convert
    // inside the kernels, and so do the in-node switch under
    // backend.xgmi.half_types and the per-packet loop under
    // backend.hip.half_packets; without its key the per-packet loop's first
    // burst hook, or the in-node switch (XgmiSwitch::AllReduceSlice), throws
    // for such a slice, before anything is written, rather than run it as
    // another type
    const size_t bytes = t.numel * DataTypeSize(t.data_type);
    // Device tensors are used in place; pinned host tensors too, through
    // their device mapping (the kernels read and write them over PCIe, both
    // directions at once — "zero-copy"); pageable host tensors are
    // staged through HBM with copies on the worker's stream.
    const PointerInfo in = QueryPointer(t.in_ptr);
    // the in-node switch reads its input twice (exponents, then quantize):
    // a host input is copied into HBM once instead of crossing PCIe twice
    void* in_d = (xs && !in.device) ? nullptr : in.dev;
    void* out_d = QueryPointer(t.out_ptr).dev;

    JobSlice staged = js;
    if (in_d) {
        staged.slice.in_ptr = in_d;
    } else {
        staged.slice.in_ptr = ws.in.get(bytes, st);
        hip_ok(hipMemcpyAsync(staged.slice.in_ptr, t.in_ptr, bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync H2D");
    }
    if (out_d) staged.slice.out_ptr = out_d;
    else staged.slice.out_ptr = (t.out_ptr == t.in_ptr) ? staged.slice.in_ptr : ws.out.get(bytes, st);

    const uint64_t B = ppp->SetupJobSlice(&staged);
    const uint64_t P = ppp->ltu_numel();
    const uint16_t W = cfg.general_.num_workers;
    const bool is_float = IsFloatType(t.data_type);
    uint64_t packets = B + (ppp->NeedsExtraBatch() ? ppp->batch_num_ltus() : 0);

    if (xs) {
        // the in-node switch: this slice across the W workers (synchronous)
        xs->AllReduceSlice(tid, staged.slice.in_ptr, staged.slice.out_ptr, t.numel, t.data_type, st);
    } else if (mode == "packet") {
        run_packet_loop(*ppp, cfg, ws, ppp->NeedsExtraBatch());
    } else if (mode == "fused" && is_float && cfg.backend_.dummy.process_packets) {
        // FLOAT32 forwards to sml_roundtrip_loopback
        sml_ok(sml_roundtrip_loopback_typed(staged.slice.in_ptr, staged.slice.out_ptr, SmlFloatType(t.data_type),
                                            t.numel, (uint32_t)P, W, nullptr, nullptr,
                                            cfg.backend_.hip.vcl ? SML_FLAG_ROUND_RNE : 0u, st),
               "sml_roundtrip_loopback");
    } else {  // bulk
        void* payload = ws.payload.get(B * P * 4, st);
        void* exps = ws.exps.get(B, st);
        ppp->PreprocessBulk(payload, exps, nullptr, false);
        if (cfg.backend_.dummy.process_packets)
            sml_ok(sml_loopback_aggregate(static_cast<int32_t*>(payload), B * P, W, 0, st), "sml_loopback_aggregate");
        ppp->PostprocessBulk(payload, exps, false);
    }
    if (!out_d)
        hip_ok(hipMemcpyAsync(t.out_ptr, staged.slice.out_ptr, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync D2H");
    // Everything is enqueued on the worker's stream (args captured at launch):
    // the caller records an event and retires the slice when it completes.
    ppp->CleanupJobSlice();
    return packets;
}

// Wait for an event: poll for a short while (a slice's kernels usually finish
// within it), then block.
void event_wait(hipEvent_t ev) {
    const bool done = SpinUntil([ev] {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipSuccess && q != hipErrorNotReady) hip_ok(q, "hipEventQuery");
        return q == hipSuccess;
    });
    if (!done) hip_ok(hipEventSynchronize(ev), "hipEventSynchronize");
}

// The oldest in-flight entry's event, while no later job is queued yet: poll
// for either its completion or a new job (a framework posts its buckets one
// call at a time — blocking on the event would serialize the next job behind
// this one's kernels), for SpinMicros(); then block on the event.  True: the
// event completed (or failed: retiring it reports that); false: a job
// arrived first, go and overlap it.
template <class HasJob>
bool event_or_job(hipEvent_t ev, HasJob has_job) {
    bool job = false;
    SpinUntil([&] { return hipEventQuery(ev) != hipErrorNotReady || (job = has_job()); });
    return !job;
}

// The work of one worker whose kernels are still running on its stream, oldest
// first: each entry is a payload and the event recorded after its work.  The
// worker takes the next job while the GPU finishes the previous one, and every
// entry is published, in order, once its event has passed.  At most
// kMaxInFlight entries; the events are pooled and destroyed with the queue.
constexpr size_t kMaxInFlight = 4;

template <class Payload>
class InFlightQueue {
  public:
    // publish(payload, error): error is null when the entry's event completed,
    // else what waiting for it threw
    typedef std::function<void(Payload&, const char* error)> Publish;
    explicit InFlightQueue(Publish publish) : publish_(std::move(publish)) {}
    ~InFlightQueue() {
        for (hipEvent_t ev : pool_) (void)hipEventDestroy(ev);
    }

    // Record an event after the work queued on `st` so far and enter the
    // payload under it.  Throws, with the payload left to the caller, if HIP
    // refuses.
    void Push(hipStream_t st, Payload&& payload) {
        if (pool_.empty()) {
            hipEvent_t ev;
            hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
            pool_.push_back(ev);
        }
        hip_ok(hipEventRecord(pool_.back(), st), "hipEventRecord");
        entries_.push_back(Entry{pool_.back(), std::move(payload)});
        pool_.pop_back();
    }

    // Wait for the oldest entry and publish it.
    void RetireOldest() {
        Entry& e = entries_.front();
        std::string error;
        try {
            event_wait(e.ev);
        } catch (const std::exception& ex) {
            error = ex.what();
        }
        publish_(e.payload, error.empty() ? nullptr : error.c_str());
        pool_.push_back(e.ev);
        entries_.pop_front();
    }

    // A worker's first step of every round.  Retires every entry whose event
    // is no longer pending; then, if the queue is full or no job follows
    // (job_follows() is false), there is nothing to overlap with and the
    // oldest entry is finished first — unless poll_for_job is set and a job
    // arrives while it is waited for.  True: start the round again.
    template <class HasJob>
    bool Settle(HasJob job_follows, bool poll_for_job) {
        while (!entries_.empty() && hipEventQuery(entries_.front().ev) != hipErrorNotReady) RetireOldest();
        if (entries_.empty() || (entries_.size() < kMaxInFlight && job_follows())) return false;
        if (entries_.size() >= kMaxInFlight || !poll_for_job || event_or_job(entries_.front().ev, job_follows))
            RetireOldest();
        return true;
    }

    // Stopping, or a stream in doubt: the entries own their buffers until
    // their kernels finish.
    void Drain() {
        while (!entries_.empty()) RetireOldest();
    }

  private:
    struct Entry {
        hipEvent_t ev;
        Payload payload;
    };
    Publish publish_;
    std::deque<Entry> entries_;
    std::vector<hipEvent_t> pool_;
};

// One round of the batch worker: the jobs it took whole, where their tensors
// live (one query per pointer) and, once planned, their T pieces each.
struct Round {
    std::vector<std::shared_ptr<Job>> jobs;
    std::vector<PlanJob> where;   // the planner's view of each job
    bool host_input = false;      // a job reads pinned host memory (zero-copy)
    std::vector<PlanPiece> pieces;
};

JobSlice SliceOf(const Round& r, const PlanPiece& pc) {
    JobSlice js{r.jobs[pc.job], r.jobs[pc.job]->tensor_};
    js.slice.numel = pc.numel;
    js.slice.OffsetPtrs(pc.offset);
    return js;
}

// Take the queued jobs, up to max_jobs in the round (blocks while the round is
// empty and nothing is queued); false when the context stopped instead.
bool TakeJobs(Context& ctx, size_t max_jobs, Round& r, uint64_t& last_seq) {
    if (!ctx.GetJobs(max_jobs, r.jobs)) return false;
    last_seq = r.jobs.back()->sched_seq.load(std::memory_order_relaxed);
    for (size_t j = r.where.size(); j < r.jobs.size(); j++) {
        const Tensor& t = r.jobs[j]->tensor_;
        const PointerInfo in = t.numel > 0 ? QueryPointer(t.in_ptr) : PointerInfo();
        const PointerInfo out = t.numel > 0 ? QueryPointer(t.out_ptr) : PointerInfo();
        r.where.push_back(PlanJob{in.dev, out.dev, t.numel, t.data_type});
        r.host_input = r.host_input || in.host_mapped();
    }
    return true;
}

// Zero-copy host buckets: a framework posts its buckets one call at a time, so
// the first one would otherwise go alone into a small launch; PCIe moves
// 31 GB/s each way in a 26 MB launch but 37-42 in 100 MB+ ones
// (profiles/r02/zero_copy_probes.json).  While the next job follows within
// coalesce_us of the last, it joins this round.
void CoalesceHostBuckets(Context& ctx, uint32_t coalesce_us, size_t max_jobs, Round& r, uint64_t& last_seq) {
    if (coalesce_us == 0 || !r.host_input) return;
    auto last = std::chrono::steady_clock::now();
    while (r.jobs.size() < max_jobs && ctx.GetContextState() == Context::RUNNING) {
        if (ctx.HasJobAfter(last_seq)) {
            if (!TakeJobs(ctx, max_jobs, r, last_seq)) break;
            last = std::chrono::steady_clock::now();
        } else if (std::chrono::steady_clock::now() - last > std::chrono::microseconds(coalesce_us)) {
            break;
        } else {
            std::this_thread::yield();
        }
    }
}

// Queue the plan's steps on the pre/post-processor's stream, in order.  A step
// that fails fails exactly its own pieces, after the stream has drained:
// nothing may still touch their buffers when they are published FAILED.
void ExecutePlan(const BatchPlan& plan, Round& r, Context& ctx, const Config& cfg, HipExponentQuantizerPPP& ppp,
                 WorkerState& ws) {
    const uint32_t rne = cfg.backend_.hip.vcl ? SML_FLAG_ROUND_RNE : 0u;   // the VCL=1 build's rounding
    std::vector<sml_typed_slice> table;
    for (const PlanStep& s : plan.steps) {
        try {
            if (s.kind == PlanStep::kLaunch) {   // fp32, fp16 and bf16 slices in one table
                table.clear();
                for (size_t i = s.first; i < s.first + s.count; i++) {
                    const PlanSlice& sl = plan.slices[i];
                    table.push_back(sml_typed_slice{sl.in, sl.out, sl.numel, (uint32_t)sl.data_type, 0u});
                }
                ctx.GetStats().AddBatchCall(table.size());
                sml_ok(sml_roundtrip_loopback_batch_typed(table.data(), (uint32_t)table.size(),
                                                          (uint32_t)cfg.general_.packet_numel,
                                                          cfg.general_.num_workers, rne, ppp.stream()),
                       "sml_roundtrip_loopback_batch_typed");
            } else {   // INT32 and pageable-host slices
                PlanPiece& pc = r.pieces[s.first];
                JobSlice js = SliceOf(r, pc);
                ctx.GetStats().AddSingleSlice();
                pc.packets = run_slice(ppp, cfg, ws, js, nullptr, pc.tid);
            }
        } catch (const std::exception& e) {
            fprintf(stderr, "[switchml] batch worker: job %llu failed: %s\n",
                    (unsigned long long)r.jobs[r.pieces[s.fail_first].job]->id_, e.what());
            (void)hipStreamSynchronize(ppp.stream());
            for (size_t i = s.fail_first; i < s.fail_end; i++) r.pieces[i].ok = false;
        }
    }
}

}  // namespace

void* DeviceAddress(void* p) { return QueryPointer(p).dev; }
bool IsDevicePointer(const void* p) { return QueryPointer(p).device; }

LoopbackBackend::LoopbackBackend(Context& context, Config& config) : context_(context), config_(config) {}

LoopbackBackend::~LoopbackBackend() { CleanupWorker(); }

void LoopbackBackend::SetupWorker() {
    if (config_.general_.backend == "xgmi" && !xgmi_) xgmi_.reset(new XgmiSwitch(config_, context_.device()));
    if (BatchEligible()) {
        threads_.emplace_back(&LoopbackBackend::BatchMain, this);
        return;
    }
    for (int i = 0; i < config_.general_.num_worker_threads; i++)
        threads_.emplace_back(&LoopbackBackend::WorkerMain, this, (WorkerTid)i);
}

bool LoopbackBackend::BatchEligible() const {
    const GeneralConfig& g = config_.general_;
    return config_.backend_.hip.batch_jobs > 0 && config_.backend_.hip.mode == "fused" && g.backend == "dummy" &&
           g.prepostprocessor != "bypass" && config_.backend_.dummy.process_packets &&
           config_.backend_.dummy.bandwidth <= 0;
}

// Batched dispatch.  The reference's worker threads each run their FIFO slice
// of every job (dummy_worker_thread.cc:73-177) because a CPU core is the unit
// of parallelism; on the GPU one launch already fills the chip, so here ONE
// thread takes the queued jobs whole and runs every slice of up to
// batch_jobs of them in one sml_roundtrip_loopback_batch_typed call — the
// same slice geometry (so the same bits) with one launch per element type
// present (FLOAT32, FLOAT16, BFLOAT16) and one event per batch instead of
// num_worker_threads launches per job.  Jobs whose buffers overlap an
// earlier job of the batch start a new launch (stream order keeps them in
// FIFO order); INT32 and pageable-host jobs run slice by slice through
// run_slice on the same stream.  Completion of every slice is reported under
// its own worker thread id, so the scheduler, Stats and failure semantics are
// those of the threaded path.
// What shares a launch, what splits one and what a failure fails is decided
// by PlanBatch (batch_plan.h); the rounds in flight are an InFlightQueue.
void LoopbackBackend::BatchMain() {
    const GeneralConfig& g = config_.general_;
    const int T = g.num_worker_threads;
    std::shared_ptr<PrePostProcessor> ppp;
    try {
        hip_ok(hipSetDevice(context_.device()), "hipSetDevice");
        ppp = PrePostProcessor::CreateInstance(config_, 0, g.packet_numel * 4, g.max_outstanding_packets / T);
    } catch (const std::exception& e) {
        fprintf(stderr, "[switchml] batch worker: %s\n", e.what());
    }
    auto* hip_ppp = dynamic_cast<HipExponentQuantizerPPP*>(ppp.get());
    const size_t max_jobs = std::max<size_t>(1, std::min<size_t>(config_.backend_.hip.batch_jobs,
                                                                  SML_MAX_BATCH_SLICES / std::max(1, T)));
    const PlanParams params{T, g.packet_numel, g.max_outstanding_packets / T, config_.backend_.dummy.fail_worker_thread,
                            g.instant_job_completion, hip_ppp != nullptr, SML_MAX_BATCH_SLICES};
    auto publish = [this](Round& r, const char* error) {
        if (error) fprintf(stderr, "[switchml] batch worker: %s\n", error);
        for (const PlanPiece& pc : r.pieces) {
            const JobSlice js = SliceOf(r, pc);
            const bool good = !error && pc.ok;
            if (good) context_.GetStats().AddSlice(pc.tid, pc.packets, pc.numel * DataTypeSize(js.slice.data_type));
            context_.NotifyJobSliceCompletion(pc.tid, js, good);
        }
    };
    InFlightQueue<Round> inflight(publish);
    WorkerState ws;
    uint64_t last_seq = 0;
    while (context_.GetContextState() == Context::RUNNING) {
        // Nothing to overlap with: finish the oldest round first.  (Unlike the
        // threaded path this does not poll for a new job meanwhile: jobs that
        // arrive while the round runs join the next launch — for zero-copy
        // host buckets larger launches move more bytes per second over PCIe;
        // measured: configs[4] pinned 2.95 ms this way, 3.23 ms polling.)
        if (inflight.Settle([&] { return context_.HasJobAfter(last_seq); }, false)) continue;
        Round cur;
        if (!TakeJobs(context_, max_jobs, cur, last_seq)) continue;
        CoalesceHostBuckets(context_, config_.backend_.hip.coalesce_us, max_jobs, cur, last_seq);
        BatchPlan plan = PlanBatch(cur.where, params);
        cur.pieces = std::move(plan.pieces);
        if (hip_ppp) ExecutePlan(plan, cur, context_, config_, *hip_ppp, ws);
        // Every job taken here shares ONE completion event, recorded after
        // the last launch: jobs that must be split into several launches do
        // not pay an event between kernels each.
        try {
            if (!hip_ppp) throw SwitchMLFatal("no pre/post-processor");
            inflight.Push(hip_ppp->stream(), std::move(cur));
        } catch (const std::exception& e) {
            if (hip_ppp) (void)hipStreamSynchronize(hip_ppp->stream());   // nothing may still touch the buffers
            inflight.Drain();
            publish(cur, e.what());
        }
    }
    // stopping: rounds in flight own their buffers until their kernels finish
    inflight.Drain();
}

void LoopbackBackend::CleanupWorker() {
    {
        std::lock_guard<std::mutex> lk(wire_mutex_);
    }
    wire_cv_.notify_all();
    for (auto& t : threads_)
        if (t.joinable()) t.join();
    threads_.clear();
    xgmi_.reset();   // leave the session (a barrier with the other workers)
}

void LoopbackBackend::WorkerMain(WorkerTid tid) {
    const GeneralConfig& g = config_.general_;
    const bool bypass = g.prepostprocessor == "bypass";
    std::shared_ptr<PrePostProcessor> ppp;
    std::string setup_error;
    try {
        if (!bypass) hip_ok(hipSetDevice(context_.device()), "hipSetDevice");
        // dummy_worker_thread.cc:59-62: ltu = packet_numel * 4 bytes, b_max = mop / T
        ppp = PrePostProcessor::CreateInstance(config_, tid, g.packet_numel * 4,
                                               g.max_outstanding_packets / g.num_worker_threads);
    } catch (const std::exception& e) {
        setup_error = e.what();
        fprintf(stderr, "[switchml] worker thread %d: %s\n", tid, e.what());
    }
    auto* hip_ppp = dynamic_cast<HipExponentQuantizerPPP*>(ppp.get());
    const float bw = config_.backend_.dummy.bandwidth;
    // Slices whose kernels are still running (InFlightQueue); the simulated
    // wire (bandwidth > 0) keeps the strict one-at-a-time loop of
    // dummy_worker_thread.cc.
    struct InFlight {
        JobSlice js;
        uint64_t packets;
    };
    InFlightQueue<InFlight> inflight([this, tid](InFlight& f, const char* error) {
        if (error)
            fprintf(stderr, "[switchml] worker thread %d: job %llu failed: %s\n", tid,
                    (unsigned long long)f.js.job->id_, error);
        else
            context_.GetStats().AddSlice(tid, f.packets, f.js.slice.numel * DataTypeSize(f.js.slice.data_type));
        context_.NotifyJobSliceCompletion(tid, f.js, !error);
    });
    WorkerState ws;
    JobSlice js;
    uint64_t last_seq = 0;  // sched_seq of the last job this thread took a slice of
    // this worker's stream did not finish within the in-node switch's bounded
    // wait: every later slice fails at once, nothing waits on the stream again
    bool wedged = false;
    const DummyBackendConfig& dummy = config_.backend_.dummy;
    while (context_.GetContextState() == Context::RUNNING) {
        // nothing to overlap with (yet): finish the oldest slice, unless a job arrives first
        if (inflight.Settle([&] { return context_.HasJobAfter(last_seq); }, true)) continue;
        if (!context_.GetJobSlice(tid, js)) continue;
        last_seq = js.job->sched_seq.load(std::memory_order_relaxed);
        // empty slices and instant_job_completion never touch the PPP
        // (dummy_worker_thread.cc:87-93)
        const bool work = js.slice.numel > 0 && !g.instant_job_completion;
        bool ok = !work || ppp != nullptr;
        if (work && tid == config_.backend_.dummy.fail_worker_thread) {   // injected fault
            ok = false;
            // with the in-node switch the fault fails the exchange for every
            // worker (as a real mid-exchange failure does), not a barrier wait
            if (xgmi_) xgmi_->Poison();
        }
        if (work && wedged) ok = false;
        uint64_t packets = 0;
        if (ok && work) {
            try {
                if (hip_ppp && tid == dummy.stall_worker_thread && dummy.stall_ms > 0)   // injected stall
                    sml_ok(sml_debug_stall(dummy.stall_ms * 1000u, hip_ppp->stream()), "sml_debug_stall");
                packets = run_slice(*ppp, config_, ws, js, xgmi_.get(), tid);
                if (hip_ppp && bw <= 0) {
                    inflight.Push(hip_ppp->stream(), InFlight{js, packets});
                    js = JobSlice();
                    continue;
                }
                if (hip_ppp) stream_wait(hip_ppp->stream());
            } catch (const std::exception& e) {
                fprintf(stderr, "[switchml] worker thread %d: job %llu failed: %s\n", tid,
                        (unsigned long long)js.job->id_, e.what());
                // nothing may still touch the buffers when the slice is
                // published FAILED.  With the in-node switch the wait is
                // bounded (backend.xgmi.timeout_ms): a device that does not
                // finish fails the slice now, and the worker, its stream and
                // buffers are abandoned rather than blocking here forever.
                if (hip_ppp && xgmi_) {
                    if (xgmi_->Wedged() || !xgmi_->WaitBounded(hip_ppp->stream())) {
                        wedged = true;
                        hip_ppp->Abandon();   // its stream stays alive: the switch's reaper waits on it
                        ws.Abandon();
                        xgmi_->NoteStuckStream(tid, hip_ppp->stream());
                    }
                } else if (hip_ppp) {
                    (void)hipStreamSynchronize(hip_ppp->stream());
                }
                ok = false;
            }
            if (ok && bw > 0) {  // the dummy backend's simulated wire time (dummy_backend.cc:124-133)
                const double ns = 1000.0 * (double)packets * g.packet_numel * 4 * 8 * g.num_worker_threads / bw;
                // interruptible: Stop() must not wait out a simulated wire
                std::unique_lock<std::mutex> lk(wire_mutex_);
                wire_cv_.wait_for(lk, std::chrono::nanoseconds((int64_t)std::min(ns, 9.0e18)),
                                  [this] { return context_.GetContextState() != Context::RUNNING; });
            }
            if (ok) context_.GetStats().AddSlice(tid, packets, js.slice.numel * DataTypeSize(js.slice.data_type));
        }
        context_.NotifyJobSliceCompletion(tid, js, ok);
        js = JobSlice();
    }
    // stopping: the in-flight slices still own their buffers until their
    // kernels finish; then they are published (FAILED: the context stopped)
    inflight.Drain();
}

}  // namespace switchml
