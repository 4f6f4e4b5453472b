// xgmi_switch.cc — see xgmi_switch.h.
#include "xgmi_switch.h"

#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <thread>

#include "hip_exponent_quantizer_ppp.h"
#include "hip_util.h"

namespace switchml {

namespace {

constexpr uint32_t kMagic = 0x534d4c58u;   // "SMLX"
constexpr int kMaxW = SML_MAX_SWITCH_WORKERS;
constexpr int kMaxT = 16;
constexpr size_t kHandle = sizeof(hipIpcMemHandle_t);

constexpr const char* kWho = "xgmi switch: ";   // every message here starts with it (hip_ok, sml_ok, Fatal)

[[noreturn]] void Fatal(const std::string& what) { throw SwitchMLFatal(kWho + what); }

// Reapers of wedged switches (XgmiSwitch::Wedged): how many are still
// waiting for their streams to drain before they free what they hold.
std::mutex g_reap_mu;
std::condition_variable g_reap_cv;
int g_reaping = 0;

}  // namespace

// The session segment (zero-filled when created).
struct alignas(64) ShmBarrier {
    std::atomic<uint32_t> count;
    std::atomic<uint32_t> gen;
    char pad[56];
};

struct ShmPlanes {
    unsigned char exps[kHandle], payload[kHandle], out[kHandle];
    std::atomic<uint32_t> published;
};

struct XgmiShm {
    std::atomic<uint32_t> magic;
    uint32_t W, T, P;
    uint64_t cap;
    std::atomic<int32_t> creator_pid;      // worker 0, which creates the segment (O_EXCL)
    std::atomic<uint32_t> poisoned;        // a worker failed inside an exchange: every later barrier throws
    std::atomic<uint32_t> attached;
    std::atomic<uint32_t> detached;
    uint32_t push;                         // backend.xgmi.push of worker 0 (every worker must match)
    uint32_t half_types;                   // backend.xgmi.half_types of worker 0 (likewise)
    std::atomic<uint32_t> disagree;        // a worker's configuration does not match worker 0's: every worker fails setup
    ShmBarrier bar[kMaxT + 1];             // [t]: worker thread t; [kMaxT]: setup / teardown
    ShmPlanes planes[kMaxW][kMaxT];
};

static_assert(std::atomic<uint32_t>::is_always_lock_free, "shared-memory atomics must be lock-free");

namespace {
bool pid_alive(int32_t pid) { return pid > 0 && (kill(pid, 0) == 0 || errno == EPERM); }

// mmap of a segment another process creates: worker 0 sizes it (ftruncate)
// only after its O_EXCL create, so a file opened in between is still 0 bytes
// and touching its mapping would raise SIGBUS.  A segment shorter than
// XgmiShm is "not ready" (or stale): closed, nullptr returned.  Closes fd.
XgmiShm* map_sized(int fd, int prot) {
    struct stat st;
    void* m = MAP_FAILED;
    if (fstat(fd, &st) == 0 && (uint64_t)st.st_size >= sizeof(XgmiShm))
        m = mmap(nullptr, sizeof(XgmiShm), prot, MAP_SHARED, fd, 0);
    close(fd);
    return m == MAP_FAILED ? nullptr : static_cast<XgmiShm*>(m);
}

// A plane's IPC handle into its field of the segment (ShmPlanes).
void export_plane(const void* plane, unsigned char* field) {
    hipIpcMemHandle_t h;
    hip_ok(hipIpcGetMemHandle(&h, const_cast<void*>(plane)), "hipIpcGetMemHandle", kWho);
    memcpy(field, &h, kHandle);
}
}  // namespace

// Worker 0 creates the segment (O_EXCL), replacing one left behind by a run
// whose worker 0 is gone; the other workers wait for a segment whose creator
// is alive.  So no worker joins a crashed run's barrier counts or handles.
void XgmiSwitch::OpenSegment() {
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms_);
    if (rank_ == 0) {
        for (int attempt = 0;; attempt++) {
            const int fd = shm_open(name_.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
            if (fd >= 0) {
                created_ = true;
                const bool sized = ftruncate(fd, sizeof(XgmiShm)) == 0;
                void* m = sized ? mmap(nullptr, sizeof(XgmiShm), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0)
                                : MAP_FAILED;
                close(fd);
                if (m == MAP_FAILED) Fatal("mapping " + name_ + ": " + strerror(errno));
                shm_ = static_cast<XgmiShm*>(m);
                shm_->W = (uint32_t)W_;
                shm_->T = (uint32_t)T_;
                shm_->P = P_;
                shm_->cap = cap_;
                shm_->push = push_ ? 1u : 0u;
                shm_->half_types = half_types_ ? 1u : 0u;
                shm_->creator_pid.store(getpid());
                shm_->magic.store(kMagic, std::memory_order_release);
                return;
            }
            if (errno != EEXIST || attempt > 3) Fatal("shm_open " + name_ + ": " + strerror(errno));
            const int fe = shm_open(name_.c_str(), O_RDONLY, 0600);
            if (fe >= 0) {
                // a segment too short to hold the header is stale (its creator
                // died between create and size): replaced below
                if (XgmiShm* o = map_sized(fe, PROT_READ)) {
                    const int32_t pid = o->creator_pid.load();
                    munmap(o, sizeof(XgmiShm));
                    if (pid_alive(pid) && pid != getpid())
                        Fatal("session " + name_ + " is in use by process " + std::to_string(pid) +
                              " (pick another backend.xgmi.session)");
                }
            }
            fprintf(stderr, "[switchml] %sreplacing %s left behind by an earlier run\n", kWho, name_.c_str());
            shm_unlink(name_.c_str());
        }
    }
    for (;;) {
        const int fd = shm_open(name_.c_str(), O_RDWR, 0600);
        if (fd >= 0) {
            // not yet sized by worker 0: not ready, retry (map_sized)
            if (XgmiShm* s = map_sized(fd, PROT_READ | PROT_WRITE)) {
                void* m = s;
                while (s->magic.load(std::memory_order_acquire) != kMagic &&
                       std::chrono::steady_clock::now() < deadline)
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                if (s->magic.load(std::memory_order_acquire) == kMagic && pid_alive(s->creator_pid.load())) {
                    shm_ = s;
                    return;
                }
                munmap(m, sizeof(XgmiShm));   // stale: worker 0 replaces it
            }
        }
        if (std::chrono::steady_clock::now() > deadline)
            Fatal("worker 0 did not open session " + name_ + " within backend.xgmi.timeout_ms");
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
}

XgmiSwitch::XgmiSwitch(const Config& config, int device) {
    const GeneralConfig& g = config.general_;
    rank_ = g.rank;
    W_ = g.num_workers;
    T_ = g.num_worker_threads;
    P_ = (uint32_t)g.packet_numel;
    cap_ = (config.backend_.xgmi.max_slice_numel + 1023) / 1024 * 1024;
    timeout_ms_ = config.backend_.xgmi.timeout_ms;
    round_flags_ = config.backend_.hip.vcl ? SML_FLAG_ROUND_RNE : 0u;
    push_ = config.backend_.xgmi.push;
    half_types_ = config.backend_.xgmi.half_types;
    fail_setup_ = config.backend_.xgmi.fail_setup;
    if (W_ < 1 || W_ > kMaxW) Fatal("num_workers must be 1..16");
    if (T_ < 1 || T_ > kMaxT) Fatal("num_worker_threads must be 1..16");
    if (rank_ < 0 || rank_ >= W_) Fatal("general.rank must be < num_workers");
    name_ = "/switchml-" + config.backend_.xgmi.session;
    try {
        Setup(device);
    } catch (...) {
        // a worker that joined the session and then failed (e.g. it cannot
        // map a peer's plane: the first contact with another GPU) poisons
        // it, so the peers' first exchange fails at once instead of waiting
        // out backend.xgmi.timeout_ms at a barrier this worker never reaches
        if (attached_) Poison();
        Release();   // no planes, mappings or segment left behind by a failed construction
        throw;
    }
}

void XgmiSwitch::Setup(int device) {
    hip_ok(hipSetDevice(device), "hipSetDevice", kWho);
    device_ = device;
    {
        // an earlier switch of this process that wedged still holds peer
        // mappings until its streams drain: wait for its reaper (bounded)
        std::unique_lock<std::mutex> lk(g_reap_mu);
        if (!g_reap_cv.wait_for(lk, std::chrono::milliseconds(timeout_ms_), [] { return g_reaping == 0; }))
            Fatal("an earlier session's device work has not finished (its planes and "
                  "peer mappings are still held); restart the process");
    }
    OpenSegment();
    if (shm_->attached.fetch_add(1) >= (uint32_t)W_) Fatal("session " + name_ + " already has num_workers workers");
    attached_ = true;

    const uint64_t cap_b = (cap_ + 63) / 64 + 64;   // blocks at the smallest packet size, padded
    planes_.resize(T_);
    for (int t = 0; t < T_; t++) {
        ThreadPlanes& tp = planes_[t];
        hip_ok(hipMalloc(&tp.exps, cap_b), "hipMalloc", kWho);
        // + W packets of the largest size: the inbox's W rows of ceil(B / W)
        // blocks may exceed B blocks by up to W - 1 (push form; xgmi_shards.h)
        hip_ok(hipMalloc(&tp.payload, (cap_ + (uint64_t)kMaxW * 1024) * 4), "hipMalloc", kWho);
        hip_ok(hipMalloc(&tp.out, cap_ * 4), "hipMalloc", kWho);
        hip_ok(hipMalloc(&tp.gexp, cap_b), "hipMalloc", kWho);
        hip_ok(hipStreamCreateWithFlags(&tp.xst, hipStreamNonBlocking), "hipStreamCreate", kWho);
        ShmPlanes& sp = shm_->planes[rank_][t];
        export_plane(tp.exps, sp.exps);
        export_plane(tp.payload, sp.payload);
        export_plane(tp.out, sp.out);
        sp.published.store(1, std::memory_order_release);
    }
    Barrier(kMaxT);   // every worker's handles are published
    // The outcome of this worker's setup is held back until every worker has
    // imported (or failed to import) every peer's planes: a worker that
    // failed must not free its exported planes while a peer is still inside
    // hipIpcOpenMemHandle on them — the importer then hangs in the runtime
    // (measured on MI355X, the N = 8 first-contact rehearsal: > 90 s).
    // A worker that differs from worker 0 says so in the segment, so that
    // every worker (worker 0 included, which cannot see it otherwise) fails
    // setup with the same error once all have compared.
    const char* disagree =
        "workers disagree on num_workers / num_worker_threads / packet_numel / max_slice_numel / push / half_types";
    std::string err;
    if (shm_->W != (uint32_t)W_ || shm_->T != (uint32_t)T_ || shm_->P != P_ || shm_->cap != cap_ ||
        shm_->push != (push_ ? 1u : 0u) || shm_->half_types != (half_types_ ? 1u : 0u)) {
        shm_->disagree.store(1, std::memory_order_release);
        err = disagree;
    } else if (fail_setup_)
        err = "injected setup failure (backend.xgmi.fail_setup)";
    else
        try {
            OpenPeers();
        } catch (const std::exception& e) {
            err = e.what();
        }
    try {
        Barrier(kMaxT);   // every worker is done importing
    } catch (const std::exception& e) {
        if (err.empty()) err = e.what();
    }
    if (shm_->disagree.load(std::memory_order_acquire)) err = disagree;
    if (!err.empty()) throw SwitchMLFatal(err.rfind(kWho, 0) == 0 ? err : kWho + err);
}

// A peer's plane from its handle in the segment, recorded for ClosePeers.
void* XgmiSwitch::ImportPlane(const unsigned char* field) {
    void* p;
    hipIpcMemHandle_t h;
    memcpy(&h, field, kHandle);
    hip_ok(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle", kWho);
    opened_.push_back(p);
    return p;
}

// Map every peer's planes of every worker thread (hipIpc; over xGMI on a node).
void XgmiSwitch::OpenPeers() {
    for (int t = 0; t < T_; t++) {
        ThreadPlanes& tp = planes_[t];
        tp.peer_exps.resize(W_);
        tp.peer_payload.resize(W_);
        tp.peer_out.resize(W_);
        for (int w = 0; w < W_; w++) {
            if (w == rank_) {
                tp.peer_exps[w] = tp.exps;
                tp.peer_payload[w] = tp.payload;
                tp.peer_out[w] = tp.out;
                continue;
            }
            const ShmPlanes& sp = shm_->planes[w][t];
            if (!sp.published.load(std::memory_order_acquire)) Fatal("peer planes missing");
            tp.peer_exps[w] = static_cast<const int8_t*>(ImportPlane(sp.exps));
            tp.peer_payload[w] = static_cast<const int32_t*>(ImportPlane(sp.payload));
            tp.peer_out[w] = static_cast<const float*>(ImportPlane(sp.out));
        }
    }
}

void XgmiSwitch::ClosePeers(std::vector<void*>& opened) {
    for (void* p : opened) (void)hipIpcCloseMemHandle(p);
    opened.clear();
}

void XgmiSwitch::FreePlanes(ThreadPlanes& tp) {
    (void)hipFree(tp.exps);
    (void)hipFree(tp.payload);
    (void)hipFree(tp.out);
    (void)hipFree(tp.gexp);
    if (tp.xst) (void)hipStreamDestroy(tp.xst);
}

// Everything this worker holds, in reverse order of Setup; safe on a
// partially built instance.
void XgmiSwitch::Release() {
    if (Wedged() && (!planes_.empty() || !opened_.empty())) {
        // device work that has not finished may still use the planes, the
        // peer mappings and the streams: a detached reaper frees them once
        // every stream involved has drained (never, if the device is hung)
        fprintf(stderr, "[switchml] %sdevice work did not finish; %zu planes and %zu peer mappings "
                        "are freed once it does\n", kWho, planes_.size() * 4, opened_.size());
        struct Remains {
            std::vector<ThreadPlanes> planes;
            std::vector<void*> opened;
            int device;
        };
        auto* rem = new Remains{std::move(planes_), std::move(opened_), device_};
        planes_.clear();
        opened_.clear();
        {
            std::lock_guard<std::mutex> lk(g_reap_mu);
            g_reaping++;
        }
        std::thread([rem] {
            (void)hipSetDevice(rem->device);
            for (ThreadPlanes& tp : rem->planes) {
                if (tp.stuck) (void)hipStreamSynchronize(tp.stuck);
                if (tp.xst) (void)hipStreamSynchronize(tp.xst);
            }
            ClosePeers(rem->opened);
            for (ThreadPlanes& tp : rem->planes) FreePlanes(tp);
            delete rem;
            std::lock_guard<std::mutex> lk(g_reap_mu);
            g_reaping--;
            g_reap_cv.notify_all();
        }).detach();
    }
    ClosePeers(opened_);
    for (ThreadPlanes& tp : planes_) FreePlanes(tp);
    planes_.clear();
    if (!shm_) return;
    bool last = false;
    if (attached_) last = shm_->detached.fetch_add(1) + 1 == (uint32_t)W_;
    const bool poisoned = shm_->poisoned.load() != 0;
    munmap(shm_, sizeof(XgmiShm));
    shm_ = nullptr;
    // the last worker out removes the name; so does worker 0 when the session
    // failed (no peer may join it again)
    if (last || (created_ && poisoned)) shm_unlink(name_.c_str());
}

XgmiSwitch::~XgmiSwitch() {
    if (!shm_) return;
    if (Wedged()) Poison();   // the peers must not wait for this worker's teardown barriers
    if (!shm_->poisoned.load()) {
        try {
            Barrier(kMaxT);   // nobody reads a peer's planes any more
        } catch (...) {
        }
        ClosePeers(opened_);
        try {
            Barrier(kMaxT);   // every mapping of our planes is closed
        } catch (...) {
        }
    }
    Release();
}

void XgmiSwitch::NoteStuckStream(int tid, hipStream_t st) {
    if (tid >= 0 && tid < (int)planes_.size()) planes_[tid].stuck = st;
}

void XgmiSwitch::Poison() {
    if (shm_) shm_->poisoned.store(1, std::memory_order_release);
}

void XgmiSwitch::ThrowIfPoisoned() {
    if (shm_->poisoned.load(std::memory_order_acquire)) Fatal("the session failed on another worker");
}

// Sense-reversing barrier over the W workers (one per worker thread, so the
// T slices of a job are exchanged independently).  Polls; a worker that does
// not arrive within backend.xgmi.timeout_ms fails the slice.
void XgmiSwitch::Barrier(int index) {
    ShmBarrier& b = shm_->bar[index];
    ThrowIfPoisoned();
    const uint32_t g = b.gen.load(std::memory_order_acquire);
    if (b.count.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)W_) {
        b.count.store(0, std::memory_order_relaxed);
        b.gen.store(g + 1, std::memory_order_release);
        return;
    }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms_);
    uint32_t spins = 0;
    while (b.gen.load(std::memory_order_acquire) == g) {
        if (++spins > 256) {
            std::this_thread::yield();
            if ((spins & 1023) == 0) {
                // A worker that failed mid-exchange poisons the session: its
                // arrival (or absence) would put every later barrier of this
                // thread index out of phase, so nobody proceeds past it.
                ThrowIfPoisoned();
                if (std::chrono::steady_clock::now() > deadline) {
                    Poison();
                    Fatal("barrier timeout (a worker did not arrive)");
                }
            }
        }
    }
}

bool XgmiSwitch::StreamSync(hipStream_t st, bool bounded_only) {
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms_);
    for (uint32_t spins = 0;; spins++) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) return true;
        if (q != hipErrorNotReady) {
            wedged_.store(true, std::memory_order_release);   // a failed stream: its work's state is unknown
            if (bounded_only) return false;
            hip_ok(q, "hipStreamQuery", kWho);
        }
        if (spins > 256) {
            std::this_thread::yield();
            if ((spins & 1023) == 0 && std::chrono::steady_clock::now() > deadline) {
                wedged_.store(true, std::memory_order_release);
                if (bounded_only) return false;
                Fatal("device work did not finish within backend.xgmi.timeout_ms");
            }
        }
    }
}

namespace {
// The writer's half of every hand-off to the peers: write
// this GPU's L2 back before the stream sync that precedes the barrier.
void release(hipStream_t st) { sml_ok(sml_release_to_peers(st), "sml_release_to_peers", kWho); }
constexpr uint32_t kPeer = SML_FLAG_PEER_PLANES;   // the reader's half: acquire in the reading kernels

// Element `i` of a buffer of `type` elements (a tensor slice, or an out plane:
// cap_ floats, which a 16-bit slice uses as a plane of cap_ 2-byte elements).
const void* at(const void* p, uint64_t i, DataType type) { return static_cast<const char*>(p) + i * DataTypeSize(type); }
void* at(void* p, uint64_t i, DataType type) { return static_cast<char*>(p) + i * DataTypeSize(type); }
// What the typed copy takes: a float type as the kernels know it, INT32 as itself.
sml_data_type_t CopyType(DataType type) { return type == INT32 ? SML_INT32 : SmlFloatType(type); }
}  // namespace

// The end of every phase of an exchange: release what the phase wrote for
// the peers, wait (bounded) for every stream the phase used, in the order
// given, then meet the peers at worker thread tid's barrier.
void XgmiSwitch::HandOff(int tid, std::initializer_list<PhaseStream> streams) {
    for (const PhaseStream& s : streams)
        if (s.release) release(s.st);
    for (const PhaseStream& s : streams) StreamSync(s.st);
    Barrier(tid);
}

// The switch's exponent max over the W planes into gexp, then K3: quantize
// with the global exponents into the own BE payload plane (pull), or each
// shard w straight into row `rank` of worker w's inbox (push: one K3 launch
// per shard, W − 1 of them writing over xGMI).  `in` holds elements of
// `type` (a float type; FLOAT32 forwards to sml_quantize_pack).
void XgmiSwitch::Quantize(ThreadPlanes& tp, const void* in, DataType type, const ShardPlan& plan, hipStream_t st) {
    const uint16_t W = (uint16_t)W_;
    const sml_data_type_t dt = SmlFloatType(type);
    sml_ok(sml_switch_exps(tp.peer_exps.data(), W, plan.B, tp.gexp, kPeer, st), "sml_switch_exps", kWho);
    if (!push_) {
        sml_ok(sml_quantize_pack_typed(in, dt, plan.n, P_, W, tp.gexp, tp.payload, nullptr, round_flags_, st),
               "sml_quantize_pack", kWho);
        return;
    }
    for (int w = 0; w < W_; w++) {
        const Shard sh = plan.shard(w);
        if (!sh.nb) continue;
        int32_t* row = const_cast<int32_t*>(tp.peer_payload[w]) + plan.inbox_row(rank_);
        sml_ok(sml_quantize_pack_typed(at(in, sh.offset, type), dt, sh.numel, P_, W, tp.gexp + sh.b0, row, nullptr,
                                       round_flags_, st), "sml_quantize_pack", kWho);
    }
}

// K6: the wrapping sum of this worker's shard over the W planes, dequantized
// into the own output plane as elements of `type` (a 16-bit type: narrowed
// here, once, so every worker ends with the owner's bits).
void XgmiSwitch::Aggregate(ThreadPlanes& tp, DataType type, const ShardPlan& plan, hipStream_t st) {
    const Shard sh = plan.shard(rank_);
    if (!sh.nb) return;
    const int32_t* planes[kMaxW];
    const int8_t* exps[kMaxW];
    for (int w = 0; w < W_; w++) {
        // pull: worker w's plane at this shard; push: row w of the own inbox
        planes[w] = push_ ? tp.payload + plan.inbox_row(w) : tp.peer_payload[w] + sh.offset;
        exps[w] = tp.gexp + sh.b0;
    }
    sml_ok(sml_switch_aggregate_typed(planes, exps, (uint16_t)W_, sh.numel, P_, nullptr, nullptr,
                                      at(tp.out, sh.offset, type), SmlFloatType(type), kPeer, st),
           "sml_switch_aggregate", kWho);
}

// A slice of a float type (FLOAT32, or FLOAT16 / BFLOAT16 under
// backend.xgmi.half_types: the kernels convert, the out plane and the
// multicast carry 2-byte elements), chunk by chunk, pipelined on two streams (the caller's
// `st` for the local HBM work, tp.xst for the xGMI phases):
//   prologue   K2(0) | barrier | max + K3(0) | barrier
//   chunk c    K6(c) on xst  beside  K2(c+1) on st          | barrier
//              gather(c) on xst  beside  max + K3(c+1) on st | barrier
// Push form: chunk c's phase 1 also writes the own shard into every peer's
// out plane, and phase 2's gather becomes one local copy of the own out plane
// (all W shards are there after the barrier); the out plane is next written
// in chunk c + 1's phase 1, after the barrier that ends phase 2.
// Every plane's readers finish before the barrier that precedes its next
// writer: exps (peers' max of chunk c+1, phase 2) before K2(c+2) (phase 1 of
// the next chunk); payload (peers' K6(c), phase 1) before K3(c+1) (phase 2);
// out (peers' gather(c), phase 2) before K6(c+1); gexp (own K6(c)) before
// the max of chunk c+1.  So one set of planes serves the pipeline.
// Each "| barrier" is one HandOff.  What xst wrote for the peers (K6's shard)
// is released as soon as it is queued, before the next chunk's work is
// enqueued on st; the gather writes the caller's tensor, which no peer reads.
void XgmiSwitch::FloatSlice(int tid, const void* in, void* out, uint64_t numel, DataType type, hipStream_t st) {
    ThreadPlanes& tp = planes_[tid];
    const hipStream_t xst = tp.xst;
    const uint64_t nchunks = (numel + cap_ - 1) / cap_;
    auto plan = [&](uint64_t c) { return ShardPlan(std::min<uint64_t>(cap_, numel - c * cap_), P_, (uint64_t)W_); };
    auto k2 = [&](uint64_t c) {
        sml_ok(sml_exponents_typed(at(in, c * cap_, type), SmlFloatType(type), plan(c).n, P_, tp.exps, st),
               "sml_exponents", kWho);
    };
    auto k3 = [&](uint64_t c) { Quantize(tp, at(in, c * cap_, type), type, plan(c), st); };   // the max, then K3
    auto k6 = [&](uint64_t c) {
        Aggregate(tp, type, plan(c), xst);
        if (push_) PushShard(tp, type, plan(c), xst);   // the multicast, as writes into the peers' out planes
        release(xst);
    };
    auto gather = [&](uint64_t c) {
        if (!push_) return Gather(tp, at(out, c * cap_, type), type, plan(c), xst);
        // every shard is in the own out plane now: one local copy
        const void* src = tp.out;
        void* dst = at(out, c * cap_, type);
        const uint64_t n = plan(c).n;
        sml_ok(sml_copy_segments_typed(&src, &dst, &n, 1, CopyType(type), kPeer, xst), "sml_copy_segments", kWho);
    };
    k2(0);
    HandOff(tid, {{st, true}});
    k3(0);
    HandOff(tid, {{st, true}});
    for (uint64_t c = 0; c < nchunks; c++) {
        const bool next = c + 1 < nchunks;
        k6(c);
        if (next) k2(c + 1);
        HandOff(tid, {{xst, false}, {st, next}});
        gather(c);
        if (next) k3(c + 1);
        HandOff(tid, {{xst, false}, {st, next}});   // peers are done reading our planes before they are written again
    }
}

// Push form: this worker's dequantized shard (blocks [rank S, ...) of the own
// out plane) written into the same place of every peer's out plane (W − 1
// segments in one launch, over xGMI), so that after the next barrier every
// out plane holds all W shards.
void XgmiSwitch::PushShard(ThreadPlanes& tp, DataType type, const ShardPlan& plan, hipStream_t st) {
    const Shard sh = plan.shard(rank_);
    if (!sh.nb || W_ == 1) return;
    const void* srcs[kMaxW];
    void* dsts[kMaxW];
    uint64_t cnt[kMaxW];
    uint32_t k = 0;
    for (int w = 0; w < W_; w++) {
        if (w == rank_) continue;
        srcs[k] = at(tp.out, sh.offset, type);
        dsts[k] = at(const_cast<float*>(tp.peer_out[w]), sh.offset, type);
        cnt[k] = sh.numel;
        k++;
    }
    sml_ok(sml_copy_segments_typed(srcs, dsts, cnt, k, CopyType(type), 0, st), "sml_copy_segments", kWho);
}

// Worker w's shard of every plane (blocks [w S, min((w+1) S, B))) from its
// out plane into `out`, one sml_copy_segments_typed launch for the W shards
// (elements of `type`: 32-bit words, or a 16-bit slice's 2-byte elements).
void XgmiSwitch::Gather(ThreadPlanes& tp, void* out, DataType type, const ShardPlan& plan, hipStream_t st) {
    const void* srcs[kMaxW];
    void* dsts[kMaxW];
    uint64_t cnt[kMaxW];
    uint32_t k = 0;
    for (int w = 0; w < W_; w++) {
        const Shard sh = plan.shard(w);
        if (!sh.nb) continue;
        srcs[k] = at(tp.peer_out[w], sh.offset, type);
        dsts[k] = at(out, sh.offset, type);
        cnt[k] = sh.numel;
        k++;
    }
    sml_ok(sml_copy_segments_typed(srcs, dsts, cnt, k, CopyType(type), kPeer, st), "sml_copy_segments", kWho);
}

// An INT32 chunk, on the caller's stream alone:
//   copy into the own payload plane | barrier | sum of the own shard into
//   the own out plane | barrier | gather | barrier
// The sum runs over the shard's whole blocks (inside the planes: a chunk is
// at most cap_ words, a multiple of P); the gather copies the n words.  The
// last barrier keeps the planes from being rewritten (the next chunk's copy)
// while a peer still gathers from them; it hands nothing off, so no release.
void XgmiSwitch::IntChunk(int tid, const int32_t* in, int32_t* out, uint64_t n, hipStream_t st) {
    ThreadPlanes& tp = planes_[tid];
    const ShardPlan plan(n, P_, (uint64_t)W_);
    const Shard sh = plan.shard(rank_);
    sml_ok(sml_copy_words(in, tp.payload, n, st), "sml_copy_words", kWho);
    HandOff(tid, {{st, true}});
    if (sh.nb) {
        const int32_t* planes[kMaxW];
        for (int w = 0; w < W_; w++) planes[w] = tp.peer_payload[w] + sh.offset;
        int32_t* dst = reinterpret_cast<int32_t*>(tp.out) + sh.offset;
        sml_ok(sml_switch_aggregate(planes, nullptr, (uint16_t)W_, sh.words, P_, dst, nullptr, nullptr,
                                    SML_FLAG_PAYLOAD_LE | kPeer, st), "sml_switch_aggregate", kWho);
    }
    HandOff(tid, {{st, sh.nb != 0}});
    Gather(tp, out, INT32, plan, st);
    HandOff(tid, {{st, false}});
}

void XgmiSwitch::AllReduceSlice(int tid, const void* in, void* out, uint64_t numel, DataType type, hipStream_t st) {
    if (tid < 0 || tid >= T_) Fatal("bad worker thread id");
    // without backend.xgmi.half_types every worker refuses the same job here,
    // before any barrier (the CollNet plugin never posts one: its
    // reduceSupport is then 0 for these types under xgmi)
    if (IsHalfType(type) && !half_types_)
        Fatal(std::string(DataTypeName(type)) +
              " jobs are not supported with backend = xgmi; use backend = dummy (mode bulk or fused)");
    if (numel == 0) return;
    if (Wedged()) Fatal("an earlier slice's device work did not finish");
    ThrowIfPoisoned();
    try {
        if (IsFloatType(type)) {
            FloatSlice(tid, in, out, numel, type, st);
            return;
        }
        for (uint64_t off = 0; off < numel; off += cap_) {
            const uint64_t n = std::min<uint64_t>(cap_, numel - off);
            IntChunk(tid, static_cast<const int32_t*>(in) + off, static_cast<int32_t*>(out) + off, n, st);
        }
    } catch (...) {
        // this worker's arrival count is now out of phase with its peers':
        // fail the session for everyone rather than let a barrier pair
        // different phases
        Poison();
        // nothing may still touch the planes when the slice is reported
        // failed — unless a wait already timed out (wedged): then waiting
        // again would only add timeout_ms per stream
        if (!Wedged()) (void)StreamSync(st, true);
        if (!Wedged()) (void)StreamSync(planes_[tid].xst, true);
        throw;
    }
}

}  // namespace switchml
