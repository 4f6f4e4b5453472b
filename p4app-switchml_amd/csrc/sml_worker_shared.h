// sml_worker_shared.h — what the RDMA worker's completion loop does not owe
// to the message's length, shared by its two families: sml_rdma_worker_*
// (sml_rdma_worker.hip: a message is one wave's registers, up to 1024 words)
// and sml_msg_worker_* (sml_msg_worker.hip: a message is a workgroup's, up to
// 16384).  The state's layout, the record writers, the reset / judge / resend
// kernels, and on the host every argument check of the five calls, made once
// here for both (`any_msg`: the long family's msg_numel and pkts_per_msg).
// include/switchml_rdma_worker.h has the semantics.
//
// d_state: a 64-byte slice header (WkSlice), then one 32-byte record per QP
// (WkQp: two 16-byte loads).
#ifndef SML_WORKER_SHARED_H_
#define SML_WORKER_SHARED_H_

#include "sml_host.h"
#include "sml_packet_phases.h"
#include "switchml_messages.h"

namespace sml {

constexpr uint32_t kWkMaxQps = SML_MAX_FRAME_SWITCH_SLOTS;   // a QP per message slot of the switch's pool
constexpr uint64_t kWkMaxRecords = 0x7fffffffull;            // a claim word holds a record's index
constexpr uint32_t kWkNoClaim = 0xffffffffu;
constexpr uint32_t kWkCandidate = 0xffu;                     // verdict[i] between the two passes
constexpr uint32_t kWkRecordBytes = sizeof(sml_rdma_arrival);
static_assert(kWkRecordBytes == 24 && offsetof(sml_rdma_arrival, addr) == 16, "two stores: 16 bytes, then 8");
static_assert(sizeof(sml_rdma_completion) == 8, "one 8-byte load");

struct WkSlice {                    // the slice under way (all zero: none)
    uint64_t in, out, numel;
    uint64_t B, total;              // blocks; messages (B + b for the float types)
    uint32_t b, pad0;               // QPs in use = messages of a batch
    uint64_t pad1[2];
};
struct WkQp {
    uint64_t msg_id;                // the message this QP has outstanding (expects back)
    uint32_t claim;                 // lowest candidate index of the call under way, else kWkNoClaim
    uint32_t imm;                   // the outstanding message's immediate, for a resend
    int32_t exp;                    // the exponent received with the QP's previous message
    uint32_t flag;                  // the pool flag the outstanding message went out with
    uint32_t pad[2];
};
static_assert(sizeof(WkSlice) == 64 && sizeof(WkQp) == 32 && offsetof(WkQp, exp) == 16, "header, two 16-byte halves");

struct WkArgs {
    const u2* completions;          // poll
    const uint32_t* qpns;           // resend
    uint64_t n;
    const WkSlice* slice;
    WkQp* qps;
    const uint8_t* rx;
    uint8_t* tx;
    uint8_t* sends;
    uint8_t* verdict;
    unsigned long long* counts;     // [4] or nullptr
    uint32_t worker, W, Q, first_slot, src_base, ppm, msg_bytes;
    uint32_t M, wpm;                // the long family's geometry: words, waves per message
    bool flt;
};

// d_sends[i]: QP q's outstanding message, or the null record.
__device__ __forceinline__ void wk_send_record(const WkArgs& a, uint64_t i, bool live, uint32_t q, uint32_t flag,
                                               uint32_t imm) {
    uint8_t* const p = a.sends + i * kWkRecordBytes;
    const uint32_t rkey = (((a.first_slot + q) * a.ppm) << 1) | (flag & 1u);    // < 2^14 * 2^8 * 2
    const uint64_t addr = live ? (uint64_t)q * a.msg_bytes : 0;
    *reinterpret_cast<u4a*>(p) = live ? u4a{a.worker, rkey, imm, a.src_base + q} : u4a{0xffffffffu, 0u, 0u, 0u};
    *reinterpret_cast<u2*>(p + 16) = u2{(uint32_t)addr, (uint32_t)(addr >> 32)};
}

__device__ __forceinline__ void wk_store_qp(WkQp* qp, uint64_t msg_id, uint32_t imm, int exp, uint32_t flag) {
    u4* const p = reinterpret_cast<u4*>(qp);
    p[0] = mku4((uint32_t)msg_id, (uint32_t)(msg_id >> 32), kWkNoClaim, imm);
    p[1] = mku4((uint32_t)exp, flag, 0u, 0u);
}

__device__ __forceinline__ uint64_t wk_real_words(uint64_t numel, uint64_t k, uint64_t M) {
    return numel - k * M < M ? numel - k * M : M;
}

static __global__ __launch_bounds__(kBlockThreads) void k_wk_reset(WkSlice* slice, WkQp* qps, uint32_t Q) {
    const uint32_t t = blockIdx.x * kBlockThreads + threadIdx.x;
    if (t < sizeof(WkSlice) / 8) reinterpret_cast<uint64_t*>(slice)[t] = 0;
    for (uint32_t q = t; q < Q; q += gridDim.x * kBlockThreads)
        wk_store_qp(qps + q, 0, 0u, 0, 1u);                     // flipped to 0 before the first message
}

// PostSendWr(qpn, true): the outstanding message's record again.
static __global__ __launch_bounds__(kBlockThreads) void k_wk_resend(WkArgs a) {
    const uint32_t b = a.slice->b;
    const uint64_t total = a.slice->total;
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const uint32_t q = a.qpns[i];
        bool live = q < b;
        uint32_t flag = 0, imm = 0;
        if (live) {
            const WkQp* const qp = a.qps + q;
            live = qp->msg_id < total;
            flag = qp->flag;
            imm = qp->imm;
        }
        wk_send_record(a, i, live, live ? q : 0u, flag, imm);
    }
}

// Pass 1 of a poll: every completion against the state as the call found it.
static __global__ __launch_bounds__(kBlockThreads) void k_wk_judge(WkArgs a) {
    __shared__ uint32_t hist[4];
    tally_init(hist);
    const uint32_t b = a.slice->b;
    const uint64_t total = a.slice->total;
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const u2 c = a.completions[i];
        uint32_t v = SML_RDMA_WORKER_IGNORED;
        if (c.x < b) {
            WkQp* const qp = a.qps + c.x;
            const u4 lo = *reinterpret_cast<const u4*>(qp);
            const uint64_t msg_id = ((uint64_t)lo.y << 32) | lo.x;
            if (msg_id < total) {
                v = ((c.y ^ lo.x) & 0xffffu) ? (uint32_t)SML_RDMA_WORKER_WRONG : kWkCandidate;
                if (v == kWkCandidate) atomicMin(&qp->claim, (uint32_t)i);
            }
        }
        a.verdict[i] = (uint8_t)v;
        if (v == kWkCandidate) continue;
        wk_send_record(a, i, false, 0u, 0u, 0u);
        if (a.counts) tally_add(hist[v], 1u);
    }
    if (!a.counts) return;
    tally_flush(hist, a.counts);
}

// ------------------------------------------------------------ host side

struct WkLayout {
    uint64_t qps, total;
};

inline bool wk_layout(uint32_t Q, WkLayout& l) {
    if (Q == 0 || Q > kWkMaxQps) return false;
    l.qps = sizeof(WkSlice);
    l.total = l.qps + (uint64_t)sizeof(WkQp) * Q;
    return true;
}

// The checks of sml_rdma_worker_params every call shares, after its NULL
// checks.  sml_rdma_worker_* take a packet-sized message of 1, 2, 4, 8 or 16
// packets; sml_msg_worker_* (any_msg) every length the sml_msg_* entry points
// serve and 1..256 packets.
inline sml_status_t wk_check_params(bool any_msg, const sml_rdma_worker_params* p, uint64_t n) {
    const uint32_t ppm = p->pkts_per_msg;
    WkLayout l;
    if (!(any_msg ? sml_msg_numel_supported(p->msg_numel) != 0 : valid_packet(p->msg_numel)) ||
        !wk_layout(p->num_qps, l) || n > kWkMaxRecords)
        return SML_ERR_UNSUPPORTED;
    if (any_msg ? ppm == 0 || ppm > 256 : ppm != 1 && ppm != 2 && ppm != 4 && ppm != 8 && ppm != 16)
        return SML_ERR_UNSUPPORTED;
    if ((uint64_t)p->first_slot + p->num_qps > kWkMaxQps) return SML_ERR_UNSUPPORTED;
    if (p->data_type != SML_FLOAT32 && p->data_type != SML_INT32 && p->data_type != SML_FLOAT16 &&
        p->data_type != SML_BFLOAT16)
        return SML_ERR_UNSUPPORTED;
    return SML_OK;
}

inline WkArgs wk_args(const sml_rdma_worker_params* p, void* d_state, uint64_t n) {
    WkArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.slice = static_cast<const WkSlice*>(d_state);
    a.qps = reinterpret_cast<WkQp*>(static_cast<uint8_t*>(d_state) + sizeof(WkSlice));
    a.worker = p->worker;
    a.W = p->num_workers;
    a.Q = p->num_qps;
    a.first_slot = p->first_slot;
    a.src_base = p->src_base;
    a.ppm = p->pkts_per_msg;
    a.msg_bytes = 4u * p->msg_numel;
    a.M = p->msg_numel;
    a.wpm = (p->msg_numel + kTileElems - 1) / kTileElems;
    a.flt = p->data_type != SML_INT32;
    return a;
}

// The slice's element policy: INT32 and FLOAT32 are their words.
template <class F>
static void wk_dispatch_type(uint32_t data_type, F&& f) {
    if (data_type == SML_FLOAT16) f(Slice16<kHalfF16>{});
    else if (data_type == SML_BFLOAT16) f(Slice16<kHalfBF16>{});
    else f(SliceWords{});
}

// Each call of both families up to its family's own launch: every check in the
// header's order, then the arguments.  *go: the caller has work to launch.

inline sml_status_t wk_reset(void* d_state, uint32_t num_qps, void* stream) {
    if (!d_state) return SML_ERR_INVALID_ARG;
    WkLayout l;
    if (!wk_layout(num_qps, l)) return SML_ERR_UNSUPPORTED;
    if (!aligned16(d_state)) return SML_ERR_ALIGNMENT;
    uint8_t* const st8 = static_cast<uint8_t*>(d_state);
    k_wk_reset<<<grid_for_vec(num_qps), kBlockThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<WkSlice*>(st8), reinterpret_cast<WkQp*>(st8 + l.qps), num_qps);
    return launch_check();
}

inline sml_status_t wk_begin_args(bool any_msg, const sml_rdma_worker_params* prm, const void* d_in, void* d_out,
                                  uint64_t numel, void* d_state, void* tx, sml_rdma_arrival* d_sends, WkArgs* a,
                                  WkSlice* s) {
    if (!prm || prm->num_workers == 0 || !d_state || !d_sends) return SML_ERR_INVALID_ARG;
    if (numel && (!d_in || !d_out || !tx)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = wk_check_params(any_msg, prm, 0);
    if (st != SML_OK) return st;
    const bool flt = prm->data_type != SML_INT32;
    const uintptr_t esz = prm->data_type == SML_FLOAT16 || prm->data_type == SML_BFLOAT16 ? 2 : 4;
    if (!aligned16(d_state) || !aligned16(tx) || !aligned8(d_sends)) return SML_ERR_ALIGNMENT;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & (esz - 1)) return SML_ERR_ALIGNMENT;

    *a = wk_args(prm, d_state, 0);
    a->tx = static_cast<uint8_t*>(tx);
    a->sends = reinterpret_cast<uint8_t*>(d_sends);
    memset(s, 0, sizeof(*s));
    s->in = (uint64_t)(uintptr_t)d_in;
    s->out = (uint64_t)(uintptr_t)d_out;
    s->numel = numel;
    s->B = sml_num_blocks(numel, prm->msg_numel);
    s->b = (uint32_t)(s->B < prm->num_qps ? s->B : prm->num_qps);
    s->total = flt ? s->B + s->b : s->B;
    return SML_OK;
}

// On *go the judge pass is on the stream and the family's accept pass follows.
inline sml_status_t wk_poll_judge(bool any_msg, const sml_rdma_worker_params* prm,
                                  const sml_rdma_completion* d_completions, uint64_t n, void* d_state, const void* rx,
                                  void* tx, sml_rdma_arrival* d_sends, uint8_t* d_verdict, uint64_t* d_counts,
                                  void* stream, WkArgs* a, bool* go) {
    *go = false;
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (n && (!d_completions || !d_state || !rx || !tx || !d_sends || !d_verdict)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = wk_check_params(any_msg, prm, n);
    if (st != SML_OK) return st;
    if (n == 0) return SML_OK;
    const uintptr_t r0 = (uintptr_t)rx, t0 = (uintptr_t)tx, span = (uintptr_t)prm->num_qps * 4u * prm->msg_numel;
    if (r0 != t0 && r0 < t0 + span && t0 < r0 + span) return SML_ERR_INVALID_ARG;   // one buffer, or two apart
    if (!aligned16(d_state) || !aligned16(rx) || !aligned16(tx)) return SML_ERR_ALIGNMENT;
    if (!aligned8(d_completions) || !aligned8(d_sends) || !aligned8(d_counts)) return SML_ERR_ALIGNMENT;

    *a = wk_args(prm, d_state, n);
    a->completions = reinterpret_cast<const u2*>(d_completions);
    a->rx = static_cast<const uint8_t*>(rx);
    a->tx = static_cast<uint8_t*>(tx);
    a->sends = reinterpret_cast<uint8_t*>(d_sends);
    a->verdict = d_verdict;
    a->counts = reinterpret_cast<unsigned long long*>(d_counts);
    k_wk_judge<<<grid_for_vec(n), kBlockThreads, 0, (hipStream_t)stream>>>(*a);
    *go = true;
    return SML_OK;
}

inline sml_status_t wk_resend(bool any_msg, const sml_rdma_worker_params* prm, const uint32_t* d_qpns, uint64_t n,
                              void* d_state, sml_rdma_arrival* d_sends, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (n && (!d_qpns || !d_state || !d_sends)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = wk_check_params(any_msg, prm, n);
    if (st != SML_OK) return st;
    if (n == 0) return SML_OK;
    if (!aligned16(d_state) || !aligned4(d_qpns) || !aligned8(d_sends)) return SML_ERR_ALIGNMENT;
    WkArgs a = wk_args(prm, d_state, n);
    a.qpns = d_qpns;
    a.sends = reinterpret_cast<uint8_t*>(d_sends);
    k_wk_resend<<<grid_for_vec(n), kBlockThreads, 0, (hipStream_t)stream>>>(a);
    return launch_check();
}

}  // namespace sml

#endif  // SML_WORKER_SHARED_H_
