// sml_rdma_worker.hip — the RDMA worker's completion loop on gfx950 (DESIGN §9
// F4, "Worker side"): rdma_worker_thread.cc:159-294 and PostSendWr (:318-379)
// over a batch of completions per call, with what the loop keeps per queue
// pair (QP) in d_state: the expected message id, the exponent received with
// the QP's previous message, the pool flag.  What a call emits is the
// sml_rdma_arrival records sml_rdma_switch takes (include/
// switchml_rdma_worker.h has the semantics).
//
// The rule is per QP and the data is per message, so the split is the RDMA
// switch's: cheap threads decide, waves move data.
//   k_wk_judge   thread per completion, the state read-only but for the claim
//                words: IGNORED / WRONG are written (with their null record),
//                a matching record marks itself a candidate and puts its index
//                into its QP's claim word with an atomic min.
//   k_wk_accept  wave per completion.  A candidate that does not hold its QP's
//                claim is a duplicate delivery: WRONG.  The holder has message
//                m of QP q, as U = M / 256 slices of 16 bytes a lane (the
//                packet phases of sml_packet_phases.h, which the bursts use):
//                it asks for the result words (rx), the QP's record, block m
//                or m + b of the slice (the next message's payload) and block
//                m + b (the next message's exponent), waits once, and only
//                then stores: the dequantized block to the output, the next
//                message over the received one (tx may be rx, and either may
//                lie across PCIe, where a posted write may overtake a read
//                still outstanding), and from one lane the QP's record, the
//                send record and the verdict.  The exponent of block m - b is
//                the one this QP received with message m - b: no per-block
//                exponent array, O(Q) state.
//   k_wk_begin   wave per QP: PostSendWr of messages 0..b-1 (exponent of block q,
//                or the INT32 byte swap); k_wk_resend: thread per entry.
// No LDS but the verdict tallies, no scratch; asm only waits.
//
// d_state: a 64-byte slice header (WkSlice), then one 32-byte record per QP
// (WkQp: two 16-byte loads).
#include "sml_host.h"
#include "sml_packet_phases.h"

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
    uint32_t worker, W, Q, first_slot, src_base, ppm_shift, msg_bytes;
    bool flt;
};

// d_sends[i]: QP q's outstanding message, or the null record.
__device__ __forceinline__ void wk_send_record(const WkArgs& a, uint64_t i, bool live, uint32_t q, uint32_t flag,
                                               uint32_t imm) {
    uint8_t* const p = a.sends + i * kWkRecordBytes;
    const uint32_t rkey = (((a.first_slot + q) << a.ppm_shift) << 1) | (flag & 1u);
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

__global__ __launch_bounds__(kBlockThreads) void k_wk_reset(WkSlice* slice, WkQp* qps, uint32_t Q) {
    const uint32_t t = blockIdx.x * kBlockThreads + threadIdx.x;
    if (t < sizeof(WkSlice) / 8) reinterpret_cast<uint64_t*>(slice)[t] = 0;
    for (uint32_t q = t; q < Q; q += gridDim.x * kBlockThreads)
        wk_store_qp(qps + q, 0, 0u, 0, 1u);                     // flipped to 0 before the first message
}

// PostSendWr(q) for the first batch, a wave per QP.
template <class E, int M>
__global__ __launch_bounds__(kBlockThreads) void k_wk_begin(WkArgs a, WkSlice s) {
    const PacketLanes<M> g{};
    constexpr int U = PacketLanes<M>::U;
    if (blockIdx.x == 0 && threadIdx.x == 0) *const_cast<WkSlice*>(a.slice) = s;
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    for (uint32_t q = blockIdx.x * kWavesPerBlock + wave_index(); q < a.Q; q += nwaves) {
        if (q >= s.b) {
            if (g.lane == 0) wk_send_record(a, q, false, 0u, 0u, 0u);
            continue;
        }
        const uint64_t n = wk_real_words(s.numel, q, M);
        uint32_t x[U][4];
        load_words<E>(g, reinterpret_cast<const typename E::raw*>(s.in) + (uint64_t)q * M, n, x);
        uint32_t imm = q & 0xffffu;
        if (a.flt) {
            imm |= ((uint32_t)block_exponent(g, x) & 0xffu) << 16;
        } else {
            uint32_t w[U][4] = {};
            pack_block<M, false>(g, false, x, 0.0f, n, w);
            store_words(g, reinterpret_cast<uint32_t*>(a.tx + (uint64_t)q * a.msg_bytes), n, w);
        }
        if (g.lane == 0) {
            const uint32_t flag = (a.qps[q].flag ^ 1u) & 1u;
            wk_store_qp(a.qps + q, q, imm, 0, flag);
            wk_send_record(a, q, true, q, flag, imm);
        }
    }
}

// PostSendWr(qpn, true): the outstanding message's record again.
__global__ __launch_bounds__(kBlockThreads) void k_wk_resend(WkArgs a) {
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
__global__ __launch_bounds__(kBlockThreads) void k_wk_judge(WkArgs a) {
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

// Pass 2 of a poll, a wave per completion: PostprocessSingle(m), msg_id += b,
// PostSendWr for the claim's holder.
template <class E, int M, bool RNE>
__global__ __launch_bounds__(kBlockThreads) void k_wk_accept(WkArgs a) {
    typedef typename E::raw raw;
    __shared__ uint32_t hist[4];
    tally_init(hist);
    const PacketLanes<M> g{};
    constexpr int U = PacketLanes<M>::U;
    const WkSlice s = *a.slice;
    const raw* const in = reinterpret_cast<const raw*>(s.in);
    raw* const out = reinterpret_cast<raw*>(s.out);
    const bool flt = a.flt;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); i < a.n; i += nwaves) {
        if (a.verdict[i] != kWkCandidate) continue;
        const u2 c = a.completions[i];
        const uint32_t q = c.x;                                 // < b <= Q: judged
        WkQp* const qp = a.qps + q;
        const u4 lo = *reinterpret_cast<const u4*>(qp);
        if (lo.z != (uint32_t)i) {                              // a lower index holds (or held) the claim
            if (g.lane == 0) {
                a.verdict[i] = SML_RDMA_WORKER_WRONG;
                wk_send_record(a, i, false, 0u, 0u, 0u);
                if (a.counts) tally_add(hist[SML_RDMA_WORKER_WRONG], 1u);
            }
            continue;
        }
        // message m: what each half touches
        const uint64_t m = ((uint64_t)lo.y << 32) | lo.x;       // < total: judged
        const uint64_t next = m + s.b;
        const bool posts = next < s.total;                      // float types: then m < B
        const bool post_on = !flt || m >= s.b;
        const uint64_t k_post = !post_on ? 0 : flt ? m - s.b : m;
        const uint64_t n_post = post_on ? wk_real_words(s.numel, k_post, M) : 0;
        const uint64_t k_pre = flt ? m : next;
        const uint64_t n_pre = posts ? wk_real_words(s.numel, k_pre, M) : 0;
        const uint64_t n_exp = flt && next < s.B ? wk_real_words(s.numel, next, M) : 0;
        uint8_t* const txq = a.tx + (uint64_t)q * a.msg_bytes;

        // ---- every load up front, the received message's first; one wait
        uint32_t w[U][4], xq[U][4], xe[U][4];
        load_words(g, reinterpret_cast<const uint32_t*>(a.rx + (uint64_t)q * a.msg_bytes), n_post, w);
        const u4 hi = reinterpret_cast<const u4*>(qp)[1];
        load_words<E>(g, in + (n_pre ? k_pre : 0) * M, n_pre, xq);
        load_words<E>(g, in + (n_exp ? next : 0) * M, n_exp, xe);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        // ---- PostprocessSingle(m)
        const int e_kept = (int)hi.x;
        const int e_recv = (int)(int8_t)(uint8_t)(c.y >> 16);
        unpack_block<E>(g, flt, w, flt ? scale_for(a.W, e_kept) : 0.0f, n_post, out + k_post * M);

        // ---- PostSendWr of message m + b into the same buffer
        pack_block<M, RNE>(g, flt, xq, flt ? scale_for(a.W, e_recv) : 0.0f, n_pre, w);
        store_words(g, reinterpret_cast<uint32_t*>(txq), n_pre, w);
        const int e_next = n_exp ? block_exponent(g, xe) : 0;
        if (g.lane == 0) {
            const uint32_t flag = posts ? (hi.y ^ 1u) & 1u : hi.y;
            const uint32_t imm = posts ? ((uint32_t)next & 0xffffu) | (((uint32_t)e_next & 0xffu) << 16) : lo.w;
            wk_store_qp(qp, next, imm, flt && m < s.B ? e_recv : e_kept, flag);
            wk_send_record(a, i, posts, posts ? q : 0u, flag, imm);
            const uint32_t v = posts ? SML_RDMA_WORKER_POSTED : SML_RDMA_WORKER_FINISHED;
            a.verdict[i] = (uint8_t)v;
            if (a.counts) tally_add(hist[v], 1u);
        }
    }
    if (!a.counts) return;
    tally_flush(hist, a.counts);
}

struct WkLayout {
    uint64_t qps, total;
};

static bool wk_layout(uint32_t Q, WkLayout& l) {
    if (Q == 0 || Q > kWkMaxQps) return false;
    l.qps = sizeof(WkSlice);
    l.total = l.qps + (uint64_t)sizeof(WkQp) * Q;
    return true;
}

// The checks of sml_rdma_worker_params every call shares, after its NULL checks.
static sml_status_t wk_check_params(const sml_rdma_worker_params* p, uint64_t n) {
    const uint32_t ppm = p->pkts_per_msg;
    WkLayout l;
    if (!valid_packet(p->msg_numel) || !wk_layout(p->num_qps, l) || n > kWkMaxRecords) return SML_ERR_UNSUPPORTED;
    if (ppm != 1 && ppm != 2 && ppm != 4 && ppm != 8 && ppm != 16) return SML_ERR_UNSUPPORTED;
    if ((uint64_t)p->first_slot + p->num_qps > kWkMaxQps) return SML_ERR_UNSUPPORTED;
    if (p->data_type != SML_FLOAT32 && p->data_type != SML_INT32 && p->data_type != SML_FLOAT16 &&
        p->data_type != SML_BFLOAT16)
        return SML_ERR_UNSUPPORTED;
    return SML_OK;
}

static WkArgs wk_args(const sml_rdma_worker_params* p, void* d_state, uint64_t n) {
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
    a.ppm_shift = (uint32_t)__builtin_ctz(p->pkts_per_msg);
    a.msg_bytes = 4u * p->msg_numel;
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

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_rdma_worker_state_bytes(uint32_t num_qps) {
    WkLayout l;
    return wk_layout(num_qps, l) ? l.total : 0;
}

sml_status_t sml_rdma_worker_reset(void* d_state, uint32_t num_qps, void* stream) {
    if (!d_state) return SML_ERR_INVALID_ARG;
    WkLayout l;
    if (!wk_layout(num_qps, l)) return SML_ERR_UNSUPPORTED;
    if (!aligned16(d_state)) return SML_ERR_ALIGNMENT;
    uint8_t* const st8 = static_cast<uint8_t*>(d_state);
    k_wk_reset<<<grid_for_vec(num_qps), kBlockThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<WkSlice*>(st8), reinterpret_cast<WkQp*>(st8 + l.qps), num_qps);
    return launch_check();
}

sml_status_t sml_rdma_worker_begin(const sml_rdma_worker_params* prm, const void* d_in, void* d_out, uint64_t numel,
                                   void* d_state, void* tx, sml_rdma_arrival* d_sends, void* stream) {
    if (!prm || prm->num_workers == 0 || !d_state || !d_sends) return SML_ERR_INVALID_ARG;
    if (numel && (!d_in || !d_out || !tx)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = wk_check_params(prm, 0);
    if (st != SML_OK) return st;
    const bool flt = prm->data_type != SML_INT32;
    const uintptr_t esz = prm->data_type == SML_FLOAT16 || prm->data_type == SML_BFLOAT16 ? 2 : 4;
    if (!aligned16(d_state) || !aligned16(tx) || !aligned8(d_sends)) return SML_ERR_ALIGNMENT;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & (esz - 1)) return SML_ERR_ALIGNMENT;

    WkArgs a = wk_args(prm, d_state, 0);
    a.tx = static_cast<uint8_t*>(tx);
    a.sends = reinterpret_cast<uint8_t*>(d_sends);
    WkSlice s;
    memset(&s, 0, sizeof(s));
    s.in = (uint64_t)(uintptr_t)d_in;
    s.out = (uint64_t)(uintptr_t)d_out;
    s.numel = numel;
    s.B = sml_num_blocks(numel, prm->msg_numel);
    s.b = (uint32_t)(s.B < prm->num_qps ? s.B : prm->num_qps);
    s.total = flt ? s.B + s.b : s.B;
    const uint32_t grid = grid_for_tiles(prm->num_qps);
    wk_dispatch_type(prm->data_type, [&](auto Ec) {
        using E = decltype(Ec);
        dispatch_packet(prm->msg_numel,
                        [&](auto Mc) { k_wk_begin<E, Mc()><<<grid, kBlockThreads, 0, (hipStream_t)stream>>>(a, s); });
    });
    return launch_check();
}

sml_status_t sml_rdma_worker_poll(const sml_rdma_worker_params* prm, const sml_rdma_completion* d_completions,
                                  uint64_t n, void* d_state, const void* rx, void* tx, sml_rdma_arrival* d_sends,
                                  uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (n && (!d_completions || !d_state || !rx || !tx || !d_sends || !d_verdict)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = wk_check_params(prm, n);
    if (st != SML_OK) return st;
    if (n == 0) return SML_OK;
    const uintptr_t r0 = (uintptr_t)rx, t0 = (uintptr_t)tx, span = (uintptr_t)prm->num_qps * 4u * prm->msg_numel;
    if (r0 != t0 && r0 < t0 + span && t0 < r0 + span) return SML_ERR_INVALID_ARG;   // one buffer, or two apart
    if (!aligned16(d_state) || !aligned16(rx) || !aligned16(tx)) return SML_ERR_ALIGNMENT;
    if (!aligned8(d_completions) || !aligned8(d_sends) || !aligned8(d_counts)) return SML_ERR_ALIGNMENT;

    WkArgs a = wk_args(prm, d_state, n);
    a.completions = reinterpret_cast<const u2*>(d_completions);
    a.rx = static_cast<const uint8_t*>(rx);
    a.tx = static_cast<uint8_t*>(tx);
    a.sends = reinterpret_cast<uint8_t*>(d_sends);
    a.verdict = d_verdict;
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    const hipStream_t s = (hipStream_t)stream;
    k_wk_judge<<<grid_for_vec(n), kBlockThreads, 0, s>>>(a);
    const uint32_t grid = grid_for_tiles(n);
    const bool rne = a.flt && (prm->flags & SML_FLAG_ROUND_RNE) != 0;    // INT32 does not round
    wk_dispatch_type(prm->data_type, [&](auto Ec) {
        using E = decltype(Ec);
        dispatch_packet(prm->msg_numel, [&](auto Mc) {
            dispatch_bools([&](auto RNE) { k_wk_accept<E, Mc(), RNE()><<<grid, kBlockThreads, 0, s>>>(a); }, rne);
        });
    });
    return launch_check();
}

sml_status_t sml_rdma_worker_resend(const sml_rdma_worker_params* prm, const uint32_t* d_qpns, uint64_t n,
                                    void* d_state, sml_rdma_arrival* d_sends, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (n && (!d_qpns || !d_state || !d_sends)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = wk_check_params(prm, n);
    if (st != SML_OK) return st;
    if (n == 0) return SML_OK;
    if (!aligned16(d_state) || !aligned4(d_qpns) || !aligned8(d_sends)) return SML_ERR_ALIGNMENT;
    WkArgs a = wk_args(prm, d_state, n);
    a.qpns = d_qpns;
    a.sends = reinterpret_cast<uint8_t*>(d_sends);
    k_wk_resend<<<grid_for_vec(n), kBlockThreads, 0, (hipStream_t)stream>>>(a);
    return launch_check();
}

}  // extern "C"
