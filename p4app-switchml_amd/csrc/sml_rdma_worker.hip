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
// The state's layout, the record writers, the judge / resend / reset kernels and
// the host's argument checks are sml_worker_shared.h's, which the long
// messages' family (sml_msg_worker.hip) shares.
#include "sml_worker_shared.h"

namespace sml {

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

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_rdma_worker_state_bytes(uint32_t num_qps) {
    WkLayout l;
    return wk_layout(num_qps, l) ? l.total : 0;
}

sml_status_t sml_rdma_worker_reset(void* d_state, uint32_t num_qps, void* stream) {
    return wk_reset(d_state, num_qps, stream);
}

sml_status_t sml_rdma_worker_begin(const sml_rdma_worker_params* prm, const void* d_in, void* d_out, uint64_t numel,
                                   void* d_state, void* tx, sml_rdma_arrival* d_sends, void* stream) {
    WkArgs a;
    WkSlice s;
    const sml_status_t st = wk_begin_args(false, prm, d_in, d_out, numel, d_state, tx, d_sends, &a, &s);
    if (st != SML_OK) return st;
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
    WkArgs a;
    bool go;
    const sml_status_t st = wk_poll_judge(false, prm, d_completions, n, d_state, rx, tx, d_sends, d_verdict, d_counts,
                                          stream, &a, &go);
    if (!go) return st;
    const hipStream_t s = (hipStream_t)stream;
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
    return wk_resend(false, prm, d_qpns, n, d_state, d_sends, stream);
}

}  // extern "C"
