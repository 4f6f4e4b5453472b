// sml_msg_worker.hip — the RDMA worker's completion loop for LONG messages on
// gfx950 (include/switchml_msg_worker.h, DESIGN §9 F4 "Worker side", "Long
// messages"): sml_rdma_worker_*'s five calls for every msg_numel the sml_msg_*
// entry points serve (a multiple of 64 up to 16384 words) and 1..256 packets a
// message.  The rule, the state, the records and the argument checks are
// sml_worker_shared.h's, with the judge / resend / reset kernels; what is new
// here is the data movement, because sml_rdma_worker.hip's accept rests on "a
// message is one wave's registers" and a 16384-word message is 16 waves' worth
// for each of its three streams.
//
// Geometry: sml_msg_deal.h's.  A message occupies wpm = ceil(M / 1024) waves
// of ONE workgroup; slice s (256 words, the last masked to 64 / 128 / 192) goes
// to wave s % wpm, at most 4 a wave.  The result words (rx), the next message
// (tx), the slice's blocks and the output are all dealt the same way: a wave
// stores to tx only at the offsets whose rx words it loaded itself, and only
// after its single wait, so tx == rx and buffers across PCIe (where a posted
// write may overtake a read still outstanding) need no barrier of their own.
//   k_mw_accept  workgroup of wpm waves per completion.  Every wave reads the
//                verdict, the completion and the QP's record; a candidate that
//                does not hold the claim is WRONG and the whole workgroup
//                leaves (the decision is uniform: a stale read sees WRONG or
//                no claim, and leaves too).  The holder's waves ask for their
//                slices of the result, of block m (or m + b) and of block
//                m + b, wait once, dequantize to the output, quantize into tx
//                under the received exponent, and reduce block m + b with the
//                DPP reduce.  The maximum crosses waves through one LDS word a
//                wave and ONE barrier, as in sml_messages.hip.  That barrier
//                also orders the state: every wave has read verdict[i] and the
//                QP's record before it, and only after it does wave 0's lane 0
//                write the record (which clears the claim), the send record
//                and the verdict.  The LDS words are double-buffered by trip.
//                A message of one wave (M <= 1024) needs neither the LDS step
//                nor the barrier, and four such share a workgroup.
//   k_mw_begin   workgroup of wpm waves per QP: block q's exponent across the
//                waves (the same LDS step), or the INT32 byte swap.
// One code object serves every M (wpm, M are launch arguments); the bound is
// the 1024-thread workgroup's 128 VGPRs.  Static LDS only; no scratch.
#include "sml_msg_deal.h"
#include "sml_worker_shared.h"
#include "switchml_msg_worker.h"

namespace sml {

constexpr int kMwThreads = kMsgMaxWaves * kWave;

// This lane's slices of a message: slice u of wave `part` starts at word j(u).
// Every phase touches words j + t < n only, and n <= M, so slices past the
// message's end drop out of every phase without a test of their own.
struct MsgLanes {
    uint32_t wpm, part;
    int lane;
    __device__ __forceinline__ uint64_t j(int u) const { return msg_offset(wpm, u, part, lane); }
};

template <class E = SliceWords>
__device__ __forceinline__ void mw_load(MsgLanes g, const typename E::raw* buf, uint64_t n, uint32_t (&w)[kMsgU][4]) {
#pragma unroll
    for (int u = 0; u < kMsgU; u++) E::load_group(buf, g.j(u), n, w[u]);
}

__device__ __forceinline__ void mw_store(MsgLanes g, uint32_t* buf, uint64_t n, const uint32_t (&w)[kMsgU][4]) {
#pragma unroll
    for (int u = 0; u < kMsgU; u++) store_group(buf, g.j(u), n, w[u]);
}

// This wave's maximum of |x| over its slices, wave-uniform.
__device__ __forceinline__ uint32_t mw_wave_max(const uint32_t (&x)[kMsgU][4]) {
    uint32_t m = 0;
#pragma unroll
    for (int u = 0; u < kMsgU; u++) m = umax(m, max4(as_f4(x[u])));
    return group_max<256>(m);
}

// The workgroup's maximum from its waves': one LDS word per wave, the barrier,
// then every 16-lane row reads the wpm <= 16 words (sml_messages.hip's step).
// smax: this trip's words.  Every wave of the workgroup arrives here.  A
// one-wave message has its maximum already and shares no state with another
// wave: no LDS step and no barrier (its workgroup holds other messages' waves).
__device__ __forceinline__ uint32_t mw_cross_max(MsgLanes g, uint32_t m, uint32_t* smax) {
    if (g.wpm == 1) return m;
    if (g.lane == 0) smax[g.part] = m;
    __syncthreads();
    const uint32_t l = (uint32_t)g.lane & 15u;
    m = group_max<64>(smax[l < g.wpm ? l : g.wpm - 1]);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}

// Which messages a workgroup takes.  wpm > 1: its waves are one message's, and
// it strides over messages by the grid.  wpm == 1: kWavesPerBlock messages a
// workgroup, a wave each (one-wave workgroups start too slowly to stream).
struct MsgTurn {
    uint64_t first, stride;
    bool leader;                    // the lane that writes the message's records
};

__device__ __forceinline__ MsgTurn mw_turn(uint32_t wpm, MsgLanes& g) {
    if (wpm > 1) return MsgTurn{blockIdx.x, gridDim.x, threadIdx.x == 0};
    const uint32_t wave = g.part;
    g.part = 0;
    return MsgTurn{(uint64_t)blockIdx.x * kWavesPerBlock + wave, (uint64_t)gridDim.x * kWavesPerBlock, g.lane == 0};
}

// pack_block / unpack_block of sml_packet_phases.h on a message's lanes: the
// same arithmetic word for word (the packet family's bits at a packet-sized M).
template <bool RNE>
__device__ __forceinline__ void mw_pack(MsgLanes g, bool flt, const uint32_t (&x)[kMsgU][4], float s, uint64_t n,
                                        uint32_t (&w)[kMsgU][4]) {
    const uint64_t body = n / 16 * 16;
#pragma unroll
    for (int u = 0; u < kMsgU; u++) {
        const uint64_t j = g.j(u);
        const u4 v = flt ? quantize4<RNE>(as_f4(x[u]), s, j, body) : mku4(x[u][0], x[u][1], x[u][2], x[u][3]);
        const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (j + t < n) w[u][t] = bswap(vv[t]);
    }
}

template <class E>
__device__ __forceinline__ void mw_unpack(MsgLanes g, bool flt, const uint32_t (&w)[kMsgU][4], float s, uint64_t n,
                                          typename E::raw* out) {
#pragma unroll
    for (int u = 0; u < kMsgU; u++) {
        uint32_t v[4];
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = flt ? __float_as_uint(dequantize1(bswap(w[u][t]), s)) : bswap(w[u][t]);
        E::store_group(out, g.j(u), n, v);
    }
}

// PostSendWr(q) for the first batch, a workgroup of wpm waves per QP.
template <class E>
__global__ __launch_bounds__(kMwThreads) void k_mw_begin(WkArgs a, WkSlice s) {
    __shared__ uint32_t smax[2][kMsgMaxWaves];
    MsgLanes g{a.wpm, wave_index(), (int)(threadIdx.x & (kWave - 1))};
    const MsgTurn turn = mw_turn(a.wpm, g);
    const uint64_t M = a.M;
    if (blockIdx.x == 0 && threadIdx.x == 0) *const_cast<WkSlice*>(a.slice) = s;
    uint32_t trip = 0;
    for (uint64_t q = turn.first; q < a.Q; q += turn.stride) {
        if (q >= s.b) {
            if (turn.leader) wk_send_record(a, q, false, 0u, 0u, 0u);
            continue;
        }
        const uint64_t n = wk_real_words(s.numel, q, M);
        uint32_t x[kMsgU][4];
        mw_load<E>(g, reinterpret_cast<const typename E::raw*>(s.in) + (uint64_t)q * M, n, x);
        uint32_t imm = (uint32_t)q & 0xffffu;
        if (a.flt) {                                            // uniform across the workgroup
            const uint32_t m = mw_cross_max(g, mw_wave_max(x), smax[trip]);
            trip ^= 1u;
            imm |= ((uint32_t)exponent_of(m) & 0xffu) << 16;
        } else {
            uint32_t w[kMsgU][4] = {};
            mw_pack<false>(g, false, x, 0.0f, n, w);
            mw_store(g, reinterpret_cast<uint32_t*>(a.tx + (uint64_t)q * a.msg_bytes), n, w);
        }
        if (turn.leader) {
            const uint32_t flag = (a.qps[q].flag ^ 1u) & 1u;
            wk_store_qp(a.qps + q, q, imm, 0, flag);
            wk_send_record(a, q, true, (uint32_t)q, flag, imm);
        }
    }
}

// Pass 2 of a poll, a workgroup of wpm waves per completion: PostprocessSingle(m),
// msg_id += b, PostSendWr for the claim's holder.
template <class E, bool RNE>
__global__ __launch_bounds__(kMwThreads) void k_mw_accept(WkArgs a) {
    typedef typename E::raw raw;
    __shared__ uint32_t hist[4];
    __shared__ uint32_t smax[2][kMsgMaxWaves];
    tally_init(hist);
    MsgLanes g{a.wpm, wave_index(), (int)(threadIdx.x & (kWave - 1))};
    const MsgTurn turn = mw_turn(a.wpm, g);
    const uint64_t M = a.M;
    const WkSlice s = *a.slice;
    const raw* const in = reinterpret_cast<const raw*>(s.in);
    raw* const out = reinterpret_cast<raw*>(s.out);
    const bool flt = a.flt;
    uint32_t trip = 0;
    for (uint64_t i = turn.first; i < a.n; i += turn.stride) {
        // Every wave reads the verdict and the QP's record for itself; wave 0
        // changes them only behind the barrier below, which every wave of a
        // holder reaches after these reads.
        if (a.verdict[i] != kWkCandidate) continue;
        const u2 c = a.completions[i];
        const uint32_t q = c.x;                                 // < b <= Q: judged
        WkQp* const qp = a.qps + q;
        const u4 lo = *reinterpret_cast<const u4*>(qp);
        if (lo.z != (uint32_t)i) {                              // a lower index holds (or held) the claim
            if (turn.leader) {
                a.verdict[i] = SML_RDMA_WORKER_WRONG;
                wk_send_record(a, i, false, 0u, 0u, 0u);
                if (a.counts) tally_add(hist[SML_RDMA_WORKER_WRONG], 1u);
            }
            continue;
        }
        // message m: what each half touches (uniform across the workgroup)
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

        // ---- this wave's slices of every stream up front, the received message's first; one wait
        uint32_t w[kMsgU][4], xq[kMsgU][4], xe[kMsgU][4];
        mw_load(g, reinterpret_cast<const uint32_t*>(a.rx + (uint64_t)q * a.msg_bytes), n_post, w);
        const u4 hi = reinterpret_cast<const u4*>(qp)[1];
        mw_load<E>(g, in + (n_pre ? k_pre : 0) * M, n_pre, xq);
        mw_load<E>(g, in + (n_exp ? next : 0) * M, n_exp, xe);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        // ---- PostprocessSingle(m)
        const int e_kept = (int)hi.x;
        const int e_recv = (int)(int8_t)(uint8_t)(c.y >> 16);
        mw_unpack<E>(g, flt, w, flt ? scale_for(a.W, e_kept) : 0.0f, n_post, out + k_post * M);

        // ---- PostSendWr of message m + b into the same buffer, dealt as rx was
        mw_pack<RNE>(g, flt, xq, flt ? scale_for(a.W, e_recv) : 0.0f, n_pre, w);
        mw_store(g, reinterpret_cast<uint32_t*>(txq), n_pre, w);

        // ---- block m + b's maximum across the waves; the barrier every wave of a
        // holder takes (n_exp == 0 too: its slices are zeros), behind which the state moves
        const uint32_t mx = mw_cross_max(g, mw_wave_max(xe), smax[trip]);
        trip ^= 1u;
        if (turn.leader) {
            const int e_next = n_exp ? exponent_of(mx) : 0;
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

// A workgroup per message (kWavesPerBlock one-wave messages), up to the grid limit.
static uint32_t mw_threads(uint32_t wpm) { return (wpm == 1 ? kWavesPerBlock : wpm) * kWave; }

static uint32_t mw_grid(uint64_t nmsgs, uint32_t wpm) {
    uint64_t g = wpm == 1 ? (nmsgs + kWavesPerBlock - 1) / kWavesPerBlock : nmsgs;
    if (g == 0) g = 1;
    const uint32_t lim = g_grid_limit.load(std::memory_order_relaxed);
    if (lim && g > lim) g = lim;
    if (g > 0x7fffffffull) g = 0x7fffffffull;
    return (uint32_t)g;
}

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_msg_worker_state_bytes(uint32_t num_qps) {
    WkLayout l;
    return wk_layout(num_qps, l) ? l.total : 0;
}

sml_status_t sml_msg_worker_reset(void* d_state, uint32_t num_qps, void* stream) {
    return wk_reset(d_state, num_qps, stream);
}

sml_status_t sml_msg_worker_begin(const sml_rdma_worker_params* prm, const void* d_in, void* d_out, uint64_t numel,
                                  void* d_state, void* tx, sml_rdma_arrival* d_sends, void* stream) {
    WkArgs a;
    WkSlice s;
    const sml_status_t st = wk_begin_args(true, prm, d_in, d_out, numel, d_state, tx, d_sends, &a, &s);
    if (st != SML_OK) return st;
    wk_dispatch_type(prm->data_type, [&](auto Ec) {
        k_mw_begin<decltype(Ec)><<<mw_grid(prm->num_qps, a.wpm), mw_threads(a.wpm), 0, (hipStream_t)stream>>>(a, s);
    });
    return launch_check();
}

sml_status_t sml_msg_worker_poll(const sml_rdma_worker_params* prm, const sml_rdma_completion* d_completions,
                                 uint64_t n, void* d_state, const void* rx, void* tx, sml_rdma_arrival* d_sends,
                                 uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    WkArgs a;
    bool go;
    const sml_status_t st = wk_poll_judge(true, prm, d_completions, n, d_state, rx, tx, d_sends, d_verdict, d_counts,
                                          stream, &a, &go);
    if (!go) return st;
    const bool rne = a.flt && (prm->flags & SML_FLAG_ROUND_RNE) != 0;    // INT32 does not round
    wk_dispatch_type(prm->data_type, [&](auto Ec) {
        dispatch_bools([&](auto RNE) {
            k_mw_accept<decltype(Ec), RNE()><<<mw_grid(n, a.wpm), mw_threads(a.wpm), 0, (hipStream_t)stream>>>(a);
        }, rne);
    });
    return launch_check();
}

sml_status_t sml_msg_worker_resend(const sml_rdma_worker_params* prm, const uint32_t* d_qpns, uint64_t n,
                                   void* d_state, sml_rdma_arrival* d_sends, void* stream) {
    return wk_resend(true, prm, d_qpns, n, d_state, d_sends, stream);
}

}  // extern "C"
