// sml_frame_worker.hip — the DPDK worker's receive loop on gfx950 (DESIGN §9
// F3, "Worker side"): dpdk_worker_thread.cc:274-389 with ReusePacket and
// ResendPacketCallback over a batch of received frames per call, with what
// the loop keeps per outstanding packet in d_state: the pkt_id a tx slot
// expects back and the exponent received with the slot's previous frame
// (include/switchml_frame_worker.h has the semantics).  The wire format is
// sml_frame_wire.h's; the phases of a packet are sml_packet_phases.h's.
//
// The rule is per slot and the data is per frame, so the split is the RDMA
// worker's — cheap threads decide, lane groups move data — but a DPDK packet
// is small, and a wave per frame would leave 48 lanes idle at P = 64.  A frame
// is held by a group of G = P / 4 lanes, each with 16 bytes of the payload:
// 4 frames per wave at P = 64 (a group is one 16-lane DPP row), 2 at P = 128,
// the whole wave from P = 256 on, with U = P / 256 slices a lane.  The phases
// take the lane's index in its group as PacketLanes' lane, so they are the
// bursts' code; the block exponent is group_max<P> (the row reduce, and for
// P >= 128 the rows through SGPRs).
//   k_fw_judge   thread per frame, the state read-only but for the claim
//                words: header dwords 10-12 (job, pkt_id, pool and exponent)
//                are all it reads of a frame; IGNORED / WRONG are written with
//                their NONE entry, a frame that carries the id its slot
//                expects marks itself a candidate and puts its index into the
//                slot's claim word with an atomic min.
//   k_fw_accept  group per frame.  A candidate that does not hold its slot's
//                claim is a later copy: WRONG.  The holder has packet p of
//                slot j: it asks for the payload (16-byte chunks at the
//                header's odd 4-byte offset), block p of the slice (the next
//                frame's payload; INT32: block p + b) and block p + b (the
//                next frame's exponent), waits once, and only then stores:
//                the dequantized block to the output, frame p + b into tx slot
//                j — payload by the frame kernels' store policy, the 13 header
//                dwords from the group's first 13 lanes (52 lanes for 4
//                frames) — and from one lane the slot's record, d_sends[i] and
//                the verdict.  The body is one wave-uniform path: a group that
//                has nothing to do loads and stores through empty masks, so
//                the cross-lane reduce never sits under a divergent branch.
//   k_fw_begin   group per slot with the same packing: frames 0..b-1;
//   k_fw_resend, k_fw_reset: thread per entry.
// No LDS but the verdict tallies, no scratch; asm only waits.
//
// d_state: a 64-byte slice header (FwSlice), then one 16-byte record per slot
// (FwSlot: one 16-byte load).
#include "sml_frame_wire.h"
#include "sml_packet_phases.h"

namespace sml {

constexpr uint32_t kFwMaxSlots = SML_MAX_FRAME_SWITCH_SLOTS;   // a tx slot per slot of the switch's pool
constexpr uint64_t kFwMaxFrames = 0x7fffffffull;               // a claim word holds a frame's index
constexpr uint64_t kFwMaxPktIds = 0xffffffffull;               // pkt_id is 32 bits on the wire
constexpr uint32_t kFwNoClaim = 0xffffffffu;
constexpr uint32_t kFwCandidate = 0xffu;                       // verdict[i] between the two passes
constexpr uint64_t kFwNone = SML_FRAME_WORKER_NONE;

struct FwSlice {                    // the slice under way (all zero: none)
    uint64_t in, out, numel;
    uint64_t B, total;              // blocks; frames (B + b for the float types)
    uint32_t b, pad0;               // tx slots in use = frames of a batch
    uint64_t pad1[2];
};
struct FwSlot {
    uint32_t expected_lo, expected_hi;   // the pkt_id this slot has outstanding (expects back); >= total: finished
    uint32_t claim;                      // lowest candidate index of the call under way, else kFwNoClaim
    int32_t exp;                         // the exponent received with the slot's previous frame
};
static_assert(sizeof(FwSlice) == 64 && sizeof(FwSlot) == 16 && offsetof(FwSlot, claim) == 8, "header, one 16-byte load");

struct FwArgs {
    const uint8_t* rx;              // poll
    uint64_t rx_stride;
    const unsigned long long* live; // poll: the ring's live count, or nullptr
    const uint32_t* slots_in;       // resend
    uint64_t n;
    const FwSlice* slice;
    FwSlot* slots;
    uint8_t* tx;
    uint64_t tx_stride;
    unsigned long long* sends;
    uint8_t* verdict;
    unsigned long long* counts;     // [4] or nullptr
    uint32_t W, Q, job, pool_start, pool_shift;
    bool flt, nts;                  // a float type; tx payloads take non-temporal stores
    uint32_t hdr[wire::kConstDwords];   // wire::worker_header
};

// How a wave holds frames of P words: groups of G lanes, F frames a wave.
template <int P>
struct FwGroups {
    static constexpr int G = P / 4 < kWave ? P / 4 : kWave;
    static constexpr int F = kWave / G;
    static constexpr int kReduce = P < 256 ? P : 256;   // group_max's width: the group, a wave at most
    static_assert(G >= wire::kHeaderDwords, "a group's first lanes store its frame's header");
};

__device__ __forceinline__ uint64_t fw_expected(u4 rec) { return ((uint64_t)rec.y << 32) | rec.x; }

__device__ __forceinline__ void fw_store_slot(FwSlot* s, uint64_t expected, int exp) {
    *reinterpret_cast<u4*>(s) = mku4((uint32_t)expected, (uint32_t)(expected >> 32), kFwNoClaim, (uint32_t)exp);
}

__device__ __forceinline__ uint64_t fw_real_words(uint64_t numel, uint64_t k, uint64_t P) {
    return numel - k * P < P ? numel - k * P : P;
}

// Header dwords 10-12 of received frame i: one 12-byte load.
typedef uint32_t fw_u3a __attribute__((ext_vector_type(3), aligned(4)));
__device__ __forceinline__ fw_u3a fw_rx_header(const FwArgs& a, uint64_t i) {
    return *reinterpret_cast<const fw_u3a*>(a.rx + i * a.rx_stride + 4 * wire::kDwJob);
}

// Dword `d` of frame p's header as BuildPacket and PreprocessSingle leave it.
__device__ __forceinline__ uint32_t fw_header_dword(const FwArgs& a, int d, uint64_t p, uint32_t exp_byte) {
    uint32_t dw = a.hdr[0];
#pragma unroll
    for (int i = 1; i < wire::kConstDwords; i++) dw = d == i ? a.hdr[i] : dw;
    if (d == wire::kDwPktId) dw = (uint32_t)p;
    if (d == wire::kDwPool)
        dw = wire::pool_dword_at(a.pool_start, a.Q, (uint32_t)((p + a.pool_shift) % (2ull * a.Q)), exp_byte);
    return dw;
}

// Frame p into tx slot j from the group that holds its payload words w (all P
// of them: a partial block's tail is zero): payload chunks, then the header
// from lanes 0..12.  `on`: the group writes at all.
template <int P, int U>
__device__ __forceinline__ void fw_store_frame(const FwArgs& a, PacketLanes<P> g, bool on, uint32_t j, uint64_t p,
                                               uint32_t exp_byte, const uint32_t (&w)[U][4]) {
    if (!on) return;
    uint8_t* const f = a.tx + (uint64_t)j * a.tx_stride;
#pragma unroll
    for (int u = 0; u < U; u++) {
        u4a* const dst = reinterpret_cast<u4a*>(f + wire::kHeaderBytes + 4 * g.j(u));
        const u4a v{w[u][0], w[u][1], w[u][2], w[u][3]};
        if (a.nts) SML_NT_STORE16_UNALIGNED(v, dst);
        else *dst = v;
    }
    if (g.lane < wire::kHeaderDwords) reinterpret_cast<uint32_t*>(f)[g.lane] = fw_header_dword(a, g.lane, p, exp_byte);
}

// The exponent of the block in x (0 past its real words), the same value in
// every lane of the group.
template <int P, int U>
__device__ __forceinline__ int fw_block_exponent(const uint32_t (&x)[U][4]) {
    uint32_t m = 0;
#pragma unroll
    for (int u = 0; u < U; u++) m = umax(m, max4(as_f4(x[u])));
    return exponent_of(group_max<FwGroups<P>::kReduce>(m));
}

__global__ __launch_bounds__(kBlockThreads) void k_fw_reset(FwSlice* slice, FwSlot* slots, uint32_t Q) {
    const uint32_t t = blockIdx.x * kBlockThreads + threadIdx.x;
    if (t < sizeof(FwSlice) / 8) reinterpret_cast<uint64_t*>(slice)[t] = 0;
    for (uint32_t q = t; q < Q; q += gridDim.x * kBlockThreads) fw_store_slot(slots + q, ~0ull, 0);
}

// Frames 0..b-1 into tx slots 0..b-1, a group per slot.
template <class E, int P>
__global__ __launch_bounds__(kBlockThreads) void k_fw_begin(FwArgs a, FwSlice s) {
    typedef FwGroups<P> L;
    constexpr int U = PacketLanes<P>::U;
    const int lane = threadIdx.x & (kWave - 1);
    const PacketLanes<P> g{lane % L::G};
    if (blockIdx.x == 0 && threadIdx.x == 0) *const_cast<FwSlice*>(a.slice) = s;
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    const uint32_t ntiles = (a.Q + L::F - 1) / L::F;
    for (uint32_t t = blockIdx.x * kWavesPerBlock + wave_index(); t < ntiles; t += nwaves) {
        const uint32_t q = t * L::F + lane / L::G;
        const bool live = q < s.b;
        const uint64_t n = live ? fw_real_words(s.numel, q, P) : 0;
        uint32_t x[U][4], w[U][4] = {};
        load_words<E>(g, reinterpret_cast<const typename E::raw*>(s.in) + (uint64_t)(live ? q : 0) * P, n, x);
        const int e = fw_block_exponent<P>(x);                 // INT32: not used
        if (!a.flt) pack_block<P, false>(g, false, x, 0.0f, n, w);
        fw_store_frame(a, g, live, q, q, a.flt ? (uint32_t)e : 0u, w);
        if (g.lane == 0 && q < a.Q) {
            fw_store_slot(a.slots + q, live ? q : ~0ull, 0);
            a.sends[q] = live ? q : kFwNone;
        }
    }
}

// ResendPacketCallback: the slot again where its frame is outstanding.
__global__ __launch_bounds__(kBlockThreads) void k_fw_resend(FwArgs a) {
    const uint32_t b = a.slice->b;
    const uint64_t total = a.slice->total;
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const uint32_t q = a.slots_in[i];
        const bool live = q < b && fw_expected(*reinterpret_cast<const u4*>(a.slots + q)) < total;
        a.sends[i] = live ? q : kFwNone;
    }
}

// Pass 1 of a poll: every frame against the state as the call found it.
__global__ __launch_bounds__(kBlockThreads) void k_fw_judge(FwArgs a) {
    __shared__ uint32_t hist[4];
    tally_init(hist);
    const uint32_t b = a.slice->b;
    const uint64_t total = a.slice->total;
    uint64_t live = a.live ? *a.live : a.n;
    if (b == 0) live = 0;                                       // no slice under way
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        uint32_t v = SML_FRAME_WORKER_IGNORED;
        if (i < live) {
            const fw_u3a h = fw_rx_header(a, i);
            const uint32_t pid = wire::pkt_id(h.y);
            v = SML_FRAME_WORKER_WRONG;
            if (wire::job(h.x) == a.job && pid < total) {
                FwSlot* const slot = a.slots + pid % b;
                if (fw_expected(*reinterpret_cast<const u4*>(slot)) == pid) {
                    v = kFwCandidate;
                    atomicMin(&slot->claim, (uint32_t)i);
                }
            }
        }
        a.verdict[i] = (uint8_t)v;
        if (v == kFwCandidate) continue;
        a.sends[i] = kFwNone;
        if (a.counts) tally_add(hist[v], 1u);
    }
    if (!a.counts) return;
    tally_flush(hist, a.counts);
}

// Pass 2 of a poll, a group per frame: PostprocessSingle(p), expected += b,
// ReusePacket for the claim's holder.
template <class E, int P, bool RNE>
__global__ __launch_bounds__(kBlockThreads) void k_fw_accept(FwArgs a) {
    typedef typename E::raw raw;
    typedef FwGroups<P> L;
    constexpr int U = PacketLanes<P>::U;
    __shared__ uint32_t hist[4];
    tally_init(hist);
    const int lane = threadIdx.x & (kWave - 1);
    const PacketLanes<P> g{lane % L::G};
    const FwSlice s = *a.slice;
    const raw* const in = reinterpret_cast<const raw*>(s.in);
    raw* const out = reinterpret_cast<raw*>(s.out);
    const bool flt = a.flt;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t ntiles = (a.n + L::F - 1) / L::F;
    for (uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); t < ntiles; t += nwaves) {
        const uint64_t i = t * L::F + lane / L::G;
        const bool cand = i < a.n && a.verdict[i] == kFwCandidate;
        // the frame's id and exponent, its slot's record: who holds the claim
        fw_u3a h = {0u, 0u, 0u};
        if (cand) h = fw_rx_header(a, i);
        const uint64_t p = wire::pkt_id(h.y);                   // < total: judged
        const uint32_t j = cand ? (uint32_t)p % s.b : 0u;       // a candidate: b > 0
        u4 rec = mku4(0u, 0u, kFwNoClaim, 0u);
        if (cand) rec = *reinterpret_cast<const u4*>(a.slots + j);
        const bool hold = cand && rec.z == (uint32_t)i;         // else a lower index holds (or held) the claim
        // packet p: what each half touches
        const uint64_t next = p + s.b;
        const bool posts = hold && next < s.total;              // float types: then p < B
        const bool post_on = hold && (!flt || p >= s.b);
        const uint64_t k_post = !post_on ? 0 : flt ? p - s.b : p;
        const uint64_t n_post = post_on ? fw_real_words(s.numel, k_post, P) : 0;
        const uint64_t k_pre = flt ? p : next;
        const uint64_t n_pre = posts ? fw_real_words(s.numel, k_pre, P) : 0;
        const uint64_t n_exp = posts && flt && next < s.B ? fw_real_words(s.numel, next, P) : 0;

        // ---- every load up front, the received payload's first; one wait
        uint32_t w[U][4], xq[U][4], xe[U][4];
        load_words(g, reinterpret_cast<const uint32_t*>(a.rx + (hold ? i : 0) * a.rx_stride + wire::kHeaderBytes),
                   n_post, w);
        load_words<E>(g, in + (n_pre ? k_pre : 0) * P, n_pre, xq);
        load_words<E>(g, in + (n_exp ? next : 0) * P, n_exp, xe);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

        // ---- PostprocessSingle(p)
        const int e_kept = (int)rec.w;
        const int e_recv = (int)(int8_t)(uint8_t)wire::exp_byte(h.z);
        unpack_block<E>(g, flt, w, flt ? scale_for(a.W, e_kept) : 0.0f, n_post, out + k_post * P);

        // ---- ReusePacket: frame p + b into the slot
        uint32_t f[U][4] = {};                                  // a partial block's tail words are 0
        pack_block<P, RNE>(g, flt, xq, flt ? scale_for(a.W, e_recv) : 0.0f, n_pre, f);
        const int e_block = fw_block_exponent<P>(xe);           // every lane takes part in the reduce
        const int e_next = n_exp ? e_block : 0;                 // 0 when p + b >= B (and for INT32)
        fw_store_frame(a, g, posts, j, next, (uint32_t)e_next, f);
        if (g.lane == 0 && cand) {
            uint32_t v = SML_FRAME_WORKER_WRONG;
            if (hold) {
                fw_store_slot(a.slots + j, next, flt && p < s.B ? e_recv : e_kept);
                v = posts ? SML_FRAME_WORKER_POSTED : SML_FRAME_WORKER_FINISHED;
            }
            a.sends[i] = posts ? (unsigned long long)j : kFwNone;
            a.verdict[i] = (uint8_t)v;
            if (a.counts) tally_add(hist[v], 1u);
        }
    }
    if (!a.counts) return;
    tally_flush(hist, a.counts);
}

struct FwLayout {
    uint64_t slots, total;
};

static bool fw_layout(uint32_t Q, FwLayout& l) {
    if (Q == 0 || Q > kFwMaxSlots) return false;
    l.slots = sizeof(FwSlice);
    l.total = l.slots + (uint64_t)sizeof(FwSlot) * Q;
    return true;
}

// The checks of sml_frame_worker_params every call shares, after its NULL checks.
static sml_status_t fw_check_params(const sml_frame_worker_params* p, uint64_t n) {
    FwLayout l;
    if (!valid_packet(p->packet_numel) || !fw_layout(p->frame.max_outstanding_pkts, l) || n > kFwMaxFrames)
        return SML_ERR_UNSUPPORTED;
    if ((uint64_t)p->frame.pool_index_start + p->frame.max_outstanding_pkts > kFwMaxSlots) return SML_ERR_UNSUPPORTED;
    if (p->data_type != SML_FLOAT32 && p->data_type != SML_INT32 && p->data_type != SML_FLOAT16 &&
        p->data_type != SML_BFLOAT16)
        return SML_ERR_UNSUPPORTED;
    return SML_OK;
}

static FwArgs fw_args(const sml_frame_worker_params* p, void* d_state, uint64_t n) {
    FwArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.slice = static_cast<const FwSlice*>(d_state);
    a.slots = reinterpret_cast<FwSlot*>(static_cast<uint8_t*>(d_state) + sizeof(FwSlice));
    a.W = p->num_workers;
    a.Q = p->frame.max_outstanding_pkts;
    a.job = (uint8_t)p->frame.job_id;
    a.pool_start = p->frame.pool_index_start;
    a.pool_shift = p->frame.pool_index_shift;
    a.flt = p->data_type != SML_INT32;
    wire::worker_header(p->frame, p->packet_numel, a.hdr);
    return a;
}

// The tx ring's payload store policy, the frame kernels': non-temporal for a
// ring in device memory from the threshold on; host rings keep the default.
static bool fw_tx_nt(const void* tx, uint64_t bytes) {
    if (!nt_from(bytes)) return false;
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, tx) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return pa.type == hipMemoryTypeDevice;
}

// The slice's element policy: INT32 and FLOAT32 are their words.
template <class F>
static void fw_dispatch_type(uint32_t data_type, F&& f) {
    if (data_type == SML_FLOAT16) f(Slice16<kHalfF16>{});
    else if (data_type == SML_BFLOAT16) f(Slice16<kHalfBF16>{});
    else f(SliceWords{});
}

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_frame_worker_state_bytes(uint32_t max_outstanding_pkts) {
    FwLayout l;
    return fw_layout(max_outstanding_pkts, l) ? l.total : 0;
}

sml_status_t sml_frame_worker_reset(void* d_state, uint32_t max_outstanding_pkts, void* stream) {
    if (!d_state) return SML_ERR_INVALID_ARG;
    FwLayout l;
    if (!fw_layout(max_outstanding_pkts, l)) return SML_ERR_UNSUPPORTED;
    if (!aligned16(d_state)) return SML_ERR_ALIGNMENT;
    uint8_t* const st8 = static_cast<uint8_t*>(d_state);
    k_fw_reset<<<grid_for_vec(max_outstanding_pkts), kBlockThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<FwSlice*>(st8), reinterpret_cast<FwSlot*>(st8 + l.slots), max_outstanding_pkts);
    return launch_check();
}

sml_status_t sml_frame_worker_begin(const sml_frame_worker_params* prm, const void* d_in, void* d_out, uint64_t numel,
                                    void* d_state, void* tx, uint64_t tx_stride, uint64_t* d_sends, void* stream) {
    if (!prm || prm->num_workers == 0 || !d_state || !d_sends) return SML_ERR_INVALID_ARG;
    if (numel && (!d_in || !d_out || !tx)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = fw_check_params(prm, 0);
    if (st != SML_OK) return st;
    const uint32_t P = prm->packet_numel, Q = prm->frame.max_outstanding_pkts;
    const bool flt = prm->data_type != SML_INT32;
    FwSlice s;
    memset(&s, 0, sizeof(s));
    s.in = (uint64_t)(uintptr_t)d_in;
    s.out = (uint64_t)(uintptr_t)d_out;
    s.numel = numel;
    s.B = sml_num_blocks(numel, P);
    s.b = (uint32_t)(s.B < Q ? s.B : Q);
    s.total = flt ? s.B + s.b : s.B;
    if (s.total > kFwMaxPktIds) return SML_ERR_UNSUPPORTED;
    const uintptr_t esz = prm->data_type == SML_FLOAT16 || prm->data_type == SML_BFLOAT16 ? 2 : 4;
    if (!aligned16(d_state) || !aligned8(d_sends)) return SML_ERR_ALIGNMENT;
    if (numel && !wire::frame_set_fits(tx, tx_stride, P)) return SML_ERR_ALIGNMENT;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & (esz - 1)) return SML_ERR_ALIGNMENT;

    FwArgs a = fw_args(prm, d_state, 0);
    a.tx = static_cast<uint8_t*>(tx);
    a.tx_stride = tx_stride;
    a.nts = numel && fw_tx_nt(tx, (uint64_t)Q * tx_stride);
    a.sends = reinterpret_cast<unsigned long long*>(d_sends);
    fw_dispatch_type(prm->data_type, [&](auto Ec) {
        using E = decltype(Ec);
        dispatch_packet(P, [&](auto Pc) {
            const uint32_t grid = grid_for_tiles((Q + FwGroups<Pc()>::F - 1) / FwGroups<Pc()>::F);
            k_fw_begin<E, Pc()><<<grid, kBlockThreads, 0, (hipStream_t)stream>>>(a, s);
        });
    });
    return launch_check();
}

sml_status_t sml_frame_worker_poll(const sml_frame_worker_params* prm, const void* rx, uint64_t n, uint64_t rx_stride,
                                   const uint64_t* d_num_frames, void* d_state, void* tx, uint64_t tx_stride,
                                   uint64_t* d_sends, uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (n && (!rx || !d_state || !tx || !d_sends || !d_verdict)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = fw_check_params(prm, n);
    if (st != SML_OK) return st;
    if (n == 0) return SML_OK;
    const uint32_t P = prm->packet_numel, Q = prm->frame.max_outstanding_pkts;
    const uintptr_t r0 = (uintptr_t)rx, t0 = (uintptr_t)tx;
    if (r0 < t0 + (uintptr_t)Q * tx_stride && t0 < r0 + (uintptr_t)n * rx_stride) return SML_ERR_INVALID_ARG;
    if (!wire::frame_set_fits(rx, rx_stride, P) || !wire::frame_set_fits(tx, tx_stride, P)) return SML_ERR_ALIGNMENT;
    if (!aligned16(d_state) || !aligned8(d_num_frames) || !aligned8(d_sends) || !aligned8(d_counts))
        return SML_ERR_ALIGNMENT;

    FwArgs a = fw_args(prm, d_state, n);
    a.rx = static_cast<const uint8_t*>(rx);
    a.rx_stride = rx_stride;
    a.live = reinterpret_cast<const unsigned long long*>(d_num_frames);
    a.tx = static_cast<uint8_t*>(tx);
    a.tx_stride = tx_stride;
    a.nts = fw_tx_nt(tx, (uint64_t)Q * tx_stride);
    a.sends = reinterpret_cast<unsigned long long*>(d_sends);
    a.verdict = d_verdict;
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    const hipStream_t s = (hipStream_t)stream;
    k_fw_judge<<<grid_for_vec(n), kBlockThreads, 0, s>>>(a);
    const bool rne = a.flt && (prm->flags & SML_FLAG_ROUND_RNE) != 0;    // INT32 does not round
    fw_dispatch_type(prm->data_type, [&](auto Ec) {
        using E = decltype(Ec);
        dispatch_packet(P, [&](auto Pc) {
            const uint32_t grid = grid_for_tiles((n + FwGroups<Pc()>::F - 1) / FwGroups<Pc()>::F);
            dispatch_bools([&](auto RNE) { k_fw_accept<E, Pc(), RNE()><<<grid, kBlockThreads, 0, s>>>(a); }, rne);
        });
    });
    return launch_check();
}

sml_status_t sml_frame_worker_resend(const sml_frame_worker_params* prm, const uint32_t* d_slots, uint64_t n,
                                     void* d_state, uint64_t* d_sends, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (n && (!d_slots || !d_state || !d_sends)) return SML_ERR_INVALID_ARG;
    const sml_status_t st = fw_check_params(prm, n);
    if (st != SML_OK) return st;
    if (n == 0) return SML_OK;
    if (!aligned16(d_state) || !aligned4(d_slots) || !aligned8(d_sends)) return SML_ERR_ALIGNMENT;
    FwArgs a = fw_args(prm, d_state, n);
    a.slots_in = d_slots;
    a.sends = reinterpret_cast<unsigned long long*>(d_sends);
    k_fw_resend<<<grid_for_vec(n), kBlockThreads, 0, (hipStream_t)stream>>>(a);
    return launch_check();
}

}  // extern "C"
