// sml_packets.hip — the reference's per-packet PreprocessSingle /
// PostprocessSingle (ppp.cc:69-192, 194-299) for a BURST of packets in one
// launch: what a DPDK worker does between rte_eth_rx_burst and
// rte_eth_tx_burst (dpdk_worker_thread.cc:276-345: PostprocessSingle for
// every received packet, then ReusePacket -> PreprocessSingle of pkt_id + b,
// dpdk_worker_thread_utils.inc:134,177), or an RDMA worker over its
// completions (rdma_worker_thread.cc:244,356).
//
// One wave per packet (a packet is at most 1024 elements = one wave's tile);
// the packet buffers are anywhere the device can address (HBM, or pinned host
// memory such as a NIC's mbuf pool) and are read / written in place:
//   preprocess, packet q:  q >= b: block k = q - b quantized with the scale
//                          of the exponent received for packet k, htonl'd,
//                          the n = min(P, numel - kP) real words written
//                          (the reference leaves the tail of a partial block
//                          stale, ppp.cc:102-109: so do we);
//                          q < B: the exponent of block q into byte 0 of the
//                          extra-info slot (byte 1 untouched, ppp.cc:154)
//   postprocess, packet q: q >= b: block q - b dequantized from the packet
//                          into the slice output (n words);
//                          q < B: the packet's exponent byte kept as block
//                          q's received exponent (ppp.cc:254-260 keeps the
//                          scale; the kernels derive the same scale from it)
// INT32 slices: byte swaps both ways, packet q = block q (ppp.cc:158-190,
// 262-298).  Bit-identical to calling the per-packet entry points in order;
// the only ordering the reference's loop guarantees — packet q + b is
// preprocessed after packet q is postprocessed — is the caller's, across
// bursts (a burst holding both q and q + b is refused), or the exchange
// burst's, which does both for a received packet in one wave (post of q,
// then pre of q + b into the same buffer: one launch per rx burst).
//
// FLOAT16 / BFLOAT16 slices (the sml_*_burst_typed entry points): a block of
// the slice is widened to fp32 bits as it is loaded and the dequantized fp32
// values are narrowed (round to nearest even) as they are stored; everything
// between — wire words, exponents, scales — is the FLOAT32 packet, byte for
// byte.  The slice's element type is the policy E of the two slice-side
// phases (SliceWords, Slice16<H>), nothing else knows it.
//
// Each rule is written once.  Device: the phases of one packet (PacketLanes,
// real_words, load_words / store_words for packets and blocks of the slice,
// store_block_exponent, pack_block, unpack_block, payload_of), which the three
// bodies preprocess_one / postprocess_one / exchange_one only compose.  Host:
// check_burst (every argument rule) and launch_burst (the one launch site).
#include <algorithm>
#include <chrono>

#include "sml_host.h"

namespace sml {

// ---- the phases of one packet ---------------------------------------------
// A packet of P words is held by one wave as U slices of 256 words: lane l
// holds words [j(u), j(u) + 4), j(u) = 256 u + 4 l.  Every phase touches
// words j + t < n only, and n <= P, so the lanes past a packet of fewer than
// 256 words (4 l >= P) drop out of every phase without a test of their own.
template <int P>
struct PacketLanes {
    static constexpr int U = P > 256 ? P / 256 : 1;
    const int lane = threadIdx.x & (kWave - 1);
    __device__ __forceinline__ uint64_t j(int u) const { return (uint64_t)u * 256 + lane * 4; }
};

// The real words of block k: P, or what the slice has left in its last block.
template <int P>
__device__ __forceinline__ uint64_t real_words(const sml_packet_burst& a, uint64_t k) {
    return a.numel - k * P < P ? a.numel - k * P : P;
}

// A lane's four words [j, j + 4) of the n words of a buffer: one 16-byte access
// where the group is whole (a packet over PCIe then costs one access per 64 B
// line, not four), single words in the group that n cuts.  The load gives 0
// past n; the store writes nothing at or past n.
__device__ __forceinline__ void load_group(const uint32_t* buf, uint64_t j, uint64_t n, uint32_t (&v)[4]) {
    if (j + 4 <= n) {
        const u4a q = *reinterpret_cast<const u4a*>(buf + j);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = j + t < n ? buf[j + t] : 0u;
    }
}

__device__ __forceinline__ void store_group(uint32_t* buf, uint64_t j, uint64_t n, const uint32_t (&v)[4]) {
    if (j + 4 <= n) {
        *reinterpret_cast<u4a*>(buf + j) = u4a{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (j + t < n) buf[j + t] = v[t];
    }
}

// What a buffer's elements are to load_group / store_group: the words
// themselves (packet buffers; FLOAT32 and INT32 slices, whose elements are
// their bits), or 16-bit floats held as fp32 bits in registers (FLOAT16 /
// BFLOAT16 slices).  is_float: whether the slice takes the float rules — a
// 16-bit instance has no INT32 branch.
struct SliceWords {
    typedef uint32_t raw;
    static __device__ __forceinline__ bool is_float(const sml_packet_burst& a) { return a.data_type == SML_FLOAT32; }
    static __device__ __forceinline__ void load_group(const raw* buf, uint64_t j, uint64_t n, uint32_t (&v)[4]) {
        sml::load_group(buf, j, n, v);
    }
    static __device__ __forceinline__ void store_group(raw* buf, uint64_t j, uint64_t n, const uint32_t (&v)[4]) {
        sml::store_group(buf, j, n, v);
    }
};

// A lane's four elements are one 8-byte access through the 2-byte-aligned
// vector type where the group is whole (a slice starts at any element),
// single elements in the group that n cuts; widened (exact) right after the
// load, narrowed (round to nearest even) right before the store.
template <int H>
struct Slice16 {
    typedef uint16_t raw;
    static __device__ __forceinline__ bool is_float(const sml_packet_burst&) { return true; }
    static __device__ __forceinline__ void load_group(const raw* buf, uint64_t j, uint64_t n, uint32_t (&v)[4]) {
        if (j + 4 <= n) {
            const h4a q = *reinterpret_cast<const h4a*>(buf + j);
            v[0] = __float_as_uint(widen16<H>(q.x)), v[1] = __float_as_uint(widen16<H>(q.y));
            v[2] = __float_as_uint(widen16<H>(q.z)), v[3] = __float_as_uint(widen16<H>(q.w));
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) v[t] = j + t < n ? __float_as_uint(widen16<H>(buf[j + t])) : 0u;
        }
    }
    static __device__ __forceinline__ void store_group(raw* buf, uint64_t j, uint64_t n, const uint32_t (&v)[4]) {
        if (j + 4 <= n) {
            *reinterpret_cast<h4a*>(buf + j) =
                h4a{narrow16<H>(__uint_as_float(v[0])), narrow16<H>(__uint_as_float(v[1])),
                    narrow16<H>(__uint_as_float(v[2])), narrow16<H>(__uint_as_float(v[3]))};
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (j + t < n) buf[j + t] = narrow16<H>(__uint_as_float(v[t]));
        }
    }
};

// Elements [0, n) of a buffer <-> w: a packet buffer's words (E = SliceWords),
// or a block of the slice as fp32 bits.
template <class E = SliceWords, int P, int U>
__device__ __forceinline__ void load_words(PacketLanes<P> g, const typename E::raw* buf, uint64_t n,
                                           uint32_t (&w)[U][4]) {
#pragma unroll
    for (int u = 0; u < U; u++) E::load_group(buf, g.j(u), n, w[u]);
}

template <class E = SliceWords, int P, int U>
__device__ __forceinline__ void store_words(PacketLanes<P> g, typename E::raw* buf, uint64_t n,
                                            const uint32_t (&w)[U][4]) {
#pragma unroll
    for (int u = 0; u < U; u++) E::store_group(buf, g.j(u), n, w[u]);
}

// Block k of the slice (FLOAT32: its bits as words), for load_words<E>.
template <class E, int P>
__device__ __forceinline__ const typename E::raw* block_words(const sml_packet_burst& a, uint64_t k) {
    return reinterpret_cast<const typename E::raw*>(a.in) + k * P;
}
// Block k of the output, for unpack_block<E>.
template <class E, int P>
__device__ __forceinline__ typename E::raw* block_out(const sml_packet_burst& a, uint64_t k) {
    return reinterpret_cast<typename E::raw*>(a.out) + k * P;
}
__device__ __forceinline__ f4 as_f4(const uint32_t (&v)[4]) {
    return mkf4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// The exponent of the block in x (0 past its real words) into byte 0 of the
// packet's extra-info slot; byte 1 is never written (ppp.cc:154).
template <int P, int U>
__device__ __forceinline__ void store_block_exponent(PacketLanes<P> g, const uint32_t (&x)[U][4], void* extra) {
    uint32_t m = 0;
#pragma unroll
    for (int u = 0; u < U; u++) m = umax(m, max4(as_f4(x[u])));
    m = group_max<256>(m);                                  // the wave's max = the packet's
    if (g.lane == 0) *static_cast<int8_t*>(extra) = (int8_t)exponent_of(m);
}

// The n words of the block in x, big-endian, into w; the other words of w
// keep their value.  FLOAT32: quantized with scale s, VCL=1 rounding (RNE) on
// the 16-aligned body of the block; INT32: as they are.
template <int P, bool RNE, int U>
__device__ __forceinline__ void pack_block(PacketLanes<P> g, bool flt, const uint32_t (&x)[U][4], float s, uint64_t n,
                                           uint32_t (&w)[U][4]) {
    const uint64_t body = n / 16 * 16;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t j = g.j(u);
        const u4 v = flt ? quantize4<RNE>(as_f4(x[u]), s, j, body) : mku4(x[u][0], x[u][1], x[u][2], x[u][3]);
        const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (j + t < n) w[u][t] = bswap(vv[t]);
    }
}

// Words [0, n) of w into the n elements of a block of the output: dequantized
// with scale s (a float type; a 16-bit one narrowed by E's store), or
// byte-swapped (INT32).
template <class E, int P, int U>
__device__ __forceinline__ void unpack_block(PacketLanes<P> g, bool flt, const uint32_t (&w)[U][4], float s, uint64_t n,
                                             typename E::raw* out) {
#pragma unroll
    for (int u = 0; u < U; u++) {
        uint32_t v[4];   // every word of the group converted, whole group or not: four divisions in flight
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = flt ? __float_as_uint(dequantize1(bswap(w[u][t]), s)) : bswap(w[u][t]);
        E::store_group(out, g.j(u), n, v);
    }
}

// Which block packet q carries: FLOAT32 packets run one window behind their
// exponents (block q - b, none for q < b); INT32 packet q carries block q.
struct Payload { bool on; uint64_t k; };
__device__ __forceinline__ Payload payload_of(const sml_packet_burst& a, bool flt, uint64_t q) {
    const bool on = !flt || q >= a.batch_num_ltus;
    return {on, !on ? 0 : flt ? q - a.batch_num_ltus : q};
}

// ---- the three per-packet bodies ------------------------------------------
// PreprocessSingle of packet q: its block into the packet with the scale of
// the exponent received for that block (recv_exps, in memory), only the real
// words written; the exponent of block q into the extra slot (FLOAT32, q < B).
template <class E, int P, bool RNE>
__device__ __forceinline__ void preprocess_one(const sml_packet_burst& a, uint32_t i) {
    const PacketLanes<P> g{};
    constexpr int U = PacketLanes<P>::U;
    const uint64_t q = a.pkt_ids[i];
    const uint64_t B = (a.numel + P - 1) / P;
    const bool flt = E::is_float(a);
    const Payload pay = payload_of(a, flt, q);
    uint32_t x[U][4];
    if (pay.on) {
        const uint64_t n = real_words<P>(a, pay.k);
        const int e = flt ? (int)a.recv_exps[pay.k] : 0;   // asked for ahead of the block: one wait for both
        uint32_t w[U][4] = {};
        load_words<E>(g, block_words<E, P>(a, pay.k), n, x);
        const float s = flt ? scale_for(a.num_workers, e) : 0.0f;
        pack_block<P, RNE>(g, flt, x, s, n, w);
        store_words(g, static_cast<uint32_t*>(a.entries[i]), n, w);
    }
    if (flt && q < B) {
        load_words<E>(g, block_words<E, P>(a, q), real_words<P>(a, q), x);
        store_block_exponent(g, x, a.extras[i]);
    }
}

// PostprocessSingle of packet q: its block out of the packet into the slice
// output; the packet's exponent byte kept as block q's received exponent.
template <class E, int P>
__device__ __forceinline__ void postprocess_one(const sml_packet_burst& a, uint32_t i) {
    const PacketLanes<P> g{};
    constexpr int U = PacketLanes<P>::U;
    const uint64_t q = a.pkt_ids[i];
    const uint64_t B = (a.numel + P - 1) / P;
    const bool flt = E::is_float(a);
    const Payload pay = payload_of(a, flt, q);
    if (pay.on) {
        const uint64_t n = real_words<P>(a, pay.k);
        const int e = flt ? (int)a.recv_exps[pay.k] : 0;   // asked for ahead of the packet: one wait for both
        uint32_t w[U][4];
        load_words(g, static_cast<const uint32_t*>(a.entries[i]), n, w);
        const float s = flt ? scale_for(a.num_workers, e) : 0.0f;
        unpack_block<E>(g, flt, w, s, n, block_out<E, P>(a, pay.k));
    }
    if (flt && q < B && g.lane == 0) a.recv_exps[q] = *static_cast<const int8_t*>(a.extras[i]);
}

// One wave per RECEIVED packet q, the DPDK receive loop's two calls on one
// mbuf in one launch (dpdk_worker_thread.cc:300-345: PostprocessSingle of the
// packet, then ReusePacket -> PreprocessSingle of pkt_id + b into the same
// buffer, dpdk_worker_thread_utils.inc:134,177), optionally preceded by the
// dummy backend's ProcessPacket (x W on all P words, dummy_backend.cc:72-84):
//   FLOAT32  post: q >= b: block q - b dequantized with recv_exps[q - b];
//                  q < B: the packet's exponent byte -> recv_exps[q]
//            pre (q < B, i.e. q + b < B + b): block q quantized with that same
//                  received exponent (its n real words; a partial block's tail
//                  keeps the packet's words), exponent of block q + b into
//                  byte 0 of the extra slot when q + b < B
//   INT32    post: block q byte-swapped into out; pre (q + b < B): block q + b
//                  byte-swapped into the buffer (b = the packet window)
// Every load of the packet is waited for before its buffer is written: the
// reads and the writes of one buffer may cross PCIe (pinned mbufs), where a
// posted write may overtake an outstanding read.
template <class E, int P, bool RNE, bool PROC>
__device__ __forceinline__ void exchange_one(const sml_packet_burst& a, uint32_t i) {
    const PacketLanes<P> g{};
    constexpr int U = PacketLanes<P>::U;
    const uint64_t q = a.pkt_ids[i];
    const uint64_t B = (a.numel + P - 1) / P;
    const uint64_t b = a.batch_num_ltus;
    const bool flt = E::is_float(a);
    uint32_t* ent = static_cast<uint32_t*>(a.entries[i]);

    // what each half touches: post reads words [0, n_post) of the packet
    // (all P under PROC), pre rewrites words [0, n_pre) with block k_pre
    const Payload post = payload_of(a, flt, q);
    const uint64_t n_post = post.on ? real_words<P>(a, post.k) : 0;
    const uint64_t k_pre = flt ? q : q + b;
    const uint64_t n_pre = k_pre < B ? real_words<P>(a, k_pre) : 0;
    const uint64_t n_exp = flt && q + b < B ? real_words<P>(a, q + b) : 0;   // the block whose exponent goes out

    // ---- every load up front; the packet's own (words, aggregated exponent
    // byte: they may cross PCIe) first, so that they are in flight together
    uint32_t w[U][4], xq[U][4], xe[U][4];
    load_words(g, ent, PROC ? P : n_post, w);
    const int e_recv = flt && q < B ? (int)*static_cast<const int8_t*>(a.extras[i]) : 0;
    const int e_post = flt && post.on ? (int)a.recv_exps[post.k] : 0;
    load_words<E>(g, block_words<E, P>(a, n_pre ? k_pre : 0), n_pre, xq);
    load_words<E>(g, block_words<E, P>(a, n_exp ? q + b : 0), n_exp, xe);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // ---- ProcessPacket, postprocess
    const uint32_t W = a.num_workers;
    if constexpr (PROC) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int t = 0; t < 4; t++) w[u][t] = bswap(bswap(w[u][t]) * W);
    }
    unpack_block<E>(g, flt, w, flt ? scale_for(W, e_post) : 0.0f, n_post, block_out<E, P>(a, post.k));
    if (flt && q < B && g.lane == 0) a.recv_exps[q] = (int8_t)e_recv;

    // ---- preprocess of q + b into the same buffer: its words are the new
    // packet's, or (PROC) the processed ones where the new packet has none
    pack_block<P, RNE>(g, flt, xq, flt ? scale_for(W, e_recv) : 0.0f, n_pre, w);
    store_words(g, ent, PROC ? P : n_pre, w);
    if (n_exp) store_block_exponent(g, xe, a.extras[i]);
}

// One launch per burst: a wave per packet.  E: the slice's element policy.
template <class E, int P, bool RNE>
__global__ __launch_bounds__(kBlockThreads) void k_preprocess_burst(sml_packet_burst a) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + wave_index();
    if (i < a.count) preprocess_one<E, P, RNE>(a, i);
}

template <class E, int P>
__global__ __launch_bounds__(kBlockThreads) void k_postprocess_burst(sml_packet_burst a) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + wave_index();
    if (i < a.count) postprocess_one<E, P>(a, i);
}

template <class E, int P, bool RNE, bool PROC>
__global__ __launch_bounds__(kBlockThreads) void k_exchange_burst(sml_packet_burst a) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + wave_index();
    if (i < a.count) exchange_one<E, P, RNE, PROC>(a, i);
}

// ---- the persistent burst server (include/switchml_hip.h) ----------------
// kServerGroups resident workgroups of 16 waves — one wave per packet of a
// full burst — poll a doorbell in coherent, device-mapped host memory.  Per
// burst, in every workgroup: thread 0 polls the doorbell with relaxed
// system-scope loads and, once it moves, acquires at system scope (no stale
// copy of the host-written descriptor or packets); a barrier orders the other
// threads after it; the descriptor is copied into LDS with system-scope
// loads; the waves run their packets (the same per-packet bodies as the
// one-launch-per-burst kernels); a barrier orders every wave's stores before
// thread 0, which releases them at system scope and arrives on a counter in
// device memory.  The last workgroup to arrive resets the counter and
// publishes the burst's sequence number with a system-scope release store;
// the host submits the next burst only after that, so no workgroup can run
// ahead into the next burst.  FLOAT32 and INT32 slices only (SliceWords): a
// 16-bit slice never comes here (check_burst refuses it for the server).  The loop ends on `stop` or after idle_ticks of
// wall clock without a doorbell, so every wave reaches the exit on its own;
// the host restarts a server that has been idle for half that long before
// ringing it again, so a doorbell never races an idle exit.
constexpr int kServerThreads = 1024;
constexpr int kServerGroups = SML_MAX_BURST / (kServerThreads / kWave);   // 4

struct alignas(64) ServerCtl {
    uint64_t doorbell;         // host: (sequence number << 2) | SML_BURST_* of the last submitted burst
    uint32_t stop;             // host: 1 = leave the loop
    uint32_t pad_stop;
    uint64_t pad0[6];
    uint64_t done;             // device: sequence number of the last completed burst
    uint32_t exited[kServerGroups];   // device: workgroup g has left its loop
    uint64_t pad2[5];
    sml_packet_burst burst;    // host: the submitted burst
};

// A system-scope load without acquire semantics: polling must not invalidate
// the caches on every probe (an acquire load does); the one acquire fence
// follows the probe that sees the doorbell.
template <class T>
__device__ __forceinline__ T sys_poll(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int P, bool RNE>
__global__ __launch_bounds__(kServerThreads) void k_burst_server(ServerCtl* ctl, uint32_t* arrive,
                                                                 uint64_t idle_ticks) {
    __shared__ sml_packet_burst sa;
    __shared__ uint64_t s_seq;
    __shared__ int s_cmd;
    constexpr uint32_t kWaves = kServerThreads / kWave;
    constexpr uint32_t kAllWaves = kWaves * kServerGroups;
    const uint32_t tid = threadIdx.x;
    uint64_t seen = tid == 0 ? sys_poll(&ctl->done) : 0;
    for (;;) {
        if (tid == 0) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            int cmd = -1;
            uint64_t db = seen;
            for (;;) {
                if (sys_poll(&ctl->stop)) break;
                db = sys_poll(&ctl->doorbell) >> 2;
                if (db != seen) {
                    // acquire once, by the thread that saw the doorbell; the
                    // barrier below orders every other thread after it.  The
                    // op rides in the doorbell word (no second round trip).
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                    cmd = (int)(sys_poll(&ctl->doorbell) & 3u);
                    break;
                }
                if (__builtin_amdgcn_s_memrealtime() - t0 > idle_ticks) break;
                __builtin_amdgcn_s_sleep(2);
            }
            s_cmd = cmd;
            s_seq = db;
        }
        __syncthreads();
        const int cmd = s_cmd;
        if (cmd < 0) break;
        static_assert(sizeof(sml_packet_burst) % 8 == 0, "descriptor copied in 8-byte words");
        constexpr uint32_t kWords = sizeof(sml_packet_burst) / 8;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(&ctl->burst);
        uint64_t* dst = reinterpret_cast<uint64_t*>(&sa);
        for (uint32_t k = tid; k < kWords; k += kServerThreads)
            dst[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __syncthreads();
        const uint32_t n = sa.count;
        const bool proc = (sa.flags & SML_FLAG_PROCESS_PACKET) != 0;
        for (uint32_t i = blockIdx.x * kWaves + wave_index(); i < n; i += kAllWaves) {
            if (cmd == SML_BURST_PRE) preprocess_one<SliceWords, P, RNE>(sa, i);
            else if (cmd == SML_BURST_POST) postprocess_one<SliceWords, P>(sa, i);
            else if (proc) exchange_one<SliceWords, P, RNE, true>(sa, i);
            else exchange_one<SliceWords, P, RNE, false>(sa, i);
        }
        __syncthreads();
        if (tid == 0) {
            seen = s_seq;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // this workgroup's stores, system-wide
            const uint32_t before = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (before == kServerGroups - 1) {              // the last one: every group's stores are released
                __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&ctl->done, seen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    if (tid == 0) __hip_atomic_store(&ctl->exited[blockIdx.x], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Host checks of a burst for op SML_BURST_PRE / POST / EXCHANGE, shared by the
// launched entry points and the server.  The preprocess reads the slice, the
// postprocess writes the output, the exchange does both; its packet window b
// applies to INT32 slices too (the next packet is q + b).  half_ok (the
// _typed entry points): FLOAT16 / BFLOAT16 pass, under the FLOAT32 rules.
static sml_status_t check_burst(const sml_packet_burst* a, uint32_t op, bool half_ok = false) {
    const bool window = op == SML_BURST_EXCHANGE;
    if (!a) return SML_ERR_INVALID_ARG;
    if (!valid_packet(a->packet_numel)) return SML_ERR_UNSUPPORTED;
    if (a->count > SML_MAX_BURST || a->num_workers == 0) return SML_ERR_INVALID_ARG;
    const bool half = a->data_type == SML_FLOAT16 || a->data_type == SML_BFLOAT16;
    if (a->data_type != SML_FLOAT32 && a->data_type != SML_INT32 && !(half && half_ok)) return SML_ERR_UNSUPPORTED;
    if (a->count == 0) return SML_OK;
    if ((op != SML_BURST_POST && !a->in) || (op != SML_BURST_PRE && !a->out)) return SML_ERR_INVALID_ARG;
    const uint64_t P = a->packet_numel;
    const uint64_t B = sml_num_blocks(a->numel, (uint32_t)P);
    const bool flt = a->data_type != SML_INT32;
    const uint64_t b = flt || window ? a->batch_num_ltus : 0;
    if ((flt || window) && b > B) return SML_ERR_INVALID_ARG;
    if (window && b == 0) return SML_ERR_INVALID_ARG;
    if (flt && !a->recv_exps) return SML_ERR_INVALID_ARG;
    const uint64_t total = flt ? B + b : B;
    bool run = true;   // ids q0, q0 + 1, ... (a ring pass): distinct, and q0 + b is not among them if count <= b
    for (uint32_t i = 0; i < a->count; i++) {
        const uint64_t q = a->pkt_ids[i];
        if (q >= total || !a->entries[i] || (flt && q < B && !a->extras[i])) return SML_ERR_INVALID_ARG;
        if (window && flt && q + b < B && !a->extras[i]) return SML_ERR_INVALID_ARG;
        run = run && q == a->pkt_ids[0] + i;
    }
    if (run && (b == 0 || a->count <= b)) return SML_OK;
    // any other order: distinct, and never q and q + b together (sorted copy)
    uint64_t ids[SML_MAX_BURST];
    std::copy(a->pkt_ids, a->pkt_ids + a->count, ids);
    std::sort(ids, ids + a->count);
    for (uint32_t i = 1; i < a->count; i++)
        if (ids[i] == ids[i - 1]) return SML_ERR_INVALID_ARG;
    if (b)
        for (uint32_t i = 0; i < a->count; i++)
            if (std::binary_search(ids, ids + a->count, ids[i] + b)) return SML_ERR_INVALID_ARG;
    return SML_OK;
}

// The slice's element policy from its sml_data_type_t (checked by check_burst).
template <class F>
static void dispatch_slice_type(uint32_t data_type, F&& f) {
    if (data_type == SML_FLOAT16) f(Slice16<kHalfF16>{});
    else if (data_type == SML_BFLOAT16) f(Slice16<kHalfBF16>{});
    else f(SliceWords{});
}

// One launch for the burst, a wave per packet, on `stream`: the kernel of op
// for the slice's element type, the burst's packet size and the flags that op
// knows.
static sml_status_t launch_burst(const sml_packet_burst* burst, uint32_t op, void* stream, bool half_ok = false) {
    const sml_status_t st = check_burst(burst, op, half_ok);
    if (st != SML_OK || burst->count == 0) return st;
    const sml_packet_burst& a = *burst;
    const dim3 grid((a.count + kWavesPerBlock - 1) / kWavesPerBlock);
    const hipStream_t s = (hipStream_t)stream;
    const bool rne = (a.flags & SML_FLAG_ROUND_RNE) != 0;
    const bool proc = (a.flags & SML_FLAG_PROCESS_PACKET) != 0;
    dispatch_slice_type(a.data_type, [&](auto Ec) {
        using E = decltype(Ec);
        dispatch_packet(a.packet_numel, [&](auto Pc) {
            dispatch_bools([&](auto RNE, auto PROC) {
                if (op == SML_BURST_PRE) k_preprocess_burst<E, Pc(), RNE()><<<grid, kBlockThreads, 0, s>>>(a);
                else if (op == SML_BURST_POST) k_postprocess_burst<E, Pc()><<<grid, kBlockThreads, 0, s>>>(a);
                else k_exchange_burst<E, Pc(), RNE(), PROC()><<<grid, kBlockThreads, 0, s>>>(a);
            }, rne, proc);
        });
    });
    return launch_check();
}

// The _typed entry points: FLOAT32 / INT32 (and a NULL burst) are the untyped
// twin's, before any check of their own; the 16-bit types run their instances
// under the FLOAT32 argument rules; anything else is unsupported.
static sml_status_t launch_burst_typed(const sml_packet_burst* burst, uint32_t op, void* stream) {
    if (!burst || burst->data_type == SML_FLOAT32 || burst->data_type == SML_INT32)
        return launch_burst(burst, op, stream);
    if (burst->data_type != SML_FLOAT16 && burst->data_type != SML_BFLOAT16) return SML_ERR_UNSUPPORTED;
    return launch_burst(burst, op, stream, true);
}

}  // namespace sml

using namespace sml;

extern "C" {

sml_status_t sml_preprocess_burst(const sml_packet_burst* burst, void* stream) {
    return launch_burst(burst, SML_BURST_PRE, stream);
}

sml_status_t sml_postprocess_burst(const sml_packet_burst* burst, void* stream) {
    return launch_burst(burst, SML_BURST_POST, stream);
}

sml_status_t sml_exchange_burst(const sml_packet_burst* burst, void* stream) {
    return launch_burst(burst, SML_BURST_EXCHANGE, stream);
}

sml_status_t sml_preprocess_burst_typed(const sml_packet_burst* burst, void* stream) {
    return launch_burst_typed(burst, SML_BURST_PRE, stream);
}

sml_status_t sml_postprocess_burst_typed(const sml_packet_burst* burst, void* stream) {
    return launch_burst_typed(burst, SML_BURST_POST, stream);
}

sml_status_t sml_exchange_burst_typed(const sml_packet_burst* burst, void* stream) {
    return launch_burst_typed(burst, SML_BURST_EXCHANGE, stream);
}

}  // extern "C"

struct sml_burst_server {
    sml::ServerCtl* ctl = nullptr;    // host address (coherent, device-mapped)
    sml::ServerCtl* dctl = nullptr;   // the same memory at its device address
    uint32_t* arrive = nullptr;       // device memory: workgroups done with the current burst
    hipStream_t stream = nullptr;
    uint32_t packet_numel = 0;
    bool rne = false;
    uint64_t idle_ticks = 0;
    std::chrono::milliseconds restart_after{50};   // half the server's idle time
    uint64_t seq = 0;
    bool launched = false;            // a kernel was launched and not yet joined
    std::chrono::steady_clock::time_point last_activity;
};

namespace {

uint64_t host_load(const volatile uint64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }

bool any_exited(const sml_burst_server* s) {
    for (int g = 0; g < sml::kServerGroups; g++)
        if (__atomic_load_n(&s->ctl->exited[g], __ATOMIC_ACQUIRE)) return true;
    return false;
}

// Stop a launched server (if any) and wait for every workgroup to leave.
sml_status_t server_join(sml_burst_server* s) {
    if (!s->launched) return SML_OK;
    __atomic_store_n(&s->ctl->stop, 1u, __ATOMIC_RELEASE);
    s->launched = false;
    return sml::hip_check(hipStreamSynchronize(s->stream));
}

sml_status_t server_launch(sml_burst_server* s) {
    sml_status_t st = server_join(s);
    if (st != SML_OK) return st;
    for (int g = 0; g < sml::kServerGroups; g++) __atomic_store_n(&s->ctl->exited[g], 0u, __ATOMIC_RELEASE);
    __atomic_store_n(&s->ctl->stop, 0u, __ATOMIC_RELEASE);
    // The new kernel starts from seen = done.  After a failed burst (timeout,
    // a workgroup's idle exit mid-burst) done lags the last doorbell; the
    // relaunched server would take that stale doorbell for a new burst and
    // replay its descriptor (an exchange burst applied twice, or buffers of a
    // finished slice).  No kernel runs here (joined above): mark every rung
    // doorbell as handled.
    __atomic_store_n(&s->ctl->done, s->seq, __ATOMIC_RELEASE);
    st = sml::hip_check(hipMemsetAsync(s->arrive, 0, sizeof(uint32_t), s->stream));
    if (st != SML_OK) return st;
    const dim3 grid(sml::kServerGroups), block(sml::kServerThreads);
    sml::dispatch_packet(s->packet_numel, [&](auto Pc) {
        sml::dispatch_bools([&](auto RNE) {
            sml::k_burst_server<Pc(), RNE()><<<grid, block, 0, s->stream>>>(s->dctl, s->arrive, s->idle_ticks);
        }, s->rne);
    });
    st = sml::launch_check();
    s->launched = st == SML_OK;
    s->last_activity = std::chrono::steady_clock::now();
    return st;
}

}  // namespace

extern "C" {

sml_status_t sml_burst_server_create(uint32_t packet_numel, uint32_t flags, uint32_t idle_ms,
                                     sml_burst_server** out) {
    if (!out) return SML_ERR_INVALID_ARG;
    *out = nullptr;
    if (!sml::valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (flags & ~SML_FLAG_ROUND_RNE) return SML_ERR_INVALID_ARG;
    int dev = 0, rate_khz = 0;
    sml_status_t st = sml::hip_check(hipGetDevice(&dev));
    if (st == SML_OK) st = sml::hip_check(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev));
    if (st != SML_OK) return st;
    auto* s = new sml_burst_server;
    const uint32_t ms = idle_ms ? idle_ms : 100;
    s->packet_numel = packet_numel;
    s->rne = (flags & SML_FLAG_ROUND_RNE) != 0;
    s->idle_ticks = (uint64_t)(rate_khz > 0 ? rate_khz : 100000) * ms;
    s->restart_after = std::chrono::milliseconds(ms / 2);
    void* h = nullptr;
    void* d = nullptr;
    st = sml::hip_check(hipHostMalloc(&h, sizeof(sml::ServerCtl), hipHostMallocMapped | hipHostMallocCoherent));
    if (st == SML_OK) {
        memset(h, 0, sizeof(sml::ServerCtl));
        st = sml::hip_check(hipHostGetDevicePointer(&d, h, 0));
    }
    if (st == SML_OK) st = sml::hip_check(hipMalloc(reinterpret_cast<void**>(&s->arrive), 64));
    if (st == SML_OK) st = sml::hip_check(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (st != SML_OK) {
        if (h) (void)hipHostFree(h);
        if (s->arrive) (void)hipFree(s->arrive);
        delete s;
        return st;
    }
    s->ctl = static_cast<sml::ServerCtl*>(h);
    s->dctl = static_cast<sml::ServerCtl*>(d);
    *out = s;
    return SML_OK;
}

sml_status_t sml_burst_server_submit(sml_burst_server* s, uint32_t op, const sml_packet_burst* burst) {
    if (!s || op > SML_BURST_EXCHANGE) return SML_ERR_INVALID_ARG;
    sml_status_t st = sml::check_burst(burst, op);
    if (st != SML_OK || burst->count == 0) return st;
    if (burst->packet_numel != s->packet_numel || ((burst->flags & SML_FLAG_ROUND_RNE) != 0) != s->rne)
        return SML_ERR_INVALID_ARG;   // fixed per server
    // not running, left its loop, or close to its idle exit: (re)start it, so
    // the doorbell below never races an idle exit
    if (!s->launched || any_exited(s) ||
        std::chrono::steady_clock::now() - s->last_activity > s->restart_after) {
        st = server_launch(s);
        if (st != SML_OK) return st;
    }
    memcpy(&s->ctl->burst, burst, sizeof(sml_packet_burst));
    __atomic_store_n(&s->ctl->doorbell, (++s->seq << 2) | op, __ATOMIC_RELEASE);
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::seconds(10);
    for (uint32_t spins = 0; host_load(&s->ctl->done) != s->seq; spins++) {
        if ((spins & 255) != 255) continue;
        if (any_exited(s) && host_load(&s->ctl->done) != s->seq) {
            (void)server_join(s);
            strncpy(sml::g_last_error, "burst server: a workgroup left its loop during a burst",
                    sizeof(sml::g_last_error) - 1);
            return SML_ERR_HIP;
        }
        if (std::chrono::steady_clock::now() > t_end) {
            (void)server_join(s);
            strncpy(sml::g_last_error, "burst server: no completion within 10 s", sizeof(sml::g_last_error) - 1);
            return SML_ERR_HIP;
        }
    }
    s->last_activity = std::chrono::steady_clock::now();
    return SML_OK;
}

sml_status_t sml_burst_server_stop(sml_burst_server* s) {
    if (!s) return SML_ERR_INVALID_ARG;
    return server_join(s);
}

sml_status_t sml_burst_server_start(sml_burst_server* s) {
    if (!s) return SML_ERR_INVALID_ARG;
    if (s->launched && !any_exited(s)) return SML_OK;
    return server_launch(s);
}

sml_status_t sml_burst_server_inject_unanswered(sml_burst_server* s, uint32_t op, const sml_packet_burst* burst) {
    if (!s || !burst || op > SML_BURST_EXCHANGE) return SML_ERR_INVALID_ARG;
    const sml_status_t st = server_join(s);
    if (st != SML_OK) return st;
    memcpy(&s->ctl->burst, burst, sizeof(sml_packet_burst));
    __atomic_store_n(&s->ctl->doorbell, (++s->seq << 2) | op, __ATOMIC_RELEASE);
    return SML_OK;
}

sml_status_t sml_burst_server_destroy(sml_burst_server* s) {
    if (!s) return SML_OK;
    const sml_status_t st = sml_burst_server_stop(s);
    (void)hipStreamDestroy(s->stream);
    (void)hipFree(s->arrive);
    (void)hipHostFree(s->ctl);
    delete s;
    return st;
}

}  // extern "C"
