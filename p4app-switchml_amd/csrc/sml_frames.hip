// sml_frames.hip — DPDK wire frames on gfx950: the transmit
// side (BuildPacket + PreprocessSingle for every packet of a slice,
// client_lib/src/backends/dpdk/dpdk_worker_thread_utils.inc:42-135) and the
// receive side (DpdkWorkerThread's rx loop, dpdk_worker_thread.cc:300-345,
// with PostprocessSingle per accepted frame), and their C-ABI entry points.
// The kernels that touch the slice's typed buffer are the templates of
// sml_frame_kernels.h, instantiated here for FLOAT32 and INT32; the FLOAT16 /
// BFLOAT16 instances are sml_frames_half.hip's.  The frame's layout is
// sml_frame_wire.h's.
#include "sml_frame_kernels.h"

namespace sml {

// Pass 1, thread per frame: frames of another job, out-of-range or already
// received pkt_ids are discarded; the others claim their pkt_id.  Counting:
// the workgroup's discards, tallied and sent by tally_flush_accepted
// (sml_device.h; same-address atomics from every workgroup serialize in one
// L2 channel: ~40 us at 262 k frames).
__global__ __launch_bounds__(kBlockThreads) void k_rx_claim(RxArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    const uint64_t f0 = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    if (!a.counts) {
        // no counters: non-returning atomics, the wave does not wait for them
        for (uint64_t f = f0; f < a.nframes; f += stride) {
            const RxHdr h = rx_header(a, f);
            if (h.ok) atomicMax(a.state + h.pid, ((unsigned long long)rx_tag(f) << 32) | h.exp);
        }
        return;
    }
    __shared__ uint32_t disc[1];
    tally_init(disc);
    uint32_t mine = 0;
    for (uint64_t f = f0; f < a.nframes; f += stride) {
        const RxHdr h = rx_header(a, f);
        if (!h.ok) { mine++; continue; }
        const unsigned long long v = ((unsigned long long)rx_tag(f) << 32) | h.exp;
        if (atomicMax(a.state + h.pid, v) != 0ull) mine++;          // duplicate or received earlier
    }
    tally_add(disc[0], mine);
    tally_flush_accepted(disc, a.counts, a.nframes);
}

// --------------------------------------- INT32 job slices, receive side
//
// An INT32 frame is self-contained — pkt_id k carries block k's words and
// there is no exponent to take from another frame (NeedsExtraBatch false,
// ppp.cc:65-67; PostprocessSingle's INT32 branch, ppp.cc:262-298) — so one
// pass in stream order decides and writes each frame: no claim pass over the
// headers, no second walk in block order.  State: uint64[2B + 6] per slice:
// [0, B) the claim words (the rx bitmap), then six header words, kRx* below:
//   [B]      the call sequence c of this slice;
//   [B + 1]  the conflicts resolved in the slice so far (a statistic: copies
//            that arrived ahead of an earlier one);
//   [B + 2]  the conflicts of the call in progress, 0 between calls;
//   [B + 3]  the length of that call's dirty list (past B: it overflowed),
//            0 between calls;
//   [B + 4]  arrivals: the fix-up workgroups that have finished over the
//            slice's life, never reset: kRxFixupBlocks * c between calls;
//   [B + 5]  what [B + 3] held when the last finished call's fix-up ended (a
//            statistic: whether that fix-up walked the list or scanned);
// and [B + 6, 2B + 6) the dirty list: the pkt_ids marked dirty in the call
// (appended by the claim that sets a pkt_id's dirty bit), so the fix-up
// visits only them.  The fix-up's workgroups all read the call's counters at
// their start; the one that finishes last clears them and advances c
// (k_rx_int32_fixup).
// A frame's tag is
//   (0xFFFFFFFF - c) << 32 | (0x7FFFFFFF - f) << 1      (bit 0: dirty),
// larger for an earlier call and, within a call, for an earlier frame f, so
// a 64-bit atomicMax on state[pkt_id] keeps the first copy of the stream,
// and a pkt_id accepted by an earlier call (higher tag) discards every later
// copy — the reference's "seen before" test (dpdk_worker_thread.cc:316-342)
// without a retirement pass.  The atomic's old value decides:
//   0                  first claim of the pkt_id: write, accepted;
//   above the tag      an earlier copy (or call) holds it: discarded;
//   below the tag      this frame is earlier than the copy that claimed first
//                      and already wrote: write too, mark the pkt_id dirty,
//                      count a conflict (the counts stay exact: the displaced
//                      copy was counted accepted, this one is counted as the
//                      discard).
// Which of two racing writes lands last is not ordered, so the fix-up
// (k_rx_int32_fixup, same stream) rewrites every dirty pkt_id from its final
// winner — the highest tag, the first copy — and then advances c.  It walks
// the dirty list over a grid of workgroups (not one workgroup
// scanning all B state words for one conflict); a list that overflowed its
// B entries (one pkt_id can be appended again when a later claim's
// atomicMax clears its dirty bit for an instant) falls back to the scan of
// every state word, over the same grid.  Copies
// of one pkt_id are normally identical (retransmissions), but the rule holds
// for any payloads.
constexpr uint32_t kRxI32MaxFrames = 0x7FFFFFFFu;
constexpr uint32_t kRxFixupBlocks = 128;   // k_rx_int32_fixup's grid
// The header words of an INT32 slice's state, as offsets from state + B.
constexpr uint32_t kRxCall = 0, kRxTotal = 1, kRxConflicts = 2, kRxListed = 3, kRxArrivals = 4, kRxLastListed = 5,
                   kRxList = 6;

__host__ __device__ constexpr int rx_int32_slices(int P) { return P / 256 > 4 ? P / 256 : 4; }

__device__ __forceinline__ unsigned long long rx_int32_tag(uint32_t call, uint64_t f) {
    return ((unsigned long long)(0xFFFFFFFFu - call) << 32) | ((unsigned long long)(kRxI32MaxFrames - (uint32_t)f) << 1);
}

// A wave takes F = U * 256 / P consecutive frames per tile (4 frames at
// P = 256): every lane loads one of the tile's F headers (lane l < F's is
// the one used) and its 16-byte payload chunks; lane l < F then makes frame
// l's claim, and the decision and the pkt_id are shuffled to the lanes
// holding that frame's chunks.  Software-pipelined: the next tile's header
// and payload loads are issued before this tile's claim, so a wave waits on
// one round trip per tile (the claim's, with the next loads under it) rather
// than two in series (loads, then the claim).
template <int P>
struct RxI32Tile {
    static constexpr int kU = rx_int32_slices(P);
    u3a hv;
    u4a w[kU];
};

template <int P>
__device__ __forceinline__ void rx_int32_load(const RxArgs& a, uint64_t t, int lane, RxI32Tile<P>& r) {
    constexpr int kU = RxI32Tile<P>::kU;
    constexpr int kChunksPerFrame = P / 4;
    constexpr int kF = kU * kWave / kChunksPerFrame;
    const uint64_t f0 = t * kF;
    // header first (the claim needs it first); indices clamped into the call
    // so every load is unconditional and in flight at once
    uint64_t fh = f0 + (uint64_t)(lane % kF);
    fh = fh < a.nframes ? fh : a.nframes - 1;
    r.hv = *reinterpret_cast<const u3a*>(a.frames + fh * a.stride + 4 * wire::kDwJob);
#pragma unroll
    for (int u = 0; u < kU; u++) {
        const int c = u * kWave + lane;
        uint64_t f = f0 + c / kChunksPerFrame;
        f = f < a.nframes ? f : a.nframes - 1;
        r.w[u] = __builtin_nontemporal_load(reinterpret_cast<const u4a*>(
            a.frames + f * a.stride + wire::kHeaderBytes + 16ull * (c % kChunksPerFrame)));
    }
}

template <int P, bool NT>
__global__ __launch_bounds__(kBlockThreads) void k_rx_int32(RxArgs a) {
    constexpr int kU = RxI32Tile<P>::kU;
    constexpr int kChunksPerFrame = P / 4;
    constexpr int kF = kU * kWave / kChunksPerFrame;          // frames per tile
    static_assert(kF >= 1 && kF <= kWave, "frames per tile");
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t ntiles = (a.nframes + kF - 1) / kF;
    unsigned long long* const hdr = a.state + a.nblocks;
    const uint32_t call = (uint32_t)hdr[kRxCall];
    uint32_t disc = 0;
    uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index();
    RxI32Tile<P> cur, nxt;
    if (t < ntiles) rx_int32_load<P>(a, t, lane, cur);
    for (; t < ntiles; t += nwaves) {
        const uint64_t tn = t + nwaves;
        if (tn < ntiles) rx_int32_load<P>(a, tn, lane, nxt);
        const uint64_t f0 = t * kF;
        // lane l < kF: the claim of frame f0 + l
        bool write = false;
        uint32_t pid = wire::pkt_id(cur.hv.y);
        if (lane < kF && f0 + lane < a.nframes) {
            const uint64_t f = f0 + lane;
            const bool ok = rx_accepts(a, cur.hv.x, cur.hv.y, a.nblocks);
            bool keep = false;
            if (ok) {
                const unsigned long long tag = rx_int32_tag(call, f);
                const unsigned long long old = atomicMax(a.state + pid, tag);
                if (old == 0ull) {
                    write = true;
                    keep = true;
                } else if ((old & ~1ull) < tag) {
                    write = true;
                    atomicAdd(hdr + kRxConflicts, 1ull);
                    if (!(atomicOr(a.state + pid, 1ull) & 1ull)) {   // this claim made it dirty: list it
                        const unsigned long long i = atomicAdd(hdr + kRxListed, 1ull);
                        if (i < a.nblocks) hdr[kRxList + i] = pid;
                    }
                }
            }
            if (!keep) disc++;
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int c = u * kWave + lane;
            const int src = c / kChunksPerFrame;
            const bool wr = __shfl(write ? 1 : 0, src) != 0;
            const uint64_t k = (uint32_t)__shfl((int)pid, src);
            if (!wr) continue;
            const uint64_t off = k * P + 4ull * (c % kChunksPerFrame);
            if (off >= a.numel) continue;
            const u4a& w = cur.w[u];
            const f4 o = __builtin_bit_cast(f4, mku4(bswap(w.x), bswap(w.y), bswap(w.z), bswap(w.w)));
            float* p = static_cast<float*>(a.out) + off;
            if (a.numel - off >= 4 && ((uintptr_t)p & 15u) == 0) {
                // a wave's F frames land anywhere in the output (their pkt_ids),
                // so not SML_NT_STORE16: its buffer resource spans +-1 GiB
                // around the first lane's address
                if constexpr (NT) SML_NT_STORE16_UNALIGNED(o, reinterpret_cast<f4*>(p));
                else *reinterpret_cast<f4*>(p) = o;
            }
            else store4_guarded(p, o, 0, a.numel - off);
        }
        cur = nxt;
    }
    if (!a.counts) return;
    __shared__ uint32_t bdisc[1];
    tally_init(bdisc);
    tally_add(bdisc[0], disc);
    tally_flush_accepted(bdisc, a.counts, a.nframes);
}

// Rewrite dirty pkt_id k from the frame its tag names (the first copy), the
// whole wave lane-strided over the block's words.
__device__ __forceinline__ void rx_int32_rewrite(const RxArgs& a, uint32_t P, uint64_t k, unsigned long long s,
                                                 int lane) {
    const uint64_t f = kRxI32MaxFrames - ((uint32_t)s >> 1);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.frames + f * a.stride + wire::kHeaderBytes);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.out) + k * P;
    const uint64_t valid = a.numel - k * P < P ? a.numel - k * P : P;
    for (uint64_t i = lane; i < valid; i += kWave) dst[i] = bswap(src[i]);
}

// kRxFixupBlocks workgroups, after k_rx_int32 on the same stream.  Every
// workgroup reads the call's sequence c, conflict count n and list length at
// its start; with conflicts (n != 0) it takes its share of the dirty pkt_ids,
// each rewritten from the frame its tag names (the first copy) and cleaned.
// Then it draws a ticket from the arrivals word, and the workgroup that draws
// the launch's last one runs the epilogue: the slice's total accumulates, the
// list length is kept as a statistic, the call's two counters are cleared and
// c advances.  Without conflicts that is all a launch does.
//
// The ticket is one relaxed agent-scope atomic per workgroup, with no release
// or acquire fence, because it hands no data over: the last arriver reads
// nothing that another workgroup of this launch wrote.  What it orders is
// only that the epilogue's stores come after every workgroup's reads of c, n
// and the list length, and they do: those reads precede the workgroup's own
// ticket in program order (the work branches on them, and the barrier before
// the ticket has every wave past that work), and the epilogue follows the
// last ticket.  The next call sees the epilogue's stores by stream order.
// The arrivals word only ever grows, kRxFixupBlocks per launch, so nothing
// has to reset it between calls.
__global__ __launch_bounds__(kBlockThreads) void k_rx_int32_fixup(RxArgs a, uint32_t P) {
    unsigned long long* const hdr = a.state + a.nblocks;
    const unsigned long long call = hdr[kRxCall];
    const unsigned long long n = hdr[kRxConflicts];
    const unsigned long long listed = hdr[kRxListed];
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index();
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    if (n && listed <= a.nblocks) {
        // the dirty list, one pkt_id per wave at a time; the wave that finds
        // the bit set rewrites the block, then cleans the bit (an id listed
        // twice is rewritten twice with the same words, or found clean)
        for (uint64_t i = wave; i < listed; i += nwaves) {
            const uint64_t k = hdr[kRxList + i];
            const unsigned long long s = a.state[k];
            if (s & 1ull) {
                rx_int32_rewrite(a, P, k, s, lane);
                if (lane == 0) a.state[k] = s & ~1ull;
            }
        }
    } else if (n) {
        // the list overflowed: every state word, 64 per wave at a time; the
        // dirty ones (a ballot) rewritten one after another by the whole wave
        for (uint64_t k0 = wave * kWave; k0 < a.nblocks; k0 += nwaves * kWave) {
            const uint64_t k = k0 + lane;
            const unsigned long long s = k < a.nblocks ? a.state[k] : 0ull;
            unsigned long long dirty = __ballot((s & 1ull) != 0);
            while (dirty) {
                const int j = __builtin_ctzll(dirty);
                dirty &= dirty - 1;
                const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)s, j);
                rx_int32_rewrite(a, P, k0 + j, lo, lane);
            }
            if (s & 1ull) a.state[k] = s & ~1ull;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long ticket =
        __hip_atomic_fetch_add(hdr + kRxArrivals, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket % kRxFixupBlocks != kRxFixupBlocks - 1) return;
    if (n) hdr[kRxTotal] += n;
    hdr[kRxLastListed] = listed;
    hdr[kRxConflicts] = 0ull;
    hdr[kRxListed] = 0ull;
    hdr[kRxCall] = call + 1;
}

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_frame_bytes(uint32_t packet_numel) { return wire::frame_bytes(packet_numel); }

uint64_t sml_rx_state_words(uint64_t numel, uint32_t packet_numel, uint32_t batch_max, int int32) {
    if (!valid_packet(packet_numel)) return 0;
    const uint64_t B = sml_num_blocks(numel, packet_numel);
    if (int32) return 2 * B + kRxList;   // claim words, header words, dirty list (k_rx_int32)
    const uint64_t w = B + (B < batch_max ? B : batch_max);
    return w ? w : 1;
}

}  // extern "C"

namespace sml {

// FrameArgs of one slice's frames: geometry, pool indices and the constant
// header dwords.
static void frame_args(const sml_frame_params* prm, uint64_t numel, uint32_t P, uint16_t W, uint64_t b,
                       void* frames, uint64_t stride, FrameArgs& a) {
    a.xcd = g_xcd_chunk.load(std::memory_order_relaxed);
    a.numel = numel;
    a.nblocks = sml_num_blocks(numel, P);
    a.ntiles = (a.nblocks * P + kTileElems - 1) / kTileElems;
    a.b = b;
    a.gexp = nullptr;
    a.frames = static_cast<uint8_t*>(frames);
    a.stride = stride;
    a.W = W;
    a.pool_start = prm->pool_index_start;
    a.pool_shift = prm->pool_index_shift;
    a.mop = prm->max_outstanding_pkts ? prm->max_outstanding_pkts : 1;
    wire::worker_header(*prm, P, a.hdr);
}

// Payload store policy: non-temporal for a frame set in device memory from
// the threshold on (written once, handed on); host frames (a NIC's pinned
// mbufs) keep the default policy.
static bool frames_nt(const void* frames, uint64_t bytes) {
    if (!nt_from(bytes)) return false;
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, frames) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return pa.type == hipMemoryTypeDevice;
}

// The frame set of every frame entry point: present, 4-byte aligned, frames
// of P elements at a 4-byte multiple stride.
static sml_status_t check_frames(const void* frames, uint64_t stride, uint32_t P) {
    if (!frames) return SML_ERR_INVALID_ARG;
    if (!wire::frame_set_fits(frames, stride, P)) return SML_ERR_ALIGNMENT;
    return SML_OK;
}

// The fields the two receive entry points share; b, exps, out, W and xcd are
// the caller's.
static RxArgs rx_args(const void* frames, uint64_t num_frames, uint64_t stride, uint64_t numel, uint32_t P,
                      uint64_t job_id, uint64_t* d_state, uint64_t* d_counts) {
    RxArgs a;
    a.frames = static_cast<const uint8_t*>(frames);
    a.nframes = num_frames;
    a.stride = stride;
    a.numel = numel;
    a.nblocks = sml_num_blocks(numel, P);
    a.state = reinterpret_cast<unsigned long long*>(d_state);
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.job = (uint8_t)job_id;
    return a;
}

// The transmit side of a float slice of any type (the two entry points
// below): d_in holds FLOAT32 elements (4-byte aligned) or, through the typed
// entry point, FLOAT16 / BFLOAT16 ones (2-byte aligned).  Every check comes
// before the launch.
static sml_status_t quantize_frames(const void* d_in, sml_data_type_t dt, uint64_t numel, uint32_t P, uint16_t W,
                                    const int8_t* d_global_exps, uint32_t batch_max, const sml_frame_params* prm,
                                    void* frames, uint64_t stride, void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (W == 0 || !prm || batch_max == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    const uintptr_t align = dt == SML_FLOAT32 ? 3u : 1u;
    if (!d_in || ((uintptr_t)d_in & align)) return SML_ERR_INVALID_ARG;
    if (const sml_status_t s = check_frames(frames, stride, P); s != SML_OK) return s;
    FrameArgs a;
    const uint64_t B = sml_num_blocks(numel, P);
    frame_args(prm, numel, P, W, B < batch_max ? B : batch_max, frames, stride, a);
    a.in = d_in;
    a.gexp = d_global_exps;
    dim3 grid(grid_for_tiles(a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const bool nts = frames_nt(frames, (a.nblocks + a.b) * stride);
    if (dt != SML_FLOAT32) {
        launch_quantize_frames_h(a, dt == SML_FLOAT16, P, d_global_exps != nullptr, nts, grid, st);
        return launch_check();
    }
    const bool al = aligned16(d_in);
    dispatch_packet(P, [&](auto Pc) {
        dispatch_bools([&](auto AL, auto GLOBAL, auto NTS) {
            k_quantize_frames<Pc(), ElemF32<AL()>, GLOBAL(), NTS(), false><<<grid, kBlockThreads, 0, st>>>(a);
        }, al, d_global_exps != nullptr, nts);
    });
    return launch_check();
}

// The receive side likewise: the claim pass sees no element; the apply pass
// writes d_out as FLOAT32 (4-byte aligned) or as a 16-bit type (2-byte
// aligned), with the store policy chosen by the output's bytes.
static sml_status_t dequantize_frames(const void* frames, uint64_t num_frames, uint64_t stride, uint64_t numel,
                                      uint32_t P, uint16_t W, uint32_t batch_max, uint64_t job_id, int8_t* d_exps,
                                      uint64_t* d_state, void* d_out, sml_data_type_t dt, uint64_t* d_counts,
                                      void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (W == 0 || batch_max == 0) return SML_ERR_INVALID_ARG;
    if (num_frames == 0) return SML_OK;
    if (num_frames >= 0xFFFFFFFEull) return SML_ERR_UNSUPPORTED;
    if (!d_state || (numel && (!d_exps || !d_out))) return SML_ERR_INVALID_ARG;
    if (const sml_status_t s = check_frames(frames, stride, P); s != SML_OK) return s;
    const uint64_t elem = dt == SML_FLOAT32 ? 4 : 2;
    if ((uintptr_t)d_out & (elem - 1)) return SML_ERR_ALIGNMENT;
    if (!aligned8(d_state) || !aligned8(d_counts)) return SML_ERR_ALIGNMENT;
    RxArgs a = rx_args(frames, num_frames, stride, numel, P, job_id, d_state, d_counts);
    const uint32_t U = (uint32_t)rx_slices((int)P);
    a.xcd = xcd_chunk_for(U);
    a.b = a.nblocks < batch_max ? a.nblocks : batch_max;
    a.exps = d_exps;
    a.out = d_out;
    a.W = W;
    hipStream_t st = (hipStream_t)stream;
    k_rx_claim<<<grid_for_vec(num_frames), kBlockThreads, 0, st>>>(a);
    const uint64_t tile = (uint64_t)U * kWave * 4;
    const uint64_t ntiles = (a.nblocks * P + tile - 1) / tile;
    if (ntiles) {
        const dim3 grid(grid_for_tiles(ntiles));
        // the output takes non-temporal stores from the threshold on, as K4's
        const bool nt = nt_from(elem * numel);
        if (dt != SML_FLOAT32) {
            launch_rx_apply_h(a, dt == SML_FLOAT16, P, nt, grid, st);
        } else {
            dispatch_packet(P, [&](auto Pc) {
                dispatch_bools([&](auto NT) { k_rx_apply<Pc(), ElemF32<true>, NT()><<<grid, kBlockThreads, 0, st>>>(a); },
                               nt);
            });
        }
    }
    return launch_check();
}

}  // namespace sml

extern "C" {

sml_status_t sml_quantize_pack_frames(const float* d_in, uint64_t numel, uint32_t P, uint16_t W,
                                      const int8_t* d_global_exps, uint32_t batch_max,
                                      const sml_frame_params* prm, void* frames, uint64_t stride, void* stream) {
    return quantize_frames(d_in, SML_FLOAT32, numel, P, W, d_global_exps, batch_max, prm, frames, stride, stream);
}

sml_status_t sml_quantize_pack_frames_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel, uint32_t P,
                                            uint16_t W, const int8_t* d_global_exps, uint32_t batch_max,
                                            const sml_frame_params* prm, void* frames, uint64_t stride,
                                            void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (data_type != SML_FLOAT32 && !is_half(data_type)) return SML_ERR_UNSUPPORTED;
    return quantize_frames(d_in, data_type, numel, P, W, d_global_exps, batch_max, prm, frames, stride, stream);
}

sml_status_t sml_pack_frames_int32(const int32_t* d_in, uint64_t numel, uint32_t P, const sml_frame_params* prm,
                                   void* frames, uint64_t stride, void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (!prm) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!d_in || !aligned4(d_in)) return SML_ERR_INVALID_ARG;
    if (const sml_status_t s = check_frames(frames, stride, P); s != SML_OK) return s;
    FrameArgs a;
    frame_args(prm, numel, P, 1, 0, frames, stride, a);       // INT32: no extra batch
    a.in = d_in;                                              // words moved as bits
    dim3 grid(grid_for_tiles(a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const bool nts = frames_nt(frames, a.nblocks * stride);
    dispatch_packet(P, [&](auto Pc) {
        dispatch_bools([&](auto AL, auto NTS) {
            // I32 exists only without global exponents: it has no scale
            k_quantize_frames<Pc(), ElemF32<AL()>, false, NTS(), true><<<grid, kBlockThreads, 0, st>>>(a);
        }, aligned16(d_in), nts);
    });
    return launch_check();
}

sml_status_t sml_dequantize_frames(const void* frames, uint64_t num_frames, uint64_t stride,
                                   uint64_t numel, uint32_t P, uint16_t W, uint32_t batch_max,
                                   uint64_t job_id, int8_t* d_exps, uint64_t* d_state, float* d_out,
                                   uint64_t* d_counts, void* stream) {
    return dequantize_frames(frames, num_frames, stride, numel, P, W, batch_max, job_id, d_exps, d_state, d_out,
                             SML_FLOAT32, d_counts, stream);
}

sml_status_t sml_dequantize_frames_typed(const void* frames, uint64_t num_frames, uint64_t stride, uint64_t numel,
                                         uint32_t P, uint16_t W, uint32_t batch_max, uint64_t job_id, int8_t* d_exps,
                                         uint64_t* d_state, void* d_out, sml_data_type_t data_type,
                                         uint64_t* d_counts, void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (data_type != SML_FLOAT32 && !is_half(data_type)) return SML_ERR_UNSUPPORTED;
    return dequantize_frames(frames, num_frames, stride, numel, P, W, batch_max, job_id, d_exps, d_state, d_out,
                             data_type, d_counts, stream);
}

sml_status_t sml_unpack_frames_int32(const void* frames, uint64_t num_frames, uint64_t stride, uint64_t numel,
                                     uint32_t P, uint64_t job_id, uint64_t* d_state, int32_t* d_out,
                                     uint64_t* d_counts, void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (num_frames == 0) return SML_OK;
    if (num_frames > kRxI32MaxFrames) return SML_ERR_UNSUPPORTED;
    if (!d_state || (numel && !d_out)) return SML_ERR_INVALID_ARG;
    if (const sml_status_t s = check_frames(frames, stride, P); s != SML_OK) return s;
    if (!aligned4(d_out)) return SML_ERR_ALIGNMENT;
    if (!aligned8(d_state) || !aligned8(d_counts)) return SML_ERR_ALIGNMENT;
    RxArgs a = rx_args(frames, num_frames, stride, numel, P, job_id, d_state, d_counts);
    a.xcd = g_xcd_chunk.load(std::memory_order_relaxed);
    a.b = 0;                                                  // INT32: no extra batch
    a.exps = nullptr;
    a.out = d_out;                                            // words stored as bits
    a.W = 1;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t frames_per_tile = (uint64_t)rx_int32_slices((int)P) * kWave * 4 / P;
    const dim3 grid(grid_for_tiles((num_frames + frames_per_tile - 1) / frames_per_tile));
    dispatch_packet(P, [&](auto Pc) {
        dispatch_bools([&](auto NT) { k_rx_int32<Pc(), NT()><<<grid, kBlockThreads, 0, st>>>(a); },
                       nt_from(4 * numel));
    });
    // a grid that spreads a call's dirty pkt_ids over the chip; with no
    // conflict its workgroups read two words and end
    k_rx_int32_fixup<<<kRxFixupBlocks, kBlockThreads, 0, st>>>(a, P);
    return launch_check();
}

sml_status_t sml_rx_reset(uint64_t* d_state, uint64_t num_words, void* stream) {
    if (num_words == 0) return SML_OK;
    if (!d_state || !aligned8(d_state)) return SML_ERR_INVALID_ARG;
    return hip_check(hipMemsetAsync(d_state, 0, num_words * 8, (hipStream_t)stream));
}

}  // extern "C"
