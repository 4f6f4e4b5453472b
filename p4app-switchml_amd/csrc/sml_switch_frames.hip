// sml_switch_frames.hip — the switch's side of the DPDK frames on gfx950
// ("Switch side"): the Tofino pipeline's slot logic
// (p4/bitmap_checker.p4, p4/workers_counter.p4, p4/next_step_selector.p4,
// p4/udp_sender.p4) with the aggregation pinned on planes by K6
// (p4/processor.p4:48-54, p4/exponents.p4:48-54), over a batch of arrived
// frames per call and registers that persist in d_state.
//
// The pipeline is sequential per slot; a call makes it parallel with the
// claim-then-apply shape of the receive side (sml_frames.hip):
//   k_fs_claim    thread per frame: a 64-bit atomic on the (slot, worker) word
//                 keeps the pair's lowest-index frame and its set — the set the
//                 call handles for the pair (the other set's frames: DEFERRED).
//   k_fs_verdict  thread per frame: with the slot's <= 32 claim words and the
//                 registers as the call found them, a frame knows the whole
//                 history of its slot up to its own index — who contributed
//                 before it — hence its flag and its verdict.  The frame that
//                 is its slot's first lists the slot as touched.
//   k_fs_apply    wave per touched slot: the new contributors' payloads summed
//                 into (or written over) the slot's words, the exponents maxed,
//                 bitmap and count advanced, the claim words cleared.
//   k_fs_result   wave per input frame: it loads the frame's header dwords and
//                 its verdict, and on BROADCAST / RETRANSMIT writes
//                 udp_sender's frame from the slot's words (any other verdict:
//                 the wave ends there).
// Each launch reads only what an earlier launch on the stream (or an earlier
// call) wrote and no workgroup waits on another: within a launch every claim
// word, register and accumulator word has one writer (the wave of its slot)
// or is only read.
//
// d_state: [0] the touched-slot count; claim words uint64[S][32] (0 = none,
// else ~((frame << 1) | set), so atomicMax keeps the lowest frame); per
// (slot, set) bitmap, count and exponent pair (uint32 each); the touched list
// uint32[S]; the accumulators uint32[S][2][P] in host order.
//
// The wire on both sides of a call is below the switch: sml_frame_gather
// builds a call's input from the workers' tx frame sets ("ingress"), and
// sml_frame_switch_deliver replicates the results into one receive ring per
// worker ("egress").  The frame's layout is sml_frame_wire.h's.
#include "sml_frame_wire.h"

namespace sml {

constexpr uint32_t kFsMaxWorkers = SML_MAX_FRAME_SWITCH_WORKERS;
constexpr uint64_t kFsHead = 64;                   // bytes before the claim words

struct FsWorker {
    uint32_t mac_lo;        // mac[0..3], memory order
    uint32_t mac_hi_ck;     // mac[4..5] | IPv4 header checksum of a result to this worker << 16
    uint32_t ip;            // ip_be, memory order
};

struct FsArgs {
    const uint8_t* frames;
    uint64_t nframes;
    uint64_t stride;
    uint8_t* out;
    uint64_t out_stride;
    uint8_t* verdict;
    unsigned long long* counts;     // [5] or nullptr
    uint32_t* touched_count;
    unsigned long long* claims;     // [S][32]
    uint32_t* bitmap;               // [S][2]
    uint32_t* count;                // [S][2]
    uint32_t* exps;                 // [S][2]: wire::exp_pair
    uint32_t* touched;              // [S]
    uint32_t* acc;                  // [S][2][P]
    uint32_t S, W;
    uint32_t sw_mac_lo16;           // switch mac[0..1]
    uint32_t sw_mac_hi;             // switch mac[2..5]
    uint32_t sw_ip;
    uint32_t len_dw4;               // result dword kDwIpLen: IPv4 total length (BE), identification 0
    uint32_t udp_len_be;            // the result's UDP length as a 16-bit value in memory order
    FsWorker workers[kFsMaxWorkers];
};

// What the parser and the worker table make of frame f.
struct FsHdr {
    uint32_t w, s, v;
    bool ok;                        // a known worker and a slot of the pool
};

__device__ __forceinline__ FsHdr fs_header(const FsArgs& a, uint32_t d6, uint32_t d7, uint32_t d12) {
    const uint32_t ip = wire::src_ip(d6, d7);
    const uint32_t idx = wire::pool_index(d12);
    FsHdr h;
    h.w = kFsMaxWorkers;
    for (uint32_t u = 0; u < a.W; u++) h.w = (a.workers[u].ip == ip && h.w == kFsMaxWorkers) ? u : h.w;
    h.s = wire::pool_slot(idx);
    h.v = wire::pool_set(idx);
    h.ok = h.w < kFsMaxWorkers && h.s < a.S;
    return h;
}

__device__ __forceinline__ FsHdr fs_header(const FsArgs& a, uint64_t f) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a.frames + f * a.stride);
    const uint32_t d6 = p[wire::kDwSrcIp], d7 = p[wire::kDwDstIp], d12 = p[wire::kDwPool];
    return fs_header(a, d6, d7, d12);
}

// workers_counter.p4's register action, n times: 0 -> W - 1, else one down.
__device__ __forceinline__ uint32_t fs_count_after(uint32_t c, uint32_t n, uint32_t W) {
    for (uint32_t i = 0; i < n; i++) c = c == 0 ? W - 1 : c - 1;
    return c;
}

__device__ __forceinline__ unsigned long long fs_claim_word(uint64_t f, uint32_t v) {
    return ~(((unsigned long long)f << 1) | v);
}

// Pass 1: the (slot, worker) pair's lowest-index frame, with its set.
__global__ __launch_bounds__(kBlockThreads) void k_fs_claim(FsArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.touched_count = 0;      // this call's list starts empty
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t f = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; f < a.nframes; f += stride) {
        const FsHdr h = fs_header(a, f);
        if (h.ok) atomicMax(a.claims + (uint64_t)h.s * kFsMaxWorkers + h.w, fs_claim_word(f, h.v));
    }
}

// Pass 2: every frame's verdict from the registers as the call found them and
// its slot's claim words.  In the call, worker u touches slot s once as far as
// the registers go — at its claimed frame f_u, in its call set: there bit u of
// that set's bitmap is set and bit u of the other set's cleared, and if the
// bit was clear, u is a new contributor: the count steps.  Every later frame
// of u (same set) finds its bit set: a retransmission.  So the count that
// frame f sees is the call's starting count stepped once per new contributor
// of its set claimed below f.
__global__ __launch_bounds__(kBlockThreads) void k_fs_verdict(FsArgs a) {
    __shared__ uint32_t hist[5];                              // frames per verdict
    tally_init(hist);
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t f = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; f < a.nframes; f += stride) {
        const FsHdr h = fs_header(a, f);
        uint32_t verdict = SML_VERDICT_IGNORED;
        bool lists = false;
        if (h.ok) {
            const unsigned long long* cl = a.claims + (uint64_t)h.s * kFsMaxWorkers;
            const unsigned long long mine = ~cl[h.w];
            const uint32_t bm = a.bitmap[2 * h.s + h.v];
            const uint32_t c0 = a.count[2 * h.s + h.v];
            if ((uint32_t)(mine & 1ull) != h.v) {
                verdict = SML_VERDICT_DEFERRED;
            } else {
                uint32_t nbefore = 0;                  // new contributors of (s, v) claimed below f
                uint64_t first = ~0ull;                // the slot's lowest claimed frame
                for (uint32_t u = 0; u < a.W; u++) {
                    const unsigned long long c = cl[u];
                    if (c == 0ull) continue;
                    const uint64_t fu = (~c) >> 1;
                    first = fu < first ? fu : first;
                    if ((uint32_t)((~c) & 1ull) == h.v && !((bm >> u) & 1u) && fu < f) nbefore++;
                }
                const bool fresh = (mine >> 1) == f && !((bm >> h.w) & 1u);
                uint32_t flag = fs_count_after(c0, nbefore, a.W);
                if (a.W == 1) flag = fresh ? 1u : 0u;
                if (fresh) verdict = flag == 1u ? SML_VERDICT_BROADCAST : SML_VERDICT_CONSUMED;
                else verdict = flag == 0u ? SML_VERDICT_RETRANSMIT : SML_VERDICT_CONSUMED;
                lists = first == f;                    // once per touched slot
            }
            // a deferred frame can be its slot's first only if it is its pair's
            // first, and then it is not deferred: the list is complete
        }
        a.verdict[f] = (uint8_t)verdict;
        if (lists) a.touched[atomicAdd(a.touched_count, 1u)] = h.s;
        if (a.counts) tally_add(hist[verdict], 1u);
    }
    if (!a.counts) return;
    tally_flush(hist, a.counts);
}

__device__ __forceinline__ int fs_max_i8(uint32_t a, uint32_t b) {
    const int x = (int8_t)a, y = (int8_t)b;
    return x > y ? x : y;
}

// Pass 3, wave per touched slot: lane u < W holds worker u's claim.  Per set:
// the bitmap's bits move as the claims say; the new contributors (claimed in
// this set, bit clear at the start) are summed in.  A contributor that found
// the bitmap empty at its index WRITES (p4/processor.p4:99-102): whatever the
// slot held, and whatever was added below that index, is gone — the sum starts
// at the last such contributor (the first, for any stream that follows the
// protocol).
template <int P>
__global__ __launch_bounds__(kBlockThreads) void k_fs_apply(FsArgs a) {
    constexpr int kChunks = P / 4;                             // 16-byte chunks of a payload
    constexpr int kPer = (kChunks + kWave - 1) / kWave;        // chunks per lane
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    const uint32_t ntouched = *a.touched_count;
    for (uint32_t i = blockIdx.x * kWavesPerBlock + wave_index(); i < ntouched; i += nwaves) {
        const uint32_t s = a.touched[i];
        unsigned long long* const clp = a.claims + (uint64_t)s * kFsMaxWorkers;
        const unsigned long long c = lane < (int)kFsMaxWorkers ? clp[lane] : 0ull;
        const uint64_t fu = (~c) >> 1;
        const bool live = c != 0ull && fu < a.nframes;         // (a claim names a frame of this call)
        const uint32_t cs = (uint32_t)((~c) & 1ull);
        // exponent bytes of this lane's claimed frame
        uint32_t ed = 0;
        if (live) ed = wire::exp_pair(*reinterpret_cast<const uint32_t*>(a.frames + fu * a.stride + 4 * wire::kDwPool));
#pragma unroll 1
        for (uint32_t v = 0; v < 2; v++) {
            const uint32_t setmask = (uint32_t)__ballot(live && cs == v);
            const uint32_t clrmask = (uint32_t)__ballot(live && cs != v);
            if (!(setmask | clrmask)) continue;
            const uint32_t bm0 = a.bitmap[2 * s + v];
            const uint32_t c0 = a.count[2 * s + v];
            const bool contrib = live && cs == v && !((bm0 >> lane) & 1u);
            const uint32_t cmask = (uint32_t)__ballot(contrib);
            // the bitmap as this lane's claimed frame finds it
            uint32_t before = bm0;
            for (uint32_t x = 0; x < a.W; x++) {
                const uint64_t fx = shfl_u64(fu, (int)x);
                if (fx < fu) {
                    if ((setmask >> x) & 1u) before |= 1u << x;
                    if ((clrmask >> x) & 1u) before &= ~(1u << x);
                }
            }
            const bool writer = contrib && before == 0u;
            const uint32_t wmask = (uint32_t)__ballot(writer);
            uint64_t fw = 0;                                   // the last writer's frame
            for (uint32_t m = wmask; m; m &= m - 1) {
                const int j = __builtin_ctz(m);
                const uint64_t fj = shfl_u64(fu, j);
                fw = fj > fw ? fj : fw;
            }
            const bool eff = contrib && (wmask == 0u || fu >= fw);
            const uint32_t emask = (uint32_t)__ballot(eff);
            if (cmask) {
                // the contributors one after another (every lane takes part in
                // the shuffle that names the frame), a lane's chunks side by side
                uint32_t* const acc = a.acc + ((uint64_t)2 * s + v) * P;
                u4 sum[kPer];
#pragma unroll
                for (int k = 0; k < kPer; k++) {
                    const int ch = k * kWave + lane;
                    sum[k] = mku4(0u, 0u, 0u, 0u);
                    if (wmask == 0u && ch < kChunks) sum[k] = *reinterpret_cast<const u4*>(acc + 4 * ch);
                }
                for (uint32_t m = emask; m; m &= m - 1) {
                    const int j = __builtin_ctz(m);
                    const uint64_t fj = shfl_u64(fu, j);
                    const uint8_t* const pl = a.frames + fj * a.stride + wire::kHeaderBytes;
                    u4a w[kPer];
#pragma unroll
                    for (int k = 0; k < kPer; k++) {
                        const int ch = k * kWave + lane;
                        // a lane past the payload (P < 256) rereads chunk 0 and drops it
                        w[k] = __builtin_nontemporal_load(reinterpret_cast<const u4a*>(pl + 16 * (ch < kChunks ? ch : 0)));
                    }
#pragma unroll
                    for (int k = 0; k < kPer; k++) {
                        sum[k].x += bswap(w[k].x); sum[k].y += bswap(w[k].y);
                        sum[k].z += bswap(w[k].z); sum[k].w += bswap(w[k].w);
                    }
                }
#pragma unroll
                for (int k = 0; k < kPer; k++) {
                    const int ch = k * kWave + lane;
                    if (ch < kChunks) *reinterpret_cast<u4*>(acc + 4 * ch) = sum[k];
                }
                // exponents: signed int8 max, each byte on its own; -128 is the identity
                int e0 = eff ? (int)(int8_t)(ed & 0xffu) : -128;
                int e1 = eff ? (int)(int8_t)((ed >> 8) & 0xffu) : -128;
#pragma unroll
                for (int d = 1; d < (int)kFsMaxWorkers; d <<= 1) {
                    const int o0 = __shfl_xor(e0, d), o1 = __shfl_xor(e1, d);
                    e0 = o0 > e0 ? o0 : e0;
                    e1 = o1 > e1 ? o1 : e1;
                }
                if (lane == 0) {
                    if (wmask == 0u) {
                        const uint32_t old = a.exps[2 * s + v];
                        e0 = fs_max_i8(old & 0xffu, (uint32_t)e0 & 0xffu);
                        e1 = fs_max_i8((old >> 8) & 0xffu, (uint32_t)e1 & 0xffu);
                    }
                    a.exps[2 * s + v] = ((uint32_t)e0 & 0xffu) | (((uint32_t)e1 & 0xffu) << 8);
                }
            }
            if (lane == 0) {
                a.bitmap[2 * s + v] = (bm0 | setmask) & ~clrmask;
                a.count[2 * s + v] = fs_count_after(c0, (uint32_t)__builtin_popcount(cmask), a.W);
            }
        }
        if (lane < (int)kFsMaxWorkers && c != 0ull) clp[lane] = 0ull;   // the next call's claims start empty
    }
}

// Pass 4: udp_sender.p4's frame for every BROADCAST / RETRANSMIT verdict, a
// wave per input frame (a wave whose frame has no result ends after its header
// and verdict loads): the header lanes store the header (a dword each),
// every lane its 16-byte chunks of the slot's words, byte-swapped to wire
// order.  One frame per wave keeps the result frames' load-to-store chains
// (verdict, header, slot words) side by side instead of in series.
template <int P>
__global__ __launch_bounds__(kBlockThreads) void k_fs_result(FsArgs a) {
    constexpr int kChunks = P / 4;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t f = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); f < a.nframes; f += nwaves) {
        // the header goes out with the verdict, not behind it
        const uint32_t* in = reinterpret_cast<const uint32_t*>(a.frames + f * a.stride);
        const uint32_t d6 = in[wire::kDwSrcIp], d7 = in[wire::kDwDstIp], d8 = in[wire::kDwSrcPort],
                       d9 = in[wire::kDwUdpLen], d10 = in[wire::kDwJob], d11 = in[wire::kDwPktId],
                       d12 = in[wire::kDwPool];
        const uint32_t vd = a.verdict[f];
        if (vd != SML_VERDICT_BROADCAST && vd != SML_VERDICT_RETRANSMIT) continue;
        const FsHdr h = fs_header(a, d6, d7, d12);
        if (!h.ok) continue;                               // a verdict 1 / 2 is never an ignored frame's
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.w);
        const uint32_t sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(2 * h.s + h.v));
        const FsWorker wk = a.workers[w];
        const uint32_t ex = a.exps[sv];
        uint32_t dw = wk.mac_lo;                                // lane kDwDstMac
        dw = lane == wire::kDwMacs ? wire::result_macs(wk.mac_hi_ck, a.sw_mac_lo16) : dw;
        dw = lane == wire::kDwSrcMac ? a.sw_mac_hi : dw;
        dw = lane == wire::kDwEthIp ? wire::kResultEthIp : dw;
        dw = lane == wire::kDwIpLen ? a.len_dw4 : dw;
        dw = lane == wire::kDwIpTtl ? wire::kResultIpTtl : dw;
        dw = lane == wire::kDwSrcIp ? wire::result_src_ip(wk.mac_hi_ck >> 16, a.sw_ip) : dw;
        dw = lane == wire::kDwDstIp ? wire::result_dst_ip(a.sw_ip, wk.ip) : dw;
        dw = lane == wire::kDwSrcPort ? wire::result_src_port(wk.ip, d9) : dw;
        dw = lane == wire::kDwUdpLen ? wire::result_udp_len(d8, a.udp_len_be) : dw;
        dw = lane == wire::kDwJob ? wire::result_job(d10) : dw;
        dw = lane == wire::kDwPktId ? d11 : dw;                 // tsi
        dw = lane == wire::kDwPool ? wire::result_pool(d12, ex) : dw;
        uint8_t* const o = a.out + f * a.out_stride;
        if (lane < wire::kHeaderDwords) reinterpret_cast<uint32_t*>(o)[lane] = dw;
        const uint32_t* const acc = a.acc + (uint64_t)sv * P;
        for (int ch = lane; ch < kChunks; ch += kWave) {
            const u4 q = *reinterpret_cast<const u4*>(acc + 4 * ch);
            *reinterpret_cast<u4a*>(o + wire::kHeaderBytes + 16 * ch) = u4a{bswap(q.x), bswap(q.y), bswap(q.z), bswap(q.w)};
        }
    }
}

// The pieces of d_state.
struct FsLayout {
    uint64_t claims, bitmap, count, exps, touched, acc, total;
};

static bool fs_layout(uint32_t S, uint32_t P, FsLayout& l) {
    if (!valid_packet(P) || S == 0 || S > SML_MAX_FRAME_SWITCH_SLOTS) return false;
    l.claims = kFsHead;
    l.bitmap = l.claims + 8ull * kFsMaxWorkers * S;
    l.count = l.bitmap + 8ull * S;
    l.exps = l.count + 8ull * S;
    l.touched = l.exps + 8ull * S;
    l.acc = (l.touched + 4ull * S + 15) & ~15ull;
    l.total = l.acc + 8ull * S * P;
    return true;
}

// The worker table of FsArgs / FdArgs: MAC, address and the IPv4 header
// checksum of a result frame to each worker.
static void fs_worker_table(const sml_frame_switch_params& prm, FsWorker* tbl) {
    const uint32_t total_len = wire::ipv4_total_len(prm.packet_numel);
    for (uint32_t u = 0; u < prm.num_workers; u++) {
        const sml_switch_worker& wk = prm.workers[u];
        memcpy(&tbl[u].mac_lo, wk.mac, 4);
        tbl[u].mac_hi_ck = (uint32_t)wk.mac[4] | ((uint32_t)wk.mac[5] << 8) |
                           (wire::result_ipv4_checksum(total_len, prm.switch_ip_be, wk.ip_be) << 16);
        tbl[u].ip = wk.ip_be;
    }
}

// ------------------------------------------------------------------ egress
// sml_frame_switch_deliver: the multicast group of next_step_selector.p4 and
// udp_sender.p4's per-port rewrite, into one receive ring per worker.  The
// position of a copy in its ring is a per-worker exclusive prefix count over
// the call's frames — a grid-wide dependency, taken in three launches:
//   k_fd_count  thread per frame: the set of workers that get a copy (verdict,
//               the asker's address for a RETRANSMIT, the drop mask) goes to
//               masks[f]; a wave ballot per worker counts the copies of the
//               wave's kFdGroup frames into counts[u][group].
//   k_fd_scan   workgroup per worker: its row of group counts becomes the
//               exclusive prefix, kFdScanTile groups a step with a carry; the
//               ring count as the call found it is kept in base[u] and
//               d_ring_count[u] advances; delivered / overflow are counted.
//   k_fd_copy   wave per input frame: the masks of the frames below it in its
//               group give, with a ballot per copy, the position; the frame is
//               read once and stored once per copy, a BROADCAST's destination
//               MAC, address and checksum replaced from the worker table.
// No workgroup waits on another and no atomic decides a position: every ring
// position, count word and prefix word has one writer per launch.
constexpr int kFdGroup = kWave;                              // frames per count group
constexpr int kFdScanPer = 4;                                // groups per scan thread
constexpr int kFdScanTile = kBlockThreads * kFdScanPer;      // groups per scan step
constexpr uint64_t kFdHead = 8 * kFsMaxWorkers;              // scratch bytes before the masks

struct FdArgs {
    const uint8_t* out;             // sml_frame_switch's out_frames
    uint64_t nframes;
    uint64_t out_stride;
    const uint8_t* verdict;
    const uint32_t* drop;           // nullable
    uint8_t* rings;
    uint64_t ring_bytes, ring_frames, rx_stride;
    unsigned long long* ring_count; // [W]
    unsigned long long* counts;     // [4] or nullptr
    unsigned long long* base;       // scratch [32]: ring_count as the call found it
    uint32_t* masks;                // scratch [nframes]: bit u = worker u gets a copy
    uint32_t* prefix;               // scratch [W][group_stride]: counts, then their exclusive prefix
    uint64_t ngroups;               // ceil(nframes / kFdGroup)
    uint64_t group_stride;
    uint32_t W;
    FsWorker workers[kFsMaxWorkers];
};

// Pass 1.  Workgroup b takes frames [256 b, 256 b + 256): a wave's frames are
// one group.
__global__ __launch_bounds__(kBlockThreads) void k_fd_count(FdArgs a) {
    __shared__ uint32_t lost[2];                               // dropped, unroutable
    tally_init(lost);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t all = 0xffffffffu >> (32 - a.W);
    const uint64_t nblocks = (a.nframes + kBlockThreads - 1) / kBlockThreads;
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t f = b * kBlockThreads + threadIdx.x;
        uint32_t mask = 0, dropped = 0;
        bool unroutable = false;
        if (f < a.nframes) {
            const uint32_t vd = a.verdict[f];
            if (vd == SML_VERDICT_BROADCAST) {
                mask = all;
            } else if (vd == SML_VERDICT_RETRANSMIT) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(a.out + f * a.out_stride);
                const uint32_t ip = wire::dst_ip(p[wire::kDwDstIp], p[wire::kDwSrcPort]);
                for (uint32_t u = 0; u < a.W; u++) mask = (a.workers[u].ip == ip && mask == 0u) ? 1u << u : mask;
                unroutable = mask == 0u;
            }
            const uint32_t dm = (a.drop && mask) ? a.drop[f] : 0u;
            dropped = (uint32_t)__builtin_popcount(mask & dm);
            mask &= ~dm;
            a.masks[f] = mask;
        }
        uint32_t mine = 0;                                     // lane u: worker u's copies in this group
        for (uint32_t u = 0; u < a.W; u++) {
            const uint32_t c = (uint32_t)__builtin_popcountll(__ballot((mask >> u) & 1u));
            mine = lane == u ? c : mine;
        }
        const uint64_t g = b * kWavesPerBlock + wave_index();
        if (lane < a.W && g < a.ngroups) a.prefix[lane * a.group_stride + g] = mine;
        if (a.counts) {
            tally_add(lost[0], dropped);
            tally_add(lost[1], unroutable ? 1u : 0u);
        }
    }
    if (!a.counts) return;
    tally_flush(lost, a.counts, 1, 2);                         // counts[1], counts[3]
}

// Pass 2, workgroup u: worker u's group counts -> their exclusive prefix, in
// place; then the ring's count moves on.
__global__ __launch_bounds__(kBlockThreads) void k_fd_scan(FdArgs a) {
    __shared__ uint32_t wtot[kWavesPerBlock];
    const uint32_t u = blockIdx.x;
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    uint32_t* const row = a.prefix + (uint64_t)u * a.group_stride;
    uint32_t carry = 0;
    for (uint64_t t0 = 0; t0 < a.ngroups; t0 += kFdScanTile) {
        const uint64_t g0 = t0 + (uint64_t)threadIdx.x * kFdScanPer;
        uint32_t c[kFdScanPer], s = 0;
#pragma unroll
        for (int k = 0; k < kFdScanPer; k++) {
            c[k] = g0 + k < a.ngroups ? row[g0 + k] : 0u;
            s += c[k];
        }
        uint32_t inc = s;                                      // inclusive over the wave's threads
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
            inc += (int)lane >= d ? o : 0u;
        }
        if (lane == kWave - 1) wtot[wv] = inc;
        __syncthreads();
        uint32_t x = carry + inc - s, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kWavesPerBlock; w++) {
            x += w < wv ? wtot[w] : 0u;
            total += wtot[w];
        }
#pragma unroll
        for (int k = 0; k < kFdScanPer; k++) {
            if (g0 + k < a.ngroups) row[g0 + k] = x;
            x += c[k];
        }
        carry += total;
        __syncthreads();                                       // wtot is the next step's too
    }
    if (threadIdx.x == 0) {
        const uint64_t old = a.ring_count[u], end = old + carry;
        const uint64_t over = old >= a.ring_frames ? carry : end > a.ring_frames ? end - a.ring_frames : 0;
        a.base[u] = old;
        a.ring_count[u] = end < a.ring_frames ? end : a.ring_frames;
        if (a.counts) {
            if (carry - over) atomicAdd(a.counts + 0, (unsigned long long)(carry - over));
            if (over) atomicAdd(a.counts + 2, (unsigned long long)over);
        }
    }
}

// Pass 3, wave per input frame, held in a FrameRegs (sml_frame_wire.h) (a wave whose frame has no copy ends after its
// group's mask load).
template <int P>
__global__ __launch_bounds__(kBlockThreads) void k_fd_copy(FdArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t f = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); f < a.nframes; f += nwaves) {
        const uint64_t g = f / kFdGroup, f0 = g * kFdGroup;
        const uint32_t at = (uint32_t)(f - f0);
        const uint32_t m = f0 + lane < a.nframes ? a.masks[f0 + lane] : 0u;
        const uint32_t own = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)at);
        if (own == 0u) continue;
        const uint32_t below = (uint32_t)lane < at ? m : 0u;   // the group's frames before this one
        const bool bcast = a.verdict[f] == SML_VERDICT_BROADCAST;
        FrameRegs<P> fr;
        fr.load(a.out + f * a.out_stride, lane);
        for (uint32_t rest = own; rest; rest &= rest - 1) {
            const uint32_t u = (uint32_t)__builtin_ctz(rest);
            const uint64_t pos = a.base[u] + a.prefix[u * a.group_stride + g] +
                                 (uint64_t)__builtin_popcountll(__ballot((below >> u) & 1u));
            if (pos >= a.ring_frames) continue;                // overflow: counted by the scan
            uint32_t dw = fr.dw;
            if (bcast) {                                       // RETRANSMIT: the asker's frame as it is
                const FsWorker wk = a.workers[u];
                dw = lane == wire::kDwDstMac ? wk.mac_lo : dw;
                dw = lane == wire::kDwMacs ? wire::copy_macs(dw, wk.mac_hi_ck & 0xffffu) : dw;
                dw = lane == wire::kDwSrcIp ? wire::copy_checksum(dw, wk.mac_hi_ck >> 16) : dw;
                dw = lane == wire::kDwDstIp ? wire::copy_dst_ip_lo(dw, wk.ip) : dw;
                dw = lane == wire::kDwSrcPort ? wire::copy_dst_ip_hi(dw, wk.ip) : dw;
            }
            fr.store(a.rings + u * a.ring_bytes + pos * a.rx_stride, lane, dw);
        }
    }
}

// ----------------------------------------------------------------- ingress
// sml_frame_gather: a switch call's input from the workers' tx frame sets, a
// wave per output frame.
struct FgArgs {
    const uint8_t* sets[kFsMaxWorkers];
    uint32_t num_sets;
    uint64_t set_frames, set_stride;
    const uint32_t* set;
    const unsigned long long* index;
    uint64_t n;
    uint8_t* dst;
    uint64_t dst_stride;
    unsigned long long* skipped;    // nullable
};

template <int P>
__global__ __launch_bounds__(kBlockThreads) void k_fg_gather(FgArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); j < a.n; j += nwaves) {
        const uint32_t s = a.set[j];
        const uint64_t i = a.index[j];
        if (s >= a.num_sets || i >= a.set_frames) {
            if (lane == 0 && a.skipped) atomicAdd(a.skipped, 1ull);
            continue;
        }
        FrameRegs<P> fr;
        fr.load(a.sets[s] + i * a.set_stride, lane);
        fr.store(a.dst + j * a.dst_stride, lane, fr.dw);
    }
}

// The pieces of sml_frame_switch_deliver's d_scratch.
struct FdLayout {
    uint64_t masks, prefix, ngroups, group_stride, total;
};

static FdLayout fd_layout(uint64_t num_frames, uint32_t W) {
    FdLayout l;
    l.ngroups = (num_frames + kFdGroup - 1) / kFdGroup;
    l.group_stride = (l.ngroups + 3) & ~3ull;
    l.masks = kFdHead;
    l.prefix = (l.masks + 4 * num_frames + 15) & ~15ull;
    l.total = l.prefix + 4ull * W * l.group_stride;
    return l;
}

constexpr uint64_t kFdMaxFrames = 0x7fffffffull;               // positions and counts of a call fit 32 bits

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_frame_switch_state_bytes(uint32_t num_slots, uint32_t packet_numel) {
    FsLayout l;
    return fs_layout(num_slots, packet_numel, l) ? l.total : 0;
}

sml_status_t sml_frame_switch_reset(void* d_state, uint32_t num_slots, uint32_t packet_numel, void* stream) {
    if (!d_state) return SML_ERR_INVALID_ARG;
    FsLayout l;
    if (!fs_layout(num_slots, packet_numel, l)) return SML_ERR_UNSUPPORTED;
    if (!aligned8(d_state)) return SML_ERR_ALIGNMENT;
    // everything but the accumulators: a slot's words are written before they are read
    return hip_check(hipMemsetAsync(d_state, 0, l.acc, (hipStream_t)stream));
}

sml_status_t sml_frame_switch(const sml_frame_switch_params* prm, const void* frames, uint64_t num_frames,
                              uint64_t stride, void* d_state, void* out_frames, uint64_t out_stride,
                              uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (num_frames && (!frames || !d_state || !out_frames || !d_verdict)) return SML_ERR_INVALID_ARG;
    const uint32_t P = prm->packet_numel, S = prm->num_slots, W = prm->num_workers;
    FsLayout l;
    if (!fs_layout(S, P, l) || W > kFsMaxWorkers) return SML_ERR_UNSUPPORTED;
    if (num_frames == 0) return SML_OK;
    if (!wire::frame_set_fits(frames, stride, P)) return SML_ERR_ALIGNMENT;
    if (!wire::frame_set_fits(out_frames, out_stride, P)) return SML_ERR_ALIGNMENT;
    if (!aligned8(d_state) || !aligned8(d_counts)) return SML_ERR_ALIGNMENT;

    FsArgs a;
    memset(&a, 0, sizeof(a));
    uint8_t* const st8 = static_cast<uint8_t*>(d_state);
    a.frames = static_cast<const uint8_t*>(frames);
    a.nframes = num_frames;
    a.stride = stride;
    a.out = static_cast<uint8_t*>(out_frames);
    a.out_stride = out_stride;
    a.verdict = d_verdict;
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.touched_count = reinterpret_cast<uint32_t*>(st8);
    a.claims = reinterpret_cast<unsigned long long*>(st8 + l.claims);
    a.bitmap = reinterpret_cast<uint32_t*>(st8 + l.bitmap);
    a.count = reinterpret_cast<uint32_t*>(st8 + l.count);
    a.exps = reinterpret_cast<uint32_t*>(st8 + l.exps);
    a.touched = reinterpret_cast<uint32_t*>(st8 + l.touched);
    a.acc = reinterpret_cast<uint32_t*>(st8 + l.acc);
    a.S = S;
    a.W = W;
    a.sw_mac_lo16 = (uint32_t)prm->switch_mac[0] | ((uint32_t)prm->switch_mac[1] << 8);
    memcpy(&a.sw_mac_hi, prm->switch_mac + 2, 4);
    a.sw_ip = prm->switch_ip_be;
    a.len_dw4 = wire::be16(wire::ipv4_total_len(P));
    a.udp_len_be = wire::be16(wire::udp_len(P));
    fs_worker_table(*prm, a.workers);

    hipStream_t st = (hipStream_t)stream;
    const uint32_t gframes = grid_for_vec(num_frames);
    k_fs_claim<<<gframes, kBlockThreads, 0, st>>>(a);
    k_fs_verdict<<<gframes, kBlockThreads, 0, st>>>(a);
    // at most one touched slot per frame, and per slot of the pool
    const uint64_t slots = num_frames < S ? num_frames : S;
    const uint32_t gslots = grid_for_tiles(slots);
    const uint32_t gresult = grid_for_tiles(num_frames);
    dispatch_packet(P, [&](auto Pc) {
        k_fs_apply<Pc()><<<gslots, kBlockThreads, 0, st>>>(a);
        k_fs_result<Pc()><<<gresult, kBlockThreads, 0, st>>>(a);
    });
    return launch_check();
}

uint64_t sml_frame_switch_deliver_scratch_bytes(uint64_t num_frames, uint32_t num_workers) {
    if (num_workers == 0 || num_workers > kFsMaxWorkers || num_frames > kFdMaxFrames) return 0;
    return fd_layout(num_frames, num_workers).total;
}

sml_status_t sml_frame_switch_deliver(const sml_frame_switch_params* prm, const void* out_frames,
                                      uint64_t num_frames, uint64_t out_stride, const uint8_t* d_verdict,
                                      const uint32_t* d_drop, void* rings, uint64_t ring_bytes,
                                      uint64_t ring_frames, uint64_t rx_stride, uint64_t* d_ring_count,
                                      uint64_t* d_counts, void* d_scratch, void* stream) {
    if (!prm || prm->num_workers == 0) return SML_ERR_INVALID_ARG;
    if (num_frames && (!out_frames || !d_verdict || !rings || !d_ring_count || !d_scratch)) return SML_ERR_INVALID_ARG;
    const uint32_t P = prm->packet_numel, W = prm->num_workers;
    if (!valid_packet(P) || W > kFsMaxWorkers || ring_frames == 0 || num_frames > kFdMaxFrames)
        return SML_ERR_UNSUPPORTED;
    if (num_frames == 0) return SML_OK;
    if (!wire::frame_set_fits(out_frames, out_stride, P)) return SML_ERR_ALIGNMENT;
    if (!wire::frame_set_fits(rings, rx_stride, P) || ring_bytes % 4) return SML_ERR_ALIGNMENT;
    if (ring_frames > ~0ull / rx_stride || ring_bytes < ring_frames * rx_stride) return SML_ERR_ALIGNMENT;
    if (!aligned4(d_drop) || !aligned8(d_ring_count) || !aligned8(d_counts) || !aligned16(d_scratch))
        return SML_ERR_ALIGNMENT;

    const FdLayout l = fd_layout(num_frames, W);
    uint8_t* const sc8 = static_cast<uint8_t*>(d_scratch);
    FdArgs a;
    memset(&a, 0, sizeof(a));
    a.out = static_cast<const uint8_t*>(out_frames);
    a.nframes = num_frames;
    a.out_stride = out_stride;
    a.verdict = d_verdict;
    a.drop = d_drop;
    a.rings = static_cast<uint8_t*>(rings);
    a.ring_bytes = ring_bytes;
    a.ring_frames = ring_frames;
    a.rx_stride = rx_stride;
    a.ring_count = reinterpret_cast<unsigned long long*>(d_ring_count);
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.base = reinterpret_cast<unsigned long long*>(sc8);
    a.masks = reinterpret_cast<uint32_t*>(sc8 + l.masks);
    a.prefix = reinterpret_cast<uint32_t*>(sc8 + l.prefix);
    a.ngroups = l.ngroups;
    a.group_stride = l.group_stride;
    a.W = W;
    fs_worker_table(*prm, a.workers);

    hipStream_t st = (hipStream_t)stream;
    k_fd_count<<<grid_for_vec(num_frames), kBlockThreads, 0, st>>>(a);
    k_fd_scan<<<W, kBlockThreads, 0, st>>>(a);
    const uint32_t gcopy = grid_for_tiles(num_frames);
    dispatch_packet(P, [&](auto Pc) { k_fd_copy<Pc()><<<gcopy, kBlockThreads, 0, st>>>(a); });
    return launch_check();
}

sml_status_t sml_frame_gather(const void* const* sets, uint32_t num_sets, uint64_t set_frames, uint64_t set_stride,
                              const uint32_t* d_set, const uint64_t* d_index, uint64_t n, uint32_t packet_numel,
                              void* dst, uint64_t dst_stride, uint64_t* d_skipped, void* stream) {
    if (!sets || num_sets == 0) return SML_ERR_INVALID_ARG;
    if (n && (!d_set || !d_index || !dst)) return SML_ERR_INVALID_ARG;
    if (!valid_packet(packet_numel) || num_sets > kFsMaxWorkers) return SML_ERR_UNSUPPORTED;
    if (n == 0) return SML_OK;
    for (uint32_t s = 0; s < num_sets; s++)
        if (!sets[s]) return SML_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < num_sets; s++)
        if (!wire::frame_set_fits(sets[s], set_stride, packet_numel)) return SML_ERR_ALIGNMENT;
    if (!wire::frame_set_fits(dst, dst_stride, packet_numel)) return SML_ERR_ALIGNMENT;
    if (!aligned4(d_set) || !aligned8(d_index) || !aligned8(d_skipped)) return SML_ERR_ALIGNMENT;

    FgArgs a;
    memset(&a, 0, sizeof(a));
    for (uint32_t s = 0; s < num_sets; s++) a.sets[s] = static_cast<const uint8_t*>(sets[s]);
    a.num_sets = num_sets;
    a.set_frames = set_frames;
    a.set_stride = set_stride;
    a.set = d_set;
    a.index = reinterpret_cast<const unsigned long long*>(d_index);
    a.n = n;
    a.dst = static_cast<uint8_t*>(dst);
    a.dst_stride = dst_stride;
    a.skipped = reinterpret_cast<unsigned long long*>(d_skipped);
    const uint32_t grid = grid_for_tiles(n);
    dispatch_packet(packet_numel, [&](auto Pc) { k_fg_gather<Pc()><<<grid, kBlockThreads, 0, (hipStream_t)stream>>>(a); });
    return launch_check();
}

}  // extern "C"
