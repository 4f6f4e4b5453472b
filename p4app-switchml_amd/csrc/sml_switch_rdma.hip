// sml_switch_rdma.hip — the switch's side of the RDMA messages on gfx950
// ("Switch side"): the slot logic of sml_switch_frames.hip
// (p4/bitmap_checker.p4, p4/workers_counter.p4, p4/next_step_selector.p4) at
// message granularity, with p4/rdma_sender.p4's results, over a batch of
// completion records per call and registers that persist in d_state.
//
// What differs from the frame switch is the data movement.  A record is the
// parsed header the frame passes lack: 24 bytes, two wide loads, and neither
// claim nor verdict touches a payload.  A message is contiguous and 16-byte
// aligned, so is every result, and a result's place is named by its record
// (worker u's copy at rx + u * rx_bytes + addr), not prefix-counted.  So the
// sum never goes back to memory on its way out:
//   k_rs_claim    thread per record: a 64-bit atomic max on the (slot, worker)
//                 word keeps the pair's lowest-index record and its set.
//   k_rs_verdict  thread per record: the frame switch's rule over the slot's
//                 <= 32 claim words and the registers as the call found them.
//                 A BROADCAST / RETRANSMIT record pushes itself on its (slot,
//                 set)'s result list — the head in d_state, the link in the
//                 record's own d_out_imm word, which only such a record may
//                 write — and counts its dropped copies.  The slot's first
//                 record lists the slot as touched.
//   k_rs_apply    wave per touched slot: the new contributors' messages, up to
//                 kInFlight of them loaded before the first add, byte-swapped
//                 and summed in registers (or written over the slot from the
//                 contributor that found the bitmap empty), the exponents
//                 maxed across lanes, the registers advanced, the claim words
//                 cleared.  Then the slot's result list is walked: each record
//                 gets its immediate, and the sum goes from the registers,
//                 byte-swapped once, to every receive region the record names,
//                 16 bytes a lane with `sc1 nt` stores.  A slot touched
//                 without a result writes only its registers.
// A message over a wave: chunk k * 64 + lane, 16 bytes each — 4 per lane at
// 1024 words, one per lane at 256, the low 16 / 32 lanes at 64 / 128.  A slot
// keeps its wave at every size: lanes 0..31 are also the slot's workers (the
// ballots over the claims), which two slots in one wave would have to share.
//
// d_state: [0] the touched-slot count; claim words uint64[S][32] (0 = none,
// else ~((record << 1) | set)); per (slot, set) bitmap, count, exponent pair
// and result-list head (uint32 each; head 0 = empty, else record + 1); the
// touched list uint32[S]; the accumulators uint32[S][2][M] in host order.
#include "sml_host.h"

namespace sml {

constexpr uint32_t kRsMaxWorkers = SML_MAX_FRAME_SWITCH_WORKERS;
constexpr uint32_t kRsMaxSlots = SML_MAX_FRAME_SWITCH_SLOTS;
constexpr uint64_t kRsHead = 64;                   // bytes before the claim words
constexpr uint64_t kRsMaxRecords = 0x7fffffffull;  // a list head holds record + 1 in 32 bits
constexpr uint32_t kRsRecordBytes = sizeof(sml_rdma_arrival);
static_assert(kRsRecordBytes == 24 && offsetof(sml_rdma_arrival, addr) == 16, "two loads: 16 bytes, then 8");

struct RsArgs {
    const uint8_t* arrivals;
    uint64_t n;
    const uint8_t* landing;
    uint64_t landing_stride, landing_msgs;
    uint8_t* rx;
    uint64_t rx_bytes;
    uint64_t addr_max;              // the highest addr a result fits at
    const uint32_t* drop;           // nullable
    uint32_t* out_imm;
    uint8_t* verdict;
    unsigned long long* counts;     // [6] or nullptr
    uint32_t* touched_count;
    unsigned long long* claims;     // [S][32]
    uint32_t* bitmap;               // [S][2]
    uint32_t* count;                // [S][2]
    uint32_t* exps;                 // [S][2]: e0 | e1 << 8
    uint32_t* rhead;                // [S][2]: the result list
    uint32_t* touched;              // [S]
    uint32_t* acc;                  // [S][2][M]
    uint32_t S, W;
    uint32_t ppm_shift;             // log2(pkts_per_msg)
    uint32_t fits;                  // rx_bytes holds a message at all
};

// Record i as the passes see it.
struct RsRec {
    uint32_t w, s, v, imm, src;
    uint64_t addr;
    bool ok;                        // not IGNORED
};

__device__ __forceinline__ RsRec rs_record(const RsArgs& a, uint64_t i) {
    const uint8_t* p = a.arrivals + i * kRsRecordBytes;
    const u4a lo = *reinterpret_cast<const u4a*>(p);           // 8-byte aligned: one dwordx4
    const u2 hi = *reinterpret_cast<const u2*>(p + 16);
    RsRec r;
    r.w = lo.x;
    r.imm = lo.z;
    r.src = lo.w;
    r.addr = ((uint64_t)hi.y << 32) | hi.x;
    const uint32_t idx = lo.y >> 1;
    r.v = lo.y & 1u;
    r.s = idx >> a.ppm_shift;
    r.ok = (idx & ((1u << a.ppm_shift) - 1u)) == 0u && r.s < a.S && r.w < a.W && r.src < a.landing_msgs &&
           (r.addr & 15u) == 0u && a.fits && r.addr <= a.addr_max;
    return r;
}

// workers_counter.p4's register action, n times: 0 -> W - 1, else one down.
__device__ __forceinline__ uint32_t rs_count_after(uint32_t c, uint32_t n, uint32_t W) {
    for (uint32_t i = 0; i < n; i++) c = c == 0 ? W - 1 : c - 1;
    return c;
}

// Pass 1: the (slot, worker) pair's lowest-index record, with its set.
__global__ __launch_bounds__(kBlockThreads) void k_rs_claim(RsArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.touched_count = 0;      // this call's list starts empty
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const RsRec r = rs_record(a, i);
        if (r.ok) atomicMax(a.claims + (uint64_t)r.s * kRsMaxWorkers + r.w, ~(((unsigned long long)i << 1) | r.v));
    }
}

// Pass 2: every record's verdict, by k_fs_verdict's argument: in the call,
// worker u moves its slot's registers once, at its claimed record, so the count
// record i sees is the call's starting count stepped once per new contributor
// of its set claimed below i.
__global__ __launch_bounds__(kBlockThreads) void k_rs_verdict(RsArgs a) {
    __shared__ uint32_t hist[6];                              // records per verdict, dropped copies
    tally_init(hist);
    const uint32_t all = 0xffffffffu >> (32 - a.W);
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const RsRec r = rs_record(a, i);
        uint32_t verdict = SML_VERDICT_IGNORED, dropped = 0;
        bool lists = false;
        if (r.ok) {
            const unsigned long long* cl = a.claims + (uint64_t)r.s * kRsMaxWorkers;
            const unsigned long long mine = ~cl[r.w];
            const uint32_t bm = a.bitmap[2 * r.s + r.v];
            const uint32_t c0 = a.count[2 * r.s + r.v];
            if ((uint32_t)(mine & 1ull) != r.v) {
                verdict = SML_VERDICT_DEFERRED;
            } else {
                uint32_t nbefore = 0;                  // new contributors of (s, v) claimed below i
                uint64_t first = ~0ull;                // the slot's lowest claimed record
                for (uint32_t u = 0; u < a.W; u++) {
                    const unsigned long long c = cl[u];
                    if (c == 0ull) continue;
                    const uint64_t iu = (~c) >> 1;
                    first = iu < first ? iu : first;
                    if ((uint32_t)((~c) & 1ull) == r.v && !((bm >> u) & 1u) && iu < i) nbefore++;
                }
                const bool fresh = (mine >> 1) == i && !((bm >> r.w) & 1u);
                uint32_t flag = rs_count_after(c0, nbefore, a.W);
                if (a.W == 1) flag = fresh ? 1u : 0u;
                if (fresh) verdict = flag == 1u ? SML_VERDICT_BROADCAST : SML_VERDICT_CONSUMED;
                else verdict = flag == 0u ? SML_VERDICT_RETRANSMIT : SML_VERDICT_CONSUMED;
                lists = first == i;                    // once per touched slot
                if (verdict != SML_VERDICT_CONSUMED) {
                    // the slot's wave finds its result records here; out_imm[i] is the link until then
                    a.out_imm[i] = atomicExch(a.rhead + 2 * r.s + r.v, (uint32_t)i + 1u);
                    const uint32_t mask = verdict == SML_VERDICT_BROADCAST ? all : 1u << r.w;
                    dropped = (uint32_t)__builtin_popcount(mask & (a.drop ? a.drop[i] : 0u));
                }
            }
        }
        a.verdict[i] = (uint8_t)verdict;
        if (lists) a.touched[atomicAdd(a.touched_count, 1u)] = r.s;
        if (a.counts) {
            tally_add(hist[verdict], 1u);
            tally_add(hist[5], dropped);
        }
    }
    if (!a.counts) return;
    tally_flush(hist, a.counts);
}

__device__ __forceinline__ int rs_max_i8(uint32_t a, uint32_t b) {
    const int x = (int8_t)a, y = (int8_t)b;
    return x > y ? x : y;
}

__device__ __forceinline__ uint32_t rs_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Pass 3, wave per touched slot: lane u < W holds worker u's claim.  Per set,
// k_fs_apply's bookkeeping (who contributes, who writes over the slot), then
// the sum in registers, then the set's results from those registers.
template <int M>
__global__ __launch_bounds__(kBlockThreads) void k_rs_apply(RsArgs a) {
    constexpr int kChunks = M / 4;                             // 16-byte chunks of a message
    constexpr int kPer = (kChunks + kWave - 1) / kWave;        // chunks per lane
    constexpr int kInFlight = kPer == 4 ? 2 : 4;               // contributors loaded before the first add
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t all = 0xffffffffu >> (32 - a.W);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    const uint32_t ntouched = *a.touched_count;
    for (uint32_t t = blockIdx.x * kWavesPerBlock + wave_index(); t < ntouched; t += nwaves) {
        const uint32_t s = rs_uniform(a.touched[t]);
        unsigned long long* const clp = a.claims + (uint64_t)s * kRsMaxWorkers;
        const unsigned long long c = lane < (int)kRsMaxWorkers ? clp[lane] : 0ull;
        const uint64_t iu = (~c) >> 1;
        const bool live = c != 0ull && iu < a.n;               // (a claim names a record of this call)
        const uint32_t cs = (uint32_t)((~c) & 1ull);
        // this lane's claimed record: its exponent bytes and where its message landed
        uint32_t ed = 0, src = 0;
        if (live) {
            const u2 d = *reinterpret_cast<const u2*>(a.arrivals + iu * kRsRecordBytes + 8);
            ed = d.x >> 16;
            src = d.y;
        }
#pragma unroll 1
        for (uint32_t v = 0; v < 2; v++) {
            const uint32_t setmask = (uint32_t)__ballot(live && cs == v);
            const uint32_t clrmask = (uint32_t)__ballot(live && cs != v);
            if (!(setmask | clrmask)) continue;
            const uint32_t bm0 = a.bitmap[2 * s + v];
            const uint32_t c0 = a.count[2 * s + v];
            const bool contrib = live && cs == v && !((bm0 >> lane) & 1u);
            const uint32_t cmask = (uint32_t)__ballot(contrib);
            // the bitmap as this lane's claimed record finds it
            uint32_t before = bm0;
            for (uint32_t x = 0; x < a.W; x++) {
                const uint64_t ix = shfl_u64(iu, (int)x);
                if (ix < iu) {
                    if ((setmask >> x) & 1u) before |= 1u << x;
                    if ((clrmask >> x) & 1u) before &= ~(1u << x);
                }
            }
            const bool writer = contrib && before == 0u;
            const uint32_t wmask = (uint32_t)__ballot(writer);
            uint64_t iw = 0;                                   // the last writer's record
            for (uint32_t m = wmask; m; m &= m - 1) {
                const uint64_t ij = shfl_u64(iu, __builtin_ctz(m));
                iw = ij > iw ? ij : iw;
            }
            const bool eff = contrib && (wmask == 0u || iu >= iw);
            const uint32_t emask = (uint32_t)__ballot(eff);
            if (lane == 0) {
                a.bitmap[2 * s + v] = (bm0 | setmask) & ~clrmask;
                a.count[2 * s + v] = rs_count_after(c0, (uint32_t)__builtin_popcount(cmask), a.W);
            }
            const uint32_t rh = rs_uniform(a.rhead[2 * s + v]);
            if (!cmask && !rh) continue;                       // neither a sum nor a result: registers only

            uint32_t* const acc = a.acc + ((uint64_t)2 * s + v) * M;
            u4 sum[kPer];
#pragma unroll
            for (int k = 0; k < kPer; k++) {
                const int ch = k * kWave + lane;
                sum[k] = mku4(0u, 0u, 0u, 0u);
                if (wmask == 0u && ch < kChunks) sum[k] = *reinterpret_cast<const u4*>(acc + 4 * ch);
            }
            uint32_t ex = a.exps[2 * s + v];
            if (cmask) {
                // kInFlight contributors' loads go out before the first add; a
                // lane past the message (M < 256) rereads chunk 0 and drops it
                for (uint32_t m = emask; m;) {
                    u4 w[kInFlight][kPer];
#pragma unroll
                    for (int b = 0; b < kInFlight; b++) {
#pragma unroll
                        for (int k = 0; k < kPer; k++) w[b][k] = mku4(0u, 0u, 0u, 0u);
                        if (m) {
                            const int j = __builtin_ctz(m);
                            m &= m - 1;
                            const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)src, j);
                            const uint8_t* const pl = a.landing + (uint64_t)sj * a.landing_stride;
#pragma unroll
                            for (int k = 0; k < kPer; k++) {
                                const int ch = k * kWave + lane;
                                w[b][k] = __builtin_nontemporal_load(
                                    reinterpret_cast<const u4*>(pl + 16 * (ch < kChunks ? ch : 0)));
                            }
                        }
                    }
#pragma unroll
                    for (int b = 0; b < kInFlight; b++)
#pragma unroll
                        for (int k = 0; k < kPer; k++) {
                            sum[k].x += bswap(w[b][k].x); sum[k].y += bswap(w[b][k].y);
                            sum[k].z += bswap(w[b][k].z); sum[k].w += bswap(w[b][k].w);
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
                for (int d = 1; d < (int)kRsMaxWorkers; d <<= 1) {
                    const int o0 = __shfl_xor(e0, d), o1 = __shfl_xor(e1, d);
                    e0 = o0 > e0 ? o0 : e0;
                    e1 = o1 > e1 ? o1 : e1;
                }
                e0 = (int)rs_uniform((uint32_t)e0);            // lane 0: the max over lanes 0..31
                e1 = (int)rs_uniform((uint32_t)e1);
                if (wmask == 0u) {
                    e0 = rs_max_i8(ex & 0xffu, (uint32_t)e0 & 0xffu);
                    e1 = rs_max_i8((ex >> 8) & 0xffu, (uint32_t)e1 & 0xffu);
                }
                ex = ((uint32_t)e0 & 0xffu) | (((uint32_t)e1 & 0xffu) << 8);
                if (lane == 0) a.exps[2 * s + v] = ex;
            }
            if (!rh) continue;

            // rdma_sender.p4: the sum as the wire carries it, to every region a result record names
            u4 out[kPer];
#pragma unroll
            for (int k = 0; k < kPer; k++) out[k] = mku4(bswap(sum[k].x), bswap(sum[k].y), bswap(sum[k].z), bswap(sum[k].w));
            for (uint32_t r = rh; r;) {
                const uint64_t i = r - 1u;
                const uint8_t* const rec = a.arrivals + i * kRsRecordBytes;
                const uint32_t w = rs_uniform(*reinterpret_cast<const uint32_t*>(rec));
                const uint32_t imm = rs_uniform(*reinterpret_cast<const uint32_t*>(rec + 8));
                const uint64_t addr = uniform_u64(*reinterpret_cast<const unsigned long long*>(rec + 16));
                const uint32_t dm = a.drop ? a.drop[i] : 0u;
                const uint32_t to = a.verdict[i] == SML_VERDICT_BROADCAST ? all : 1u << w;
                r = rs_uniform(a.out_imm[i]);                  // the link, before the immediate takes its place
                if (lane == 0) a.out_imm[i] = (imm & 0xffffu) | (ex << 16);
                for (uint32_t m = rs_uniform(to & ~dm); m; m &= m - 1) {
                    uint8_t* const dst = a.rx + (uint64_t)__builtin_ctz(m) * a.rx_bytes + addr;
#pragma unroll
                    for (int k = 0; k < kPer; k++) {
                        const int ch = k * kWave + lane;
                        if (ch < kChunks) SML_NT_STORE16(out[k], dst + 16 * ch);
                    }
                }
            }
            if (lane == 0) a.rhead[2 * s + v] = 0u;            // the next call's lists start empty
        }
        if (lane < (int)kRsMaxWorkers && c != 0ull) clp[lane] = 0ull;   // the next call's claims start empty
    }
}

// The pieces of d_state.
struct RsLayout {
    uint64_t claims, bitmap, count, exps, rhead, touched, acc, total;
};

static bool rs_layout(uint32_t S, uint32_t M, RsLayout& l) {
    if (!valid_packet(M) || S == 0 || S > kRsMaxSlots) return false;
    l.claims = kRsHead;
    l.bitmap = l.claims + 8ull * kRsMaxWorkers * S;
    l.count = l.bitmap + 8ull * S;
    l.exps = l.count + 8ull * S;
    l.rhead = l.exps + 8ull * S;
    l.touched = l.rhead + 8ull * S;
    l.acc = (l.touched + 4ull * S + 15) & ~15ull;
    l.total = l.acc + 8ull * S * M;
    return true;
}

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_rdma_switch_state_bytes(uint32_t num_slots, uint32_t msg_numel) {
    RsLayout l;
    return rs_layout(num_slots, msg_numel, l) ? l.total : 0;
}

sml_status_t sml_rdma_switch_reset(void* d_state, uint32_t num_slots, uint32_t msg_numel, void* stream) {
    if (!d_state) return SML_ERR_INVALID_ARG;
    RsLayout l;
    if (!rs_layout(num_slots, msg_numel, l)) return SML_ERR_UNSUPPORTED;
    if (!aligned16(d_state)) return SML_ERR_ALIGNMENT;
    // everything but the accumulators: a slot's words are written before they are read
    return hip_check(hipMemsetAsync(d_state, 0, l.acc, (hipStream_t)stream));
}

sml_status_t sml_rdma_switch(const sml_rdma_switch_params* prm, const sml_rdma_arrival* d_arrivals, uint64_t n,
                             const void* landing, uint64_t landing_stride, uint64_t landing_msgs, void* d_state,
                             void* rx, uint64_t rx_bytes, const uint32_t* d_drop, uint32_t* d_out_imm,
                             uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    if (!prm) return SML_ERR_INVALID_ARG;
    if (n && (!d_arrivals || !landing || !d_state || !rx || !d_out_imm || !d_verdict)) return SML_ERR_INVALID_ARG;
    const uint32_t M = prm->msg_numel, S = prm->num_slots, W = prm->num_workers, ppm = prm->pkts_per_msg;
    RsLayout l;
    if (!rs_layout(S, M, l) || W == 0 || W > kRsMaxWorkers || n > kRsMaxRecords) return SML_ERR_UNSUPPORTED;
    if (ppm != 1 && ppm != 2 && ppm != 4 && ppm != 8 && ppm != 16) return SML_ERR_UNSUPPORTED;
    if (n == 0) return SML_OK;
    if (!aligned16(landing) || landing_stride % 16 || landing_stride < 4ull * M) return SML_ERR_ALIGNMENT;
    if (!aligned16(rx) || rx_bytes % 16 || !aligned16(d_state)) return SML_ERR_ALIGNMENT;
    if (!aligned8(d_arrivals) || !aligned4(d_drop) || !aligned4(d_out_imm) || !aligned8(d_counts))
        return SML_ERR_ALIGNMENT;

    RsArgs a;
    memset(&a, 0, sizeof(a));
    uint8_t* const st8 = static_cast<uint8_t*>(d_state);
    a.arrivals = reinterpret_cast<const uint8_t*>(d_arrivals);
    a.n = n;
    a.landing = static_cast<const uint8_t*>(landing);
    a.landing_stride = landing_stride;
    a.landing_msgs = landing_msgs;
    a.rx = static_cast<uint8_t*>(rx);
    a.rx_bytes = rx_bytes;
    a.fits = rx_bytes >= 4ull * M;
    a.addr_max = a.fits ? rx_bytes - 4ull * M : 0;
    a.drop = d_drop;
    a.out_imm = d_out_imm;
    a.verdict = d_verdict;
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.touched_count = reinterpret_cast<uint32_t*>(st8);
    a.claims = reinterpret_cast<unsigned long long*>(st8 + l.claims);
    a.bitmap = reinterpret_cast<uint32_t*>(st8 + l.bitmap);
    a.count = reinterpret_cast<uint32_t*>(st8 + l.count);
    a.exps = reinterpret_cast<uint32_t*>(st8 + l.exps);
    a.rhead = reinterpret_cast<uint32_t*>(st8 + l.rhead);
    a.touched = reinterpret_cast<uint32_t*>(st8 + l.touched);
    a.acc = reinterpret_cast<uint32_t*>(st8 + l.acc);
    a.S = S;
    a.W = W;
    a.ppm_shift = (uint32_t)__builtin_ctz(ppm);

    hipStream_t st = (hipStream_t)stream;
    const uint32_t grecords = grid_for_vec(n);
    k_rs_claim<<<grecords, kBlockThreads, 0, st>>>(a);
    k_rs_verdict<<<grecords, kBlockThreads, 0, st>>>(a);
    // at most one touched slot per record, and per slot of the pool
    const uint32_t gslots = grid_for_tiles(n < S ? n : S);
    dispatch_packet(M, [&](auto Mc) { k_rs_apply<Mc()><<<gslots, kBlockThreads, 0, st>>>(a); });
    return launch_check();
}

}  // extern "C"
