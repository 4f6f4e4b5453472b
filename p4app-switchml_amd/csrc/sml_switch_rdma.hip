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
    // sml_msg_switch only: any pkts_per_msg, and a message as items of slices
    uint32_t ppm;                   // pkts_per_msg, 1..256
    uint64_t ppm_hi;                // ceil(2^64 / ppm) (ppm > 1): the quotient is one __umul64hi
    uint32_t M;                     // msg_numel
    uint32_t G;                     // items per slot: ceil(M / 1024)
};

// Record i as the passes see it.
struct RsRec {
    uint32_t w, s, v, imm, src;
    uint64_t addr;
    bool ok;                        // not IGNORED
};

// POW2: sml_rdma_switch's grid, a shift and a mask.  Otherwise any pkts_per_msg
// up to 256, with K4's host-computed reciprocal (msg_magic, sml_messages.hip):
// ppm_hi = ceil(2^64 / ppm) is at most ppm / 2^64 too large as a fraction, idx
// is below 2^31, so idx * ppm_hi / 2^64 exceeds idx / ppm by less than
// 2^31 * 256 / 2^64 < 1 / ppm and its floor is the exact quotient.
template <bool POW2>
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
    bool grid;
    if constexpr (POW2) {
        r.s = idx >> a.ppm_shift;
        grid = (idx & ((1u << a.ppm_shift) - 1u)) == 0u;
    } else {
        r.s = a.ppm == 1u ? idx : (uint32_t)__umul64hi((uint64_t)idx, a.ppm_hi);
        grid = r.s * a.ppm == idx;
    }
    r.ok = grid && r.s < a.S && r.w < a.W && r.src < a.landing_msgs &&
           (r.addr & 15u) == 0u && a.fits && r.addr <= a.addr_max;
    return r;
}

// workers_counter.p4's register action, n times: 0 -> W - 1, else one down.
__device__ __forceinline__ uint32_t rs_count_after(uint32_t c, uint32_t n, uint32_t W) {
    for (uint32_t i = 0; i < n; i++) c = c == 0 ? W - 1 : c - 1;
    return c;
}

// Pass 1: the (slot, worker) pair's lowest-index record, with its set.
template <bool POW2>
__global__ __launch_bounds__(kBlockThreads) void k_rs_claim(RsArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.touched_count = 0;      // this call's list starts empty
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const RsRec r = rs_record<POW2>(a, i);
        if (r.ok) atomicMax(a.claims + (uint64_t)r.s * kRsMaxWorkers + r.w, ~(((unsigned long long)i << 1) | r.v));
    }
}

// Pass 2: every record's verdict, by k_fs_verdict's argument: in the call,
// worker u moves its slot's registers once, at its claimed record, so the count
// record i sees is the call's starting count stepped once per new contributor
// of its set claimed below i.
template <bool POW2>
__global__ __launch_bounds__(kBlockThreads) void k_rs_verdict(RsArgs a) {
    __shared__ uint32_t hist[6];                              // records per verdict, dropped copies
    tally_init(hist);
    const uint32_t all = 0xffffffffu >> (32 - a.W);
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < a.n; i += stride) {
        const RsRec r = rs_record<POW2>(a, i);
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

// ---------------------------------------------------------------- long messages
// sml_msg_switch: any msg_numel the sml_msg_* entry points serve, up to 16384
// words.  Claim and verdict are the passes above; a message no longer fits one
// wave's registers, so pass 3 becomes two launches, neither with a wave that
// waits on another:
//   k_ms_data    wave per (touched slot, item).  A message is ceil(M / 256)
//                slices of one wave-wide 16-byte access (the last one masked to
//                its multiple of 16 lanes), a slot is G = ceil(M / 1024) items,
//                and slice j goes to item j mod G: at most 4 slices a lane at
//                every M, none idle while another holds 4.  The wave recomputes
//                its slot's bookkeeping, then does k_rs_apply's sum and results
//                for its slices alone.  It writes its part of the accumulator
//                and of the receive regions and nothing else: the registers,
//                the claim words, the list heads and the links in d_out_imm are
//                read by the slot's other waves in the same launch.
//   k_ms_commit  wave per touched slot, after the data pass: the same
//                bookkeeping, then everything k_rs_apply does to registers —
//                bitmap, count, exponents, the immediates over the links, the
//                list head and the claim words cleared.
constexpr int kMsPer = 4;          // slices per item at most: ceil(M / 256) <= 4 ceil(M / 1024)
constexpr int kMsInFlight = 2;     // contributors loaded before the first add (k_rs_apply's at 4 chunks a lane)

// A slot's claim words over a wave: lane u < 32 holds worker u's, with its
// claimed record's exponent bytes and where its message landed.
struct MsClaims {
    unsigned long long c;
    uint64_t iu;
    uint32_t cs, ed, src;
    bool live;                      // the claim names a record of this call
};

__device__ __forceinline__ MsClaims ms_claims(const RsArgs& a, uint32_t s, int lane) {
    MsClaims k;
    k.c = lane < (int)kRsMaxWorkers ? a.claims[(uint64_t)s * kRsMaxWorkers + lane] : 0ull;
    k.iu = (~k.c) >> 1;
    k.live = k.c != 0ull && k.iu < a.n;
    k.cs = (uint32_t)((~k.c) & 1ull);
    k.ed = 0;
    k.src = 0;
    if (k.live) {
        const u2 d = *reinterpret_cast<const u2*>(a.arrivals + k.iu * kRsRecordBytes + 8);
        k.ed = d.x >> 16;
        k.src = d.y;
    }
    return k;
}

// One (slot, set) as the call found it — k_fs_apply's bookkeeping: who claims
// the set, who contributes, who writes over the slot, whose words count.  Read
// only: both passes get the same answer as long as the commit pass's stores
// come after it.  False when no claim of the slot concerns the set.
struct MsSet {
    uint32_t setmask, clrmask, cmask, wmask, emask;   // ballots over the workers
    uint32_t bm0, c0, rh;           // bitmap, count, result-list head
    bool eff;                       // this lane's worker is an effective contributor
};

__device__ __forceinline__ bool ms_set(const RsArgs& a, uint32_t s, uint32_t v, int lane, const MsClaims& k, MsSet& q) {
    q.setmask = (uint32_t)__ballot(k.live && k.cs == v);
    q.clrmask = (uint32_t)__ballot(k.live && k.cs != v);
    if (!(q.setmask | q.clrmask)) return false;
    q.bm0 = a.bitmap[2 * s + v];
    q.c0 = a.count[2 * s + v];
    const bool contrib = k.live && k.cs == v && !((q.bm0 >> lane) & 1u);
    q.cmask = (uint32_t)__ballot(contrib);
    // the bitmap as this lane's claimed record finds it
    uint32_t before = q.bm0;
    for (uint32_t x = 0; x < a.W; x++) {
        const uint64_t ix = shfl_u64(k.iu, (int)x);
        if (ix < k.iu) {
            if ((q.setmask >> x) & 1u) before |= 1u << x;
            if ((q.clrmask >> x) & 1u) before &= ~(1u << x);
        }
    }
    const bool writer = contrib && before == 0u;
    q.wmask = (uint32_t)__ballot(writer);
    uint64_t iw = 0;                                   // the last writer's record
    for (uint32_t m = q.wmask; m; m &= m - 1) {
        const uint64_t ij = shfl_u64(k.iu, __builtin_ctz(m));
        iw = ij > iw ? ij : iw;
    }
    q.eff = contrib && (q.wmask == 0u || k.iu >= iw);
    q.emask = (uint32_t)__ballot(q.eff);
    q.rh = rs_uniform(a.rhead[2 * s + v]);
    return true;
}

// Pass 3 of the long path.  Item t = (touched slot t / G, item t % G); the
// item's slices are g, g + G, g + 2 G, g + 3 G, lane l of slice j holding the
// 16-byte chunk 64 j + l of the message.
__global__ __launch_bounds__(kBlockThreads) void k_ms_data(RsArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t all = 0xffffffffu >> (32 - a.W);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    const uint32_t nchunks = a.M / 4;                          // 16-byte chunks of a message
    const uint32_t nitems = *a.touched_count * a.G;
    for (uint32_t t = blockIdx.x * kWavesPerBlock + wave_index(); t < nitems; t += nwaves) {
        const uint32_t ts = t / a.G, g = t - ts * a.G;
        const uint32_t s = rs_uniform(a.touched[ts]);
        const MsClaims k = ms_claims(a, s, lane);
        const uint32_t ch0 = g * kWave + (uint32_t)lane, step = a.G * kWave;   // chunk ch0 + i step, i < kMsPer
#pragma unroll 1
        for (uint32_t v = 0; v < 2; v++) {
            MsSet q;
            if (!ms_set(a, s, v, lane, k, q)) continue;
            if (!q.cmask && !q.rh) continue;                   // neither a sum nor a result: registers only

            uint8_t* const acc = reinterpret_cast<uint8_t*>(a.acc + ((uint64_t)2 * s + v) * a.M);
            u4 sum[kMsPer];
#pragma unroll
            for (int i = 0; i < kMsPer; i++) {
                const uint32_t ch = ch0 + i * step;
                sum[i] = mku4(0u, 0u, 0u, 0u);
                if (q.wmask == 0u && ch < nchunks) sum[i] = *reinterpret_cast<const u4*>(acc + 16 * ch);
            }
            if (q.cmask) {
                for (uint32_t m = q.emask; m;) {
                    u4 w[kMsInFlight][kMsPer];
#pragma unroll
                    for (int b = 0; b < kMsInFlight; b++) {
#pragma unroll
                        for (int i = 0; i < kMsPer; i++) w[b][i] = mku4(0u, 0u, 0u, 0u);
                        if (m) {
                            const int j = __builtin_ctz(m);
                            m &= m - 1;
                            const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)k.src, j);
                            const uint8_t* const pl = a.landing + (uint64_t)sj * a.landing_stride;
#pragma unroll
                            for (int i = 0; i < kMsPer; i++) {
                                const uint32_t ch = ch0 + i * step;
                                if (ch < nchunks)
                                    w[b][i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(pl + 16 * ch));
                            }
                        }
                    }
#pragma unroll
                    for (int b = 0; b < kMsInFlight; b++)
#pragma unroll
                        for (int i = 0; i < kMsPer; i++) {
                            sum[i].x += bswap(w[b][i].x); sum[i].y += bswap(w[b][i].y);
                            sum[i].z += bswap(w[b][i].z); sum[i].w += bswap(w[b][i].w);
                        }
                }
#pragma unroll
                for (int i = 0; i < kMsPer; i++) {
                    const uint32_t ch = ch0 + i * step;
                    if (ch < nchunks) *reinterpret_cast<u4*>(acc + 16 * ch) = sum[i];
                }
            }
            if (!q.rh) continue;

            // rdma_sender.p4: this item's slices as the wire carries them, to every region a result record names
            u4 out[kMsPer];
#pragma unroll
            for (int i = 0; i < kMsPer; i++)
                out[i] = mku4(bswap(sum[i].x), bswap(sum[i].y), bswap(sum[i].z), bswap(sum[i].w));
            for (uint32_t r = q.rh; r;) {
                const uint64_t i = r - 1u;
                const uint8_t* const rec = a.arrivals + i * kRsRecordBytes;
                const uint32_t w = rs_uniform(*reinterpret_cast<const uint32_t*>(rec));
                const uint64_t addr = uniform_u64(*reinterpret_cast<const unsigned long long*>(rec + 16));
                const uint32_t dm = a.drop ? a.drop[i] : 0u;
                const uint32_t to = a.verdict[i] == SML_VERDICT_BROADCAST ? all : 1u << w;
                r = rs_uniform(a.out_imm[i]);                  // the link: the commit pass puts the immediate there
                for (uint32_t m = rs_uniform(to & ~dm); m; m &= m - 1) {
                    uint8_t* const dst = a.rx + (uint64_t)__builtin_ctz(m) * a.rx_bytes + addr;
#pragma unroll
                    for (int x = 0; x < kMsPer; x++) {
                        const uint32_t ch = ch0 + x * step;
                        if (ch < nchunks) SML_NT_STORE16(out[x], dst + 16 * ch);
                    }
                }
            }
        }
    }
}

// Pass 4 of the long path, wave per touched slot: the registers.
__global__ __launch_bounds__(kBlockThreads) void k_ms_commit(RsArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    const uint32_t ntouched = *a.touched_count;
    for (uint32_t t = blockIdx.x * kWavesPerBlock + wave_index(); t < ntouched; t += nwaves) {
        const uint32_t s = rs_uniform(a.touched[t]);
        const MsClaims k = ms_claims(a, s, lane);
#pragma unroll 1
        for (uint32_t v = 0; v < 2; v++) {
            MsSet q;
            if (!ms_set(a, s, v, lane, k, q)) continue;
            if (lane == 0) {
                a.bitmap[2 * s + v] = (q.bm0 | q.setmask) & ~q.clrmask;
                a.count[2 * s + v] = rs_count_after(q.c0, (uint32_t)__builtin_popcount(q.cmask), a.W);
            }
            if (!q.cmask && !q.rh) continue;
            uint32_t ex = a.exps[2 * s + v];
            if (q.cmask) {
                // exponents: signed int8 max, each byte on its own; -128 is the identity
                int e0 = q.eff ? (int)(int8_t)(k.ed & 0xffu) : -128;
                int e1 = q.eff ? (int)(int8_t)((k.ed >> 8) & 0xffu) : -128;
#pragma unroll
                for (int d = 1; d < (int)kRsMaxWorkers; d <<= 1) {
                    const int o0 = __shfl_xor(e0, d), o1 = __shfl_xor(e1, d);
                    e0 = o0 > e0 ? o0 : e0;
                    e1 = o1 > e1 ? o1 : e1;
                }
                e0 = (int)rs_uniform((uint32_t)e0);            // lane 0: the max over lanes 0..31
                e1 = (int)rs_uniform((uint32_t)e1);
                if (q.wmask == 0u) {
                    e0 = rs_max_i8(ex & 0xffu, (uint32_t)e0 & 0xffu);
                    e1 = rs_max_i8((ex >> 8) & 0xffu, (uint32_t)e1 & 0xffu);
                }
                ex = ((uint32_t)e0 & 0xffu) | (((uint32_t)e1 & 0xffu) << 8);
                if (lane == 0) a.exps[2 * s + v] = ex;
            }
            if (!q.rh) continue;
            for (uint32_t r = q.rh; r;) {
                const uint64_t i = r - 1u;
                const uint32_t imm = rs_uniform(*reinterpret_cast<const uint32_t*>(a.arrivals + i * kRsRecordBytes + 8));
                r = rs_uniform(a.out_imm[i]);                  // the link, before the immediate takes its place
                if (lane == 0) a.out_imm[i] = (imm & 0xffffu) | (ex << 16);
            }
            if (lane == 0) a.rhead[2 * s + v] = 0u;            // the next call's lists start empty
        }
        // the next call's claims start empty
        if (lane < (int)kRsMaxWorkers && k.c != 0ull) a.claims[(uint64_t)s * kRsMaxWorkers + lane] = 0ull;
    }
}

// The pieces of d_state.
struct RsLayout {
    uint64_t claims, bitmap, count, exps, rhead, touched, acc, total;
};


// sml_rdma_switch's pool holds packet-sized messages, sml_msg_switch's (any_msg)
// every length the sml_msg_* entry points serve: the same layout, M general.
static bool rs_layout(uint32_t S, uint32_t M, bool any_msg, RsLayout& l) {
    if (!(any_msg ? sml_msg_numel_supported(M) != 0 : valid_packet(M)) || S == 0 || S > kRsMaxSlots) return false;
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

static sml_status_t rs_reset(void* d_state, uint32_t S, uint32_t M, bool any_msg, void* stream) {
    if (!d_state) return SML_ERR_INVALID_ARG;
    RsLayout l;
    if (!rs_layout(S, M, any_msg, l)) return SML_ERR_UNSUPPORTED;
    if (!aligned16(d_state)) return SML_ERR_ALIGNMENT;
    // everything but the accumulators: a slot's words are written before they are read
    return hip_check(hipMemsetAsync(d_state, 0, l.acc, (hipStream_t)stream));
}

// Both families' call: every check before any launch, in one order, then the
// record passes and the family's own data movement.
static sml_status_t rs_call(bool any_msg, const sml_rdma_switch_params* prm, const sml_rdma_arrival* d_arrivals,
                            uint64_t n, const void* landing, uint64_t landing_stride, uint64_t landing_msgs,
                            void* d_state, void* rx, uint64_t rx_bytes, const uint32_t* d_drop, uint32_t* d_out_imm,
                            uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    if (!prm) return SML_ERR_INVALID_ARG;
    if (n && (!d_arrivals || !landing || !d_state || !rx || !d_out_imm || !d_verdict)) return SML_ERR_INVALID_ARG;
    const uint32_t M = prm->msg_numel, S = prm->num_slots, W = prm->num_workers, ppm = prm->pkts_per_msg;
    RsLayout l;
    if (!rs_layout(S, M, any_msg, l) || W == 0 || W > kRsMaxWorkers || n > kRsMaxRecords) return SML_ERR_UNSUPPORTED;
    if (any_msg ? ppm == 0 || ppm > 256 : ppm != 1 && ppm != 2 && ppm != 4 && ppm != 8 && ppm != 16)
        return SML_ERR_UNSUPPORTED;
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

    hipStream_t st = (hipStream_t)stream;
    const uint32_t grecords = grid_for_vec(n);
    // at most one touched slot per record, and per slot of the pool
    const uint64_t nslots = n < S ? n : S;
    if (!any_msg) {
        a.ppm_shift = (uint32_t)__builtin_ctz(ppm);
        k_rs_claim<true><<<grecords, kBlockThreads, 0, st>>>(a);
        k_rs_verdict<true><<<grecords, kBlockThreads, 0, st>>>(a);
        const uint32_t gslots = grid_for_tiles(nslots);
        dispatch_packet(M, [&](auto Mc) { k_rs_apply<Mc()><<<gslots, kBlockThreads, 0, st>>>(a); });
        return launch_check();
    }
    a.ppm = ppm;
    a.ppm_hi = ppm == 1 ? 0 : ~0ull / ppm + 1;     // a power of two: 2^64 / ppm, else floor + 1 = ceil
    a.M = M;
    a.G = (M + 1023) / 1024;
    k_rs_claim<false><<<grecords, kBlockThreads, 0, st>>>(a);
    k_rs_verdict<false><<<grecords, kBlockThreads, 0, st>>>(a);
    // the touched count is known on the device only: a wave per item of every slot that can be touched
    k_ms_data<<<grid_for_tiles(nslots * a.G), kBlockThreads, 0, st>>>(a);
    k_ms_commit<<<grid_for_tiles(nslots), kBlockThreads, 0, st>>>(a);
    return launch_check();
}

}  // namespace sml

using namespace sml;

extern "C" {

uint64_t sml_rdma_switch_state_bytes(uint32_t num_slots, uint32_t msg_numel) {
    RsLayout l;
    return rs_layout(num_slots, msg_numel, false, l) ? l.total : 0;
}

sml_status_t sml_rdma_switch_reset(void* d_state, uint32_t num_slots, uint32_t msg_numel, void* stream) {
    return rs_reset(d_state, num_slots, msg_numel, false, stream);
}

sml_status_t sml_rdma_switch(const sml_rdma_switch_params* prm, const sml_rdma_arrival* d_arrivals, uint64_t n,
                             const void* landing, uint64_t landing_stride, uint64_t landing_msgs, void* d_state,
                             void* rx, uint64_t rx_bytes, const uint32_t* d_drop, uint32_t* d_out_imm,
                             uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    return rs_call(false, prm, d_arrivals, n, landing, landing_stride, landing_msgs, d_state, rx, rx_bytes, d_drop,
                   d_out_imm, d_verdict, d_counts, stream);
}

uint64_t sml_msg_switch_state_bytes(uint32_t num_slots, uint32_t msg_numel) {
    RsLayout l;
    return rs_layout(num_slots, msg_numel, true, l) ? l.total : 0;
}

sml_status_t sml_msg_switch_reset(void* d_state, uint32_t num_slots, uint32_t msg_numel, void* stream) {
    return rs_reset(d_state, num_slots, msg_numel, true, stream);
}

sml_status_t sml_msg_switch(const sml_rdma_switch_params* prm, const sml_rdma_arrival* d_arrivals, uint64_t n,
                            const void* landing, uint64_t landing_stride, uint64_t landing_msgs, void* d_state,
                            void* rx, uint64_t rx_bytes, const uint32_t* d_drop, uint32_t* d_out_imm,
                            uint8_t* d_verdict, uint64_t* d_counts, void* stream) {
    return rs_call(true, prm, d_arrivals, n, landing, landing_stride, landing_msgs, d_state, rx, rx_bytes, d_drop,
                   d_out_imm, d_verdict, d_counts, stream);
}

}  // extern "C"
