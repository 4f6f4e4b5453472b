// sml_messages.hip — long RDMA messages (include/switchml_messages.h): the
// plane kernels for one exponent per MESSAGE of M elements, M any multiple of
// 64 up to 16384 (rdma_worker_thread.cc:86-88 quantizes per message, and
// config.cc:185-192 accepts every multiple of the packet size).  The plane
// kernels of sml_planes.h rest on "a packet lies inside one wave's tile"; a
// message of more than 1024 elements spans several waves, so its maximum has
// to cross waves.  The arithmetic is sml_device.h's, unchanged.
//
// Geometry (K1 / K2 / K3 and the fused round trip).  A message is cut into
// S = ceil(M / 256) slices of one wave-wide 16-byte load; the last slice is
// masked to 64, 128 or 192 elements when M is no multiple of 256.  A message
// occupies wpm = ceil(M / 1024) waves of one workgroup, 1 to 16, and its
// slices are dealt round-robin: slice s goes to wave s % wpm as that wave's
// slice s / wpm, so every wave keeps at most 4 slices (16 elements per lane)
// and the waves' loads of one round are consecutive KiB of the message.
// 16 waves x 16 elements per lane = 16384.  A workgroup is one message's wpm
// waves; with wpm = 1 or 2 it holds 4 or 2 messages at a time (4 waves).  wpm
// is a launch parameter, not a template one: rounding it up to a power of two
// left messages just above one (8448 elements on 16 waves) with half-empty
// waves and cost them 7 % (K1) and 25 % (round trip) on the 256 MiB stream
// against the 9 waves they run on now (a one-off probe).
// A message of at most 1024 elements has a wave of its own (no packing of
// several small messages into one wave's registers).
//
// Each element is read from HBM once and each payload word written once: the
// slices stay in registers between the maximum and the quantize.  A wave
// reduces its slices with the DPP reduce (group_max<256>), lane 0 writes one
// word to LDS, and after ONE barrier every wave of the message reads the wpm
// words of its message and reduces them inside a 16-lane row.  The LDS words
// are double-buffered by loop trip, so a fast wave's next maximum never lands
// on a word a slow wave still has to read, and one barrier per message is
// enough.  K3 takes no barrier at all: it reads the message's exponent once
// per wave, after its data loads are in flight.
//
// K4 is a stream on 512-element tiles (the plane kernels' measured K4 shape).
// M is a multiple of 64, so the 16 lanes of a 64-element chunk share a message
// and a 16-byte vector never straddles two.  The message of a chunk comes from
// two multiplications with host-computed reciprocals (msg_magic), exact for
// every numel < 2^56: no division in the kernel.
//
// The batched round trip (k_msg_roundtrip_batch, switchml_msg_batch.h) is the
// fused round trip's geometry over the slices of a table of kernel arguments.
#include "sml_host.h"
#include "sml_msg_deal.h"
#include "switchml_messages.h"

namespace sml {

template <class T>
struct MsgArgs {
    const T* in;
    T* out;                 // the round trip's output (unused by K1 / K2 / K3)
    uint64_t numel;
    uint64_t nmsgs;         // B
    uint64_t ngroups;       // ceil(B / messages per workgroup)
    const int8_t* gexp;     // global exponents (K3) or nullptr
    u4* payload;            // B*M words, 16-B aligned; nullable (K2, the round trip)
    int8_t* exps_out;       // nullable
    uint32_t M;
    uint32_t wpm;           // waves per message: ceil(M / 1024)
    uint32_t per_group;     // messages a workgroup holds at a time: 4, 2 (wpm 1, 2) or 1
    uint32_t W;
    uint32_t xcd;           // xcd_block chunk (0 = plain order)
};

// The scale table of a workgroup of any size, 192 threads (3 waves) to 1024
// (build_lut is the 256-thread form).
__device__ __forceinline__ void msg_build_lut(float* lut, uint32_t W) {
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = scale_for(W, (int)(int8_t)(uint8_t)i);
    __syncthreads();
}

// The loads of this wave's slices of message `msg`: whole vectors inside the
// slice, element by element across its end, zeros outside the message (a zero
// never wins the maximum and quantizes to the 0 the plane's tail holds).
template <class E, class T>
__device__ __forceinline__ void msg_load(const MsgArgs<T>& a, uint64_t msg, uint32_t part, int lane, f4 (&v)[kMsgU]) {
    const bool live = msg < a.nmsgs;
    const uint64_t mbase = live ? msg * a.M : 0;
    if (live && a.M % kTileElems == 0 && mbase + a.M <= a.numel) {
#pragma unroll
        for (int u = 0; u < kMsgU; u++) v[u] = E::load4(a.in + mbase + msg_offset(a.wpm, u, part, lane));
        return;
    }
#pragma unroll
    for (int u = 0; u < kMsgU; u++) {
        const uint32_t off = msg_offset(a.wpm, u, part, lane);
        const uint64_t idx = mbase + off;
        v[u] = mkf4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live && off < a.M) {
            if (idx + 4 <= a.numel) v[u] = E::load4(a.in + idx);
            else if (idx < a.numel) v[u] = E::load4_guarded(a.in + idx, idx, a.numel);
        }
    }
}

// Quantize + pack one vector; the round trip (RT) goes on through the dummy
// backend's x W and the dequantize to the output, as roundtrip_compute does.
template <class E, bool BE, bool RNE, bool NTS, bool RT, bool NT, class T>
__device__ __forceinline__ void msg_slice(const MsgArgs<T>& a, uint64_t idx, f4 v, float s, int e, uint64_t body) {
    const u4 qv = quantize4<RNE>(v, s, idx, body);
    if (a.payload) {
        u4 wq = qv;
        if constexpr (BE) wq = mku4(bswap(qv.x), bswap(qv.y), bswap(qv.z), bswap(qv.w));
        store_payload_as<NTS>(a.payload + idx / 4, wq);
    }
    if constexpr (RT) {
        const bool pow2 = (a.W & (a.W - 1)) == 0;
        f4 o;
        if (pow2) {
            const float r = rcp_scale_pow2(31 - __builtin_clz(a.W), e);
            o = mkf4(dequant1<true>(qv.x * a.W, r), dequant1<true>(qv.y * a.W, r), dequant1<true>(qv.z * a.W, r),
                     dequant1<true>(qv.w * a.W, r));
        } else {
            o = mkf4(dequant1<false>(qv.x * a.W, s), dequant1<false>(qv.y * a.W, s), dequant1<false>(qv.z * a.W, s),
                     dequant1<false>(qv.w * a.W, s));
        }
        if (idx + 4 <= a.numel) E::template store4<NT>(a.out + idx, o);
        else if (idx < a.numel) E::store4_guarded(a.out + idx, o, idx, a.numel);
    }
}

// Exponent, quantize and pack of one loaded message part.  smax: this loop
// trip's 16 LDS words, one per wave of the workgroup.
template <class E, bool GLOBAL, bool BE, bool RNE, bool NTS, bool RT, bool NT, class T>
__device__ __forceinline__ void msg_compute(const MsgArgs<T>& a, uint64_t msg, uint32_t wave, uint32_t part, int lane,
                                            const f4 (&v)[kMsgU], const float* lut, uint32_t* smax) {
    const bool live = msg < a.nmsgs;
    int e;
    if constexpr (GLOBAL) {
        e = live ? (int)a.gexp[msg] : 0;       // one read per wave: msg is wave-uniform
    } else {
        uint32_t m = max4(v[0]);
#pragma unroll
        for (int u = 1; u < kMsgU; u++) m = umax(m, max4(v[u]));
        m = group_max<256>(m);                 // the wave's maximum, wave-uniform
        if (a.wpm > 1) {                       // the same branch in every wave of the workgroup
            if (lane == 0) smax[wave] = m;
            __syncthreads();
            // every 16-lane row reads the wpm <= 16 words of this wave's message
            const uint32_t l = (uint32_t)lane & 15u;
            m = group_max<64>(smax[wave - part + (l < a.wpm ? l : a.wpm - 1)]);
            m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        }
        e = exponent_of(m);
        if (a.exps_out && live && part == 0 && lane == 0) a.exps_out[msg] = (int8_t)e;
    }
    if (!live) return;
    if constexpr (!RT) {
        if (!a.payload) return;
    }
    const float s = lut[(uint8_t)e];
    const uint64_t mbase = msg * a.M;
    const uint64_t n = a.numel - mbase < (uint64_t)a.M ? a.numel - mbase : (uint64_t)a.M;
    const uint64_t body = mbase + (n - n % 16);            // the message's VCL body (RNE)
    // A message that fills its waves takes a branch-free slice loop (a skip per
    // slice makes hipcc wait for the previous slice's store: sml_planes.h).
    if (a.M % kTileElems == 0) {
#pragma unroll
        for (int u = 0; u < kMsgU; u++)
            msg_slice<E, BE, RNE, NTS, RT, NT>(a, mbase + msg_offset(a.wpm, u, part, lane), v[u], s, e, body);
        return;
    }
#pragma unroll
    for (int u = 0; u < kMsgU; u++) {
        const uint32_t off = msg_offset(a.wpm, u, part, lane);
        if (off < a.M) msg_slice<E, BE, RNE, NTS, RT, NT>(a, mbase + off, v[u], s, e, body);
    }
}

// K1 (fused), K2 (payload == nullptr), K3 (GLOBAL) and, with RT, the fused
// loopback round trip.  Workgroup g of the permuted order takes message group
// g, g + gridDim.x, ...; the next group's loads are issued before the loop
// comes round, and the first group's before the scale table and its barrier.
// One code object serves every workgroup size (the launch's wpm * per_group
// waves): the bound is the largest, 128 VGPRs a lane, and no instance needs
// more than 69.
template <class E, bool GLOBAL, bool BE, bool RNE, bool NTS, bool RT, bool NT>
__global__ __launch_bounds__(kMsgMaxWaves * kWave) void k_msg_quantize(MsgArgs<typename E::raw> a) {
    __shared__ float lut[256];
    __shared__ uint32_t smax[2][kMsgMaxWaves];
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = wave_index();
    // several messages a workgroup only for wpm = 1, 2: a mask and a shift
    const uint32_t part = a.per_group == 1 ? wave : wave & (a.wpm - 1);
    const uint32_t sub = a.per_group == 1 ? 0u : wave >> (a.wpm - 1);
    uint64_t g = xcd_block(a.xcd);
    f4 v[kMsgU];
    if (g < a.ngroups) msg_load<E>(a, g * a.per_group + sub, part, lane, v);
    if (RT || a.payload) msg_build_lut(lut, a.W);
    for (uint32_t trip = 0; g < a.ngroups; trip ^= 1u) {
        msg_compute<E, GLOBAL, BE, RNE, NTS, RT, NT>(a, g * a.per_group + sub, wave, part, lane, v, lut, smax[trip]);
        g += gridDim.x;
        if (g < a.ngroups) msg_load<E>(a, g * a.per_group + sub, part, lane, v);
    }
}

// The fused round trip over a batch of slices (of one or several jobs) in ONE
// launch (include/switchml_msg_batch.h).  The batch's message groups are
// numbered consecutively over the slices: slice s owns ceil(B_s / per_group)
// groups, group_end[s] = groups of slices 0..s, so a group never spans two
// slices and a slice's messages restart at its own first element.  The table
// travels as kernel arguments, 1816 bytes for every T.
template <class T>
struct MsgBatchArgs {
    const T* in[SML_MAX_BATCH_SLICES];
    T* out[SML_MAX_BATCH_SLICES];
    uint64_t numel[SML_MAX_BATCH_SLICES];
    uint32_t group_end[SML_MAX_BATCH_SLICES];
    uint32_t nslices;
    uint32_t M;
    uint32_t wpm;
    uint32_t per_group;
    uint32_t W;
    uint32_t xcd;
};
static_assert(sizeof(MsgBatchArgs<float>) <= 4096 && sizeof(MsgBatchArgs<uint16_t>) == sizeof(MsgBatchArgs<float>),
              "the table travels as kernel arguments");

// The slice of message group g as the single-slice kernel's arguments, and the
// group's first message inside that slice.  g is workgroup-uniform: the search
// over group_end is scalar loads and scalar branches.  No division: nmsgs is
// not the slice's count but a bound that answers "is message k live" for the
// messages of this group alone, from k * M < numel.  A slice whose count is no
// multiple of per_group ends in a group with dead messages, whose waves take
// msg_compute's barrier and store nothing.
template <class T>
__device__ __forceinline__ uint64_t msg_batch_group(const MsgBatchArgs<T>& b, uint32_t g, MsgArgs<T>& a) {
    uint32_t lo = 0, hi = b.nslices - 1;                 // first s with group_end[s] > g
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (b.group_end[mid] > g) hi = mid;
        else lo = mid + 1;
    }
    const uint64_t k0 = (uint64_t)(g - (lo ? b.group_end[lo - 1] : 0u)) * b.per_group;
    a.in = b.in[lo];
    a.out = b.out[lo];
    a.numel = b.numel[lo];
    a.nmsgs = k0 + 1;                                    // a group exists for its first message
    for (uint32_t j = 1; j < b.per_group; j++) a.nmsgs += (k0 + j) * b.M < a.numel;
    a.ngroups = 0;
    a.gexp = nullptr;
    a.payload = nullptr;
    a.exps_out = nullptr;
    a.M = b.M;
    a.wpm = b.wpm;
    a.per_group = b.per_group;
    a.W = b.W;
    a.xcd = b.xcd;
    return k0;
}

// k_msg_quantize's round trip with the slice looked up once per loop trip.
// The next group may belong to the next slice: its lookup comes before its
// loads, the loaded registers travel with their own slice's arguments (nxt
// becomes cur), and the stores use the slice the loads came from.  A lane
// stores exactly the elements it loaded, after their loads, and slices do not
// overlap, so in == out within a slice is safe.
template <class E, bool RNE, bool NT>
__global__ __launch_bounds__(kMsgMaxWaves * kWave) void k_msg_roundtrip_batch(MsgBatchArgs<typename E::raw> b) {
    __shared__ float lut[256];
    __shared__ uint32_t smax[2][kMsgMaxWaves];
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = wave_index();
    const uint32_t part = b.per_group == 1 ? wave : wave & (b.wpm - 1);
    const uint32_t sub = b.per_group == 1 ? 0u : wave >> (b.wpm - 1);
    const uint64_t ngroups = b.group_end[b.nslices - 1];
    uint64_t g = xcd_block(b.xcd);
    MsgArgs<typename E::raw> cur, nxt;
    uint64_t k = 0, kn = 0;
    f4 v[kMsgU];
    if (g < ngroups) {
        k = msg_batch_group(b, (uint32_t)g, cur) + sub;
        msg_load<E>(cur, k, part, lane, v);
    }
    msg_build_lut(lut, b.W);
    for (uint32_t trip = 0; g < ngroups; trip ^= 1u) {
        g += gridDim.x;
        const bool more = g < ngroups;
        if (more) kn = msg_batch_group(b, (uint32_t)g, nxt) + sub;
        msg_compute<E, false, true, RNE, false, true, NT>(cur, k, wave, part, lane, v, lut, smax[trip]);
        if (more) {
            msg_load<E>(nxt, kn, part, lane, v);
            cur = nxt;
            k = kn;
        }
    }
}

// floor(c / d) for chunks of 64 elements, d = M / 64 in 1..256, without a
// division in the kernel. hi = ceil(2^64 / d) (0 for d == 1, which needs
// none): mulhi(c, hi) = floor(c / d) while c * (hi * d - 2^64) < 2^64, and
// hi * d - 2^64 < d <= 2^8, so for every c < 2^56.  lo = ceil(2^20 / d):
// (r * lo) >> 20 = floor(r / d) while r * (lo * d - 2^20) < 2^20, r < 2^12.
struct MsgMagic {
    uint64_t hi;
    uint32_t lo;
    uint32_t d;
};

inline MsgMagic msg_magic(uint32_t M) {
    MsgMagic m;
    m.d = M / 64;
    m.hi = m.d == 1 ? 0 : ~0ull / m.d + 1;      // d a power of two: 2^64 / d, else floor + 1 = ceil
    m.lo = ((1u << 20) + m.d - 1) / m.d;
    return m;
}

template <class T>
struct MsgDequantArgs {
    const u4* payload;
    const int8_t* exps;
    T* out;
    uint64_t numel;
    uint64_t nmsgs;
    uint64_t ntiles;        // ceil(numel / 512)
    MsgMagic magic;
    uint32_t W;
    uint32_t xcd;
};

// One exponent byte through the scalar data cache: the aligned dword that
// holds it (p must be wave-uniform).
__device__ __forceinline__ uint32_t uniform_byte(const int8_t* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return (*reinterpret_cast<ConstU32*>(a & ~(uintptr_t)3) >> (8 * (a & 3u))) & 0xffu;
}

// K4 for messages: k_dequantize's stream, with the message of each 64-element
// chunk from the tile's first message k0 and the chunk's distance to it.
template <class E, bool BE, bool RCP, bool NT>
__global__ __launch_bounds__(kBlockThreads) void k_msg_dequantize(MsgDequantArgs<typename E::raw> a) {
    constexpr int U = 2, kElems = tile_elems<U>(), kChunks = kElems / 64;
    __shared__ float lut[256];
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    if constexpr (RCP) build_rcp_lut(lut, a.W);
    else build_lut(lut, a.W);
    for (uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index(); t < a.ntiles; t += nwaves) {
        const uint64_t base = t * kElems, c0 = t * kChunks;
        const bool full = base + kElems <= a.numel;
        const uint64_t k0 = a.magic.d == 1 ? c0 : __umul64hi(c0, a.magic.hi);
        const uint32_t r0 = (uint32_t)(c0 - k0 * a.magic.d);
        // M >= 512: the tile touches its first message and at most the next one,
        // whose two exponent bytes are wave-uniform (a byte load per lane per
        // slice costs the plane kernels ~8 %)
        const bool two = a.magic.d >= (uint32_t)kChunks;
        float s0 = 0.0f, s1 = 0.0f;
        if (two) {
            s0 = lut[uniform_byte(a.exps + k0)];
            s1 = lut[uniform_byte(a.exps + (k0 + 1 < a.nmsgs ? k0 + 1 : k0))];
        }
        u4 w[U];
        float s[U];
        if (full && two) {
            // the stream's common case, branch-free (blocks shared with the
            // partial tile make hipcc wait for the previous slice's store:
            // k_dequantize)
#pragma unroll
            for (int u = 0; u < U; u++) {
                w[u] = __builtin_nontemporal_load(a.payload + (base + (uint64_t)(u * kWave + lane) * 4) / 4);
                s[u] = ((r0 + (uint32_t)(u * 4 + (lane >> 4))) * a.magic.lo) >> 20 ? s1 : s0;
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                E::template store4<NT>(a.out + base + (uint64_t)(u * kWave + lane) * 4, dequant_words<BE, RCP>(w[u], s[u]));
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
            if (full || idx < a.numel) {
                w[u] = __builtin_nontemporal_load(a.payload + idx / 4);
                const uint32_t dk = ((r0 + (uint32_t)(u * 4 + (lane >> 4))) * a.magic.lo) >> 20;
                s[u] = two ? (dk ? s1 : s0) : lut[(uint8_t)a.exps[k0 + dk]];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
            if (!full && idx >= a.numel) continue;
            const f4 o = dequant_words<BE, RCP>(w[u], s[u]);
            if (full) E::template store4<NT>(a.out + idx, o);
            else E::store4_guarded(a.out + idx, o, idx, a.numel);
        }
    }
}

// ------------------------------------------------------------ host side

inline bool msg_supported(uint32_t M) { return M >= 64 && M <= SML_MSG_NUMEL_MAX && M % SML_MSG_NUMEL_STEP == 0; }
inline bool msg_float_type(sml_data_type_t dt) { return dt == SML_FLOAT32 || is_half(dt); }
constexpr uint64_t kMsgNumelLimit = 1ull << 56;          // msg_magic's range

// The element policy of a slice by its variant: fp32 16-byte aligned or not,
// FLOAT16 or BFLOAT16.
template <bool F16>
using MsgHalf = Elem16<F16 ? kHalfF16 : kHalfBF16>;

// Geometry of a launch: message groups, the one-shot grid, and XCD runs of the
// plane kernels' byte length (g_xcd_chunk workgroups of 4 tiles of 4 KiB).
// (A is MsgArgs, or MsgBatchArgs with its group count.)
template <class A>
static uint32_t msg_grid(A& a, uint64_t ngroups) {
    const uint64_t run = (uint64_t)g_xcd_chunk.load(std::memory_order_relaxed) * 4 * kTileElems;
    const uint64_t c = run / ((uint64_t)a.per_group * a.M);
    a.xcd = run == 0 ? 0u : (uint32_t)(c ? c : 1);
    uint64_t g = ngroups;
    const uint32_t lim = g_grid_limit.load(std::memory_order_relaxed);
    if (lim && g > lim) g = lim;
    if (g > 0x7fffffffull) g = 0x7fffffffull;
    return (uint32_t)g;
}

inline uint32_t msg_per_group(uint32_t wpm) { return wpm <= 2 ? kWavesPerBlock / wpm : 1; }

template <class T>
static uint32_t msg_geometry(MsgArgs<T>& a) {
    a.wpm = msg_waves(a.M);
    a.per_group = msg_per_group(a.wpm);
    a.ngroups = (a.nmsgs + a.per_group - 1) / a.per_group;
    return msg_grid(a, a.ngroups);
}

// K1 / K2 / K3 and the round trip (d_out != nullptr) of one typed slice; the
// callers have made every check.
template <template <bool> class EV, class T>
static sml_status_t msg_launch(const T* d_in, T* d_out, bool variant, uint64_t numel, uint32_t M, uint16_t W,
                               const int8_t* d_gexp, int32_t* d_payload, int8_t* d_exps_out, uint32_t flags,
                               void* stream) {
    MsgArgs<T> a;
    a.in = d_in;
    a.out = d_out;
    a.numel = numel;
    a.nmsgs = numel / M + (numel % M != 0);
    a.gexp = d_gexp;
    a.payload = reinterpret_cast<u4*>(d_payload);
    a.exps_out = d_gexp ? nullptr : d_exps_out;
    a.M = M;
    a.W = W;
    const dim3 grid(msg_geometry(a));
    hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE), rne = flags & SML_FLAG_ROUND_RNE;
    const uint32_t threads = a.wpm * a.per_group * kWave;
    if (d_out) {
        // the round trip: the payload plane keeps the default policy, the
        // output streams past the Infinity Cache (plane_roundtrip's rule)
        dispatch_bools([&](auto V, auto BE, auto RNE, auto NT) {
            k_msg_quantize<EV<V()>, false, BE(), RNE(), false, true, NT()><<<grid, threads, 0, st>>>(a);
        }, variant, be, rne, nt_from(sizeof(T) * numel));
    } else {
        dispatch_bools([&](auto GLOBAL, auto V, auto BE, auto RNE, auto NTS) {
            k_msg_quantize<EV<V()>, GLOBAL(), BE(), RNE(), NTS(), false, false><<<grid, threads, 0, st>>>(a);
        }, d_gexp != nullptr, variant, be, rne, d_payload && nt_from(4 * numel));
    }
    return launch_check();
}

template <template <bool> class EV, class T>
static sml_status_t msg_dequantize(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel, uint32_t M,
                                   uint16_t W, T* d_out, bool variant, uint32_t flags, void* stream) {
    MsgDequantArgs<T> a;
    a.payload = reinterpret_cast<const u4*>(d_payload);
    a.exps = d_exps;
    a.out = d_out;
    a.numel = numel;
    a.nmsgs = numel / M + (numel % M != 0);
    a.ntiles = (numel + 511) / 512;
    a.magic = msg_magic(M);
    a.W = W;
    a.xcd = xcd_chunk_for(2);
    const dim3 grid(grid_for_tiles(a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE), rcp = (W & (W - 1)) == 0;
    dispatch_bools([&](auto V, auto BE, auto RCP, auto NT) {
        k_msg_dequantize<EV<V()>, BE(), RCP(), NT()><<<grid, kBlockThreads, 0, st>>>(a);
    }, variant, be, rcp, nt_from(sizeof(T) * numel));
    return launch_check();
}

// A typed buffer's alignment: 4 bytes for fp32, 2 for a 16-bit type.
static bool msg_elem_ok(const void* p, sml_data_type_t dt) {
    return p && ((uintptr_t)p & (dt == SML_FLOAT32 ? 3u : 1u)) == 0;
}

// The checks every entry point shares, from msg_numel on (the header's order).
static sml_status_t msg_common(sml_data_type_t dt, uint64_t numel, uint32_t M) {
    if (!msg_supported(M) || !msg_float_type(dt) || numel >= kMsgNumelLimit) return SML_ERR_UNSUPPORTED;
    return SML_OK;
}

// The packet sizes of the plane kernels, which these entry points hand over to
// (one wave per message of less than 1024 elements would idle most lanes).
static bool msg_is_packet(uint32_t M) { return M <= 512 && valid_packet(M); }

static sml_status_t msg_quantize_any(const void* d_in, void* d_out, sml_data_type_t dt, uint64_t numel, uint32_t M,
                                     uint16_t W, const int8_t* d_gexp, int32_t* d_payload, int8_t* d_exps_out,
                                     uint32_t flags, void* stream) {
    if (dt == SML_FLOAT32) {
        const float* in = static_cast<const float*>(d_in);
        float* out = static_cast<float*>(d_out);
        return msg_launch<ElemF32>(in, out, aligned16(in) && aligned16(out), numel, M, W, d_gexp, d_payload,
                                   d_exps_out, flags, stream);
    }
    return msg_launch<MsgHalf>(static_cast<const uint16_t*>(d_in), static_cast<uint16_t*>(d_out), dt == SML_FLOAT16,
                               numel, M, W, d_gexp, d_payload, d_exps_out, flags, stream);
}

// One non-empty, checked slice into the table of its element type; false when
// the launch would number more than 2^32 - 1 groups.
template <class T>
static bool msg_batch_add(MsgBatchArgs<T>& a, uint64_t& groups, const sml_typed_slice& sl) {
    const uint64_t nmsgs = sl.numel / a.M + (sl.numel % a.M != 0);
    groups += (nmsgs + a.per_group - 1) / a.per_group;
    if (groups > 0xFFFFFFFFull) return false;
    a.in[a.nslices] = static_cast<const T*>(sl.in);
    a.out[a.nslices] = static_cast<T*>(sl.out);
    a.numel[a.nslices] = sl.numel;
    a.group_end[a.nslices] = (uint32_t)groups;
    a.nslices++;
    return true;
}

// The launch of one type's filled table: nothing for an empty one, the
// single-slice kernel for one slice, else one k_msg_roundtrip_batch.  fp32
// takes the unaligned form whatever the slices' starts (FIFO slices start
// anywhere), as the packet batch does.
template <template <bool> class EV, class T>
static sml_status_t msg_batch_launch(MsgBatchArgs<T>& a, bool variant, sml_data_type_t dt, bool rne, bool nt,
                                     void* stream) {
    if (a.nslices == 0) return SML_OK;
    if (a.nslices == 1)
        return msg_quantize_any(a.in[0], a.out[0], dt, a.numel[0], a.M, (uint16_t)a.W, nullptr, nullptr, nullptr,
                                rne ? SML_FLAG_ROUND_RNE : 0u, stream);
    const dim3 grid(msg_grid(a, a.group_end[a.nslices - 1]));
    const uint32_t threads = a.wpm * a.per_group * kWave;
    hipStream_t st = (hipStream_t)stream;
    dispatch_bools([&](auto V, auto RNE, auto NT) {
        k_msg_roundtrip_batch<EV<V()>, RNE(), NT()><<<grid, threads, 0, st>>>(a);
    }, variant, rne, nt);
    return launch_check();
}

// fp32 slices of a batch: always the 4-byte-aligned form.
template <bool>
using MsgBatchF32 = ElemF32<false>;

}  // namespace sml

using namespace sml;

extern "C" {

int sml_msg_numel_supported(uint32_t msg_numel) { return msg_supported(msg_numel) ? 1 : 0; }

sml_status_t sml_msg_exponents(const void* d_in, sml_data_type_t dt, uint64_t numel, uint32_t msg_numel,
                               int8_t* d_exps, void* stream) {
    if (numel && !d_exps) return SML_ERR_INVALID_ARG;
    const sml_status_t s = msg_common(dt, numel, msg_numel);
    if (s != SML_OK) return s;
    if (numel == 0) return SML_OK;
    if (!msg_elem_ok(d_in, dt)) return SML_ERR_INVALID_ARG;
    if (msg_is_packet(msg_numel)) return sml_exponents_typed(d_in, dt, numel, msg_numel, d_exps, stream);
    return msg_quantize_any(d_in, nullptr, dt, numel, msg_numel, 1, nullptr, nullptr, d_exps, 0, stream);
}

sml_status_t sml_msg_quantize_pack(const void* d_in, sml_data_type_t dt, uint64_t numel, uint32_t msg_numel,
                                   uint16_t num_workers, const int8_t* d_global_exps, int32_t* d_payload,
                                   int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel && !d_payload) return SML_ERR_INVALID_ARG;
    if (d_global_exps && d_exps_out && d_exps_out != d_global_exps) return SML_ERR_INVALID_ARG;
    const sml_status_t s = msg_common(dt, numel, msg_numel);
    if (s != SML_OK) return s;
    if (numel == 0) return SML_OK;
    if (!msg_elem_ok(d_in, dt)) return SML_ERR_INVALID_ARG;
    if (!aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    if (msg_is_packet(msg_numel))
        return sml_quantize_pack_typed(d_in, dt, numel, msg_numel, num_workers, d_global_exps, d_payload, d_exps_out,
                                       flags, stream);
    return msg_quantize_any(d_in, nullptr, dt, numel, msg_numel, num_workers, d_global_exps, d_payload, d_exps_out,
                            flags, stream);
}

sml_status_t sml_msg_dequantize(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel, uint32_t msg_numel,
                                uint16_t num_workers, void* d_out, sml_data_type_t dt, uint32_t flags, void* stream) {
    const sml_status_t s = msg_common(dt, numel, msg_numel);
    if (s != SML_OK) return s;
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!d_payload || !d_exps || !msg_elem_ok(d_out, dt)) return SML_ERR_INVALID_ARG;
    if (!aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    if (msg_is_packet(msg_numel))
        return sml_dequantize_typed(d_payload, d_exps, numel, msg_numel, num_workers, d_out, dt, flags, stream);
    if (dt == SML_FLOAT32)
        return msg_dequantize<ElemF32>(d_payload, d_exps, numel, msg_numel, num_workers, static_cast<float*>(d_out),
                                       aligned16(d_out), flags, stream);
    return msg_dequantize<MsgHalf>(d_payload, d_exps, numel, msg_numel, num_workers, static_cast<uint16_t*>(d_out),
                                   dt == SML_FLOAT16, flags, stream);
}

sml_status_t sml_msg_roundtrip_loopback(const void* d_in, void* d_out, sml_data_type_t dt, uint64_t numel,
                                        uint32_t msg_numel, uint16_t num_workers, int32_t* d_payload,
                                        int8_t* d_exps_out, uint32_t flags, void* stream) {
    const sml_status_t s = msg_common(dt, numel, msg_numel);
    if (s != SML_OK) return s;
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!msg_elem_ok(d_in, dt) || !msg_elem_ok(d_out, dt)) return SML_ERR_INVALID_ARG;
    if (d_payload && !aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    if (msg_is_packet(msg_numel))
        return sml_roundtrip_loopback_typed(d_in, d_out, dt, numel, msg_numel, num_workers, d_payload, d_exps_out,
                                            flags, stream);
    return msg_quantize_any(d_in, d_out, dt, numel, msg_numel, num_workers, nullptr, d_payload, d_exps_out, flags,
                            stream);
}

sml_status_t sml_msg_roundtrip_loopback_batch(const sml_typed_slice* slices, uint32_t num_slices, uint32_t msg_numel,
                                              uint16_t num_workers, uint32_t flags, void* stream) {
    if (!msg_supported(msg_numel)) return SML_ERR_UNSUPPORTED;
    if (num_workers == 0 || num_slices > SML_MAX_BATCH_SLICES || (num_slices && !slices)) return SML_ERR_INVALID_ARG;
    // One table per element type, every slice checked before any launch.
    MsgBatchArgs<float> f32;
    MsgBatchArgs<uint16_t> h[2];   // [0] BFLOAT16, [1] FLOAT16
    f32.nslices = h[0].nslices = h[1].nslices = 0;
    f32.M = h[0].M = h[1].M = msg_numel;
    f32.wpm = h[0].wpm = h[1].wpm = msg_waves(msg_numel);
    f32.per_group = h[0].per_group = h[1].per_group = msg_per_group(f32.wpm);
    f32.W = h[0].W = h[1].W = num_workers;
    uint64_t groups_f32 = 0, groups_h[2] = {0, 0}, out_bytes = 0;
    for (uint32_t i = 0; i < num_slices; i++) {
        const sml_typed_slice& sl = slices[i];
        if (sl.reserved != 0) return SML_ERR_INVALID_ARG;
        const sml_data_type_t dt = (sml_data_type_t)sl.data_type;
        if (!msg_float_type(dt) || sl.numel >= kMsgNumelLimit) return SML_ERR_UNSUPPORTED;
        if (sl.numel == 0) continue;
        if (!msg_elem_ok(sl.in, dt) || !msg_elem_ok(sl.out, dt)) return SML_ERR_INVALID_ARG;
        const int k = dt == SML_FLOAT16;
        if (!(dt == SML_FLOAT32 ? msg_batch_add(f32, groups_f32, sl) : msg_batch_add(h[k], groups_h[k], sl)))
            return SML_ERR_UNSUPPORTED;
        out_bytes += (dt == SML_FLOAT32 ? 4 : 2) * sl.numel;
    }
    if (f32.nslices + h[0].nslices + h[1].nslices == 0) return SML_OK;
    // the packet sizes sml_msg_roundtrip_loopback hands over: the packet batch
    if (msg_is_packet(msg_numel))
        return sml_roundtrip_loopback_batch_typed(slices, num_slices, msg_numel, num_workers, flags, stream);
    // the outputs of the whole call past the Infinity Cache: non-temporal stores
    const bool rne = flags & SML_FLAG_ROUND_RNE, nt = nt_from(out_bytes);
    sml_status_t s = msg_batch_launch<MsgBatchF32>(f32, false, SML_FLOAT32, rne, nt, stream);
    for (int k = 0; k < 2 && s == SML_OK; k++)
        s = msg_batch_launch<MsgHalf>(h[k], k == 1, k ? SML_FLOAT16 : SML_BFLOAT16, rne, nt, stream);
    return s;
}

}  // extern "C"
