// sml_planes.h — the plane kernels as templates on the element policy E
// (ElemF32<ALIGNED> / Elem16<H>, sml_device.h): K1 / K2 / K3 quantize + pack,
// K4 dequantize and the fused loopback round trip, with the host-side set-up
// of each (checks, arguments, launch).  sml_quantizer.hip instantiates them
// for fp32 and sml_half.hip for FLOAT16 / BFLOAT16, so the two units build in
// parallel.  An element is widened to fp32 by E's loads and narrowed by its
// stores; everything between is the same code for every type.
#ifndef SML_PLANES_H_
#define SML_PLANES_H_

#include "sml_host.h"

namespace sml {

// -------------------------------------------------------------- kernels

// K3: the tile's global exponents (one scalar load per slice when aligned).
template <int P, int U, class T>
__device__ __forceinline__ void global_tile_exponents(const QuantArgs<T>& a, uint64_t base, int lane, int (&e)[U]) {
    if (base + tile_elems<U>() <= a.nblocks * P && slice_exps_scalar_ok<P>(a.gexp)) {
#pragma unroll
        for (int u = 0; u < U; u++) e[u] = (int)(int8_t)slice_exponent_byte<P>(a.gexp, base, u, lane);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++) {
            uint64_t pkt = (base + (uint64_t)(u * kWave + lane) * 4) / P;
            e[u] = pkt < a.nblocks ? (int)a.gexp[pkt] : 0;
        }
    }
}

// Quantize + pack 4 consecutive elements (one lane's part of a slice).
template <int P, bool BE, bool RNE, bool NTS, class T>
__device__ __forceinline__ void quant_slice(const QuantArgs<T>& a, uint64_t idx, f4 v, const float* lut, int e) {
    const float s = lut[(uint8_t)e];
    uint64_t body = 0;
    if constexpr (RNE) body = vcl_body<P>(idx, a.numel);
    u4 q = quantize4<RNE>(v, s, idx, body);
    if constexpr (BE) { q.x = bswap(q.x); q.y = bswap(q.y); q.z = bswap(q.z); q.w = bswap(q.w); }
    store_payload_as<NTS>(a.payload + idx / 4, q);
}

// Exponents, quantize and pack of one loaded tile (K3: `e` holds the global
// exponents already).
template <int P, bool GLOBAL, bool BE, bool RNE, int U, bool NTS, class T>
__device__ __forceinline__ void quant_tile(const QuantArgs<T>& a, uint64_t base, int lane, const f4 (&v)[U],
                                           const float* lut, int (&e)[U]) {
    const uint64_t padded = a.nblocks * P;
    constexpr int kElems = tile_elems<U>();
    if constexpr (!GLOBAL) {
        tile_exponents<P>(v, e);
        // Written out here and in roundtrip_compute: behind a helper hipcc
        // orders the scalar instructions around the one-store form's exponent
        // store differently in every instance with 2 or 4 packets per tile
        // (DESIGN §11), and the measured fp32 code is kept as it is.
        if (a.exps_out) {
            constexpr int kPk = kElems / P;       // packets per tile
            if (((uintptr_t)a.exps_out & (kPk - 1)) == 0 && base + kElems <= padded) {
                store_tile_exponents<P>(a.exps_out + base / P, lane, e);
            } else {
                store_exponents<P>(a.exps_out, base, lane, e, a.nblocks);
            }
        }
    }
    if (!a.payload) return;
    // A tile inside the padded plane takes a branch-free slice loop.  With a
    // per-slice `continue` here, hipcc's wait-count pass sees paths that skip
    // a slice and waits vmcnt(0) at the top of EVERY slice — i.e. on the
    // previous slice's store as well — which cost K3 (whose first use of the
    // loaded data is inside this loop) 3 % against K1 (whose exponent reduce
    // consumes all four slices first): profiles/r02/k1_vs_k3_counters.json,
    // ab_k3_waitcnt.json.
    if (base + kElems <= padded) {
#pragma unroll
        for (int u = 0; u < U; u++) quant_slice<P, BE, RNE, NTS>(a, base + (uint64_t)(u * kWave + lane) * 4, v[u], lut, e[u]);
        return;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
        if (idx < padded) quant_slice<P, BE, RNE, NTS>(a, idx, v[u], lut, e[u]);
    }
}

// K1 (fused exponent + quantize + pack), K2 (exponents only: payload == nullptr)
// and K3 (given global exponents: GLOBAL = true).  A wave's tile is U slices
// of 256 elements (one vector load per lane per slice, all issued before any
// arithmetic); U = 4 by default — four loads in flight per lane keep the
// stream at the copy rate, smaller tiles measured slower.
template <int P, class E, bool GLOBAL, bool BE, bool RNE, int U, bool NTS = false>
__global__ __launch_bounds__(kBlockThreads) void k_quantize_pack(QuantArgs<typename E::raw> a) {
    __shared__ float lut[256];
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    // The wave's first tile is loaded BEFORE the workgroup builds its scale
    // table: the table and its barrier run while the loads are in flight (a
    // plain s_barrier does not wait for them), instead of delaying the first
    // HBM request of every workgroup of the one-shot grid: K1 +1.1 / +1.7 %
    // at 256 / 128 MiB (profiles/r04/ab_lut_early.json).
    uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index();
    f4 v[U];
    if (t < a.ntiles) load_tile<E>(a, t * tile_elems<U>(), lane, v);
    if (a.payload) build_lut(lut, a.W);
    while (t < a.ntiles) {
        const uint64_t base = t * tile_elems<U>();
        int e[U];
        // K3: the exponent dword is read after the data loads are in flight
        if constexpr (GLOBAL) global_tile_exponents<P>(a, base, lane, e);
        quant_tile<P, GLOBAL, BE, RNE, U, NTS>(a, base, lane, v, lut, e);
        t += nwaves;
        if (t < a.ntiles) load_tile<E>(a, t * tile_elems<U>(), lane, v);
    }
}

template <class T>
struct DequantArgs {
    const u4* payload;
    const int8_t* exps;
    T* out;
    uint64_t numel;
    uint64_t ntiles;        // ceil(numel / tile_elems<U>())
    uint32_t W;
    uint32_t xcd;           // xcd_block chunk (0 = plain order)
};

// K4: dequantize the aggregated payload (PostprocessSingle, ppp.cc:197-251).
// RCP (power-of-two W): multiply by the exact reciprocal instead of the IEEE
// division — same bits (rcp_scale_pow2).
template <int P, class E, bool BE, bool RCP, bool NT = false, int U = kU>
__global__ __launch_bounds__(kBlockThreads) void k_dequantize(DequantArgs<typename E::raw> a) {
    __shared__ float lut[256];
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    constexpr int kElems = tile_elems<U>();
    uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index();
    if constexpr (RCP) build_rcp_lut(lut, a.W);
    else build_lut(lut, a.W);
    for (; t < a.ntiles; t += nwaves) {
        const uint64_t base = t * kElems;
        const bool full = base + kElems <= a.numel;
        u4 w[U];
        float s[U];
        if (full && slice_exps_scalar_ok<P>(a.exps)) {
            // Full tile: each slice's exponent bytes with one scalar load
            // (measured: a per-lane byte load per slice costs ~8 % at
            // P != 256), then a branch-free slice loop — shared per-slice
            // blocks with the partial-tile path made hipcc wait vmcnt(0), on
            // the previous slice's store too, before every slice.
#pragma unroll
            for (int u = 0; u < U; u++) {
                w[u] = __builtin_nontemporal_load(a.payload + (base + (uint64_t)(u * kWave + lane) * 4) / 4);
                s[u] = lut[slice_exponent_byte<P>(a.exps, base, u, lane)];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
                E::template store4<NT>(a.out + idx, dequant_words<BE, RCP>(w[u], s[u]));
            }
            continue;
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
                if (full || idx < a.numel) {
                    w[u] = __builtin_nontemporal_load(a.payload + idx / 4);
                    s[u] = lut[(uint8_t)a.exps[idx / P]];
                }
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

template <class T>
struct RoundTripArgs {
    const T* in;
    T* out;
    uint64_t numel;
    uint64_t nblocks;
    uint64_t ntiles;        // ceil(B*P / tile_elems<U>())
    u4* payload;            // nullable: on-wire plane as sent
    int8_t* exps_out;       // nullable
    uint32_t W;
    uint32_t xcd;           // xcd_block chunk (0 = plain order)
};

// Fused dummy-backend round trip: PreprocessSingle -> ProcessPacket (x W) ->
// PostprocessSingle for every packet of the slice in one HBM pass.  One tile
// of one slice (blocks restart at the slice start, as in the reference):
// load_tile issues the tile's loads, roundtrip_compute does the rest.  A lane
// stores exactly the elements it loaded, after their loads, so in == out is
// safe.
template <int P, class E, bool BE, bool RNE, bool NT, int U>
__device__ __forceinline__ void roundtrip_compute(const RoundTripArgs<typename E::raw>& a, uint64_t t,
                                                  const float* lut, int lane, const f4 (&v)[U]) {
    static_assert(U * 256 >= P, "a tile holds whole packets");
    constexpr int kElems = tile_elems<U>();
    const bool pow2 = (a.W & (a.W - 1)) == 0;
    const uint32_t log2W = 31 - __builtin_clz(a.W);
    const uint64_t padded = a.nblocks * P;
    const uint64_t base = t * kElems;
    const bool full = base + kElems <= a.numel;
    int e[U];
    tile_exponents<P>(v, e);
    if (a.exps_out) {
        constexpr int kPk = kElems / P;
        if (((uintptr_t)a.exps_out & (kPk - 1)) == 0 && base + kElems <= padded)
            store_tile_exponents<P>(a.exps_out + base / P, lane, e);
        else
            store_exponents<P>(a.exps_out, base, lane, e, a.nblocks);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
        if (idx >= padded) continue;
        const float s = lut[(uint8_t)e[u]];
        uint64_t body = 0;
        if constexpr (RNE) body = vcl_body<P>(idx, a.numel);
        const u4 qv = quantize4<RNE>(v[u], s, idx, body);
        const uint32_t q[4] = {qv.x, qv.y, qv.z, qv.w};
        if (a.payload) {
            u4 wq = BE ? mku4(bswap(q[0]), bswap(q[1]), bswap(q[2]), bswap(q[3]))
                          : mku4(q[0], q[1], q[2], q[3]);
            store_payload(a.payload + idx / 4, wq);
        }
        // DummyBackend::ProcessPacket: int32 wrap multiply by W; then the
        // dequantize (exact reciprocal multiply for power-of-two W, as K4), on
        // the four scalar words: through dequant_words on a vector, hipcc's
        // block layout of the fp32 instances changes.
        f4 o;
        if (pow2) {
            const float r = rcp_scale_pow2(log2W, e[u]);
            o = mkf4(dequant1<true>(q[0] * a.W, r), dequant1<true>(q[1] * a.W, r), dequant1<true>(q[2] * a.W, r),
                     dequant1<true>(q[3] * a.W, r));
        } else {
            o = mkf4(dequant1<false>(q[0] * a.W, s), dequant1<false>(q[1] * a.W, s), dequant1<false>(q[2] * a.W, s),
                     dequant1<false>(q[3] * a.W, s));
        }
        if (full) E::template store4<NT>(a.out + idx, o);
        else if (idx < a.numel) E::store4_guarded(a.out + idx, o, idx, a.numel);
    }
}

template <int P, class E, bool BE, bool RNE, bool NT = false, int U = kU>
__device__ __forceinline__ void roundtrip_tile(const RoundTripArgs<typename E::raw>& a, uint64_t t, const float* lut,
                                               int lane) {
    f4 v[U];
    load_tile<E>(a, t * tile_elems<U>(), lane, v);
    roundtrip_compute<P, E, BE, RNE, NT, U>(a, t, lut, lane, v);
}

template <int P, class E, bool BE, bool RNE, bool NT = false, int U = kU>
__global__ __launch_bounds__(kBlockThreads) void k_roundtrip(RoundTripArgs<typename E::raw> a) {
    __shared__ float lut[256];
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index();
    // As K1: the first tile's loads go out before the scale table is built
    // (measured level here, +0.1-0.3 %: profiles/r04/ab_lut_early2.json).
    f4 v[U];
    if (t < a.ntiles) load_tile<E>(a, t * tile_elems<U>(), lane, v);
    build_lut(lut, a.W);
    while (t < a.ntiles) {
        roundtrip_compute<P, E, BE, RNE, NT, U>(a, t, lut, lane, v);
        t += nwaves;
        if (t < a.ntiles) load_tile<E>(a, t * tile_elems<U>(), lane, v);
    }
}

// The fused round trip over a batch of slices (of one or several jobs) in ONE
// launch: the slices' tiles are numbered consecutively (tile_end[s] = tiles of
// slices 0..s), each wave finds its slice by a binary search over that
// wave-uniform table (kernel arguments, scalar loads) and runs the slice's
// own block geometry.  Slices start at any element (FIFO slices, pinned host
// tensors): fp32 takes the unaligned form, which streams at the aligned rate,
// a 16-bit type its one form.  1808 bytes of kernel arguments for every T.
template <class T>
struct RoundTripBatchArgs {
    const T* in[SML_MAX_BATCH_SLICES];
    T* out[SML_MAX_BATCH_SLICES];
    uint64_t numel[SML_MAX_BATCH_SLICES];
    uint32_t tile_end[SML_MAX_BATCH_SLICES];
    uint32_t nslices;
    uint32_t W;
    uint32_t xcd;
};
static_assert(sizeof(RoundTripBatchArgs<float>) <= 4096 && sizeof(RoundTripBatchArgs<uint16_t>) == sizeof(RoundTripBatchArgs<float>),
              "the table travels as kernel arguments");

template <int P, class E, bool RNE, bool NT = false, int U = kU>
__global__ __launch_bounds__(kBlockThreads) void k_roundtrip_batch(RoundTripBatchArgs<typename E::raw> a) {
    __shared__ float lut[256];
    build_lut(lut, a.W);
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    const uint32_t ntiles = a.tile_end[a.nslices - 1];
    for (uint32_t t = (uint32_t)xcd_block(a.xcd) * kWavesPerBlock + wave_index(); t < ntiles; t += nwaves) {
        uint32_t lo = 0, hi = a.nslices - 1;             // first s with tile_end[s] > t
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.tile_end[mid] > t) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t t0 = lo ? a.tile_end[lo - 1] : 0u;
        RoundTripArgs<typename E::raw> r;
        r.in = a.in[lo];
        r.out = a.out[lo];
        r.numel = a.numel[lo];
        r.nblocks = r.numel / P + (r.numel % P != 0);
        r.ntiles = a.tile_end[lo] - t0;
        r.payload = nullptr;
        r.exps_out = nullptr;
        r.W = a.W;
        r.xcd = a.xcd;
        roundtrip_tile<P, E, true, RNE, NT, U>(r, t - t0, lut, lane);
    }
}

// ------------------------------------------------------------ host side
//
// One set-up per kernel, for every element type: EV<V> is the element policy
// of the slice's variant V (fp32: 16-byte aligned or not; 16-bit: FLOAT16 or
// BFLOAT16), U the tile's slices, Us the slice counts the type instantiates.

template <class T>
inline bool elem_aligned(const T* p) { return ((uintptr_t)p & (sizeof(T) - 1)) == 0; }

template <template <bool> class EV, int... Us, class T>
sml_status_t plane_quantize(const T* d_in, bool variant, uint32_t U, uint64_t numel, uint32_t P, uint16_t W,
                            const int8_t* d_gexp, int32_t* d_payload, int8_t* d_exps_out, uint32_t flags,
                            void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (numel == 0) return SML_OK;
    if (!d_in || !elem_aligned(d_in)) return SML_ERR_INVALID_ARG;
    if (d_payload && !aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    QuantArgs<T> a;
    a.xcd = xcd_chunk_for(U);
    a.in = d_in;
    a.numel = numel;
    a.nblocks = sml_num_blocks(numel, P);
    const uint64_t te = 256ull * U;
    a.ntiles = (a.nblocks * P + te - 1) / te;
    a.gexp = d_gexp;
    a.payload = reinterpret_cast<u4*>(d_payload);
    a.exps_out = d_gexp ? nullptr : d_exps_out;
    a.W = W;
    dim3 grid(grid_for_tiles(a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE), rne = flags & SML_FLAG_ROUND_RNE;
    // payload store policy by plane size
    const bool nts = d_payload && nt_from(4 * numel);
    // Flags outermost, the store policy innermost: the order in which the
    // instances are created.  hipcc's code for twelve fp32 K3 instances (P =
    // 128 / 256, one slice) differs with it — registers and block layout, same
    // arithmetic — and this order gives the code that was measured.
    dispatch_bools([&](auto GLOBAL, auto V, auto BE, auto RNE) {
        dispatch_packet(P, [&](auto Pc) {
            dispatch_slices<Us...>(U, [&](auto Uc) {
                dispatch_bools([&](auto NTS) {
                    // a tile holds whole packets: fewer than P / 256 slices cannot
                    // occur (the callers' U) and would run 4
                    constexpr int kUc = Uc() * 256 >= Pc() ? Uc() : 4;
                    k_quantize_pack<Pc(), EV<V()>, GLOBAL(), BE(), RNE(), kUc, NTS()><<<grid, kBlockThreads, 0, st>>>(a);
                }, nts);
            });
        });
    }, d_gexp != nullptr, variant, be, rne);
    return launch_check();
}

template <template <bool> class EV, int... Us, class T>
sml_status_t plane_dequantize(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel, uint32_t P, uint16_t W,
                              T* d_out, bool variant, uint32_t U, uint32_t flags, void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (W == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!d_payload || !d_exps || !d_out || !elem_aligned(d_out)) return SML_ERR_INVALID_ARG;
    if (!aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    DequantArgs<T> a;
    a.xcd = xcd_chunk_for(U);
    a.payload = reinterpret_cast<const u4*>(d_payload);
    a.exps = d_exps;
    a.out = d_out;
    a.numel = numel;
    a.ntiles = (numel + 256 * U - 1) / (256 * U);
    a.W = W;
    dim3 grid(grid_for_tiles(a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE);
    const bool rcp = (a.W & (a.W - 1)) == 0;     // power-of-two W: exact reciprocal
    const bool nt = nt_from(sizeof(T) * numel);  // output plane past the Infinity Cache
    dispatch_packet(P, [&](auto Pc) {
        dispatch_slices<Us...>(U, [&](auto Uc) {
            dispatch_bools([&](auto V, auto BE, auto RCP, auto NT) {
                k_dequantize<Pc(), EV<V()>, BE(), RCP(), NT(), Uc()><<<grid, kBlockThreads, 0, st>>>(a);
            }, variant, be, rcp, nt);
        });
    });
    return launch_check();
}

template <template <bool> class EV, int... Us, class T>
sml_status_t plane_roundtrip(const T* d_in, T* d_out, bool variant, uint32_t U, uint64_t numel, uint32_t P,
                             uint16_t W, int32_t* d_payload, int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (!valid_packet(P)) return SML_ERR_UNSUPPORTED;
    if (W == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!d_in || !d_out || !elem_aligned(d_in) || !elem_aligned(d_out)) return SML_ERR_INVALID_ARG;
    if (d_payload && !aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    RoundTripArgs<T> a;
    a.xcd = xcd_chunk_for(U);
    a.in = d_in;
    a.out = d_out;
    a.numel = numel;
    a.nblocks = sml_num_blocks(numel, P);
    a.ntiles = (a.nblocks * P + 256 * U - 1) / (256 * U);
    a.payload = reinterpret_cast<u4*>(d_payload);
    a.exps_out = d_exps_out;
    a.W = W;
    dim3 grid(grid_for_tiles(a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE), rne = flags & SML_FLAG_ROUND_RNE;
    const bool nt = nt_from(sizeof(T) * numel);   // output plane past the Infinity Cache
    dispatch_packet(P, [&](auto Pc) {
        dispatch_slices<Us...>(U, [&](auto Uc) {
            dispatch_bools([&](auto V, auto BE, auto RNE, auto NT) {
                // P = 1024 always runs 4 slices (the callers' U): a tile holds the packet
                constexpr int kUc = Pc() == 1024 ? 4 : Uc();
                k_roundtrip<Pc(), EV<V()>, BE(), RNE(), NT(), kUc><<<grid, kBlockThreads, 0, st>>>(a);
            }, variant, be, rne, nt);
        });
    });
    return launch_check();
}

// One slice into the table of a batched launch on tiles of `tile` elements
// (a table holds at most SML_MAX_BATCH_SLICES: the callers' check).  Empty
// slices touch nothing and take no entry.
template <class T>
sml_status_t batch_add(RoundTripBatchArgs<T>& a, uint64_t& tiles, const void* in, void* out, uint64_t numel, uint32_t P,
                       uint64_t tile) {
    if (numel == 0) return SML_OK;
    const T* i = static_cast<const T*>(in);
    T* o = static_cast<T*>(out);
    if (!i || !o || !elem_aligned(i) || !elem_aligned(o)) return SML_ERR_INVALID_ARG;
    tiles += (sml_num_blocks(numel, P) * P + tile - 1) / tile;
    if (tiles > 0xFFFFFFFFull) return SML_ERR_UNSUPPORTED;
    a.in[a.nslices] = i;
    a.out[a.nslices] = o;
    a.numel[a.nslices] = numel;
    a.tile_end[a.nslices] = (uint32_t)tiles;
    a.nslices++;
    return SML_OK;
}

// The fp32 batched launch (sml_quantizer.hip) in its two steps, for
// sml_roundtrip_loopback_batch_typed (sml_half.hip), which fills and checks
// the tables of every type before it launches any: the elements of an fp32
// batch tile for packets of P, and the launch of a filled table (one slice:
// the single-slice kernel) with non-temporal stores or not.
uint64_t batch_tile_f32(uint32_t P);
sml_status_t batch_launch_f32(RoundTripBatchArgs<float>& a, uint32_t P, uint16_t W, uint32_t flags, bool nt,
                              void* stream);

}  // namespace sml

#endif  // SML_PLANES_H_
