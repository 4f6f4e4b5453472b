// sml_half.hip — FLOAT16 / BFLOAT16 job slices: the 16-bit counterparts of
// the plane kernels of sml_quantizer.hip (K1h / K2h / K3h quantize + pack,
// K4h dequantize, the fused loopback round trip) and the typed C-ABI entry
// points (include/switchml_hip.h, sml_*_typed).
//
// The switch carries int32 words, and the reference knows no 16-bit type; for
// the one type the switch does not carry (ncclUint8) its plugin widens on the
// way in and narrows on the way out (switchml_plugin.cc:328-337, 370-378).
// The same rule here, inside the streaming kernels: an element is widened to
// fp32 in registers right after its load (exact), everything between is the
// FLOAT32 path of sml_device.h unchanged (block exponent, scale, roundf / VCL
// rounding, big-endian pack, dequantize), and the fp32 result is narrowed
// (round to nearest even) right before its store.  The wire format does not
// change: int32 payload words and one int8 exponent per packet of P elements,
// so B = ceil(numel / P) whatever the element size.
//
// Layout: the fp32 unit's tile — lane l of slice u holds elements
// [u*256 + 4l, +4), here one 8-byte load per lane per slice, four slices in
// flight (2 KiB per wave, the bytes the fp32 kernels keep in flight with two
// 16-byte slices) — so the per-packet reduce, the exponent stores and the
// payload stores are the fp32 unit's.  Slices start at any element: every
// typed access is declared 2-byte aligned (h4a, sml_device.h), and a partial
// last tile goes element by element, so no byte outside [ptr, ptr + 2 numel)
// is read or written.
#include "sml_host.h"

namespace sml {

// Slices per tile, every kernel here (P = 1024 needs 4).  Against 2 and 8 at
// P = 256, 64 Mi elements cold (profiles/half/ab_slices.json): K1h 64.2 / 65.1
// / 68.2 us, K4h 61.0 / 61.9 / 62.8, the round trip 59.6 / 51.1 / 49.3.
constexpr int kHU = 4;
constexpr int kHElems = tile_elems<kHU>();     // 1024

struct HalfQuantArgs {
    const uint16_t* in;
    uint64_t numel;
    uint64_t nblocks;       // B
    uint64_t ntiles;        // ceil(B*P / 1024)
    const int8_t* gexp;     // global exponents (K3h) or nullptr (K1h)
    u4* payload;            // B*P words, 16-B aligned (nullptr: exponents only, K2h)
    int8_t* exps_out;       // nullable
    uint32_t W;
    uint32_t xcd;
};

template <int H, int U>
__device__ __forceinline__ void load_tile_h(const uint16_t* in, uint64_t numel, uint64_t base, int lane, f4 (&v)[U]) {
    if (base + tile_elems<U>() <= numel) {
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = load4h<H>(in + base + (u * kWave + lane) * 4);
    } else {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
            v[u] = load4h_guarded<H>(in + idx, idx, numel);
        }
    }
}

// VCL body end of the block holding idx (quant_slice of the fp32 unit): the
// first n - n % 16 elements of the block round to nearest even.
template <int P>
__device__ __forceinline__ uint64_t rne_body(uint64_t idx, uint64_t numel) {
    const uint64_t blk0 = idx / P * P;
    const uint64_t n = numel - blk0 < (uint64_t)P ? numel - blk0 : (uint64_t)P;
    return blk0 + (n - n % 16);
}

// The block exponents of a loaded tile, written to exps_out when given.
template <int P, int U>
__device__ __forceinline__ void own_exponents(const f4 (&v)[U], int (&e)[U], int8_t* exps_out, uint64_t base,
                                              int lane, uint64_t nblocks) {
    tile_exponents<P>(v, e);
    if (!exps_out) return;
    constexpr int kPk = tile_elems<U>() / P;
    if (((uintptr_t)exps_out & (kPk - 1)) == 0 && base + tile_elems<U>() <= nblocks * P)
        store_tile_exponents<P>(exps_out + base / P, lane, e);
    else
        store_exponents<P>(exps_out, base, lane, e, nblocks);
}

// K1h (fused exponent + quantize + pack), K2h (payload == nullptr) and K3h
// (GLOBAL: given exponents) — k_quantize_pack on a 16-bit input.
template <int H, int P, bool GLOBAL, bool BE, bool RNE, bool NTS>
__global__ __launch_bounds__(kBlockThreads) void k_quantize_pack_h(HalfQuantArgs a) {
    __shared__ float lut[256];
    constexpr int U = kHU;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t padded = a.nblocks * P;
    // as K1: the first tile's loads go out before the scale table is built
    uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index();
    f4 v[U];
    if (t < a.ntiles) load_tile_h<H>(a.in, a.numel, t * kHElems, lane, v);
    if (a.payload) build_lut(lut, a.W);
    while (t < a.ntiles) {
        const uint64_t base = t * kHElems;
        int e[U];
        if constexpr (GLOBAL) {
            if (base + kHElems <= padded && slice_exps_scalar_ok<P>(a.gexp)) {
#pragma unroll
                for (int u = 0; u < U; u++) e[u] = (int)(int8_t)slice_exponent_byte<P>(a.gexp, base, u, lane);
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint64_t pkt = (base + (uint64_t)(u * kWave + lane) * 4) / P;
                    e[u] = pkt < a.nblocks ? (int)a.gexp[pkt] : 0;
                }
            }
        } else {
            own_exponents<P>(v, e, a.exps_out, base, lane, a.nblocks);
        }
        if (a.payload) {
            auto quant_slice = [&](int u, uint64_t idx) {
                u4 q = quantize4<RNE>(v[u], lut[(uint8_t)e[u]], idx, RNE ? rne_body<P>(idx, a.numel) : 0);
                if constexpr (BE) { q.x = bswap(q.x); q.y = bswap(q.y); q.z = bswap(q.z); q.w = bswap(q.w); }
                store_payload_as<NTS>(a.payload + idx / 4, q);
            };
            // a tile inside the padded plane takes a branch-free slice loop
            // (the fp32 unit's quant_tile says why)
            if (base + kHElems <= padded) {
#pragma unroll
                for (int u = 0; u < U; u++) quant_slice(u, base + (uint64_t)(u * kWave + lane) * 4);
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
                    if (idx < padded) quant_slice(u, idx);
                }
            }
        }
        t += nwaves;
        if (t < a.ntiles) load_tile_h<H>(a.in, a.numel, t * kHElems, lane, v);
    }
}

// ntohl (BE) -> int -> float, divided by the scale or multiplied by its exact
// reciprocal (power-of-two W): PostprocessSingle's per-element arithmetic, as
// the fp32 unit's dequant_words.
template <bool BE, bool RCP>
__device__ __forceinline__ f4 dequant_words_h(u4 w, float s) {
    if constexpr (BE) { w.x = bswap(w.x); w.y = bswap(w.y); w.z = bswap(w.z); w.w = bswap(w.w); }
    if constexpr (RCP)
        return mkf4((float)(int32_t)w.x * s, (float)(int32_t)w.y * s, (float)(int32_t)w.z * s, (float)(int32_t)w.w * s);
    else
        return mkf4(dequantize1(w.x, s), dequantize1(w.y, s), dequantize1(w.z, s), dequantize1(w.w, s));
}

struct HalfDequantArgs {
    const u4* payload;
    const int8_t* exps;
    uint16_t* out;
    uint64_t numel;
    uint64_t ntiles;        // ceil(numel / 1024)
    uint32_t W;
    uint32_t xcd;
};

// K4h: k_dequantize with a 16-bit output.
template <int H, int P, bool BE, bool RCP, bool NT>
__global__ __launch_bounds__(kBlockThreads) void k_dequantize_h(HalfDequantArgs a) {
    __shared__ float lut[256];
    constexpr int U = kHU;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    if constexpr (RCP) build_rcp_lut(lut, a.W);
    else build_lut(lut, a.W);
    for (uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index(); t < a.ntiles; t += nwaves) {
        const uint64_t base = t * kHElems;
        u4 w[U];
        float s[U];
        if (base + kHElems <= a.numel && slice_exps_scalar_ok<P>(a.exps)) {
            // full tile: one scalar exponent load per slice, branch-free stores
#pragma unroll
            for (int u = 0; u < U; u++) {
                w[u] = __builtin_nontemporal_load(a.payload + (base + (uint64_t)(u * kWave + lane) * 4) / 4);
                s[u] = lut[slice_exponent_byte<P>(a.exps, base, u, lane)];
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                store4h<H, NT>(a.out + base + (uint64_t)(u * kWave + lane) * 4, dequant_words_h<BE, RCP>(w[u], s[u]));
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
            if (idx >= a.numel) continue;
            const u4 q = __builtin_nontemporal_load(a.payload + idx / 4);
            const f4 o = dequant_words_h<BE, RCP>(q, lut[(uint8_t)a.exps[idx / P]]);
            store4h_guarded<H>(a.out + idx, o, idx, a.numel);
        }
    }
}

struct HalfRoundTripArgs {
    const uint16_t* in;
    uint16_t* out;
    uint64_t numel;
    uint64_t nblocks;
    uint64_t ntiles;        // ceil(B*P / 1024)
    u4* payload;            // nullable: on-wire plane as sent
    int8_t* exps_out;       // nullable
    uint32_t W;
    uint32_t xcd;
};

// The fused loopback round trip (k_roundtrip) on 16-bit elements: widen ->
// PreprocessSingle -> ProcessPacket (x W) -> PostprocessSingle -> narrow in
// one HBM pass.  A lane stores exactly the elements it loaded, after their
// loads, so in == out is safe.
template <int H, int P, bool BE, bool RNE, bool NT>
__global__ __launch_bounds__(kBlockThreads) void k_roundtrip_h(HalfRoundTripArgs a) {
    __shared__ float lut[256];
    constexpr int U = kHU;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const bool pow2 = (a.W & (a.W - 1)) == 0;
    const uint32_t log2W = 31 - __builtin_clz(a.W);
    const uint64_t padded = a.nblocks * P;
    uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index();
    f4 v[U];
    if (t < a.ntiles) load_tile_h<H>(a.in, a.numel, t * kHElems, lane, v);
    build_lut(lut, a.W);
    while (t < a.ntiles) {
        const uint64_t base = t * kHElems;
        const bool full = base + kHElems <= a.numel;
        int e[U];
        own_exponents<P>(v, e, a.exps_out, base, lane, a.nblocks);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t idx = base + (uint64_t)(u * kWave + lane) * 4;
            if (idx >= padded) continue;
            const float s = lut[(uint8_t)e[u]];
            const u4 q = quantize4<RNE>(v[u], s, idx, RNE ? rne_body<P>(idx, a.numel) : 0);
            if (a.payload)
                store_payload(a.payload + idx / 4, BE ? mku4(bswap(q.x), bswap(q.y), bswap(q.z), bswap(q.w)) : q);
            // DummyBackend::ProcessPacket: int32 wrap multiply by W; then the
            // dequantize (exact reciprocal multiply for power-of-two W, as K4)
            f4 o;
            if (pow2) {
                const float r = rcp_scale_pow2(log2W, e[u]);
                o = mkf4((float)(int32_t)(q.x * a.W) * r, (float)(int32_t)(q.y * a.W) * r,
                         (float)(int32_t)(q.z * a.W) * r, (float)(int32_t)(q.w * a.W) * r);
            } else {
                o = mkf4(dequantize1(q.x * a.W, s), dequantize1(q.y * a.W, s), dequantize1(q.z * a.W, s),
                         dequantize1(q.w * a.W, s));
            }
            if (full) store4h<H, NT>(a.out + idx, o);
            else if (idx < a.numel) store4h_guarded<H>(a.out + idx, o, idx, a.numel);
        }
        t += nwaves;
        if (t < a.ntiles) load_tile_h<H>(a.in, a.numel, t * kHElems, lane, v);
    }
}

// 16-bit type -> its compile-time constant (callers have checked it is one).
template <class F>
inline void dispatch_half(sml_data_type_t dt, F&& f) {
    if (dt == SML_FLOAT16) f(int_c<kHalfF16>{});
    else f(int_c<kHalfBF16>{});
}

inline bool is_half(sml_data_type_t dt) { return dt == SML_FLOAT16 || dt == SML_BFLOAT16; }
inline bool aligned2(const void* p) { return ((uintptr_t)p & 1u) == 0; }

static sml_status_t quantize_common_h(const void* d_in, sml_data_type_t dt, uint64_t numel, uint32_t P, uint16_t W,
                                      const int8_t* d_gexp, int32_t* d_payload, int8_t* d_exps_out, uint32_t flags,
                                      void* stream) {
    if (numel == 0) return SML_OK;
    if (!d_in || !aligned2(d_in)) return SML_ERR_INVALID_ARG;
    if (d_payload && !aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    HalfQuantArgs a;
    a.xcd = xcd_chunk_for(kHU);
    a.in = static_cast<const uint16_t*>(d_in);
    a.numel = numel;
    a.nblocks = sml_num_blocks(numel, P);
    a.ntiles = (a.nblocks * P + kHElems - 1) / kHElems;
    a.gexp = d_gexp;
    a.payload = reinterpret_cast<u4*>(d_payload);
    a.exps_out = d_gexp ? nullptr : d_exps_out;
    a.W = W;
    const dim3 grid(grid_for_tiles(a.ntiles));
    const hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE), rne = flags & SML_FLAG_ROUND_RNE;
    const bool nts = d_payload && nt_from(4 * numel);   // payload store policy by plane size
    dispatch_half(dt, [&](auto Hc) {
        dispatch_packet(P, [&](auto Pc) {
            dispatch_bools([&](auto GLOBAL, auto BE, auto RNE, auto NTS) {
                k_quantize_pack_h<Hc(), Pc(), GLOBAL(), BE(), RNE(), NTS()><<<grid, kBlockThreads, 0, st>>>(a);
            }, d_gexp != nullptr, be, rne, nts);
        });
    });
    return launch_check();
}

}  // namespace sml

using namespace sml;

extern "C" {

sml_status_t sml_exponents_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel, uint32_t packet_numel,
                                 int8_t* d_exps, void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (data_type == SML_FLOAT32) return sml_exponents(static_cast<const float*>(d_in), numel, packet_numel, d_exps, stream);
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    if (numel && !d_exps) return SML_ERR_INVALID_ARG;
    return quantize_common_h(d_in, data_type, numel, packet_numel, 1, nullptr, nullptr, d_exps, 0, stream);
}

sml_status_t sml_quantize_pack_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel,
                                     uint32_t packet_numel, uint16_t num_workers, const int8_t* d_global_exps,
                                     int32_t* d_payload, int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (data_type == SML_FLOAT32)
        return sml_quantize_pack(static_cast<const float*>(d_in), numel, packet_numel, num_workers, d_global_exps,
                                 d_payload, d_exps_out, flags, stream);
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel && !d_payload) return SML_ERR_INVALID_ARG;
    if (d_global_exps && d_exps_out && d_exps_out != d_global_exps) return SML_ERR_INVALID_ARG;
    return quantize_common_h(d_in, data_type, numel, packet_numel, num_workers, d_global_exps, d_payload, d_exps_out,
                             flags, stream);
}

sml_status_t sml_dequantize_typed(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel,
                                  uint32_t packet_numel, uint16_t num_workers, void* d_out,
                                  sml_data_type_t data_type, uint32_t flags, void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (data_type == SML_FLOAT32)
        return sml_dequantize(d_payload, d_exps, numel, packet_numel, num_workers, static_cast<float*>(d_out), flags,
                              stream);
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!d_payload || !d_exps || !d_out || !aligned2(d_out)) return SML_ERR_INVALID_ARG;
    if (!aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    HalfDequantArgs a;
    a.xcd = xcd_chunk_for(kHU);
    a.payload = reinterpret_cast<const u4*>(d_payload);
    a.exps = d_exps;
    a.out = static_cast<uint16_t*>(d_out);
    a.numel = numel;
    a.ntiles = (numel + kHElems - 1) / kHElems;
    a.W = num_workers;
    const dim3 grid(grid_for_tiles(a.ntiles));
    const hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE);
    const bool rcp = (a.W & (a.W - 1)) == 0;   // power-of-two W: exact reciprocal
    const bool nt = nt_from(2 * numel);        // output plane past the Infinity Cache
    dispatch_half(data_type, [&](auto Hc) {
        dispatch_packet(packet_numel, [&](auto Pc) {
            dispatch_bools([&](auto BE, auto RCP, auto NT) {
                k_dequantize_h<Hc(), Pc(), BE(), RCP(), NT()><<<grid, kBlockThreads, 0, st>>>(a);
            }, be, rcp, nt);
        });
    });
    return launch_check();
}

sml_status_t sml_roundtrip_loopback_typed(const void* d_in, void* d_out, sml_data_type_t data_type, uint64_t numel,
                                          uint32_t packet_numel, uint16_t num_workers, int32_t* d_payload,
                                          int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (data_type == SML_FLOAT32)
        return sml_roundtrip_loopback(static_cast<const float*>(d_in), static_cast<float*>(d_out), numel, packet_numel,
                                      num_workers, d_payload, d_exps_out, flags, stream);
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel == 0) return SML_OK;
    if (!d_in || !d_out || !aligned2(d_in) || !aligned2(d_out)) return SML_ERR_INVALID_ARG;
    if (d_payload && !aligned16(d_payload)) return SML_ERR_ALIGNMENT;
    HalfRoundTripArgs a;
    a.xcd = xcd_chunk_for(kHU);
    a.in = static_cast<const uint16_t*>(d_in);
    a.out = static_cast<uint16_t*>(d_out);
    a.numel = numel;
    a.nblocks = sml_num_blocks(numel, packet_numel);
    a.ntiles = (a.nblocks * packet_numel + kHElems - 1) / kHElems;
    a.payload = reinterpret_cast<u4*>(d_payload);
    a.exps_out = d_exps_out;
    a.W = num_workers;
    const dim3 grid(grid_for_tiles(a.ntiles));
    const hipStream_t st = (hipStream_t)stream;
    const bool be = !(flags & SML_FLAG_PAYLOAD_LE), rne = flags & SML_FLAG_ROUND_RNE;
    const bool nt = nt_from(2 * numel);   // output plane past the Infinity Cache
    dispatch_half(data_type, [&](auto Hc) {
        dispatch_packet(packet_numel, [&](auto Pc) {
            dispatch_bools([&](auto BE, auto RNE, auto NT) {
                k_roundtrip_h<Hc(), Pc(), BE(), RNE(), NT()><<<grid, kBlockThreads, 0, st>>>(a);
            }, be, rne, nt);
        });
    });
    return launch_check();
}

}  // extern "C"
