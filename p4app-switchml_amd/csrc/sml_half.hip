// sml_half.hip — FLOAT16 / BFLOAT16 job slices: the 16-bit instantiations of
// the plane kernels of sml_planes.h (K1h / K2h / K3h quantize + pack, K4h
// dequantize, the fused loopback round trip and its batched form) and the
// typed C-ABI entry points (include/switchml_hip.h, sml_*_typed).  The fp32
// instantiations are sml_quantizer.hip's.
//
// The switch carries int32 words, and the reference knows no 16-bit type; for
// the one type the switch does not carry (ncclUint8) its plugin widens on the
// way in and narrows on the way out (switchml_plugin.cc:328-337, 370-378).
// The same rule here, inside the streaming kernels: an element is widened to
// fp32 in registers right after its load (exact), everything between is the
// FLOAT32 path unchanged (block exponent, scale, roundf / VCL rounding,
// big-endian pack, dequantize), and the fp32 result is narrowed (round to
// nearest even) right before its store.  The wire format does not change:
// int32 payload words and one int8 exponent per packet of P elements, so
// B = ceil(numel / P) whatever the element size.
//
// Layout: the fp32 unit's tile — lane l of slice u holds elements
// [u*256 + 4l, +4), here one 8-byte load per lane per slice, four slices in
// flight (2 KiB per wave, the bytes the fp32 kernels keep in flight with two
// 16-byte slices) — so the per-packet reduce, the exponent stores and the
// payload stores are the fp32 unit's.  Slices start at any element: every
// typed access is declared 2-byte aligned (h4a, sml_device.h), and a partial
// last tile goes element by element, so no byte outside [ptr, ptr + 2 numel)
// is read or written.
#include "sml_planes.h"

namespace sml {

// Slices per tile, every kernel here (P = 1024 needs 4).  Against 2 and 8 at
// P = 256, 64 Mi elements cold (profiles/half/ab_slices.json): K1h 64.2 / 65.1
// / 68.2 us, K4h 61.0 / 61.9 / 62.8, the round trip 59.6 / 51.1 / 49.3.
constexpr int kHU = 4;

// The element policy of a 16-bit slice by its variant: FLOAT16 or BFLOAT16.
template <bool F16>
using ElemHalf = Elem16<F16 ? kHalfF16 : kHalfBF16>;

static sml_status_t quantize_common_h(const void* d_in, sml_data_type_t dt, uint64_t numel, uint32_t P, uint16_t W,
                                      const int8_t* d_gexp, int32_t* d_payload, int8_t* d_exps_out, uint32_t flags,
                                      void* stream) {
    return plane_quantize<ElemHalf, kHU>(static_cast<const uint16_t*>(d_in), dt == SML_FLOAT16, kHU, numel, P, W,
                                         d_gexp, d_payload, d_exps_out, flags, stream);
}

// The batched round trip of one 16-bit type: a filled table in one launch of
// k_roundtrip_batch on the single-slice kernels' kHU-slice tiles (one slice:
// the single-slice kernel, as the fp32 batch does).
static sml_status_t batch_launch_h(RoundTripBatchArgs<uint16_t>& a, bool f16, uint32_t P, uint16_t W, bool rne, bool nt,
                                   void* stream) {
    if (a.nslices == 0) return SML_OK;
    if (a.nslices == 1)
        return plane_roundtrip<ElemHalf, kHU>(a.in[0], a.out[0], f16, kHU, a.numel[0], P, W, nullptr, nullptr,
                                              rne ? SML_FLAG_ROUND_RNE : 0u, stream);
    a.xcd = xcd_chunk_for(kHU);
    a.W = W;
    const dim3 grid(grid_for_tiles(a.tile_end[a.nslices - 1]));
    hipStream_t st = (hipStream_t)stream;
    dispatch_packet(P, [&](auto Pc) {
        dispatch_bools([&](auto F16, auto RNE, auto NT) {
            k_roundtrip_batch<Pc(), ElemHalf<F16()>, RNE(), NT(), kHU><<<grid, kBlockThreads, 0, st>>>(a);
        }, f16, rne, nt);
    });
    return launch_check();
}

}  // namespace sml

using namespace sml;

extern "C" {

// SML_FLOAT32 is forwarded before any check made here, so the fp32 entry
// point's own checks, in its own order, decide the status (switchml_hip.h).
sml_status_t sml_exponents_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel, uint32_t packet_numel,
                                 int8_t* d_exps, void* stream) {
    if (data_type == SML_FLOAT32) return sml_exponents(static_cast<const float*>(d_in), numel, packet_numel, d_exps, stream);
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    if (numel && !d_exps) return SML_ERR_INVALID_ARG;
    return quantize_common_h(d_in, data_type, numel, packet_numel, 1, nullptr, nullptr, d_exps, 0, stream);
}

sml_status_t sml_quantize_pack_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel,
                                     uint32_t packet_numel, uint16_t num_workers, const int8_t* d_global_exps,
                                     int32_t* d_payload, int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (data_type == SML_FLOAT32)
        return sml_quantize_pack(static_cast<const float*>(d_in), numel, packet_numel, num_workers, d_global_exps,
                                 d_payload, d_exps_out, flags, stream);
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
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
    if (data_type == SML_FLOAT32)
        return sml_dequantize(d_payload, d_exps, numel, packet_numel, num_workers, static_cast<float*>(d_out), flags,
                              stream);
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    return plane_dequantize<ElemHalf, kHU>(d_payload, d_exps, numel, packet_numel, num_workers,
                                           static_cast<uint16_t*>(d_out), data_type == SML_FLOAT16, kHU, flags,
                                           stream);
}

sml_status_t sml_roundtrip_loopback_typed(const void* d_in, void* d_out, sml_data_type_t data_type, uint64_t numel,
                                          uint32_t packet_numel, uint16_t num_workers, int32_t* d_payload,
                                          int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (data_type == SML_FLOAT32)
        return sml_roundtrip_loopback(static_cast<const float*>(d_in), static_cast<float*>(d_out), numel, packet_numel,
                                      num_workers, d_payload, d_exps_out, flags, stream);
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    return plane_roundtrip<ElemHalf, kHU>(static_cast<const uint16_t*>(d_in), static_cast<uint16_t*>(d_out),
                                          data_type == SML_FLOAT16, kHU, numel, packet_numel, num_workers, d_payload,
                                          d_exps_out, flags, stream);
}

sml_status_t sml_roundtrip_loopback_batch_typed(const sml_typed_slice* slices, uint32_t num_slices,
                                                uint32_t packet_numel, uint16_t num_workers, uint32_t flags,
                                                void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (num_workers == 0 || num_slices > SML_MAX_BATCH_SLICES || (num_slices && !slices)) return SML_ERR_INVALID_ARG;
    // One table per element type, every slice checked before any launch.
    RoundTripBatchArgs<float> f32;
    RoundTripBatchArgs<uint16_t> h[2];   // [0] BFLOAT16, [1] FLOAT16
    f32.nslices = h[0].nslices = h[1].nslices = 0;
    uint64_t tiles_f32 = 0, tiles_h[2] = {0, 0}, out_bytes = 0;
    for (uint32_t i = 0; i < num_slices; i++) {
        const sml_typed_slice& sl = slices[i];
        if (sl.reserved != 0) return SML_ERR_INVALID_ARG;
        sml_status_t s;
        if (sl.data_type == SML_FLOAT32) {
            s = batch_add(f32, tiles_f32, sl.in, sl.out, sl.numel, packet_numel, batch_tile_f32(packet_numel));
            out_bytes += 4 * sl.numel;
        } else if (sl.data_type == SML_FLOAT16 || sl.data_type == SML_BFLOAT16) {
            const int k = sl.data_type == SML_FLOAT16;
            s = batch_add(h[k], tiles_h[k], sl.in, sl.out, sl.numel, packet_numel, (uint64_t)tile_elems<kHU>());
            out_bytes += 2 * sl.numel;
        } else {
            return SML_ERR_UNSUPPORTED;
        }
        if (s != SML_OK) return s;
    }
    // the outputs of the whole call past the Infinity Cache: non-temporal stores
    const bool rne = flags & SML_FLAG_ROUND_RNE, nt = nt_from(out_bytes);
    sml_status_t s = batch_launch_f32(f32, packet_numel, num_workers, flags, nt, stream);
    for (int k = 0; k < 2 && s == SML_OK; k++)
        s = batch_launch_h(h[k], k == 1, packet_numel, num_workers, rne, nt, stream);
    return s;
}

}  // extern "C"
