// sml_half.hip — FLOAT16 / BFLOAT16 job slices: the 16-bit instantiations of
// the plane kernels of sml_planes.h (K1h / K2h / K3h quantize + pack, K4h
// dequantize, the fused loopback round trip) and the typed C-ABI entry points
// (include/switchml_hip.h, sml_*_typed).  The fp32 instantiations are
// sml_quantizer.hip's.
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

inline bool is_half(sml_data_type_t dt) { return dt == SML_FLOAT16 || dt == SML_BFLOAT16; }

static sml_status_t quantize_common_h(const void* d_in, sml_data_type_t dt, uint64_t numel, uint32_t P, uint16_t W,
                                      const int8_t* d_gexp, int32_t* d_payload, int8_t* d_exps_out, uint32_t flags,
                                      void* stream) {
    return plane_quantize<ElemHalf, kHU>(static_cast<const uint16_t*>(d_in), dt == SML_FLOAT16, kHU, numel, P, W,
                                         d_gexp, d_payload, d_exps_out, flags, stream);
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
    return plane_dequantize<ElemHalf, kHU>(d_payload, d_exps, numel, packet_numel, num_workers,
                                           static_cast<uint16_t*>(d_out), data_type == SML_FLOAT16, kHU, flags,
                                           stream);
}

sml_status_t sml_roundtrip_loopback_typed(const void* d_in, void* d_out, sml_data_type_t data_type, uint64_t numel,
                                          uint32_t packet_numel, uint16_t num_workers, int32_t* d_payload,
                                          int8_t* d_exps_out, uint32_t flags, void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (data_type == SML_FLOAT32)
        return sml_roundtrip_loopback(static_cast<const float*>(d_in), static_cast<float*>(d_out), numel, packet_numel,
                                      num_workers, d_payload, d_exps_out, flags, stream);
    if (!is_half(data_type)) return SML_ERR_UNSUPPORTED;
    return plane_roundtrip<ElemHalf, kHU>(static_cast<const uint16_t*>(d_in), static_cast<uint16_t*>(d_out),
                                          data_type == SML_FLOAT16, kHU, numel, packet_numel, num_workers, d_payload,
                                          d_exps_out, flags, stream);
}

}  // extern "C"
