// sml_frames_half.hip — FLOAT16 / BFLOAT16 job slices over DPDK frames: the
// 16-bit instantiations of the frame kernels of sml_frame_kernels.h, launched
// by the typed entry points of sml_frames.hip (sml_quantize_pack_frames_typed,
// sml_dequantize_frames_typed).  The FLOAT32 and INT32 instantiations are
// sml_frames.hip's.
//
// The rule of sml_half.hip, applied to frames: the transmit kernel widens an
// element to fp32 in registers right after its load (exact), and everything
// from there on — block exponent, scale, roundf, the big-endian words, the
// headers, the extra batch — is the FLOAT32 slice of the widened values, so
// the frame set is that slice's byte for byte.  The receive side's claim pass
// sees no element at all; its apply pass dequantizes to fp32 as ever and
// narrows (round to nearest even) right before the store.
//
// Layout: the fp32 kernels' tiles.  tx: 1024 elements per wave, one 8-byte
// load per lane per slice, four in flight.  rx: rx_slices(P) slices, one
// 8-byte store per lane per slice.  Slices start at any element: every typed
// access is declared 2-byte aligned (h4a, sml_device.h) and a partial tail
// goes element by element, so no byte outside [ptr, ptr + 2 numel) is read or
// written.
#include "sml_frame_kernels.h"

namespace sml {

// The element policy of a 16-bit slice by its variant: FLOAT16 or BFLOAT16.
template <bool F16>
using ElemHalf = Elem16<F16 ? kHalfF16 : kHalfBF16>;

void launch_quantize_frames_h(const FrameArgs& a, bool f16, uint32_t P, bool global, bool nts, dim3 grid,
                              hipStream_t st) {
    dispatch_packet(P, [&](auto Pc) {
        dispatch_bools([&](auto F16, auto GLOBAL, auto NTS) {
            k_quantize_frames<Pc(), ElemHalf<F16()>, GLOBAL(), NTS(), false><<<grid, kBlockThreads, 0, st>>>(a);
        }, f16, global, nts);
    });
}

void launch_rx_apply_h(const RxArgs& a, bool f16, uint32_t P, bool nt, dim3 grid, hipStream_t st) {
    dispatch_packet(P, [&](auto Pc) {
        dispatch_bools([&](auto F16, auto NT) {
            k_rx_apply<Pc(), ElemHalf<F16()>, NT()><<<grid, kBlockThreads, 0, st>>>(a);
        }, f16, nt);
    });
}

}  // namespace sml
