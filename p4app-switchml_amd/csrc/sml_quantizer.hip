// sml_quantizer.hip — CDNA4 (gfx950) kernels for the planes of SwitchML's
// end-host pre/post-processor (CpuExponentQuantizerPPP,
// client_lib/src/prepostprocessors/cpu_exponent_quantizer_ppp.cc = "ppp.cc")
// and their C-ABI entry points (include/switchml_hip.h): the fp32
// instantiations of the plane kernels of sml_planes.h (K1 fused exponent +
// quantize + pack, K2 exponents, K3 quantize with given exponents, K4
// dequantize, the fused loopback round trip), the batched round trip, the word
// streams (loopback x W, INT32 byteswap), RDMA immediates and the copy probe.
// Tile layout, numerics and parity notes: sml_device.h; 16-bit slices:
// sml_half.hip; DPDK frames: sml_frames.hip.
#include "sml_planes.h"

namespace sml {

thread_local char g_last_error[256] = "";
std::atomic<uint32_t> g_grid_limit{0};
std::atomic<uint32_t> g_xcd_chunk{64};

// -------------------------------------------------------------- kernels

// Word streams in the quantizer's tile shape (1024 words per wave, 16-B
// non-temporal loads, default-policy stores, XCD order, one-shot grid; any
// 4-byte alignment; in may alias out):
//  * K5 DummyBackend::ProcessPacket over the payload plane: per word bswap,
//    int32 wrap multiply by W, bswap (dummy_backend.cc:72-84); LE words skip
//    the swaps;
//  * INT32 path: byteswap (ppp.cc:158-190, 262-298).
struct LoopbackOp {
    uint32_t W;
    bool be;
    __device__ __forceinline__ uint32_t operator()(uint32_t q) const { return be ? bswap(bswap(q) * W) : q * W; }
};
struct BswapOp {
    __device__ __forceinline__ uint32_t operator()(uint32_t q) const { return bswap(q); }
};

// Measurement probe (not on the hot path): the same 1024-element tiles and
// the same access policy as the quantize kernel — non-temporal 16-B loads,
// and 16-B stores under K1's store policy for a plane of that size
// (non-temporal from g_nt_threshold bytes on, default policy below) — no
// arithmetic: the practical HBM ceiling the quantize kernel is compared
// against.
template <bool NTS, int U>
__global__ __launch_bounds__(kBlockThreads) void k_stream_copy(const u4* in, u4* out, uint64_t ntiles, uint32_t xcd) {
    struct { uint32_t xcd; } a{xcd};
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    constexpr uint64_t kVecs = tile_elems<U>() / 4;
    for (uint64_t t = xcd_block(a.xcd) * kWavesPerBlock + wave_index(); t < ntiles; t += nwaves) {
        u4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = __builtin_nontemporal_load(in + t * kVecs + u * kWave + lane);
#pragma unroll
        for (int u = 0; u < U; u++) store_payload_as<NTS>(out + t * kVecs + u * kWave + lane, v[u]);
    }
}

// RDMA immediates: (msg_id & 0xFFFF) | exponent byte << 16 (rdma_worker_thread.cc:341-356).
__global__ __launch_bounds__(kBlockThreads) void k_rdma_imm(const int8_t* exps, uint64_t B, uint64_t total,
                                                            uint32_t* imm) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    for (uint64_t m = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; m < total; m += stride) {
        const uint32_t e = exps && m < B ? (uint32_t)(uint8_t)exps[m] : 0u;
        imm[m] = (uint32_t)(m & 0xFFFFu) | (e << 16);
    }
}

// Fault injection (sml_debug_stall): one wave that occupies its stream for
// `ticks` of the constant-rate wall clock, then exits — a kernel that does
// not finish within a caller's timeout, yet always ends on its own.
constexpr uint32_t kMaxStallMicros = 60u * 1000u * 1000u;
__global__ __launch_bounds__(64) void k_stall(uint64_t ticks) {
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

__global__ void k_scale_lut(float* lut, uint32_t W) {
    lut[threadIdx.x] = scale_for(W, (int)(int8_t)(uint8_t)threadIdx.x);
}

// ------------------------------------------------------------ host side

// Slices per K1/K2/K3 tile: 4 (1024-element tiles), 2 or 1 (never below
// P / 256), or 0 = the default, 2 for every kernel (sml_set_quantize_tile_slices).
// Final kernels (early loads, sc1 nt stores; profiles/r04/ab_slices_final.json,
// 4 cold buckets, interleaved medians): 2-slice tiles against 4 at 256 MiB
// K1 -3.1 %, K3 -2.0 %, K2 -3.2 % time (K1 -4.9 % at 128 MiB).  Before the
// early loads and sc1 (round 4's first sweep), measured with non-temporal payload stores
// on the bench workload, steps cycling 4 buckets (round 4,
// profiles/r04/ab_slices_nt.json, interleaved medians): K1 with 2-slice tiles
// +1.3 / +0.6 / +3.8 / +0.9 % at 128 / 256 / 512 / 1024 MiB, K3 -2.8 % and
// K2 -2.6 % at 256 MiB; 1-slice tiles lose everywhere (K1 -3 %, K2 -35 %:
// one 1 KiB load in flight per wave is latency-bound).  Round 2's sweep ran
// before the non-temporal stores and had 2-slice K1 level cold.
static std::atomic<uint32_t> g_quant_slices{0};

// Payload planes (and K4 / round-trip fp32 outputs) of at least this many
// bytes take non-temporal stores (sml_set_payload_nt_threshold; UINT64_MAX =
// never, 0 = always).  Measured on cold HBM — steps cycling distinct buckets,
// the pattern of a real job where a plane is written once and handed on
// (profiles/r03/ab_cold_policy*.json, interleaved medians): non-temporal
// stores win at 64 / 128 / 256 MiB planes for K1 (+4.1 / +3.5 / +4.6 %), K4
// (+5.6 / +6.3 / +4.5 %) and the fused round trip (+4.2 / +3.1 / +3.5 %).
// Default-policy stores win only when ONE plane is rewritten step after step
// (it then stays in the 256 MiB Infinity Cache: K1 7.13 vs 6.31 TB/s at
// 256 MiB, 6.54 vs 6.09 at 128 MiB; level at 64 MiB).  So planes from a
// quarter of the Infinity Cache on stream non-temporally; smaller ones (a
// framework's 25 MiB gradient buckets) keep the default policy, so their
// next reader can find them in the cache.  Bytes are identical either way.
std::atomic<uint64_t> g_nt_threshold{64ull << 20};

// Slices per K4 / fused round-trip tile: 4 or 2 (sml_set_stream_tile_slices;
// 0 = the default, 2 for both — a round-trip tile holds whole packets, so
// P = 1024 keeps 4.  Final kernels, profiles/r04/ab_stream_slices_final.json:
// 2 against 4 at 256 / 128 MiB, K4 -0.8 / -1.9 %, the round trip -3.4 / -3.6 %
// time; round 4's first sweep, before the early loads and sc1 stores, had
// the round trip level).
static std::atomic<uint32_t> g_stream_slices{0};

static uint32_t stream_slices(uint32_t dflt) {
    const uint32_t want = g_stream_slices.load(std::memory_order_relaxed);
    return want ? want : dflt;
}

static uint32_t quant_slices(uint32_t P) {
    const uint32_t need = P > 256 ? P / 256 : 1;
    uint32_t want = g_quant_slices.load(std::memory_order_relaxed);
    if (want == 0) want = 2u;
    return want > need ? want : need;
}

// K1 / K2 / K3 on an fp32 slice: the aligned form when the slice allows it.
static sml_status_t quantize_f32(const float* d_in, uint64_t numel, uint32_t P, uint16_t W, const int8_t* d_gexp,
                                 int32_t* d_payload, int8_t* d_exps_out, uint32_t flags, void* stream) {
    return plane_quantize<ElemF32, 1, 2, 4>(d_in, aligned16(d_in), quant_slices(P), numel, P, W, d_gexp, d_payload,
                                            d_exps_out, flags, stream);
}

// Tile slices of the fp32 batch (P = 1024: 4): the single-slice round trip's
// 2 — against 4 on 4 cold jobs: a 256 MiB job as 4 FIFO slices 86.22 ->
// 85.86 us, 4 x 25 MiB buckets 36.10 -> 35.32 us
// (profiles/r04/ab_batch_slices.json).
static uint32_t batch_slices_f32(uint32_t P) { return P > 512 ? 4u : 2u; }

uint64_t batch_tile_f32(uint32_t P) { return (uint64_t)batch_slices_f32(P) * kWave * 4; }

sml_status_t batch_launch_f32(RoundTripBatchArgs<float>& a, uint32_t P, uint16_t W, uint32_t flags, bool nt,
                              void* stream) {
    if (a.nslices == 0) return SML_OK;
    if (a.nslices == 1)   // one slice: the single-slice kernel (aligned form when the slice allows it)
        return sml_roundtrip_loopback(a.in[0], a.out[0], a.numel[0], P, W, nullptr, nullptr,
                                      flags & SML_FLAG_ROUND_RNE, stream);
    const uint32_t U = batch_slices_f32(P);
    a.xcd = xcd_chunk_for(U);
    a.W = W;
    const dim3 grid(grid_for_tiles(a.tile_end[a.nslices - 1]));
    hipStream_t st = (hipStream_t)stream;
    const bool rne = flags & SML_FLAG_ROUND_RNE;
    dispatch_packet(P, [&](auto Pc) {
        dispatch_slices<2, kU>(U, [&](auto Uc) {
            dispatch_bools([&](auto RNE, auto NT) {
                // P = 1024 always runs the default slices (U above): a tile holds the packet
                constexpr int kUc = Pc() <= 512 ? Uc() : kU;
                k_roundtrip_batch<Pc(), ElemF32<false>, RNE(), NT(), kUc><<<grid, kBlockThreads, 0, st>>>(a);
            }, rne, nt);
        });
    });
    return launch_check();
}

}  // namespace sml

using namespace sml;

extern "C" {

int sml_abi_version(void) { return SML_ABI_VERSION; }

const char* sml_status_string(sml_status_t s) {
    switch (s) {
        case SML_OK: return "SML_OK";
        case SML_ERR_INVALID_ARG: return "SML_ERR_INVALID_ARG";
        case SML_ERR_UNSUPPORTED: return "SML_ERR_UNSUPPORTED";
        case SML_ERR_ALIGNMENT: return "SML_ERR_ALIGNMENT";
        case SML_ERR_HIP: return "SML_ERR_HIP";
    }
    return "SML_ERR_UNKNOWN";
}

const char* sml_last_error(void) { return g_last_error; }

uint32_t sml_set_grid_limit(uint32_t max_workgroups) {
    return g_grid_limit.exchange(max_workgroups);
}

uint32_t sml_set_xcd_chunk(uint32_t chunk) {
    return g_xcd_chunk.exchange(chunk);
}

uint64_t sml_set_payload_nt_threshold(uint64_t bytes) { return g_nt_threshold.exchange(bytes); }

uint32_t sml_set_stream_tile_slices(uint32_t slices) {
    return g_stream_slices.exchange(slices == 2 || slices == 4 ? slices : 0u);
}

uint32_t sml_set_quantize_tile_slices(uint32_t slices) {
    return g_quant_slices.exchange(slices == 1 || slices == 2 || slices == 4 ? slices : 0u);
}

uint64_t sml_num_blocks(uint64_t numel, uint32_t packet_numel) {
    if (packet_numel == 0) return 0;
    // ceil(numel*4 / (P*4)) of ppp.cc:56-57, without the byte-count overflow
    return numel / packet_numel + (numel % packet_numel != 0);
}

sml_status_t sml_scale_lut(uint16_t num_workers, float lut[256]) {
    if (num_workers == 0 || !lut) return SML_ERR_INVALID_ARG;
    for (int i = 0; i < 256; i++) {
        int e = (int)(int8_t)(uint8_t)i;
        float denom = (float)num_workers * powf(2.0f, (float)e);
        lut[i] = (float)((double)2147483647 / (double)denom);
    }
    return SML_OK;
}

sml_status_t sml_scale_lut_device(uint16_t num_workers, float* d_lut, void* stream) {
    if (num_workers == 0 || !d_lut) return SML_ERR_INVALID_ARG;
    k_scale_lut<<<1, 256, 0, (hipStream_t)stream>>>(d_lut, num_workers);
    return launch_check();
}

sml_status_t sml_exponents(const float* d_in, uint64_t numel, uint32_t packet_numel,
                           int8_t* d_exps, void* stream) {
    if (numel && !d_exps) return SML_ERR_INVALID_ARG;
    return quantize_f32(d_in, numel, packet_numel, 1, nullptr, nullptr, d_exps, 0, stream);
}

sml_status_t sml_quantize_pack(const float* d_in, uint64_t numel, uint32_t packet_numel,
                               uint16_t num_workers, const int8_t* d_global_exps,
                               int32_t* d_payload, int8_t* d_exps_out,
                               uint32_t flags, void* stream) {
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (numel && !d_payload) return SML_ERR_INVALID_ARG;
    if (d_global_exps && d_exps_out && d_exps_out != d_global_exps) return SML_ERR_INVALID_ARG;
    return quantize_f32(d_in, numel, packet_numel, num_workers, d_global_exps, d_payload, d_exps_out, flags, stream);
}

sml_status_t sml_dequantize(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel,
                            uint32_t packet_numel, uint16_t num_workers, float* d_out,
                            uint32_t flags, void* stream) {
    // measured: 2-slice tiles +0.6 / +2.8 / +3.3 % at 128 / 256 / 512 MiB
    return plane_dequantize<ElemF32, 2, 4>(d_payload, d_exps, numel, packet_numel, num_workers, d_out,
                                           aligned16(d_out), stream_slices(2), flags, stream);
}

sml_status_t sml_roundtrip_loopback(const float* d_in, float* d_out, uint64_t numel,
                                    uint32_t packet_numel, uint16_t num_workers,
                                    int32_t* d_payload, int8_t* d_exps_out,
                                    uint32_t flags, void* stream) {
    // a tile holds whole packets: P = 1024 needs 4 slices
    const uint32_t U = packet_numel > 512 ? 4u : stream_slices(2);
    // in and out share the slice offset, so one alignment test covers both
    // unless the caller passed differently aligned buffers.
    return plane_roundtrip<ElemF32, 2, 4>(d_in, d_out, aligned16(d_in) && aligned16(d_out), U, numel, packet_numel,
                                          num_workers, d_payload, d_exps_out, flags, stream);
}

sml_status_t sml_roundtrip_loopback_batch(const sml_slice* slices, uint32_t num_slices, uint32_t packet_numel,
                                          uint16_t num_workers, uint32_t flags, void* stream) {
    if (!valid_packet(packet_numel)) return SML_ERR_UNSUPPORTED;
    if (num_workers == 0 || num_slices > SML_MAX_BATCH_SLICES || (num_slices && !slices)) return SML_ERR_INVALID_ARG;
    RoundTripBatchArgs<float> a;
    a.nslices = 0;
    uint64_t tiles = 0, out_bytes = 0;
    for (uint32_t i = 0; i < num_slices; i++) {
        const sml_status_t s = batch_add(a, tiles, slices[i].in, slices[i].out, slices[i].numel, packet_numel,
                                         batch_tile_f32(packet_numel));
        if (s != SML_OK) return s;
        out_bytes += 4 * slices[i].numel;
    }
    // the outputs of the whole batch past the Infinity Cache: non-temporal stores
    return batch_launch_f32(a, packet_numel, num_workers, flags, nt_from(out_bytes), stream);
}

sml_status_t sml_rdma_imm(const int8_t* d_exps, uint64_t B, uint32_t batch_max, uint32_t* d_imm, void* stream) {
    if (B == 0) return SML_OK;
    // a FLOAT32 slice needs its exponent plane: a null one is an error, not
    // an INT32 slice (sml_rdma_imm_int32 is that)
    if (!d_imm || !d_exps || batch_max == 0) return SML_ERR_INVALID_ARG;
    const uint64_t total = B + (B < batch_max ? B : batch_max);
    k_rdma_imm<<<grid_for_vec(total), kBlockThreads, 0, (hipStream_t)stream>>>(d_exps, B, total, d_imm);
    return launch_check();
}

sml_status_t sml_rdma_imm_int32(uint64_t B, uint32_t* d_imm, void* stream) {
    if (B == 0) return SML_OK;
    if (!d_imm) return SML_ERR_INVALID_ARG;
    // B messages (no extra batch, ppp.cc:65-67), byte 2 untouched (0)
    k_rdma_imm<<<grid_for_vec(B), kBlockThreads, 0, (hipStream_t)stream>>>(nullptr, B, B, d_imm);
    return launch_check();
}

sml_status_t sml_debug_stall(uint32_t microseconds, void* stream) {
    if (microseconds == 0) return SML_OK;
    if (microseconds > kMaxStallMicros) return SML_ERR_INVALID_ARG;
    int dev = 0, khz = 0;
    sml_status_t s = hip_check(hipGetDevice(&dev));
    if (s == SML_OK) s = hip_check(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    if (s != SML_OK) return s;
    if (khz <= 0) return SML_ERR_HIP;
    k_stall<<<1, 64, 0, (hipStream_t)stream>>>((uint64_t)microseconds * (uint64_t)khz / 1000u);
    return launch_check();
}

sml_status_t sml_stream_copy(const void* d_in, void* d_out, uint64_t bytes, void* stream) {
    if (bytes == 0) return SML_OK;
    if (!d_in || !d_out || !aligned16(d_in) || !aligned16(d_out) || bytes % (kTileElems * 4)) return SML_ERR_ALIGNMENT;
    // K1's tile shape (its slices per tile at P = 256) and store policy for an
    // output plane of `bytes` (sml_quantize_pack)
    const uint32_t U = quant_slices(256);
    const uint64_t ntiles = bytes / (256 * U * 4);
    const uint32_t xcd = xcd_chunk_for(U);
    auto in = reinterpret_cast<const u4*>(d_in);
    auto out = reinterpret_cast<u4*>(d_out);
    const bool nts = nt_from(bytes);
    const dim3 grid(grid_for_tiles(ntiles));
    hipStream_t st = (hipStream_t)stream;
    dispatch_slices<1, 2, 4>(U, [&](auto Uc) {
        dispatch_bools([&](auto NTS) {
            k_stream_copy<NTS(), Uc()><<<grid, kBlockThreads, 0, st>>>(in, out, ntiles, xcd);
        }, nts);
    });
    return launch_check();
}

sml_status_t sml_bswap_i32(const int32_t* d_in, int32_t* d_out, uint64_t numel, void* stream) {
    if (numel == 0) return SML_OK;
    if (!d_in || !d_out || !aligned4(d_in) || !aligned4(d_out)) return SML_ERR_INVALID_ARG;
    const uint64_t ntiles = (numel + kTileElems - 1) / kTileElems;
    k_words<<<grid_for_tiles(ntiles), kBlockThreads, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const uint32_t*>(d_in), reinterpret_cast<uint32_t*>(d_out), numel,
        g_xcd_chunk.load(std::memory_order_relaxed), BswapOp{});
    return launch_check();
}

sml_status_t sml_loopback_aggregate(int32_t* d_payload, uint64_t count, uint16_t num_workers,
                                    uint32_t flags, void* stream) {
    if (num_workers == 0) return SML_ERR_INVALID_ARG;
    if (count == 0) return SML_OK;
    if (!d_payload) return SML_ERR_INVALID_ARG;
    if (!aligned16(d_payload) || (count & 3u)) return SML_ERR_ALIGNMENT;
    const uint64_t ntiles = (count + kTileElems - 1) / kTileElems;
    uint32_t* p = reinterpret_cast<uint32_t*>(d_payload);
    k_words<<<grid_for_tiles(ntiles), kBlockThreads, 0, (hipStream_t)stream>>>(
        p, p, count, g_xcd_chunk.load(std::memory_order_relaxed),
        LoopbackOp{num_workers, !(flags & SML_FLAG_PAYLOAD_LE)});
    return launch_check();
}

}  // extern "C"
