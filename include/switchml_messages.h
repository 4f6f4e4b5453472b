/* switchml_messages.h — long RDMA messages, part of the C ABI of
 * libswitchml_hip.so: switchml_hip.h includes it beside the other sub-headers,
 * and a caller includes switchml_hip.h.  Symbols are only added:
 * sml_abi_version() stays as it is.
 *
 * The RDMA backend quantizes per MESSAGE: RdmaWorkerThread creates its
 * pre/post-processor with ltu_size = msg_numel * 4 (rdma_worker_thread.cc:
 * 86-88), so one exponent covers backend.rdma.msg_numel elements, and
 * config.cc:185-192 accepts every msg_numel that is a multiple of
 * general.packet_numel (64 or 256) — up to 64 packets of 256 elements with the
 * shipped window.  These entry points are sml_exponents_typed,
 * sml_quantize_pack_typed, sml_dequantize_typed and
 * sml_roundtrip_loopback_typed (switchml_hip.h) with M = msg_numel in place of
 * the packet size P, for every such M:
 *   B = ceil(numel / M); message k covers elements [kM, min((k+1)M, numel));
 *   one int8 exponent per message; the payload plane is int32[B*M], 16-byte
 *   aligned; words of the last, partial message past numel are written as 0.
 *   M: any multiple of SML_MSG_NUMEL_STEP from 64 to SML_MSG_NUMEL_MAX.  For
 *   M in {64, 128, 256, 512, 1024} the results are those of the entry points
 *   above, bit for bit.
 *   data_type: SML_FLOAT32, SML_FLOAT16, SML_BFLOAT16 (widened right after the
 *   load, narrowed round-to-nearest-even right before the store).  A typed
 *   buffer starts at any element (4-byte alignment for FLOAT32, 2-byte for the
 *   16-bit types); no byte outside it is touched; in == out is allowed for the
 *   round trip.
 *   flags: SML_FLAG_PAYLOAD_LE, SML_FLAG_ROUND_RNE (the VCL body is the first
 *   n - n % 16 elements of each message, n the message's real element count).
 *   sml_msg_quantize_pack: d_global_exps != NULL is K3 (d_exps_out NULL or
 *   equal to it, not written), NULL is K1 (d_exps_out nullable).
 *   sml_msg_roundtrip_loopback: d_payload / d_exps_out nullable, as the twin.
 * Status, every check before any launch, in this order (the FLOAT32 twins'):
 *   sml_msg_exponents: d_exps NULL with numel > 0 -> SML_ERR_INVALID_ARG;
 *   sml_msg_quantize_pack: num_workers == 0, d_payload NULL with numel > 0, or
 *     d_exps_out given beside a different d_global_exps -> SML_ERR_INVALID_ARG;
 *   all four, then: msg_numel unsupported -> SML_ERR_UNSUPPORTED; data_type
 *     SML_INT32 or any other value -> SML_ERR_UNSUPPORTED (an INT32 slice needs
 *     no exponent and is size-free already: sml_bswap_i32); numel >= 2^56 ->
 *     SML_ERR_UNSUPPORTED; num_workers == 0 -> SML_ERR_INVALID_ARG; numel == 0
 *     -> SML_OK, nothing launched; a NULL or misaligned typed buffer, a NULL
 *     plane the call needs -> SML_ERR_INVALID_ARG; a payload plane off 16 bytes
 *     -> SML_ERR_ALIGNMENT.
 *
 * What a caller composes from what exists:
 *   the RDMA immediates of a slice: sml_rdma_imm on the message exponent plane
 *     (sml_msg_exponents or sml_msg_quantize_pack's d_exps_out);
 *   the switch such workers talk to: sml_msg_switch (switchml_msg_switch.h),
 *     sml_rdma_switch's slot pool, worker bitmap, retransmission and receive
 *     regions for every msg_numel served here and pkts_per_msg up to 256;
 *   the completion loop that drives it message by message: sml_msg_worker_begin
 *     / _poll / _resend (switchml_msg_worker.h), sml_rdma_worker's per-QP state
 *     and records at the same msg_numel and pkts_per_msg;
 *   a W-worker switch step on whole planes, without a slot pool:
 *     sml_msg_exponents per worker -> sml_switch_exps ->
 *     sml_msg_quantize_pack with the global exponents per worker ->
 *     sml_switch_aggregate with d_out = NULL (the payload sum knows no block
 *     size: pass any packet size that divides B*M, such as 64) ->
 *     sml_msg_dequantize.
 *   the batched round trip over the FIFO slices of several jobs:
 *     sml_msg_roundtrip_loopback_batch (switchml_msg_batch.h), which the
 *     client's bulk and fused modes reach at general.packet_numel = msg_numel.
 * Not served at msg_numel > 1024 (they keep returning SML_ERR_UNSUPPORTED): the
 * per-packet bursts and the burst server, the DPDK frames, sml_rdma_switch and
 * the sml_rdma_worker_* calls themselves (their sml_msg_switch and
 * sml_msg_worker_* twins serve them), sml_roundtrip_loopback_batch_typed
 * itself, and in the client backend.hip.mode = packet and backend = xgmi. */
#ifndef SWITCHML_MESSAGES_H_
#define SWITCHML_MESSAGES_H_

#include "switchml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SML_MSG_NUMEL_STEP 64u      /* msg_numel is a multiple of this */
#define SML_MSG_NUMEL_MAX  16384u   /* 64 packets of 256 elements */

/* 1 when msg_numel is served by the sml_msg_* entry points, else 0. */
int sml_msg_numel_supported(uint32_t msg_numel);

sml_status_t sml_msg_exponents(const void* d_in, sml_data_type_t data_type, uint64_t numel, uint32_t msg_numel,
                               int8_t* d_exps, void* stream);
sml_status_t sml_msg_quantize_pack(const void* d_in, sml_data_type_t data_type, uint64_t numel, uint32_t msg_numel,
                                   uint16_t num_workers, const int8_t* d_global_exps, int32_t* d_payload,
                                   int8_t* d_exps_out, uint32_t flags, void* stream);
sml_status_t sml_msg_dequantize(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel, uint32_t msg_numel,
                                uint16_t num_workers, void* d_out, sml_data_type_t data_type, uint32_t flags,
                                void* stream);
sml_status_t sml_msg_roundtrip_loopback(const void* d_in, void* d_out, sml_data_type_t data_type, uint64_t numel,
                                        uint32_t msg_numel, uint16_t num_workers, int32_t* d_payload,
                                        int8_t* d_exps_out, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_MESSAGES_H_ */
