/* switchml_msg_batch.h — the batched round trip for long RDMA messages, part of
 * the C ABI of libswitchml_hip.so: switchml_hip.h includes it beside the other
 * sub-headers, and a caller includes switchml_hip.h.  Symbols are only added:
 * sml_abi_version() stays as it is.
 *
 * sml_msg_roundtrip_loopback_batch is sml_roundtrip_loopback_batch_typed
 * (switchml_hip.h) with M = msg_numel in place of the packet size P, for every
 * M that sml_msg_numel_supported (switchml_messages.h) accepts: the client's
 * batch worker runs the FIFO slices of its queued jobs at
 * general.packet_numel = M through it, one launch per element type present.
 *   Slice i gets exactly
 *     sml_msg_roundtrip_loopback(in, out, data_type, numel, msg_numel,
 *                                num_workers, NULL, NULL,
 *                                flags & SML_FLAG_ROUND_RNE, stream)
 *   bit for bit: its messages start at its own first element, no planes are
 *   written.  For M in {64, 128, 256, 512, 1024} the results are
 *   sml_roundtrip_loopback_batch_typed's.
 *   data_type per slice: SML_FLOAT32, SML_FLOAT16, SML_BFLOAT16; types may be
 *   mixed in one call.  A slice starts at any element (4-byte alignment for
 *   FLOAT32, 2-byte for the 16-bit types); no byte outside it is read or
 *   written; in == out within a slice is allowed; slices must not overlap each
 *   other.  At most SML_MAX_BATCH_SLICES slices a call; numel == 0 slices are
 *   skipped.  Flags: SML_FLAG_ROUND_RNE (the payload byte order is not
 *   observable here).
 *   Launches: at most one per element type present.  A type with exactly one
 *   non-empty slice takes sml_msg_roundtrip_loopback's kernel; the packet sizes
 *   that entry point hands to the packet kernels (M <= 512) hand the whole call
 *   to sml_roundtrip_loopback_batch_typed.  Output stores are non-temporal by
 *   the call's total output bytes over every slice and type
 *   (sml_set_payload_nt_threshold); the grid honours sml_set_grid_limit.
 * Status, every check before any launch, in this order (the typed batch's):
 *   msg_numel unsupported -> SML_ERR_UNSUPPORTED; num_workers == 0,
 *   num_slices > SML_MAX_BATCH_SLICES, slices == NULL with num_slices > 0 ->
 *   SML_ERR_INVALID_ARG; then slice by slice: reserved != 0 ->
 *   SML_ERR_INVALID_ARG; data_type SML_INT32 or any other value, or
 *   numel >= 2^56 -> SML_ERR_UNSUPPORTED; with numel > 0, a NULL or misaligned
 *   in / out -> SML_ERR_INVALID_ARG; more than 2^32 - 1 message groups in one
 *   launch (a group is the 4, 2 or 1 messages a workgroup holds at a time) ->
 *   SML_ERR_UNSUPPORTED.  No non-empty slice: SML_OK, the device is not
 *   touched. */
#ifndef SWITCHML_MSG_BATCH_H_
#define SWITCHML_MSG_BATCH_H_

#include "switchml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

sml_status_t sml_msg_roundtrip_loopback_batch(const sml_typed_slice* slices, uint32_t num_slices,
                                              uint32_t msg_numel, uint16_t num_workers, uint32_t flags,
                                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_MSG_BATCH_H_ */
