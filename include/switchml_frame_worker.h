/* switchml_frame_worker.h — the worker's side of the DPDK frames (SURVEY §8
 * F3), part of the C ABI of libswitchml_hip.so: switchml_hip.h includes it at
 * its end beside the two RDMA headers, and a caller includes switchml_hip.h.
 * Symbols are only added: sml_abi_version() stays as it is.
 *
 * The DPDK worker thread's receive loop (dpdk_worker_thread.cc:274-389, with
 * ReusePacket and ResendPacketCallback, dpdk_worker_thread_utils.inc) over a
 * batch of received frames per call, with what the loop keeps per outstanding
 * packet — the pkt_id a tx slot expects back and the exponent received with
 * the slot's previous frame — in d_state across calls.  The result of packet p
 * carries the exponent under which block p is quantized into packet p + b, and
 * at most max_outstanding_pkts (Q) packets are in flight: what a call emits is
 * the tx slots to send, as indices sml_frame_gather takes as they stand.
 *
 * Parameters: a sml_frame_params (the addresses, job_id, pool_index_start,
 * pool_index_shift, max_outstanding_pkts = Q in 1..16384, pool_index_start + Q
 * <= 16384) and num_workers, data_type (SML_FLOAT32, SML_INT32, SML_FLOAT16,
 * SML_BFLOAT16), packet_numel P, flags (SML_FLAG_ROUND_RNE).
 *
 * Buffers.  tx is a ring of Q frame slots tx_stride bytes apart; rx is a dense
 * run of n received frames rx_stride apart, what sml_frame_switch_deliver
 * leaves in a worker's ring.  Both are device memory or pinned, device-mapped
 * host memory, 4-byte aligned, with strides >= sml_frame_bytes(P) and a
 * multiple of 4.  tx and rx must not overlap (SML_ERR_INVALID_ARG): received
 * frames arrive in any order while tx slots are fixed, so the reference's mbuf
 * reuse cannot be modelled by aliasing.  d_in / d_out are the job slice,
 * `numel` elements of data_type, aligned to the element; d_in == d_out is
 * allowed.
 *
 * d_state: sml_frame_worker_state_bytes(Q) bytes — a 64-byte slice header and
 * one 16-byte record per slot (the pkt_id it expects back, a claim word, the
 * exponent received with the slot's previous frame): O(Q).  There is no
 * per-pkt_id bitmap: with one expected id per slot, pkt_id < expected is
 * "received before".
 *
 * sml_frame_worker_reset: no slice under way.
 *
 * sml_frame_worker_begin (:274-300): B = ceil(numel / P), b = min(Q, B),
 * total = B + b frames for the float types, B for INT32 (NeedsExtraBatch).
 *   p < b: tx slot p holds frame p byte for byte as
 *     sml_quantize_pack_frames_typed builds it — header, pool index
 *     PktId2PoolIndex(p, start, shift, Q), block p's exponent, zero payload —
 *     or, INT32, frame p of sml_pack_frames_int32; slot p expects pkt_id p;
 *     d_sends[p] = p;
 *   b <= q < Q: d_sends[q] = SML_FRAME_WORKER_NONE (all ones).
 *   d_sends is uint64, so that an array of it is a d_index of sml_frame_gather
 *   as it stands: gather skips an out-of-range index and counts it.
 *   numel == 0: SML_OK, b = 0, every entry NONE.
 *
 * sml_frame_worker_poll (:300-389) over the n frames of rx; the state is judged
 * as it stands at the start of the call.  d_num_frames: nullable, a device
 * uint64, the ring's live count — pass d_ring_count + u as deliver leaves it;
 * the host then needs to know only the ring's capacity n.
 *   Frame i is IGNORED, and not read, when i >= *d_num_frames or no slice is
 *   under way.  It is WRONG (stats_wrong_pkts_received) when byte 43 !=
 *   (uint8_t)job_id; when pkt_id >= total; when pkt_id != the id slot
 *   pkt_id % b expects, whether an earlier one (a duplicate) or a later one;
 *   and when it is a candidate — none of the above — but not the lowest-index
 *   candidate of its slot in this call: the first copy wins and a later copy's
 *   payload is never used.  A WRONG or IGNORED frame changes no byte of tx,
 *   d_out or the state.
 *   One divergence: the reference's bitmap would accept a pkt_id ahead of what
 *   was sent.  A correct switch cannot produce one; here it is WRONG.
 *   An accepted frame, packet p on slot j, in this order:
 *     PostprocessSingle(p) — a float type, p >= b: block p - b dequantized from
 *       the payload under the exponent kept for j, its real words only,
 *       narrowed (round to nearest even) for the 16-bit types; p < B: byte 50
 *       is kept as the slot's exponent (a signed int8).  INT32: block p
 *       ntohl'd into d_out;
 *     expected += b; still below total -> ReusePacket: tx slot j becomes frame
 *       p + b byte for byte as the bulk tx would build it under the received
 *       global exponents — pkt_id p + b, the pool dword PktId2PoolIndex(p + b,
 *       ...) with block p + b's exponent (0 when p + b >= B), payload = block p
 *       quantized under the exponent just received (roundf, or
 *       SML_FLAG_ROUND_RNE on the 16-aligned body of the block), zero tail
 *       words in a partial last block; INT32: block p + b byte-swapped —
 *       d_sends[i] = j and the verdict POSTED.  Else the verdict is FINISHED.
 *   Every d_sends[i] that is not POSTED is NONE.  d_counts[v] is added to per
 *   verdict; the slice is complete when POSTED + FINISHED have summed to total.
 *
 * sml_frame_worker_resend (ResendPacketCallback): d_sends[i] is slot d_slots[i]
 * again if it has a frame outstanding (a slot of the slice that has not
 * finished), else NONE.  The frame is still in the tx ring: nothing is rebuilt
 * and nothing else changes.
 *
 *   d_state: 16-byte aligned, opaque; sml_frame_worker_reset before the first
 *     call;  d_sends: uint64[Q] (begin) or [n];  d_slots: uint32[n];
 *     d_verdict: uint8[n];  d_counts: uint64[4], nullable;  device memory,
 *     8-byte aligned (d_slots: 4).
 * Status, every check before any launch: params NULL, num_workers == 0, or a
 * NULL pointer with work to do (begin: d_state, d_sends, and with numel > 0
 * d_in, d_out, tx; poll, n > 0: rx, d_state, tx, d_sends, d_verdict; resend,
 * n > 0: d_slots, d_state, d_sends) -> SML_ERR_INVALID_ARG; packet_numel not a
 * packet size, Q not in 1..16384, pool_index_start + Q > 16384, data_type not
 * one of the four, n >= 2^31, a slice of more than 2^32 - 1 frames (pkt_id is
 * 32 bits on the wire) -> SML_ERR_UNSUPPORTED; n == 0 -> SML_OK, nothing
 * launched; tx and rx overlapping -> SML_ERR_INVALID_ARG; a buffer or stride
 * off its alignment -> SML_ERR_ALIGNMENT.  poll and resend take the slice from
 * d_state: their params are the ones begin was given.
 * Calls on one state are ordered by their stream, one at a time.  Launches:
 * reset, begin (a lane group per slot) and resend (a thread per entry) one
 * each; poll two — judge (a thread per frame: header dwords 10-12 read,
 * IGNORED / WRONG written, a candidate claims its slot with an atomic min of
 * its index) and accept (P / 4 lanes per frame, 4 frames per wave at P = 64:
 * the claim's holder loads the payload, the slot's record and the two blocks
 * of the slice, waits once, and only then writes d_out, tx, the state and its
 * entry). */
#ifndef SWITCHML_FRAME_WORKER_H_
#define SWITCHML_FRAME_WORKER_H_

#include "switchml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sml_frame_worker_params {
    sml_frame_params frame;  /* addresses, job_id, pool_index_start / _shift, max_outstanding_pkts = Q */
    uint16_t num_workers;    /* W of the scale */
    uint16_t data_type;      /* SML_FLOAT32, SML_INT32, SML_FLOAT16, SML_BFLOAT16 */
    uint32_t packet_numel;   /* P: 64,128,256,512,1024 */
    uint32_t flags;          /* SML_FLAG_ROUND_RNE */
} sml_frame_worker_params;

/* sml_frame_worker_poll's verdict per received frame */
#define SML_FRAME_WORKER_WRONG    0   /* stats_wrong_pkts_received: another job, duplicate or unexpected id */
#define SML_FRAME_WORKER_POSTED   1   /* accepted; the slot's next frame is built, d_sends[i] is the slot */
#define SML_FRAME_WORKER_FINISHED 2   /* accepted; the slot has no further frame in this slice */
#define SML_FRAME_WORKER_IGNORED  3   /* past the ring's live count, or no slice under way */
/* a d_sends entry that sends nothing */
#define SML_FRAME_WORKER_NONE 0xFFFFFFFFFFFFFFFFull

/* Bytes of d_state for max_outstanding_pkts slots; 0 on an unsupported count. */
uint64_t sml_frame_worker_state_bytes(uint32_t max_outstanding_pkts);
/* One small kernel on `stream`.  Status: d_state NULL -> SML_ERR_INVALID_ARG;
 * bad max_outstanding_pkts -> SML_ERR_UNSUPPORTED; d_state not 16-byte aligned
 * -> SML_ERR_ALIGNMENT. */
sml_status_t sml_frame_worker_reset(void* d_state, uint32_t max_outstanding_pkts, void* stream);
sml_status_t sml_frame_worker_begin(const sml_frame_worker_params* params, const void* d_in, void* d_out,
                                    uint64_t numel, void* d_state, void* tx, uint64_t tx_stride, uint64_t* d_sends,
                                    void* stream);
sml_status_t sml_frame_worker_poll(const sml_frame_worker_params* params, const void* rx, uint64_t n,
                                   uint64_t rx_stride, const uint64_t* d_num_frames, void* d_state, void* tx,
                                   uint64_t tx_stride, uint64_t* d_sends, uint8_t* d_verdict, uint64_t* d_counts,
                                   void* stream);
sml_status_t sml_frame_worker_resend(const sml_frame_worker_params* params, const uint32_t* d_slots, uint64_t n,
                                     void* d_state, uint64_t* d_sends, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_FRAME_WORKER_H_ */
