/* switchml_rdma_worker.h — the worker's side of the RDMA messages (SURVEY §8
 * F4), part of the C ABI of libswitchml_hip.so: switchml_hip.h includes it
 * beside switchml_rdma_switch.h, and a caller includes switchml_hip.h.  Symbols
 * are only added: sml_abi_version() stays as it is.
 *
 * The RDMA worker's completion loop (rdma_worker_thread.cc:159-294, with
 * PostSendWr, :318-379) over a batch of completions per call, with what the
 * loop keeps per queue pair (QP) — the expected message id, the exponent
 * received with the QP's previous message, the pool flag — in d_state across
 * calls and job slices.  What a call emits is sml_rdma_arrival records
 * (switchml_rdma_switch.h): the send work requests of the worker, and, where
 * sml_rdma_switch plays the switch, that call's input as it stands.
 *
 * Buffers.  QP q's message buffer is tx + q * 4 * msg_numel; its result arrives
 * at rx + q * 4 * msg_numel.  tx == rx is allowed — the reference's single
 * registered buffer (:241, :322, :339) — otherwise the two must not overlap
 * (SML_ERR_INVALID_ARG).  Both are device memory or pinned, device-mapped host
 * memory, 16-byte aligned.  d_in / d_out are the job slice, `numel` elements
 * of data_type, aligned to the element's size; d_in == d_out is allowed.
 *
 * sml_rdma_worker_reset: no slice is under way, and every QP's pool flag is 1,
 * "flipped to 0 before the first message" (:118-125).  The flag survives
 * sml_rdma_worker_begin, as the reference's rkey survives job slices: were it
 * reset, the first message of a second slice would reach the switch in the set
 * the QP used last and be taken for a retransmission.
 *
 * sml_rdma_worker_begin (:156-192): B = ceil(numel / msg_numel), b = min(Q, B),
 * total = B + b messages for the float types, B for INT32 (NeedsExtraBatch).
 *   q < b: msg_id[q] = q, then PostSendWr(q): the flag is flipped, imm =
 *     q & 0xFFFF, and PreprocessSingle(q) — a float type: block q's exponent
 *     into imm byte 2 and no payload word written (the buffer keeps its bytes,
 *     as at ppp.cc); INT32: block q byte-swapped into the buffer, its real
 *     words only — and d_sends[q] = {worker, rkey = ((first_slot + q) *
 *     pkts_per_msg) << 1 | flag, imm, src = src_base + q, addr = q * 4 *
 *     msg_numel};
 *   b <= q < Q: d_sends[q] is the null record: worker = 0xFFFFFFFF, every other
 *     field 0.  sml_rdma_switch answers it IGNORED, so a d_sends array can be
 *     handed to the switch as it is.
 *   numel == 0: SML_OK, b = 0, every record null.
 *
 * sml_rdma_worker_poll (:206-260) over the n completions {qpn = wr_id & 0xFFFF,
 * imm = imm_data in host order}; the state is judged as it stands at the start
 * of the call.
 *   Record i is IGNORED when qpn >= b or that QP has msg_id >= total (a worker
 *   with no slice begun has b = 0).  Otherwise it is a candidate when
 *   (imm & 0xFFFF) == (msg_id[qpn] & 0xFFFF), else WRONG.  Among a QP's
 *   candidates in one call the lowest index is accepted and the rest are WRONG:
 *   the QP's next message is sent only after the call returns, so a second
 *   match is a duplicate delivery of the same message.  A WRONG or IGNORED
 *   record changes nothing: no byte of tx, d_out or the state.
 *   An accepted record, message m on QP q, in this order (the exponent read
 *   precedes its overwrite):
 *     PostprocessSingle(m) — a float type: m >= b: block m - b dequantized from
 *       rx under the exponent kept for q, its real words, narrowed (round to
 *       nearest even) for the 16-bit types; m < B: the QP keeps imm byte 2 as a
 *       signed int8.  INT32: block m byte-swapped into d_out;
 *     msg_id += b; still below total -> PostSendWr: the flag is flipped; a
 *       float type: block m quantized under the exponent just received into
 *       tx, real words only, and block m + b's exponent into imm byte 2 (0
 *       when m + b >= B); INT32: block m + b byte-swapped into tx; d_sends[i]
 *       is the record and the verdict POSTED.  Else the verdict is FINISHED.
 *   Every d_sends[i] that is not POSTED is the null record.  d_counts[v] is
 *   added to per verdict; the slice is complete when POSTED + FINISHED have
 *   summed to total.  imm byte 3 is sent as 0 and ignored on receipt.
 *
 * sml_rdma_worker_resend (PostSendWr(qpn, true), :287-291): d_sends[i] is QP
 * d_qpns[i]'s outstanding message again — same flag, imm, src and addr — or
 * the null record for a QP outside the slice or one that has finished.
 * Nothing else changes.
 *
 *   d_state: sml_rdma_worker_state_bytes() bytes of device memory, 16-byte
 *     aligned, opaque; sml_rdma_worker_reset before the first call;
 *   d_completions: sml_rdma_completion[n]; d_sends: sml_rdma_arrival[Q] (begin)
 *     or [n]; d_qpns: uint32[n]; d_verdict: uint8[n]; d_counts: uint64[4],
 *     nullable; device memory, 8-byte aligned (d_qpns: 4).
 * Status, every check before any launch: params NULL, num_workers == 0, or a
 * NULL pointer with work to do (begin: d_state, d_sends, and with numel > 0
 * d_in, d_out, tx; poll, n > 0: d_completions, d_state, rx, tx, d_sends,
 * d_verdict; resend, n > 0: d_qpns, d_state, d_sends) -> SML_ERR_INVALID_ARG;
 * msg_numel not a packet size, pkts_per_msg not one of 1, 2, 4, 8, 16, num_qps
 * not in 1..16384, first_slot + num_qps > 16384, data_type not one of the
 * four, n >= 2^31 -> SML_ERR_UNSUPPORTED; n == 0 -> SML_OK, nothing launched;
 * rx / tx / d_state / the slice / a record array off its alignment ->
 * SML_ERR_ALIGNMENT.  poll and resend take the slice from d_state: their
 * params are the ones begin was given.
 * Calls on one state are ordered by their stream, one at a time.  Launches:
 * reset, begin (a wave per QP) and resend (a thread per entry) one each; poll
 * two — judge (a thread per completion: IGNORED / WRONG written, a candidate
 * claims its QP with an atomic min of its index) and accept (a wave per
 * completion: the claim's holder loads the result, the QP's state and the two
 * blocks of the slice, waits once, and only then writes d_out, tx, the state
 * and its record). */
#ifndef SWITCHML_RDMA_WORKER_H_
#define SWITCHML_RDMA_WORKER_H_

#include "switchml_rdma_switch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sml_rdma_completion {
    uint32_t qpn;      /* wr_id & 0xFFFF: the QP's index in its worker thread */
    uint32_t imm;      /* imm_data, host order: bits 0-15 msg_id, byte 2 = the exponent */
} sml_rdma_completion;

typedef struct sml_rdma_worker_params {
    uint32_t worker;        /* this worker's index in the records it emits */
    uint16_t num_workers;   /* W of the scale */
    uint16_t data_type;     /* SML_FLOAT32, SML_INT32, SML_FLOAT16, SML_BFLOAT16 */
    uint32_t msg_numel;     /* M: 64..1024 (a packet size) */
    uint32_t pkts_per_msg;  /* 1,2,4,8,16 */
    uint32_t num_qps;       /* Q = max_outstanding_msgs, 1..16384 */
    uint32_t first_slot;    /* message slot of QP 0 (queue_pairs * tid, :121-125); first_slot + Q <= 16384 */
    uint32_t src_base;      /* QP q's message is message src_base + q of the switch's landing region */
    uint32_t flags;         /* SML_FLAG_ROUND_RNE */
} sml_rdma_worker_params;

/* sml_rdma_worker_poll's verdict per completion */
#define SML_RDMA_WORKER_WRONG    0   /* stats_wrong_pkts_received: duplicate or unexpected id */
#define SML_RDMA_WORKER_POSTED   1   /* accepted; the QP's next message is built, d_sends[i] is its record */
#define SML_RDMA_WORKER_FINISHED 2   /* accepted; the QP has no further message in this slice */
#define SML_RDMA_WORKER_IGNORED  3   /* qpn is not a QP of the slice under way, or that QP has finished */

/* Bytes of d_state for num_qps queue pairs; 0 on an unsupported num_qps. */
uint64_t sml_rdma_worker_state_bytes(uint32_t num_qps);
/* One small kernel on `stream`.  Status: d_state NULL -> SML_ERR_INVALID_ARG;
 * bad num_qps -> SML_ERR_UNSUPPORTED; d_state not 16-byte aligned ->
 * SML_ERR_ALIGNMENT. */
sml_status_t sml_rdma_worker_reset(void* d_state, uint32_t num_qps, void* stream);
sml_status_t sml_rdma_worker_begin(const sml_rdma_worker_params* params, const void* d_in, void* d_out,
                                   uint64_t numel, void* d_state, void* tx, sml_rdma_arrival* d_sends, void* stream);
sml_status_t sml_rdma_worker_poll(const sml_rdma_worker_params* params, const sml_rdma_completion* d_completions,
                                  uint64_t n, void* d_state, const void* rx, void* tx, sml_rdma_arrival* d_sends,
                                  uint8_t* d_verdict, uint64_t* d_counts, void* stream);
sml_status_t sml_rdma_worker_resend(const sml_rdma_worker_params* params, const uint32_t* d_qpns, uint64_t n,
                                    void* d_state, sml_rdma_arrival* d_sends, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_RDMA_WORKER_H_ */
