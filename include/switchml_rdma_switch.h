/* switchml_rdma_switch.h — the switch's side of the RDMA messages (SURVEY §8
 * F4), part of the C ABI of libswitchml_hip.so: switchml_hip.h includes it
 * beside the frame switch, and a caller includes switchml_hip.h.  Symbols are
 * only added: sml_abi_version() stays as it is.
 *
 * What the Tofino pipeline does to the RDMA messages W workers send it, at
 * message granularity, a batch of landed messages per call, with the switch's
 * registers in d_state across calls.  RoCE frames never reach the GPU — the
 * NIC terminates them, and on a UC queue pair it completes a message whole or
 * not at all (p4/rdma_receiver.p4's PSN rule) — so a call sees whole messages,
 * landed 16-byte aligned in a registered region, and one completion record per
 * message (an ibv_poll_cq loop fills them: INTEGRATION.md):
 *   worker: the queue pair's worker, 0..num_workers-1;
 *   rkey:   the pool index as rdma_worker_thread.cc:118-128 builds it: bit 0 =
 *           the set, bits 1.. = message slot * pkts_per_msg;
 *   imm:    imm_data in host order: bits 0-15 msg_id, byte 2 = e0, byte 3 = e1
 *           (sml_rdma_imm / sml_rdma_imm_int32 build it);
 *   src:    the message's msg_numel big-endian words start at
 *           landing + src * landing_stride;
 *   addr:   the RETH address: the byte offset of the result in every worker's
 *           receive region.
 * Slot s = (rkey >> 1) / pkts_per_msg, set v = rkey & 1.  A record with
 * (rkey >> 1) % pkts_per_msg != 0, s >= num_slots, worker >= num_workers,
 * src >= landing_msgs, addr not 16-byte aligned or addr + 4 * msg_numel >
 * rx_bytes is IGNORED and nothing changes.  Otherwise the rule is
 * sml_frame_switch's (switchml_hip.h), record by record in index order
 * (p4/bitmap_checker.p4, p4/workers_counter.p4, p4/processor.p4:48-54,
 * p4/exponents.p4:48-54, p4/next_step_selector.p4):
 *   before = bitmap[s][v]; bitmap[s][v] |= 1 << worker; bitmap[s][1-v] &= ~(1 << worker);
 *   not a retransmission (before has no bit `worker`): flag = count[s][v], then
 *     count = count == 0 ? W - 1 : count - 1 (W == 1: flag = 1); the slot's
 *     msg_numel words, e0 and e1 are WRITTEN when before == 0, else the words are
 *     added mod 2^32 (ntohl first) and e0, e1 take the signed int8 max, each on
 *     its own; flag == 1 -> BROADCAST, else CONSUMED;
 *   a retransmission: flag = count[s][v], unchanged (W == 1: flag = 0);
 *     flag == 0, a full slot -> RETRANSMIT, else CONSUMED.
 * The results are p4/rdma_sender.p4's, on the sending side of the NIC:
 *   BROADCAST at record i: the slot's words (htonl) are written at
 *     rx + u * rx_bytes + addr_i for every worker u whose bit in d_drop[i] is
 *     clear (d_drop NULL: nothing dropped);
 *   RETRANSMIT: the same to the asking worker only (its drop bit applies);
 *   both: d_out_imm[i] = (imm_i & 0xFFFF) | e0 << 16 | e1 << 24 (set_immediate:
 *     the triggering message's id, the slot's exponents);
 *   any other verdict: d_out_imm[i] and every receive region stay untouched.
 * d_counts[0..4] are added to by verdict (SML_VERDICT_*), d_counts[5] by the
 * copies a drop bit kept from being written.
 *   One call is that pipeline over the call's records in index order, under
 * sml_frame_switch's rule and with its stated limits: per (slot, worker) the
 * call handles the records of the set that pair's lowest-index record carries;
 * the pair's records of the other set come back DEFERRED, change nothing and
 * are resubmitted by the caller.  Equal to the sequential pipeline for streams
 * that follow the worker protocol; for any other stream verdicts, bitmaps and
 * counts are still the pipeline's and a result carries the slot's words and
 * exponents as they stand at the END of the call.  Two results of one call to
 * the same address of the same worker are written in no particular order.
 *   d_arrivals: sml_rdma_arrival[n], device memory, 8-byte aligned;
 *   landing, rx: device memory or pinned, device-mapped host memory, 16-byte
 *     aligned; landing_stride >= 4 * msg_numel and a multiple of 16; rx holds
 *     num_workers regions of rx_bytes (a multiple of 16) each;
 *   d_state: sml_rdma_switch_state_bytes() bytes of device memory, 16-byte
 *     aligned, opaque, cleared by sml_rdma_switch_reset before the first call;
 *   d_drop: uint32[n] or NULL; d_out_imm: uint32[n]; d_verdict: uint8[n];
 *     d_counts: uint64[6], nullable, 8-byte aligned; device memory.  Between
 *     the launches of a call d_out_imm[i] of a result record holds scratch.
 * Status, every check before any launch: params NULL, or (n > 0) a NULL
 * d_arrivals / landing / d_state / rx / d_out_imm / d_verdict ->
 * SML_ERR_INVALID_ARG; msg_numel not a packet size, pkts_per_msg not one of
 * 1, 2, 4, 8, 16, num_workers not in 1..32, num_slots not in 1..16384, n >=
 * 2^31 -> SML_ERR_UNSUPPORTED; n == 0 -> SML_OK, nothing launched; a buffer or
 * stride off its alignment (landing_stride < 4 * msg_numel included) ->
 * SML_ERR_ALIGNMENT.
 * Three launches on `stream`: claim (thread per record), verdicts (thread per
 * record; a result record joins its slot's list), apply and results (wave per
 * touched slot: the new contributors' messages summed in registers, the
 * registers advanced, and the sum written from registers to the receive
 * regions of the slot's result records).
 *   Messages of more than 1024 words, and any pkts_per_msg up to 256: the
 * sml_msg_switch* twins of these three calls (switchml_msg_switch.h). */
#ifndef SWITCHML_RDMA_SWITCH_H_
#define SWITCHML_RDMA_SWITCH_H_

#include "switchml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sml_rdma_arrival {
    uint32_t worker;   /* index 0..W-1 (the QP's worker; >= W: IGNORED) */
    uint32_t rkey;     /* bit 0 = set, bits 1.. = message slot * pkts_per_msg */
    uint32_t imm;      /* imm_data, host order: bits 0-15 msg_id, byte 2 = e0, byte 3 = e1 */
    uint32_t src;      /* the message's payload = landing + src * landing_stride */
    uint64_t addr;     /* RETH address: byte offset of the result in every worker's receive region */
} sml_rdma_arrival;

typedef struct sml_rdma_switch_params {
    uint16_t num_workers;     /* 1..32 */
    uint32_t num_slots;       /* 1..16384 message slots, two sets each */
    uint32_t msg_numel;       /* 64,128,256,512,1024 */
    uint32_t pkts_per_msg;    /* 1,2,4,8,16: msg_numel / the MTU's packet_numel */
} sml_rdma_switch_params;

/* Bytes of d_state for a pool of num_slots message slots of msg_numel words; 0
 * on an unsupported msg_numel or num_slots. */
uint64_t sml_rdma_switch_state_bytes(uint32_t num_slots, uint32_t msg_numel);
/* Clear the switch's registers (bitmaps, counts, the per-call scratch): one
 * async memset on `stream`.  Status: d_state NULL -> SML_ERR_INVALID_ARG; bad
 * num_slots / msg_numel -> SML_ERR_UNSUPPORTED; d_state not 16-byte aligned ->
 * SML_ERR_ALIGNMENT. */
sml_status_t sml_rdma_switch_reset(void* d_state, uint32_t num_slots, uint32_t msg_numel, void* stream);
sml_status_t sml_rdma_switch(const sml_rdma_switch_params* params, const sml_rdma_arrival* d_arrivals, uint64_t n,
                             const void* landing, uint64_t landing_stride, uint64_t landing_msgs,
                             void* d_state, void* rx, uint64_t rx_bytes, const uint32_t* d_drop,
                             uint32_t* d_out_imm, uint8_t* d_verdict, uint64_t* d_counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_RDMA_SWITCH_H_ */
