/* switchml_msg_switch.h — the switch's side of LONG RDMA messages (SURVEY §8
 * F4), part of the C ABI of libswitchml_hip.so: switchml_hip.h includes it
 * beside the other sub-headers, and a caller includes switchml_hip.h.  Symbols
 * are only added: sml_abi_version() stays as it is.
 *
 * The RDMA backend's message is any multiple of its packet size
 * (rdma_worker_thread.cc:86-88, config.cc:185-192), and the sml_msg_* entry
 * points (switchml_messages.h) quantize such messages on the worker's side.
 * These three are the switch such a worker talks to: sml_rdma_switch_state_bytes
 * / sml_rdma_switch_reset / sml_rdma_switch (switchml_rdma_switch.h) in
 * everything — the record and params structures, the rule record by record
 * (bitmap, count, write-or-add mod 2^32, signed int8 exponent max per byte,
 * BROADCAST / RETRANSMIT / CONSUMED / IGNORED / DEFERRED), the results (words
 * written htonl at rx + u * rx_bytes + addr, d_out_imm as set_immediate builds
 * it), d_counts, deferral and its stated limits, the buffers' requirements, and
 * the argument checks: same order, same status per cause, all before any
 * launch — except what they accept:
 *   msg_numel:    any value for which sml_msg_numel_supported() returns 1 (a
 *                 multiple of 64 from 64 to 16384);
 *   pkts_per_msg: any integer 1..256.
 * The record grid stays (rkey >> 1) % pkts_per_msg == 0 and the slot
 * (rkey >> 1) / pkts_per_msg; num_workers 1..32, num_slots 1..16384.  d_state
 * has sml_rdma_switch's layout with msg_numel general (the accumulators are
 * 8 * num_slots * msg_numel bytes) and is sized, cleared and used by this
 * family only.  Where both families take the arguments, the results are the
 * same bit for bit.
 * Status: as sml_rdma_switch, with "msg_numel not a packet size" read as
 * "msg_numel unsupported" and "pkts_per_msg not one of 1, 2, 4, 8, 16" as
 * "pkts_per_msg not in 1..256".
 * Four launches on `stream`: claim and verdicts (thread per record, as
 * sml_rdma_switch's), the data pass (wave per touched slot and item of up to
 * 4 x 256 words dealt round-robin over the message: the new contributors'
 * slices summed in registers, written to the accumulator and, swapped once, to
 * the receive regions of the slot's result records) and the commit pass (wave
 * per touched slot: bitmap, count, exponents, immediates, per-call scratch). */
#ifndef SWITCHML_MSG_SWITCH_H_
#define SWITCHML_MSG_SWITCH_H_

#include "switchml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_state for a pool of num_slots message slots of msg_numel words; 0
 * on an unsupported msg_numel or num_slots. */
uint64_t sml_msg_switch_state_bytes(uint32_t num_slots, uint32_t msg_numel);
/* Clear the switch's registers: one async memset on `stream`.  Status as
 * sml_rdma_switch_reset. */
sml_status_t sml_msg_switch_reset(void* d_state, uint32_t num_slots, uint32_t msg_numel, void* stream);
sml_status_t sml_msg_switch(const sml_rdma_switch_params* params, const sml_rdma_arrival* d_arrivals, uint64_t n,
                            const void* landing, uint64_t landing_stride, uint64_t landing_msgs,
                            void* d_state, void* rx, uint64_t rx_bytes, const uint32_t* d_drop,
                            uint32_t* d_out_imm, uint8_t* d_verdict, uint64_t* d_counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_MSG_SWITCH_H_ */
