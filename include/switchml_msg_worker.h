/* switchml_msg_worker.h — the worker's side of LONG RDMA messages (SURVEY §8
 * F4), part of the C ABI of libswitchml_hip.so: switchml_hip.h includes it
 * beside the other sub-headers, and a caller includes switchml_hip.h.  Symbols
 * are only added: sml_abi_version() stays as it is.
 *
 * The RDMA backend's message is any multiple of its packet size
 * (rdma_worker_thread.cc:86-88, config.cc:185-192).  The sml_msg_* entry points
 * (switchml_messages.h) quantize such messages and sml_msg_switch
 * (switchml_msg_switch.h) is the slot pool they are sent to; these five are the
 * worker's completion loop that drives it message by message:
 * sml_rdma_worker_state_bytes / _reset / _begin / _poll / _resend
 * (switchml_rdma_worker.h) in everything — the parameter structure, the
 * completion and arrival records, the verdict codes, the semantics word for
 * word (B, b, total; the judge rule, the lowest index winning among a QP's
 * candidates; PostprocessSingle, then msg_id += b, then PostSendWr; the null
 * records; resend; d_counts), the buffers' requirements, and the argument
 * checks: same order, same status per cause, all before any launch — except
 * what they accept:
 *   msg_numel:    any value for which sml_msg_numel_supported() returns 1 (a
 *                 multiple of 64 from 64 to 16384);
 *   pkts_per_msg: any integer 1..256, so the record's rkey is
 *                 ((first_slot + q) * pkts_per_msg) << 1 | flag.
 * num_qps 1..16384 and first_slot + num_qps <= 16384 as there; FLOAT32,
 * FLOAT16, BFLOAT16 and INT32; SML_FLAG_ROUND_RNE as in sml_msg_quantize_pack:
 * the VCL body is the first n - n % 16 real elements of each message.
 * d_state has sml_rdma_worker's layout (64 bytes + 32 per QP), and a state
 * reset by one family can be driven by the other.  Where both families take
 * the arguments, the results are the same bit for bit.
 * Status: as the sml_rdma_worker_* calls, with "msg_numel not a packet size"
 * read as "msg_numel unsupported" and "pkts_per_msg not one of 1, 2, 4, 8, 16"
 * as "pkts_per_msg not in 1..256".
 * Launches: reset, resend and poll's judge pass are sml_rdma_worker's kernels.
 * begin is a workgroup of ceil(msg_numel / 1024) waves per QP, poll's accept
 * pass a workgroup of that many waves per completion: a message's 256-word
 * slices are dealt round-robin to the waves (at most 4 a wave), each wave
 * loads its slices of the result, of the next message's block and of the block
 * whose exponent goes out with it, waits once, and stores; the block's
 * maximum crosses the waves through LDS and one barrier, behind which one lane
 * writes the QP's state, the send record and the verdict. */
#ifndef SWITCHML_MSG_WORKER_H_
#define SWITCHML_MSG_WORKER_H_

#include "switchml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_state for num_qps queue pairs; 0 on an unsupported num_qps. */
uint64_t sml_msg_worker_state_bytes(uint32_t num_qps);
/* One small kernel on `stream`.  Status as sml_rdma_worker_reset. */
sml_status_t sml_msg_worker_reset(void* d_state, uint32_t num_qps, void* stream);
sml_status_t sml_msg_worker_begin(const sml_rdma_worker_params* params, const void* d_in, void* d_out,
                                  uint64_t numel, void* d_state, void* tx, sml_rdma_arrival* d_sends, void* stream);
sml_status_t sml_msg_worker_poll(const sml_rdma_worker_params* params, const sml_rdma_completion* d_completions,
                                 uint64_t n, void* d_state, const void* rx, void* tx, sml_rdma_arrival* d_sends,
                                 uint8_t* d_verdict, uint64_t* d_counts, void* stream);
sml_status_t sml_msg_worker_resend(const sml_rdma_worker_params* params, const uint32_t* d_qpns, uint64_t n,
                                   void* d_state, sml_rdma_arrival* d_sends, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_MSG_WORKER_H_ */
