/*
 * switchml_hip.h — C-ABI of the MI355X-native SwitchML end-host
 * pre/post-processor (exponent quantizer) and its loopback/switch helpers.
 *
 * This is the drop-in boundary for the hot path of SwitchML's client_lib:
 * what `CpuExponentQuantizerPPP` (client_lib/src/prepostprocessors/
 * cpu_exponent_quantizer_ppp.{h,cc}) does one 1 KiB LTU at a time on the
 * CPU, these entry points do for a whole job slice at once on the GPU — the
 * "bulk" hooks the reference reserved in prepostprocessor.h:112-116.
 *
 * Conventions
 *  - plain C types only; every pointer argument named d_* is DEVICE memory
 *    (hipMalloc / torch CUDA tensor); `stream` is a hipStream_t passed as
 *    void* (NULL = the legacy default stream).  Calls are asynchronous on
 *    that stream, like every HIP launch.
 *  - no exceptions cross this ABI; every entry point returns sml_status_t.
 *    The reference aborts with LOG(FATAL) on a bad data type / PPP name
 *    (ppp.cc:190,297; prepostprocessor.cc:39); here that is an error code.
 *  - "job slice" = one contiguous run of `numel` elements, exactly what a
 *    worker thread receives from FifoScheduler::GetJobSlice
 *    (schedulers/fifo_scheduler.cc:93-109).  Blocks (LTUs) restart at the
 *    slice start.  Block k covers elements [k*P, min((k+1)*P, numel)).
 *  - planes: the per-packet exponent plane `exps[B]` (int8, byte 0 of the
 *    reference's 2-byte extra-info slot) and the payload plane `payload[B*P]`
 *    (int32, big-endian by default = the packet's wire bytes).  Packet p of
 *    the reference's stream carries exps[p] (p < B) and payload block p-b
 *    (p >= b); see DESIGN.md §2 and SURVEY.md §8 A6.  Payload words of the
 *    last, partial block past `numel` are written as 0 (the reference
 *    leaves stale ring bytes there).
 *  - B = sml_num_blocks(numel, P) = ceil(numel / P)   (ppp.cc:56-57)
 *
 * All file:line citations are relative to /root/reference/dev_root/.
 */
#ifndef SWITCHML_HIP_H_
#define SWITCHML_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SML_ABI_VERSION 2   /* 2: flags on sml_switch_exps / sml_copy_segments, sml_release_to_peers */

typedef enum {
    SML_OK = 0,
    SML_ERR_INVALID_ARG = 1,   /* null pointer with numel > 0, bad W, ... */
    SML_ERR_UNSUPPORTED = 2,   /* packet_numel not in {64,128,256,512,1024}, bad dtype */
    SML_ERR_ALIGNMENT = 3,     /* payload plane not 16-byte aligned */
    SML_ERR_HIP = 4            /* a HIP runtime call or launch failed */
} sml_status_t;

/* client_lib/src/common.h:51-55 */
typedef enum {
    SML_FLOAT32 = 0,
    SML_INT32 = 1,
    SML_FLOAT16 = 2,    /* IEEE binary16; the sml_*_typed entry points only */
    SML_BFLOAT16 = 3    /* bfloat16; the sml_*_typed entry points only */
} sml_data_type_t;

/* flags for the quantize / dequantize entry points */
#define SML_FLAG_PAYLOAD_LE   0x1u  /* payload plane in host (little-endian) order: the
                                       form RCCL can sum (switch-sim mode); default is
                                       big-endian wire order as htonl() at ppp.cc:103 */
#define SML_FLAG_ROUND_RNE    0x2u  /* VCL=1 semantics (ppp.cc:88-99): round-to-nearest-even
                                       on the 16-aligned body of each block, scalar
                                       half-away tail; out-of-range -> INT32_MIN.
                                       PARITY UNPINNED (VCL is un-vendored). Default is the
                                       VCL=0 scalar path: roundf half-away-from-zero. */
#define SML_FLAG_PEER_PLANES  0x4u  /* the switch entry points (sml_switch_aggregate,
                                       sml_switch_exps, sml_copy_segments): some input
                                       planes were written by OTHER GPUs (peers' HBM mapped
                                       over xGMI).  Every workgroup performs a system-scope
                                       acquire before its first load, so no copy of a peer
                                       line this GPU cached before the peer rewrote it is
                                       read; the peer must have run sml_release_to_peers
                                       after its writes (memory model). */

int sml_abi_version(void);
const char* sml_status_string(sml_status_t s);
/* Last HIP error string seen by this library on the calling thread ("" if none). */
const char* sml_last_error(void);

/* ceil(numel*4 / (packet_numel*4)) — CpuExponentQuantizerPPP::SetupJobSlice, ppp.cc:54-62 */
uint64_t sml_num_blocks(uint64_t numel, uint32_t packet_numel);

/* Host: scale factors for all 256 int8 exponents, lut[(uint8_t)e] =
 *   (float)(double(INT32_MAX) / (num_workers * powf(2, e)))
 * — the scale PostprocessSingle stores from the received global exponent,
 * ppp.cc:254-260.  num_workers >= 1. */
sml_status_t sml_scale_lut(uint16_t num_workers, float lut[256]);

/* Device: the same 256 scales as computed INSIDE the kernels (test hook that
 * proves the device formula equals sml_scale_lut bit for bit). d_lut: float[256]. */
sml_status_t sml_scale_lut_device(uint16_t num_workers, float* d_lut, void* stream);

/* K2 — exponent plane only: d_exps[k] = int8 exponent of block k (max |x|,
 * NaN skipped, ((bits & 0x7f800000) >> 23) - 126) — the exponent half of
 * PreprocessSingle, ppp.cc:115-156.  Used before the exponent exchange in
 * switch-sim mode (the switch's signed int8 max, p4/exponents.p4:48-54). */
sml_status_t sml_exponents(const float* d_in, uint64_t numel, uint32_t packet_numel,
                           int8_t* d_exps, void* stream);

/* K1 / K3 — quantize + pack, the quantize half of PreprocessSingle
 * (ppp.cc:72-113):  payload[k*P+i] = htonl((int32)roundf(x[k*P+i] * scale(W, e_k)))
 *  - d_global_exps == NULL  (K1, fused): e_k is the block's own exponent, as
 *    the dummy/loopback backend returns it unchanged (dummy_backend.cc:72-84);
 *    d_exps_out (nullable) receives the exponent plane.
 *  - d_global_exps != NULL  (K3): e_k = d_global_exps[k], the switch's
 *    aggregated exponent; d_exps_out must be NULL or equal to it (not written).
 *  d_payload: int32[B*P], 16-byte aligned.  d_in may have any 4-byte alignment
 *  (slices start at arbitrary element offsets). */
sml_status_t sml_quantize_pack(const float* d_in, uint64_t numel, uint32_t packet_numel,
                               uint16_t num_workers, const int8_t* d_global_exps,
                               int32_t* d_payload, int8_t* d_exps_out,
                               uint32_t flags, void* stream);

/* K4 — dequantize the aggregated payload, the dequantize half of
 * PostprocessSingle (ppp.cc:197-251):
 *   out[k*P+i] = (float)(int32)ntohl(payload[k*P+i]) / scale(W, exps[k])
 * (int->float RNE, IEEE division).  Only `numel` outputs are written.
 * d_out may have any 4-byte alignment; d_payload 16-byte aligned. */
sml_status_t sml_dequantize(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel,
                            uint32_t packet_numel, uint16_t num_workers, float* d_out,
                            uint32_t flags, void* stream);

/* INT32 jobs — byte-order conversion only (ppp.cc:158-190 pre, 262-298 post).
 * d_out[i] = bswap32(d_in[i]) for i < numel; in == out allowed. */
sml_status_t sml_bswap_i32(const int32_t* d_in, int32_t* d_out, uint64_t numel, void* stream);

/* K5 — the dummy backend's "switch": every BE payload word is multiplied by
 * num_workers with int32 wrap-around, exponents pass through unchanged
 * (DummyBackend::ProcessPacket, client_lib/src/backends/dummy/dummy_backend.cc:72-84).
 * count = B*P words (stale/zero tails included, as the reference does). */
sml_status_t sml_loopback_aggregate(int32_t* d_payload, uint64_t count, uint16_t num_workers,
                                    uint32_t flags, void* stream);

/* Fused loopback round trip for FLOAT32 (dummy backend, one pass over HBM):
 * exponent -> quantize -> x num_workers -> dequantize, writing d_out[numel]
 * and, when d_payload != NULL, the on-wire payload plane as sent (before the
 * loopback multiply) and d_exps_out.  Bit-identical to K1 -> K5 -> K4. */
sml_status_t sml_roundtrip_loopback(const float* d_in, float* d_out, uint64_t numel,
                                    uint32_t packet_numel, uint16_t num_workers,
                                    int32_t* d_payload, int8_t* d_exps_out,
                                    uint32_t flags, void* stream);

/* The fused round trip over a batch of job slices in ONE launch (the
 * client's worker submits every slice of the jobs queued so far together):
 * slice i is exactly sml_roundtrip_loopback(in, out, numel, ...) — its blocks
 * start at its own first element (FIFO slices, fifo_scheduler.cc:93-109) — and
 * no payload / exponent planes are written.  Any 4-byte alignment; slices
 * must not overlap each other (a slice's in == out is fine); numel == 0
 * slices are skipped.  Flags: SML_FLAG_ROUND_RNE (the payload byte order is
 * not observable here). */
#define SML_MAX_BATCH_SLICES 64
typedef struct sml_slice {
    const float* in;
    float* out;
    uint64_t numel;
} sml_slice;
sml_status_t sml_roundtrip_loopback_batch(const sml_slice* slices, uint32_t num_slices, uint32_t packet_numel,
                                          uint16_t num_workers, uint32_t flags, void* stream);

/* ---- The switch's aggregation ---------------------------
 * K6: what the Tofino pipeline does to W workers' packets for one slot, over
 * whole planes, fused with the worker's dequantize:
 *   d_payload_out[i] = htonl(sum_w ntohl(d_payloads[w][i]))  wrapping bit<32>
 *                      (p4/processor.p4:48-54; LE words with
 *                      SML_FLAG_PAYLOAD_LE: no swaps), i < B*P
 *   d_exps_out[k]    = max_w (int8) d_exps[w][k]   (p4/exponents.p4:48-54)
 *   d_out[i]         = (float)(int32)sum_i / scale(W, e_max[i/P]), i < numel
 *                      (PostprocessSingle, ppp.cc:197-251; W = num_workers)
 * d_payloads / d_exps are HOST arrays of num_workers DEVICE pointers: local
 * buffers, or peers' HBM mapped over xGMI (hipIpcOpenMemHandle) — the
 * peer-to-peer switch.  Any of the three outputs may be NULL (not all);
 * d_exps may be NULL when d_exps_out and d_out are.  Payload planes 16-byte
 * aligned (B*P words each); d_payload_out may alias d_payloads[w].
 * num_workers <= SML_MAX_SWITCH_WORKERS. */
#define SML_MAX_SWITCH_WORKERS 16
sml_status_t sml_switch_aggregate(const int32_t* const* d_payloads, const int8_t* const* d_exps,
                                  uint16_t num_workers, uint64_t numel, uint32_t packet_numel,
                                  int32_t* d_payload_out, int8_t* d_exps_out, float* d_out,
                                  uint32_t flags, void* stream);

/* ---- FLOAT16 / BFLOAT16 job slices ----------------------------------------
 * The typed counterparts of sml_exponents, sml_quantize_pack, sml_dequantize,
 * sml_roundtrip_loopback and sml_switch_aggregate: the same argument lists,
 * with void* for the typed buffer and its sml_data_type_t next to it.
 *   SML_FLOAT16 / SML_BFLOAT16: the kernels convert.  x32[i] = (float)x[i]
 *     (exact) right after the load; everything between is the FLOAT32 path on
 *     x32, unchanged (block exponent, scale, roundf or SML_FLAG_ROUND_RNE, the
 *     big-endian pack, the dequantize to an fp32 y32); y[i] = (T)y32[i], round
 *     to nearest even, right before the store (overflow -> +-inf, fp16 results
 *     below the normal range -> fp16 denormals, NaN -> a NaN of T).  The planes
 *     are the FLOAT32 ones: int32 payload words and one int8 exponent per
 *     packet of P elements, B = ceil(numel / P) whatever the element size.
 *   SML_FLOAT32: the untyped entry point, exactly.  No check of the typed
 *     function's own comes before the fp32 twin's, so for every argument
 *     list — several faults at once included — the call returns the status,
 *     runs the kernels and writes the bits of its fp32 twin.  This holds for
 *     every sml_*_typed entry point of this header (the batch, the frames and
 *     sml_copy_segments_typed among them).
 *   SML_INT32 (or any other value): SML_ERR_UNSUPPORTED.
 * Typed buffers of a 16-bit type need 2-byte alignment only (a slice starts
 * at any element) and no byte outside [ptr, ptr + 2 * numel) is touched;
 * payload planes 16-byte aligned, as above.  in == out is allowed for the
 * round trip.  Batches of 16-bit slices go through
 * sml_roundtrip_loopback_batch_typed (below), DPDK frames through
 * sml_quantize_pack_frames_typed / sml_dequantize_frames_typed (with the
 * frames, below), the in-node switch's multicast of a 16-bit shard through
 * sml_copy_segments_typed (with sml_copy_segments, below).  A 16-bit slice's RDMA messages need no entry point of
 * their own: sml_quantize_pack_typed at packet_numel = msg_numel gives the
 * message payloads and sml_rdma_imm on its exponent plane the immediates.
 * Per-packet bursts of a 16-bit slice go through sml_preprocess_burst_typed /
 * sml_postprocess_burst_typed / sml_exchange_burst_typed (with the bursts,
 * below).  The untyped burst entry points, the burst server and
 * sml_roundtrip_loopback_batch take no 16-bit type (a burst whose data_type
 * is one returns SML_ERR_UNSUPPORTED there). */
sml_status_t sml_exponents_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel,
                                 uint32_t packet_numel, int8_t* d_exps, void* stream);
sml_status_t sml_quantize_pack_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel,
                                     uint32_t packet_numel, uint16_t num_workers,
                                     const int8_t* d_global_exps, int32_t* d_payload, int8_t* d_exps_out,
                                     uint32_t flags, void* stream);
sml_status_t sml_dequantize_typed(const int32_t* d_payload, const int8_t* d_exps, uint64_t numel,
                                  uint32_t packet_numel, uint16_t num_workers, void* d_out,
                                  sml_data_type_t data_type, uint32_t flags, void* stream);
sml_status_t sml_roundtrip_loopback_typed(const void* d_in, void* d_out, sml_data_type_t data_type,
                                          uint64_t numel, uint32_t packet_numel, uint16_t num_workers,
                                          int32_t* d_payload, int8_t* d_exps_out,
                                          uint32_t flags, void* stream);
sml_status_t sml_switch_aggregate_typed(const int32_t* const* d_payloads, const int8_t* const* d_exps,
                                        uint16_t num_workers, uint64_t numel, uint32_t packet_numel,
                                        int32_t* d_payload_out, int8_t* d_exps_out, void* d_out,
                                        sml_data_type_t data_type, uint32_t flags, void* stream);

/* The batched round trip over slices of any float type (what the client's
 * batch worker sends: the FIFO slices of the FLOAT32, FLOAT16 and BFLOAT16
 * jobs queued so far).  Slice i gets exactly
 *   sml_roundtrip_loopback_typed(in, out, data_type, numel, packet_numel,
 *                                num_workers, NULL, NULL,
 *                                flags & SML_FLAG_ROUND_RNE, stream)
 * — its blocks start at its own first element, no planes are written.  Types
 * may be mixed in one call; at most SML_MAX_BATCH_SLICES slices over all
 * types; slices must not overlap each other (a slice's in == out is fine);
 * numel == 0 slices are skipped.  A 16-bit slice starts at any 2-byte
 * offset, an fp32 slice at any 4-byte offset, and no byte outside a slice is
 * read or written.
 *   Launches: at most one per element type present.  The FLOAT32 slices go
 * through sml_roundtrip_loopback_batch's kernel, each 16-bit type through its
 * own instance of the 16-bit batch kernel; a type with one non-empty slice
 * takes the single-slice kernel.  The order of these launches on `stream` is
 * unspecified — the slices do not overlap, so it cannot be observed.  Stores
 * are non-temporal when the call's total output (all slices, all types)
 * reaches sml_set_payload_nt_threshold.
 *   Every slice is checked before anything is launched, so a call that
 * returns one of these has launched nothing: SML_ERR_UNSUPPORTED for a bad
 * packet_numel, a slice whose data_type is SML_INT32 or any other value, or
 * more than 2^32 - 1 tiles in one launch; SML_ERR_INVALID_ARG for
 * num_workers == 0, num_slices > SML_MAX_BATCH_SLICES, slices == NULL with
 * num_slices > 0, a NULL in / out with numel > 0, a 16-bit slice not 2-byte
 * aligned, a FLOAT32 slice not 4-byte aligned, or reserved != 0.  A call
 * without a non-empty slice returns SML_OK and does not touch the device. */
typedef struct sml_typed_slice {
    const void* in;
    void* out;
    uint64_t numel;
    uint32_t data_type;   /* sml_data_type_t: SML_FLOAT32, SML_FLOAT16 or SML_BFLOAT16 */
    uint32_t reserved;    /* 0 */
} sml_typed_slice;
sml_status_t sml_roundtrip_loopback_batch_typed(const sml_typed_slice* slices, uint32_t num_slices,
                                                uint32_t packet_numel, uint16_t num_workers,
                                                uint32_t flags, void* stream);

/* The switch's exponent half alone (p4/exponents.p4:48-54): d_exps_out[k] =
 * max_w (int8) d_exps[w][k], k < num_blocks — W planes of num_blocks bytes
 * (local or mapped peers' planes; HOST array of DEVICE pointers).  Planes
 * and output at any byte alignment (one dword per plane and 4 blocks when all
 * are 4-byte aligned, bytes otherwise).
 * Status, in this order: num_workers == 0, d_exps NULL or d_exps_out NULL ->
 * SML_ERR_INVALID_ARG; num_workers > SML_MAX_SWITCH_WORKERS ->
 * SML_ERR_UNSUPPORTED; num_blocks == 0 -> SML_OK (nothing to do, the table is
 * not read); a NULL plane in the table -> SML_ERR_INVALID_ARG. */
sml_status_t sml_switch_exps(const int8_t* const* d_exps, uint16_t num_workers, uint64_t num_blocks,
                             int8_t* d_exps_out, uint32_t flags, void* stream);

/* Copy num_words 32-bit words (any 4-byte alignment; either side may be a
 * peer's mapped plane or pinned host memory): the all-gather step of the
 * in-node switch backend.  16-B accesses, the streaming kernels' tile shape.
 * Status: num_words == 0 -> SML_OK whatever the pointers; else a NULL
 * pointer or one not 4-byte aligned, on either side -> SML_ERR_INVALID_ARG. */
sml_status_t sml_copy_words(const void* d_src, void* d_dst, uint64_t num_words, void* stream);

/* Up to SML_MAX_SWITCH_WORKERS copies in ONE launch: d_dsts[i][0..n_i) =
 * d_srcs[i][0..n_i), n_i = num_words[i] (HOST arrays of DEVICE pointers, any
 * 4-byte alignment; segments must not overlap).  The in-node switch's
 * multicast: the tiles are dealt round-robin over the segments, so W peers'
 * shards come over their xGMI links at the same time, not one after another. */
sml_status_t sml_copy_segments(const void* const* d_srcs, void* const* d_dsts, const uint64_t* num_words,
                               uint32_t num_segments, uint32_t flags, void* stream);

/* The same multicast for a job of any type: d_dsts[i][0..n_i) =
 * d_srcs[i][0..n_i) as elements of data_type, n_i = numel[i].
 *   SML_FLOAT32 / SML_INT32: forwards to sml_copy_segments (same kernel,
 *     checks and bits).
 *   SML_FLOAT16 / SML_BFLOAT16: 2-byte elements.  A 16-bit shard ends on an
 *     odd element and lands in a slice that starts at any element, so every
 *     source and destination needs 2-byte alignment only, each independently,
 *     and n_i may be odd; no byte outside [dst, dst + 2 n_i) is written, none
 *     outside [src, src + 2 n_i) read.  Empty segments touch nothing; segments
 *     must not overlap.
 * Any other type: SML_ERR_UNSUPPORTED.  A NULL table, a NULL or odd pointer
 * with n_i > 0, or more than SML_MAX_SWITCH_WORKERS segments:
 * SML_ERR_INVALID_ARG.  Every check precedes the launch. */
sml_status_t sml_copy_segments_typed(const void* const* d_srcs, void* const* d_dsts, const uint64_t* numel,
                                     uint32_t num_segments, sml_data_type_t data_type, uint32_t flags, void* stream);

/* The writer's half of a hand-off to other GPUs: a system-scope release on
 * every XCD of the stream's device (each XCD's L2 writes its dirty lines back
 * to HBM), ordered after the work already on `stream`.  The in-node switch
 * runs it after the kernels that write planes peers will read, before the
 * stream synchronization that precedes the workers' barrier; the readers'
 * kernels then take SML_FLAG_PEER_PLANES (the acquire).  One small launch. */
sml_status_t sml_release_to_peers(void* stream);

/* ---- per-packet calls, a burst per launch ---------------------------------
 * PreprocessSingle / PostprocessSingle (ppp.cc:69-192, 194-299) for up to
 * SML_MAX_BURST packets of one job slice in ONE launch: the DPDK worker's rx
 * burst (PostprocessSingle per received packet, dpdk_worker_thread.cc:300-345)
 * and the tx burst it refills (ReusePacket -> PreprocessSingle of pkt_id + b,
 * dpdk_worker_thread_utils.inc:134,177), or an RDMA worker's completions
 * (rdma_worker_thread.cc:244,356).  entries[i] / extras[i] are packet i's
 * payload words and 2-byte extra-info slot, anywhere the DEVICE can address
 * (HBM, or pinned host memory such as a NIC's buffer pool) — read / written in
 * place.  Packet q of a FLOAT32 slice: preprocess writes block q - b's
 * quantized big-endian words (q >= b; only the block's real words, a partial
 * block's tail stays as it was) and block q's exponent into byte 0 of the
 * extra slot (q < B); postprocess dequantizes block q - b into `out` (q >= b)
 * and keeps the packet's exponent byte as block q's received exponent in
 * recv_exps[q] (q < B).  INT32 slices: byte swaps, packet q = block q.
 * recv_exps: DEVICE array of B int8 owned by the caller for the slice.  Bit-
 * identical to the per-packet calls in the reference's order; packet ids of a
 * burst are distinct and never include both q and q + b (the reference sends
 * q + b only after receiving q).  Flags: SML_FLAG_ROUND_RNE. */
#define SML_MAX_BURST 64
typedef struct {
    const float* in;          /* the job slice (int32 words for INT32; elements of data_type under */
    float* out;               /* the sml_*_burst_typed entry points, below: a C caller casts)      */
    uint64_t numel;
    uint32_t packet_numel;    /* P */
    uint16_t num_workers;     /* W */
    uint16_t data_type;       /* sml_data_type_t */
    uint64_t batch_num_ltus;  /* b (FLOAT32: the extra batch) */
    int8_t* recv_exps;
    uint32_t count;
    uint32_t flags;
    uint64_t pkt_ids[SML_MAX_BURST];
    void* entries[SML_MAX_BURST];
    void* extras[SML_MAX_BURST];
} sml_packet_burst;
sml_status_t sml_preprocess_burst(const sml_packet_burst* burst, void* stream);
sml_status_t sml_postprocess_burst(const sml_packet_burst* burst, void* stream);

/* The receive loop's two calls on one buffer in ONE launch: for every
 * RECEIVED packet q of the burst, PostprocessSingle(q) and then — when packet
 * q + b exists (q + b < B + b for FLOAT32, q + b < B for INT32; b =
 * batch_num_ltus, the packet window, for both types here) —
 * PreprocessSingle(q + b) into the same entries[i] / extras[i]: DpdkWorkerThread's
 * receive loop, PostprocessSingle then ReusePacket (dpdk_worker_thread.cc:
 * 300-345, dpdk_worker_thread_utils.inc:134,177), and DummyWorkerThread's
 * loop trip (dummy_worker_thread.cc:106-163).  Bit-identical to
 * sml_postprocess_burst followed by sml_preprocess_burst of the ids q + b.
 * With SML_FLAG_PROCESS_PACKET the dummy backend's ProcessPacket (all P words
 * x num_workers, wrapping, exponent unchanged; dummy_backend.cc:72-84) is
 * applied to each packet first, and all P words are written back (the words
 * the preprocess does not rewrite keep the processed values). */
#define SML_FLAG_PROCESS_PACKET 0x8u
sml_status_t sml_exchange_burst(const sml_packet_burst* burst, void* stream);

/* The three burst entry points for a slice of any type: the same struct, with
 * `in` / `out` pointing at elements of data_type (a C caller casts its
 * 16-bit pointers to const float* / float*; the struct keeps its layout).
 *   SML_FLOAT32 / SML_INT32: the untyped entry point, exactly — forwarded
 *     before any check of the typed function's own, so status and bits are
 *     those of the twin for every argument list.
 *   SML_FLOAT16 / SML_BFLOAT16: the kernels convert, by the rule of the other
 *     sml_*_typed entry points: x32 = (float)x (exact) right after a block of
 *     the slice is loaded, every packet rule above on x32 as for a FLOAT32
 *     slice (exponent of block q into byte 0 of the extra slot, block q - b
 *     under the received exponent, only the real words of a partial block,
 *     recv_exps, SML_FLAG_PROCESS_PACKET, SML_FLAG_ROUND_RNE), the
 *     dequantized fp32 value narrowed to the type with round to nearest even
 *     right before the store.  B = ceil(numel / P) and B + b packets, as for
 *     FLOAT32; packet buffers, extra slots and recv_exps are byte for byte
 *     those of a FLOAT32 slice holding the widened values.  `in` and `out`
 *     need 2-byte alignment only; no byte outside [in, in + 2 numel) is read,
 *     none outside [out, out + 2 numel) written; in == out is allowed.  The
 *     argument rules are the FLOAT32 ones: for one argument list every status
 *     equals that of data_type = SML_FLOAT32.
 *   Any other data_type: SML_ERR_UNSUPPORTED.
 * The burst server (below) is not typed: a 16-bit burst takes launches. */
sml_status_t sml_preprocess_burst_typed(const sml_packet_burst* burst, void* stream);
sml_status_t sml_postprocess_burst_typed(const sml_packet_burst* burst, void* stream);
sml_status_t sml_exchange_burst_typed(const sml_packet_burst* burst, void* stream);

/* A persistent burst server, for packet buffers in HOST memory (a NIC's
 * mbuf pool in pinned memory): there a burst launch costs a launch, PCIe
 * round trips and a host synchronisation, ≈ 20 µs per burst (DESIGN.md §9
 * F1).  The server is one resident workgroup that polls a doorbell in
 * coherent, device-mapped host memory.  sml_burst_server_submit() writes the
 * burst, rings the doorbell and returns once the burst is complete (it spins
 * on the completion word the server publishes with a system-scope release):
 * the same bytes as sml_preprocess_burst (op SML_BURST_PRE),
 * sml_postprocess_burst (SML_BURST_POST) or sml_exchange_burst
 * (SML_BURST_EXCHANGE, SML_FLAG_PROCESS_PACKET honoured), a wave per packet.
 * The server starts with the first submit, leaves its loop after `idle_ms`
 * (0 = 100) without a burst, or on sml_burst_server_stop(), and is restarted
 * by the next submit; destroy stops it and frees it.  While it runs it
 * occupies one CU and a device-wide synchronisation waits for it, so a
 * caller stops it between job slices.
 * packet_numel and SML_FLAG_ROUND_RNE are fixed per server (a burst with
 * other values is refused); one server per calling thread; the current
 * device is the server's.  FLOAT32 and INT32 slices only: a burst whose
 * data_type is SML_FLOAT16 / SML_BFLOAT16 returns SML_ERR_UNSUPPORTED (such a
 * slice goes through the sml_*_burst_typed launches). */
typedef struct sml_burst_server sml_burst_server;
#define SML_BURST_PRE 0u
#define SML_BURST_POST 1u
#define SML_BURST_EXCHANGE 2u
sml_status_t sml_burst_server_create(uint32_t packet_numel, uint32_t flags, uint32_t idle_ms,
                                     sml_burst_server** server_out);
sml_status_t sml_burst_server_submit(sml_burst_server* server, uint32_t op, const sml_packet_burst* burst);
/* Leave the loop now and wait for it (the next submit restarts the server);
 * the server's memory and stream are kept for that. */
sml_status_t sml_burst_server_stop(sml_burst_server* server);
sml_status_t sml_burst_server_destroy(sml_burst_server* server);
/* Start the server now (it idles on the doorbell) instead of on the first
 * submit: takes the launch off the first burst's latency.  A relaunch marks
 * every doorbell rung before it as handled, so a burst that failed (a
 * timeout, a workgroup's idle exit mid-burst) is never replayed. */
sml_status_t sml_burst_server_start(sml_burst_server* server);
/* Fault injection for tests: stop the server, then write `burst` and ring the
 * doorbell for it with no server to answer — the state a failed submit
 * leaves (done < doorbell).  Never used on the data path. */
sml_status_t sml_burst_server_inject_unanswered(sml_burst_server* server, uint32_t op,
                                                const sml_packet_burst* burst);

/* Plane sharing for the peer-to-peer switch: export the allocation holding
 * d_ptr as an IPC handle of sml_ipc_handle_bytes() bytes plus d_ptr's byte
 * offset inside it; open a peer's handle in this process (returns the
 * allocation base: add the offset; the mapping reaches the peer GPU's HBM
 * over xGMI, peer access enabled on first use); close it again. */
uint32_t sml_ipc_handle_bytes(void);
sml_status_t sml_ipc_get_handle(const void* d_ptr, void* handle_out, uint64_t* offset_out);
sml_status_t sml_ipc_open_handle(const void* handle, void** d_ptr_out);
sml_status_t sml_ipc_close_handle(void* d_ptr);

/* ---- DPDK/UDP wire frames --------------------------------
 * The DPDK backend builds one Ethernet frame per packet
 * (client_lib/src/backends/dpdk/dpdk_worker_thread_utils.inc:67-135,
 * BuildPacket): Eth(14) + IPv4(20) + UDP(8) + SwitchML header(8:
 * job_type_size, short_job_id, pkt_id (host order), switch_pool_index (BE))
 * + 2-byte extra info (byte 0 = exponent) + packet_numel BE int32 words at
 * offset 52.  Frame p of a job slice (p in [0, B + b), b = min(batch_max, B))
 * carries exps[p] (p < B) and payload block p - b (p >= b), its pool index
 * PktId2PoolIndex(p, start, shift, max_outstanding) (:42-52).
 * Addresses are given in network byte order, as DpdkBackend::E2eAddress. */
typedef struct sml_frame_params {
    uint8_t dst_mac[6];               /* the switch's MAC */
    uint8_t src_mac[6];               /* the worker thread's MAC */
    uint32_t src_ip_be, dst_ip_be;    /* worker, switch (network order) */
    uint16_t src_port_be, dst_port_be;
    uint64_t job_id;                  /* low 8 bits -> short_job_id */
    uint32_t pool_index_start;        /* switch_pool_index_start of the worker thread */
    uint32_t pool_index_shift;        /* switch_pool_index_shift carried across jobs */
    uint32_t max_outstanding_pkts;    /* per worker thread */
} sml_frame_params;

/* Bytes of one frame: 52 + 4 * packet_numel. */
uint64_t sml_frame_bytes(uint32_t packet_numel);

/* Words of the per-slice rx state (d_state) a receive call needs: FLOAT32
 * (sml_dequantize_frames; FLOAT16 / BFLOAT16 through
 * sml_dequantize_frames_typed alike) max(1, B + b) with b = min(batch_max, B); INT32
 * (sml_unpack_frames_int32, int32 != 0) 2B + 6.  B = ceil(numel / P). */
uint64_t sml_rx_state_words(uint64_t numel, uint32_t packet_numel, uint32_t batch_max, int int32);

/* Fused K1 -> frames: quantize + pack one job slice straight into B + b
 * frames at `frame_stride` bytes apart (>= sml_frame_bytes, multiple of 4).
 * `frames` may be device memory or pinned, device-mapped host memory (the
 * NIC's buffers: the kernel then writes them over PCIe).  d_global_exps as
 * for sml_quantize_pack.  Bytes the reference leaves stale (extra-info byte
 * 1, the exponent of frames p >= B, the payload of frames p < b, IPv4
 * identification/TOS/fragment) are written as 0; IPv4 and UDP checksums are
 * left for NIC offload exactly as BuildPacket does (IP 0, UDP = pseudo-header
 * sum, rte_ipv4_phdr_cksum). */
sml_status_t sml_quantize_pack_frames(const float* d_in, uint64_t numel, uint32_t packet_numel,
                                      uint16_t num_workers, const int8_t* d_global_exps,
                                      uint32_t batch_max, const sml_frame_params* params,
                                      void* frames, uint64_t frame_stride, void* stream);

/* Receive side of the DPDK backend (dpdk_worker_thread.cc:300-345): frames
 * the switch returned for one job slice, `num_frames` of them at
 * `frame_stride` bytes apart, in any order (rx bursts gathered into a ring;
 * device or pinned, device-mapped host memory).  A frame is accepted as the
 * worker's receive loop accepts it: short_job_id (byte 43) equal to
 * (uint8_t)job_id and a pkt_id (bytes 44-47, host order) not received
 * before — in an earlier call for the slice, or earlier in `frames` (the
 * first copy wins, :316-330); a pkt_id >= B + b is discarded too.  Every
 * accepted frame is PostprocessSingle'd (ppp.cc:197-260): frame pkt_id < B
 * gives the global exponent of block pkt_id (byte 50, also stored to
 * d_exps[pkt_id]); frame pkt_id >= b gives the aggregated payload of block
 * k = pkt_id - b (BE words at byte 52), dequantized with exponent k into
 * d_out[k*P .. k*P + min(P, numel - k*P)).  As in the reference, the frame
 * carrying exponent k must come in this call or an earlier one for the slice
 * (the switch returns it first).
 *   d_exps:   int8[B], out (the slice's received global exponents)
 *   d_state:  uint64[B + b], 8-B aligned, the rx bitmap (+ received
 *             exponents): zero-filled by the caller before the slice's first
 *             call (rte_bitmap_reset), persists across its calls
 *   d_counts: uint64[2] {accepted, discarded}, added to; nullable, 8-B aligned
 * Two launches on `stream`: claim (thread per frame), then dequantize +
 * retire the winners (wave per 1024 output elements). */
sml_status_t sml_dequantize_frames(const void* frames, uint64_t num_frames, uint64_t frame_stride,
                                   uint64_t numel, uint32_t packet_numel, uint16_t num_workers,
                                   uint32_t batch_max, uint64_t job_id, int8_t* d_exps,
                                   uint64_t* d_state, float* d_out, uint64_t* d_counts,
                                   void* stream);

/* FLOAT16 / BFLOAT16 job slices over the same frames: the argument lists of
 * sml_quantize_pack_frames and sml_dequantize_frames with void* for the typed
 * buffer and its sml_data_type_t next to it, by the convention of the other
 * sml_*_typed entry points (above).
 *   SML_FLOAT16 / SML_BFLOAT16: the kernels convert.  tx: x32[i] = (float)x[i]
 *     (exact) right after the load, and the frame set is byte for byte the
 *     one sml_quantize_pack_frames builds from x32 — headers (job_type_size
 *     and short_job_id included), pkt_ids, pool indices, exponent bytes, the
 *     zero payload of the extra batch, BE int32 words, zero tail words of a
 *     partial last block.  The wire format knows no element size:
 *     B = ceil(numel / P) and b = min(batch_max, B) as for FLOAT32.  rx: the
 *     claim, the state words, the first-copy-wins rule, d_exps and d_counts
 *     are sml_dequantize_frames'; an accepted payload is dequantized to an
 *     fp32 y32 as there and stored as (T)y32, round to nearest even (overflow
 *     -> +-inf, fp16 results below the normal range -> fp16 denormals, NaN ->
 *     a NaN of T); a block without a winner in the call keeps its bytes.
 *   SML_FLOAT32: exactly sml_quantize_pack_frames / sml_dequantize_frames
 *     (same kernels, same bytes).
 *   SML_INT32 (or any other value): SML_ERR_UNSUPPORTED.
 * A 16-bit buffer needs 2-byte alignment only (a slice starts at any element)
 * and no byte outside [ptr, ptr + 2 * numel) is read (tx) or written (rx).
 * One that is not 2-byte aligned gets what the FLOAT32 entry point gives a
 * buffer that is not 4-byte aligned: SML_ERR_INVALID_ARG (tx),
 * SML_ERR_ALIGNMENT (rx).  Every check happens before anything is launched.
 * sml_rx_state_words (int32 = 0) and sml_rx_reset serve a 16-bit slice as
 * they are: the state is per pkt_id and knows no element type. */
sml_status_t sml_quantize_pack_frames_typed(const void* d_in, sml_data_type_t data_type, uint64_t numel,
                                            uint32_t packet_numel, uint16_t num_workers,
                                            const int8_t* d_global_exps, uint32_t batch_max,
                                            const sml_frame_params* params, void* frames,
                                            uint64_t frame_stride, void* stream);
sml_status_t sml_dequantize_frames_typed(const void* frames, uint64_t num_frames, uint64_t frame_stride,
                                         uint64_t numel, uint32_t packet_numel, uint16_t num_workers,
                                         uint32_t batch_max, uint64_t job_id, int8_t* d_exps,
                                         uint64_t* d_state, void* d_out, sml_data_type_t data_type,
                                         uint64_t* d_counts, void* stream);

/* INT32 job slices (DataType::INT32, common.h:51-55) over the same frames.
 * The INT32 pre/post-processor only reorders bytes and needs no extra batch
 * (NeedsExtraBatch is false, ppp.cc:65-67), so a slice has B frames and frame
 * p carries block p: BuildPacket's headers (as sml_quantize_pack_frames,
 * extra-info bytes 0) and htonl of the block's words (ppp.cc:158-190; words
 * past numel in the last frame are 0). */
sml_status_t sml_pack_frames_int32(const int32_t* d_in, uint64_t numel, uint32_t packet_numel,
                                   const sml_frame_params* params, void* frames, uint64_t frame_stride,
                                   void* stream);

/* The receive loop for an INT32 job slice: acceptance as for
 * sml_dequantize_frames (this job, a pkt_id < B not received before, the
 * first copy wins), and PostprocessSingle's INT32 branch (ppp.cc:262-298):
 * ntohl of the accepted frame's words into d_out[pkt_id*P ..
 * pkt_id*P + min(P, numel - pkt_id*P)).  d_state: uint64[2B + 6] (the rx
 * bitmap, the slice's call sequence, the slice's count of copies that
 * claimed ahead of an earlier copy, the conflict count and dirty-list length
 * of the call in progress (0 between calls), the fix-up workgroups finished
 * so far (128 per call), the list length the last call's fix-up found, then
 * up to B listed pkt_ids),
 * zeroed per slice (sml_rx_reset), persists across calls; d_counts as for
 * sml_dequantize_frames.  One pass in stream order over the frames (an INT32
 * frame needs no other frame) plus a fix-up over a grid of workgroups that
 * rewrites the listed pkt_ids only (all B state words if the list
 * overflowed), on `stream`;
 * num_frames < 2^31 per call, fewer than 2^32 - 1 calls per slice. */
sml_status_t sml_unpack_frames_int32(const void* frames, uint64_t num_frames, uint64_t frame_stride,
                                     uint64_t numel, uint32_t packet_numel, uint64_t job_id,
                                     uint64_t* d_state, int32_t* d_out, uint64_t* d_counts, void* stream);

/* rte_bitmap_reset for one slice (dpdk_worker_thread.cc, per job slice):
 * zero d_state (uint64[B + b]; for INT32 slices uint64[2B + 6]) before the
 * slice's first sml_dequantize_frames / sml_unpack_frames_int32
 * call.  One async memset on `stream`. */
sml_status_t sml_rx_reset(uint64_t* d_state, uint64_t num_words, void* stream);

/* ---- The switch's side of the DPDK frames (SURVEY §8 A11 over F3) --------
 * What the Tofino pipeline does to the frames W workers send it, a batch of
 * arrived frames per call, with the switch's registers in d_state across
 * calls: the slot pool with its two sets, the worker bitmap and the worker
 * count (p4/bitmap_checker.p4, p4/workers_counter.p4), the wrapping bit<32>
 * sum and the signed int8 exponent max (p4/processor.p4:48-54,
 * p4/exponents.p4:48-54), the "last packet broadcasts, a retransmission to a
 * full slot is answered, anything else is consumed" rule
 * (p4/next_step_selector.p4, controller/next_step_selector.py) and the result
 * frame (p4/udp_sender.p4).
 *   A frame is one of sml_quantize_pack_frames' / sml_pack_frames_int32's.  Its
 * worker w is the index of workers[] whose ip_be equals bytes 26-29, its slot
 * s the 14 low bits of the big-endian pool index at bytes 48-49, its set v
 * that index's bit 15.  An unknown source address or s >= num_slots: IGNORED,
 * nothing changes.  Otherwise, frame by frame in index order:
 *   before = bitmap[s][v]; bitmap[s][v] |= 1 << w; bitmap[s][1-v] &= ~(1 << w);
 *   not a retransmission (before has no bit w): flag = count[s][v], then
 *     count = count == 0 ? W - 1 : count - 1 (W == 1: flag = 1); the slot's P
 *     words and two exponent bytes are WRITTEN when before == 0, else the words
 *     are added mod 2^32 (host order; the result carries htonl) and the
 *     exponents take the signed int8 max, byte 50 and byte 51 each on its own;
 *     flag == 1 -> BROADCAST, else CONSUMED;
 *   a retransmission: flag = count[s][v], unchanged (W == 1: flag = 0);
 *     flag == 0, a full slot -> RETRANSMIT, else CONSUMED.
 * BROADCAST / RETRANSMIT: the result frame is written at out_frames +
 * i * out_stride for input frame i (every other output position keeps its
 * bytes).  Eth dst = workers[w].mac, src = switch_mac, IPv4 (0x45 0x00, total
 * length, id / flags / fragment 0, TTL 64, UDP, a real header checksum, src =
 * the switch, dst = the worker), UDP (src port = the frame's dst port, dst
 * port = its src port, length, checksum 0), byte 42 = 0x10 | (byte 42 & 7),
 * bytes 43-47 echoed, bytes 48-49 the received pool index with bit 14 cleared,
 * bytes 50-51 the slot's exponents, from byte 52 the slot's P words.  A
 * BROADCAST is written once, addressed to the worker whose frame completed
 * the slot: the other W - 1 copies differ in the destination fields and the
 * checksum only and are the caller's to make.
 *   One call is that pipeline over the call's frames in index order, with one
 * rule that makes it parallel: for each (slot, worker) the call handles the
 * frames of the set that pair's lowest-index frame carries; the pair's frames
 * of the other set get DEFERRED and change nothing — the caller resubmits
 * them in a later call, a reordering the network could have produced.  Equal
 * to the sequential pipeline for streams that follow the worker protocol (a
 * worker sends packet p + max_outstanding into a slot only after it received
 * the result of packet p from it; loss, duplication and reordering within
 * that window).  For any other stream the verdicts, the bitmaps and the counts
 * are still the pipeline's, and a result frame carries the slot's words as
 * they stand at the END of the call (an answer to a retransmission that
 * precedes a new contribution to its slot and set in the same call differs).
 *   frames / out_frames: device memory or pinned, device-mapped host memory,
 *     4-byte aligned, strides >= sml_frame_bytes(P) and a multiple of 4;
 *   d_state: sml_frame_switch_state_bytes() bytes of device memory, 8-byte
 *     aligned, opaque, cleared by sml_frame_switch_reset before the first call;
 *   d_verdict: uint8[num_frames], out;  d_counts: uint64[5] indexed by
 *     verdict, added to; nullable, 8-byte aligned.
 * Status, every check before any launch: params NULL, num_workers == 0, or
 * (num_frames > 0) a NULL frames / d_state / out_frames / d_verdict ->
 * SML_ERR_INVALID_ARG; packet_numel not a packet size, num_workers >
 * SML_MAX_FRAME_SWITCH_WORKERS, num_slots not in 1..16384 ->
 * SML_ERR_UNSUPPORTED; num_frames == 0 -> SML_OK, nothing launched; a buffer
 * or stride off its alignment -> SML_ERR_ALIGNMENT.
 * Four launches on `stream`: claim (thread per frame), verdicts (thread per
 * frame), apply (wave per touched slot), results (wave per input frame; it
 * writes only for a BROADCAST / RETRANSMIT verdict). */
#define SML_MAX_FRAME_SWITCH_WORKERS 32          /* worker_bitmap_t is 32 bits */
#define SML_MAX_FRAME_SWITCH_SLOTS 16384         /* pool indices 0..16383, two sets each */
#define SML_VERDICT_CONSUMED   0
#define SML_VERDICT_BROADCAST  1
#define SML_VERDICT_RETRANSMIT 2
#define SML_VERDICT_IGNORED    3
#define SML_VERDICT_DEFERRED   4
typedef struct sml_switch_worker { uint8_t mac[6]; uint32_t ip_be; } sml_switch_worker;
typedef struct sml_frame_switch_params {
    uint8_t  switch_mac[6];  uint32_t switch_ip_be;
    uint16_t num_workers;                    /* 1..32 */
    uint32_t num_slots;                      /* 1..16384: pool indices 0..num_slots-1, two sets each */
    uint32_t packet_numel;                   /* 64,128,256,512,1024 */
    sml_switch_worker workers[SML_MAX_FRAME_SWITCH_WORKERS];
} sml_frame_switch_params;

/* Bytes of d_state for a pool of num_slots slots of packet_numel words; 0 on
 * an unsupported packet_numel or num_slots. */
uint64_t sml_frame_switch_state_bytes(uint32_t num_slots, uint32_t packet_numel);
/* Clear the switch's registers (bitmaps, counts, the per-call scratch): async
 * memsets on `stream`.  Status: d_state NULL -> SML_ERR_INVALID_ARG; bad
 * num_slots / packet_numel -> SML_ERR_UNSUPPORTED; d_state not 8-byte aligned
 * -> SML_ERR_ALIGNMENT. */
sml_status_t sml_frame_switch_reset(void* d_state, uint32_t num_slots, uint32_t packet_numel, void* stream);
sml_status_t sml_frame_switch(const sml_frame_switch_params* params,
                              const void* frames, uint64_t num_frames, uint64_t frame_stride,
                              void* d_state, void* out_frames, uint64_t out_stride,
                              uint8_t* d_verdict, uint64_t* d_counts, void* stream);

/* The egress of one sml_frame_switch call (above): the multicast group of
 * p4/next_step_selector.p4 and p4/udp_sender.p4's per-port destination, into
 * one receive ring per worker.  out_frames / num_frames / out_stride /
 * d_verdict are what that call left; worker u's ring starts at rings +
 * u * ring_bytes and holds up to ring_frames frames rx_stride bytes apart — a
 * dense run, as sml_dequantize_frames / sml_unpack_frames_int32 take it.
 *   The input frames i in ascending order:
 *   BROADCAST: a copy for every worker u in 0..num_workers-1, out_frames[i]
 *     with bytes 0-5 = workers[u].mac, bytes 30-33 = workers[u].ip_be and bytes
 *     24-25 = the IPv4 header checksum of sml_frame_switch's result header to
 *     worker u; every other byte, ports included, unchanged (the copy for the
 *     worker the switch addressed the frame to is out_frames[i] byte for byte);
 *   RETRANSMIT: one copy, unchanged, for the first worker whose ip_be equals
 *     bytes 30-33; no such worker: nothing, counted `unroutable`;
 *   any other verdict: nothing, out_frames[i] is not read.
 *   A copy whose bit in d_drop[i] is set (bit u = the copy for worker u) is not
 *   written and is counted `dropped`.  A surviving copy is appended to worker
 *   u's ring at position d_ring_count[u] + (the surviving copies for u from
 *   frames below i in this call): each ring holds its worker's frames in
 *   ascending input order behind what earlier calls left (per-port FIFO; the
 *   order is part of the contract).  Positions >= ring_frames are not written
 *   and are counted `overflow`; d_ring_count[u] ends at min(old + survivors,
 *   ring_frames).  No other byte of a ring is touched.
 *   rings: device memory or pinned, device-mapped host memory, 4-byte aligned;
 *     rx_stride >= sml_frame_bytes(P), ring_bytes >= ring_frames * rx_stride,
 *     both multiples of 4;
 *   d_drop: uint32[num_frames] or NULL (nothing dropped); d_ring_count:
 *     uint64[num_workers], in / out; d_counts: uint64[4] {delivered, dropped,
 *     overflow, unroutable}, added to, nullable; device memory, 8-byte aligned
 *     (d_drop 4);
 *   d_scratch: sml_frame_switch_deliver_scratch_bytes(num_frames, num_workers)
 *     bytes of device memory, 16-byte aligned, contents free between calls (the
 *     per-frame copy sets and the per-worker prefix counts of the call).
 * Status, every check before any launch: params NULL, num_workers == 0, or
 * (num_frames > 0) a NULL out_frames / d_verdict / rings / d_ring_count /
 * d_scratch -> SML_ERR_INVALID_ARG; packet_numel not a packet size,
 * num_workers > SML_MAX_FRAME_SWITCH_WORKERS, ring_frames == 0, num_frames >=
 * 2^31 -> SML_ERR_UNSUPPORTED; num_frames == 0 -> SML_OK, nothing launched; a
 * buffer or stride off its alignment, or ring_bytes < ring_frames * rx_stride
 * -> SML_ERR_ALIGNMENT.
 * Three launches on `stream`: counts (thread per frame, a wave ballot per
 * worker), the scan of the counts (workgroup per worker), the copy (wave per
 * input frame; it reads a frame once and writes its copies). */
uint64_t sml_frame_switch_deliver_scratch_bytes(uint64_t num_frames, uint32_t num_workers);
sml_status_t sml_frame_switch_deliver(const sml_frame_switch_params* params,
                                      const void* out_frames, uint64_t num_frames, uint64_t out_stride,
                                      const uint8_t* d_verdict, const uint32_t* d_drop,
                                      void* rings, uint64_t ring_bytes, uint64_t ring_frames, uint64_t rx_stride,
                                      uint64_t* d_ring_count, uint64_t* d_counts, void* d_scratch, void* stream);

/* The ingress of a sml_frame_switch call: its input from the workers' tx
 * frame sets.  sets: a host array of num_sets <= 32 base pointers (device or
 * pinned, device-mapped memory, 4-byte aligned), each set_frames frames
 * set_stride bytes apart.  Output frame j (dst + j * dst_stride) is the
 * sml_frame_bytes(P) bytes of frame d_index[j] of set d_set[j]; an entry with
 * d_set[j] >= num_sets or d_index[j] >= set_frames writes nothing and adds 1
 * to *d_skipped (device uint64, nullable).  d_set: uint32[n], d_index:
 * uint64[n], device memory.  One launch on `stream`, a wave per frame.
 * Status: sets NULL, num_sets == 0, or (n > 0) a NULL d_set / d_index / dst /
 * entry of sets -> SML_ERR_INVALID_ARG; packet_numel not a packet size or
 * num_sets > 32 -> SML_ERR_UNSUPPORTED; n == 0 -> SML_OK, nothing launched; a
 * buffer or stride off its alignment (strides >= sml_frame_bytes(P), multiples
 * of 4; d_index and d_skipped 8-byte aligned) -> SML_ERR_ALIGNMENT. */
sml_status_t sml_frame_gather(const void* const* sets, uint32_t num_sets, uint64_t set_frames, uint64_t set_stride,
                              const uint32_t* d_set, const uint64_t* d_index, uint64_t n, uint32_t packet_numel,
                              void* dst, uint64_t dst_stride, uint64_t* d_skipped, void* stream);

/* ncclUint8 buckets of the CollNet plugin (switchml_plugin.cc:318-337,
 * 370-378: "SwitchML does not really support uint8"): each byte widened to an
 * int32 for the INT32 all-reduce, and the summed words narrowed back (mod
 * 256).  Device or device-mapped memory; one launch each on `stream`.
 * Widening zero-extends (a byte is 0..255); narrowing keeps the low byte.
 * The uint8 side may start at any byte; the int32 side is 4-byte aligned.
 * Status (both): n == 0 -> SML_OK whatever the pointers; else a NULL pointer,
 * or an int32 side (sml_widen_u8_i32's d_out, sml_narrow_i32_u8's d_in) not
 * 4-byte aligned -> SML_ERR_INVALID_ARG. */
sml_status_t sml_widen_u8_i32(const uint8_t* d_in, int32_t* d_out, uint64_t n, void* stream);
sml_status_t sml_narrow_i32_u8(const int32_t* d_in, uint8_t* d_out, uint64_t n, void* stream);

/* ---- RDMA messages --------------------------------------
 * The RDMA backend's LTU is a message of msg_numel (1024) elements
 * (rdma_worker_thread.cc:86-88): its payload is block m of the planes built
 * with packet_numel = msg_numel.  The exponent travels in the 32-bit
 * immediate: imm = (msg_id & 0xFFFF) | (exponent byte << 16), byte 3 = 0
 * (rdma_worker_thread.cc:341-356; PreprocessSingle writes byte 2).  Message
 * m in [0, B + b) carries exps[m] for m < B; the byte is 0 for m >= B.
 * d_imm: uint32[B + b] (host byte order, as ibv_send_wr.imm_data is filled).
 * d_exps must not be null (SML_ERR_INVALID_ARG): an INT32 slice has its own
 * entry point below. */
sml_status_t sml_rdma_imm(const int8_t* d_exps, uint64_t num_blocks, uint32_t batch_max,
                          uint32_t* d_imm, void* stream);

/* An INT32 slice's immediates: B messages (no extra batch, ppp.cc:65-67),
 * imm = msg_id & 0xFFFF (the INT32 PreprocessSingle leaves byte 2 alone).
 * d_imm: uint32[B]. */
sml_status_t sml_rdma_imm_int32(uint64_t num_blocks, uint32_t* d_imm, void* stream);

/* Measurement probe (not part of the PPP): copy `bytes` (a multiple of 4 KiB,
 * 16-B aligned buffers) with the quantize kernel's tile shape (K1's slices
 * per wave tile) and access policy (non-temporal loads; non-temporal stores from the payload
 * non-temporal threshold on, default-policy stores below it — the store
 * policy sml_quantize_pack uses for an output plane of `bytes`) — the
 * practical HBM ceiling bench.py reports. */
sml_status_t sml_stream_copy(const void* d_in, void* d_out, uint64_t bytes, void* stream);

/* Fault injection for tests (not part of the PPP): one small kernel that
 * keeps `stream` busy for `microseconds` of the device's wall clock (at most
 * 60 s; SML_ERR_INVALID_ARG above) and then ends on its own — a device that
 * does not finish within a caller's timeout (backend.dummy.stall_worker_thread
 * uses it to exercise the in-node switch's bounded waits), never a hang. */
sml_status_t sml_debug_stall(uint32_t microseconds, void* stream);

/* Launch-geometry knob for experiments: workgroups per launch for the
 * streaming kernels (0 = one 256-thread workgroup per 4 tiles of 1024
 * elements, i.e. no grid-stride).  Process-wide; returns the previous value. */
uint32_t sml_set_grid_limit(uint32_t max_workgroups);

/* Launch-order knob: the streaming kernels permute workgroups so that each
 * of the 8 XCDs sweeps runs of `chunk` consecutive workgroups' data (default
 * 64; 0 = plain blockIdx order).  Process-wide; returns the previous value. */
uint32_t sml_set_xcd_chunk(uint32_t chunk);

/* Tuning knob: slices of 256 elements per wave tile in sml_exponents /
 * sml_quantize_pack (K1/K2/K3): 4, 2 or 1 for every kernel — never below
 * P / 256 — or 0 (the default; any other value restores it): 2, measured
 * fastest for all three on the final kernels.
 * Results are identical for every size.  Returns the
 * previous value. */
uint32_t sml_set_quantize_tile_slices(uint32_t slices);

/* Tuning knob: slices of 256 elements per wave tile in sml_dequantize (K4)
 * and sml_roundtrip_loopback (the fused round trip; P = 1024 keeps 4): 4 or
 * 2 for both, or 0 = the default, 2 for both (as measured).
 * Results are identical for every size.  Returns
 * the previous value. */
uint32_t sml_set_stream_tile_slices(uint32_t slices);

/* Tuning knob: output planes of at least `bytes` bytes are written with
 * non-temporal stores — the payload plane of sml_quantize_pack (K1/K3), the
 * fp32 output of sml_dequantize (K4), sml_roundtrip_loopback and
 * sml_roundtrip_loopback_batch (by the batch's total output), the typed
 * output of their sml_*_typed counterparts (by its bytes;
 * sml_roundtrip_loopback_batch_typed by the call's total output over every
 * slice and type), the fp32 output of sml_dequantize_frames (the typed output
 * of sml_dequantize_frames_typed by its bytes, 2 * numel for a 16-bit type),
 * the payloads of a device-memory frame set of sml_quantize_pack_frames and
 * sml_quantize_pack_frames_typed (host frame sets keep default stores) and the
 * sml_stream_copy probe; default 64 MiB, a quarter of the 256 MiB Infinity
 * Cache — DESIGN.md §4); UINT64_MAX = never, 0 = always.
 * Results are identical either way.  Returns the previous value. */
uint64_t sml_set_payload_nt_threshold(uint64_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* SWITCHML_HIP_H_ */
