"""switchml_amd — Python front end of the MI355X-native SwitchML end-host
pre/post-processor (libswitchml_hip.so, C-ABI in include/switchml_hip.h).

Thin ctypes layer over the C-ABI for tests, bench and the torch.distributed
switch simulation.  Tensors are torch CUDA (HIP) tensors; every call is
enqueued on torch's current stream unless a stream is given.  There is no CPU
fallback: if the HIP library is missing or the tensor is not on the GPU, the
call raises.

This file only re-exports: abi.py owns the C ABI, glue.py the torch side, and
planes, switch, packets, frames, frame_switch and knobs one subsystem's
wrappers each.  Importing it imports neither torch nor numpy and loads no library.
"""
from .abi import (BFLOAT16, BURST_EXCHANGE, BURST_POST, BURST_PRE, FLAG_PAYLOAD_LE, FLAG_PEER_PLANES,
                  FLAG_PROCESS_PACKET, FLAG_ROUND_RNE, FLOAT16, FLOAT32, HEADER_PATH, INT32, LIB_PATH,
                  MAX_BATCH_SLICES, MAX_BURST, MAX_FRAME_SWITCH_SLOTS, MAX_FRAME_SWITCH_WORKERS, MAX_SWITCH_WORKERS,
                  PACKET_NUMELS, SML_ERR_ALIGNMENT, SML_ERR_HIP, SML_ERR_INVALID_ARG, SML_ERR_UNSUPPORTED, SML_OK,
                  VERDICT_BROADCAST, VERDICT_CONSUMED, VERDICT_DEFERRED, VERDICT_IGNORED, VERDICT_RETRANSMIT,
                  FrameParams, FrameSwitchParams, PacketBurst, Slice, SwitchMLError, SwitchWorker, TypedSlice,
                  header_symbols, lib)
from .frame_switch import FrameSwitch, frame_switch_params, gather_frames
from .frames import (RxSlice, RxSliceInt32, dequantize_frames, frame_bytes, frame_params, pack_frames_int32,
                     quantize_pack_frames, rdma_imm, unpack_frames_int32)
from .knobs import (debug_stall, set_grid_limit, set_payload_nt_threshold, set_quantize_tile_slices,
                    set_stream_tile_slices, set_xcd_chunk, stream_copy)
from .packets import BurstServer, exchange_burst, packet_burst, postprocess_burst, preprocess_burst
from .planes import (bswap_i32, dequantize, exponents, fifo_slice, loopback_aggregate, num_blocks, quantize_pack,
                     quantize_pack_launcher, roundtrip_loopback, roundtrip_loopback_batch, scale_lut,
                     scale_lut_device, shard_quantize_pack)
from .switch import (copy_segments, copy_segments_typed, copy_words, narrow_i32_u8, release_to_peers,
                     switch_aggregate, switch_exps, widen_u8_i32)
