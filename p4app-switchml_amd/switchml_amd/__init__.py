"""switchml_amd — Python front end of the MI355X-native SwitchML end-host
pre/post-processor (libswitchml_hip.so, C-ABI in include/switchml_hip.h).

Thin ctypes layer over the C-ABI for tests, bench and the torch.distributed
switch simulation.  Tensors are torch CUDA (HIP) tensors; every call is
enqueued on torch's current stream unless a stream is given.  There is no CPU
fallback: if the HIP library is missing or the tensor is not on the GPU, the
call raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libswitchml_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "switchml_hip.h")

SML_OK = 0
SML_ERR_INVALID_ARG = 1
SML_ERR_UNSUPPORTED = 2
SML_ERR_ALIGNMENT = 3
SML_ERR_HIP = 4

FLAG_PAYLOAD_LE = 0x1
FLAG_ROUND_RNE = 0x2
FLAG_PEER_PLANES = 0x4   # inputs written by other GPUs: acquire first (sml_release_to_peers on the writer)
FLAG_PROCESS_PACKET = 0x8   # sml_exchange_burst: the dummy backend's ProcessPacket (x W) on each packet first

PACKET_NUMELS = (64, 128, 256, 512, 1024)

# sml_data_type_t
FLOAT32, INT32, FLOAT16, BFLOAT16 = 0, 1, 2, 3

_lib = None


class FrameParams(ctypes.Structure):
    """sml_frame_params (include/switchml_hip.h): addresses in network byte order."""
    _fields_ = [("dst_mac", ctypes.c_uint8 * 6), ("src_mac", ctypes.c_uint8 * 6),
                ("src_ip_be", ctypes.c_uint32), ("dst_ip_be", ctypes.c_uint32),
                ("src_port_be", ctypes.c_uint16), ("dst_port_be", ctypes.c_uint16),
                ("job_id", ctypes.c_uint64), ("pool_index_start", ctypes.c_uint32),
                ("pool_index_shift", ctypes.c_uint32), ("max_outstanding_pkts", ctypes.c_uint32)]


def frame_params(dst_mac=b"\x02\x00\x00\x00\x00\x01", src_mac=b"\x02\x00\x00\x00\x00\x02",
                 src_ip="10.0.0.1", dst_ip="10.0.0.253", src_port=4000, dst_port=48879, job_id=0,
                 pool_index_start=0, pool_index_shift=0, max_outstanding_pkts=64) -> FrameParams:
    import socket
    from .frame_wire import ip_be
    fp = FrameParams()
    fp.dst_mac[:] = list(dst_mac)
    fp.src_mac[:] = list(src_mac)
    fp.src_ip_be = ip_be(src_ip)
    fp.dst_ip_be = ip_be(dst_ip)
    fp.src_port_be = socket.htons(src_port)
    fp.dst_port_be = socket.htons(dst_port)
    fp.job_id = job_id
    fp.pool_index_start = pool_index_start
    fp.pool_index_shift = pool_index_shift
    fp.max_outstanding_pkts = max_outstanding_pkts
    return fp


MAX_FRAME_SWITCH_WORKERS = 32
MAX_FRAME_SWITCH_SLOTS = 16384
# sml_frame_switch's verdict per input frame
VERDICT_CONSUMED, VERDICT_BROADCAST, VERDICT_RETRANSMIT, VERDICT_IGNORED, VERDICT_DEFERRED = range(5)


class SwitchWorker(ctypes.Structure):
    """sml_switch_worker: a worker's MAC and its IPv4 address in network byte order."""
    _fields_ = [("mac", ctypes.c_uint8 * 6), ("ip_be", ctypes.c_uint32)]


class FrameSwitchParams(ctypes.Structure):
    """sml_frame_switch_params (include/switchml_hip.h)."""
    _fields_ = [("switch_mac", ctypes.c_uint8 * 6), ("switch_ip_be", ctypes.c_uint32),
                ("num_workers", ctypes.c_uint16), ("num_slots", ctypes.c_uint32),
                ("packet_numel", ctypes.c_uint32), ("workers", SwitchWorker * MAX_FRAME_SWITCH_WORKERS)]


def frame_switch_params(workers, num_slots: int, packet_numel: int = 256, switch_mac=b"\x02\x00\x00\x00\x00\x01",
                        switch_ip="10.0.0.253") -> FrameSwitchParams:
    """`workers`: a (mac bytes, dotted IPv4 string) pair per worker, in worker-id order."""
    from .frame_wire import ip_be
    workers = list(workers)
    if len(workers) > MAX_FRAME_SWITCH_WORKERS:
        raise ValueError(f"at most {MAX_FRAME_SWITCH_WORKERS} workers (worker_bitmap_t is 32 bits)")
    sp = FrameSwitchParams()
    sp.switch_mac[:] = list(switch_mac)
    sp.switch_ip_be = ip_be(switch_ip)
    sp.num_workers = len(workers)
    sp.num_slots = num_slots
    sp.packet_numel = packet_numel
    for i, (mac, ip) in enumerate(workers):
        sp.workers[i].mac[:] = list(mac)
        sp.workers[i].ip_be = ip_be(ip)
    return sp


MAX_BURST = 64


class PacketBurst(ctypes.Structure):
    """sml_packet_burst (include/switchml_hip.h): up to MAX_BURST per-packet
    calls of one job slice in one launch."""
    _fields_ = [("in_", ctypes.c_void_p), ("out", ctypes.c_void_p), ("numel", ctypes.c_uint64),
                ("packet_numel", ctypes.c_uint32), ("num_workers", ctypes.c_uint16), ("data_type", ctypes.c_uint16),
                ("batch_num_ltus", ctypes.c_uint64), ("recv_exps", ctypes.c_void_p), ("count", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("pkt_ids", ctypes.c_uint64 * MAX_BURST),
                ("entries", ctypes.c_void_p * MAX_BURST), ("extras", ctypes.c_void_p * MAX_BURST)]


class SwitchMLError(RuntimeError):
    def __init__(self, fn: str, status: int):
        L = lib()
        msg = L.sml_status_string(status).decode()
        err = L.sml_last_error().decode()
        super().__init__(f"{fn} failed: {msg}" + (f" ({err})" if err else ""))
        self.status = status


def lib():
    """Load libswitchml_hip.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found — build it with `make -C p4app-switchml_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    u64, u32, u16, i32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_int, ctypes.c_void_p
    L.sml_abi_version.restype = i32
    L.sml_abi_version.argtypes = []
    L.sml_status_string.restype = ctypes.c_char_p
    L.sml_status_string.argtypes = [i32]
    L.sml_last_error.restype = ctypes.c_char_p
    L.sml_last_error.argtypes = []
    L.sml_num_blocks.restype = u64
    L.sml_num_blocks.argtypes = [u64, u32]
    L.sml_scale_lut.restype = i32
    L.sml_scale_lut.argtypes = [u16, vp]
    L.sml_scale_lut_device.restype = i32
    L.sml_scale_lut_device.argtypes = [u16, vp, vp]
    L.sml_exponents.restype = i32
    L.sml_exponents.argtypes = [vp, u64, u32, vp, vp]
    L.sml_quantize_pack.restype = i32
    L.sml_quantize_pack.argtypes = [vp, u64, u32, u16, vp, vp, vp, u32, vp]
    L.sml_dequantize.restype = i32
    L.sml_dequantize.argtypes = [vp, vp, u64, u32, u16, vp, u32, vp]
    L.sml_bswap_i32.restype = i32
    L.sml_bswap_i32.argtypes = [vp, vp, u64, vp]
    L.sml_loopback_aggregate.restype = i32
    L.sml_loopback_aggregate.argtypes = [vp, u64, u16, u32, vp]
    L.sml_roundtrip_loopback.restype = i32
    L.sml_roundtrip_loopback.argtypes = [vp, vp, u64, u32, u16, vp, vp, u32, vp]
    L.sml_roundtrip_loopback_batch.restype = i32
    L.sml_roundtrip_loopback_batch.argtypes = [vp, u32, u32, u16, u32, vp]
    L.sml_set_grid_limit.restype = u32
    L.sml_set_grid_limit.argtypes = [u32]
    L.sml_stream_copy.restype = i32
    L.sml_stream_copy.argtypes = [vp, vp, u64, vp]
    L.sml_rdma_imm.restype = i32
    L.sml_rdma_imm.argtypes = [vp, u64, u32, vp, vp]
    L.sml_rdma_imm_int32.restype = i32
    L.sml_rdma_imm_int32.argtypes = [u64, vp, vp]
    L.sml_debug_stall.restype = i32
    L.sml_debug_stall.argtypes = [u32, vp]
    L.sml_frame_bytes.restype = u64
    L.sml_frame_bytes.argtypes = [u32]
    L.sml_rx_state_words.restype = u64
    L.sml_rx_state_words.argtypes = [u64, u32, u32, i32]
    L.sml_quantize_pack_frames.restype = i32
    L.sml_quantize_pack_frames.argtypes = [vp, u64, u32, u16, vp, u32, ctypes.POINTER(FrameParams), vp, u64, vp]
    L.sml_set_quantize_tile_slices.restype = u32
    L.sml_set_quantize_tile_slices.argtypes = [u32]
    L.sml_set_stream_tile_slices.restype = u32
    L.sml_set_stream_tile_slices.argtypes = [u32]
    L.sml_set_payload_nt_threshold.restype = u64
    L.sml_set_payload_nt_threshold.argtypes = [u64]
    L.sml_set_xcd_chunk.restype = u32
    L.sml_set_xcd_chunk.argtypes = [u32]
    L.sml_dequantize_frames.restype = i32
    L.sml_dequantize_frames.argtypes = [vp, u64, u64, u64, u32, u16, u32, u64, vp, vp, vp, vp, vp]
    L.sml_quantize_pack_frames_typed.restype = i32
    L.sml_quantize_pack_frames_typed.argtypes = [vp, i32, u64, u32, u16, vp, u32, ctypes.POINTER(FrameParams), vp, u64,
                                                 vp]
    L.sml_dequantize_frames_typed.restype = i32
    L.sml_dequantize_frames_typed.argtypes = [vp, u64, u64, u64, u32, u16, u32, u64, vp, vp, vp, i32, vp, vp]
    L.sml_rx_reset.restype = i32
    L.sml_rx_reset.argtypes = [vp, u64, vp]
    L.sml_pack_frames_int32.restype = i32
    L.sml_pack_frames_int32.argtypes = [vp, u64, u32, ctypes.POINTER(FrameParams), vp, u64, vp]
    L.sml_unpack_frames_int32.restype = i32
    L.sml_unpack_frames_int32.argtypes = [vp, u64, u64, u64, u32, u64, vp, vp, vp, vp]
    L.sml_frame_switch_state_bytes.restype = u64
    L.sml_frame_switch_state_bytes.argtypes = [u32, u32]
    L.sml_frame_switch_reset.restype = i32
    L.sml_frame_switch_reset.argtypes = [vp, u32, u32, vp]
    L.sml_frame_switch.restype = i32
    L.sml_frame_switch.argtypes = [ctypes.POINTER(FrameSwitchParams), vp, u64, u64, vp, vp, u64, vp, vp, vp]
    L.sml_frame_switch_deliver_scratch_bytes.restype = u64
    L.sml_frame_switch_deliver_scratch_bytes.argtypes = [u64, u32]
    L.sml_frame_switch_deliver.restype = i32
    L.sml_frame_switch_deliver.argtypes = [ctypes.POINTER(FrameSwitchParams), vp, u64, u64, vp, vp, vp, u64, u64, u64,
                                           vp, vp, vp, vp]
    L.sml_frame_gather.restype = i32
    L.sml_frame_gather.argtypes = [ctypes.POINTER(vp), u32, u64, u64, vp, vp, u64, u32, vp, u64, vp, vp]
    L.sml_switch_aggregate.restype = i32
    L.sml_switch_aggregate.argtypes = [vp, vp, u16, u64, u32, vp, vp, vp, u32, vp]
    L.sml_exponents_typed.restype = i32
    L.sml_exponents_typed.argtypes = [vp, i32, u64, u32, vp, vp]
    L.sml_quantize_pack_typed.restype = i32
    L.sml_quantize_pack_typed.argtypes = [vp, i32, u64, u32, u16, vp, vp, vp, u32, vp]
    L.sml_dequantize_typed.restype = i32
    L.sml_dequantize_typed.argtypes = [vp, vp, u64, u32, u16, vp, i32, u32, vp]
    L.sml_roundtrip_loopback_typed.restype = i32
    L.sml_roundtrip_loopback_typed.argtypes = [vp, vp, i32, u64, u32, u16, vp, vp, u32, vp]
    L.sml_roundtrip_loopback_batch_typed.restype = i32
    L.sml_roundtrip_loopback_batch_typed.argtypes = [vp, u32, u32, u16, u32, vp]
    L.sml_switch_aggregate_typed.restype = i32
    L.sml_switch_aggregate_typed.argtypes = [vp, vp, u16, u64, u32, vp, vp, vp, i32, u32, vp]
    L.sml_copy_segments.restype = i32
    L.sml_copy_segments.argtypes = [vp, vp, vp, u32, u32, vp]
    L.sml_copy_segments_typed.restype = i32
    L.sml_copy_segments_typed.argtypes = [vp, vp, vp, u32, i32, u32, vp]
    L.sml_switch_exps.restype = i32
    L.sml_switch_exps.argtypes = [vp, u16, u64, vp, u32, vp]
    L.sml_copy_words.restype = i32
    L.sml_copy_words.argtypes = [vp, vp, u64, vp]
    L.sml_widen_u8_i32.restype = i32
    L.sml_widen_u8_i32.argtypes = [vp, vp, u64, vp]
    L.sml_narrow_i32_u8.restype = i32
    L.sml_narrow_i32_u8.argtypes = [vp, vp, u64, vp]
    L.sml_release_to_peers.restype = i32
    L.sml_release_to_peers.argtypes = [vp]
    L.sml_preprocess_burst.restype = i32
    L.sml_preprocess_burst.argtypes = [ctypes.POINTER(PacketBurst), vp]
    L.sml_postprocess_burst.restype = i32
    L.sml_postprocess_burst.argtypes = [ctypes.POINTER(PacketBurst), vp]
    L.sml_exchange_burst.restype = i32
    L.sml_exchange_burst.argtypes = [ctypes.POINTER(PacketBurst), vp]
    L.sml_preprocess_burst_typed.restype = i32
    L.sml_preprocess_burst_typed.argtypes = [ctypes.POINTER(PacketBurst), vp]
    L.sml_postprocess_burst_typed.restype = i32
    L.sml_postprocess_burst_typed.argtypes = [ctypes.POINTER(PacketBurst), vp]
    L.sml_exchange_burst_typed.restype = i32
    L.sml_exchange_burst_typed.argtypes = [ctypes.POINTER(PacketBurst), vp]
    L.sml_burst_server_create.restype = i32
    L.sml_burst_server_create.argtypes = [u32, u32, u32, ctypes.POINTER(vp)]
    L.sml_burst_server_submit.restype = i32
    L.sml_burst_server_submit.argtypes = [vp, u32, ctypes.POINTER(PacketBurst)]
    L.sml_burst_server_destroy.restype = i32
    L.sml_burst_server_destroy.argtypes = [vp]
    L.sml_burst_server_stop.restype = i32
    L.sml_burst_server_stop.argtypes = [vp]
    L.sml_burst_server_start.restype = i32
    L.sml_burst_server_start.argtypes = [vp]
    L.sml_burst_server_inject_unanswered.restype = i32
    L.sml_burst_server_inject_unanswered.argtypes = [vp, u32, ctypes.POINTER(PacketBurst)]
    L.sml_ipc_handle_bytes.restype = u32
    L.sml_ipc_handle_bytes.argtypes = []
    L.sml_ipc_get_handle.restype = i32
    L.sml_ipc_get_handle.argtypes = [vp, vp, ctypes.POINTER(u64)]
    L.sml_ipc_open_handle.restype = i32
    L.sml_ipc_open_handle.argtypes = [vp, ctypes.POINTER(vp)]
    L.sml_ipc_close_handle.restype = i32
    L.sml_ipc_close_handle.argtypes = [vp]
    _lib = L
    return L


def header_symbols(path: str = HEADER_PATH) -> list[str]:
    """Every function the C-ABI header declares (for the export test)."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sml_[a-z0-9_]+)\s*\(", src)))


def _check(fn: str, status: int):
    if status != SML_OK:
        raise SwitchMLError(fn, status)


def num_blocks(numel: int, packet_numel: int = 256) -> int:
    return int(lib().sml_num_blocks(numel, packet_numel))


def fifo_slice(numel: int, num_slices: int, t: int) -> tuple[int, int]:
    """(offset, numel) of slice t of a job split num_slices ways — the FIFO
    scheduler's rule (client_lib/src/schedulers/fifo_scheduler.cc:93-109):
    the first numel % num_slices slices get one extra element.  Used for the
    multi-GPU sharding mode (slice g -> GPU g, as worker thread g would get it)."""
    if num_slices <= 0 or not 0 <= t < num_slices:
        raise ValueError("need 0 <= t < num_slices")
    n = numel // num_slices
    rem = numel % num_slices
    if t < rem:
        n += 1
        return t * n, n
    return t * n + rem, n


def shard_quantize_pack(job, rank: int, world: int, packet_numel: int = 256, num_workers: int = 1,
                        flags: int = 0, stream=None):
    """Sharding mode: K1 over this rank's FIFO slice of `job` (a 1-D fp32
    device tensor holding the whole job).  Returns (offset, payload, exps);
    blocks restart at the slice start, exactly as for worker thread `rank`
    of `world` (ppp.cc:54-62 per slice)."""
    off, n = fifo_slice(job.numel(), world, rank)
    payload, exps = quantize_pack(job[off:off + n], packet_numel, num_workers, flags=flags, stream=stream)
    return off, payload, exps


def set_grid_limit(max_workgroups: int) -> int:
    return int(lib().sml_set_grid_limit(max_workgroups))


def set_payload_nt_threshold(nbytes: int) -> int:
    """Payload planes (and K4 / round-trip outputs) of at least `nbytes`
    bytes take non-temporal stores (default 64 MiB, a quarter of the Infinity
    Cache; 2**64-1 = never, 0 = always); returns the previous threshold."""
    return int(lib().sml_set_payload_nt_threshold(nbytes))


def set_quantize_tile_slices(slices: int) -> int:
    """Slices of 256 elements per K1/K2/K3 wave tile: 4, 2 or 1 for every
    kernel (never below P/256), or 0 = the default, 2 slices for every kernel
    (never below P/256); returns the previous setting."""
    return int(lib().sml_set_quantize_tile_slices(slices))


def set_stream_tile_slices(slices: int) -> int:
    """Slices of 256 elements per K4 / fused round-trip wave tile: 4 or 2,
    or 0 = the default; returns the previous setting."""
    return int(lib().sml_set_stream_tile_slices(slices))


def set_xcd_chunk(chunk: int) -> int:
    """Workgroups per contiguous run on one XCD (0 = plain order); returns the previous value."""
    return int(lib().sml_set_xcd_chunk(chunk))


# ------------------------------------------------------------- torch glue --

def _torch():
    import torch
    return torch


def _stream(stream, like=None):
    """The HIP stream to launch on: the given one, else torch's current
    stream of `like`'s device (else of the current device)."""
    torch = _torch()
    if stream is None:
        dev = like.device if like is not None and getattr(like, "is_cuda", False) else None
        stream = torch.cuda.current_stream(dev)
    return ctypes.c_void_p(stream.cuda_stream)


def _dev(t, dtype, name):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or not (t.is_cuda or t.is_pinned()):
        raise TypeError(f"{name} must be a CUDA (HIP) tensor or pinned host memory (read by the "
                        "kernel over PCIe) — the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _float_type(dtype, name):
    """sml_data_type_t of a float bucket's torch dtype: fp32, or one of the
    16-bit types the kernels convert (the sml_*_typed entry points)."""
    torch = _torch()
    code = {torch.float32: FLOAT32, torch.float16: FLOAT16, torch.bfloat16: BFLOAT16}.get(dtype)
    if code is None:
        raise TypeError(f"{name} must be float32, float16 or bfloat16, got {dtype}")
    return code


def scale_lut(num_workers: int):
    import numpy as np
    out = np.empty(256, dtype=np.float32)
    _check("sml_scale_lut", lib().sml_scale_lut(num_workers, out.ctypes.data))
    return out


def scale_lut_device(num_workers: int, device="cuda", stream=None):
    torch = _torch()
    out = torch.empty(256, dtype=torch.float32, device=device)
    _check("sml_scale_lut_device", lib().sml_scale_lut_device(num_workers, _dev(out, torch.float32, "lut"), _stream(stream, out)))
    return out


def exponents(x, packet_numel: int = 256, out=None, stream=None):
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    if out is None:
        out = torch.empty(B, dtype=torch.int8, device=x.device)
    dt = _float_type(x.dtype, "x")
    _check("sml_exponents_typed", lib().sml_exponents_typed(
        _dev(x, x.dtype, "x"), dt, x.numel(), packet_numel, _dev(out, torch.int8, "exps"), _stream(stream, x)))
    return out


def quantize_pack(x, packet_numel: int = 256, num_workers: int = 1, global_exps=None,
                  payload=None, exps_out=None, want_exps: bool = True, flags: int = 0, stream=None):
    """Returns (payload int32[B*P] (BE words unless FLAG_PAYLOAD_LE), exps int8[B] or None).
    `x` is fp32, or fp16 / bf16 (widened inside the kernel: the planes are
    those of x.float())."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    if payload is None:
        payload = torch.empty(B * packet_numel, dtype=torch.int32, device=x.device)
    if global_exps is None and want_exps and exps_out is None:
        exps_out = torch.empty(B, dtype=torch.int8, device=x.device)
    g = None if global_exps is None else _dev(global_exps, torch.int8, "global_exps")
    e = None if exps_out is None else _dev(exps_out, torch.int8, "exps_out")
    dt = _float_type(x.dtype, "x")
    _check("sml_quantize_pack_typed", lib().sml_quantize_pack_typed(
        _dev(x, x.dtype, "x"), dt, x.numel(), packet_numel, num_workers, g,
        _dev(payload, torch.int32, "payload"), e, flags, _stream(stream, x)))
    return payload, (global_exps if global_exps is not None else exps_out)


def quantize_pack_launcher(x, packet_numel: int, num_workers: int, payload, exps_out=None, global_exps=None,
                           flags: int = 0, stream=None):
    """A zero-argument callable that launches sml_quantize_pack_typed on these
    tensors: every argument checked and converted once, so a loop over the
    same bucket (a training step's gradient bucket, the bench's steps) pays
    one C call per launch instead of the wrapper's tensor checks.  The
    tensors must stay alive while the callable is used."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    if payload.numel() != B * packet_numel:
        raise ValueError(f"payload must hold B*P = {B * packet_numel} words")
    if exps_out is not None and exps_out.numel() != B:
        raise ValueError(f"exps_out must hold B = {B} bytes")
    dt = _float_type(x.dtype, "x")
    args = (x.numel(), packet_numel, num_workers,
            None if global_exps is None else _dev(global_exps, torch.int8, "global_exps"),
            _dev(payload, torch.int32, "payload"),
            None if exps_out is None else _dev(exps_out, torch.int8, "exps_out"), flags, _stream(stream, x))
    fn, args = lib().sml_quantize_pack_typed, (_dev(x, x.dtype, "x"), dt) + args

    def launch():
        s = fn(*args)
        if s != SML_OK:
            raise SwitchMLError("sml_quantize_pack_typed", s)
    return launch


def dequantize(payload, exps, numel: int, packet_numel: int = 256, num_workers: int = 1,
               out=None, flags: int = 0, stream=None, out_dtype=None):
    """K4 into `out`, or into a new bucket of `out_dtype` (default fp32; fp16 /
    bf16: the fp32 result narrowed inside the kernel, round to nearest even)."""
    torch = _torch()
    if out is None:
        out = torch.empty(numel, dtype=out_dtype or torch.float32, device=payload.device)
    elif out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype {out_dtype}")
    dt = _float_type(out.dtype, "out")
    _check("sml_dequantize_typed", lib().sml_dequantize_typed(
        _dev(payload, torch.int32, "payload"), _dev(exps, torch.int8, "exps"), numel, packet_numel,
        num_workers, _dev(out, out.dtype, "out"), dt, flags, _stream(stream, payload)))
    return out


def bswap_i32(x, out=None, stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(x)
    _check("sml_bswap_i32", lib().sml_bswap_i32(_dev(x, torch.int32, "x"), _dev(out, torch.int32, "out"),
                                                x.numel(), _stream(stream, x)))
    return out


def loopback_aggregate(payload, num_workers: int, flags: int = 0, stream=None):
    torch = _torch()
    _check("sml_loopback_aggregate", lib().sml_loopback_aggregate(
        _dev(payload, torch.int32, "payload"), payload.numel(), num_workers, flags, _stream(stream, payload)))
    return payload


def roundtrip_loopback(x, packet_numel: int = 256, num_workers: int = 1, out=None,
                       payload=None, exps_out=None, flags: int = 0, stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(x)
    p = None if payload is None else _dev(payload, torch.int32, "payload")
    e = None if exps_out is None else _dev(exps_out, torch.int8, "exps_out")
    dt = _float_type(x.dtype, "x")   # the same type in and out
    _check("sml_roundtrip_loopback_typed", lib().sml_roundtrip_loopback_typed(
        _dev(x, x.dtype, "x"), _dev(out, x.dtype, "out"), dt, x.numel(), packet_numel,
        num_workers, p, e, flags, _stream(stream, x)))
    return out


class Slice(ctypes.Structure):
    """sml_slice: one job slice of a batched round trip."""
    _fields_ = [("in_", ctypes.c_void_p), ("out", ctypes.c_void_p), ("numel", ctypes.c_uint64)]


MAX_BATCH_SLICES = 64


class TypedSlice(ctypes.Structure):
    """sml_typed_slice: one job slice of a batched round trip over any float type."""
    _fields_ = [("in_", ctypes.c_void_p), ("out", ctypes.c_void_p), ("numel", ctypes.c_uint64),
                ("data_type", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def roundtrip_loopback_batch(slices, packet_numel: int = 256, num_workers: int = 1, flags: int = 0, stream=None):
    """The fused round trip over several slices in one call: `slices` is a
    list of (x, out) device (or pinned host) tensor pairs, fp32, fp16 or bf16
    (a pair's two dtypes equal, the pairs' dtypes free); slice i gets exactly
    roundtrip_loopback(x_i, out=out_i) — its blocks start at its own first
    element.  The list goes whole through sml_roundtrip_loopback_batch_typed:
    one launch per dtype present (an all-fp32 list: the one launch of
    sml_roundtrip_loopback_batch)."""
    for x, o in slices:
        if x.numel() != o.numel():
            raise ValueError("slice in/out sizes differ")
        if getattr(x, "dtype", None) != getattr(o, "dtype", None):
            raise TypeError(f"slice in/out dtypes differ: {x.dtype}, {o.dtype}")
    st = _stream(stream, slices[0][0]) if slices else None
    arr = (TypedSlice * max(1, len(slices)))()
    for i, (x, o) in enumerate(slices):
        dt = _float_type(getattr(x, "dtype", None), "x")
        arr[i] = TypedSlice(_dev(x, x.dtype, "x").value, _dev(o, x.dtype, "out").value, x.numel(), dt, 0)
    _check("sml_roundtrip_loopback_batch_typed", lib().sml_roundtrip_loopback_batch_typed(
        arr, len(slices), packet_numel, num_workers, flags, st))


MAX_SWITCH_WORKERS = 16


def switch_aggregate(payloads, exps=None, numel: int | None = None, packet_numel: int = 256,
                     payload_out=None, exps_out=None, out=None, flags: int = 0, stream=None, out_dtype=None):
    """K6: the switch's per-slot aggregation over W worker planes, fused with
    the dequantize (p4/processor.p4:48-54 wrapping bit<32> sum,
    p4/exponents.p4:48-54 signed int8 max, then PostprocessSingle with
    scale(W, e_max), ppp.cc:197-251).  `payloads`: W int32 planes of B*P
    words (BE unless FLAG_PAYLOAD_LE); `exps`: W int8 planes of B bytes.
    Writes whichever of payload_out / exps_out / out is given; with none
    given, returns a new bucket `out` of `numel` elements of `out_dtype`
    (default fp32; fp16 / bf16, or a typed `out`: narrowed inside the kernel)."""
    torch = _torch()
    W = len(payloads)
    if W == 0 or W > MAX_SWITCH_WORKERS:
        raise ValueError(f"1 <= workers <= {MAX_SWITCH_WORKERS}, got {W}")
    n_words = payloads[0].numel()
    if any(p.numel() != n_words for p in payloads):
        raise ValueError("payload planes differ in size")
    if numel is None:
        numel = n_words
    B = num_blocks(numel, packet_numel)
    if B * packet_numel != n_words:
        raise ValueError(f"payload planes hold {n_words} words, B*P = {B * packet_numel}")
    if exps is not None:
        if len(exps) != W or any(e.numel() != B for e in exps):
            raise ValueError("need one exponent plane of B bytes per payload plane")
    if out is None and (out_dtype is not None or (payload_out is None and exps_out is None)):
        out = torch.empty(numel, dtype=out_dtype or torch.float32, device=payloads[0].device)
    elif out is not None and out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype {out_dtype}")
    dt = FLOAT32 if out is None else _float_type(out.dtype, "out")
    # planes are int32 tensors, or (peer-to-peer switch) mapped peer planes
    # exposing data_ptr()/numel() only
    pp = (ctypes.c_void_p * W)(*[_dev(p, torch.int32, "payloads[w]").value if isinstance(p, torch.Tensor)
                                 else p.data_ptr() for p in payloads])
    ep = None if exps is None else (ctypes.c_void_p * W)(*[_dev(e, torch.int8, "exps[w]").value for e in exps])
    _check("sml_switch_aggregate_typed", lib().sml_switch_aggregate_typed(
        ctypes.cast(pp, ctypes.c_void_p), None if ep is None else ctypes.cast(ep, ctypes.c_void_p), W, numel,
        packet_numel,
        None if payload_out is None else _dev(payload_out, torch.int32, "payload_out"),
        None if exps_out is None else _dev(exps_out, torch.int8, "exps_out"),
        None if out is None else _dev(out, out.dtype, "out"), dt, flags, _stream(stream, payloads[0])))
    return out


def switch_exps(exps, out=None, flags: int = 0, stream=None):
    """sml_switch_exps: the switch's exponent half alone, out[k] = the signed
    int8 max over the W planes `exps` (int8, equal length) of byte k
    (p4/exponents.p4:48-54).  The planes and `out` may sit at any byte
    alignment.  flags = FLAG_PEER_PLANES when planes were written by other
    GPUs.  Returns `out`."""
    torch = _torch()
    W = len(exps)
    if W == 0 or W > MAX_SWITCH_WORKERS:
        raise ValueError(f"1 <= workers <= {MAX_SWITCH_WORKERS}, got {W}")
    B = exps[0].numel()
    if any(e.numel() != B for e in exps):
        raise ValueError("exponent planes differ in size")
    if out is None:
        out = torch.empty(B, dtype=torch.int8, device=exps[0].device)
    elif out.numel() != B:
        raise ValueError(f"out must hold B = {B} bytes")
    ep = (ctypes.c_void_p * W)(*[_dev(e, torch.int8, "exps[w]").value for e in exps])
    _check("sml_switch_exps", lib().sml_switch_exps(
        ctypes.cast(ep, ctypes.c_void_p), W, B, _dev(out, torch.int8, "out"), flags, _stream(stream, exps[0])))
    return out


def copy_words(src, dst, stream=None):
    """sml_copy_words: `src` copied into `dst`, 32-bit tensors of equal numel
    (any 32-bit dtypes, any 4-byte alignment; CUDA or pinned host).  Returns
    `dst`."""
    if src.numel() != dst.numel() or src.element_size() != 4 or dst.element_size() != 4:
        raise ValueError("src and dst are 32-bit tensors of equal numel")
    _check("sml_copy_words", lib().sml_copy_words(_dev(src, src.dtype, "src"), _dev(dst, dst.dtype, "dst"),
                                                  src.numel(), _stream(stream, src)))
    return dst


def widen_u8_i32(x, out=None, stream=None):
    """sml_widen_u8_i32: each uint8 of `x` zero-extended into an int32 (the
    CollNet plugin's ncclUint8 buckets on their way into the INT32
    all-reduce).  `x` may start at any byte.  Returns `out`."""
    torch = _torch()
    if out is None:
        out = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    elif out.numel() != x.numel():
        raise ValueError("x and out differ in numel")
    _check("sml_widen_u8_i32", lib().sml_widen_u8_i32(_dev(x, torch.uint8, "x"), _dev(out, torch.int32, "out"),
                                                      x.numel(), _stream(stream, x)))
    return out


def narrow_i32_u8(x, out=None, stream=None):
    """sml_narrow_i32_u8: the low byte of each int32 of `x` (the sum mod 256),
    back into a uint8 bucket at any byte.  Returns `out`."""
    torch = _torch()
    if out is None:
        out = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    elif out.numel() != x.numel():
        raise ValueError("x and out differ in numel")
    _check("sml_narrow_i32_u8", lib().sml_narrow_i32_u8(_dev(x, torch.int32, "x"), _dev(out, torch.uint8, "out"),
                                                        x.numel(), _stream(stream, x)))
    return out


def _segment_tables(pairs, dtype=None):
    """The three tables of a segment copy — sources, destinations, element
    counts, as void* — from (src, dst) tensor pairs of equal numel, all of
    `dtype` (None: any 32-bit dtypes, each tensor its own)."""
    k = len(pairs)
    srcs = (ctypes.c_void_p * max(1, k))()
    dsts = (ctypes.c_void_p * max(1, k))()
    numel = (ctypes.c_uint64 * max(1, k))()
    for i, (s, d) in enumerate(pairs):
        if s.numel() != d.numel() or (dtype is None and (s.element_size() != 4 or d.element_size() != 4)):
            raise ValueError("segments are pairs of equal-size " + ("32-bit tensors" if dtype is None else "tensors"))
        srcs[i] = _dev(s, dtype or s.dtype, "src").value
        dsts[i] = _dev(d, dtype or d.dtype, "dst").value
        numel[i] = s.numel()
    return tuple(ctypes.cast(t, ctypes.c_void_p) for t in (srcs, dsts, numel))


def copy_segments(pairs, flags: int = 0, stream=None):
    """sml_copy_segments: every (src, dst) pair of 32-bit tensors (same
    numel; CUDA or pinned host) copied in ONE launch, the tiles dealt
    round-robin over the pairs (the in-node switch's multicast).
    flags = FLAG_PEER_PLANES when sources were written by other GPUs."""
    if len(pairs) > MAX_SWITCH_WORKERS:
        raise ValueError(f"at most {MAX_SWITCH_WORKERS} segments")
    srcs, dsts, words = _segment_tables(pairs)
    _check("sml_copy_segments", lib().sml_copy_segments(
        srcs, dsts, words, len(pairs), flags, _stream(stream, pairs[0][0] if pairs else None)))


def copy_segments_typed(pairs, flags: int = 0, stream=None):
    """sml_copy_segments_typed: every (src, dst) pair of tensors of one dtype
    (same numel; CUDA or pinned host) copied in ONE launch.  float16 /
    bfloat16 pairs may start at any element (views at odd offsets) and hold
    an odd number of elements; float32 / int32 pairs go to sml_copy_segments'
    kernel.  The in-node switch's multicast of a job of that type."""
    torch = _torch()
    k = len(pairs)
    if k > MAX_SWITCH_WORKERS:
        raise ValueError(f"at most {MAX_SWITCH_WORKERS} segments")
    dtypes = {t.dtype for pair in pairs for t in pair}
    if len(dtypes) > 1:
        raise TypeError(f"segments are tensors of one dtype, got {sorted(map(str, dtypes))}")
    dtype = dtypes.pop() if dtypes else torch.float32
    dt = INT32 if dtype == torch.int32 else _float_type(dtype, "segments")
    srcs, dsts, numel = _segment_tables(pairs, dtype)
    _check("sml_copy_segments_typed", lib().sml_copy_segments_typed(
        srcs, dsts, numel, k, dt, flags, _stream(stream, pairs[0][0] if pairs else None)))


def packet_burst(x, out, packet_numel: int, num_workers: int, batch_num_ltus: int, recv_exps, pkt_ids,
                 entries, extras, flags: int = 0) -> PacketBurst:
    """A PacketBurst over slice `x` (fp32, fp16, bf16 or int32 CUDA tensor) and
    output `out`; entries / extras are device-addressable addresses (ints).
    A 16-bit slice's burst runs through preprocess_burst / postprocess_burst /
    exchange_burst (the typed entry points), not through a BurstServer."""
    torch = _torch()
    if len(pkt_ids) > MAX_BURST:
        raise ValueError(f"at most {MAX_BURST} packets per burst")
    b = PacketBurst()
    b.in_ = x.data_ptr()
    b.out = out.data_ptr() if out is not None else None
    b.numel = x.numel()
    b.packet_numel = packet_numel
    b.num_workers = num_workers
    b.data_type = {torch.int32: INT32, torch.float16: FLOAT16, torch.bfloat16: BFLOAT16}.get(x.dtype, FLOAT32)
    b.batch_num_ltus = batch_num_ltus
    b.recv_exps = recv_exps.data_ptr() if recv_exps is not None else None
    b.count = len(pkt_ids)
    b.flags = flags
    for i, (q, e, x_) in enumerate(zip(pkt_ids, entries, extras)):
        b.pkt_ids[i], b.entries[i], b.extras[i] = q, e, x_
    return b


def preprocess_burst(burst: PacketBurst, stream=None, like=None):
    """sml_preprocess_burst_typed: PreprocessSingle for every packet of the
    burst (a FLOAT32 / INT32 burst is sml_preprocess_burst's)."""
    _check("sml_preprocess_burst", lib().sml_preprocess_burst_typed(ctypes.byref(burst), _stream(stream, like)))


def postprocess_burst(burst: PacketBurst, stream=None, like=None):
    """sml_postprocess_burst_typed: PostprocessSingle for every packet of the
    burst (a FLOAT32 / INT32 burst is sml_postprocess_burst's)."""
    _check("sml_postprocess_burst", lib().sml_postprocess_burst_typed(ctypes.byref(burst), _stream(stream, like)))


def exchange_burst(burst: PacketBurst, stream=None, like=None):
    """sml_exchange_burst_typed: for every received packet q, PostprocessSingle(q)
    then PreprocessSingle(q + b) into the same buffer (the DPDK receive loop's
    post + ReusePacket) in one launch; FLAG_PROCESS_PACKET applies the dummy
    backend's ProcessPacket (x W) first."""
    _check("sml_exchange_burst", lib().sml_exchange_burst_typed(ctypes.byref(burst), _stream(stream, like)))


BURST_PRE, BURST_POST, BURST_EXCHANGE = 0, 1, 2


class BurstServer:
    """sml_burst_server_*: a persistent workgroup that runs bursts submitted
    through a doorbell in host memory (for packet buffers in pinned host
    memory).  submit() returns with the burst complete; close() stops it."""

    def __init__(self, packet_numel: int, flags: int = 0, idle_ms: int = 100):
        self._h = ctypes.c_void_p()
        _check("sml_burst_server_create", lib().sml_burst_server_create(packet_numel, flags, idle_ms,
                                                                        ctypes.byref(self._h)))

    def submit(self, op: int, burst: PacketBurst):
        _check("sml_burst_server_submit", lib().sml_burst_server_submit(self._h, op, ctypes.byref(burst)))

    def stop(self):
        """Leave the loop now (the next submit restarts it)."""
        _check("sml_burst_server_stop", lib().sml_burst_server_stop(self._h))

    def start(self):
        """Start the loop now instead of on the next submit."""
        _check("sml_burst_server_start", lib().sml_burst_server_start(self._h))

    def inject_unanswered(self, op: int, burst: PacketBurst):
        """Test fault injection: ring the doorbell for `burst` with the server
        stopped (what a failed submit leaves behind)."""
        _check("sml_burst_server_inject_unanswered",
               lib().sml_burst_server_inject_unanswered(self._h, op, ctypes.byref(burst)))

    def close(self):
        if self._h:
            h, self._h = self._h, None
            _check("sml_burst_server_destroy", lib().sml_burst_server_destroy(h))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().sml_burst_server_destroy(self._h)
            self._h = None


def release_to_peers(stream=None, device=None):
    """sml_release_to_peers: system-scope release on every XCD after the work
    on `stream` (the writer's half of a hand-off to other GPUs)."""
    if stream is None:
        stream = _torch().cuda.current_stream(device)
    _check("sml_release_to_peers", lib().sml_release_to_peers(_stream(stream)))


def stream_copy(src, dst, stream=None):
    """Measurement probe: non-temporal tile copy (src/dst same byte size)."""
    nbytes = src.numel() * src.element_size()
    _check("sml_stream_copy", lib().sml_stream_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                                                    nbytes, _stream(stream, src)))
    return dst


def frame_bytes(packet_numel: int = 256) -> int:
    return int(lib().sml_frame_bytes(packet_numel))


def quantize_pack_frames(x, params: FrameParams, packet_numel: int = 256, num_workers: int = 1,
                         batch_max: int = 64, global_exps=None, frames=None, stride: int | None = None,
                         stream=None):
    """Fused quantize + pack straight into DPDK frames (B + b frames of
    `stride` bytes, uint8).  `frames` may be a device tensor or pinned host
    memory (the NIC's buffers).  `x` is fp32, or fp16 / bf16 (widened inside
    the kernel: the frames are those of x.float())."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    b = min(B, batch_max)
    stride = stride or frame_bytes(packet_numel)
    if frames is None:
        frames = torch.empty((B + b) * stride, dtype=torch.uint8, device=x.device)
    g = None if global_exps is None else _dev(global_exps, torch.int8, "global_exps")
    dt = _float_type(x.dtype, "x")
    _check("sml_quantize_pack_frames_typed", lib().sml_quantize_pack_frames_typed(
        _dev(x, x.dtype, "x"), dt, x.numel(), packet_numel, num_workers, g, batch_max,
        ctypes.byref(params), _dev(frames, torch.uint8, "frames"), stride, _stream(stream, x)))
    return frames


class RxSlice:
    """Receive-side state of one job slice for dequantize_frames: the
    received exponents, the rx bitmap (DpdkWorkerThread's rte_bitmap,
    dpdk_worker_thread.cc:316-342) and {accepted, discarded} counters.
    `dtype` is the output's element type: fp32, or fp16 / bf16 (narrowed
    inside the kernel); a given `out` must be of it."""

    def __init__(self, numel: int, packet_numel: int = 256, batch_max: int = 64, device="cuda",
                 out=None, dtype=None):
        torch = _torch()
        dtype = dtype or (out.dtype if out is not None else torch.float32)
        _float_type(dtype, "dtype")
        if out is not None and out.dtype != dtype:
            raise TypeError(f"out is {out.dtype}, dtype {dtype}")
        self.dtype = dtype
        self.numel, self.packet_numel, self.batch_max = numel, packet_numel, batch_max
        B = num_blocks(numel, packet_numel)
        self.exps = torch.zeros(B, dtype=torch.int8, device=device)
        self.state = torch.zeros(int(lib().sml_rx_state_words(numel, packet_numel, batch_max, 0)),
                                 dtype=torch.int64, device=device)
        self.counts = torch.zeros(2, dtype=torch.int64, device=device)
        self.out = out if out is not None else torch.zeros(numel, dtype=dtype, device=device)

    def reset(self, stream=None):
        """rte_bitmap_reset for a new job slice: zero the rx state (one async
        memset, sml_rx_reset)."""
        torch = _torch()
        _check("sml_rx_reset", lib().sml_rx_reset(_dev(self.state, torch.int64, "state"), self.state.numel(),
                                                  _stream(stream, self.state)))


def dequantize_frames(frames, num_frames: int, rx: RxSlice, num_workers: int = 1, job_id: int = 0,
                      stride: int | None = None, stream=None):
    """PostprocessSingle over received DPDK frames (any order; duplicates and
    other jobs' frames discarded), writing rx.out / rx.exps / rx.counts.
    An fp16 / bf16 rx.out is narrowed inside the kernel."""
    torch = _torch()
    stride = stride or frame_bytes(rx.packet_numel)
    dt = _float_type(rx.out.dtype, "rx.out")
    _check("sml_dequantize_frames_typed", lib().sml_dequantize_frames_typed(
        _dev(frames, torch.uint8, "frames"), num_frames, stride, rx.numel, rx.packet_numel, num_workers,
        rx.batch_max, job_id, _dev(rx.exps, torch.int8, "exps"), _dev(rx.state, torch.int64, "state"),
        _dev(rx.out, rx.out.dtype, "out"), dt, _dev(rx.counts, torch.int64, "counts"), _stream(stream, rx.out)))
    return rx.out


def pack_frames_int32(x, params: FrameParams, packet_numel: int = 256, frames=None, stride: int | None = None,
                      stream=None):
    """An INT32 job slice straight into DPDK frames: B frames (no extra
    batch), frame p = BuildPacket's headers + htonl of block p's words."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    stride = stride or frame_bytes(packet_numel)
    if frames is None:
        frames = torch.empty(B * stride, dtype=torch.uint8, device=x.device)
    _check("sml_pack_frames_int32", lib().sml_pack_frames_int32(
        _dev(x, torch.int32, "x"), x.numel(), packet_numel, ctypes.byref(params),
        _dev(frames, torch.uint8, "frames"), stride, _stream(stream, x)))
    return frames


class RxSliceInt32:
    """Receive-side state of one INT32 job slice for unpack_frames_int32: the
    rx bitmap over its B pkt_ids, six header words and the fix-up's dirty
    list (uint64[2B + 6], sml_rx_state_words), {accepted, discarded}
    counters, the output.

    The header words' indices into `state` (sml_frames.hip, kRx*): CALL the
    slice's call sequence, TOTAL the conflicts resolved so far, CONFLICTS and
    LISTED the conflict count and dirty-list length of the call in progress
    (0 between calls), ARRIVALS the fix-up workgroups finished over the
    slice's life (FIXUP_BLOCKS per call), LAST_LISTED what LISTED held when
    the last call's fix-up ended; LIST is the dirty list's first word."""

    FIXUP_BLOCKS = 128          # k_rx_int32_fixup's grid (kRxFixupBlocks)

    def __init__(self, numel: int, packet_numel: int = 256, device="cuda", out=None):
        torch = _torch()
        self.numel, self.packet_numel = numel, packet_numel
        self.nblocks = num_blocks(numel, packet_numel)
        (self.CALL, self.TOTAL, self.CONFLICTS, self.LISTED, self.ARRIVALS, self.LAST_LISTED,
         self.LIST) = range(self.nblocks, self.nblocks + 7)
        self.state = torch.zeros(int(lib().sml_rx_state_words(numel, packet_numel, 1, 1)), dtype=torch.int64,
                                 device=device)
        self.counts = torch.zeros(2, dtype=torch.int64, device=device)
        self.out = out if out is not None else torch.zeros(numel, dtype=torch.int32, device=device)

    @property
    def conflicts(self) -> int:
        """Copies of a pkt_id that claimed it ahead of an earlier copy and were
        resolved by the fix-up, over the slice so far (reads the device)."""
        return int(self.state[self.TOTAL].item())

    def reset(self, stream=None):
        """rte_bitmap_reset for a new job slice (sml_rx_reset)."""
        torch = _torch()
        _check("sml_rx_reset", lib().sml_rx_reset(_dev(self.state, torch.int64, "state"), self.state.numel(),
                                                  _stream(stream, self.state)))


def unpack_frames_int32(frames, num_frames: int, rx: RxSliceInt32, job_id: int = 0, stride: int | None = None,
                        stream=None):
    """PostprocessSingle's INT32 branch over received DPDK frames (any order;
    duplicates, other jobs' frames and pkt_id >= B discarded): ntohl into rx.out."""
    torch = _torch()
    stride = stride or frame_bytes(rx.packet_numel)
    _check("sml_unpack_frames_int32", lib().sml_unpack_frames_int32(
        _dev(frames, torch.uint8, "frames"), num_frames, stride, rx.numel, rx.packet_numel, job_id,
        _dev(rx.state, torch.int64, "state"), _dev(rx.out, torch.int32, "out"),
        _dev(rx.counts, torch.int64, "counts"), _stream(stream, rx.out)))
    return rx.out


class FrameSwitch:
    """The switch between DPDK workers (sml_frame_switch): owns the slot
    pool's registers on the device and aggregates a batch of arrived frames
    per call.  `workers`: a (mac bytes, dotted IPv4) pair per worker, or a
    ready FrameSwitchParams as `params`."""

    def __init__(self, workers=None, num_slots: int = 64, packet_numel: int = 256, device="cuda",
                 switch_mac=b"\x02\x00\x00\x00\x00\x01", switch_ip="10.0.0.253", params=None):
        torch = _torch()
        self.params = params if params is not None else frame_switch_params(
            workers, num_slots, packet_numel, switch_mac=switch_mac, switch_ip=switch_ip)
        self.packet_numel = int(self.params.packet_numel)
        self.num_slots = int(self.params.num_slots)
        nbytes = int(lib().sml_frame_switch_state_bytes(self.num_slots, self.packet_numel))
        if nbytes == 0:
            raise SwitchMLError("sml_frame_switch_state_bytes", SML_ERR_UNSUPPORTED)
        self.state = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        self.counts = torch.zeros(5, dtype=torch.int64, device=device)
        # the egress (deliver): the workers' receive rings and their fill counts
        self.rings = None
        self.ring_count = torch.zeros(int(self.params.num_workers), dtype=torch.int64, device=device)
        self.deliver_counts = torch.zeros(4, dtype=torch.int64, device=device)
        self._scratch = None
        self.reset()

    def reset(self, stream=None):
        """Clear the switch's registers: every slot empty, both sets (sml_frame_switch_reset)."""
        torch = _torch()
        _check("sml_frame_switch_reset", lib().sml_frame_switch_reset(
            _dev(self.state, torch.int64, "state"), self.num_slots, self.packet_numel, _stream(stream, self.state)))

    def __call__(self, frames, num_frames: int, out=None, stride: int | None = None, out_stride: int | None = None,
                 verdict=None, stream=None):
        """Aggregate `num_frames` arrived frames (`stride` bytes apart; device
        or pinned host memory).  Returns (out, verdict, counts): the result
        frame of input frame i at out[i * out_stride:] where verdict[i] is
        VERDICT_BROADCAST or VERDICT_RETRANSMIT (other positions keep their
        bytes), the uint8 verdicts, and the switch's running per-verdict
        counters.  VERDICT_DEFERRED frames are to be resubmitted in a later call."""
        torch = _torch()
        stride = stride or frame_bytes(self.packet_numel)
        out_stride = out_stride or stride
        dev = self.state.device
        if out is None:
            out = torch.zeros(max(1, num_frames) * out_stride, dtype=torch.uint8, device=dev)
        if verdict is None:
            verdict = torch.empty(max(1, num_frames), dtype=torch.uint8, device=dev)
        _check("sml_frame_switch", lib().sml_frame_switch(
            ctypes.byref(self.params), _dev(frames, torch.uint8, "frames"), num_frames, stride,
            _dev(self.state, torch.int64, "state"), _dev(out, torch.uint8, "out"), out_stride,
            _dev(verdict, torch.uint8, "verdict"), _dev(self.counts, torch.int64, "counts"),
            _stream(stream, self.state)))
        return out, verdict[:num_frames], self.counts

    def reset_rings(self, stream=None):
        """Empty every worker's receive ring: the ring counts and the delivery
        counters go to zero (the rings keep their bytes)."""
        torch = _torch()
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            self.ring_count.zero_()
            self.deliver_counts.zero_()

    def deliver(self, out, verdict, num_frames: int, rings=None, ring_frames: int | None = None, drop=None,
                out_stride: int | None = None, rx_stride: int | None = None, ring_bytes: int | None = None,
                ring_count=None, stream=None):
        """The egress of one call (sml_frame_switch_deliver): `out` / `verdict`
        as __call__ returned them; every BROADCAST is appended to every
        worker's ring, addressed to that worker, every RETRANSMIT to its
        asker's, in input order behind what earlier calls left.  `rings`:
        uint8 [W, ring_frames, rx_stride] (device or pinned host memory), or
        any contiguous uint8 tensor with `ring_frames`, `rx_stride` and
        `ring_bytes` given; None = the switch's own (allocated on first use,
        `ring_frames` frames per worker).  `drop`: int32 [num_frames], bit u =
        the copy for worker u is lost.  `ring_count`: int64 [W], default the
        switch's own.  Returns (rings, ring_count, counts) with counts =
        {delivered, dropped, overflow, unroutable}, running."""
        torch = _torch()
        fb = frame_bytes(self.packet_numel)
        W = int(self.params.num_workers)
        dev = self.state.device
        if rings is None:
            rings = self.rings
        if rings is None:
            if not ring_frames:
                raise ValueError("ring_frames is needed to allocate the rings")
            rings = torch.zeros((W, ring_frames, rx_stride or fb), dtype=torch.uint8, device=dev)
        if rings.dim() == 3:
            ring_frames = ring_frames or rings.shape[1]
            rx_stride = rx_stride or rings.shape[2]
            ring_bytes = ring_bytes or rings.shape[1] * rings.shape[2]
        rx_stride = rx_stride or fb
        if not ring_frames:
            raise ValueError("ring_frames is needed for rings that are not [W, ring_frames, rx_stride]")
        ring_bytes = ring_bytes or ring_frames * rx_stride
        if rings.numel() < (W - 1) * ring_bytes + ring_frames * rx_stride:
            raise ValueError("rings is smaller than W rings of ring_bytes")
        self.rings = rings
        ring_count = ring_count if ring_count is not None else self.ring_count
        need = int(lib().sml_frame_switch_deliver_scratch_bytes(num_frames, W))
        if self._scratch is None or self._scratch.numel() * 8 < need:
            self._scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        d = None if drop is None else _dev(drop, torch.int32, "drop")
        _check("sml_frame_switch_deliver", lib().sml_frame_switch_deliver(
            ctypes.byref(self.params), _dev(out, torch.uint8, "out"), num_frames, out_stride or fb,
            _dev(verdict, torch.uint8, "verdict"), d, _dev(rings, torch.uint8, "rings"), ring_bytes, ring_frames,
            rx_stride, _dev(ring_count, torch.int64, "ring_count"), _dev(self.deliver_counts, torch.int64, "counts"),
            _dev(self._scratch, torch.int64, "scratch"), _stream(stream, self.state)))
        return rings, ring_count, self.deliver_counts


def gather_frames(sets, set_idx, frame_idx, packet_numel: int = 256, set_frames: int | None = None,
                  set_stride: int | None = None, out=None, out_stride: int | None = None, skipped=None, stream=None):
    """One switch call's input from the workers' tx frame sets
    (sml_frame_gather): output frame j = frame frame_idx[j] (int64) of
    sets[set_idx[j]] (int32).  `sets`: up to 32 uint8 tensors (device or pinned
    host memory) of `set_frames` frames `set_stride` bytes apart (default:
    packed, as many as the smallest set holds).  An entry out of range writes
    nothing and adds 1 to `skipped` (int64 [1], device).  Returns (out, skipped)."""
    torch = _torch()
    fb = frame_bytes(packet_numel)
    set_stride = set_stride or fb
    out_stride = out_stride or fb
    sets = list(sets)
    if not sets:
        raise ValueError("at least one set")
    if set_frames is None:
        set_frames = min(s.numel() // set_stride for s in sets)
    elif any(s.numel() < (set_frames - 1) * set_stride + fb for s in sets):
        raise ValueError("a set is smaller than set_frames frames")
    n = set_idx.numel()
    if frame_idx.numel() != n:
        raise ValueError("set_idx and frame_idx differ in length")
    dev = set_idx.device
    if out is None:
        out = torch.zeros(max(1, n) * out_stride, dtype=torch.uint8, device=dev)
    if skipped is None:
        skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * len(sets))(*[_dev(s, torch.uint8, "sets").value for s in sets])
    _check("sml_frame_gather", lib().sml_frame_gather(
        ptrs, len(sets), set_frames, set_stride, _dev(set_idx, torch.int32, "set_idx"),
        _dev(frame_idx, torch.int64, "frame_idx"), n, packet_numel, _dev(out, torch.uint8, "out"), out_stride,
        _dev(skipped, torch.int64, "skipped"), _stream(stream, set_idx)))
    return out, skipped


def debug_stall(microseconds: int, stream=None):
    """Fault injection for tests: keep `stream` busy for `microseconds` of
    device wall-clock time (<= 60 s), then end (sml_debug_stall)."""
    _check("sml_debug_stall", lib().sml_debug_stall(int(microseconds), _stream(stream)))


def rdma_imm(exps, batch_max: int = 64, stream=None, num_blocks_int32: int | None = None, device=None):
    """RDMA immediates of one slice's B + b messages (uint32 in host order, as
    int32 tensor): (msg_id & 0xFFFF) | exponent << 16.  exps=None with
    num_blocks_int32=B: an INT32 slice's B messages, msg_id & 0xFFFF."""
    torch = _torch()
    if exps is None:
        B = int(num_blocks_int32)
        out = torch.empty(B, dtype=torch.int32, device=device or "cuda")
        _check("sml_rdma_imm_int32", lib().sml_rdma_imm_int32(B, _dev(out, torch.int32, "imm"),
                                                             _stream(stream, out)))
        return out
    B = exps.numel()
    out = torch.empty(B + min(B, batch_max), dtype=torch.int32, device=exps.device)
    _check("sml_rdma_imm", lib().sml_rdma_imm(_dev(exps, torch.int8, "exps"), B, batch_max,
                                             _dev(out, torch.int32, "imm"), _stream(stream, exps)))
    return out
