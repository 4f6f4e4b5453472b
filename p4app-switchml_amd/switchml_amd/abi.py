"""The C ABI of libswitchml_hip.so, and the only Python module that knows it:
the constants, structures and prototypes of include/switchml_hip.h (the
kernels) and include/switchml_client.h (the client Context), written by hand
from the two headers and held to them type by type by tests/test_abi_cpu.py.

Plain ctypes: neither torch nor numpy is imported, and the library is loaded
on the first lib() / call(), not on import.  There is no CPU fallback: if the
library was not built, lib() raises.
"""
from __future__ import annotations

import ctypes
import os
import re

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libswitchml_hip.so")
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(PKG_DIR)), "include")
HEADER_PATH = os.path.join(_INCLUDE, "switchml_hip.h")
CLIENT_HEADER_PATH = os.path.join(_INCLUDE, "switchml_client.h")

# sml_status_t
SML_OK, SML_ERR_INVALID_ARG, SML_ERR_UNSUPPORTED, SML_ERR_ALIGNMENT, SML_ERR_HIP = range(5)

FLAG_PAYLOAD_LE = 0x1
FLAG_ROUND_RNE = 0x2
FLAG_PEER_PLANES = 0x4   # inputs written by other GPUs: acquire first (sml_release_to_peers on the writer)
FLAG_PROCESS_PACKET = 0x8   # sml_exchange_burst: the dummy backend's ProcessPacket (x W) on each packet first

PACKET_NUMELS = (64, 128, 256, 512, 1024)

# sml_data_type_t
FLOAT32, INT32, FLOAT16, BFLOAT16 = 0, 1, 2, 3

MAX_BATCH_SLICES = 64
MAX_SWITCH_WORKERS = 16
MAX_BURST = 64
MAX_FRAME_SWITCH_WORKERS = 32
MAX_FRAME_SWITCH_SLOTS = 16384
# sml_frame_switch's verdict per input frame
VERDICT_CONSUMED, VERDICT_BROADCAST, VERDICT_RETRANSMIT, VERDICT_IGNORED, VERDICT_DEFERRED = range(5)
# sml_burst_server_submit's op
BURST_PRE, BURST_POST, BURST_EXCHANGE = 0, 1, 2

u64, u32, u16, u8, i32, vp = (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint16, ctypes.c_uint8, ctypes.c_int,
                              ctypes.c_void_p)
cstr, ptr = ctypes.c_char_p, ctypes.POINTER


class Slice(ctypes.Structure):
    """sml_slice: one job slice of a batched round trip."""
    _fields_ = [("in_", vp), ("out", vp), ("numel", u64)]


class TypedSlice(ctypes.Structure):
    """sml_typed_slice: one job slice of a batched round trip over any float type."""
    _fields_ = [("in_", vp), ("out", vp), ("numel", u64), ("data_type", u32), ("reserved", u32)]


class PacketBurst(ctypes.Structure):
    """sml_packet_burst: up to MAX_BURST per-packet calls of one job slice in one launch."""
    _fields_ = [("in_", vp), ("out", vp), ("numel", u64), ("packet_numel", u32), ("num_workers", u16),
                ("data_type", u16), ("batch_num_ltus", u64), ("recv_exps", vp), ("count", u32), ("flags", u32),
                ("pkt_ids", u64 * MAX_BURST), ("entries", vp * MAX_BURST), ("extras", vp * MAX_BURST)]


class FrameParams(ctypes.Structure):
    """sml_frame_params (include/switchml_hip.h): addresses in network byte order."""
    _fields_ = [("dst_mac", u8 * 6), ("src_mac", u8 * 6), ("src_ip_be", u32), ("dst_ip_be", u32),
                ("src_port_be", u16), ("dst_port_be", u16), ("job_id", u64), ("pool_index_start", u32),
                ("pool_index_shift", u32), ("max_outstanding_pkts", u32)]


class SwitchWorker(ctypes.Structure):
    """sml_switch_worker: a worker's MAC and its IPv4 address in network byte order."""
    _fields_ = [("mac", u8 * 6), ("ip_be", u32)]


class FrameSwitchParams(ctypes.Structure):
    """sml_frame_switch_params (include/switchml_hip.h)."""
    _fields_ = [("switch_mac", u8 * 6), ("switch_ip_be", u32), ("num_workers", u16), ("num_slots", u32),
                ("packet_numel", u32), ("workers", SwitchWorker * MAX_FRAME_SWITCH_WORKERS)]


_burst, _frame, _switch = ptr(PacketBurst), ptr(FrameParams), ptr(FrameSwitchParams)

# entry point -> (restype, argtypes): every function of the two headers, in the headers' order
SIGNATURES = {
    # include/switchml_hip.h
    "sml_abi_version": (i32, []),
    "sml_status_string": (cstr, [i32]),
    "sml_last_error": (cstr, []),
    "sml_num_blocks": (u64, [u64, u32]),
    "sml_scale_lut": (i32, [u16, vp]),
    "sml_scale_lut_device": (i32, [u16, vp, vp]),
    "sml_exponents": (i32, [vp, u64, u32, vp, vp]),
    "sml_quantize_pack": (i32, [vp, u64, u32, u16, vp, vp, vp, u32, vp]),
    "sml_dequantize": (i32, [vp, vp, u64, u32, u16, vp, u32, vp]),
    "sml_bswap_i32": (i32, [vp, vp, u64, vp]),
    "sml_loopback_aggregate": (i32, [vp, u64, u16, u32, vp]),
    "sml_roundtrip_loopback": (i32, [vp, vp, u64, u32, u16, vp, vp, u32, vp]),
    "sml_roundtrip_loopback_batch": (i32, [ptr(Slice), u32, u32, u16, u32, vp]),
    "sml_switch_aggregate": (i32, [vp, vp, u16, u64, u32, vp, vp, vp, u32, vp]),
    "sml_exponents_typed": (i32, [vp, i32, u64, u32, vp, vp]),
    "sml_quantize_pack_typed": (i32, [vp, i32, u64, u32, u16, vp, vp, vp, u32, vp]),
    "sml_dequantize_typed": (i32, [vp, vp, u64, u32, u16, vp, i32, u32, vp]),
    "sml_roundtrip_loopback_typed": (i32, [vp, vp, i32, u64, u32, u16, vp, vp, u32, vp]),
    "sml_switch_aggregate_typed": (i32, [vp, vp, u16, u64, u32, vp, vp, vp, i32, u32, vp]),
    "sml_roundtrip_loopback_batch_typed": (i32, [ptr(TypedSlice), u32, u32, u16, u32, vp]),
    "sml_switch_exps": (i32, [vp, u16, u64, vp, u32, vp]),
    "sml_copy_words": (i32, [vp, vp, u64, vp]),
    "sml_copy_segments": (i32, [vp, vp, vp, u32, u32, vp]),
    "sml_copy_segments_typed": (i32, [vp, vp, vp, u32, i32, u32, vp]),
    "sml_release_to_peers": (i32, [vp]),
    "sml_preprocess_burst": (i32, [_burst, vp]),
    "sml_postprocess_burst": (i32, [_burst, vp]),
    "sml_exchange_burst": (i32, [_burst, vp]),
    "sml_preprocess_burst_typed": (i32, [_burst, vp]),
    "sml_postprocess_burst_typed": (i32, [_burst, vp]),
    "sml_exchange_burst_typed": (i32, [_burst, vp]),
    "sml_burst_server_create": (i32, [u32, u32, u32, ptr(vp)]),
    "sml_burst_server_submit": (i32, [vp, u32, _burst]),
    "sml_burst_server_stop": (i32, [vp]),
    "sml_burst_server_destroy": (i32, [vp]),
    "sml_burst_server_start": (i32, [vp]),
    "sml_burst_server_inject_unanswered": (i32, [vp, u32, _burst]),
    "sml_ipc_handle_bytes": (u32, []),
    "sml_ipc_get_handle": (i32, [vp, vp, ptr(u64)]),
    "sml_ipc_open_handle": (i32, [vp, ptr(vp)]),
    "sml_ipc_close_handle": (i32, [vp]),
    "sml_frame_bytes": (u64, [u32]),
    "sml_rx_state_words": (u64, [u64, u32, u32, i32]),
    "sml_quantize_pack_frames": (i32, [vp, u64, u32, u16, vp, u32, _frame, vp, u64, vp]),
    "sml_dequantize_frames": (i32, [vp, u64, u64, u64, u32, u16, u32, u64, vp, vp, vp, vp, vp]),
    "sml_quantize_pack_frames_typed": (i32, [vp, i32, u64, u32, u16, vp, u32, _frame, vp, u64, vp]),
    "sml_dequantize_frames_typed": (i32, [vp, u64, u64, u64, u32, u16, u32, u64, vp, vp, vp, i32, vp, vp]),
    "sml_pack_frames_int32": (i32, [vp, u64, u32, _frame, vp, u64, vp]),
    "sml_unpack_frames_int32": (i32, [vp, u64, u64, u64, u32, u64, vp, vp, vp, vp]),
    "sml_rx_reset": (i32, [vp, u64, vp]),
    "sml_frame_switch_state_bytes": (u64, [u32, u32]),
    "sml_frame_switch_reset": (i32, [vp, u32, u32, vp]),
    "sml_frame_switch": (i32, [_switch, vp, u64, u64, vp, vp, u64, vp, vp, vp]),
    "sml_frame_switch_deliver_scratch_bytes": (u64, [u64, u32]),
    "sml_frame_switch_deliver": (i32, [_switch, vp, u64, u64, vp, vp, vp, u64, u64, u64, vp, vp, vp, vp]),
    "sml_frame_gather": (i32, [ptr(vp), u32, u64, u64, vp, vp, u64, u32, vp, u64, vp, vp]),
    "sml_widen_u8_i32": (i32, [vp, vp, u64, vp]),
    "sml_narrow_i32_u8": (i32, [vp, vp, u64, vp]),
    "sml_rdma_imm": (i32, [vp, u64, u32, vp, vp]),
    "sml_rdma_imm_int32": (i32, [u64, vp, vp]),
    "sml_stream_copy": (i32, [vp, vp, u64, vp]),
    "sml_debug_stall": (i32, [u32, vp]),
    "sml_set_grid_limit": (u32, [u32]),
    "sml_set_xcd_chunk": (u32, [u32]),
    "sml_set_quantize_tile_slices": (u32, [u32]),
    "sml_set_stream_tile_slices": (u32, [u32]),
    "sml_set_payload_nt_threshold": (u64, [u64]),
    # include/switchml_client.h
    "sml_context_start": (i32, [cstr]),
    "sml_context_stop": (i32, []),
    "sml_context_state": (i32, []),
    "sml_context_last_error": (cstr, []),
    "sml_context_config": (cstr, []),
    "sml_allreduce_async": (i32, [vp, vp, u64, i32, i32, ptr(vp)]),
    "sml_allreduce": (i32, [vp, vp, u64, i32, i32]),
    "sml_wait_for_all_jobs": (i32, []),
    "sml_job_wait": (i32, [vp]),
    "sml_job_status": (i32, [vp]),
    "sml_job_id": (u64, [vp]),
    "sml_job_release": (None, [vp]),
    "sml_context_stats": (i32, [vp]),
    "sml_context_batch_stats": (i32, [vp]),
    "sml_ppp_per_ltu_calls": (i32, [cstr]),
}

_lib = None


def lib():
    """Load libswitchml_hip.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found — build it with `make -C p4app-switchml_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


class SwitchMLError(RuntimeError):
    def __init__(self, fn: str, status: int):
        L = lib()
        msg = L.sml_status_string(status).decode()
        err = L.sml_last_error().decode()
        super().__init__(f"{fn} failed: {msg}" + (f" ({err})" if err else ""))
        self.status = status


def call(name: str, *args) -> None:
    """Call the entry point `name`, which returns an sml_status_t; a status
    other than SML_OK raises SwitchMLError naming it."""
    status = getattr(_lib or lib(), name)(*args)
    if status != SML_OK:
        raise SwitchMLError(name, status)


def header_symbols(path: str = HEADER_PATH) -> list[str]:
    """Every function the C-ABI header declares (for the export test)."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sml_[a-z0-9_]+)\s*\(", src)))
