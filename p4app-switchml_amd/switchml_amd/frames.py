"""A worker's DPDK frames: the tx kernels (quantize + pack, INT32 pack straight
into frames), the receive-side state of a job slice and the rx kernels over
it, and the RDMA immediates."""
from __future__ import annotations

import ctypes

from .abi import FrameParams, call, lib
from .glue import _dev, _float_type, _opt, _stream, _torch
from .planes import num_blocks


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


def frame_bytes(packet_numel: int = 256) -> int:
    return int(lib().sml_frame_bytes(packet_numel))


def _stride(stride, packet_numel: int) -> int:
    """The bytes between two frames of a call: packed, unless given."""
    return stride or frame_bytes(packet_numel)


def _tx_frames(x, num_frames: int, packet_numel: int, frames, stride):
    """(frames, stride) of a tx call: a new uint8 tensor of `num_frames`
    frames on x's device, unless given."""
    torch = _torch()
    stride = _stride(stride, packet_numel)
    if frames is None:
        frames = torch.empty(num_frames * stride, dtype=torch.uint8, device=x.device)
    return frames, stride


def quantize_pack_frames(x, params: FrameParams, packet_numel: int = 256, num_workers: int = 1,
                         batch_max: int = 64, global_exps=None, frames=None, stride: int | None = None,
                         stream=None):
    """Fused quantize + pack straight into DPDK frames (B + b frames of
    `stride` bytes, uint8).  `frames` may be a device tensor or pinned host
    memory (the NIC's buffers).  `x` is fp32, or fp16 / bf16 (widened inside
    the kernel: the frames are those of x.float())."""
    torch = _torch()
    B = num_blocks(x.numel(), packet_numel)
    frames, stride = _tx_frames(x, B + min(B, batch_max), packet_numel, frames, stride)
    g = _opt(global_exps, torch.int8, "global_exps")
    dt = _float_type(x.dtype, "x")
    call("sml_quantize_pack_frames_typed", _dev(x, x.dtype, "x"), dt, x.numel(), packet_numel, num_workers, g,
         batch_max, ctypes.byref(params), _dev(frames, torch.uint8, "frames"), stride, _stream(stream, x))
    return frames


def pack_frames_int32(x, params: FrameParams, packet_numel: int = 256, frames=None, stride: int | None = None,
                      stream=None):
    """An INT32 job slice straight into DPDK frames: B frames (no extra
    batch), frame p = BuildPacket's headers + htonl of block p's words."""
    torch = _torch()
    frames, stride = _tx_frames(x, num_blocks(x.numel(), packet_numel), packet_numel, frames, stride)
    call("sml_pack_frames_int32", _dev(x, torch.int32, "x"), x.numel(), packet_numel, ctypes.byref(params),
         _dev(frames, torch.uint8, "frames"), stride, _stream(stream, x))
    return frames


class _RxState:
    """What the two receive-side states share: `state`, the uint64 words
    sml_rx_state_words asks for, zeroed, and {accepted, discarded} `counts`."""

    def _alloc(self, batch_max: int, int32: int, device):
        torch = _torch()
        self.state = torch.zeros(int(lib().sml_rx_state_words(self.numel, self.packet_numel, batch_max, int32)),
                                 dtype=torch.int64, device=device)
        self.counts = torch.zeros(2, dtype=torch.int64, device=device)

    def reset(self, stream=None):
        """rte_bitmap_reset for a new job slice: zero the rx state (one async
        memset, sml_rx_reset)."""
        torch = _torch()
        call("sml_rx_reset", _dev(self.state, torch.int64, "state"), self.state.numel(), _stream(stream, self.state))


class RxSlice(_RxState):
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
        self._alloc(batch_max, 0, device)
        self.out = out if out is not None else torch.zeros(numel, dtype=dtype, device=device)


def dequantize_frames(frames, num_frames: int, rx: RxSlice, num_workers: int = 1, job_id: int = 0,
                      stride: int | None = None, stream=None):
    """PostprocessSingle over received DPDK frames (any order; duplicates and
    other jobs' frames discarded), writing rx.out / rx.exps / rx.counts.
    An fp16 / bf16 rx.out is narrowed inside the kernel."""
    torch = _torch()
    stride = _stride(stride, rx.packet_numel)
    dt = _float_type(rx.out.dtype, "rx.out")
    call("sml_dequantize_frames_typed", _dev(frames, torch.uint8, "frames"), num_frames, stride, rx.numel,
         rx.packet_numel, num_workers, rx.batch_max, job_id, _dev(rx.exps, torch.int8, "exps"),
         _dev(rx.state, torch.int64, "state"), _dev(rx.out, rx.out.dtype, "out"), dt,
         _dev(rx.counts, torch.int64, "counts"), _stream(stream, rx.out))
    return rx.out


class RxSliceInt32(_RxState):
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
        self._alloc(1, 1, device)
        self.out = out if out is not None else torch.zeros(numel, dtype=torch.int32, device=device)

    @property
    def conflicts(self) -> int:
        """Copies of a pkt_id that claimed it ahead of an earlier copy and were
        resolved by the fix-up, over the slice so far (reads the device)."""
        return int(self.state[self.TOTAL].item())


def unpack_frames_int32(frames, num_frames: int, rx: RxSliceInt32, job_id: int = 0, stride: int | None = None,
                        stream=None):
    """PostprocessSingle's INT32 branch over received DPDK frames (any order;
    duplicates, other jobs' frames and pkt_id >= B discarded): ntohl into rx.out."""
    torch = _torch()
    stride = _stride(stride, rx.packet_numel)
    call("sml_unpack_frames_int32", _dev(frames, torch.uint8, "frames"), num_frames, stride, rx.numel,
         rx.packet_numel, job_id, _dev(rx.state, torch.int64, "state"), _dev(rx.out, torch.int32, "out"),
         _dev(rx.counts, torch.int64, "counts"), _stream(stream, rx.out))
    return rx.out


def rdma_imm(exps, batch_max: int = 64, stream=None, num_blocks_int32: int | None = None, device=None):
    """RDMA immediates of one slice's B + b messages (uint32 in host order, as
    int32 tensor): (msg_id & 0xFFFF) | exponent << 16.  exps=None with
    num_blocks_int32=B: an INT32 slice's B messages, msg_id & 0xFFFF."""
    torch = _torch()
    if exps is None:
        B = int(num_blocks_int32)
        out = torch.empty(B, dtype=torch.int32, device=device or "cuda")
        call("sml_rdma_imm_int32", B, _dev(out, torch.int32, "imm"), _stream(stream, out))
        return out
    B = exps.numel()
    out = torch.empty(B + min(B, batch_max), dtype=torch.int32, device=exps.device)
    call("sml_rdma_imm", _dev(exps, torch.int8, "exps"), B, batch_max, _dev(out, torch.int32, "imm"),
         _stream(stream, exps))
    return out
