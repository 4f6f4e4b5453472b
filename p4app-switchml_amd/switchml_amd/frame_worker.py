"""One DPDK worker thread's receive loop on the device (sml_frame_worker_*,
DESIGN §9 F3 "Worker side"): the per-slot state (expected pkt_id, kept
exponent) lives in device memory; `begin` builds a slice's first batch into the
tx ring, `poll` accepts a batch of received frames and rebuilds each slot's
next frame, `resend` names an outstanding one again.  What they return are tx
slot indices (int64, FRAME_WORKER_NONE = -1 for "nothing"), which
gather_frames takes as its frame_idx as they are."""
from __future__ import annotations

import ctypes

from .abi import (BFLOAT16, FLOAT16, FLOAT32, INT32, SML_ERR_UNSUPPORTED, FrameParams, FrameWorkerParams,
                  SwitchMLError, call, lib)
from .frames import frame_bytes
from .glue import _dev, _opt, _stream, _torch
from .planes import num_blocks


class FrameWorker:
    """Owns one worker thread's slot state and verdict counts on the device.
    `params`: the thread's FrameParams (frame_params()); its
    max_outstanding_pkts is the tx ring's slot count Q."""

    def __init__(self, params: FrameParams, num_workers: int, packet_numel: int = 256, dtype=None, device="cuda",
                 flags: int = 0):
        torch = _torch()
        dtype = torch.float32 if dtype is None else dtype
        code = {torch.float32: FLOAT32, torch.int32: INT32, torch.float16: FLOAT16, torch.bfloat16: BFLOAT16}.get(dtype)
        if code is None:
            raise TypeError(f"dtype must be float32, int32, float16 or bfloat16, got {dtype}")
        self.dtype, self.packet_numel = dtype, packet_numel
        self.num_slots = int(params.max_outstanding_pkts)
        self.params = FrameWorkerParams(params, num_workers, code, packet_numel, flags)
        nbytes = int(lib().sml_frame_worker_state_bytes(self.num_slots))
        if nbytes == 0:
            raise SwitchMLError("sml_frame_worker_state_bytes", SML_ERR_UNSUPPORTED)
        self.state = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        # WRONG, POSTED, FINISHED, IGNORED: running
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        self.total = None                       # frames of the slice begun last
        self.reset()

    def _state(self):
        return _dev(self.state, _torch().int64, "state")

    def _ring(self, t, frames, stride, name):
        torch = _torch()
        stride = stride or frame_bytes(self.packet_numel)
        if frames and t.numel() < (frames - 1) * stride + frame_bytes(self.packet_numel):
            raise ValueError(f"{name} is smaller than {frames} frames {stride} bytes apart")
        return _dev(t, torch.uint8, name), stride

    def reset(self, stream=None):
        """No slice under way; the counters go to zero.  pool_index_shift keeps its value."""
        call("sml_frame_worker_reset", self._state(), self.num_slots, _stream(stream, self.state))
        self.counts.zero_()
        self.total = None

    def begin(self, x, out, tx, tx_stride: int | None = None, stream=None):
        """Start the slice x -> out (tensors of the worker's dtype, out may be
        x): frames 0..b-1 into the tx ring (uint8, num_slots slots `tx_stride`
        apart), and the slots to send, one entry per slot (NONE past the
        batch).  A slice after the first moves pool_index_shift on by the
        frames of the one before (dpdk_worker_thread.cc:392)."""
        torch = _torch()
        if x.numel() != out.numel():
            raise ValueError("x and out must hold the same number of elements")
        fp = self.params.frame
        if self.total is not None:
            fp.pool_index_shift = (fp.pool_index_shift + self.total) % (2 * self.num_slots)
        B = num_blocks(x.numel(), self.packet_numel)
        self.total = B if self.dtype == torch.int32 else B + min(B, self.num_slots)
        sends = torch.empty(self.num_slots, dtype=torch.int64, device=self.state.device)
        ring, tx_stride = self._ring(tx, self.num_slots, tx_stride, "tx")
        call("sml_frame_worker_begin", ctypes.byref(self.params), _dev(x, self.dtype, "x"),
             _dev(out, self.dtype, "out"), x.numel(), self._state(), ring, tx_stride,
             _dev(sends, torch.int64, "sends"), _stream(stream, self.state))
        return sends

    def poll(self, rx, n: int, tx, num_frames=None, rx_stride: int | None = None, tx_stride: int | None = None,
             stream=None):
        """One call over the n frames of `rx` (uint8, `rx_stride` apart; what
        deliver left in this worker's ring).  `num_frames`: an int64 device
        tensor of one element, the ring's live count (FrameSwitch.ring_count[u:u + 1]):
        frames from it on are IGNORED unread, so n may be the ring's capacity.
        Returns (verdict uint8 [n], sends int64 [n]); sends[i] is the tx slot
        rebuilt where verdict[i] is FRAME_WORKER_POSTED, else NONE."""
        torch = _torch()
        dev = self.state.device
        sends = torch.empty(max(1, n), dtype=torch.int64, device=dev)
        verdict = torch.empty(max(1, n), dtype=torch.uint8, device=dev)
        d_rx, rx_stride = self._ring(rx, n, rx_stride, "rx")
        d_tx, tx_stride = self._ring(tx, self.num_slots, tx_stride, "tx")
        call("sml_frame_worker_poll", ctypes.byref(self.params), d_rx, n, rx_stride,
             _opt(num_frames, torch.int64, "num_frames"), self._state(), d_tx, tx_stride,
             _dev(sends, torch.int64, "sends"), _dev(verdict, torch.uint8, "verdict"),
             _dev(self.counts, torch.int64, "counts"), _stream(stream, self.state))
        return verdict[:n], sends[:n]

    def resend(self, slots, stream=None):
        """The slot again for each tx slot index in `slots` (a sequence or an
        int32 device tensor) that has a frame outstanding, else NONE; nothing
        else changes."""
        torch = _torch()
        if not isinstance(slots, torch.Tensor):
            slots = torch.tensor(list(slots), dtype=torch.int32).to(self.state.device)
        n = slots.numel()
        sends = torch.empty(max(1, n), dtype=torch.int64, device=self.state.device)
        call("sml_frame_worker_resend", ctypes.byref(self.params), _dev(slots, torch.int32, "slots"), n, self._state(),
             _dev(sends, torch.int64, "sends"), _stream(stream, self.state))
        return sends[:n]
