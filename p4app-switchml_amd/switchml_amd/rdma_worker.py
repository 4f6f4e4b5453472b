"""One RDMA worker thread's completion loop on the device (sml_rdma_worker_*
and, for long messages, sml_msg_worker_*: DESIGN §9 F4 "Worker side"): the per-QP state (expected message id, kept
exponent, pool flag) lives in device memory; `begin` posts a slice's first
batch, `poll` accepts a batch of completions and builds each QP's next
message, `resend` repeats an outstanding one.  What they return are
sml_rdma_arrival records, which RdmaSwitch.step takes as they are."""
from __future__ import annotations

import ctypes

from .abi import (BFLOAT16, FLOAT16, FLOAT32, INT32, PACKET_NUMELS, SML_ERR_UNSUPPORTED, RdmaCompletion, RdmaWorkerParams,
                  SwitchMLError, call, lib)
from .glue import _dev, _stream, _torch
from .rdma_switch import ARRIVAL_BYTES

COMPLETION_BYTES = ctypes.sizeof(RdmaCompletion)
# numpy's view of sml_rdma_completion (np.dtype(COMPLETION_FIELDS)); the package itself does not import numpy
COMPLETION_FIELDS = [("qpn", "<u4"), ("imm", "<u4")]


class RdmaWorker:
    """Owns one worker thread's QP state and verdict counts on the device.  A
    packet-sized message with pkts_per_msg 1, 2, 4, 8 or 16 runs on
    sml_rdma_worker_*; every other supported length (a multiple of 64 up to
    16384 words) and pkts_per_msg up to 256 on sml_msg_worker_*, chosen here
    once."""

    def __init__(self, worker: int, num_workers: int, num_qps: int, msg_numel: int = 1024, pkts_per_msg: int = 4,
                 first_slot: int = 0, src_base: int = 0, dtype=None, device="cuda", flags: int = 0):
        torch = _torch()
        dtype = torch.float32 if dtype is None else dtype
        code = {torch.float32: FLOAT32, torch.int32: INT32, torch.float16: FLOAT16, torch.bfloat16: BFLOAT16}.get(dtype)
        if code is None:
            raise TypeError(f"dtype must be float32, int32, float16 or bfloat16, got {dtype}")
        self.dtype, self.num_qps, self.msg_numel = dtype, num_qps, msg_numel
        self.params = RdmaWorkerParams(worker, num_workers, code, msg_numel, pkts_per_msg, num_qps, first_slot,
                                       src_base, flags)
        # the family of entry points this object calls: "sml_rdma_worker" or "sml_msg_worker"
        short = msg_numel in PACKET_NUMELS and pkts_per_msg in (1, 2, 4, 8, 16)
        self.entry = "sml_rdma_worker" if short else "sml_msg_worker"
        nbytes = int(getattr(lib(), self.entry + "_state_bytes")(num_qps))
        if nbytes == 0:
            raise SwitchMLError(self.entry + "_state_bytes", SML_ERR_UNSUPPORTED)
        self.state = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        # WRONG, POSTED, FINISHED, IGNORED: running
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        self.reset()

    def _state(self):
        return _dev(self.state, _torch().int64, "state")

    def _sends(self, n):
        """n records, as the int64 view [n, 3] RdmaSwitch.step takes."""
        torch = _torch()
        return torch.empty((max(1, n), ARRIVAL_BYTES // 8), dtype=torch.int64, device=self.state.device)

    def _buffer(self, t, name):
        if t.numel() * t.element_size() < self.num_qps * 4 * self.msg_numel:
            raise ValueError(f"{name} must hold a message per QP")
        return _dev(t, t.dtype, name)

    def reset(self, stream=None):
        """No slice under way, every QP's pool flag 1; the counters go to zero."""
        call(self.entry + "_reset", self._state(), self.num_qps, _stream(stream, self.state))
        self.counts.zero_()

    def begin(self, x, out, tx, stream=None):
        """Start the slice x -> out (tensors of the worker's dtype, out may be
        x): the first batch's records, one per QP (null records past the
        batch).  `tx`: the QPs' message buffers, num_qps * msg_numel words."""
        if x.numel() != out.numel():
            raise ValueError("x and out must hold the same number of elements")
        sends = self._sends(self.num_qps)
        call(self.entry + "_begin", ctypes.byref(self.params), _dev(x, self.dtype, "x"),
             _dev(out, self.dtype, "out"), x.numel(), self._state(), self._buffer(tx, "tx"),
             _dev(sends, sends.dtype, "sends"), _stream(stream, self.state))
        return sends

    def poll(self, completions, rx, tx, stream=None):
        """One call over a batch of completions: a structured numpy array of
        COMPLETION_FIELDS, or a contiguous int64 / int32 device tensor viewing
        whole records.  `rx`: where the QPs' results arrived (may be `tx`).
        Returns (verdict uint8 [n], sends int64 [n, 3]); sends[i] is QP's next
        message where verdict[i] is RDMA_WORKER_POSTED, else the null record."""
        torch = _torch()
        dev = self.state.device
        if not isinstance(completions, torch.Tensor):
            if completions.dtype.itemsize != COMPLETION_BYTES or \
                    completions.dtype.names != tuple(n for n, _ in COMPLETION_FIELDS):
                raise TypeError("completions must have sml_rdma_completion's dtype (COMPLETION_FIELDS)")
            completions = torch.from_numpy(completions.reshape(-1).copy().view("i8")).to(dev)
        if completions.dtype not in (torch.int32, torch.int64) or not completions.is_contiguous():
            raise TypeError("completions must be a contiguous int32 or int64 view of the records")
        nbytes = completions.numel() * completions.element_size()
        if nbytes % COMPLETION_BYTES:
            raise ValueError(f"completions must hold whole {COMPLETION_BYTES}-byte records")
        n = nbytes // COMPLETION_BYTES
        sends = self._sends(n)
        verdict = torch.empty(max(1, n), dtype=torch.uint8, device=dev)
        call(self.entry + "_poll", ctypes.byref(self.params), _dev(completions, completions.dtype, "completions"), n,
             self._state(), self._buffer(rx, "rx"), self._buffer(tx, "tx"), _dev(sends, sends.dtype, "sends"),
             _dev(verdict, torch.uint8, "verdict"), _dev(self.counts, torch.int64, "counts"),
             _stream(stream, self.state))
        return verdict[:n], sends[:n]

    def resend(self, qpns, stream=None):
        """The outstanding message's record again for each QP index in `qpns`
        (a sequence or an int32 device tensor); nothing else changes."""
        torch = _torch()
        if not isinstance(qpns, torch.Tensor):
            qpns = torch.tensor(list(qpns), dtype=torch.int32).to(self.state.device)
        n = qpns.numel()
        sends = self._sends(n)
        call(self.entry + "_resend", ctypes.byref(self.params), _dev(qpns, torch.int32, "qpns"), n, self._state(),
             _dev(sends, sends.dtype, "sends"), _stream(stream, self.state))
        return sends[:n]
