"""The switch between RDMA workers (sml_rdma_switch and, for long messages,
sml_msg_switch: DESIGN §9 F4 "Switch side"): the slot pool that aggregates a
batch of landed messages per call and writes the results into the workers'
receive regions."""
from __future__ import annotations

import ctypes

from .abi import PACKET_NUMELS, SML_ERR_UNSUPPORTED, RdmaArrival, RdmaSwitchParams, SwitchMLError, call, lib
from .glue import _dev, _opt, _stream, _torch

ARRIVAL_BYTES = ctypes.sizeof(RdmaArrival)
# numpy's view of sml_rdma_arrival (np.dtype(ARRIVAL_FIELDS)); the package itself does not import numpy
ARRIVAL_FIELDS = [("worker", "<u4"), ("rkey", "<u4"), ("imm", "<u4"), ("src", "<u4"), ("addr", "<u8")]


def rdma_rkey(slot: int, set_: int, pkts_per_msg: int) -> int:
    """The pool index a worker puts in the rkey (rdma_worker_thread.cc:118-128)."""
    return ((slot * pkts_per_msg) << 1) | set_


class RdmaSwitch:
    """Owns the message slots' registers on the device; `step` is one call
    over a batch of completion records.  A packet-sized message with
    pkts_per_msg 1, 2, 4, 8 or 16 runs on sml_rdma_switch*; every other
    supported length (a multiple of 64 up to 16384 words) and pkts_per_msg up
    to 256 on sml_msg_switch*, chosen here once."""

    def __init__(self, num_workers: int, num_slots: int, msg_numel: int = 1024, pkts_per_msg: int = 4,
                 device="cuda"):
        torch = _torch()
        self.params = RdmaSwitchParams(num_workers, num_slots, msg_numel, pkts_per_msg)
        self.num_workers, self.num_slots = num_workers, num_slots
        self.msg_numel, self.pkts_per_msg = msg_numel, pkts_per_msg
        # the family of entry points this object calls: "sml_rdma_switch" or "sml_msg_switch"
        short = msg_numel in PACKET_NUMELS and pkts_per_msg in (1, 2, 4, 8, 16)
        self.entry = "sml_rdma_switch" if short else "sml_msg_switch"
        nbytes = int(getattr(lib(), self.entry + "_state_bytes")(num_slots, msg_numel))
        if nbytes == 0:
            raise SwitchMLError(self.entry + "_state_bytes", SML_ERR_UNSUPPORTED)
        self.state = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        # CONSUMED, BROADCAST, RETRANSMIT, IGNORED, DEFERRED, dropped copies: running
        self.counts = torch.zeros(6, dtype=torch.int64, device=device)
        self.reset()

    def reset(self, stream=None):
        """Every slot empty, both sets (the family's _reset); the counters go to zero."""
        torch = _torch()
        call(self.entry + "_reset", _dev(self.state, torch.int64, "state"), self.num_slots, self.msg_numel,
             _stream(stream, self.state))
        self.counts.zero_()

    def _records(self, arrivals):
        """(tensor, n) of a structured numpy array of the record's dtype, or of
        an integer tensor that views whole records."""
        torch = _torch()
        if not isinstance(arrivals, torch.Tensor):
            if arrivals.dtype.itemsize != ARRIVAL_BYTES or arrivals.dtype.names != tuple(n for n, _ in ARRIVAL_FIELDS):
                raise TypeError("arrivals must have sml_rdma_arrival's dtype (ARRIVAL_FIELDS)")
            flat = arrivals.reshape(-1).copy().view("u1")
            return torch.from_numpy(flat).to(self.state.device), arrivals.size
        if arrivals.dtype not in (torch.uint8, torch.int32, torch.int64) or not arrivals.is_contiguous():
            raise TypeError("arrivals must be a contiguous uint8, int32 or int64 view of the records")
        nbytes = arrivals.numel() * arrivals.element_size()
        if nbytes % ARRIVAL_BYTES:
            raise ValueError(f"arrivals must hold whole {ARRIVAL_BYTES}-byte records")
        return arrivals, nbytes // ARRIVAL_BYTES

    def step(self, arrivals, landing, rx, drop=None, verdict=None, out_imm=None, stream=None):
        """One call.  `landing`: [landing_msgs, stride] of landed messages,
        `rx`: [num_workers, rx_bytes / itemsize], the workers' receive regions
        (both uint8 or int32, device or pinned host memory, contiguous).
        `drop`: int32 [n], bit u = worker u's copy of record i's result is
        lost.  Returns (verdict uint8 [n], out_imm int32 [n]); out_imm[i] is
        written where verdict[i] is VERDICT_BROADCAST or VERDICT_RETRANSMIT.
        VERDICT_DEFERRED records are to be resubmitted in a later call."""
        torch = _torch()
        records, n = self._records(arrivals)
        if landing.dim() != 2 or rx.dim() != 2 or rx.shape[0] != self.num_workers:
            raise ValueError("landing must be [landing_msgs, stride] and rx [num_workers, rx_bytes]")
        dev = self.state.device
        if verdict is None:
            verdict = torch.empty(max(1, n), dtype=torch.uint8, device=dev)
        if out_imm is None:
            out_imm = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
        if verdict.numel() < n or out_imm.numel() < n or (drop is not None and drop.numel() < n):
            raise ValueError("verdict, out_imm and drop hold an entry per record")
        call(self.entry, ctypes.byref(self.params), _dev(records, records.dtype, "arrivals"), n,
             _dev(landing, landing.dtype, "landing"), landing.shape[1] * landing.element_size(), landing.shape[0],
             _dev(self.state, torch.int64, "state"), _dev(rx, rx.dtype, "rx"), rx.shape[1] * rx.element_size(),
             _opt(drop, torch.int32, "drop"), _dev(out_imm, torch.int32, "out_imm"),
             _dev(verdict, torch.uint8, "verdict"), _dev(self.counts, torch.int64, "counts"),
             _stream(stream, self.state))
        return verdict[:n], out_imm[:n]
