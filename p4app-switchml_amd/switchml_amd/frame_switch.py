"""The switch between DPDK workers: the slot pool that aggregates a batch of
arrived frames per call, its egress into the workers' receive rings and its
ingress from their tx frame sets."""
from __future__ import annotations

import contextlib
import ctypes

from .abi import (MAX_FRAME_SWITCH_WORKERS, SML_ERR_UNSUPPORTED, FrameSwitchParams, SwitchMLError, call, lib)
from .frames import frame_bytes
from .glue import _dev, _opt, _ptr_table, _stream, _torch


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
        call("sml_frame_switch_reset", _dev(self.state, torch.int64, "state"), self.num_slots, self.packet_numel,
             _stream(stream, self.state))

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
        call("sml_frame_switch", ctypes.byref(self.params), _dev(frames, torch.uint8, "frames"), num_frames, stride,
             _dev(self.state, torch.int64, "state"), _dev(out, torch.uint8, "out"), out_stride,
             _dev(verdict, torch.uint8, "verdict"), _dev(self.counts, torch.int64, "counts"),
             _stream(stream, self.state))
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
        d = _opt(drop, torch.int32, "drop")
        call("sml_frame_switch_deliver", ctypes.byref(self.params), _dev(out, torch.uint8, "out"), num_frames,
             out_stride or fb, _dev(verdict, torch.uint8, "verdict"), d, _dev(rings, torch.uint8, "rings"),
             ring_bytes, ring_frames, rx_stride, _dev(ring_count, torch.int64, "ring_count"),
             _dev(self.deliver_counts, torch.int64, "counts"), _dev(self._scratch, torch.int64, "scratch"),
             _stream(stream, self.state))
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
    call("sml_frame_gather", _ptr_table(sets, torch.uint8, "sets"), len(sets), set_frames, set_stride,
         _dev(set_idx, torch.int32, "set_idx"), _dev(frame_idx, torch.int64, "frame_idx"), n, packet_numel,
         _dev(out, torch.uint8, "out"), out_stride, _dev(skipped, torch.int64, "skipped"), _stream(stream, set_idx))
    return out, skipped
