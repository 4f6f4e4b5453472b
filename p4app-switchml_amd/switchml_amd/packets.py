"""Per-packet calls, a burst per launch: PreprocessSingle / PostprocessSingle /
the receive loop's exchange for up to MAX_BURST packets, and the persistent
burst server for packet buffers in pinned host memory."""
import ctypes

from .abi import BFLOAT16, FLOAT16, FLOAT32, INT32, MAX_BURST, PacketBurst, call, lib
from .glue import _stream, _torch


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
    call("sml_preprocess_burst_typed", ctypes.byref(burst), _stream(stream, like))


def postprocess_burst(burst: PacketBurst, stream=None, like=None):
    """sml_postprocess_burst_typed: PostprocessSingle for every packet of the
    burst (a FLOAT32 / INT32 burst is sml_postprocess_burst's)."""
    call("sml_postprocess_burst_typed", ctypes.byref(burst), _stream(stream, like))


def exchange_burst(burst: PacketBurst, stream=None, like=None):
    """sml_exchange_burst_typed: for every received packet q, PostprocessSingle(q)
    then PreprocessSingle(q + b) into the same buffer (the DPDK receive loop's
    post + ReusePacket) in one launch; FLAG_PROCESS_PACKET applies the dummy
    backend's ProcessPacket (x W) first."""
    call("sml_exchange_burst_typed", ctypes.byref(burst), _stream(stream, like))


class BurstServer:
    """sml_burst_server_*: a persistent workgroup that runs bursts submitted
    through a doorbell in host memory (for packet buffers in pinned host
    memory).  submit() returns with the burst complete; close() stops it."""

    def __init__(self, packet_numel: int, flags: int = 0, idle_ms: int = 100):
        self._h = ctypes.c_void_p()
        call("sml_burst_server_create", packet_numel, flags, idle_ms, ctypes.byref(self._h))

    def submit(self, op: int, burst: PacketBurst):
        call("sml_burst_server_submit", self._h, op, ctypes.byref(burst))

    def stop(self):
        """Leave the loop now (the next submit restarts it)."""
        call("sml_burst_server_stop", self._h)

    def start(self):
        """Start the loop now instead of on the next submit."""
        call("sml_burst_server_start", self._h)

    def inject_unanswered(self, op: int, burst: PacketBurst):
        """Test fault injection: ring the doorbell for `burst` with the server
        stopped (what a failed submit leaves behind)."""
        call("sml_burst_server_inject_unanswered", self._h, op, ctypes.byref(burst))

    def close(self):
        if self._h:
            h, self._h = self._h, None
            call("sml_burst_server_destroy", h)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().sml_burst_server_destroy(self._h)
            self._h = None
