"""GPU: every runtime axis of every kernel launch site against the oracle,
bit for bit.

The entry points pick a template instance of their kernel from runtime
values (csrc/sml_dispatch.h): packet size, tile slices, alignment, byte
order, rounding, store policy, reciprocal form.  A constant that reaches a
kernel in the wrong template position compiles and gives wrong bits only on
the flag combination that differs, so each axis is run here with both of its
values at every packet size.  Shapes are the smallest that still cover two
full 1024-element tiles, a partial packet and a ragged tail:
n = 4 * 1024 + P + 3.

Cells other files cover already (K1 / K2 / K3 under every tile size, byte
order and rounding: test_launch_geometry.py) are not repeated.
"""
import contextlib
import functools

import numpy as np
import pytest

from oracle import oracle as O
from switchml_amd import frame_wire as FW

pytestmark = pytest.mark.gpu

from test_frames_int32 import int32_data, stream as int32_stream  # noqa: E402
from test_frames_rx import _run_gpu as run_rx, rx_stream  # noqa: E402
from test_switch_gpu import oracle_switch, worker_planes  # noqa: E402

PACKETS = (64, 128, 256, 512, 1024)
NEVER = 2 ** 64 - 1
NT = (0, NEVER)                  # non-temporal stores always / never
SENT = 0x5A5A5A5A                # words no kernel has written


def size(P):
    return 4 * 1024 + P + 3


@pytest.fixture
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


@contextlib.contextmanager
def knobs(sw):
    """The launch knobs a test moves, restored whatever happens."""
    orig = sw.set_payload_nt_threshold(NEVER)
    try:
        yield
    finally:
        sw.set_stream_tile_slices(0)
        sw.set_payload_nt_threshold(orig)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def planes(P, W, rounding=O.HALF_AWAY, seed=0):
    """One slice's oracle planes, computed once and shared read-only:
    (x, payload as sent, exponents, payload after the x W loopback, output)."""
    n = size(P)
    x = O.splitmix_normal(1000 * seed + P, n)
    q, e = O.quantize(x, P, W, rounding=rounding), O.exponents(x, P)
    agg = O.loopback_aggregate(q, W)
    return frozen(x, q, e, agg, O.dequantize(agg, e, n, P, W))


def words(t):
    return t.cpu().numpy().view(np.uint32)


def up(torch, arr, dev, off=0):
    """A copy of `arr` on the device, `off` elements past a 16-byte boundary."""
    src = torch.from_numpy(np.array(arr))
    buf = torch.empty(arr.size + 4, dtype=src.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + arr.size]
    t.copy_(src)
    return t


# ------------------------------------------------------------- planes --

@pytest.mark.parametrize("P", PACKETS)
def test_dequantize_axes(sw, cuda, P):
    """sml_dequantize: output aligned / 4-byte offset x BE / LE words x
    W = 3 (division) / 4 (reciprocal) x store policy x 2 / 4 tile slices."""
    import torch
    n = size(P)
    with knobs(sw):
        for W in (3, 4):
            _, _, e, agg, dq = planes(P, W)
            d_e = up(torch, e, cuda)
            d_be = up(torch, agg.view(np.int32), cuda)
            d_le = up(torch, O.bswap32(agg).view(np.int32), cuda)
            for off in (0, 1):
                for le in (False, True):
                    for nt in NT:
                        for sl in (2, 4):
                            sw.set_payload_nt_threshold(nt)
                            sw.set_stream_tile_slices(sl)
                            out = torch.zeros(n + 4, device=cuda)[off:off + n]
                            sw.dequantize(d_le if le else d_be, d_e, n, P, W, out=out,
                                          flags=sw.FLAG_PAYLOAD_LE if le else 0)
                            assert np.array_equal(words(out), dq.view(np.uint32)), (W, off, le, nt, sl)


@pytest.mark.parametrize("P", PACKETS)
def test_roundtrip_loopback_axes(sw, cuda, P):
    """sml_roundtrip_loopback with its payload and exponent planes: in / out
    aligned / offset x byte order x rounding x W = 3 / 4 x store policy x
    2 / 4 tile slices (P = 1024 keeps 4)."""
    import torch
    n = size(P)
    B = O.num_blocks(n, P)
    with knobs(sw):
        for W in (3, 4):
            for rne in (False, True):
                x, q, e, _, dq = planes(P, W, O.RNE_VCL if rne else O.HALF_AWAY)
                for off in (0, 1):
                    d_x = up(torch, x, cuda, off)
                    for le in (False, True):
                        flags = (sw.FLAG_PAYLOAD_LE if le else 0) | (sw.FLAG_ROUND_RNE if rne else 0)
                        want_q = O.bswap32(q) if le else q
                        for nt in NT:
                            for sl in (2, 4):
                                sw.set_payload_nt_threshold(nt)
                                sw.set_stream_tile_slices(sl)
                                out = torch.zeros(n + 4, device=cuda)[off:off + n]
                                d_q = torch.zeros(B * P, dtype=torch.int32, device=cuda)
                                d_e = torch.zeros(B, dtype=torch.int8, device=cuda)
                                sw.roundtrip_loopback(d_x, P, W, out=out, payload=d_q, exps_out=d_e, flags=flags)
                                tag = (W, rne, off, le, nt, sl)
                                assert np.array_equal(words(d_q), want_q), tag
                                assert np.array_equal(d_e.cpu().numpy(), e), tag
                                assert np.array_equal(words(out), dq.view(np.uint32)), tag


@pytest.mark.parametrize("P", PACKETS)
def test_roundtrip_loopback_batch_axes(sw, cuda, P):
    """sml_roundtrip_loopback_batch, two slices (the second at a 4-byte
    offset): rounding x store policy, each slice against the oracle."""
    import torch
    n = size(P)
    with knobs(sw):
        for W in (3, 4):
            for rne in (False, True):
                rounding = O.RNE_VCL if rne else O.HALF_AWAY
                refs = [planes(P, W, rounding, seed) for seed in (0, 1)]
                ins = [up(torch, r[0], cuda, off) for off, r in enumerate(refs)]
                for nt in NT:
                    sw.set_payload_nt_threshold(nt)
                    outs = [torch.zeros(n + 4, device=cuda)[off:off + n] for off in (0, 1)]
                    sw.roundtrip_loopback_batch(list(zip(ins, outs)), P, W,
                                                flags=sw.FLAG_ROUND_RNE if rne else 0)
                    for i, (o, r) in enumerate(zip(outs, refs)):
                        assert np.array_equal(words(o), r[4].view(np.uint32)), (W, rne, nt, i)


@pytest.mark.parametrize("W", (3, 4))
@pytest.mark.parametrize("P", PACKETS)
def test_switch_aggregate_axes(sw, cuda, P, W):
    """sml_switch_aggregate: all three outputs with the fp32 bucket aligned /
    offset x BE / LE planes, W = 3 (division) / 4 (reciprocal), and the
    payload-only form per byte order."""
    import torch
    n = size(P)
    B = O.num_blocks(n, P)
    _, gexp, pls = worker_planes(W, n, P, seed=7 * P + W)
    exps = [np.maximum(gexp.astype(np.int16) - w, -128).astype(np.int8) for w in range(W)]
    agg, e, out = oracle_switch(pls, exps, n, P, W)
    d_ex = [up(torch, x, cuda) for x in exps]
    for le in (False, True):
        flags = sw.FLAG_PAYLOAD_LE if le else 0
        d_pl = [up(torch, (O.bswap32(p) if le else p).view(np.int32), cuda) for p in pls]
        want_agg = O.bswap32(agg) if le else agg
        for off in (0, 1):
            p_out = torch.zeros(B * P, dtype=torch.int32, device=cuda)
            e_out = torch.zeros(B, dtype=torch.int8, device=cuda)
            o = torch.zeros(n + 4, device=cuda)[off:off + n]
            sw.switch_aggregate(d_pl, d_ex, n, P, payload_out=p_out, exps_out=e_out, out=o, flags=flags)
            assert np.array_equal(words(p_out), want_agg), (le, off)
            assert np.array_equal(e_out.cpu().numpy(), e), (le, off)
            assert np.array_equal(words(o), out.view(np.uint32)), (le, off)
        p_out = torch.zeros(B * P, dtype=torch.int32, device=cuda)
        sw.switch_aggregate(d_pl, None, n, P, payload_out=p_out, flags=flags)
        assert np.array_equal(words(p_out), want_agg), le


# ------------------------------------------------------------- frames --

def frame_set(torch, nframes, stride, dev):
    return torch.full((nframes * stride,), 0xAB, dtype=torch.uint8, device=dev)


def assert_frames(frames, ref, nframes, stride, fb, tag):
    got = frames.cpu().numpy().reshape(nframes, stride)
    assert np.array_equal(got[:, :fb], ref.reshape(nframes, fb)), tag
    assert np.all(got[:, fb:] == 0xAB), tag                      # padding between frames untouched


@pytest.mark.parametrize("P", PACKETS)
def test_frames_tx_axes(sw, cuda, P):
    """sml_quantize_pack_frames into device frames: slice aligned / offset x
    global exponents or not x store policy."""
    import torch
    n, W, bm = size(P), 3, 4
    x = planes(P, W)[0]
    B = O.num_blocks(n, P)
    nframes, fb = B + min(B, bm), FW.frame_bytes(P)
    stride = fb + 12
    fp = sw.frame_params(job_id=7, pool_index_start=16, pool_index_shift=3, max_outstanding_pkts=bm)
    ge = np.clip(O.exponents(x, P).astype(np.int32) + 1, -128, 127).astype(np.int8)
    with knobs(sw):
        for glob in (False, True):
            ref = O.build_frames(x, fp, P=P, num_workers=W, batch_max=bm, global_exps=ge if glob else None)
            d_ge = up(torch, ge, cuda) if glob else None
            for off in (0, 1):
                d_x = up(torch, x, cuda, off)
                for nt in NT:
                    sw.set_payload_nt_threshold(nt)
                    frames = frame_set(torch, nframes, stride, cuda)
                    sw.quantize_pack_frames(d_x, fp, P, W, batch_max=bm, global_exps=d_ge, frames=frames,
                                            stride=stride)
                    assert_frames(frames, ref, nframes, stride, fb, (glob, off, nt))


@pytest.mark.parametrize("P", PACKETS)
def test_frames_tx_int32_axes(sw, cuda, P):
    """sml_pack_frames_int32 into device frames: slice aligned / offset x
    store policy."""
    import torch
    n = size(P)
    x = int32_data(P, n)
    B, fb = O.num_blocks(n, P), FW.frame_bytes(P)
    stride = fb + 12
    fp = sw.frame_params(job_id=9, pool_index_start=16, pool_index_shift=3, max_outstanding_pkts=32)
    ref = O.build_frames_i32(x, fp, P=P)
    with knobs(sw):
        for off in (0, 1):
            d_x = up(torch, x, cuda, off)
            for nt in NT:
                sw.set_payload_nt_threshold(nt)
                frames = frame_set(torch, B, stride, cuda)
                sw.pack_frames_int32(d_x, fp, P, frames=frames, stride=stride)
                assert_frames(frames, ref, B, stride, fb, (off, nt))


@pytest.mark.parametrize("P", PACKETS)
def test_frames_rx_axes(sw, cuda, P):
    """sml_dequantize_frames and sml_unpack_frames_int32 under both output
    store policies: a shuffled stream with duplicates, other jobs' frames and
    out-of-range pkt_ids against the oracle's receive loop."""
    import torch
    n, W, bm, job = size(P), 3, 4, 0x3C
    x = planes(P, W)[0]
    fstream, _ = rx_stream(x, P, W, bm, job_id=job, seed=P)
    ref = O.dequantize_frames(fstream, fstream.shape[0], fstream.shape[1], O.RxState(n, P, bm), W, job_id=job)
    xi = int32_data(P + 1, n)
    B, fb = O.num_blocks(n, P), FW.frame_bytes(P)
    istream = int32_stream(O.build_frames_i32(xi, sw.frame_params(job_id=7), P=P), B, fb, seed=P)
    iref = O.unpack_frames_i32(istream, istream.size // fb, fb, O.RxStateI32(n, P), job_id=7)
    assert np.array_equal(iref.out, xi)
    d_istream = up(torch, istream, cuda)
    with knobs(sw):
        for nt in NT:
            sw.set_payload_nt_threshold(nt)
            out, exps, counts = run_rx(torch, sw, fstream, P, W, bm, job, n, "device")
            assert np.array_equal(out.view(np.uint32), ref.out.view(np.uint32)), nt
            assert np.array_equal(exps, ref.exps), nt
            assert counts == ref.counts, nt
            rx = sw.RxSliceInt32(n, P, device=cuda)
            sw.unpack_frames_int32(d_istream, istream.size // fb, rx, job_id=7)
            assert np.array_equal(rx.out.cpu().numpy(), iref.out), nt
            assert rx.counts.cpu().tolist() == iref.counts, nt


# ------------------------------------------------------------- bursts --
#
# One burst of 5 packets of a slice with packet window b = 5, buffers in
# device memory.  Packet q >= b carries block q - b, packet q < B the exponent
# of block q; the ids cover packets that only carry an exponent (3, 4), full
# blocks (6, 7) and the slice's partial last block (B + 4), and never hold
# both q and q + b.  The oracle's packet loop (test_packets_gpu.py) has no
# rounding mode, so what a packet must hold is stated from the oracle's planes:
# the payload of block k is O.quantize(x, P, W, rounding)[k * P:][:n_k], its
# exponent O.exponents(x, P)[k].

BURST_B = 5


def burst_ids(B):
    return [3, 4, 6, 7, B + BURST_B - 1]


def real_words(n, P, k):
    return min(P, n - k * P)


class Burst:
    """The buffers of one burst on the device, as a worker's ring holds them
    before the call: packet q >= b with block q - b as sent, exponent bytes
    of the packets q < B, everything else recognisable filler."""

    def __init__(self, sw, torch, dev, P, W, rne, flags=0):
        self.P, self.W, self.n = P, W, size(P)
        self.x, self.q, self.e, self.agg, _ = planes(P, W, O.RNE_VCL if rne else O.HALF_AWAY)
        self.B = B = O.num_blocks(self.n, P)
        self.ids = burst_ids(B)
        ent = np.full((len(self.ids), P), SENT, dtype=np.uint32)
        ext = np.zeros((len(self.ids), 2), dtype=np.uint8)
        ext[:] = (0x77, 0x99)
        recv = self.e.copy()
        for i, p in enumerate(self.ids):
            if p >= BURST_B:
                ent[i] = self.q[(p - BURST_B) * P:(p - BURST_B + 1) * P]
            if p < B:
                ext[i, 0] = self.e[p].view(np.uint8)
                recv[p] = 0x11                                   # not received yet
        self.ent0, self.ext0, self.recv0 = ent, ext, recv
        self.d_x = up(torch, self.x, dev)
        self.d_out = up(torch, np.full(self.n, SENT, dtype=np.uint32).view(np.float32), dev)
        self.d_ent = up(torch, ent.view(np.int32).reshape(-1), dev)
        self.d_ext = up(torch, ext.reshape(-1), dev)
        self.d_recv = up(torch, recv, dev)
        self.burst = sw.packet_burst(
            self.d_x, self.d_out, P, W, BURST_B, self.d_recv, self.ids,
            [self.d_ent.data_ptr() + i * P * 4 for i in range(len(self.ids))],
            [self.d_ext.data_ptr() + i * 2 for i in range(len(self.ids))], flags=flags | (sw.FLAG_ROUND_RNE if rne else 0))
        torch.cuda.synchronize()

    def got(self):
        return (words(self.d_ent).reshape(len(self.ids), self.P), self.d_ext.cpu().numpy().reshape(len(self.ids), 2),
                self.d_recv.cpu().numpy(), words(self.d_out))


def check_preprocess(bt, tag):
    """After PreprocessSingle of every packet: q >= b holds block q - b
    quantized with the received exponent (its real words; the rest stale),
    q < B the exponent of block q in byte 0 of its extra slot."""
    ent, ext = bt.ent0.copy(), bt.ext0.copy()
    # the received exponents of the blocks being sent: recv0 holds them (blocks 1, 2, B - 1)
    for i, p in enumerate(bt.ids):
        if p >= BURST_B:
            k = p - BURST_B
            m = real_words(bt.n, bt.P, k)
            ent[i, :m] = bt.q[k * bt.P:k * bt.P + m]
        if p < bt.B:
            ext[i, 0] = bt.e[p].view(np.uint8)
    g_ent, g_ext, g_recv, g_out = bt.got()
    assert np.array_equal(g_ent, ent), tag
    assert np.array_equal(g_ext, ext), tag
    assert np.array_equal(g_recv, bt.recv0), tag
    assert np.all(g_out == SENT), tag


def stale_payloads(bt, torch):
    """Overwrite the real words of the payload packets, so that the
    preprocess has to write them."""
    ent = bt.ent0.copy()
    for i, p in enumerate(bt.ids):
        if p >= BURST_B:
            ent[i, :real_words(bt.n, bt.P, p - BURST_B)] = SENT
    bt.d_ent.copy_(torch.from_numpy(ent.view(np.int32).reshape(-1)))
    for i, p in enumerate(bt.ids):
        if p < bt.B:
            bt.d_ext[2 * i] = 0x77
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", PACKETS)
def test_preprocess_burst_axes(sw, cuda, P):
    """sml_preprocess_burst: rounding half-away / RNE."""
    import torch
    for rne in (False, True):
        bt = Burst(sw, torch, cuda, P, 3, rne)
        stale_payloads(bt, torch)
        sw.preprocess_burst(bt.burst)
        check_preprocess(bt, rne)


@pytest.mark.parametrize("P", PACKETS)
def test_burst_server_axes(sw, cuda, P):
    """The persistent burst server's kernel per rounding mode: the same
    preprocess burst, submitted through the doorbell."""
    import torch
    for rne in (False, True):
        bt = Burst(sw, torch, cuda, P, 3, rne)
        stale_payloads(bt, torch)
        srv = sw.BurstServer(P, flags=sw.FLAG_ROUND_RNE if rne else 0)
        try:
            srv.submit(sw.BURST_PRE, bt.burst)
        finally:
            srv.close()
        check_preprocess(bt, rne)


@pytest.mark.parametrize("P", PACKETS)
def test_exchange_burst_axes(sw, cuda, P):
    """sml_exchange_burst: rounding x FLAG_PROCESS_PACKET.  Per received
    packet q: block q - b dequantized into the output (after the x W of
    ProcessPacket when asked), the packet's exponent kept for block q, block
    q quantized with it into the same buffer (a partial block's tail and a
    packet without a next one keep the words ProcessPacket left), and the
    exponent of block q + b in the extra slot."""
    import torch
    W = 3
    for rne in (False, True):
        for proc in (False, True):
            bt = Burst(sw, torch, cuda, P, W, rne, flags=sw.FLAG_PROCESS_PACKET if proc else 0)
            n, B = bt.n, bt.B
            sw.exchange_burst(bt.burst)
            plane = bt.agg if proc else bt.q                     # the words PostprocessSingle sees
            dq = O.dequantize(plane, bt.e, n, P, W).view(np.uint32)
            ent = O.bswap32((O.bswap32(bt.ent0).astype(np.uint64) * W % (1 << 32)).astype(np.uint32)).reshape(
                bt.ent0.shape) if proc else bt.ent0.copy()
            ext, recv = bt.ext0.copy(), bt.recv0.copy()
            out = np.full(n, SENT, dtype=np.uint32)
            for i, p in enumerate(bt.ids):
                if p >= BURST_B:
                    k = p - BURST_B
                    m = real_words(n, P, k)
                    out[k * P:k * P + m] = dq[k * P:k * P + m]
                if p < B:
                    recv[p] = bt.e[p]
                    m = real_words(n, P, p)
                    ent[i, :m] = bt.q[p * P:p * P + m]
                if p + BURST_B < B:
                    ext[i, 0] = bt.e[p + BURST_B].view(np.uint8)
            g_ent, g_ext, g_recv, g_out = bt.got()
            tag = (rne, proc)
            assert np.array_equal(g_out, out), tag
            assert np.array_equal(g_recv, recv), tag
            assert np.array_equal(g_ent, ent), tag
            assert np.array_equal(g_ext, ext), tag
