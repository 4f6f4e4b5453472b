"""A typed entry point given SML_FLOAT32 is its fp32 twin on the device: the
same bits out of both, for the nine pairs of include/switchml_hip.h.  The
Python wrappers launch through the typed entry points only, so this is also
what keeps the fp32 entry points covered on the GPU.

Both entries are called straight through lib() on the same seeded fp32 input,
each into outputs of its own that start from the same sentinel, and every
output is compared bit for bit (torch.equal on integer views).  The shapes
are the smallest at which the dispatch can differ: every packet size class,
a partial packet and a partial tile, W = 3 (no reciprocal), the input and
output at element offset 0 (16-byte aligned form) and 1 (unaligned form),
both payload byte orders, and SML_FLAG_ROUND_RNE once."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

F32 = 0
PACKETS = (64, 256, 1024)
SENT = 0x5A5A5A5A


def sizes(P):
    return (1, P - 1, P + 1, 2 * 1024 + 5)


def cases(sw):
    """(W, element offset, flags): both byte orders everywhere, RNE once."""
    for W in (1, 3):
        for off in (0, 1):
            for flags in (0, sw.FLAG_PAYLOAD_LE):
                yield W, off, flags
    yield 3, 1, sw.FLAG_ROUND_RNE


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def table(tensors):
    return ctypes.cast((ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), ctypes.c_void_p)


@pytest.fixture(scope="module")
def env(cuda):
    """(switchml_amd, torch, the seeded fp32 source: magnitudes over 2^-12..2^12)."""
    import torch
    import switchml_amd as sw
    g = torch.Generator(device="cuda")
    g.manual_seed(20)
    n = 16 * 1024 + 64
    src = torch.randn(n, device=cuda, generator=g) * torch.exp2(
        torch.randint(-12, 13, (n,), device=cuda, generator=g).float())
    assert src.data_ptr() % 16 == 0
    return sw, torch, src


def sentinel(torch, n, dtype, off=0):
    """n elements at element offset `off` of a fresh buffer filled with the
    sentinel, and that buffer (the guard elements around the view included)."""
    buf = torch.full((n + off + 4,), SENT, dtype=torch.int32, device="cuda").view(dtype)
    return buf[off:off + n], buf


def same(torch, a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("P", PACKETS)
def test_plane_entry_points(env, P):
    """exponents, quantize_pack, dequantize, roundtrip_loopback."""
    sw, torch, src = env
    L = sw.lib()
    for numel in sizes(P):
        B = sw.num_blocks(numel, P)
        for W, off, flags in cases(sw):
            x = src[off:off + numel]
            tag = (P, numel, W, off, flags)
            # [0]: the fp32 entry point's outputs, [1]: the typed one's
            exps = [sentinel(torch, B, torch.int8) for _ in range(2)]
            assert L.sml_exponents(ptr(x), numel, P, ptr(exps[0][0]), None) == 0
            assert L.sml_exponents_typed(ptr(x), F32, numel, P, ptr(exps[1][0]), None) == 0
            pay = [sentinel(torch, B * P, torch.int32) for _ in range(2)]
            qex = [sentinel(torch, B, torch.int8) for _ in range(2)]
            assert L.sml_quantize_pack(ptr(x), numel, P, W, None, ptr(pay[0][0]), ptr(qex[0][0]), flags, None) == 0
            assert L.sml_quantize_pack_typed(ptr(x), F32, numel, P, W, None, ptr(pay[1][0]), ptr(qex[1][0]), flags,
                                             None) == 0
            out = [sentinel(torch, numel, torch.float32, off) for _ in range(2)]
            assert L.sml_dequantize(ptr(pay[0][0]), ptr(qex[0][0]), numel, P, W, ptr(out[0][0]), flags, None) == 0
            assert L.sml_dequantize_typed(ptr(pay[0][0]), ptr(qex[0][0]), numel, P, W, ptr(out[1][0]), F32, flags,
                                          None) == 0
            rout = [sentinel(torch, numel, torch.float32, off) for _ in range(2)]
            rpay = [sentinel(torch, B * P, torch.int32) for _ in range(2)]
            rex = [sentinel(torch, B, torch.int8) for _ in range(2)]
            assert L.sml_roundtrip_loopback(ptr(x), ptr(rout[0][0]), numel, P, W, ptr(rpay[0][0]), ptr(rex[0][0]),
                                            flags, None) == 0
            assert L.sml_roundtrip_loopback_typed(ptr(x), ptr(rout[1][0]), F32, numel, P, W, ptr(rpay[1][0]),
                                                  ptr(rex[1][0]), flags, None) == 0
            torch.cuda.synchronize()
            for name, pair in (("exponents", exps), ("payload", pay), ("quantize exps", qex), ("dequantize", out),
                               ("roundtrip", rout), ("roundtrip payload", rpay), ("roundtrip exps", rex)):
                assert same(torch, pair[0][1], pair[1][1]), (name, tag)
            # the outputs were written at all
            for name, pair in (("payload", pay), ("dequantize", out), ("roundtrip", rout), ("roundtrip payload", rpay)):
                assert not bool((pair[1][0][:numel].view(torch.int32) == SENT).any()), (name, tag)


@pytest.mark.parametrize("P", PACKETS)
def test_switch_aggregate(env, P):
    """W planes of any words (the sum wraps) and exponents -16..16 into all
    three outputs; W = 3 takes the form without the reciprocal."""
    sw, torch, src = env
    L = sw.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    for numel in sizes(P):
        B = sw.num_blocks(numel, P)
        for W, off, flags in cases(sw):
            planes = [torch.randint(-2 ** 31, 2 ** 31 - 1, (B * P,), dtype=torch.int32, device="cuda", generator=g)
                      for _ in range(W)]
            eplanes = [torch.randint(-16, 17, (B,), dtype=torch.int8, device="cuda", generator=g) for _ in range(W)]
            pout = [sentinel(torch, B * P, torch.int32) for _ in range(2)]
            eout = [sentinel(torch, B, torch.int8) for _ in range(2)]
            out = [sentinel(torch, numel, torch.float32, off) for _ in range(2)]
            assert L.sml_switch_aggregate(table(planes), table(eplanes), W, numel, P, ptr(pout[0][0]),
                                          ptr(eout[0][0]), ptr(out[0][0]), flags, None) == 0
            assert L.sml_switch_aggregate_typed(table(planes), table(eplanes), W, numel, P, ptr(pout[1][0]),
                                                ptr(eout[1][0]), ptr(out[1][0]), F32, flags, None) == 0
            torch.cuda.synchronize()
            for name, pair in (("payload", pout), ("exps", eout), ("bucket", out)):
                assert same(torch, pair[0][1], pair[1][1]), (name, P, numel, W, off, flags)
            assert torch.equal(eout[1][0], torch.stack(eplanes).max(0).values)     # written at all


@pytest.mark.parametrize("P", PACKETS)
def test_roundtrip_batch(env, P):
    """3 slices, one of them empty, at element offsets that leave the second
    one unaligned: one table of sml_slice, one of sml_typed_slice."""
    sw, torch, src = env
    L = sw.lib()
    for numel in sizes(P):
        for W, off, flags in cases(sw):
            lens = (numel, 0, P + 1)
            starts = (off, off + numel, off + numel + 1)
            outs = []
            for typed in (False, True):
                view, buf = sentinel(torch, sum(lens) + 1, torch.float32, off)
                if typed:
                    arr = (sw.TypedSlice * 3)(*[sw.TypedSlice(src[s:].data_ptr(), view[s - off:].data_ptr(), n, F32, 0)
                                                for s, n in zip(starts, lens)])
                    assert L.sml_roundtrip_loopback_batch_typed(arr, 3, P, W, flags, None) == 0
                else:
                    arr = (sw.Slice * 3)(*[sw.Slice(src[s:].data_ptr(), view[s - off:].data_ptr(), n)
                                           for s, n in zip(starts, lens)])
                    assert L.sml_roundtrip_loopback_batch(arr, 3, P, W, flags, None) == 0
                outs.append((view, buf))
            torch.cuda.synchronize()
            assert same(torch, outs[0][1], outs[1][1]), (P, numel, W, off, flags)
            # slice 0 is the single-slice round trip of its own elements
            one, _ = sentinel(torch, numel, torch.float32, off)
            assert L.sml_roundtrip_loopback(ptr(src[off:]), ptr(one), numel, P, W, None, None,
                                            flags & sw.FLAG_ROUND_RNE, None) == 0
            torch.cuda.synchronize()
            assert same(torch, outs[1][0][:numel], one), (P, numel, W, off, flags)


@pytest.mark.parametrize("peer", [False, True], ids=["plain", "peer-planes"])
def test_copy_segments(env, peer):
    """Segments of 0, 5 and 16 * 1024 + 3 words: one group is 16 tiles of
    1024 words, so the last segment crosses into a second group."""
    sw, torch, src = env
    L = sw.lib()
    flags = sw.FLAG_PEER_PLANES if peer else 0
    lens = (0, 5, 16 * 1024 + 3)
    starts = (0, 1, 8)                       # sources at 4-byte offsets of their own
    words = src.view(torch.int32)
    srcs = [words[s:s + n] for s, n in zip(starts, lens)]
    counts = ctypes.cast((ctypes.c_uint64 * 3)(*lens), ctypes.c_void_p)
    bufs = []
    for typed in (False, True):
        view, buf = sentinel(torch, sum(lens) + 2, torch.int32, 1)
        dsts, pos = [], 0
        for n in lens:
            dsts.append(view[pos:pos + n])
            pos += n + 1                      # a guard word between segments
        if typed:
            assert L.sml_copy_segments_typed(table(srcs), table(dsts), counts, 3, F32, flags, None) == 0
        else:
            assert L.sml_copy_segments(table(srcs), table(dsts), counts, 3, flags, None) == 0
        bufs.append((buf, dsts))
    torch.cuda.synchronize()
    assert torch.equal(bufs[0][0], bufs[1][0])
    for s, d in zip(srcs, bufs[1][1]):
        assert torch.equal(s, d)
    assert int((bufs[1][0] == SENT).sum()) == bufs[1][0].numel() - sum(lens)      # guards untouched


@pytest.mark.parametrize("P", PACKETS)
def test_frames(env, P):
    """numel = 2P + 3 (B = 3) with batch_max = 2 (5 frames); the receive side
    is fed the frame set in two calls (2 frames, then 3)."""
    sw, torch, src = env
    L = sw.lib()
    numel, bm, job = 2 * P + 3, 2, 9
    F, stride = 3 + 2, sw.frame_bytes(P)
    prm = sw.frame_params(job_id=job, pool_index_start=16, pool_index_shift=3, max_outstanding_pkts=8)
    for W in (1, 3):
        for off in (0, 1):
            x = src[off:off + numel]
            fr = [torch.full((F * stride,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
            assert L.sml_quantize_pack_frames(ptr(x), numel, P, W, None, bm, ctypes.byref(prm), ptr(fr[0]), stride,
                                              None) == 0
            assert L.sml_quantize_pack_frames_typed(ptr(x), F32, numel, P, W, None, bm, ctypes.byref(prm),
                                                    ptr(fr[1]), stride, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(fr[0], fr[1]), (P, W, off)
            rxs, bufs = [], []
            for typed in (False, True):
                out, buf = sentinel(torch, numel, torch.float32, off)
                rx = sw.RxSlice(numel, P, bm, device="cuda", out=out)
                for first, count in ((0, 2), (2, 3)):
                    head = (ptr(fr[0][first * stride:]), count, stride, numel, P, W, bm, job, ptr(rx.exps),
                            ptr(rx.state), ptr(out))
                    if typed:
                        assert L.sml_dequantize_frames_typed(*head, F32, ptr(rx.counts), None) == 0
                    else:
                        assert L.sml_dequantize_frames(*head, ptr(rx.counts), None) == 0
                rxs.append(rx)
                bufs.append(buf)
            torch.cuda.synchronize()
            assert same(torch, bufs[0], bufs[1]), (P, W, off)
            assert torch.equal(rxs[0].exps, rxs[1].exps) and torch.equal(rxs[0].state, rxs[1].state), (P, W, off)
            assert torch.equal(rxs[0].counts, rxs[1].counts), (P, W, off)
            assert rxs[1].counts.tolist() == [F, 0], (P, W, off)                # every frame was taken
