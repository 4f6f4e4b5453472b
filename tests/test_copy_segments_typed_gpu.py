"""sml_copy_segments_typed on the GPU: the in-node switch's multicast of a
FLOAT16 / BFLOAT16 slice.  A 16-bit shard ends on an odd element and lands in
a tensor slice that starts at any element, so sources and destinations are
2-byte aligned only, each on its own; nothing outside a segment may be read
or written."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

# 40 000 elements span more than two groups of kSegGroup = 16 tiles of 1024
# elements (8 bytes per lane per slice), so the deal over the segments wraps;
# 33 001 ends in a partial tile after full ones; 16 385 is one group and one
# element of the next.
COUNTS = [40_000, 33_001, 1, 0, 16_385]
OFFSETS = (0, 1, 3, 7)
GUARD = 64
SENTINEL = 0x5A5A


def _layout(counts, offs):
    """Start of every segment in one buffer: a 64-element guard, the offset,
    the segment, a guard, rounded up so every region starts 128-byte aligned."""
    starts, pos = [], 0
    for n, o in zip(counts, offs):
        starts.append(pos + GUARD + o)
        pos += (GUARD + o + n + GUARD + 63) // 64 * 64
    return starts, pos


@pytest.mark.parametrize("peer", [False, True], ids=["plain", "peer-planes"])
@pytest.mark.parametrize("typ", ["fp16", "bf16"])
def test_copy_pins(cuda, typ, peer):
    """Every (source offset, destination offset) pair of {0, 1, 3, 7}^2 on
    every segment size: destinations equal sources, every guard element and
    every source is untouched, with and without SML_FLAG_PEER_PLANES."""
    import torch
    import switchml_amd as sw
    dtype = torch.float16 if typ == "fp16" else torch.bfloat16
    flags = sw.FLAG_PEER_PLANES if peer else 0
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    for a in range(4):
        for b in range(4):
            so = [OFFSETS[(a + i) % 4] for i in range(len(COUNTS))]
            do = [OFFSETS[(b + i) % 4] for i in range(len(COUNTS))]
            ss, stotal = _layout(COUNTS, so)
            ds, dtotal = _layout(COUNTS, do)
            src = torch.randint(-2 ** 15, 2 ** 15 - 1, (stotal,), dtype=torch.int16, device="cuda", generator=g)
            src_before = src.clone()
            dst = torch.full((dtotal,), SENTINEL, dtype=torch.int16, device="cuda")
            want = dst.clone()
            pairs = []
            for n, s0, d0 in zip(COUNTS, ss, ds):
                assert (src.data_ptr() + 2 * s0) % 16 == 2 * so[len(pairs)] % 16     # the offsets are what they say
                pairs.append((src[s0:s0 + n].view(dtype), dst[d0:d0 + n].view(dtype)))
                want[d0:d0 + n] = src_before[s0:s0 + n]
            sw.copy_segments_typed(pairs, flags=flags)
            torch.cuda.synchronize()
            assert torch.equal(dst, want), (so, do)            # segments copied, guards and gaps untouched
            assert torch.equal(src, src_before), (so, do)


def test_forwarding_and_errors(cuda):
    import torch
    import switchml_amd as sw
    L = sw.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    sizes, offs = [16384 * 3 + 5, 0, 1, 17, 33], [1, 0, 2, 3, 1]
    for dtype in (torch.float32, torch.int32):
        total = sum(n + o for n, o in zip(sizes, offs)) + 64
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (total,), dtype=torch.int32, device="cuda", generator=g)
        got = torch.full((total,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ref = got.clone()
        typed, plain, pos = [], [], 0
        for n, o in zip(sizes, offs):
            pos += o
            typed.append((src[pos:pos + n].view(dtype), got[pos:pos + n].view(dtype)))
            plain.append((src[pos:pos + n], ref[pos:pos + n]))
            pos += n
        sw.copy_segments_typed(typed)
        sw.copy_segments(plain)
        torch.cuda.synchronize()
        assert torch.equal(got, ref) and not torch.equal(got, torch.full_like(got, 0x5A5A5A5A))

    buf = torch.zeros(256, dtype=torch.int16, device="cuda")
    out = torch.full((256,), SENTINEL, dtype=torch.int16, device="cuda")

    def call(src_ptr, dst_ptr, n, dt):
        s = (ctypes.c_void_p * 1)(src_ptr)
        d = (ctypes.c_void_p * 1)(dst_ptr)
        c = (ctypes.c_uint64 * 1)(n)
        return L.sml_copy_segments_typed(ctypes.cast(s, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p),
                                         ctypes.cast(c, ctypes.c_void_p), 1, dt, 0, None)

    for dt in (sw.FLOAT16, sw.BFLOAT16):
        assert call(buf.data_ptr() + 1, out.data_ptr(), 16, dt) == sw.SML_ERR_INVALID_ARG      # odd source
        assert call(buf.data_ptr(), out.data_ptr() + 1, 16, dt) == sw.SML_ERR_INVALID_ARG      # odd destination
        assert call(buf.data_ptr() + 1, out.data_ptr() + 1, 0, dt) == sw.SML_OK                # all empty
    assert call(buf.data_ptr(), out.data_ptr(), 16, 4) == sw.SML_ERR_UNSUPPORTED               # no such type
    sw.copy_segments_typed([])                                                                 # no segments
    sw.copy_segments_typed([(buf[:0].view(torch.bfloat16), out[:0].view(torch.bfloat16))])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                                       # nothing was launched
    with pytest.raises(TypeError):
        sw.copy_segments_typed([(buf[:4].view(torch.float16), out[:4].view(torch.bfloat16))])
