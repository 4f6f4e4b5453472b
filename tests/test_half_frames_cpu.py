"""CPU tests of the FLOAT16 / BFLOAT16 DPDK frame entry points (no GPU
needed): sml_quantize_pack_frames_typed and sml_dequantize_frames_typed exist,
are declared, and make every argument check before they touch the device."""
import ctypes

import pytest

from switchml_amd import frame_wire as FW

F32, I32, F16, BF16 = 0, 1, 2, 3
TYPED = ("sml_quantize_pack_frames_typed", "sml_dequantize_frames_typed")


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def test_typed_frame_symbols_exported_and_declared(sw):
    L = sw.lib()
    assert [s for s in TYPED if not hasattr(L, s)] == []
    assert set(TYPED) <= set(sw.header_symbols())
    assert L.sml_abi_version() == 2          # symbols were added, nothing changed


class Mem:
    """Host memory standing in for the device buffers: no check reads it."""

    def __init__(self):
        self.backing = (ctypes.c_uint8 * 16384)()
        base = (ctypes.addressof(self.backing) + 63) & ~63
        self.buf, self.frames, self.state, self.exps, self.counts = base, base + 1024, base + 8192, base + 12288, base + 12800


@pytest.mark.parametrize("dt", [F16, BF16])
def test_tx_typed_validation_without_gpu(sw, dt):
    L, m = sw.lib(), Mem()
    prm = sw.frame_params(job_id=3)
    n, P, W, bm = 16, 256, 2, 4
    stride = FW.frame_bytes(P)

    def call(buf, dt, n, P, W, bm, frames=m.frames, stride=stride, prm=prm):
        return L.sml_quantize_pack_frames_typed(buf, dt, n, P, W, None, bm, ctypes.byref(prm) if prm else None,
                                                frames, stride, None)

    assert call(m.buf, dt, n, 100, W, bm) == sw.SML_ERR_UNSUPPORTED           # bad P
    assert call(m.buf, I32, n, P, W, bm) == sw.SML_ERR_UNSUPPORTED            # INT32 is not a float slice
    assert call(m.buf, 4, n, P, W, bm) == sw.SML_ERR_UNSUPPORTED              # no such type
    assert call(m.buf, dt, n, P, 0, bm) == sw.SML_ERR_INVALID_ARG             # W = 0
    assert call(m.buf, dt, n, P, W, 0) == sw.SML_ERR_INVALID_ARG              # batch_max = 0
    assert call(m.buf, dt, n, P, W, bm, prm=None) == sw.SML_ERR_INVALID_ARG
    assert call(m.buf, dt, 0, P, W, bm) == sw.SML_OK                          # nothing to do
    assert call(None, dt, 0, P, W, bm, frames=None) == sw.SML_OK
    assert call(None, dt, n, P, W, bm) == sw.SML_ERR_INVALID_ARG
    # an odd 16-bit pointer: what the fp32 entry point gives a pointer that is not 4-byte aligned
    fp32_misaligned = L.sml_quantize_pack_frames(m.buf + 2, n, P, W, None, bm, ctypes.byref(prm), m.frames, stride,
                                                 None)
    assert fp32_misaligned == sw.SML_ERR_INVALID_ARG
    assert call(m.buf + 1, dt, n, P, W, bm) == fp32_misaligned
    assert call(m.buf + 1, F32, n, P, W, bm) == fp32_misaligned               # FLOAT32 through the typed entry point
    # a 2-byte aligned 16-bit buffer passes: the next check that fails is the frame set's
    assert call(m.buf + 2, dt, n, P, W, bm, frames=m.frames + 2) == sw.SML_ERR_ALIGNMENT
    assert call(m.buf + 2, dt, n, P, W, bm, stride=stride - 4) == sw.SML_ERR_ALIGNMENT
    assert call(m.buf + 2, dt, n, P, W, bm, frames=None) == sw.SML_ERR_INVALID_ARG
    # two checks fail at once: the earlier one decides
    assert call(m.buf, I32, n, 100, 0, bm) == sw.SML_ERR_UNSUPPORTED
    assert call(m.buf, I32, n, P, 0, bm) == sw.SML_ERR_UNSUPPORTED            # the type before W = 0
    assert call(m.buf + 1, dt, n, P, W, bm, frames=m.frames + 2) == sw.SML_ERR_INVALID_ARG
    assert call(None, dt, 0, P, 0, bm) == sw.SML_ERR_INVALID_ARG              # W = 0 before nothing-to-do


@pytest.mark.parametrize("dt", [F16, BF16])
def test_rx_typed_validation_without_gpu(sw, dt):
    L, m = sw.lib(), Mem()
    n, P, W, bm, F = 16, 256, 2, 4, 2
    stride = FW.frame_bytes(P)

    def call(out, dt, F, P, W, bm, frames=m.frames, stride=stride, state=m.state, exps=m.exps, counts=m.counts, n=n):
        return L.sml_dequantize_frames_typed(frames, F, stride, n, P, W, bm, 7, exps, state, out, dt, counts, None)

    assert call(m.buf, dt, F, 100, W, bm) == sw.SML_ERR_UNSUPPORTED           # bad P
    assert call(m.buf, I32, F, P, W, bm) == sw.SML_ERR_UNSUPPORTED            # INT32 is not a float slice
    assert call(m.buf, 4, F, P, W, bm) == sw.SML_ERR_UNSUPPORTED              # no such type
    assert call(m.buf, dt, F, P, 0, bm) == sw.SML_ERR_INVALID_ARG             # W = 0
    assert call(m.buf, dt, F, P, W, 0) == sw.SML_ERR_INVALID_ARG              # batch_max = 0
    assert call(m.buf, dt, 0, P, W, bm) == sw.SML_OK                          # no frames: nothing to do
    assert call(None, dt, 0, P, W, bm, frames=None, state=None, exps=None, counts=None) == sw.SML_OK
    assert call(m.buf, dt, 0xFFFFFFFE, P, W, bm) == sw.SML_ERR_UNSUPPORTED    # more frames than a claim tag counts
    assert call(None, dt, F, P, W, bm) == sw.SML_ERR_INVALID_ARG
    assert call(m.buf, dt, F, P, W, bm, state=None) == sw.SML_ERR_INVALID_ARG
    assert call(m.buf, dt, F, P, W, bm, exps=None) == sw.SML_ERR_INVALID_ARG
    assert call(m.buf, dt, F, P, W, bm, frames=None) == sw.SML_ERR_INVALID_ARG
    assert call(m.buf, dt, F, P, W, bm, frames=m.frames + 2) == sw.SML_ERR_ALIGNMENT
    # an odd 16-bit pointer: what the fp32 entry point gives a pointer that is not 4-byte aligned
    fp32_misaligned = L.sml_dequantize_frames(m.frames, F, stride, n, P, W, bm, 7, m.exps, m.state, m.buf + 2,
                                              m.counts, None)
    assert fp32_misaligned == sw.SML_ERR_ALIGNMENT
    assert call(m.buf + 1, dt, F, P, W, bm) == fp32_misaligned
    assert call(m.buf + 2, F32, F, P, W, bm) == fp32_misaligned               # FLOAT32 through the typed entry point
    # a 2-byte aligned 16-bit buffer passes: the next check that fails is the state's alignment
    assert call(m.buf + 2, dt, F, P, W, bm, state=m.state + 4) == sw.SML_ERR_ALIGNMENT
    assert call(m.buf + 2, dt, F, P, W, bm, counts=m.counts + 4) == sw.SML_ERR_ALIGNMENT
    # two checks fail at once: the earlier one decides
    assert call(m.buf, I32, F, P, 0, bm) == sw.SML_ERR_UNSUPPORTED            # the type before W = 0
    assert call(None, dt, 0, P, 0, bm) == sw.SML_ERR_INVALID_ARG              # W = 0 before nothing-to-do
    assert call(None, dt, F, P, W, bm, frames=m.frames + 2) == sw.SML_ERR_INVALID_ARG


def test_rx_state_words_know_no_element_type(sw):
    """A 16-bit slice's rx state is the FLOAT32 one: per pkt_id, B + b words."""
    L = sw.lib()
    assert L.sml_rx_state_words(4113, 256, 64, 0) == 17 + 17
    assert L.sml_rx_state_words(9000, 1024, 2, 0) == 9 + 2
    assert L.sml_rx_reset(None, 0, None) == sw.SML_OK
