"""CPU tests of FLOAT16 / BFLOAT16 jobs through the in-node switch (no GPU
needed): the opt-in key backend.xgmi.half_types reaches the configuration
text, and sml_copy_segments_typed (the multicast of 2-byte elements) is
exported, declared, and checks its arguments before any HIP call."""
import ctypes

import pytest

F32, I32, F16, BF16 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def test_make_config_writes_half_types_under_backend_xgmi():
    from switchml_amd import client as C
    text = C.make_config(backend="xgmi", session="s", half_types=True)
    section = text.split("[backend.xgmi]\n")[1]
    assert "half_types = true\n" in section and "session = s\n" in section
    assert "half_types" not in text.split("[backend.xgmi]\n")[0]
    assert "half_types = false\n" in C.make_config(backend="xgmi", session="s", half_types=False)
    assert "half_types" not in C.make_config(backend="xgmi", session="s")      # the default stays unwritten


def test_half_types_is_parsed_and_printed():
    """The key round-trips through Config (LoadFromString / ToString) and
    defaults to false; a dummy-backend context with the bypass PPP touches no
    GPU."""
    from switchml_amd import client as C
    if C.state() == C.RUNNING:
        C.stop()
    try:
        for kw, line in ((dict(half_types=True), "half_types = true"), ({}, "half_types = false")):
            C.start(C.make_config(prepostprocessor="bypass", bandwidth=0, **kw))
            section = C.config_text().split("[backend.xgmi]\n")[1]
            assert line + "\n" in section, section
            C.stop()
    finally:
        if C.state() == C.RUNNING:
            C.stop()


def test_copy_segments_typed_exported_and_declared(sw):
    assert hasattr(sw.lib(), "sml_copy_segments_typed")
    assert "sml_copy_segments_typed" in sw.header_symbols()
    assert sw.lib().sml_abi_version() == 2          # a symbol was added, nothing changed
    assert callable(sw.copy_segments_typed)


def _tables(srcs, dsts, counts):
    k = len(srcs)
    s = (ctypes.c_void_p * max(1, k))(*srcs)
    d = (ctypes.c_void_p * max(1, k))(*dsts)
    n = (ctypes.c_uint64 * max(1, k))(*counts)
    return ctypes.cast(s, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p), ctypes.cast(n, ctypes.c_void_p), (s, d, n)


@pytest.mark.parametrize("dt", [F16, BF16])
def test_copy_segments_typed_validation_without_gpu(sw, dt):
    """Every check returns before a HIP call, so no device is needed."""
    call = sw.lib().sml_copy_segments_typed
    backing = (ctypes.c_uint8 * 4096)()
    base = (ctypes.addressof(backing) + 63) & ~63
    src, dst = base, base + 2048
    s, d, n, keep = _tables([src], [dst], [16])
    assert call(s, d, n, 1, 4, 0, None) == sw.SML_ERR_UNSUPPORTED                 # no such type
    assert call(s, d, n, 1, -1, 0, None) == sw.SML_ERR_UNSUPPORTED
    assert call(None, None, None, 1, 4, 0, None) == sw.SML_ERR_UNSUPPORTED        # the type is checked first
    assert call(None, d, n, 1, dt, 0, None) == sw.SML_ERR_INVALID_ARG             # null tables
    assert call(s, None, n, 1, dt, 0, None) == sw.SML_ERR_INVALID_ARG
    assert call(s, d, None, 1, dt, 0, None) == sw.SML_ERR_INVALID_ARG
    assert call(s, d, n, 17, dt, 0, None) == sw.SML_ERR_INVALID_ARG               # more than SML_MAX_SWITCH_WORKERS
    assert call(None, None, None, 0, dt, 0, None) == sw.SML_OK                    # no segments: nothing to do
    for srcs, dsts in (([src + 1], [dst]), ([src], [dst + 1]), ([None], [dst]), ([src], [None])):
        s1, d1, n1, keep1 = _tables(srcs, dsts, [16])
        assert call(s1, d1, n1, 1, dt, 0, None) == sw.SML_ERR_INVALID_ARG         # odd or null pointer, n > 0
    # an empty segment's pointers are not looked at; an all-empty call is SML_OK
    s0, d0, n0, keep0 = _tables([src + 1, None], [None, dst + 1], [0, 0])
    assert call(s0, d0, n0, 2, dt, 0, None) == sw.SML_OK
    # a bad segment after a good one still fails before anything is launched
    s2, d2, n2, keep2 = _tables([src, src + 513], [dst, dst + 512], [16, 16])
    assert call(s2, d2, n2, 2, dt, 0, None) == sw.SML_ERR_INVALID_ARG


def test_copy_segments_typed_forwards_32_bit_types_to_the_untyped_checks(sw):
    """SML_FLOAT32 / SML_INT32 take sml_copy_segments' checks: 4-byte alignment."""
    call = sw.lib().sml_copy_segments_typed
    backing = (ctypes.c_uint8 * 4096)()
    base = (ctypes.addressof(backing) + 63) & ~63
    s, d, n, keep = _tables([base + 2], [base + 2048], [16])
    for dt in (F32, I32):
        assert call(s, d, n, 1, dt, 0, None) == sw.SML_ERR_INVALID_ARG            # 2-byte aligned only
        assert call(s, d, n, 17, dt, 0, None) == sw.SML_ERR_INVALID_ARG
        assert call(None, None, None, 0, dt, 0, None) == sw.SML_OK
