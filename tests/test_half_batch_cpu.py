"""CPU tests of the typed batched round trip (no GPU needed):
sml_roundtrip_loopback_batch_typed and sml_context_batch_stats exist, and the
batch entry point checks every slice of its table before any HIP call."""
import ctypes

import numpy as np
import pytest

F32, I32, F16, BF16 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def test_symbols_exported_and_declared(sw):
    from switchml_amd import client as C
    L = sw.lib()
    assert hasattr(L, "sml_roundtrip_loopback_batch_typed") and hasattr(L, "sml_context_batch_stats")
    assert "sml_roundtrip_loopback_batch_typed" in sw.header_symbols()
    assert L.sml_abi_version() == 2          # symbols were added, nothing changed
    assert sw.MAX_BATCH_SLICES == 64
    assert ctypes.sizeof(sw.TypedSlice) == 32 and ctypes.sizeof(sw.Slice) == 24
    assert callable(C.batch_stats)


def table(sw, rows):
    arr = (sw.TypedSlice * max(1, len(rows)))()
    for i, r in enumerate(rows):
        arr[i] = sw.TypedSlice(*r)
    return arr


@pytest.fixture(scope="module")
def call(sw):
    def run(rows, P=256, W=2, n=None, arr=True):
        t = table(sw, rows) if arr else None
        return sw.lib().sml_roundtrip_loopback_batch_typed(t, len(rows) if n is None else n, P, W, 0, None)
    return run


@pytest.fixture(scope="module")
def buf():
    backing = (ctypes.c_uint8 * 8192)()
    base = (ctypes.addressof(backing) + 63) & ~63           # 64-byte aligned
    return backing, base


@pytest.mark.parametrize("dt", [F16, BF16, F32])
def test_batch_validation_without_gpu(sw, call, buf, dt):
    """Every check returns before a HIP call (null stream, no device).  A
    good first slice stands before the bad one: nothing may be launched for
    it, and on a machine without a GPU a launch would not return these."""
    _, a = buf
    b, n = a + 2048, 16
    good = (a + 4096, a + 6144, n, dt, 0)
    UNS, INV, OK = sw.SML_ERR_UNSUPPORTED, sw.SML_ERR_INVALID_ARG, sw.SML_OK
    for P in (0, 100, 2048):
        assert call([good], P=P) == UNS                                     # bad P
    assert call([good, (a, b, n, I32, 0)]) == UNS                           # INT32 is not a float slice
    assert call([good, (a, b, n, 4, 0)]) == UNS                             # no such type
    assert call([good, (a, b, n, 0xFFFFFFFF, 0)]) == UNS
    assert call([good], W=0) == INV                                         # W = 0
    assert call([good] * 65) == INV                                         # more than 64 slices
    assert call([], n=3, arr=False) == INV                                  # null table
    assert call([good, (None, b, n, dt, 0)]) == INV                         # null in
    assert call([good, (a, None, n, dt, 0)]) == INV                         # null out
    assert call([good, (a, b, n, dt, 1)]) == INV                            # reserved
    assert call([good, (a + 1, b, n, dt, 0)]) == INV                        # odd pointers
    assert call([good, (a, b + 1, n, dt, 0)]) == INV
    if dt == F32:
        assert call([good, (a + 2, b, n, dt, 0)]) == INV                    # fp32: 4-byte alignment
        assert call([good, (a, b + 2, n, dt, 0)]) == INV
    # more than 2^32 - 1 tiles in one launch: two slices of one type that
    # fit one by one (1024-element tiles for 16 bits; fp32 512 at P = 256)
    tile = 512 if dt == F32 else 1024
    half = tile * (2 ** 31)
    assert call([good, (a, b, half, dt, 0), (a, b, half, dt, 0)]) == UNS
    # empty and zero-slice calls
    assert call([]) == OK
    assert call([], arr=False) == OK
    assert call([(None, None, 0, dt, 0)] * 64) == OK
    assert call([(a + 1, b + 1, 0, dt, 0)]) == OK                           # an empty slice's pointers are not read
    # ... but its type and reserved word are checked like any slice's
    assert call([(None, None, 0, I32, 0)]) == UNS
    assert call([(None, None, 0, dt, 7)]) == INV
    # two checks fail at once: the call's own arguments come first
    assert call([(a, b, n, I32, 0)], P=100, W=0) == UNS
    assert call([(a, b, n, I32, 0)], W=0) == INV


def test_tile_limit_counts_each_type_on_its_own(sw, call, buf):
    """The 2^32 - 1 tile limit is one launch's: slices of different types go
    into different launches, so their tiles do not add up.  Checked without a
    launch: the call's last slice is bad, which decides once the limit has
    passed."""
    _, a = buf
    b = a + 2048
    per = 1024 * (2 ** 31)
    rows = [(a, b, per, F16, 0), (a, b, per, BF16, 0)]
    assert call(rows + [(a, b, 16, F16, 1)]) == sw.SML_ERR_INVALID_ARG
    assert call(rows + [(a, b, per, F16, 0), (a, b, 16, F16, 1)]) == sw.SML_ERR_UNSUPPORTED


def test_python_wrapper_refuses_mismatched_pairs(sw):
    import torch
    x = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        sw.roundtrip_loopback_batch([(x, torch.zeros(8, dtype=torch.float16))])
    with pytest.raises(TypeError):
        sw.roundtrip_loopback_batch([(torch.zeros(8), x)])


def test_batch_stats_read_zero_after_a_bypass_context_has_run():
    from switchml_amd import client as C
    if C.state() == C.RUNNING:
        C.stop()
    try:
        C.start(C.make_config(prepostprocessor="bypass", num_worker_threads=3, packet_numel=256, bandwidth=0))
        x = np.zeros(1000, dtype=np.float16)
        assert C.allreduce(x).status() == C.JOB_FINISHED
        C.wait_for_all_jobs()
        assert C.stats()["jobs_finished"] == 1
        assert C.batch_stats() == {"launches": 0, "batched_slices": 0, "single_slices": 0}
        assert C.lib().sml_context_batch_stats(None) != 0
    finally:
        if C.state() == C.RUNNING:
            C.stop()
