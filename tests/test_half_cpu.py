"""CPU tests of the FLOAT16 / BFLOAT16 support (no GPU needed): the typed
C-ABI entry points exist and validate their arguments before any HIP call,
the CollNet plugin accepts the two NCCL types, and the client counts a 16-bit
slice's packets by wire words (B = ceil(numel / P)), not by element bytes."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from test_collnet_plugin import run_driver

TYPED = ("sml_exponents_typed", "sml_quantize_pack_typed", "sml_dequantize_typed", "sml_roundtrip_loopback_typed",
         "sml_switch_aggregate_typed")
F32, I32, F16, BF16 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def test_typed_symbols_exported_and_declared(sw):
    L = sw.lib()
    assert [s for s in TYPED if not hasattr(L, s)] == []
    assert set(TYPED) <= set(sw.header_symbols())
    assert L.sml_abi_version() == 2          # symbols were added, nothing changed
    assert (sw.FLOAT32, sw.INT32, sw.FLOAT16, sw.BFLOAT16) == (F32, I32, F16, BF16)


class Calls:
    """The five typed entry points with one argument list: a typed buffer
    `buf` (input, and output for the round trip / K4 / K6), a payload plane
    `pay`, an exponent plane `exps`."""

    def __init__(self, L):
        self.L = L

    def exponents(self, buf, dt, n, P, W, pay, exps):
        return self.L.sml_exponents_typed(buf, dt, n, P, exps, None)

    def quantize(self, buf, dt, n, P, W, pay, exps):
        return self.L.sml_quantize_pack_typed(buf, dt, n, P, W, None, pay, exps, 0, None)

    def dequantize(self, buf, dt, n, P, W, pay, exps):
        return self.L.sml_dequantize_typed(pay, exps, n, P, W, buf, dt, 0, None)

    def roundtrip(self, buf, dt, n, P, W, pay, exps):
        return self.L.sml_roundtrip_loopback_typed(buf, buf, dt, n, P, W, pay, exps, 0, None)

    def switch(self, buf, dt, n, P, W, pay, exps):
        pp = (ctypes.c_void_p * 1)(pay)
        ep = (ctypes.c_void_p * 1)(exps)
        return self.L.sml_switch_aggregate_typed(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ep, ctypes.c_void_p),
                                                 1 if W else 0, n, P, None, None, buf, dt, 0, None)

    ALL = ("exponents", "quantize", "dequantize", "roundtrip", "switch")


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("name", Calls.ALL)
def test_typed_validation_without_gpu(sw, name, dt):
    """Every check returns before a HIP call, so no device is needed."""
    call = getattr(Calls(sw.lib()), name)
    backing = (ctypes.c_uint8 * 8192)()
    base = (ctypes.addressof(backing) + 63) & ~63           # 64-byte aligned
    buf, pay, exps = base, base + 1024, base + 6144
    n, P, W = 16, 256, 2
    assert call(buf, dt, n, 100, W, pay, exps) == sw.SML_ERR_UNSUPPORTED          # bad P
    assert call(buf, I32, n, P, W, pay, exps) == sw.SML_ERR_UNSUPPORTED           # INT32 is not a float bucket
    assert call(buf, 4, n, P, W, pay, exps) == sw.SML_ERR_UNSUPPORTED             # no such type
    if name != "exponents":                                                       # K2 has no W
        assert call(buf, dt, n, P, 0, pay, exps) == sw.SML_ERR_INVALID_ARG        # W = 0
    assert call(None, dt, n, P, W, pay, exps) == sw.SML_ERR_INVALID_ARG           # null typed buffer
    assert call(buf + 1, dt, n, P, W, pay, exps) == sw.SML_ERR_INVALID_ARG        # odd typed pointer
    if name != "exponents":                                                       # K2 has no payload plane
        assert call(buf, dt, n, P, W, pay + 4, exps) == sw.SML_ERR_ALIGNMENT      # payload not 16-byte aligned
    assert call(buf, dt, 0, P, W, pay, exps) == sw.SML_OK                         # nothing to do
    assert call(None, dt, 0, P, W, None, None) == sw.SML_OK
    # a 2-byte aligned typed buffer is fine as far as validation goes: the
    # next check that fails is a later one (the payload's alignment)
    if name != "exponents":
        assert call(buf + 2, dt, n, P, W, pay + 4, exps) == sw.SML_ERR_ALIGNMENT
    # two checks fail at once: the earlier one decides
    assert call(buf, dt, n, 100, 0, pay, exps) == sw.SML_ERR_UNSUPPORTED          # bad P before W = 0
    assert call(None, dt, n, P, W, pay + 4, exps) == sw.SML_ERR_INVALID_ARG       # null buffer before the payload's alignment
    assert call(buf + 1, dt, n, P, W, pay + 4, exps) == sw.SML_ERR_INVALID_ARG    # odd pointer before the payload's alignment
    # nothing to do comes after W = 0 (K2 has no W) and before the pointers
    assert call(None, dt, 0, P, 0, None, None) == (sw.SML_OK if name == "exponents" else sw.SML_ERR_INVALID_ARG)
    assert call(None, dt, 0, 100, W, None, None) == sw.SML_ERR_UNSUPPORTED


# fp32 entry point -> where its typed twin takes the sml_data_type_t
TWIN_TYPE_ARG = {"sml_exponents": 1, "sml_quantize_pack": 1, "sml_dequantize": 6, "sml_roundtrip_loopback": 2,
                 "sml_quantize_pack_frames": 1, "sml_dequantize_frames": 11, "sml_switch_aggregate": 8,
                 "sml_copy_segments": 4}


class RecordingLib:
    """The library, noting every call of an fp32 entry point that has a typed twin."""

    def __init__(self, L, calls):
        self._L, self._calls = L, calls

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if name not in TWIN_TYPE_ARG:
            return fn

        def call(*args):
            self._calls.append((name, args))
            return fn(*args)
        return call


class RecordingModule:
    """switchml_amd with lib() recording (what the C-ABI tests take as `sw`)."""

    def __init__(self, sw, calls):
        self._sw, self._lib = sw, RecordingLib(sw.lib(), calls)

    def lib(self):
        return self._lib

    def __getattr__(self, name):
        return getattr(self._sw, name)


def test_typed_float32_returns_what_its_fp32_twin_returns(sw):
    """A typed entry point given SML_FLOAT32 is its fp32 twin (switchml_hip.h):
    equal status for every argument list the C-ABI validation tests send to an
    fp32 entry point — lists where two checks fail at once included, such as a
    bad packet size with num_workers == 0 — and for a grid of bad tables,
    worker counts and planes on the switch's aggregate and segment copy.
    Every check returns before a HIP call, so no device is needed."""
    import test_capi_cpu as capi
    L = sw.lib()
    calls = []
    rec = RecordingModule(sw, calls)
    capi.test_argument_validation_without_gpu(rec)
    capi.test_frames_and_rdma_validation_without_gpu(rec)
    capi.test_rx_frames_validation_without_gpu(rec)
    assert {name for name, _ in calls} == set(TWIN_TYPE_ARG) - {"sml_switch_aggregate", "sml_copy_segments"}

    vp = ctypes.c_void_p
    backing = (ctypes.c_uint8 * 8192)()
    base = (ctypes.addressof(backing) + 63) & ~63           # 64-byte aligned
    out, pay, exps = base, base + 1024, base + 6144

    def table(k, p):
        return ctypes.cast((vp * k)(*[p] * k), vp)

    # Every list below has a fault or nothing to do, so none reaches a launch:
    # the one sound combination of each grid is left out.
    for W in (0, 1, 16, 17):
        k = max(W, 1)
        tables = ((table(k, pay), table(k, exps)),              # sound
                  (None, table(k, exps)), (table(k, pay), None),    # a null table
                  (table(k, pay + 4), table(k, exps)),              # planes off their 16 bytes
                  (table(k, None), table(k, exps)))                 # null planes
        for i, (pp, ep) in enumerate(tables):
            for P in (256, 100):
                sound = i == 0 and W in (1, 16) and P == 256
                # a bucket off its 4 bytes, no output at all, a sound bucket
                for o in (out + 2, None) + (() if sound else (out,)):
                    calls.append(("sml_switch_aggregate", (pp, ep, W, 16, P, None, None, o, 0, None)))
                calls.append(("sml_switch_aggregate", (pp, ep, W, 16, P, pay + 4, None, out, 0, None)))
                calls.append(("sml_switch_aggregate", (pp, ep, W, 0, P, None, None, None, 0, None)))
    words = ctypes.cast((ctypes.c_uint64 * 17)(*[4] * 17), vp)
    empty = ctypes.cast((ctypes.c_uint64 * 17)(), vp)
    for k in (0, 1, 16, 17):
        tables = ((table(17, out), table(17, pay)),             # sound
                  (None, table(17, pay)), (table(17, out), None),   # a null table
                  (table(17, out + 2), table(17, pay)), (table(17, out), table(17, pay + 1)),   # off their 4 bytes
                  (table(17, None), table(17, pay)))                # null segments
        for i, (srcs, dsts) in enumerate(tables):
            for n in (empty, None) + (() if i == 0 and k in (1, 16) else (words,)):
                calls.append(("sml_copy_segments", (srcs, dsts, n, k, 0, None)))

    seen = set()
    for name, args in calls:
        at = TWIN_TYPE_ARG[name]
        s32 = getattr(L, name)(*args)
        st = getattr(L, name + "_typed")(*args[:at], F32, *args[at:])
        assert st == s32, (name, args, st, s32)
        assert s32 != sw.SML_ERR_HIP, (name, args)          # a check answered, not the device
        seen.add((name, s32))
    # the lists reach every status on both sides of the grid
    for name in ("sml_switch_aggregate", "sml_copy_segments"):
        assert {s for n_, s in seen if n_ == name} >= {sw.SML_OK, sw.SML_ERR_INVALID_ARG}
    assert ("sml_switch_aggregate", sw.SML_ERR_UNSUPPORTED) in seen      # 17 workers, bad P
    assert ("sml_switch_aggregate", sw.SML_ERR_ALIGNMENT) in seen        # a plane off its 16 bytes


def test_client_data_type_sizes_and_wire_geometry():
    """sml_allreduce with data_type 2 / 3 under the bypass PPP: the job
    finishes, and every FIFO slice counts ceil(numel / P) packets (bypass has
    no extra batch) — not half of them, which counting the slice's bytes
    against the packet's would give."""
    from switchml_amd import client as C
    assert (C.FLOAT32, C.INT32, C.FLOAT16, C.BFLOAT16) == (0, 1, 2, 3)
    P, T = 256, 3
    if C.state() == C.RUNNING:
        C.stop()
    try:
        for dt, numel in ((C.FLOAT16, 1000), (C.BFLOAT16, 1000), (C.FLOAT16, 1), (C.BFLOAT16, 100_003)):
            C.start(C.make_config(prepostprocessor="bypass", num_worker_threads=T, packet_numel=P,
                                  max_outstanding_packets=255, bandwidth=0))
            x = np.zeros(numel, dtype=np.uint16)
            rc = C.lib().sml_allreduce(ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(x.ctypes.data), numel, dt,
                                        C.SUM)
            assert rc == 0, C.lib().sml_context_last_error()
            C.wait_for_all_jobs()      # the finished-jobs counter follows the job's own wake-up
            st = C.stats()
            expect = sum(O.num_blocks(O.slice_geometry(numel, T, t)[1], P) for t in range(T))
            assert st["jobs_finished"] == 1 and st["numel_submitted"] == numel
            assert st["packets"] == expect, (dt, numel)
            C.stop()
        # numpy.float16 arrays map to FLOAT16; 4 is still no data type
        C.start(C.make_config(prepostprocessor="bypass", num_worker_threads=T, packet_numel=P, bandwidth=0))
        h = np.zeros(777, dtype=np.float16)
        assert C._dtype_of(h) == C.FLOAT16
        assert C.allreduce(h).status() == C.JOB_FINISHED
        assert C.lib().sml_allreduce(ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), 777, 4,
                                      C.SUM) != 0
        assert C.lib().sml_allreduce(ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), 777, -1,
                                      C.SUM) != 0
    finally:
        if C.state() == C.RUNNING:
            C.stop()


def test_client_torch_dtypes_map_to_the_16_bit_types():
    import torch
    from switchml_amd import client as C
    assert C._dtype_of(torch.zeros(1, dtype=torch.bfloat16)) == C.BFLOAT16
    assert C._dtype_of(torch.zeros(1, dtype=torch.float16)) == C.FLOAT16
    assert C._dtype_of(torch.zeros(1, dtype=torch.float32)) == C.FLOAT32
    with pytest.raises(TypeError):
        C._dtype_of(torch.zeros(1, dtype=torch.float64))


def test_plugin_supports_fp16_bf16_sum_and_bypass_allreduce():
    """reduceSupport(ncclFloat16 = 6 / ncclBfloat16 = 9, sum) == 1, max == 0;
    a bypass-PPP all-reduce of 1000 fp16 elements reports size == 2000."""
    from switchml_amd import collnet
    assert (collnet.NCCL_FLOAT16, collnet.NCCL_BFLOAT16) == (6, 9)
    body = '''
sup2 = {}
for dt in (6, 9):
    for op in (0, 2):
        s = ctypes.c_int(); tbl.reduceSupport(dt, op, ctypes.byref(s)); sup2[f"{dt},{op}"] = s.value
out["support2"] = sup2
h = np.arange(1000, dtype=np.float16)
out["size_f16"] = run(ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), 1000, 6)
b = np.zeros(1000, dtype=np.uint16)
out["size_bf16"] = run(ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(b.ctypes.data), 1000, 9)
'''
    ini = "[general]\nprepostprocessor = bypass\nnum_worker_threads = 2\n[backend.dummy]\nbandwidth = 0\n"
    out = run_driver(body, ini)
    assert out["init"] == 0
    assert out["support2"] == {"6,0": 1, "6,2": 0, "9,0": 1, "9,2": 0}
    assert out["size_f16"] == 2000 and out["size_bf16"] == 2000


def test_plugin_declines_16_bit_types_where_the_configuration_refuses_them():
    """mode = packet (like backend = xgmi) refuses 16-bit jobs, so there
    reduceSupport(6 / 9, sum) stays 0 — the caller keeps its own algorithms —
    while fp32 is still offered; an iallreduce of such a type is
    ncclInvalidArgument (4) and creates no job.  instant_job_completion: no
    GPU is touched."""
    body = '''
sup2 = {}
for dt in (6, 9, 7):
    s = ctypes.c_int(); tbl.reduceSupport(dt, 0, ctypes.byref(s)); sup2[str(dt)] = s.value
out["support2"] = sup2
h = np.arange(64, dtype=np.float16)
out["bf16_rc"] = tbl.iallreduce(coll, ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), 64, 9, 0, None,
                                None, ctypes.byref(vp()))
out["f16_rc"] = tbl.iallreduce(coll, ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), 64, 6, 0, None,
                               None, ctypes.byref(vp()))
x = np.arange(1000, dtype=np.float32)
out["size_f32"] = run(ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(x.ctypes.data), 1000, 7)
'''
    ini = ("[general]\nprepostprocessor = hip_exponent_quantizer\ninstant_job_completion = true\n"
           "num_worker_threads = 2\n[backend.dummy]\nbandwidth = 0\n[backend.hip]\nmode = packet\ndevice = 0\n")
    out = run_driver(body, ini)
    assert out["init"] == 0
    assert out["support2"] == {"6": 0, "9": 0, "7": 1}
    assert out["bf16_rc"] == 4 and out["f16_rc"] == 4
    assert out["size_f32"] == 4000            # the communicator is still fine
