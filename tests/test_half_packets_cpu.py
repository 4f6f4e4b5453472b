"""CPU tests of FLOAT16 / BFLOAT16 slices on the per-packet paths (no GPU
needed): the three typed burst entry points are exported and declared, their
argument checks are the FLOAT32 ones (every argument list of the burst
validation tests of test_capi_cpu.py, replayed), the `backend.hip.half_packets`
key round-trips, and the CollNet plugin offers the two types under
mode = packet with the key."""
import ctypes

import pytest

from test_capi_cpu import burst_maker, header_prototypes
from test_collnet_plugin import run_driver

TYPED = ("sml_preprocess_burst_typed", "sml_postprocess_burst_typed", "sml_exchange_burst_typed")


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def test_typed_burst_symbols_are_exported_and_declared(sw):
    L = sw.lib()
    protos = header_prototypes(sw.HEADER_PATH)
    for name in TYPED:
        assert name in sw.header_symbols(), name
        assert protos[name] == ("sml_status_t", 2), name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 2, name
    assert L.sml_abi_version() == 2          # symbols added, nothing changed


def argument_lists():
    """(op, keyword arguments of burst_maker's burst) for every call of
    test_burst_validation_without_gpu and
    test_burst_null_slice_pointer_status_order, in their order."""
    lists = []
    for op in ("pre", "post", "exchange"):
        lists += [(op, dict(ids=[0], count=65)), (op, dict(ids=[20])), (op, dict(ids=[3, 3])), (op, dict(ids=[5, 1])),
                  (op, dict(ids=[2], with_extra=False)), (op, dict(ids=[]))]
    lists += [("exchange", dict(ids=[1], b=0)), ("exchange", dict(ids=[1], b=17))]
    for op, null in (("pre", "in"), ("post", "out"), ("exchange", "in"), ("exchange", "out")):
        lists += [(op, dict(ids=[1], null=(null,))), (op, dict(ids=[], null=(null,))),
                  (op, dict(ids=[1], null=(null,), packet_numel=100))]
    return lists


def test_typed_burst_argument_checks_are_the_float32_ones(sw):
    """Every argument list of the two burst validation tests through the typed
    entry points: data_type 0 and 1 give the untyped twin's status, 2 and 3
    the status of 0, 4 is unsupported; the untyped entry points still refuse
    2 and 3 (SML_ERR_UNSUPPORTED, but for the one list whose packet count is
    refused before the type is looked at, as it always was).  Host buffers:
    every check returns before any HIP call."""
    L = sw.lib()
    burst = burst_maker(sw)
    untyped = {"pre": L.sml_preprocess_burst, "post": L.sml_postprocess_burst, "exchange": L.sml_exchange_burst}
    typed = {"pre": L.sml_preprocess_burst_typed, "post": L.sml_postprocess_burst_typed,
             "exchange": L.sml_exchange_burst_typed}
    lists = argument_lists()
    assert len(lists) == 32
    seen = set()
    for op, kw in lists:
        kw = dict(kw)
        ids = kw.pop("ids")

        def status(fn, dt):
            ref = burst(ids, **kw)
            ref._obj.data_type = dt
            return fn(ref, None)

        as_f32 = status(untyped[op], 0)
        seen.add(as_f32)
        for dt in (0, 1):
            assert status(typed[op], dt) == status(untyped[op], dt), (op, kw, ids, dt)
        for dt in (2, 3):
            assert status(typed[op], dt) == as_f32, (op, kw, ids, dt)
            # unchanged: the untyped twin refuses the type, where its two
            # earlier checks (packet size: unsupported as well; more than
            # SML_MAX_BURST packets) do not decide first
            refused = sw.SML_ERR_INVALID_ARG if kw.get("count") == 65 else sw.SML_ERR_UNSUPPORTED
            assert status(untyped[op], dt) == refused, (op, kw, ids, dt)
        assert status(typed[op], 4) == sw.SML_ERR_UNSUPPORTED, (op, kw, ids)
    assert seen == {sw.SML_OK, sw.SML_ERR_INVALID_ARG, sw.SML_ERR_UNSUPPORTED}
    for fn in typed.values():                # no burst at all: the twin's answer
        assert fn(None, None) == sw.SML_ERR_INVALID_ARG


def test_packet_burst_maps_the_16_bit_dtypes(sw):
    torch = pytest.importorskip("torch")
    for dtype, code in ((torch.float32, 0), (torch.int32, 1), (torch.float16, 2), (torch.bfloat16, 3)):
        x = torch.zeros(8, dtype=dtype)
        assert sw.packet_burst(x, x, 64, 1, 1, None, [0], [0], [0]).data_type == code


def test_half_packets_key_round_trips():
    from switchml_amd import client as C
    if C.state() == C.RUNNING:
        C.stop()
    try:
        for kw, line in ((dict(half_packets=True), "half_packets = true"), ({}, "half_packets = false")):
            C.start(C.make_config(prepostprocessor="bypass", bandwidth=0, **kw))
            text = C.config_text()
            section = text.split("[backend.hip]\n")[1].split("[backend.xgmi]")[0]
            assert line + "\n" in section, section
            if not kw:                           # a default configuration opts into nothing
                assert "half_types = true" not in text and "half_packets = true" not in text
            C.stop()
    finally:
        if C.state() == C.RUNNING:
            C.stop()


def test_plugin_offers_16_bit_types_in_packet_mode_with_the_key():
    """mode = packet with half_packets = true runs 16-bit jobs, so
    reduceSupport(6 / 9, sum) is 1 and an iallreduce of fp16 elements is
    accepted (not ncclInvalidArgument).  instant_job_completion: no GPU is
    touched."""
    body = '''
sup2 = {}
for dt in (6, 9, 7):
    s = ctypes.c_int(); tbl.reduceSupport(dt, 0, ctypes.byref(s)); sup2[str(dt)] = s.value
out["support2"] = sup2
h = np.arange(64, dtype=np.float16)
out["f16_size"] = run(ctypes.c_void_p(h.ctypes.data), ctypes.c_void_p(h.ctypes.data), 64, 6)
x = np.arange(1000, dtype=np.float32)
out["size_f32"] = run(ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(x.ctypes.data), 1000, 7)
'''
    ini = ("[general]\nprepostprocessor = hip_exponent_quantizer\ninstant_job_completion = true\n"
           "num_worker_threads = 2\n[backend.dummy]\nbandwidth = 0\n[backend.hip]\nmode = packet\n"
           "half_packets = true\ndevice = 0\n")
    out = run_driver(body, ini)
    assert out["init"] == 0
    assert out["support2"] == {"6": 1, "9": 1, "7": 1}
    assert out["f16_size"] == 2 * 64          # posted and completed: not refused with 4
    assert out["size_f32"] == 4000
