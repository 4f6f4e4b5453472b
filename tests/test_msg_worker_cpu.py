"""CPU tests of the RDMA worker for long messages (no GPU needed): the ABI
table held to include/switchml_msg_worker.h, the state's size, and the
host-side status contract of the sml_msg_worker_* calls — the table of
tests/test_rdma_worker_cpu.py replayed for what the new entry points accept;
every case returns before any launch."""
import ctypes

import pytest

import test_abi_cpu as A
import test_rdma_worker_cpu as C
from switchml_amd import abi

INV, UNS, ALN, OK = C.INV, C.UNS, C.ALN, C.OK
vp = ctypes.c_void_p


def test_abi_table_equals_the_header():
    protos = A.typed_prototypes(abi.MSG_WORKER_HEADER_PATH)
    assert sorted(protos) == sorted(abi.MSG_WORKER_SIGNATURES) == abi.header_symbols(abi.MSG_WORKER_HEADER_PATH)
    L = abi.lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.MSG_WORKER_SIGNATURES[name]
        assert (restype, argtypes) == abi.RDMA_WORKER_SIGNATURES[name.replace("sml_msg_worker", "sml_rdma_worker")]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        for (base, depth), a in zip(params, argtypes):
            want = {ctypes.POINTER(C.STRUCTS[base]), vp} if base in C.STRUCTS else A.allowed(base, depth)
            assert a in want, (name, base)
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    assert '#include "switchml_msg_worker.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


@pytest.mark.parametrize("Q,ok", [(1, True), (7, True), (16384, True), (0, False), (16385, False)])
def test_state_bytes(Q, ok):
    assert abi.lib().sml_msg_worker_state_bytes(Q) == (64 + 32 * Q if ok else 0)


def call(fn, change):
    a = dict(C.GOOD, **change)
    prm = abi.RdmaWorkerParams(0, a["W"], a["dt"], a["M"], a["ppm"], a["Q"], a["fs"], 0, 0)
    ptr = lambda k: None if a[k] is None else vp(a[k])                        # noqa: E731
    L, p = abi.lib(), None if "prm" in a else ctypes.byref(prm)
    if fn == "begin":
        return L.sml_msg_worker_begin(p, ptr("x"), ptr("out"), a["numel"], ptr("st"), ptr("tx"), ptr("sends"), None)
    if fn == "poll":
        return L.sml_msg_worker_poll(p, ptr("comp"), a["n"], ptr("st"), ptr("rx"), ptr("tx"), ptr("sends"), ptr("vd"),
                                     ptr("cnt"), None)
    return L.sml_msg_worker_resend(p, ptr("qpns"), a["n"], ptr("st"), ptr("sends"), None)


# what sml_rdma_worker_* refuse and these accept leaves the table; their own limits join it
NOW_SERVED = (dict(M=2048), dict(ppm=3), dict(ppm=32), dict(n=0, ppm=3))
CASES = [c for c in C.CASES if c[2] not in NOW_SERVED] + [
    *[(fn, f"n = 0 at M={M}, ppm={ppm}", dict(n=0, M=M, ppm=ppm), OK)
      for fn in ("poll", "resend") for M, ppm in [(2048, 8), (16384, 256), (192, 3)]],
    ("begin", "M = 2048 passes the parameters", dict(M=2048, tx=65544), ALN),
    *[(fn, f"bad {k}={v}", {k: v}, UNS)                                       # M = 100 and ppm = 0 are C.CASES'
      for fn in ("begin", "poll", "resend") for k, v in [("M", 16448), ("M", 0), ("ppm", 257)]],
    ("poll", "nothing to do, bad parameters", dict(n=0, ppm=257), UNS)]


@pytest.mark.parametrize("fn,name,change,status", CASES, ids=[f"{i}-{c[0]}: {c[1]}" for i, c in enumerate(CASES)])
def test_argument_status(fn, name, change, status):
    assert call(fn, change) == status                                         # every case returns before a launch


@pytest.mark.parametrize("st,Q,status", [(None, 4, INV), (4096, 0, UNS), (4096, 16385, UNS), (None, 0, INV),
                                         (4104, 4, ALN), (4104, 0, UNS)])
def test_reset_argument_status(st, Q, status):
    assert abi.lib().sml_msg_worker_reset(None if st is None else vp(st), Q, None) == status
