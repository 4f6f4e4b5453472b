"""CPU tests of the RDMA switch for long messages (no GPU needed): the ABI
table held to include/switchml_msg_switch.h, the state's size, and the
host-side status contract of sml_msg_switch and sml_msg_switch_reset — the
table of tests/test_rdma_switch_cpu.py restated for what the new entry points
accept; every case returns before any launch."""
import ctypes

import pytest

import test_abi_cpu as A
import test_rdma_switch_cpu as C
from switchml_amd import abi

INV, UNS, ALN, OK = C.INV, C.UNS, C.ALN, C.OK
vp = ctypes.c_void_p


def test_abi_table_equals_the_header():
    protos = A.typed_prototypes(abi.MSG_SWITCH_HEADER_PATH)
    assert sorted(protos) == sorted(abi.MSG_SWITCH_SIGNATURES) == abi.header_symbols(abi.MSG_SWITCH_HEADER_PATH)
    L = abi.lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.MSG_SWITCH_SIGNATURES[name]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        for (base, depth), a in zip(params, argtypes):
            want = {ctypes.POINTER(abi.RdmaSwitchParams)} if base == "sml_rdma_switch_params" else A.allowed(base, depth)
            assert a in want, (name, base)
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    assert '#include "switchml_msg_switch.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


@pytest.mark.parametrize("S,M,ok", [(1, 64, True), (4, 2048, True), (7, 2304, True), (16384, 16384, True),
                                    (4, 100, False), (4, 16448, False), (0, 64, False), (16385, 64, False)])
def test_state_bytes(S, M, ok):
    got = abi.lib().sml_msg_switch_state_bytes(S, M)
    need = 8 * 32 * S + 4 * 8 * S + 4 * S + 8 * S * M                         # test_rdma_switch_cpu.test_state_bytes'
    assert (need <= got <= need + 128 and got % 16 == 0) if ok else got == 0


# what sml_rdma_switch refuses and this entry accepts leaves the table; its own limits join it
CASES = [c for c in C.CASES if c[1] not in (dict(M=2048), dict(ppm=3), dict(ppm=32), dict(n=0, ppm=3))] + [
    ("M=2048, ppm=8", dict(M=2048, ppm=8, n=0), OK), ("ppm=3", dict(ppm=3, n=0), OK),
    ("ppm=256, M=16384", dict(M=16384, ppm=256, n=0), OK), ("bad M", dict(M=16448), UNS),
    ("bad ppm", dict(ppm=257), UNS), ("nothing to do, bad parameters", dict(n=0, ppm=257), UNS),
    ("misaligned lstr", dict(M=2304, ppm=9, lstr=9200), ALN)]                 # 16-byte aligned, below 4 M


@pytest.mark.parametrize("name,change,status", CASES, ids=[f"{i}-{c[0]}" for i, c in enumerate(CASES)])
def test_switch_argument_status(name, change, status):
    a = dict(C.GOOD, **change)
    prm = abi.RdmaSwitchParams(a["W"], a["S"], a["M"], a["ppm"])
    ptr = lambda k: None if a[k] is None else vp(a[k])                        # noqa: E731
    got = abi.lib().sml_msg_switch(None if "prm" in a else ctypes.byref(prm), ptr("arr"), a["n"], ptr("land"),
                                   a["lstr"], a["lmsgs"], ptr("st"), ptr("rx"), a["rxb"], ptr("dr"), ptr("imm"),
                                   ptr("vd"), ptr("cnt"), None)
    assert got == status


@pytest.mark.parametrize("st,S,M,status", [(None, 4, 2304, INV), (4096, 0, 2304, UNS), (4096, 4, 16448, UNS),
                                           (None, 4, 100, INV), (4104, 4, 2304, ALN), (4104, 4, 100, UNS)])
def test_reset_argument_status(st, S, M, status):
    assert abi.lib().sml_msg_switch_reset(None if st is None else vp(st), S, M, None) == status
