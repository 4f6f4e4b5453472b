"""CPU tests of the long RDMA messages (no GPU needed): the ABI table and the
defines held to include/switchml_messages.h, sml_msg_numel_supported, the
host-side status contract of the four entry points (every case returns before
any launch), and the oracle at message sizes held to the compiled reference."""
import ctypes

import numpy as np
import pytest

import switchml_amd
import test_abi_cpu as A
from oracle import oracle as O
from switchml_amd import abi

INV, UNS, ALN, OK = abi.SML_ERR_INVALID_ARG, abi.SML_ERR_UNSUPPORTED, abi.SML_ERR_ALIGNMENT, abi.SML_OK
vp = ctypes.c_void_p


def test_abi_table_and_defines_equal_the_header():
    protos = A.typed_prototypes(abi.MESSAGES_HEADER_PATH)
    assert sorted(protos) == sorted(abi.MESSAGES_SIGNATURES) == abi.header_symbols(abi.MESSAGES_HEADER_PATH)
    L = abi.lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.MESSAGES_SIGNATURES[name]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        assert all(a in A.allowed(*p) for p, a in zip(params, argtypes)), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    assert A.defines(abi.MESSAGES_HEADER_PATH) == {"SML_MSG_NUMEL_STEP": abi.MSG_NUMEL_STEP,
                                                   "SML_MSG_NUMEL_MAX": abi.MSG_NUMEL_MAX}
    assert (switchml_amd.MSG_NUMEL_STEP, switchml_amd.MSG_NUMEL_MAX) == (64, 16384)
    assert '#include "switchml_messages.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


@pytest.mark.parametrize("M,ok", [(0, 0), (63, 0), (64, 1), (100, 0), (192, 1), (1024, 1), (2304, 1), (16384, 1),
                                  (16448, 0), (2 ** 32 - 64, 0)])
def test_msg_numel_supported(M, ok):
    assert abi.lib().sml_msg_numel_supported(M) == ok and switchml_amd.msg_numel_supported(M) == bool(ok)


# fake device addresses: no case reaches a launch
GOOD = dict(inp=4096, out=8192, dt=abi.FLOAT32, n=5000, M=2048, W=2, gexp=None, pay=65536, exps=131072)
NOTHING = dict(n=0, inp=None, out=None, pay=None, exps=None)
ENTRIES = {   # entry point -> (argument order, its typed buffer)
    "sml_msg_exponents": (("inp", "dt", "n", "M", "exps"), "inp"),
    "sml_msg_quantize_pack": (("inp", "dt", "n", "M", "W", "gexp", "pay", "exps", "flags"), "inp"),
    "sml_msg_dequantize": (("pay", "exps", "n", "M", "W", "out", "dt", "flags"), "out"),
    "sml_msg_roundtrip_loopback": (("inp", "out", "dt", "n", "M", "W", "pay", "exps", "flags"), "out"),
}
CASES = []
for fn, (_, buf) in ENTRIES.items():
    CASES += [(fn, f"M={M}", dict(M=M), UNS) for M in (0, 100, 16448)]
    CASES += [(fn, "int32", dict(dt=abi.INT32), UNS), (fn, "unknown type", dict(dt=7), UNS),
              (fn, "nothing to do", NOTHING, OK), (fn, "nothing to do, bad M", dict(NOTHING, M=100), UNS),
              (fn, "null buffer", {buf: None}, INV), (fn, "fp32 buffer off 4 bytes", {buf: GOOD[buf] + 2}, INV),
              (fn, "odd 16-bit pointer", {buf: GOOD[buf] + 1, "dt": abi.FLOAT16}, INV),
              (fn, "16-bit pointer at 2 bytes, bad M", {buf: GOOD[buf] + 2, "dt": abi.BFLOAT16, "M": 100}, UNS)]
    if fn != "sml_msg_exponents":
        CASES += [(fn, "W=0", dict(W=0), INV), (fn, "misaligned payload", dict(pay=65544), ALN),
                  (fn, "null buffer wins over alignment", {buf: None, "pay": 65544}, INV)]
# the FLOAT32 twins' order: K2 and K1 look at their planes before msg_numel, K4 and the round trip after
CASES += [("sml_msg_exponents", "null wins over unsupported", dict(exps=None, M=100), INV),
          ("sml_msg_quantize_pack", "null wins over unsupported", dict(pay=None, M=100), INV),
          ("sml_msg_quantize_pack", "W=0 wins over unsupported", dict(W=0, M=100), INV),
          ("sml_msg_quantize_pack", "two exponent planes", dict(gexp=262144), INV),
          ("sml_msg_dequantize", "unsupported wins over null", dict(pay=None, M=100), UNS),
          ("sml_msg_dequantize", "unsupported wins over W=0", dict(W=0, M=16448), UNS),
          ("sml_msg_dequantize", "null exponents", dict(exps=None), INV),
          ("sml_msg_roundtrip_loopback", "unsupported wins over null", dict(inp=None, M=100), UNS),
          ("sml_msg_roundtrip_loopback", "null input", dict(inp=None), INV)]


@pytest.mark.parametrize("fn,name,change,status", CASES, ids=[f"{c[0][8:]}-{c[1]}" for c in CASES])
def test_argument_status(fn, name, change, status):
    a = dict(GOOD, flags=0, **change)
    args = [a[k] if k in ("dt", "n", "M", "W", "flags") else (None if a[k] is None else vp(a[k]))
            for k in ENTRIES[fn][0]]
    assert getattr(abi.lib(), fn)(*args, None) == status


@pytest.mark.parametrize("M", [768, 2304, 4096])
def test_oracle_equals_the_compiled_reference_at_message_sizes(M):
    if not O.ref_available():
        pytest.skip("oracle/_ref/ is not built here")
    from test_oracle_vs_reference import check_stream
    x = O.splitmix_normal(M, 2 * M + 19)
    x[M + 5] = 300.0                                            # the second message's exponent differs
    r = O.ref_packet_stream(x, M, 3, batch=2)
    own, _ = check_stream(r, x, M, 3, None, M)
    assert own[1] > own[0] and np.array_equal(O.np_exponents(x, M), own)
