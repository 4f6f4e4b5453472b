"""CPU tests of the batched round trip for long messages (no GPU needed): the
ABI table held to include/switchml_msg_batch.h, the host-side status contract
of sml_msg_roundtrip_loopback_batch (every case returns before any launch), and
what the client's config accepts and refuses at a long general.packet_numel."""
import pytest

import test_abi_cpu as A
from switchml_amd import abi
from switchml_amd import client as C

INV, UNS, OK = abi.SML_ERR_INVALID_ARG, abi.SML_ERR_UNSUPPORTED, abi.SML_OK


def test_abi_table_equals_the_header():
    protos = A.typed_prototypes(abi.MSG_BATCH_HEADER_PATH)
    assert sorted(protos) == sorted(abi.MSG_BATCH_SIGNATURES) == abi.header_symbols(abi.MSG_BATCH_HEADER_PATH)
    L = abi.lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.MSG_BATCH_SIGNATURES[name]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        assert all(a in A.allowed(*p) for p, a in zip(params, argtypes)), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    assert A.defines(abi.MSG_BATCH_HEADER_PATH) == {}
    assert '#include "switchml_msg_batch.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


# fake device addresses: no case reaches a launch.  A slice is (in, out, numel, data_type, reserved).
GOOD = (4096, 1 << 20, 5000, abi.FLOAT32, 0)
EMPTY = (None, None, 0, abi.FLOAT16, 0)
CASES = [
    ("M=0", dict(M=0), UNS), ("M=100", dict(M=100), UNS), ("M=16448", dict(M=16448), UNS),
    ("unsupported M wins over W=0", dict(M=100, W=0), UNS),
    ("W=0", dict(W=0), INV), ("65 slices", dict(slices=[EMPTY] * 65), INV),
    ("null table", dict(slices=None, n=1), INV),
    ("null table, no slices", dict(slices=None, n=0), OK),
    ("only empty slices", dict(slices=[EMPTY, (None, None, 0, abi.FLOAT32, 0)]), OK),
    ("only empty slices at a packet size", dict(slices=[EMPTY], M=256), OK),
    ("reserved", dict(slices=[EMPTY, GOOD[:4] + (1,)]), INV),
    ("reserved wins over the type", dict(slices=[(4096, 8192, 10, abi.INT32, 1)]), INV),
    ("int32", dict(slices=[EMPTY, GOOD[:3] + (abi.INT32, 0)]), UNS),
    ("unknown type, empty slice", dict(slices=[(None, None, 0, 7, 0)]), UNS),
    ("numel 2^56", dict(slices=[GOOD[:2] + (1 << 56, abi.FLOAT32, 0)]), UNS),
    ("type wins over null", dict(slices=[(None, 8192, 10, abi.INT32, 0)]), UNS),
    ("null in", dict(slices=[(None,) + GOOD[1:]]), INV),
    ("null out", dict(slices=[EMPTY, (4096, None) + GOOD[2:]]), INV),
    ("fp32 in off 4 bytes", dict(slices=[(4098,) + GOOD[1:]]), INV),
    ("odd 16-bit out", dict(slices=[(4096, 8193, 10, abi.BFLOAT16, 0)]), INV),
    ("earlier slice's null wins over a later type", dict(slices=[(None,) + GOOD[1:], GOOD[:3] + (7, 0)]), INV),
    # 2^55 elements are 2^55 / 1024 / 4 = 2^43 groups of one type in one launch
    ("too many groups", dict(slices=[GOOD[:2] + (1 << 55, abi.FLOAT32, 0)], M=1024), UNS),
    ("too many groups at a packet size", dict(slices=[GOOD[:2] + (1 << 55, abi.FLOAT32, 0)], M=64), UNS),
    ("null wins over too many groups", dict(slices=[(None, 8192, 1 << 55, abi.FLOAT32, 0)], M=1024), INV),
]


@pytest.mark.parametrize("name,change,status", CASES, ids=[c[0] for c in CASES])
def test_argument_status(name, change, status):
    a = dict(dict(slices=[GOOD], M=2304, W=2), **change)
    table = None
    if a["slices"] is not None:
        table = (abi.TypedSlice * max(1, len(a["slices"])))(*[abi.TypedSlice(*s) for s in a["slices"]])
    n = a.get("n", 0 if table is None else len(a["slices"]))
    assert abi.lib().sml_msg_roundtrip_loopback_batch(table, n, a["M"], a["W"], 0, None) == status


def test_client_config_refuses_packet_mode_at_a_long_packet_numel():
    """Config::Validate comes before the device is looked for: the refusal
    names the key and the modes that serve it, with or without a GPU."""
    for kw in (dict(mode="packet"), dict(backend="xgmi", session="s", mode="fused")):
        with pytest.raises(C.ContextError, match=r"general\.packet_numel = 2304.*bulk or fused"):
            C.start(C.make_config(packet_numel=2304, **kw))
        assert C.state() == C.CREATED or C.state() == C.STOPPED
    with pytest.raises(C.ContextError, match=r"general\.packet_numel = 2300.*sml_msg_numel_supported"):
        C.start(C.make_config(packet_numel=2300, mode="fused"))
