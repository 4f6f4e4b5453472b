"""CPU tests of tests/golden/ref_vectors.json, the results recorded from the
compiled reference (tests/golden/make_ref_vectors.py; format: tests/ref_vectors.py).

1. The oracle (C restatement and its numpy twin) reproduces every record, bit
   for bit, NaN payload bits included.  Runs everywhere, with or without the
   reference.
2. Where oracle/_ref/ exists the records are regenerated in memory and must
   equal the committed file, so the fixture cannot go stale or be hand-edited.
"""
import importlib.util
import os

import numpy as np
import pytest

import ref_vectors as RV
from oracle import oracle as O

DOC = RV.load()


def ids(r):
    return r["name"]


def _maker():
    spec = importlib.util.spec_from_file_location("make_ref_vectors", os.path.join(RV.GOLDEN, "make_ref_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_shape_and_size():
    assert os.path.getsize(RV.PATH) <= 64 * 1024
    assert len(DOC["ppp"]) >= 30 and len(DOC["half"]) == 2 and len(DOC["context"]) >= 10
    assert {r["P"] for r in DOC["ppp"]} == {64, 128, 256, 512, 1024}
    assert {r["W"] for r in DOC["ppp"]} >= {1, 3, 8, 65535}
    assert all(r["n"] <= 8192 for r in DOC["ppp"]) and all(r["n"] <= 100_003 for r in DOC["context"])
    assert any(r["out"]["nan_at"] for r in DOC["ppp"])                  # the scale-0 block
    assert any(r["global_exps"] is not None for r in DOC["ppp"])
    assert any(r["n"] % r["P"] for r in DOC["ppp"])                     # partial last blocks
    names = [r["name"] for k in ("ppp", "half", "context") for r in DOC[k]]
    assert len(set(names)) == len(names)


def oracle_ppp(x, r, np_twin=False):
    P, W, n = r["P"], r["W"], x.size
    ge = None if r["global_exps"] is None else np.array(r["global_exps"], dtype=np.int8)
    ex, qu, de = (O.np_exponents, O.np_quantize, O.np_dequantize) if np_twin else (O.exponents, O.quantize, O.dequantize)
    own = ex(x, P)
    q = qu(x, P, W, global_exps=ge)
    out = de(O.loopback_aggregate(q, W), own if ge is None else ge, n, P, W)
    return own, q[:n], out


@pytest.mark.parametrize("np_twin", [False, True], ids=["c", "numpy"])
@pytest.mark.parametrize("r", DOC["ppp"], ids=ids)
def test_oracle_reproduces_ppp_record(r, np_twin):
    x = RV.make_input(r["input"])
    assert x.size == r["n"]
    own, q, out = oracle_ppp(x, r, np_twin)
    RV.check_plane(own, r["exps"], 2, "exponent plane")
    RV.check_plane(q, r["payload"], 8, "payload")
    RV.check_plane(out, r["out"], 8, "output", exact_nan=True)
    if r["global_exps"] is None and not np_twin:
        rt = O.dummy_allreduce(x, P=r["P"], max_outstanding_packets=r["batch"], num_worker_threads=1,
                               num_workers=r["W"])
        RV.check_plane(rt, r["out"], 8, "packet loop output", exact_nan=True)


@pytest.mark.parametrize("r", DOC["half"], ids=ids)
def test_oracle_reproduces_16_bit_record(r):
    raw, x = RV.half_input(r["input"])
    assert raw.size == r["n"] and np.isfinite(x).all()
    own, q, out = oracle_ppp(x, r)
    RV.check_plane(own, r["exps"], 2, "exponent plane")
    RV.check_plane(q, r["payload"], 8, "payload")
    RV.check_plane(out, r["out"], 8, "output", exact_nan=True)


@pytest.mark.parametrize("r", DOC["context"], ids=ids)
def test_oracle_reproduces_context_record(r):
    x = RV.make_input(r["input"])
    P, W, T, n = r["P"], r["W"], r["T"], r["n"]
    if r["type"] == "i32":
        out = (x.astype(np.int64) * (W if r["process_packets"] else 1)).astype(np.int32)
        assert np.array_equal(out.view(np.uint32),
                              O.bswap32(O.loopback_aggregate(O.bswap32(x), W if r["process_packets"] else 1)))
    elif r["process_packets"]:
        out = O.dummy_allreduce(x, P=P, max_outstanding_packets=r["mop"], num_worker_threads=T, num_workers=W)
    else:
        out = np.empty_like(x)
        for t in range(T):
            off, m = O.slice_geometry(n, T, t)
            sl = x[off:off + m]
            out[off:off + m] = O.dequantize(O.quantize(sl, P, W), O.exponents(sl, P), m, P, W)
    RV.check_plane(out, r["out"], 8, "context output", exact_nan=True)


def test_committed_fixture_is_what_the_reference_produces():
    """Only where the reference is built: the committed file, regenerated."""
    if not O.ref_available():
        if O.reference_checkout_available():
            pytest.fail("the reference checkout exists but oracle/_ref/ is not built: run __graft_entry__.build()")
        return                       # nothing to regenerate with; the tests above still hold the oracle to the file
    mk = _maker()
    with open(RV.PATH) as f:
        committed = f.read()
    assert mk.dumps(mk.make()) == committed, "ref_vectors.json is stale: run tests/golden/make_ref_vectors.py"
