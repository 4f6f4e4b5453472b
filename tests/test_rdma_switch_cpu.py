"""CPU tests of the RDMA switch (no GPU needed): the sequential model of
tests/rdma_switch_model.py against the plane-level oracle, the seeds of the
GPU's lossy closed loop on the model alone, and the host-side contract of the
three entry points — every argument check returns before any HIP call — with
the ABI table and the record layout held to include/switchml_rdma_switch.h."""
import ctypes

import numpy as np
import pytest

import rdma_switch_model as R
import switch_deliver_model as D
import test_abi_cpu as A
from oracle import oracle as O
from switchml_amd import abi, rdma_switch

LOSSY = dict(W=3, N=40, mop=8, M=64, ppm=4, q=0.1)            # the frame switch's recipe
LOSSY_SEEDS = D.LOSSY_SEEDS
INV, UNS, ALN, OK = abi.SML_ERR_INVALID_ARG, abi.SML_ERR_UNSUPPORTED, abi.SML_ERR_ALIGNMENT, abi.SML_OK
vp = ctypes.c_void_p


def lossy_inputs(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(-2 ** 31, 2 ** 31, LOSSY["N"] * LOSSY["M"], dtype=np.int64).astype(np.int32)
            for _ in range(LOSSY["W"])]


def test_model_equals_the_plane_oracle_on_a_lossless_stream():
    W, S, M, ppm = 3, 4, 64, 2
    rng = np.random.default_rng(5)
    landing = rng.integers(0, 256, (W * S, 4 * M), dtype=np.uint8)
    exps = rng.integers(0, 256, (W * S, 2), dtype=np.uint8)
    rows = [(w, R.rkey(s, 1, ppm), R.imm(s, *exps[w * S + s]), w * S + s, s * 4 * M) for w in range(W) for s in range(S)]
    recs = R.arrivals([rows[i] for i in rng.permutation(len(rows))])
    rx = np.zeros((W, S * 4 * M), dtype=np.uint8)
    verdicts, out_imm, counts = R.model_call(R.RdmaSwitchModel(W, S, M, ppm), recs, landing, rx)
    assert counts == [W * S - S, S, 0, 0, 0, 0] and len(out_imm) == S
    planes = landing.reshape(W, S * 4 * M)
    assert all(np.array_equal(rx[u].view(np.uint32), O.switch_payload([p.view(np.uint32) for p in planes]))
               for u in range(W))
    for i, word in out_imm.items():
        s = int(recs[i]["addr"]) // (4 * M)
        want = [int(O.switch_exps([exps[w * S + s, b:b + 1].view(np.int8) for w in range(W)])[0]) for b in (0, 1)]
        assert word == R.imm(s, *want)


@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_lossy_seeds_finish_on_the_model(seed):
    c, xs = LOSSY, lossy_inputs(seed)
    model = R.RdmaSwitchModel(c["W"], c["mop"], c["M"], c["ppm"])
    rx = np.zeros((c["W"], c["N"] * 4 * c["M"]), dtype=np.uint8)
    loop = R.ClosedLoop(lambda recs, drop: R.model_call(model, recs, loop.landing, rx, drop)[:2], xs, c["mop"],
                        c["M"], c["ppm"])
    assert D.lossy_loop(seed, c["W"], c["N"], c["mop"], c["q"], loop) > 0
    assert loop.verdicts[R.RETRANSMIT] > 0 and loop.verdicts[R.DEFERRED] > 0
    assert all(np.array_equal(r.view(">i4").astype(np.int32), xs[0] + xs[1] + xs[2]) for r in rx)


def test_abi_table_and_record_layout_equal_the_header():
    protos = A.typed_prototypes(abi.RDMA_SWITCH_HEADER_PATH)
    assert sorted(protos) == sorted(abi.RDMA_SWITCH_SIGNATURES) == abi.header_symbols(abi.RDMA_SWITCH_HEADER_PATH)
    L = abi.lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.RDMA_SWITCH_SIGNATURES[name]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        for (base, depth), a in zip(params, argtypes):
            want = {ctypes.POINTER(abi.RdmaSwitchParams)} if base == "sml_rdma_switch_params" else A.allowed(base, depth)
            assert a in want, (name, base)
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    T = abi.RdmaArrival
    assert ctypes.sizeof(T) == R.ARRIVAL.itemsize == rdma_switch.ARRIVAL_BYTES == 24
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [(n, R.ARRIVAL.fields[n][1]) for n in R.ARRIVAL.names]
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 4, 8, 12, 16]
    assert np.dtype(rdma_switch.ARRIVAL_FIELDS) == R.ARRIVAL
    assert '#include "switchml_rdma_switch.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


@pytest.mark.parametrize("S,M,ok", [(1, 64, True), (16384, 1024, True), (7, 256, True), (0, 64, False),
                                    (16385, 64, False), (4, 100, False), (4, 2048, False)])
def test_state_bytes(S, M, ok):
    got = abi.lib().sml_rdma_switch_state_bytes(S, M)
    # claim words, four registers per (slot, set), the touched list, the words; at most a header and padding more
    need = 8 * 32 * S + 4 * 8 * S + 4 * S + 8 * S * M
    assert (need <= got <= need + 128 and got % 16 == 0) if ok else got == 0


GOOD = dict(W=2, S=4, M=64, ppm=4, arr=4096, n=1, land=8192, lstr=256, lmsgs=8, st=16384, rx=32768, rxb=1024,
            dr=65536, imm=131072, vd=262144, cnt=524288)
CASES = [
    ("null params", dict(prm=None), INV),
    *[(f"null {k}", {k: None}, INV) for k in ("arr", "land", "st", "rx", "imm", "vd")],
    *[(f"bad {k}", {k: v}, UNS) for k, v in [("M", 100), ("M", 2048), ("ppm", 0), ("ppm", 3), ("ppm", 32), ("W", 0),
                                             ("W", 33), ("S", 0), ("S", 16385), ("n", 2 ** 31)]],
    ("null wins over unsupported", dict(M=100, arr=None), INV),
    ("unsupported wins over alignment", dict(M=100, land=8196), UNS),
    ("nothing to do", dict(n=0, arr=None, land=None, st=None, rx=None, dr=None, imm=None, vd=None, cnt=None), OK),
    ("nothing to do, bad parameters", dict(n=0, ppm=3), UNS),
    *[(f"misaligned {k}", {k: v}, ALN) for k, v in [
        ("land", 8200), ("lstr", 255), ("lstr", 264), ("lstr", 240), ("rx", 32776), ("rxb", 1032), ("st", 16392),
        ("arr", 4100), ("dr", 65538), ("imm", 131074), ("cnt", 524292)]],
]


@pytest.mark.parametrize("name,change,status", CASES, ids=[c[0] for c in CASES])
def test_switch_argument_status(name, change, status):
    a = dict(GOOD, **change)
    prm = abi.RdmaSwitchParams(a["W"], a["S"], a["M"], a["ppm"])
    ptr = lambda k: None if a[k] is None else vp(a[k])                        # noqa: E731
    got = abi.lib().sml_rdma_switch(None if "prm" in a else ctypes.byref(prm), ptr("arr"), a["n"], ptr("land"),
                                    a["lstr"], a["lmsgs"], ptr("st"), ptr("rx"), a["rxb"], ptr("dr"), ptr("imm"),
                                    ptr("vd"), ptr("cnt"), None)
    assert got == status                                                      # every case returns before a launch


@pytest.mark.parametrize("st,S,M,status", [(None, 4, 64, INV), (4096, 0, 64, UNS), (4096, 4, 100, UNS),
                                           (None, 4, 100, INV), (4104, 4, 64, ALN), (4104, 4, 100, UNS)])
def test_reset_argument_status(st, S, M, status):
    assert abi.lib().sml_rdma_switch_reset(None if st is None else vp(st), S, M, None) == status
