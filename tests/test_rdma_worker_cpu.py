"""CPU tests of the RDMA worker's calls (no GPU needed): the ABI table and both
structures held to include/switchml_rdma_worker.h, sml_rdma_worker_state_bytes,
every argument status of the four calls — each returns before any HIP call —
and the seeds of the GPU's lossy closed loop on the numpy routing alone."""
import ctypes

import numpy as np
import pytest

import test_abi_cpu as A
from switchml_amd import abi, rdma_worker

INV, UNS, ALN, OK = abi.SML_ERR_INVALID_ARG, abi.SML_ERR_UNSUPPORTED, abi.SML_ERR_ALIGNMENT, abi.SML_OK
vp = ctypes.c_void_p
STRUCTS = {"sml_rdma_worker_params": abi.RdmaWorkerParams, "sml_rdma_completion": abi.RdmaCompletion,
           "sml_rdma_arrival": abi.RdmaArrival}

LOSSY = dict(W=3, M=256, Q=4, blocks=20, p_drop=0.2, p_dup=0.15)
LOSSY_SEEDS = (1, 2, 5)


def lossy_masks(rng, n, W):
    """Per result record and worker: its copy is dropped; delivered twice in one call; once more a call later."""
    return tuple(rng.random((n, W)) < p for p in (LOSSY["p_drop"], LOSSY["p_dup"], LOSSY["p_dup"]))


@pytest.mark.parametrize("seed", LOSSY_SEEDS)
def test_lossy_seeds_drop_and_duplicate_in_the_first_round(seed):
    """Round one is W * Q records whatever happens later, and the last worker's
    are the BROADCASTs: a dropped copy there must come back as a RETRANSMIT, a
    delivered copy given twice is WRONG once, one repeated a call later too."""
    W, Q = LOSSY["W"], LOSSY["Q"]
    drop, twice, late = (m[(W - 1) * Q:] for m in lossy_masks(np.random.default_rng(seed), W * Q, W))
    assert drop.any() and (twice & ~drop).any() and (late & ~drop).any()


def test_abi_table_and_struct_layouts_equal_the_header():
    protos = A.typed_prototypes(abi.RDMA_WORKER_HEADER_PATH)
    assert sorted(protos) == sorted(abi.RDMA_WORKER_SIGNATURES) == abi.header_symbols(abi.RDMA_WORKER_HEADER_PATH)
    L = abi.lib()
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.RDMA_WORKER_SIGNATURES[name]
        assert restype in A.allowed(*ret) and len(argtypes) == len(params), name
        for (base, depth), a in zip(params, argtypes):
            assert a in ({ctypes.POINTER(STRUCTS[base]), vp} if base in STRUCTS else A.allowed(base, depth)), (name, base)
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes
    P, C = abi.RdmaWorkerParams, abi.RdmaCompletion
    assert ctypes.sizeof(P) == 32 and [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 6, 8, 12, 16, 20, 24, 28]
    assert ctypes.sizeof(C) == rdma_worker.COMPLETION_BYTES == np.dtype(rdma_worker.COMPLETION_FIELDS).itemsize == 8
    src = A.stripped(abi.RDMA_WORKER_HEADER_PATH)
    for c_name, T in list(STRUCTS.items())[:2]:                    # the header's fields, in the header's order
        body = src.split("typedef struct " + c_name)[1].split("}")[0]
        assert [d.split()[-1] for d in body.strip("{ \n").split(";") if d.strip()] == [n for n, _ in T._fields_]
    assert A.defines(abi.RDMA_WORKER_HEADER_PATH) == {
        "SML_RDMA_WORKER_WRONG": abi.RDMA_WORKER_WRONG, "SML_RDMA_WORKER_POSTED": abi.RDMA_WORKER_POSTED,
        "SML_RDMA_WORKER_FINISHED": abi.RDMA_WORKER_FINISHED, "SML_RDMA_WORKER_IGNORED": abi.RDMA_WORKER_IGNORED}
    assert '#include "switchml_rdma_worker.h"' in open(abi.HEADER_PATH).read() and L.sml_abi_version() == 2


@pytest.mark.parametrize("Q,ok", [(1, True), (7, True), (16384, True), (0, False), (16385, False)])
def test_state_bytes(Q, ok):
    got = abi.lib().sml_rdma_worker_state_bytes(Q)
    assert (got == 64 + 32 * Q) if ok else got == 0               # a slice header, a 32-byte record per QP: O(Q)


GOOD = dict(W=2, dt=abi.FLOAT32, M=64, ppm=4, Q=4, fs=0, x=4096, out=8192, numel=300, st=16384, rx=32768, tx=65536,
            sends=131072, comp=262144, vd=524288, cnt=1048576, qpns=2097152, n=3)
BAD_PARAMS = [("M", 100), ("M", 2048), ("ppm", 0), ("ppm", 3), ("ppm", 32), ("Q", 0), ("Q", 16385), ("fs", 16381),
              ("dt", 4)]
CASES = [
    *[(fn, "null params", dict(prm=None), INV) for fn in ("begin", "poll", "resend")],
    *[(fn, "no workers", dict(W=0), INV) for fn in ("begin", "poll", "resend")],
    *[("begin", f"null {k}", {k: None}, INV) for k in ("x", "out", "tx", "st", "sends")],
    *[("poll", f"null {k}", {k: None}, INV) for k in ("comp", "st", "rx", "tx", "sends", "vd")],
    *[("resend", f"null {k}", {k: None}, INV) for k in ("qpns", "st", "sends")],
    *[(fn, f"bad {k}={v}", {k: v}, UNS) for fn in ("begin", "poll", "resend") for k, v in BAD_PARAMS],
    *[(fn, "too many records", dict(n=2 ** 31), UNS) for fn in ("poll", "resend")],
    ("poll", "null wins over unsupported", dict(M=100, rx=None), INV),
    ("poll", "unsupported wins over alignment", dict(M=100, rx=32776), UNS),
    ("begin", "an empty slice still needs its state", dict(numel=0, x=None, out=None, tx=None, st=None), INV),
    ("poll", "nothing to do", dict(n=0, comp=None, st=None, rx=None, tx=None, sends=None, vd=None, cnt=None), OK),
    ("resend", "nothing to do", dict(n=0, qpns=None, st=None, sends=None), OK),
    ("poll", "nothing to do, bad parameters", dict(n=0, ppm=3), UNS),
    ("poll", "rx and tx overlap", dict(rx=65536 + 512), INV),
    *[("begin", f"misaligned {k}", {k: v}, ALN) for k, v in [("x", 4098), ("out", 8194), ("st", 16392), ("tx", 65544),
                                                             ("sends", 131076)]],
    ("begin", "a 16-bit slice at an odd byte", dict(dt=abi.BFLOAT16, x=4097), ALN),
    *[("poll", f"misaligned {k}", {k: v}, ALN) for k, v in [("st", 16392), ("rx", 32776), ("tx", 65544),
                                                            ("comp", 262148), ("sends", 131076), ("cnt", 1048580)]],
    *[("resend", f"misaligned {k}", {k: v}, ALN) for k, v in [("st", 16392), ("qpns", 2097154), ("sends", 131076)]],
]


@pytest.mark.parametrize("fn,name,change,status", CASES, ids=[f"{c[0]}: {c[1]}" for c in CASES])
def test_argument_status(fn, name, change, status):
    a = dict(GOOD, **change)
    prm = abi.RdmaWorkerParams(0, a["W"], a["dt"], a["M"], a["ppm"], a["Q"], a["fs"], 0, 0)
    ptr = lambda k: None if a[k] is None else vp(a[k])                        # noqa: E731
    L, p = abi.lib(), None if "prm" in a else ctypes.byref(prm)
    if fn == "begin":
        got = L.sml_rdma_worker_begin(p, ptr("x"), ptr("out"), a["numel"], ptr("st"), ptr("tx"), ptr("sends"), None)
    elif fn == "poll":
        got = L.sml_rdma_worker_poll(p, ptr("comp"), a["n"], ptr("st"), ptr("rx"), ptr("tx"), ptr("sends"), ptr("vd"),
                                     ptr("cnt"), None)
    else:
        got = L.sml_rdma_worker_resend(p, ptr("qpns"), a["n"], ptr("st"), ptr("sends"), None)
    assert got == status                                                      # every case returns before a launch


@pytest.mark.parametrize("st,Q,status", [(None, 4, INV), (4096, 0, UNS), (4096, 16385, UNS), (None, 0, INV),
                                         (4104, 4, ALN), (4104, 0, UNS)])
def test_reset_argument_status(st, Q, status):
    assert abi.lib().sml_rdma_worker_reset(None if st is None else vp(st), Q, None) == status
