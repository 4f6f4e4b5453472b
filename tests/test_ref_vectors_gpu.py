"""GPU tests: the HIP kernels and the C++ client held DIRECTLY to results
recorded from the compiled reference (tests/golden/ref_vectors.json, made by
tests/golden/make_ref_vectors.py), not through the oracle.  Only the committed
fixture is read.

Every PPP record goes through K2, K1, K3 (with the recorded global exponents,
or the record's own), K5 + K4, and, where the record uses its own exponents
as the dummy backend's loop does, the fused round trip, the batched round
trip (the record as one slice among two others) and the per-packet burst
path.  The two 16-bit records are fed as fp16 / bf16 tensors through the typed
entry points; the Context records run through the client on device memory in
its fused, bulk and packet modes.

Comparison is bit-exact.  The one exception is the project's NaN rule: where
the reference recorded a NaN the GPU must give a NaN (gfx950's 0/0 is
0x7fc00000, x86's 0xffc00000), and at least 99 % of the positions of every
output are compared by bits (tests/ref_vectors.py: check_plane; the generator
asserts that bound on the reference's own output).

The reference leaves the words of a partial last block past numel as it
found them (asserted on the CPU in test_oracle_vs_reference.py); the C ABI
defines them as 0, asserted here.
"""
import numpy as np
import pytest

import ref_vectors as RV

pytestmark = pytest.mark.gpu

DOC = RV.load()


def ids(r):
    return r["name"]


def sw():
    import switchml_amd
    return switchml_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def used_exps(r):
    """The exponents the record's payload and output were produced under."""
    return None if r["global_exps"] is None else np.array(r["global_exps"], dtype=np.int8)


@pytest.mark.parametrize("r", DOC["ppp"], ids=ids)
def test_kernels_reproduce_ppp_record(cuda, r):
    import torch
    s = sw()
    x = RV.make_input(r["input"])
    P, W, n = r["P"], r["W"], r["n"]
    xd = dev(x, cuda)
    ge = used_exps(r)

    e2 = s.exponents(xd, P)                                   # K2
    p1, e1 = s.quantize_pack(xd, P, W)                        # K1, own exponents
    torch.cuda.synchronize()
    RV.check_plane(host(e2), r["exps"], 2, "K2 exponent plane")
    RV.check_plane(host(e1), r["exps"], 2, "K1 exponent plane")
    if ge is None:
        RV.check_plane(host(p1)[:n], r["payload"], 8, "K1 payload")
    assert not host(p1)[n:].any(), "K1: words past numel are defined as 0"

    g = e1 if ge is None else dev(ge, cuda)                   # K3 with the exponents the reference received
    p3, _ = s.quantize_pack(xd, P, W, global_exps=g)
    torch.cuda.synchronize()
    RV.check_plane(host(p3)[:n], r["payload"], 8, "K3 payload")
    assert not host(p3)[n:].any(), "K3: words past numel are defined as 0"

    s.loopback_aggregate(p3, W)                               # K5, then K4
    out = s.dequantize(p3, g, n, P, W)
    torch.cuda.synchronize()
    RV.check_plane(host(out), r["out"], 8, "K5 + K4 output")


OWN = [r for r in DOC["ppp"] if r["global_exps"] is None]


@pytest.mark.parametrize("r", OWN, ids=ids)
def test_round_trips_reproduce_ppp_record(cuda, r):
    import torch
    s = sw()
    x = RV.make_input(r["input"])
    P, W, n = r["P"], r["W"], r["n"]
    xd = dev(x, cuda)
    rt = s.roundtrip_loopback(xd, P, W)                       # fused
    torch.cuda.synchronize()
    RV.check_plane(host(rt), r["out"], 8, "fused round trip")

    # batched: the record between two other slices, all in one buffer (ragged starts)
    a, b = 1000 + 3, 257
    buf = torch.arange(a + n + b, dtype=torch.float32, device=cuda) * 0.37 - 100.0
    buf[a:a + n] = xd
    o = torch.full_like(buf, float("nan"))
    cuts = [(0, a), (a, n), (a + n, b)]
    s.roundtrip_loopback_batch([(buf[lo:lo + m], o[lo:lo + m]) for lo, m in cuts], P, W)
    torch.cuda.synchronize()
    RV.check_plane(host(o[a:a + n]), r["out"], 8, "batched round trip")
    for lo, m in (cuts[0], cuts[2]):
        want = s.roundtrip_loopback(buf[lo:lo + m].clone(), P, W)
        assert torch.equal(o[lo:lo + m].view(torch.int32), want.view(torch.int32)), "neighbour slice"


@pytest.mark.parametrize("r", OWN, ids=ids)
def test_burst_path_reproduces_ppp_record(cuda, r):
    """One sml_exchange_burst loop over the slice, driven as
    test_packets_gpu.py drives it: a ring of b slots in HBM, the packets of a
    burst shuffled, ProcessPacket x W inside the launch; the captured packets
    and the output against the record."""
    from test_packets_gpu import run_exchange
    from oracle import oracle as O          # num_blocks only (geometry; no oracle arithmetic)
    x = RV.make_input(r["input"])
    P, W, n = r["P"], r["W"], r["n"]
    B = O.num_blocks(n, P)
    ce, cp, out, b = run_exchange(x, P, W, r["batch"], "device", cuda, np.random.default_rng(n + P), 64, True)
    assert b == min(B, r["batch"])
    RV.check_plane(ce[:B], r["exps"], 2, "packet exponent bytes")
    RV.check_plane(cp[b:].reshape(-1)[:n], r["payload"], 8, "packet payloads")
    RV.check_plane(out, r["out"], 8, "burst path output")


@pytest.mark.parametrize("r", DOC["half"], ids=ids)
def test_typed_entry_points_reproduce_16_bit_record(cuda, r):
    """Inputs exactly representable in the 16-bit type: the planes are the
    recorded ones, the outputs the recorded fp32 outputs narrowed by torch on
    the CPU (round to nearest even)."""
    import torch
    from test_half_gpu import assert_half_equal, from_bits, narrow
    s = sw()
    T = r["input"]["type"]
    raw, x32 = RV.half_input(r["input"])
    x = from_bits(raw, T)
    assert np.array_equal(x.float().numpy().view(np.uint32), x32.view(np.uint32))
    P, W, n = r["P"], r["W"], r["n"]
    xd = x.to(cuda)
    payload, exps = s.quantize_pack(xd, P, W)
    e2 = s.exponents(xd, P)
    torch.cuda.synchronize()
    RV.check_plane(host(exps), r["exps"], 2, "K1h exponent plane")
    RV.check_plane(host(e2), r["exps"], 2, "K2h exponent plane")
    RV.check_plane(host(payload)[:n], r["payload"], 8, "K1h payload")
    p3, _ = s.quantize_pack(xd, P, W, global_exps=exps)
    RV.check_plane(host(p3)[:n], r["payload"], 8, "K3h payload")

    y32 = RV.unhex(r["out"]["hex"], 8).view(np.float32)
    want = narrow(y32, T)
    s.loopback_aggregate(payload, W)
    assert_half_equal(s.dequantize(payload, exps, n, P, W, out_dtype=x.dtype), want)
    assert_half_equal(s.roundtrip_loopback(xd, P, W), want)
    o = torch.empty_like(xd)                                  # batched: one slice among two others
    before, after = xd[:70].clone(), xd[3:].clone()
    s.roundtrip_loopback_batch([(before, torch.empty_like(before)), (xd, o), (after, torch.empty_like(after))], P, W)
    torch.cuda.synchronize()
    assert_half_equal(o, want)
    # and the fp32 output of the same widened input is the record itself
    RV.check_plane(host(s.roundtrip_loopback(dev(x32, cuda), P, W)), r["out"], 8, "fp32 round trip")


@pytest.fixture
def C(cuda):
    from switchml_amd import client
    yield client
    if client.state() == client.RUNNING:
        client.stop()


@pytest.mark.parametrize("mode", ["fused", "bulk", "packet"])
@pytest.mark.parametrize("r", DOC["context"], ids=ids)
def test_client_reproduces_context_record(C, r, mode):
    """The reference's Context::AllReduce result (dummy backend) through the
    project's client on device memory."""
    import torch
    x = RV.make_input(r["input"])
    C.start(C.make_config(num_workers=r["W"], num_worker_threads=r["T"], packet_numel=r["P"],
                          max_outstanding_packets=r["mop"], bandwidth=0, process_packets=r["process_packets"],
                          mode=mode))
    xd = torch.from_numpy(x.copy()).cuda()
    if r["inplace"]:
        C.allreduce(xd)
        got = xd
    else:
        got = torch.zeros_like(xd)
        C.allreduce(xd, got)
        torch.cuda.synchronize()
        assert np.array_equal(host(xd).view(np.uint32), x.view(np.uint32)), "input changed"
    torch.cuda.synchronize()
    C.stop()
    RV.check_plane(host(got), r["out"], 8, f"client {mode}")
