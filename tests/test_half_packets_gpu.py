"""GPU tests of FLOAT16 / BFLOAT16 slices on the per-packet paths: the typed
burst entry points (sml_preprocess_burst_typed / sml_postprocess_burst_typed /
sml_exchange_burst_typed, csrc/sml_packets.hip), the client's packet mode
under backend.hip.half_packets, and the CollNet plugin on top of it.

The driver is the dummy packet loop of test_packets_gpu.py (ring of b slots
in HBM or pinned memory, the packets of each pass shuffled, bursts of at most
`cap` packets, ProcessPacket inside the launch or as a separate launch) for a
tensor of any element type.  The slice starts on an odd element of its
buffer and the output three elements into a buffer prefilled with a non-NaN
sentinel, whose elements before and after the output must survive.

Expectation: the packets — exponent bytes, payload words —
are those of the FLOAT32 slice of the widened values, byte for byte, and the
output is the oracle's fp32 output narrowed by torch on the CPU (round to
nearest even), compared by bits; an expected NaN would accept any NaN, but
none of these inputs gives one, which the tests assert."""
import ctypes

import numpy as np
import pytest

import ref_vectors as RV
from oracle import oracle as O
from test_collnet_plugin import run_driver
from test_half_client_gpu import CASES, N, assert_half_equal, bits_of, expected, make, tdtype

pytestmark = pytest.mark.gpu

DOC = RV.load()
SENT16, SENT32, SLOT = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A     # finite in every type; a slot's words before any packet


def sw():
    import switchml_amd as s
    s.lib()
    return s


def raw(t):
    """A tensor's bytes as unsigned words of its element size (numpy, host)."""
    import torch
    t = t.detach().cpu().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def filled(m, dtype, device):
    """m elements of dtype holding the sentinel bit pattern."""
    import torch
    if dtype in (torch.float16, torch.bfloat16):
        return torch.full((m,), SENT16, dtype=torch.int16, device=device).view(dtype)
    return torch.full((m,), SENT32, dtype=torch.int32, device=device).view(dtype)


def typed_entry(s):
    return {"pre": s.preprocess_burst, "post": s.postprocess_burst, "exchange": s.exchange_burst}


def untyped_entry(s):
    L = s.lib()

    def call(fn):
        def run(bt, stream):
            assert fn(ctypes.byref(bt), ctypes.c_void_p(stream.cuda_stream)) == s.SML_OK
        return run
    return {"pre": call(L.sml_preprocess_burst), "post": call(L.sml_postprocess_burst),
            "exchange": call(L.sml_exchange_burst)}


def run_loop(x, P, W, b_max, ring_place, cuda, rng, cap=64, proc=True, form="exchange", inplace=False, flags=0,
             entry=None):
    """The dummy packet loop over the float slice x (a host tensor of any float
    type): form "exchange" is run_exchange of test_packets_gpu.py (one exchange
    burst per received packet; ProcessPacket x W inside it when `proc`, else a
    separate loopback_aggregate), form "bursts" its run_bursts (separate
    postprocess and preprocess launches).  Returns the captured exponent
    bytes and payload words of every packet as sent, the output tensor, b, and
    the final ring, extra slots and received exponents."""
    import torch
    s = sw()
    entry = entry or typed_entry(s)
    n = x.numel()
    B = O.num_blocks(n, P)
    b = min(B, b_max)
    total = B + b
    base = filled(n + 2, x.dtype, cuda)
    base[1:1 + n] = x.to(cuda)
    xd = base[1:1 + n]                        # starts on an odd element
    obuf = None if inplace else filled(n + 6, x.dtype, cuda)
    out = xd if inplace else obuf[3:3 + n]
    assert xd.data_ptr() % (2 * x.element_size()) != 0
    recv = torch.zeros(B, dtype=torch.int8, device=cuda)
    if ring_place == "device":
        ring = torch.full((b * P,), SLOT, dtype=torch.int64, device=cuda).to(torch.int32)
        extra = torch.zeros(b * 2, dtype=torch.uint8, device=cuda)
    else:
        ring = torch.full((b * P,), SLOT, dtype=torch.int64).to(torch.int32).pin_memory()
        extra = torch.zeros(b * 2, dtype=torch.uint8).pin_memory()
    rbase, ebase = ring.data_ptr(), extra.data_ptr()
    cap_e = np.zeros(total, dtype=np.int8)
    cap_p = np.zeros((total, P), dtype=np.uint32)
    stream = torch.cuda.current_stream(cuda)
    in_kernel = proc and form == "exchange"

    def snapshot():
        return ring.cpu().numpy().view(np.uint32).reshape(b, P).copy()

    def processed(words):
        return O.bswap32((O.bswap32(words).astype(np.uint64) * W % (1 << 32)).astype(np.uint32))

    def capture(ids, before):
        rh = snapshot()
        eh = extra.cpu().numpy()
        for q in ids:
            sl = q % b
            cap_e[q] = eh[sl * 2].astype(np.int8) if q < B else 0
            if q >= b:
                m = min(P, n - (q - b) * P)
                cap_p[q, :m] = rh[sl, :m]
                assert np.array_equal(rh[sl, m:], before[sl, m:]), "words past a partial block's real ones rewritten"

    def bursts(op, ids, fl=flags):
        ids = list(ids)
        rng.shuffle(ids)                                       # a burst's packets in any order
        for i0 in range(0, len(ids), cap):
            part = ids[i0:i0 + cap]
            slots = [q % b for q in part]
            bt = s.packet_burst(xd, out, P, W, b, recv, part, [rbase + sl * P * 4 for sl in slots],
                                [ebase + sl * 2 for sl in slots], flags=fl)
            entry[op](bt, stream)
        torch.cuda.synchronize()

    prev = snapshot()
    bursts("pre", range(b))
    capture(range(b), prev)
    for p0 in range(0, total, b):
        w = min(b, total - p0)
        if W != 1 and not in_kernel:                           # ProcessPacket x W (dummy_backend.cc:72-84)
            s.loopback_aggregate(ring.view(torch.int32)[: w * P], W)
        torch.cuda.synchronize()
        nxt = [q + b for q in range(p0, p0 + w) if q + b < total]
        if form == "exchange":
            before = processed(snapshot()) if in_kernel else snapshot()
            bursts("exchange", range(p0, p0 + w), flags | (s.FLAG_PROCESS_PACKET if in_kernel else 0))
        else:
            bursts("post", range(p0, p0 + w))
            before = snapshot()
            bursts("pre", nxt)
        capture(nxt, before)
    # nothing outside the slice and the output was written
    sent = SENT16 if x.element_size() == 2 else SENT32
    assert raw(base[:1])[0] == sent and raw(base[1 + n:])[0] == sent, "an element next to the slice was written"
    if not inplace:
        assert (raw(obuf[:3]) == sent).all() and (raw(obuf[3 + n:]) == sent).all(), "written outside the output"
        assert np.array_equal(raw(xd), raw(x)), "the slice was written"
    return dict(pe=cap_e, pp=cap_p, out=out.detach().cpu().clone(), b=b, ring=snapshot(), extra=extra.cpu().numpy(),
                recv=recv.cpu().numpy())


def make_input(T, n, W):
    """N(0, 1) scaled by 2^(W % 4 - 2) in the type; from 2001 elements on with
    the special bit patterns of test_half_client_gpu.make."""
    import torch
    x = torch.from_numpy(O.splitmix_normal(n % 89, n) * np.float32(2.0 ** (W % 4 - 2))).to(tdtype(T))
    if n < 2001:
        return x
    b = bits_of(x).copy()
    b[5:40] = 0
    b[100:110] = 0x7BFF if T == "fp16" else 0x7F7F
    b[300:330] = np.arange(1, 31, dtype=np.uint16)
    b[1000] = 0x7C00 if T == "fp16" else 0x7F80
    b[2000] = 0x7E00 if T == "fp16" else 0x7FC0
    return torch.from_numpy(b.view(np.int16)).view(tdtype(T))


REFS = {}


def reference(T, n, W, P, b_max):
    """(input, oracle packet exponents, payloads, expected output, b): the
    packet stream of the widened fp32 slice, computed once per case."""
    import torch
    key = (T, n, W, P, b_max)
    if key not in REFS:
        x = make_input(T, n, W)
        pe, pp, ref_out, b = O.dummy_packet_stream(x.float().numpy(), P, b_max, W)
        want = torch.from_numpy(ref_out).to(x.dtype)
        assert not torch.isnan(want).any()                     # so every position is compared by bits
        REFS[key] = (x, pe, pp, want, b)
    return REFS[key]


def check_against_stream(got, T, n, W, P, b_max):
    x, pe, pp, want, b = reference(T, n, W, P, b_max)
    assert got["b"] == b
    assert np.array_equal(got["pe"], pe)
    assert np.array_equal(got["pp"], pp.view(np.uint32))
    assert got["out"].dtype == want.dtype
    assert np.array_equal(raw(got["out"]), raw(want))          # every position, by bits
    assert np.array_equal(got["recv"], pe[:got["recv"].size])


@pytest.mark.parametrize("P,W,n,b_max,ring,cap,proc", [
    (64, 2, 12_345, 50, "pinned", 17, True),
    (128, 1, 777, 64, "device", 5, True),           # B < b_max: b = B
    (256, 3, 20_011, 16, "device", 64, True),
    (256, 1, 255, 64, "pinned", 64, False),         # one partial block, the last group cut
    (512, 3, 513, 64, "pinned", 64, False),
    (1024, 8, 20_011, 7, "device", 64, False),
    (1024, 5, 4_099, 16, "pinned", 7, True),
    (256, 2, 1, 64, "device", 64, True),            # one element
    (64, 3, 67, 64, "device", 64, True),
])
@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_typed_exchange_loop_equals_widened_fp32_stream(cuda, T, P, W, n, b_max, ring, cap, proc):
    rng = np.random.default_rng(P * 7 + W + n)
    x = reference(T, n, W, P, b_max)[0]
    got = run_loop(x, P, W, b_max, ring, cuda, rng, cap, proc)
    check_against_stream(got, T, n, W, P, b_max)


@pytest.mark.parametrize("P,W,n", [(256, 3, 20_011), (64, 2, 67)])
@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_typed_pre_and_post_bursts_equal_widened_fp32_stream(cuda, T, P, W, n):
    """The same through sml_preprocess_burst_typed and
    sml_postprocess_burst_typed as separate launches."""
    rng = np.random.default_rng(P + W + n)
    x = reference(T, n, W, P, 16)[0]
    got = run_loop(x, P, W, 16, "pinned" if P == 64 else "device", cuda, rng, 11, form="bursts")
    check_against_stream(got, T, n, W, P, 16)


@pytest.mark.parametrize("P,W,n,ring", [(256, 3, 20_011, "device"), (1024, 5, 4_099, "pinned")])
@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_typed_exchange_loop_in_place(cuda, T, P, W, n, ring):
    """out is in: a block is read (its exponent, then its words, one window
    later) before the packet that carries its result comes back."""
    rng = np.random.default_rng(P + n)
    x = reference(T, n, W, P, 16)[0]
    got = run_loop(x, P, W, 16, ring, cuda, rng, 64, True, inplace=True)
    check_against_stream(got, T, n, W, P, 16)


def tie_input(T, n, P, W):
    """Every block holds 2^15 (exponent 16, scale ~ 2^15 / W) and elements
    +-W (2m + 1) 2^-16, m <= 42: W (2m + 1) <= 255 is exact in both types, and
    x * scale is m + 0.5 exactly in fp32 (for W = 3 the product's excess over
    m + 0.5 is below half an ulp), so every such element is a rounding tie."""
    import torch
    rng = np.random.default_rng(n + W)
    m = rng.integers(0, 43, n)
    x = (W * (2 * m + 1)) * 2.0 ** -16 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    x[::P] = 2.0 ** 15
    t = torch.from_numpy(x.astype(np.float32)).to(tdtype(T))
    assert np.array_equal(t.float().numpy(), x.astype(np.float32))      # exact in the type
    return t


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_typed_exchange_round_rne(cuda, T, W):
    """SML_FLAG_ROUND_RNE on tie-heavy input: the VCL=1 build's result
    (nearest even on each block's 16-element body), which differs from the
    VCL=0 one."""
    import torch
    s = sw()
    P, n, b_max = 256, 4_099, 16
    x = tie_input(T, n, P, W)
    x32 = x.float().numpy()
    kw = dict(P=P, max_outstanding_packets=b_max, num_worker_threads=1, num_workers=W)
    want = torch.from_numpy(O.dummy_allreduce(x32, vcl=True, **kw)).to(x.dtype)
    away = torch.from_numpy(O.dummy_allreduce(x32, **kw)).to(x.dtype)
    assert not torch.isnan(want).any() and not np.array_equal(raw(want), raw(away))
    got = run_loop(x, P, W, b_max, "device", cuda, np.random.default_rng(W), 64, True, flags=s.FLAG_ROUND_RNE)
    assert np.array_equal(raw(got["out"]), raw(want))
    assert not np.array_equal(raw(got["out"]), raw(away))


@pytest.mark.parametrize("r", DOC["half"], ids=lambda r: r["name"])
def test_typed_exchange_loop_reproduces_16_bit_record(cuda, r):
    """Results recorded from the compiled reference on the widened input: the
    packets carry the recorded exponent and payload planes, the output is the
    recorded fp32 output narrowed on the CPU."""
    from test_half_gpu import from_bits, narrow
    T, P, W, n = r["input"]["type"], r["P"], r["W"], r["n"]
    bits, x32 = RV.half_input(r["input"])
    x = from_bits(bits, T)
    assert np.array_equal(x.float().numpy().view(np.uint32), x32.view(np.uint32))
    got = run_loop(x, P, W, r["batch"], "device", cuda, np.random.default_rng(n), 64, True)
    B, b = O.num_blocks(n, P), got["b"]
    RV.check_plane(got["pe"][:B], r["exps"], 2, "packet exponent bytes")
    payload = got["pp"][b:].reshape(-1)[:n]                   # packet q carries block q - b
    RV.check_plane(payload, r["payload"], 8, "packet payload words")
    y32 = RV.unhex(r["out"]["hex"], 8).view(np.float32)
    assert_half_equal(got["out"], narrow(y32, T))


def test_typed_entry_points_equal_untyped_for_float32_and_int32(cuda):
    """A FLOAT32 slice and an INT32 slice through the typed entry points and
    through the untyped ones: the same ring, extra slots, received exponents
    and output, byte for byte."""
    import torch
    s = sw()
    P, W, n, b_max = 256, 3, 4_099, 8
    x = torch.from_numpy(O.splitmix_normal(31, n))
    runs = [run_loop(x, P, W, b_max, "device", cuda, np.random.default_rng(5), 5, True, entry=e)
            for e in (typed_entry(s), untyped_entry(s))]
    for k in ("pe", "pp", "ring", "extra", "recv"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert np.array_equal(raw(runs[0]["out"]), raw(runs[1]["out"]))
    ref = O.dummy_packet_stream(x.numpy(), P, b_max, W)[2]
    assert np.array_equal(raw(runs[0]["out"]), ref.view(np.uint32))

    # INT32: packet q carries block q; the first b packets, then every received
    # packet is post-processed and its buffer refilled with block q + b
    xi = np.random.default_rng(7).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    xd = torch.from_numpy(xi).to(cuda)
    B, b = O.num_blocks(n, P), 4
    stream = torch.cuda.current_stream(cuda)
    got = []
    for entry in (typed_entry(s), untyped_entry(s)):
        outd = filled(n, torch.int32, cuda)
        ring = torch.full((b * P,), SLOT, dtype=torch.int64, device=cuda).to(torch.int32)
        first = list(range(b))
        entry["pre"](s.packet_burst(xd, outd, P, W, 0, None, first, [ring.data_ptr() + q * P * 4 for q in first],
                                    [0] * b), stream)
        for p0 in range(0, B, b):
            ids = list(range(p0, min(p0 + b, B)))
            entry["exchange"](s.packet_burst(xd, outd, P, W, b, None, ids,
                                             [ring.data_ptr() + (q % b) * P * 4 for q in ids], [0] * len(ids),
                                             flags=s.FLAG_PROCESS_PACKET), stream)
        torch.cuda.synchronize()
        got.append((raw(ring), raw(outd)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][1].view(np.int32), (xi.astype(np.int64) * W).astype(np.int32))


@pytest.fixture
def C(cuda):
    from switchml_amd import client
    yield client
    if client.state() == client.RUNNING:
        client.stop()


def allreduce_everywhere(C, x, exp, T_, P):
    """Device, pinned-host and pageable-host tensors, each in place and not;
    the packet count of a job, and the input of a not-in-place job kept."""
    import torch
    xd = x.cuda()
    od = torch.zeros_like(xd)
    C.wait_for_all_jobs()
    before = C.stats()["packets"]
    C.allreduce(xd, od)
    assert_half_equal(od, exp)
    C.wait_for_all_jobs()
    blocks = [O.num_blocks(O.slice_geometry(x.numel(), T_, t)[1], P) for t in range(T_)]
    assert C.stats()["packets"] - before == sum(B + min(B, 64) for B in blocks)
    assert np.array_equal(bits_of(xd), bits_of(x))            # input untouched
    C.allreduce(xd)                                           # in place
    assert_half_equal(xd, exp)
    hx = x.clone().pin_memory()
    ho = torch.zeros_like(hx).pin_memory()
    C.allreduce(hx, ho)
    assert_half_equal(ho, exp)
    assert np.array_equal(bits_of(hx), bits_of(x))
    C.allreduce(hx)
    assert_half_equal(hx, exp)
    px = x.clone()
    po = torch.zeros_like(px)
    C.allreduce(px, po)
    assert_half_equal(po, exp)
    assert np.array_equal(bits_of(px), bits_of(x))
    C.allreduce(px)
    assert_half_equal(px, exp)


def other_types_still_run(C, T_, W, P):
    """One fp32 job and one INT32 job in the same context."""
    f = O.splitmix_normal(9, N)
    out = np.empty_like(f)
    C.allreduce(f, out)
    ref = O.dummy_allreduce(f, P=P, max_outstanding_packets=64 * T_, num_worker_threads=T_, num_workers=W)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    i = np.arange(-N // 2, N - N // 2, dtype=np.int32) * 77_777
    io = np.zeros_like(i)
    C.allreduce(i, io)
    assert np.array_equal(io, (i.astype(np.int64) * W).astype(np.int32))


@pytest.mark.parametrize("ring", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("T_,W,P", CASES)
@pytest.mark.parametrize("typ", ["fp16", "bf16"])
def test_client_packet_mode_runs_16_bit_jobs_with_the_key(C, typ, T_, W, P, ring):
    C.start(C.make_config(num_workers=W, num_worker_threads=T_, packet_numel=P, max_outstanding_packets=64 * T_,
                          bandwidth=0, mode="packet", half_packets=True, packet_ring=ring))
    assert "half_packets = true" in C.config_text()
    x = make(typ, N, seed=T_ * 10 + W)
    allreduce_everywhere(C, x, expected(x, T_, W, P), T_, P)
    other_types_still_run(C, T_, W, P)
    C.stop()


@pytest.mark.parametrize("kw", [dict(packet_ring="pinned", burst_server=True), dict(vcl=True)],
                         ids=["burst_server", "vcl"])
def test_client_packet_mode_16_bit_jobs_with_burst_server_and_vcl(C, kw):
    """burst_server = true serves the FLOAT32 and INT32 slices of the context,
    a 16-bit slice takes launches; vcl = true gives the VCL=1 build's
    rounding."""
    T_, W, P = 3, 2, 64
    C.start(C.make_config(num_workers=W, num_worker_threads=T_, packet_numel=P, max_outstanding_packets=64 * T_,
                          bandwidth=0, mode="packet", half_packets=True, **kw))
    for typ in ("bf16", "fp16"):
        x = make(typ, N, seed=41)
        allreduce_everywhere(C, x, expected(x, T_, W, P, vcl=bool(kw.get("vcl"))), T_, P)
    if not kw.get("vcl"):
        other_types_still_run(C, T_, W, P)
    C.stop()


def test_plugin_allreduce_bf16_device_in_packet_mode(cuda):
    """Through the CollNet table as RCCL's proxy calls it, under mode = packet
    with half_packets = true: a device bf16 buffer (ncclBfloat16 = 9), size ==
    2 * count, bits equal to the recipe."""
    body = '''
import torch
from oracle import oracle as O
T, W, P, n = 4, 2, 256, 20011
def expected(x):
    x32 = x.float().numpy(); y32 = np.empty_like(x32)
    for t in range(T):
        off, m = O.slice_geometry(n, T, t)
        y32[off:off + m] = O.dummy_allreduce(x32[off:off + m], P=P, max_outstanding_packets=64, num_worker_threads=1,
                                             num_workers=W)
    return torch.from_numpy(y32).to(x.dtype)
sup2 = {}
for dt in (6, 9):
    s = ctypes.c_int(); tbl.reduceSupport(dt, 0, ctypes.byref(s)); sup2[str(dt)] = s.value
out["support2"] = sup2
xb = torch.from_numpy(O.splitmix_normal(21, n)).to(torch.bfloat16)
xd = xb.cuda(); od = torch.zeros_like(xd)
out["dev_size"] = run(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(od.data_ptr()), n, 9)
exp = expected(xb)
out["no_nan"] = not bool(torch.isnan(exp).any())
out["dev_ok"] = bool(torch.equal(od.cpu().view(torch.int16), exp.view(torch.int16)))
out["dev_send_untouched"] = bool(torch.equal(xd.cpu().view(torch.int16), xb.view(torch.int16)))
'''
    ini = ("[general]\nnum_workers = 2\nnum_worker_threads = 4\npacket_numel = 256\n"
           "max_outstanding_packets = 256\n[backend.dummy]\nbandwidth = 0\n[backend.hip]\nmode = packet\n"
           "half_packets = true\n")
    out = run_driver(body, ini, preload="import torch")
    assert out["init"] == 0 and out["support2"] == {"6": 1, "9": 1}
    assert out["dev_size"] == 2 * 20011 and out["no_nan"] and out["dev_ok"] and out["dev_send_untouched"]
