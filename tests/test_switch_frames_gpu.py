"""GPU tests of the frame switch (sml_frame_switch / switchml_amd.FrameSwitch,
DESIGN §9 F3 "Switch side"): every call's verdicts, counts, result frames and
the sentinel-prefilled positions without a result are compared, bit for bit,
with the sequential model of tests/switch_frames_model.py."""
import numpy as np
import pytest

import switch_frames_model as M
from oracle import oracle as O
from switchml_amd import frame_wire as FW

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture(scope="module")
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


class Pair:
    """The GPU switch and the model, side by side, over the same workers."""

    def __init__(self, sw, W, S, P):
        self.sw, self.W, self.S, self.P = sw, W, S, P
        self.workers = M.default_workers(W)
        self.gpu = sw.FrameSwitch(self.workers, S, P, switch_mac=M.SWITCH_MAC, switch_ip=M.SWITCH_IP)
        self.model = M.SwitchModel(self.workers, S, P)
        self.counts = np.zeros(5, dtype=np.int64)

    def reset(self):
        self.gpu.reset()
        self.model.reset()

    def run_gpu(self, frames, stride=None, out_stride=None, pinned=False):
        """`frames`: a list of uint8 arrays.  Returns (verdicts, out bytes)."""
        import torch
        fb = M.frame_bytes(self.P)
        stride = stride or fb
        out_stride = out_stride or stride
        n = len(frames)
        buf = np.full(n * stride, 0xC3, dtype=np.uint8)             # bytes between frames are not the switch's
        for i, f in enumerate(frames):
            buf[i * stride:i * stride + fb] = f
        if pinned:
            d_in = torch.from_numpy(buf).pin_memory()
            d_out = torch.full((n * out_stride,), SENTINEL, dtype=torch.uint8).pin_memory()
        else:
            d_in = torch.from_numpy(buf).cuda()
            d_out = torch.full((n * out_stride,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_verdict = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        out, verdict, counts = self.gpu(d_in, n, out=d_out, stride=stride, out_stride=out_stride, verdict=d_verdict)
        torch.cuda.synchronize()
        return verdict.cpu().numpy(), out.cpu().numpy(), counts.cpu().numpy()

    def check(self, frames, **kw):
        """One call on both; everything compared.  Returns (verdicts, results)."""
        fb = M.frame_bytes(self.P)
        out_stride = kw.get("out_stride") or kw.get("stride") or fb
        verdicts, results, counts = M.model_call(self.model, frames)
        self.counts += np.array(counts, dtype=np.int64)
        got_v, got_out, got_counts = self.run_gpu(frames, **kw)
        assert got_v.tolist() == verdicts.tolist()
        assert got_counts.tolist() == self.counts.tolist()
        got_out = got_out.reshape(len(frames), out_stride)
        for i in range(len(frames)):
            if i in results:
                assert verdicts[i] in (M.BROADCAST, M.RETRANSMIT)
                bad = np.flatnonzero(got_out[i, :fb] != results[i])
                assert bad.size == 0, (i, int(verdicts[i]), bad[:8].tolist())
                assert np.all(got_out[i, fb:] == SENTINEL), i
            else:
                assert np.all(got_out[i] == SENTINEL), (i, int(verdicts[i]))
        return verdicts, results


def aggregate(frames_of_packet):
    """The wire bytes from the exponents on of W frames' aggregate, by the oracle's plane-level switch."""
    words = O.switch_payload([f[FW.HEADER_BYTES:].copy().view(np.uint32) for f in frames_of_packet])
    e0 = O.switch_exps([f[FW.EXP].copy().view(np.int8) for f in frames_of_packet])
    e1 = O.switch_exps([f[FW.EXP2].copy().view(np.int8) for f in frames_of_packet])
    return np.concatenate([e0.view(np.uint8), e1.view(np.uint8), words.view(np.uint8)])


def test_slot_reuse_overwrites(sw):
    """W = 3, P = 64, num_slots = mop = 4, packets 0 .. 2 mop + 2, a window per
    call: packets 8, 9, 10 are the third use of slots 0-2 (set 0 again) and must
    carry their own sum, not one added to packet 0-2's."""
    rng = np.random.default_rng(1)
    mop = 4
    pair = Pair(sw, 3, mop, 64)
    for k in range(3):
        packets = list(range(k * mop, min((k + 1) * mop, 2 * mop + 3)))
        frames = M.window_frames(rng, pair.P, pair.workers, mop, packets)
        verdicts, results = pair.check(frames)
        assert int(np.sum(verdicts == M.BROADCAST)) == len(packets)
        for i, r in results.items():
            p = FW.get(r, FW.PKT_ID)
            same = [f for f in frames if FW.get(f, FW.PKT_ID) == p]
            assert np.array_equal(r[FW.EXP.start:], aggregate(same)), p


def test_bytes_the_switch_ignores_are_random(sw):
    """W = 2, S = mop = 4, P = 64, one window of 8 frames, then the same 8 again
    as retransmissions.  worker_frame() leaves most of the header zero, which
    a mask reaching into a neighbouring byte would not notice; here every byte
    the switch does not read is random per frame (the destination MAC to the
    header checksum, the UDP length to the job, the tsi, bit 14 of the pool
    index), the job type byte's high bits included, and the model builds its
    results from the same bytes."""
    rng = np.random.default_rng(14)
    mop = 4
    pair = Pair(sw, 2, mop, 64)
    frames = M.window_frames(rng, pair.P, pair.workers, mop, range(mop))
    assert len(frames) == 8
    for f in frames:
        for ignored in (FW.span(FW.DST_MAC, FW.IP_CHECKSUM), FW.span(FW.UDP_LEN, FW.PKT_ID)):
            f[ignored] = rng.integers(0, 256, ignored.stop - ignored.start, dtype=np.uint8)
        FW.put(f, FW.POOL_INDEX, FW.get(f, FW.POOL_INDEX) | int(rng.integers(0, 2)) * FW.POOL_BIT14)
    assert any(FW.get(f, FW.JOB_TYPE_SIZE) & 0xe8 for f in frames)
    assert any(FW.get(f, FW.POOL_INDEX) & FW.POOL_BIT14 for f in frames)
    verdicts, results = pair.check(frames)
    assert int(np.sum(verdicts == M.BROADCAST)) == mop and int(np.sum(verdicts == M.CONSUMED)) == mop
    for i, r in results.items():
        assert FW.get(r, FW.JOB_TYPE_SIZE) == 0x10 | (FW.get(frames[i], FW.JOB_TYPE_SIZE) & 7)
        assert not FW.get(r, FW.POOL_INDEX) & FW.POOL_BIT14
        assert FW.get(r, FW.span(FW.JOB, FW.PKT_ID)) == FW.get(frames[i], FW.span(FW.JOB, FW.PKT_ID))
    verdicts, results = pair.check(frames)
    assert np.all(verdicts == M.RETRANSMIT) and len(results) == 8


@pytest.mark.parametrize("P", [64, 256, 1024])
@pytest.mark.parametrize("W", [2, 16, 32])
def test_partial_slots_across_calls(sw, P, W):
    """One window (mop = 2, workers interleaved and shuffled) cut into two
    calls at every position: a slot part-filled by one call is completed by the
    next."""
    rng = np.random.default_rng(100 * W + P)
    mop = 2
    pair = Pair(sw, W, mop, P)
    frames = M.window_frames(rng, pair.P, pair.workers, mop, range(mop))
    for cut in range(len(frames) + 1):
        pair.reset()
        total = 0
        for part in (frames[:cut], frames[cut:]):
            if part:
                verdicts, _ = pair.check(part)
                total += int(np.sum(verdicts == M.BROADCAST))
        assert total == mop, cut


def test_duplicates(sw):
    rng = np.random.default_rng(3)
    P, mop = 64, 2
    pair = Pair(sw, 3, mop, P)
    A, B, C = pair.workers
    pay = rng.integers(0, 256, (3, 4 * P), dtype=np.uint8)

    def fr(w, p, port=None):
        return M.worker_frame(P, pair.workers[w], p, M.pool_index(p, mop), pay[w], (w, 9 - w),
                              src_port=port or 4000 + w)

    # before completion -> CONSUMED; after completion in the same call -> RETRANSMIT, to the asker, with its ports
    verdicts, results = pair.check([fr(0, 0), fr(0, 0), fr(1, 0), fr(1, 0, port=777), fr(2, 0), fr(0, 0, port=555),
                                    fr(1, 0, port=666)])
    assert verdicts.tolist() == [0, 0, 0, 0, 1, 2, 2]
    assert FW.get(results[5], FW.DST_MAC) == A[0] and FW.get(results[5], FW.DST_PORT) == 555
    assert FW.get(results[6], FW.DST_MAC) == B[0] and FW.get(results[6], FW.DST_PORT) == 666
    assert np.array_equal(results[5][FW.EXP.start:], results[4][FW.EXP.start:])
    # in a later call
    verdicts, results = pair.check([fr(2, 0, port=444)])
    assert verdicts.tolist() == [2] and FW.get(results[0], FW.DST_MAC) == C[0]
    # the other workers move to the slot's other set: C's late question is still answered
    verdicts, _ = pair.check([fr(0, mop), fr(1, mop)])
    assert verdicts.tolist() == [0, 0]
    verdicts, results = pair.check([fr(2, 0)])
    assert verdicts.tolist() == [2]
    # ... and its own move completes the other set
    verdicts, _ = pair.check([fr(2, mop), fr(0, mop)])
    assert verdicts.tolist() == [1, 2]


def test_single_worker_answers_every_duplicate(sw):
    rng = np.random.default_rng(4)
    P, mop = 128, 2
    pair = Pair(sw, 1, mop, P)
    f = [M.worker_frame(P, pair.workers[0], p, M.pool_index(p, mop), rng.integers(0, 256, 4 * P, dtype=np.uint8), (p, 0))
         for p in range(4)]
    verdicts, results = pair.check([f[0], f[0], f[1], f[0]])
    assert verdicts.tolist() == [1, 2, 1, 2]
    assert np.array_equal(results[3][FW.EXP.start:], f[0][FW.EXP.start:])
    verdicts, _ = pair.check([f[1], f[2], f[2], f[3]])
    assert verdicts.tolist() == [2, 1, 2, 4]                    # f[3]: slot 1's other set, after f[1] in this call
    verdicts, _ = pair.check([f[3], f[3]])
    assert verdicts.tolist() == [1, 2]


def test_deferral(sw):
    """Both sets of a (slot, worker) in one call: the later set is DEFERRED,
    the registers do not see it, and resubmitting gives what the split stream
    gives."""
    rng = np.random.default_rng(5)
    P, mop = 64, 2
    pair = Pair(sw, 2, mop, P)
    split = Pair(sw, 2, mop, P)
    pay = rng.integers(0, 256, (2, 4, 4 * P), dtype=np.uint8)

    def fr(w, p):
        return M.worker_frame(P, pair.workers[w], p, M.pool_index(p, mop), pay[w, p], (p, w))

    call = [fr(0, 0), fr(1, 0), fr(0, 2), fr(1, 2), fr(0, 1)]
    verdicts, _ = pair.check(call)
    assert verdicts.tolist() == [0, 1, 4, 4, 0]
    assert pair.model.bitmap[0] == [3, 0]                       # set 1 of slot 0 untouched
    verdicts, results = pair.check([call[2], call[3], fr(1, 1)])
    assert verdicts.tolist() == [0, 1, 1]
    # the split stream: the same frames, the deferred ones in a call of their own
    split.check([call[0], call[1], call[4]])
    verdicts2, results2 = split.check([call[2], call[3], fr(1, 1)])
    assert verdicts2.tolist() == [0, 1, 1]
    assert all(np.array_equal(results[i], results2[i]) for i in (1, 2))


def test_ignored_frames(sw):
    rng = np.random.default_rng(6)
    P, S = 64, 3
    pair = Pair(sw, 2, S, P)
    pay = rng.integers(0, 256, 4 * P, dtype=np.uint8)
    stranger = (bytes([2, 0, 0, 0, 9, 9]), "10.0.9.9")
    frames = [M.worker_frame(P, pair.workers[0], 0, 0, pay),
              M.worker_frame(P, stranger, 0, 0, pay),                       # unknown source address
              M.worker_frame(P, pair.workers[1], 0, S, pay),                # slot >= num_slots
              M.worker_frame(P, pair.workers[1], 0, 0x8000 | 0x3fff, pay),  # ... in set 1
              M.worker_frame(P, pair.workers[1], 0, 0x4000, pay),           # bit 14 is not the slot's
              M.worker_frame(P, pair.workers[1], 0, 0, pay)]
    verdicts, results = pair.check(frames)
    assert verdicts.tolist() == [0, 3, 3, 3, 1, 2]
    assert pair.model.bitmap[0] == [3, 0] and FW.get(results[4], FW.POOL_INDEX) == 0


def test_arithmetic(sw):
    """Sums that cross +-2^31 wrap; exponents are signed (negative, -128), and
    the second exponent is maxed on its own."""
    P, mop = 64, 4
    pair = Pair(sw, 3, mop, P)
    words = np.zeros((3, P), dtype=np.uint32)
    words[0, :8] = [0x7fffffff, 0x80000000, 0xffffffff, 0x7fffffff, 0x80000000, 1, 0x40000000, 0xc0000000]
    words[1, :8] = [1, 0x80000000, 1, 0x7fffffff, 0xffffffff, 0xffffffff, 0x40000000, 0xc0000000]
    words[2, :8] = [0, 0x80000000, 0, 2, 0xffffffff, 0, 0x40000000, 0xc0000000]
    words[:, 8:] = np.random.default_rng(7).integers(0, 2 ** 32, (3, P - 8), dtype=np.uint64).astype(np.uint32)
    cases = [((-128, -128), (-128, -128), (-128, -128)), ((-5, 3), (-128, -7), (-9, -128)),
             ((127, -128), (-1, 0), (0, 127)), ((-128, 5), (-127, -128), (-128, -128))]
    frames = []
    for p, es in enumerate(cases):
        for w in range(3):
            frames.append(M.worker_frame(P, pair.workers[w], p, M.pool_index(p, mop),
                                         words[w].astype(">u4").view(np.uint8), es[w]))
    verdicts, results = pair.check(frames)
    assert int(np.sum(verdicts == M.BROADCAST)) == len(cases)
    for p, es in enumerate(cases):
        r = results[3 * p + 2]
        assert np.array_equal(FW.payload_words(r, P), words[0] + words[1] + words[2])
        assert r[FW.EXPS].copy().view(np.int8).tolist() == [max(e[0] for e in es), max(e[1] for e in es)]
    assert FW.payload_words(results[2], P)[0] == 0x80000000


@pytest.mark.parametrize("P,stride,out_stride,pinned", [
    (64, None, None, False), (64, 320, 384, False), (256, 1088, 1076, False), (256, 1076, 1152, True),
    (1024, 4160, 4148, True)])
def test_layout(sw, P, stride, out_stride, pinned):
    """Packed and 64-byte-aligned strides, out_stride != frame_stride, frames
    and results in pinned host memory."""
    rng = np.random.default_rng(P)
    mop = 3
    pair = Pair(sw, 4, mop, P)
    frames = M.window_frames(rng, pair.P, pair.workers, mop, range(mop))
    frames.insert(5, frames[0])
    verdicts, _ = pair.check(frames[:7], stride=stride, out_stride=out_stride, pinned=pinned)
    verdicts, _ = pair.check(frames[7:] + [frames[2]], stride=stride, out_stride=out_stride, pinned=pinned)
    assert int(np.sum(verdicts == M.BROADCAST)) >= 1


def test_unsupported_writes_nothing(sw):
    import ctypes
    import torch
    P = 64
    pair = Pair(sw, 2, 4, P)
    frames = M.window_frames(np.random.default_rng(8), pair.P, pair.workers, 4, range(2))
    fb = M.frame_bytes(P)
    d_in = torch.from_numpy(np.concatenate(frames)).cuda()
    d_out = torch.full((len(frames) * fb,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_verdict = torch.full((len(frames),), 0xEE, dtype=torch.uint8, device="cuda")
    state_before = pair.gpu.state.clone()
    for W, S, Pbad in [(33, 4, P), (2, 16385, P), (2, 4, 100), (33, 16385, 100)]:
        sp = sw.frame_switch_params(pair.workers, S, Pbad)
        sp.num_workers = W
        status = sw.lib().sml_frame_switch(ctypes.byref(sp), d_in.data_ptr(), len(frames), fb, pair.gpu.state.data_ptr(),
                                           d_out.data_ptr(), fb, d_verdict.data_ptr(), pair.gpu.counts.data_ptr(), None)
        assert status == sw.SML_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all()) and bool((d_verdict == 0xEE).all())
    assert torch.equal(pair.gpu.state, state_before) and pair.gpu.counts.tolist() == [0] * 5
    with pytest.raises(sw.SwitchMLError):
        sw.FrameSwitch(pair.workers, 16385, P)


@pytest.mark.parametrize("seed", range(20))
def test_lossy_streams(sw, seed):
    """The generator's closed loop (loss and duplication 0.1 each way, N = 40,
    mop = 8, P = 64) replayed call by call, the frames a call DEFERRED
    prepended to the next: every call matches the model.  The generator has
    checked that every worker got every packet's result from those calls; here
    every packet's BROADCAST — and every answer to a retransmission — carries
    the plane switch's aggregate of the W workers' packets."""
    W, N, mop, P = (2, 3, 8)[seed % 3], 40, 8, 64
    calls, payloads, exps = M.lossy_stream(1000 + seed, W, N, mop, P, q=0.1)
    pair = Pair(sw, W, mop, P)
    deferred, answered, ndeferred = [], set(), 0
    for fresh in calls:
        frames = deferred + fresh
        if not frames:
            continue
        verdicts, results = pair.check(frames)
        deferred = [frames[i] for i in range(len(frames)) if verdicts[i] == M.DEFERRED]
        ndeferred += len(deferred)
        for i, r in results.items():
            p = FW.get(r, FW.PKT_ID)
            sent = [M.worker_frame(P, pair.workers[w], p, M.pool_index(p, mop), payloads[w, p], exps[w, p])
                    for w in range(W)]
            assert np.array_equal(r[FW.EXP.start:], aggregate(sent)), (p, int(verdicts[i]))
            if verdicts[i] == M.BROADCAST:
                assert p not in answered
                answered.add(p)
    assert sorted(answered) == list(range(N))


# ------------------------------------------------------------------ end to end

def worker_params(sw, pair, w, mop, job):
    mac, ip = pair.workers[w]
    return sw.frame_params(dst_mac=M.SWITCH_MAC, src_mac=mac, src_ip=ip, dst_ip=M.SWITCH_IP, src_port=4000 + w,
                           dst_port=48879, job_id=job, pool_index_start=0, pool_index_shift=0,
                           max_outstanding_pkts=mop)


def switch_windows(pair, frame_sets, nframes, mop):
    """W workers' frame sets (device tensors, packed) through the GPU switch a
    window of mop packets per call.  Returns the BROADCAST result frames in
    pkt_id order as one device tensor, and their count."""
    import torch
    fb = M.frame_bytes(pair.P)
    sets = [f.view(-1, fb) for f in frame_sets]
    got = []
    for lo in range(0, nframes, mop):
        hi = min(lo + mop, nframes)
        call = torch.cat([s[lo:hi] for s in sets]).reshape(-1)
        n = (hi - lo) * len(sets)
        out, verdict, _ = pair.gpu(call, n)
        idx = torch.nonzero(verdict == M.BROADCAST).flatten()
        assert idx.numel() == hi - lo and int((verdict == M.CONSUMED).sum()) == n - (hi - lo)
        got.append(out.view(-1, fb)[idx])
    res = torch.cat(got)
    order = torch.argsort(res[:, FW.PKT_ID].contiguous().view(torch.int32).flatten())
    return res[order].contiguous().reshape(-1), res.shape[0]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_end_to_end_float(sw, dtype):
    """W = 3 workers' slices: frames with own exponents -> switch -> the global
    exponents from the results' exponent byte; frames quantized with those ->
    switch (after reset) -> every worker's receive loop.  The output is the
    dequantized plane-level oracle switch, bit for bit, on all three workers."""
    import torch
    P, W, mop, job = 64, 3, 4, 3
    n = 5 * P + 7
    B = O.num_blocks(n, P)
    tdt = getattr(torch, dtype)
    pair = Pair(sw, W, mop, P)
    xs = [(O.splitmix_normal(40 + w, n) * np.float32(4.0 ** w)).astype(np.float32) for w in range(W)]
    xd = [torch.from_numpy(x).cuda().to(tdt) for x in xs]
    xs = [x.float().cpu().numpy() for x in xd]                       # what the kernels widen to
    prm = [worker_params(sw, pair, w, mop, job) for w in range(W)]
    own = [sw.quantize_pack_frames(xd[w], prm[w], P, W, batch_max=mop) for w in range(W)]
    res, nres = switch_windows(pair, own, B + mop, mop)
    assert nres == B + mop
    fb = M.frame_bytes(P)
    gexp = res.view(-1, fb)[:B, FW.EXP.start].contiguous().view(torch.int8)
    want_exps = O.switch_exps([O.exponents(x, P) for x in xs])
    assert len({tuple(O.exponents(x, P).tolist()) for x in xs}) == W  # the workers' exponents differ
    assert np.array_equal(gexp.cpu().numpy(), want_exps)
    pair.gpu.reset()
    glob = [sw.quantize_pack_frames(xd[w], prm[w], P, W, batch_max=mop, global_exps=gexp) for w in range(W)]
    res, nres = switch_windows(pair, glob, B + mop, mop)
    payload = O.switch_payload([O.quantize(x, P, W, global_exps=want_exps) for x in xs])
    want = O.dequantize(payload, want_exps, n, P, W)
    if dtype != "float32":
        want = torch.from_numpy(want).to(tdt).view(torch.int16).numpy()
    for w in range(W):
        rx = sw.RxSlice(n, P, batch_max=mop, dtype=tdt)
        sw.dequantize_frames(res, nres, rx, num_workers=W, job_id=job)
        torch.cuda.synchronize()
        got = rx.out.cpu()
        got = got.view(torch.int16).numpy() if dtype != "float32" else got.numpy()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), w
        assert np.array_equal(rx.exps.cpu().numpy(), want_exps)
        assert rx.counts.tolist() == [nres, 0]


def test_end_to_end_int32(sw):
    import torch
    P, W, mop, job = 64, 2, 4, 9
    n = 5 * P + 7
    B = O.num_blocks(n, P)
    pair = Pair(sw, W, mop, P)
    rng = np.random.default_rng(11)
    xs = [rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) for _ in range(W)]
    prm = [worker_params(sw, pair, w, mop, job) for w in range(W)]
    sets = [sw.pack_frames_int32(torch.from_numpy(xs[w]).cuda(), prm[w], P) for w in range(W)]
    res, nres = switch_windows(pair, sets, B, mop)
    assert nres == B
    for w in range(W):
        rx = sw.RxSliceInt32(n, P)
        sw.unpack_frames_int32(res, nres, rx, job_id=job)
        torch.cuda.synchronize()
        assert np.array_equal(rx.out.cpu().numpy(), xs[0] + xs[1]), w       # int32 addition wraps
