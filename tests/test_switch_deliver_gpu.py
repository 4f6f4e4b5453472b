"""GPU tests of the wire on both sides of the frame switch
(sml_frame_switch_deliver / FrameSwitch.deliver, sml_frame_gather /
gather_frames; DESIGN §9 F3 "Switch side", Egress): rings, ring counts, the
four counts and gather outputs are compared byte for byte with the sequential
model of tests/switch_deliver_model.py; rings and gather destinations are
prefilled with a sentinel, so the bytes a call must not touch are compared
too."""
import numpy as np
import pytest

import switch_deliver_model as D
import switch_frames_model as M
from oracle import oracle as O
from switchml_amd import frame_wire as FW

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
# the kernels' constants (sml_switch_frames.hip): k_fd_count's workgroup takes
# kBlockThreads = 256 frames; k_fd_scan steps over kFdScanTile = 256 threads x
# kFdScanPer = 4 groups of kFdGroup = 64 frames.
COUNT_WORKGROUP_FRAMES = 256
SCAN_TILE_FRAMES = 256 * 4 * 64


@pytest.fixture(scope="module")
def sw(cuda):
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


class Rings:
    """W rings on the GPU and the model's, side by side."""

    def __init__(self, sw, model, ring_frames, rx_stride=None, ring_bytes=None, offset=0, pinned=False):
        import torch
        self.sw, self.model, self.ring_frames = sw, model, ring_frames
        self.fb = M.frame_bytes(model.P)
        self.rx_stride = rx_stride or self.fb
        self.ring_bytes = ring_bytes or ring_frames * self.rx_stride
        self.offset = offset
        nbytes = offset + model.W * self.ring_bytes
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8)
        self.buf = self.buf.pin_memory() if pinned else self.buf.cuda()
        self.gpu = sw.FrameSwitch(params=sw.frame_switch_params(
            [(m, ".".join(str(b) for b in ip)) for m, ip in model.workers], model.S, model.P,
            switch_mac=model.switch_mac, switch_ip=".".join(str(b) for b in model.switch_ip)))
        self.want = np.full(nbytes, SENTINEL, dtype=np.uint8)
        self.fill = [0] * model.W
        self.counts = np.zeros(4, dtype=np.int64)

    def deliver(self, out, verdict, n, drop=None, out_stride=None):
        """One GPU call on device tensors."""
        import torch
        d = None if drop is None else torch.from_numpy(np.asarray(drop, dtype=np.uint32).view(np.int32)).cuda()
        return self.gpu.deliver(out, verdict, n, rings=self.buf[self.offset:], ring_frames=self.ring_frames,
                                drop=d, out_stride=out_stride, rx_stride=self.rx_stride, ring_bytes=self.ring_bytes)

    def expect(self, nframes, verdicts, results, drop=None):
        """The same call on the model, into the expected image."""
        appended, counts, fill = D.deliver(self.model, [None] * nframes, verdicts, results, drop, self.fill,
                                           self.ring_frames)
        for u, fs in enumerate(appended):
            for k, f in enumerate(fs):
                lo = self.offset + u * self.ring_bytes + (self.fill[u] + k) * self.rx_stride
                self.want[lo:lo + self.fb] = f
        self.fill = fill
        self.counts += np.array(counts, dtype=np.int64)
        return appended, counts

    def check(self):
        import torch
        torch.cuda.synchronize()
        assert self.gpu.ring_count.tolist() == self.fill
        assert self.gpu.deliver_counts.tolist() == self.counts.tolist()
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, (bad[:8].tolist(), bad.size)


def to_device(results, n, fb, out_stride=None, fill=0xC3):
    """The switch's out_frames for `results` ({index: frame}): other positions hold `fill`."""
    import torch
    out_stride = out_stride or fb
    buf = np.full((n, out_stride), fill, dtype=np.uint8)
    for i, r in results.items():
        buf[i, :fb] = r
    return torch.from_numpy(buf.reshape(-1)).cuda()


def window(rng, model, mop, packets):
    """One frame per (worker, packet), shuffled; through the model: (frames, verdicts, results)."""
    frames = M.window_frames(rng, model.P, M.default_workers(model.W), mop, packets)
    verdicts, results, _ = M.model_call(model, frames)
    return frames, verdicts, results


def synthetic_host(rng, model, n):
    """n input positions: random verdicts over all five values, random bytes
    for frames (a BROADCAST's header is whatever it is; a RETRANSMIT is
    addressed to a random worker, one in 16 to nobody the table knows)."""
    fb = M.frame_bytes(model.P)
    verdicts = rng.integers(0, 5, n).astype(np.uint8)
    buf = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    to = rng.integers(0, model.W, n)
    ips = np.array([list(ip) for _, ip in model.workers], dtype=np.uint8)
    buf[:, FW.DST_IP] = ips[to]
    buf[rng.random(n) < 1 / 16, FW.DST_IP] = [10, 9, 9, 9]
    FW.put(buf, FW.PKT_ID, np.arange(n))
    results = {int(i): buf[i] for i in np.flatnonzero((verdicts == M.BROADCAST) | (verdicts == M.RETRANSMIT))}
    return verdicts, results, buf


def synthetic(rng, model, n):
    """synthetic_host, and the frames and verdicts on the device."""
    import torch
    verdicts, results, buf = synthetic_host(rng, model, n)
    return verdicts, results, torch.from_numpy(buf.reshape(-1)).cuda(), torch.from_numpy(verdicts).cuda()


@pytest.mark.parametrize("P", [64, 256, 1024])
@pytest.mark.parametrize("W", [1, 2, 32])
def test_replication(sw, P, W):
    """One window, every slot completing, through the GPU switch and deliver:
    every worker's ring holds every result, addressed to that worker, with a
    header checksum that verifies."""
    import torch
    rng = np.random.default_rng(100 * W + P)
    mop = 3
    model = M.SwitchModel(M.default_workers(W), mop, P)
    frames, verdicts, results = window(rng, model, mop, range(mop))
    n, fb = len(frames), M.frame_bytes(P)
    rings = Rings(sw, model, mop + 1)
    out, verdict, _ = rings.gpu(torch.from_numpy(np.concatenate(frames)).cuda(), n)
    rings.deliver(out, verdict, n)
    appended, counts = rings.expect(n, verdicts, results)
    assert counts == [W * mop, 0, 0, 0]
    rings.check()
    assert verdict.cpu().numpy().tolist() == verdicts.tolist()
    got = rings.buf.cpu().numpy().reshape(W, mop + 1, fb)
    for u in range(W):
        mac, ip = model.workers[u]
        for k in range(mop):
            f = got[u, k]
            assert FW.get(f, FW.DST_MAC) == mac and FW.get(f, FW.DST_IP) == ip
            assert FW.ipv4_checksum(f[FW.IP_HEADER]) == 0
        assert sorted(D.pkt_id(got[u, k]) for k in range(mop)) == list(range(mop))


@pytest.mark.parametrize("n", [1, COUNT_WORKGROUP_FRAMES - 1, COUNT_WORKGROUP_FRAMES, COUNT_WORKGROUP_FRAMES + 1,
                               SCAN_TILE_FRAMES + 1])
def test_scan_boundaries(sw, n):
    P, W = 64, 2
    rng = np.random.default_rng(n)
    model = M.SwitchModel(M.default_workers(W), 4, P)
    verdicts, results, d_out, d_verdict = synthetic(rng, model, n)
    rings = Rings(sw, model, (n + 1) // 2)
    rings.deliver(d_out, d_verdict, n)
    _, counts = rings.expect(n, verdicts, results)
    rings.check()
    assert counts[D.OVERFLOW] == 0
    if n > 64:
        assert counts[D.UNROUTABLE] > 0 and min(rings.fill) > n // 5


def test_drops_and_overflow(sw):
    P, W, n = 64, 4, 700
    rng = np.random.default_rng(31)
    model = M.SwitchModel(M.default_workers(W), 4, P)
    verdicts, results, d_out, d_verdict = synthetic(rng, model, n)
    drop = (rng.integers(0, 1 << W, n) & rng.integers(0, 1 << W, n)).astype(np.uint32)   # about a quarter of the bits
    _, _, fill_all = D.deliver(model, [None] * n, verdicts, results, drop, [0] * W, n)
    ring_frames = (min(fill_all) + max(fill_all)) // 2
    assert min(fill_all) < ring_frames < max(fill_all)               # one ring overflows mid-call, another does not
    rings = Rings(sw, model, ring_frames)
    rings.deliver(d_out, d_verdict, n, drop=drop)
    _, counts = rings.expect(n, verdicts, results, drop)
    assert counts[D.DROPPED] > 0 and counts[D.OVERFLOW] > 0
    rings.check()
    # a second call into the same rings: the full ring takes nothing more
    rings.deliver(d_out, d_verdict, n, drop=drop)
    rings.expect(n, verdicts, results, drop)
    rings.check()


@pytest.mark.parametrize("cuts", [1, 2, 5])
def test_appending_across_calls(sw, cuts):
    P, W, n = 64, 3, 611
    rng = np.random.default_rng(32)
    model = M.SwitchModel(M.default_workers(W), 4, P)
    verdicts, results, d_out, d_verdict = synthetic(rng, model, n)
    drop = (rng.integers(0, 1 << W, n) & rng.integers(0, 1 << W, n)).astype(np.uint32)
    fb = M.frame_bytes(P)
    # the whole stream in one model call is what any cutting must leave
    whole = Rings(sw, model, n)
    whole.expect(n, verdicts, results, drop)
    rings = Rings(sw, model, n)
    bounds = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n), cuts - 1, replace=False)) + [n]
    for lo, hi in zip(bounds, bounds[1:]):
        rings.deliver(d_out[lo * fb:], d_verdict[lo:hi], hi - lo, drop=drop[lo:hi])
        rings.expect(hi - lo, verdicts[lo:hi], {i - lo: r for i, r in results.items() if lo <= i < hi}, drop[lo:hi])
    rings.check()
    assert np.array_equal(rings.want, whole.want) and rings.fill == whole.fill
    assert rings.counts.tolist() == whole.counts.tolist()


@pytest.mark.parametrize("P,rx_stride,slack,offset,out_stride,pinned", [
    (64, 320, 64, 0, None, False), (64, 308, 0, 4, 384, False), (256, 1088, 12, 52, 1152, False),
    (256, 1152, 128, 0, None, True), (1024, 4160, 4, 8, None, True)])
def test_layout(sw, P, rx_stride, slack, offset, out_stride, pinned):
    """rx_stride > frame bytes, ring_bytes > ring_frames * rx_stride, a ring
    base that is only 4-byte aligned, out_stride > frame bytes, rings in pinned
    host memory."""
    W, n = 3, 300
    rng = np.random.default_rng(P + offset)
    model = M.SwitchModel(M.default_workers(W), 4, P)
    verdicts, results, d_out, d_verdict = synthetic(rng, model, n)
    fb = M.frame_bytes(P)
    if out_stride:
        d_out = to_device(results, n, fb, out_stride)
    rings = Rings(sw, model, 48, rx_stride=rx_stride, ring_bytes=48 * rx_stride + slack, offset=offset, pinned=pinned)
    assert rings.buf[offset:].data_ptr() % 16 == offset % 16
    rings.deliver(d_out, d_verdict, n, out_stride=out_stride)
    _, counts = rings.expect(n, verdicts, results)
    assert counts[D.OVERFLOW] > 0
    rings.check()


def test_own_rings_and_reset(sw):
    """FrameSwitch.deliver with the switch's own rings; reset_rings empties them."""
    import torch
    P, W, n = 64, 2, 90
    rng = np.random.default_rng(33)
    model = M.SwitchModel(M.default_workers(W), 4, P)
    verdicts, results, d_out, d_verdict = synthetic(rng, model, n)
    gpu = sw.FrameSwitch(M.default_workers(W), 4, P)
    with pytest.raises(ValueError):
        gpu.deliver(d_out, d_verdict, n)
    rings, ring_count, counts = gpu.deliver(d_out, d_verdict, n, ring_frames=n)
    assert tuple(rings.shape) == (W, n, M.frame_bytes(P)) and rings is gpu.rings
    appended, want_counts, fill = D.deliver(model, [None] * n, verdicts, results, None, [0] * W, n)
    torch.cuda.synchronize()
    assert ring_count.tolist() == fill and counts.tolist() == want_counts
    for u in range(W):
        assert np.array_equal(rings[u, :fill[u]].cpu().numpy(), np.stack(appended[u]))
    gpu.deliver(d_out, d_verdict, n)
    torch.cuda.synchronize()
    assert gpu.ring_count.tolist() == [min(2 * c, n) for c in fill]
    gpu.reset_rings()
    torch.cuda.synchronize()
    assert gpu.ring_count.tolist() == [0] * W and gpu.deliver_counts.tolist() == [0] * 4


def test_gather(sw):
    import torch
    P, nsets, set_frames, n = 64, 3, 17, 300
    fb = M.frame_bytes(P)
    set_stride, dst_stride = fb + 12, fb + 4
    rng = np.random.default_rng(34)
    host = [rng.integers(0, 256, (set_frames, set_stride), dtype=np.uint8) for _ in range(nsets)]
    dev = [torch.from_numpy(h.reshape(-1)) for h in host]
    dev = [dev[0].cuda(), dev[1].pin_memory(), dev[2].cuda()[:]]
    set_idx = rng.integers(0, nsets, n).astype(np.int32)               # n > sets x frames: repeats
    frame_idx = rng.integers(0, set_frames, n).astype(np.int64)
    set_idx[41], frame_idx[97] = nsets, set_frames                      # two entries out of range
    want, skipped = D.gather([[f[:fb] for f in h] for h in host], set_idx, frame_idx)
    assert skipped == 2
    out = torch.full((n * dst_stride,), SENTINEL, dtype=torch.uint8, device="cuda")
    got, d_skipped = sw.gather_frames(dev, torch.from_numpy(set_idx).cuda(), torch.from_numpy(frame_idx).cuda(), P,
                                      set_frames=set_frames, set_stride=set_stride, out=out, out_stride=dst_stride)
    torch.cuda.synchronize()
    image = np.full((n, dst_stride), SENTINEL, dtype=np.uint8)
    for j, f in enumerate(want):
        if f is not None:
            image[j, :fb] = f
    assert np.array_equal(got.cpu().numpy().reshape(n, dst_stride), image)
    assert d_skipped.tolist() == [2]
    sw.gather_frames(dev, torch.from_numpy(set_idx).cuda(), torch.from_numpy(frame_idx).cuda(), P,
                     set_frames=set_frames, set_stride=set_stride, out=out, out_stride=dst_stride, skipped=d_skipped)
    torch.cuda.synchronize()
    assert d_skipped.tolist() == [4]                                    # added to


# ------------------------------------------------------------- closed loop

def worker_params(sw, workers, w, mop, job):
    mac, ip = workers[w]
    return sw.frame_params(dst_mac=M.SWITCH_MAC, src_mac=mac, src_ip=ip, dst_ip=M.SWITCH_IP, src_port=4000 + w,
                           dst_port=48879, job_id=job, pool_index_start=0, pool_index_shift=0,
                           max_outstanding_pkts=mop)


def run_windows(sw, gpu, sets, nframes, mop, ring_frames):
    """W workers' frame sets (device tensors, packed) a window of mop packets
    per call: gather -> switch -> deliver, on the current stream, no host code
    between them.  Returns (rings, ring_count)."""
    import torch
    W = len(sets)
    gpu.reset()
    gpu.reset_rings()
    rings = torch.full((W, ring_frames, M.frame_bytes(gpu.packet_numel)), SENTINEL, dtype=torch.uint8, device="cuda")
    for lo in range(0, nframes, mop):
        hi = min(lo + mop, nframes)
        set_idx = torch.arange(W, dtype=torch.int32, device="cuda").repeat(hi - lo)        # workers interleaved
        frame_idx = torch.arange(lo, hi, dtype=torch.int64, device="cuda").repeat_interleave(W)
        n = W * (hi - lo)
        call, skipped = sw.gather_frames(sets, set_idx, frame_idx, gpu.packet_numel, set_frames=nframes)
        out, verdict, _ = gpu(call, n)
        gpu.deliver(out, verdict, n, rings=rings)
    torch.cuda.synchronize()
    assert skipped.tolist() == [0]
    return rings, gpu.ring_count


def check_addresses(rings, ring_count, workers):
    got = rings.cpu().numpy()
    for u, (mac, ip) in enumerate(workers):
        for k in range(int(ring_count[u])):
            assert FW.get(got[u, k], FW.DST_MAC) == mac and FW.get(got[u, k], FW.DST_IP) == M.ip_bytes(ip), (u, k)
        assert np.all(got[u, int(ring_count[u]):] == SENTINEL)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_closed_loop_float(sw, dtype):
    """test_end_to_end_float's shapes and phases with the wire on the GPU:
    each worker dequantizes its own ring."""
    import torch
    P, W, mop, job = 64, 3, 4, 3
    n = 5 * P + 7
    B = O.num_blocks(n, P)
    tdt = getattr(torch, dtype)
    workers = M.default_workers(W)
    gpu = sw.FrameSwitch(workers, mop, P, switch_mac=M.SWITCH_MAC, switch_ip=M.SWITCH_IP)
    xs = [(O.splitmix_normal(40 + w, n) * np.float32(4.0 ** w)).astype(np.float32) for w in range(W)]
    xd = [torch.from_numpy(x).cuda().to(tdt) for x in xs]
    xs = [x.float().cpu().numpy() for x in xd]
    prm = [worker_params(sw, workers, w, mop, job) for w in range(W)]
    own = [sw.quantize_pack_frames(xd[w], prm[w], P, W, batch_max=mop) for w in range(W)]
    rings, ring_count = run_windows(sw, gpu, own, B + mop, mop, B + mop)
    assert ring_count.tolist() == [B + mop] * W
    want_exps = O.switch_exps([O.exponents(x, P) for x in xs])
    # a window's results are in completion order: pkt_id p's exponent from whichever position holds it
    r0 = rings[0].cpu().numpy()
    by_pkt = {D.pkt_id(f): f for f in r0}
    gexp_host = np.array([FW.get(by_pkt[p], FW.EXP) for p in range(B)], dtype=np.uint8).view(np.int8)
    assert np.array_equal(gexp_host, want_exps)
    gexp = torch.from_numpy(gexp_host).cuda()
    glob = [sw.quantize_pack_frames(xd[w], prm[w], P, W, batch_max=mop, global_exps=gexp) for w in range(W)]
    rings, ring_count = run_windows(sw, gpu, glob, B + mop, mop, B + mop)
    check_addresses(rings, ring_count, workers)
    payload = O.switch_payload([O.quantize(x, P, W, global_exps=want_exps) for x in xs])
    want = O.dequantize(payload, want_exps, n, P, W)
    if dtype != "float32":
        want = torch.from_numpy(want).to(tdt).view(torch.int16).numpy()
    for w in range(W):
        rx = sw.RxSlice(n, P, batch_max=mop, dtype=tdt)
        sw.dequantize_frames(rings[w].reshape(-1), B + mop, rx, num_workers=W, job_id=job)
        torch.cuda.synchronize()
        got = rx.out.cpu()
        got = got.view(torch.int16).numpy() if dtype != "float32" else got.numpy()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), w
        assert np.array_equal(rx.exps.cpu().numpy(), want_exps)
        assert rx.counts.tolist() == [B + mop, 0]


def test_closed_loop_int32(sw):
    import torch
    P, W, mop, job = 64, 2, 4, 9
    n = 5 * P + 7
    B = O.num_blocks(n, P)
    workers = M.default_workers(W)
    gpu = sw.FrameSwitch(workers, mop, P, switch_mac=M.SWITCH_MAC, switch_ip=M.SWITCH_IP)
    rng = np.random.default_rng(11)
    xs = [rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) for _ in range(W)]
    prm = [worker_params(sw, workers, w, mop, job) for w in range(W)]
    sets = [sw.pack_frames_int32(torch.from_numpy(xs[w]).cuda(), prm[w], P) for w in range(W)]
    rings, ring_count = run_windows(sw, gpu, sets, B, mop, B + 1)
    assert ring_count.tolist() == [B] * W
    check_addresses(rings, ring_count, workers)
    for w in range(W):
        rx = sw.RxSliceInt32(n, P)
        sw.unpack_frames_int32(rings[w].reshape(-1), B, rx, job_id=job)
        torch.cuda.synchronize()
        assert np.array_equal(rx.out.cpu().numpy(), xs[0] + xs[1]), w       # int32 addition wraps
        assert rx.counts.tolist() == [B, 0]


class GpuSwitch:
    """lossy_loop's backend on the GPU, with the model beside it: every
    call's verdicts and rings are compared before the workers see them."""

    def __init__(self, sw, sets_dev, sets_host, workers, mop, P, ring_frames):
        import torch
        self.sw, self.P, self.W = sw, P, len(workers)
        self.sets = sets_dev
        self.model = D.ModelSwitch(sets_host, workers, mop, P, ring_frames)
        self.gpu = sw.FrameSwitch(workers, mop, P, switch_mac=M.SWITCH_MAC, switch_ip=M.SWITCH_IP)
        self.rings = torch.full((self.W, ring_frames, M.frame_bytes(P)), SENTINEL, dtype=torch.uint8, device="cuda")
        self.seen = [0] * self.W

    def call(self, batch, drop):
        import torch
        n = len(batch)
        set_idx = torch.tensor([w for w, _ in batch], dtype=torch.int32).cuda()
        frame_idx = torch.tensor([p for _, p in batch], dtype=torch.int64).cuda()
        d = torch.from_numpy(np.asarray(drop, dtype=np.uint32).view(np.int32)).cuda()
        frames, _ = self.sw.gather_frames(self.sets, set_idx, frame_idx, self.P)
        out, verdict, _ = self.gpu(frames, n)
        _, ring_count, _ = self.gpu.deliver(out, verdict, n, rings=self.rings, drop=d)
        torch.cuda.synchronize()
        verdicts = verdict.cpu().numpy()
        fill = ring_count.tolist()
        # the workers' view: the pkt_id field of the new ring entries
        got = self.rings.cpu().numpy()
        ids = FW.get(got, FW.PKT_ID)
        new_ids = [[int(p) for p in ids[u, self.seen[u]:fill[u]]] for u in range(self.W)]
        want_v, want_fill, want_ids = self.model.call(batch, drop)
        assert verdicts.tolist() == want_v.tolist()
        assert fill == want_fill and new_ids == want_ids
        for u in range(self.W):
            for k in range(self.seen[u], fill[u]):
                assert np.array_equal(got[u, k], self.model.rings[u][k]), (u, k)
        self.seen = fill
        return verdicts, fill, new_ids


@pytest.mark.parametrize("seed", D.LOSSY_SEEDS)
def test_closed_loop_lossy(sw, seed):
    """INT32 slices through gather -> switch -> deliver under ingress loss (the
    gather list) and egress loss (d_drop), DEFERRED frames resubmitted by
    index, until every worker's ring unpacks to the exact wrapping sum."""
    import torch
    c = D.LOSSY
    W, N, mop, P, job = c["W"], c["N"], c["mop"], c["P"], 5
    workers = M.default_workers(W)
    rng = np.random.default_rng(seed)
    xs = [rng.integers(-2 ** 31, 2 ** 31, N * P, dtype=np.int64).astype(np.int32) for _ in range(W)]
    prm = [worker_params(sw, workers, w, mop, job) for w in range(W)]
    sets = [sw.pack_frames_int32(torch.from_numpy(xs[w]).cuda(), prm[w], P) for w in range(W)]
    torch.cuda.synchronize()
    fb = M.frame_bytes(P)
    host = [list(s.cpu().numpy().reshape(N, fb)) for s in sets]
    switch = GpuSwitch(sw, sets, host, workers, mop, P, c["ring_frames"])
    ncalls = D.lossy_loop(seed, W, N, mop, c["q"], switch)
    assert ncalls <= 100 * N * W
    assert switch.gpu.deliver_counts.tolist() == switch.model.counts
    assert np.all(switch.rings.cpu().numpy()[:, max(switch.seen):] == SENTINEL)
    want = (xs[0].astype(np.int64) + xs[1] + xs[2]).astype(np.int32)
    for w in range(W):
        rx = sw.RxSliceInt32(N * P, P)
        sw.unpack_frames_int32(switch.rings[w].reshape(-1), switch.seen[w], rx, job_id=job)
        torch.cuda.synchronize()
        assert np.array_equal(rx.out.cpu().numpy(), want), w
        assert rx.counts.tolist() == [N, switch.seen[w] - N]
