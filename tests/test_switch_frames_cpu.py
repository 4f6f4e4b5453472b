"""CPU tests of the frame switch (no GPU needed): the sequential model of
tests/switch_frames_model.py against the oracle's plane-level switch, the
stream generator, and sml_frame_switch's host-side contract — the state size
and every argument check, which return before any HIP call."""
import ctypes

import numpy as np
import pytest

import switch_frames_model as M
from oracle import oracle as O
from switchml_amd import frame_wire as FW


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def run_calls(model, calls):
    """Every call through model_call with the deferred frames of the call
    before prepended; returns [(frames, verdicts, results)]."""
    out, deferred = [], []
    for fresh in calls:
        frames = deferred + fresh
        verdicts, results, _ = M.model_call(model, frames)
        deferred = [frames[i] for i in range(len(frames)) if verdicts[i] == M.DEFERRED]
        out.append((frames, verdicts, results))
    return out


def oracle_result(payloads, exps, p):
    """Packet p's aggregate by the oracle's plane-level switch: wire bytes, the two exponent bytes."""
    W = payloads.shape[0]
    words = O.switch_payload([payloads[w, p].view(np.uint32) for w in range(W)])
    e0 = O.switch_exps([exps[w, p, 0:1].view(np.int8) for w in range(W)])
    e1 = O.switch_exps([exps[w, p, 1:2].view(np.int8) for w in range(W)])
    return words.view(np.uint8), np.array([e0[0], e1[0]], dtype=np.int8).view(np.uint8)


@pytest.mark.parametrize("W,N,mop,P", [(3, 11, 4, 64), (2, 5, 8, 256), (8, 9, 2, 128)])
def test_lossless_stream_equals_the_plane_switch(W, N, mop, P):
    calls, payloads, exps = M.lossy_stream(5, W, N, mop, P, q=0.0)
    model = M.SwitchModel(M.default_workers(W), mop, P)
    seen = {}
    for frames, verdicts, results in run_calls(model, calls):
        assert not np.any(verdicts == M.IGNORED)
        for i, r in results.items():
            assert verdicts[i] == M.BROADCAST            # nothing is lost: nobody asks twice
            p = FW.get(r, FW.PKT_ID)
            assert p not in seen
            seen[p] = r
    assert sorted(seen) == list(range(N))
    for p, r in seen.items():
        words, e = oracle_result(payloads, exps, p)
        assert np.array_equal(r[FW.HEADER_BYTES:], words), p
        assert np.array_equal(r[FW.EXPS], e), p
        assert FW.get(r, FW.POOL_INDEX) == M.pool_index(p, mop) & ~FW.POOL_BIT14


def test_single_worker_echoes_the_payload():
    P, mop = 64, 2
    calls, payloads, exps = M.lossy_stream(9, 1, 6, mop, P, q=0.0)
    model = M.SwitchModel(M.default_workers(1), mop, P)
    for frames, verdicts, results in run_calls(model, calls):
        assert np.all(verdicts == M.BROADCAST)
        for i, r in results.items():
            assert np.array_equal(r[FW.EXP.start:], frames[i][FW.EXP.start:])
    # a duplicate is answered, with the same words
    f = M.worker_frame(P, M.default_workers(1)[0], 4, M.pool_index(4, mop), payloads[0, 4], exps[0, 4])
    verdict, r = model.frame(f)
    assert verdict == M.RETRANSMIT and np.array_equal(r[FW.EXP.start:], f[FW.EXP.start:])


def test_result_header_fields():
    # Spelled out on purpose, not through frame_wire: the independent statement of the format a module bug cannot hide in.
    P, W = 64, 2
    workers = M.default_workers(W)
    model = M.SwitchModel(workers, 4, P)
    pay = np.arange(4 * P, dtype=np.uint8)
    f0 = M.worker_frame(P, workers[0], 7, 0x8003, pay, (1, 2), src_port=1234, dst_port=48879, job=5)
    f1 = M.worker_frame(P, workers[1], 7, 0x8003, pay, (3, 1), src_port=4321, dst_port=48879, job=5)
    assert model.frame(f0) == (M.CONSUMED, None)
    verdict, r = model.frame(f1)
    assert verdict == M.BROADCAST
    n = M.frame_bytes(P)
    assert bytes(r[0:6]) == workers[1][0] and bytes(r[6:12]) == M.SWITCH_MAC and bytes(r[12:16]) == b"\x08\x00\x45\x00"
    assert (int(r[16]) << 8 | int(r[17])) == n - 14 and bytes(r[18:22]) == b"\0\0\0\0" and r[22] == 64 and r[23] == 17
    assert M.ipv4_checksum(r[14:34]) == 0                   # a header with its checksum in place sums to 0
    assert bytes(r[26:30]) == M.ip_bytes(M.SWITCH_IP) and bytes(r[30:34]) == M.ip_bytes(workers[1][1])
    assert (int(r[34]) << 8 | int(r[35])) == 48879 and (int(r[36]) << 8 | int(r[37])) == 4321
    assert (int(r[38]) << 8 | int(r[39])) == n - 34 and bytes(r[40:42]) == b"\0\0"
    assert r[42] == 0x10 | (int(f1[42]) & 7) and r[43] == 5 and bytes(r[44:48]) == bytes(f1[44:48])
    assert bytes(r[48:50]) == b"\x80\x03" and bytes(r[50:52]) == b"\x03\x02"


def test_call_rule_defers_the_other_set():
    P, mop = 64, 2
    workers = M.default_workers(2)
    model = M.SwitchModel(workers, mop, P)
    pay = np.zeros(4 * P, dtype=np.uint8)
    frames = [M.worker_frame(P, workers[0], 0, M.pool_index(0, mop), pay),
              M.worker_frame(P, workers[0], 2, M.pool_index(2, mop), pay),     # same slot, other set
              M.worker_frame(P, workers[1], 2, M.pool_index(2, mop), pay)]     # another pair: its own first
    verdicts, results, counts = M.model_call(model, frames)
    assert list(verdicts) == [M.CONSUMED, M.DEFERRED, M.CONSUMED] and counts == [2, 0, 0, 0, 1]
    assert model.bitmap[0] == [1, 2]


def test_lossy_stream_is_seeded_and_finishes():
    a = M.lossy_stream(3, 3, 12, 4, 64, q=0.1)
    b = M.lossy_stream(3, 3, 12, 4, 64, q=0.1)
    assert len(a[0]) == len(b[0]) and all(len(x) == len(y) and all(np.array_equal(f, g) for f, g in zip(x, y))
                                          for x, y in zip(a[0], b[0]))
    assert sum(len(c) for c in a[0]) >= 3 * 12


# ------------------------------------------------------------ the C entry points

def test_params_layout_matches_header(sw):
    Pm, Wk = sw.FrameSwitchParams, sw.SwitchWorker
    assert Wk.mac.offset == 0 and Wk.ip_be.offset == 8 and ctypes.sizeof(Wk) == 12
    assert Pm.switch_mac.offset == 0 and Pm.switch_ip_be.offset == 8 and Pm.num_workers.offset == 12
    assert Pm.num_slots.offset == 16 and Pm.packet_numel.offset == 20 and Pm.workers.offset == 24
    assert ctypes.sizeof(Pm) == 24 + 32 * 12


def test_state_bytes(sw):
    f = sw.lib().sml_frame_switch_state_bytes
    for S in (1, 4, 256, 16384):
        for P in sw.PACKET_NUMELS:
            n = f(S, P)
            # per (slot, set): P accumulated words, bitmap, count, exponents; 32 claim words per slot
            assert n >= S * (2 * (4 * P + 12) + 32 * 8) and n % 8 == 0
            assert n <= S * (2 * (4 * P + 12) + 32 * 8) + 4 * S + 256
    for S, P in [(0, 256), (16385, 256), (4, 100), (4, 0), (4, 2048)]:
        assert f(S, P) == 0


def test_argument_checks_without_gpu(sw):
    L = sw.lib()
    vp = ctypes.c_void_p
    f = L.sml_frame_switch
    INV, UNS, ALN, OK = sw.SML_ERR_INVALID_ARG, sw.SML_ERR_UNSUPPORTED, sw.SML_ERR_ALIGNMENT, sw.SML_OK

    def params(W=2, S=4, P=64):
        sp = sw.frame_switch_params(M.default_workers(min(W, 32)), S, P)
        sp.num_workers = W
        return ctypes.byref(sp)

    fr, st, out, vd, cnt = vp(4096), vp(8192), vp(16384), vp(32768), vp(65536)
    fb = FW.frame_bytes(64)
    # null
    assert f(None, fr, 1, fb, st, out, fb, vd, cnt, None) == INV
    assert f(params(W=0), fr, 1, fb, st, out, fb, vd, cnt, None) == INV
    for args in [(None, 1, fb, st, out, fb, vd), (fr, 1, fb, None, out, fb, vd), (fr, 1, fb, st, None, fb, vd),
                 (fr, 1, fb, st, out, fb, None)]:
        assert f(params(), *args, cnt, None) == INV
    # unsupported: packet size, workers, slots — and null wins over them
    assert f(params(P=100), fr, 1, fb, st, out, fb, vd, cnt, None) == UNS
    assert f(params(W=33), fr, 1, fb, st, out, fb, vd, cnt, None) == UNS
    assert f(params(S=0), fr, 1, fb, st, out, fb, vd, cnt, None) == UNS
    assert f(params(S=16385), fr, 1, fb, st, out, fb, vd, cnt, None) == UNS
    assert f(params(W=33, S=16385, P=100), fr, 1, fb, st, out, fb, vd, cnt, None) == UNS
    assert f(params(P=100), None, 1, fb, st, out, fb, vd, cnt, None) == INV
    assert f(params(P=100), fr, 1, 50, vp(8196), out, fb, vd, cnt, None) == UNS      # ... over alignment
    # nothing to do: no buffer is looked at, the parameters still are
    assert f(params(), None, 0, 0, None, None, 0, None, None, None) == OK
    assert f(params(P=100), None, 0, 0, None, None, 0, None, None, None) == UNS
    assert f(None, None, 0, 0, None, None, 0, None, None, None) == INV
    # alignment: frames, strides, state, counts
    assert f(params(), vp(4098), 1, fb, st, out, fb, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb - 4, st, out, fb, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb + 2, st, out, fb, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb, st, vp(16386), fb, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb, st, out, fb - 4, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb, st, out, fb + 2, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb, vp(8196), out, fb, vd, cnt, None) == ALN
    assert f(params(), fr, 1, fb, st, out, fb, vd, vp(65540), None) == ALN
    # reset
    r = L.sml_frame_switch_reset
    assert r(None, 4, 64, None) == INV
    assert r(st, 0, 64, None) == UNS and r(st, 16385, 64, None) == UNS and r(st, 4, 100, None) == UNS
    assert r(vp(8196), 4, 64, None) == ALN
    assert r(None, 0, 64, None) == INV
    assert L.sml_abi_version() == 2


def test_python_wrapper_refuses_too_many_workers(sw):
    with pytest.raises(ValueError, match="at most 32"):
        sw.frame_switch_params(M.default_workers(33), 4, 64)
