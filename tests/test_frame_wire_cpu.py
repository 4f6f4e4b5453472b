"""CPU tests of switchml_amd.frame_wire, the Python owner of the DPDK frame's
layout: the example header written out in csrc/sml_frame_wire.h, the table's
coverage, put / get on arrays and tensors, and worker_frame / pool_index against
the C oracle, the second, independent description of the frame."""
import numpy as np
import pytest

import switch_frames_model as M
from oracle import oracle as O
from switchml_amd import frame_wire as FW

# sml_frame_wire.h, above `namespace example`: worker 10.0.1.2 -> switch 10.0.0.253, P = 64, job 5, pkt_id 7, slot 3
# of set 1, exponents 3 and 1, every ignored field non-zero.
EXAMPLE = bytes.fromhex("02 00 00 00  00 01 02 00  00 00 01 01  08 00 45 a5  01 26 be ef  40 01 80 11  c3 5a 0a 00"
                        "01 02 0a 00  00 fd 10 e1  be ef 01 12  77 99 f1 05  07 00 00 00  c0 03 03 01")
WORKER, SWITCH = "10.0.1.2", "10.0.0.253"


def example():
    return np.frombuffer(EXAMPLE, dtype=np.uint8).copy()


def test_example_header_getters():
    f = example()
    assert f.size == FW.HEADER_BYTES
    want = dict(DST_MAC=bytes([2, 0, 0, 0, 0, 1]), SRC_MAC=bytes([2, 0, 0, 0, 1, 1]), ETHERTYPE=b"\x08\x00",
                IP_VER_TOS=b"\x45\xa5", IP_TOTAL_LEN=294, IP_ID_FRAG=b"\xbe\xef\x40\x01", IP_TTL=128, IP_PROTO=17,
                IP_CHECKSUM=0xc35a, SRC_IP=FW.ip_bytes(WORKER), DST_IP=FW.ip_bytes(SWITCH), SRC_PORT=4321,
                DST_PORT=48879, UDP_LEN=274, UDP_CHECKSUM=b"\x77\x99", JOB_TYPE_SIZE=0xf1, JOB=5, PKT_ID=7,
                POOL_INDEX=0xc003, EXP=3, EXP2=1)
    assert {name: FW.get(f, getattr(FW, name)) for name in FW.LAYOUT} == want
    assert FW.ipv4_total_len(64) == 294 and FW.udp_len(64) == 274 and FW.job_type_size(64) == 0x11
    idx = FW.get(f, FW.POOL_INDEX)
    assert FW.pool_slot(idx) == 3 and FW.pool_set(idx) == 1 and idx & FW.POOL_BIT14
    assert FW.get(f, FW.EXPS) == b"\x03\x01"
    assert FW.ip_be(WORKER) == 0x0201000a and FW.ip_be(SWITCH) == 0xfd00000a      # kWorkerIp, kSwitchIp: memory order


def test_example_result_frame():
    """The result to the example's worker, exponents 3 and 2, as the header's
    asserts name it: checksum bytes 63 c9, and bytes 32-51."""
    ck = FW.result_ipv4_checksum(64, SWITCH, WORKER)
    assert ck == 0x63c9 and FW.result_ipv4_checksum(64, FW.ip_bytes(SWITCH), FW.ip_bytes(WORKER)) == ck
    workers = M.default_workers(2)
    assert workers[1] == (FW.get(example(), FW.SRC_MAC), WORKER)
    model = M.SwitchModel(workers, 4, 64, switch_ip=SWITCH)
    pay = np.arange(4 * 64, dtype=np.uint8)
    first = FW.worker_frame(64, workers[0], 7, 0x8003, pay, (1, 2))
    second = np.concatenate([example(), pay])
    assert model.frame(first) == (M.CONSUMED, None)
    verdict, r = model.frame(second)
    assert verdict == M.BROADCAST
    tail = bytes.fromhex("01 02 be ef  10 e1 01 12  00 00 11 05  07 00 00 00  80 03 03 02")         # bytes 32-51
    assert bytes(r[FW.HEADER_BYTES - len(tail):FW.HEADER_BYTES]) == tail
    assert FW.get(r, FW.IP_CHECKSUM) == ck and FW.ipv4_checksum(r[FW.IP_HEADER]) == 0


def test_table_covers_the_header_once():
    spans = sorted((lo, hi) for lo, hi, _ in FW.LAYOUT.values())
    assert spans[0][0] == 0 and spans[-1][1] + 1 == len(EXAMPLE) == FW.HEADER_BYTES
    assert all(a[1] + 1 == b[0] for a, b in zip(spans, spans[1:]))              # no gap, no overlap
    for name, (lo, hi, enc) in FW.LAYOUT.items():
        assert getattr(FW, name) == slice(lo, hi + 1) and enc in (FW.BYTES, FW.BE, FW.LE), name
    assert FW.HEADER == slice(0, len(EXAMPLE)) and FW.EXPS == slice(50, len(EXAMPLE)) and FW.IP_HEADER == slice(14, 34)
    assert FW.span(FW.DST_MAC, FW.IP_CHECKSUM) == slice(0, 26) and FW.span(FW.JOB, FW.PKT_ID) == slice(43, 48)
    for P, fb in ((64, 308), (1024, 4148)):
        assert FW.frame_bytes(P) == fb and FW.payload(P) == slice(len(EXAMPLE), fb)
        assert FW.ipv4_total_len(P) == fb - 14 and FW.udp_len(P) == fb - 34


def holders():
    """A frame, frames at a stride wider than a frame, and the same as torch tensors: (name, make, frames)."""
    import torch
    fb = FW.frame_bytes(64)
    return [("1-D", lambda: np.full(fb, 0x5A, dtype=np.uint8), None),
            ("2-D", lambda: np.full((5, fb + 12), 0x5A, dtype=np.uint8), 5),
            ("tensor 1-D", lambda: torch.full((fb,), 0x5A, dtype=torch.uint8), None),
            ("tensor 2-D", lambda: torch.full((5, fb + 12), 0x5A, dtype=torch.uint8), 5)]


@pytest.mark.parametrize("name", list(FW.LAYOUT) + ["EXPS", "IP_HEADER"])
def test_put_get_round_trip(name):
    field = getattr(FW, name)
    width = field.stop - field.start
    rng = np.random.default_rng(width + field.start)
    integer = name in FW.LAYOUT and FW.LAYOUT[name][2] != FW.BYTES
    for holder, make, F in holders():
        f = make()
        shape = () if F is None else (F,)
        if integer:
            value = rng.integers(0, 1 << (8 * width), shape, dtype=np.uint64).astype(np.int64)
            value = int(value) if F is None else value
        else:
            value = rng.integers(0, 256, shape + (width,), dtype=np.uint8)
            value = bytes(value) if F is None else value
        FW.put(f, field, value)
        got = FW.get(f, field)
        assert np.array_equal(got, value) and type(got) is type(value), holder
        raw = np.asarray(f)
        outside = np.ones(raw.shape[-1], dtype=bool)
        outside[field] = False
        assert np.all(raw[..., outside] == 0x5A), holder                       # no byte outside the field changed
        # the bytes on the wire, by the field's encoding
        one = raw if F is None else raw[F - 1]
        v = value if F is None else value[F - 1]
        order = {FW.BE: "big", FW.LE: "little"}
        assert bytes(one[field]) == (int(v).to_bytes(width, order[FW.LAYOUT[name][2]]) if integer else bytes(v)), holder


def test_payload_words_round_trip():
    P = 64
    rng = np.random.default_rng(1)
    words = rng.integers(0, 2 ** 32, (3, P), dtype=np.uint64).astype(np.uint32)
    f = np.full((3, FW.frame_bytes(P) + 4), 0x5A, dtype=np.uint8)
    FW.put_payload_words(f, P, words)
    assert np.array_equal(FW.payload_words(f, P), words) and FW.payload_words(f[1], P).dtype == np.uint32
    assert bytes(f[2, FW.payload(P)]) == words[2].astype(">u4").tobytes()
    assert np.all(f[:, FW.HEADER] == 0x5A) and np.all(f[:, FW.frame_bytes(P):] == 0x5A)


@pytest.mark.parametrize("P", [64, 128, 256, 512, 1024])
def test_worker_frame_is_the_oracles_frame(P):
    """Every packet of a 3P + 5 element INT32 slice: BuildPacket's frame by the
    C oracle and worker_frame differ at most in the UDP checksum field, the
    pseudo-header sum that worker_frame leaves 0."""
    import switchml_amd as sw
    worker = (bytes([2, 0, 0, 0, 1, 7]), "10.0.1.8")
    start, shift, mop, job = 10, 3, 8, 0x1207
    fp = sw.frame_params(dst_mac=FW.SWITCH_MAC, src_mac=worker[0], src_ip=worker[1], dst_ip=FW.SWITCH_IP, src_port=4321,
                         dst_port=48879, job_id=job, pool_index_start=start, pool_index_shift=shift,
                         max_outstanding_pkts=mop)
    x = np.random.default_rng(P).integers(-2 ** 31, 2 ** 31, 3 * P + 5, dtype=np.int64).astype(np.int32)
    B = O.num_blocks(x.size, P)
    assert B == 4
    want = O.build_frames_i32(x, fp, P=P).reshape(B, FW.frame_bytes(P))
    padded = np.zeros(B * P, dtype=np.int32)
    padded[:x.size] = x
    allowed = set(range(FW.UDP_CHECKSUM.start, FW.UDP_CHECKSUM.stop))
    for p in range(B):
        got = FW.worker_frame(P, worker, p, FW.pool_index(p, mop, start, shift),
                              padded[p * P:(p + 1) * P].astype(">i4").view(np.uint8), src_port=4321, job=job)
        assert set(np.flatnonzero(got != want[p]).tolist()) <= allowed, p
        assert np.array_equal(FW.payload_words(got, P).view(np.int32), padded[p * P:(p + 1) * P])
    assert any(want[:, FW.UDP_CHECKSUM].reshape(-1))                           # the oracle does fill it


def test_pool_index_is_the_oracles():
    for mop in (1, 2, 3, 8, 64, 256):
        for start in (0, 10, 0x3ff0):
            for shift in (0, 3):
                got = [FW.pool_index(p, mop, start, shift) for p in range(5 * mop + 3)]
                assert got == [O.pool_index(p, start, shift, mop) for p in range(5 * mop + 3)], (mop, start, shift)
    assert FW.pool_index(5, 8, 10, 3) == O.pool_index(5, 10, 3, 8) == 0x800a
    assert FW.pool_index is M.pool_index and FW.worker_frame is M.worker_frame   # re-exports, not second implementations
