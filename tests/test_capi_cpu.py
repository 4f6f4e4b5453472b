"""CPU tests of the C-ABI boundary (no GPU needed): the HIP library loads,
exports every entry point include/switchml_hip.h declares, and its host-only
entry points (geometry, scale LUT, argument validation) behave — validation
returns before any HIP call, so these run without a device."""
import ctypes
import re

import numpy as np
import pytest

from oracle import oracle as O
from switchml_amd import frame_wire as FW


@pytest.fixture(scope="module")
def sw():
    import switchml_amd
    switchml_amd.lib()
    return switchml_amd


def test_exports_every_header_symbol(sw):
    syms = sw.header_symbols()
    assert len(syms) >= 12
    L = sw.lib()
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def header_prototypes(path):
    """{function: (return type, parameter count)} of a C-ABI header, comments
    stripped as header_symbols does; `(void)` counts 0."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?\**)\s*\b(sml_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = params.strip()
        protos[name] = (" ".join(ret.split()), 0 if params in ("", "void") else params.count(",") + 1)
    return protos


def test_every_header_function_has_a_ctypes_prototype(sw):
    """lib() declares restype and argtypes for every function of the header:
    without argtypes ctypes passes a Python int as a C int and truncates a
    pointer.  An unset restype reads as c_int, which a set one may equal, so
    restype is held against the header's return type instead."""
    protos = header_prototypes(sw.HEADER_PATH)
    assert sorted(protos) == sw.header_symbols()
    restype = {"sml_status_t": ctypes.c_int, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32,
               "uint64_t": ctypes.c_uint64, "const char*": ctypes.c_char_p}
    L = sw.lib()
    bad = []
    for name, (ret, nparams) in sorted(protos.items()):
        fn = getattr(L, name)
        if fn.argtypes is None or len(fn.argtypes) != nparams or fn.restype is not restype[ret]:
            bad.append((name, ret, nparams, fn.restype, fn.argtypes))
    assert not bad, bad


def test_abi_version_and_status_strings(sw):
    L = sw.lib()
    assert L.sml_abi_version() == 2
    for code, name in [(0, b"SML_OK"), (1, b"SML_ERR_INVALID_ARG"), (2, b"SML_ERR_UNSUPPORTED"),
                       (3, b"SML_ERR_ALIGNMENT"), (4, b"SML_ERR_HIP")]:
        assert L.sml_status_string(code) == name


@pytest.mark.parametrize("numel,P", [(0, 256), (1, 64), (255, 256), (256, 256), (257, 256),
                                     (16 * 2 ** 20, 256), (67_108_864, 1024), (10 ** 12 + 3, 64)])
def test_num_blocks_matches_oracle(sw, numel, P):
    assert sw.num_blocks(numel, P) == O.num_blocks(numel, P)


def test_num_blocks_no_byte_count_overflow(sw):
    # numel * 4 would wrap 64 bits; the block count must not
    for numel, P in [(2 ** 62 + 1, 256), (2 ** 64 - 1, 64), (2 ** 64 - 1, 1024)]:
        assert sw.num_blocks(numel, P) == -(-numel // P)


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 7, 8, 16, 255, 256, 1000, 4096, 65535])
def test_host_scale_lut_matches_oracle(sw, W):
    assert np.array_equal(sw.scale_lut(W).view(np.uint32), O.scale_lut(W).view(np.uint32))


def test_argument_validation_without_gpu(sw):
    L = sw.lib()
    buf = (ctypes.c_float * 16)()
    pay = (ctypes.c_int32 * 1024)()
    # unsupported packet size
    assert L.sml_quantize_pack(buf, 16, 100, 1, None, pay, None, 0, None) == sw.SML_ERR_UNSUPPORTED
    assert L.sml_dequantize(pay, None, 16, 96, 1, buf, 0, None) == sw.SML_ERR_UNSUPPORTED
    # num_workers == 0
    assert L.sml_quantize_pack(buf, 16, 256, 0, None, pay, None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_scale_lut(0, buf) == sw.SML_ERR_INVALID_ARG
    # empty job slices are a no-op (dummy_worker_thread.cc:87 skips numel <= 0)
    assert L.sml_quantize_pack(None, 0, 256, 1, None, None, None, 0, None) == sw.SML_OK
    assert L.sml_dequantize(None, None, 0, 256, 1, None, 0, None) == sw.SML_OK
    assert L.sml_bswap_i32(None, None, 0, None) == sw.SML_OK
    # null payload with work to do
    assert L.sml_quantize_pack(buf, 16, 256, 1, None, None, None, 0, None) == sw.SML_ERR_INVALID_ARG
    # misaligned payload plane
    addr = ctypes.addressof(pay) + 4
    assert L.sml_quantize_pack(buf, 16, 256, 1, None, ctypes.c_void_p(addr), None, 0, None) == sw.SML_ERR_ALIGNMENT
    # loopback count must cover whole 16-byte vectors
    assert L.sml_loopback_aggregate(pay, 6, 2, 0, None) == sw.SML_ERR_ALIGNMENT
    # two checks fail at once: the earlier one decides
    vp = ctypes.c_void_p
    b, p16, bad = ctypes.addressof(buf), ctypes.addressof(pay), ctypes.addressof(pay) + 4
    exps = ctypes.addressof(pay) + 2048
    # bad packet size with num_workers == 0: sml_quantize_pack looks at num_workers first
    assert L.sml_quantize_pack(vp(b), 16, 100, 0, None, vp(p16), None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_dequantize(vp(p16), vp(exps), 16, 100, 0, vp(b), 0, None) == sw.SML_ERR_UNSUPPORTED
    assert L.sml_roundtrip_loopback(vp(b), vp(b), 16, 100, 0, None, None, 0, None) == sw.SML_ERR_UNSUPPORTED
    # null buffer with a misaligned payload plane
    assert L.sml_quantize_pack(None, 16, 256, 1, None, vp(bad), None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_dequantize(vp(bad), vp(exps), 16, 256, 1, None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_roundtrip_loopback(None, vp(b), 16, 256, 1, vp(bad), None, 0, None) == sw.SML_ERR_INVALID_ARG
    # fp32 buffer off its 4-byte alignment with a misaligned payload plane
    assert L.sml_exponents(vp(b + 2), 16, 256, vp(exps), None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_quantize_pack(vp(b + 2), 16, 256, 1, None, vp(bad), None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_dequantize(vp(bad), vp(exps), 16, 256, 1, vp(b + 2), 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_roundtrip_loopback(vp(b + 2), vp(b + 2), 16, 256, 1, vp(bad), None, 0, None) == sw.SML_ERR_INVALID_ARG
    # numel == 0 with null pointers: nothing to do, unless an earlier check fails
    assert L.sml_exponents(None, 0, 256, None, None) == sw.SML_OK
    assert L.sml_roundtrip_loopback(None, None, 0, 256, 1, None, None, 0, None) == sw.SML_OK
    assert L.sml_quantize_pack(None, 0, 256, 0, None, None, None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_dequantize(None, None, 0, 256, 0, None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_roundtrip_loopback(None, None, 0, 256, 0, None, None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_exponents(None, 0, 100, None, None) == sw.SML_ERR_UNSUPPORTED
    assert L.sml_quantize_pack(None, 0, 100, 1, None, None, None, 0, None) == sw.SML_ERR_UNSUPPORTED


def burst_maker(sw):
    """burst(ids, ...): a reference to a FLOAT32 sml_packet_burst over host
    buffers (B = 16 blocks of 256), for the checks that return before any HIP
    call.  The buffers live as long as the returned function."""
    x = (ctypes.c_float * 4096)()
    o = (ctypes.c_float * 4096)()
    recv = (ctypes.c_int8 * 16)()
    ring = (ctypes.c_int32 * 256)()
    extra = (ctypes.c_uint8 * 2)()

    def burst(ids, b=4, with_extra=True, count=None, null=(), packet_numel=256):
        bt = sw.PacketBurst()
        bt.in_ = None if "in" in null else ctypes.addressof(x)
        bt.out = None if "out" in null else ctypes.addressof(o)
        bt.numel = 4096
        bt.packet_numel = packet_numel         # 256: B = 16
        bt.num_workers = 1
        bt.data_type = 0
        bt.batch_num_ltus = b
        bt.recv_exps = ctypes.addressof(recv)
        bt.count = len(ids) if count is None else count
        for i, q in enumerate(ids):
            bt.pkt_ids[i] = q
            bt.entries[i] = ctypes.addressof(ring)
            bt.extras[i] = ctypes.addressof(extra) if with_extra else None
        return ctypes.byref(bt)

    return burst


def test_burst_validation_without_gpu(sw):
    """sml_{pre,post}process_burst / sml_exchange_burst refuse a malformed
    burst before any HIP call: too many packets, an id past B (+ b), a
    duplicate id, q and q + b together, a zero window for the exchange, a
    missing extra slot for a FLOAT32 packet that carries an exponent."""
    L = sw.lib()
    burst = burst_maker(sw)

    bad = sw.SML_ERR_INVALID_ARG
    for fn in (L.sml_preprocess_burst, L.sml_postprocess_burst, L.sml_exchange_burst):
        assert fn(burst([0], count=65), None) == bad           # > SML_MAX_BURST
        assert fn(burst([20]), None) == bad                    # q >= B + b
        assert fn(burst([3, 3]), None) == bad                  # duplicate
        assert fn(burst([5, 1]), None) == bad                  # q and q + b (any order)
        assert fn(burst([2], with_extra=False), None) == bad   # q < B needs its extra slot
        assert fn(burst([]), None) == sw.SML_OK                # nothing to do
    assert L.sml_exchange_burst(burst([1], b=0), None) == bad  # the exchange needs its window
    assert L.sml_exchange_burst(burst([1], b=17), None) == bad  # b > B


def test_burst_null_slice_pointer_status_order(sw):
    """Pre needs `in`, post needs `out`, the exchange needs both: a burst with
    packets and the forbidden NULL is an invalid argument, the same burst
    without packets is nothing to do, and with a bad packet size as well the
    earlier check (unsupported) decides."""
    L = sw.lib()
    burst = burst_maker(sw)
    for fn, null in ((L.sml_preprocess_burst, "in"), (L.sml_postprocess_burst, "out"),
                     (L.sml_exchange_burst, "in"), (L.sml_exchange_burst, "out")):
        assert fn(burst([1], null=(null,)), None) == sw.SML_ERR_INVALID_ARG
        assert fn(burst([], null=(null,)), None) == sw.SML_OK
        assert fn(burst([1], null=(null,), packet_numel=100), None) == sw.SML_ERR_UNSUPPORTED


def test_burst_server_validation_without_gpu(sw):
    """The burst server's entry points refuse bad arguments before any HIP
    call: no server, an unsupported packet size, unknown flags."""
    L = sw.lib()
    h = ctypes.c_void_p()
    assert L.sml_burst_server_create(100, 0, 0, ctypes.byref(h)) == sw.SML_ERR_UNSUPPORTED
    assert L.sml_burst_server_create(256, 0x8, 0, ctypes.byref(h)) == sw.SML_ERR_INVALID_ARG
    assert L.sml_burst_server_submit(None, 0, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_burst_server_stop(None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_burst_server_destroy(None) == sw.SML_OK


def test_switch_exps_validation_without_gpu(sw):
    """sml_switch_exps refuses bad arguments before any launch, in the order
    include/switchml_hip.h states: no workers / no table / no output, too
    many workers, nothing to do, a NULL plane inside the table."""
    L = sw.lib()
    vp = ctypes.c_void_p
    f = L.sml_switch_exps
    bad = sw.SML_ERR_INVALID_ARG
    table = (vp * 17)(*[16 + 4 * w for w in range(17)])
    tab = ctypes.cast(table, vp)
    out = vp(4096)
    assert f(tab, 0, 8, out, 0, None) == bad                       # W = 0
    assert f(None, 1, 8, out, 0, None) == bad                      # no table
    assert f(tab, 1, 8, None, 0, None) == bad                      # no output
    assert f(None, 0, 0, None, 0, None) == bad                     # ... even with nothing to do
    assert f(tab, 17, 8, out, 0, None) == sw.SML_ERR_UNSUPPORTED   # > SML_MAX_SWITCH_WORKERS
    assert f(tab, 17, 0, out, 0, None) == sw.SML_ERR_UNSUPPORTED   # the worker count is looked at first
    assert f(tab, 16, 0, out, 0, None) == sw.SML_OK                # num_blocks = 0
    assert f(tab, 16, 0, out, sw.FLAG_PEER_PLANES, None) == sw.SML_OK
    for hole in (0, 2, 15):
        holed = (vp * 16)(*[None if w == hole else 16 + 4 * w for w in range(16)])
        assert f(ctypes.cast(holed, vp), 16, 8, out, 0, None) == bad, hole
        assert f(ctypes.cast(holed, vp), 16, 0, out, 0, None) == sw.SML_OK   # the table is not read


def test_copy_words_validation_without_gpu(sw):
    """sml_copy_words: no words is nothing to do; a NULL or a pointer off its
    4-byte alignment, on either side, is an invalid argument."""
    L = sw.lib()
    vp = ctypes.c_void_p
    f = L.sml_copy_words
    bad = sw.SML_ERR_INVALID_ARG
    assert f(None, None, 0, None) == sw.SML_OK
    assert f(vp(17), vp(18), 0, None) == sw.SML_OK
    assert f(None, vp(32), 4, None) == bad
    assert f(vp(16), None, 4, None) == bad
    for off in (1, 2, 3):
        assert f(vp(16 + off), vp(32), 4, None) == bad, off
        assert f(vp(16), vp(32 + off), 4, None) == bad, off


def test_widen_narrow_u8_validation_without_gpu(sw):
    """sml_widen_u8_i32 / sml_narrow_i32_u8: n = 0 is nothing to do; a NULL on
    either side or an int32 side off its 4-byte alignment is an invalid
    argument.  (The uint8 side may start at any byte: such a call launches, so
    it is not made here.)"""
    L = sw.lib()
    vp = ctypes.c_void_p
    bad = sw.SML_ERR_INVALID_ARG
    widen, narrow = L.sml_widen_u8_i32, L.sml_narrow_i32_u8
    assert widen(None, None, 0, None) == sw.SML_OK
    assert widen(vp(17), vp(18), 0, None) == sw.SML_OK
    assert widen(None, vp(32), 4, None) == bad
    assert widen(vp(16), None, 4, None) == bad
    assert narrow(None, None, 0, None) == sw.SML_OK
    assert narrow(vp(18), vp(17), 0, None) == sw.SML_OK
    assert narrow(None, vp(32), 4, None) == bad
    assert narrow(vp(16), None, 4, None) == bad
    for off in (1, 2, 3):
        assert widen(vp(16), vp(32 + off), 4, None) == bad, off     # int32 output
        assert widen(vp(16 + off), vp(32 + off), 4, None) == bad, off
        assert narrow(vp(32 + off), vp(16), 4, None) == bad, off    # int32 input
        assert narrow(vp(32 + off), vp(16 + off), 4, None) == bad, off


def test_grid_limit_knob(sw):
    prev = sw.set_grid_limit(1024)
    assert sw.set_grid_limit(prev) == 1024


def test_xcd_chunk_knob_default_and_roundtrip(sw):
    """Workgroup order knob: default 64, returns the previous value."""
    prev = sw.set_xcd_chunk(7)
    assert prev == 64
    assert sw.set_xcd_chunk(prev) == 7


def test_python_wrapper_rejects_cpu_tensors(sw):
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="no CPU fallback"):
        sw.quantize_pack(torch.zeros(16))


def test_frames_and_rdma_validation_without_gpu(sw):
    L = sw.lib()
    fp = sw.frame_params()
    buf = (ctypes.c_float * 16)()
    frames = (ctypes.c_uint8 * 8192)()
    assert sw.frame_bytes(256) == FW.frame_bytes(256) and sw.frame_bytes(64) == FW.frame_bytes(64)
    # unsupported packet size / stride too small / stride not a multiple of 4
    assert L.sml_quantize_pack_frames(buf, 16, 100, 1, None, 64, ctypes.byref(fp), frames, 4096, None) == sw.SML_ERR_UNSUPPORTED
    assert L.sml_quantize_pack_frames(buf, 16, 256, 1, None, 64, ctypes.byref(fp), frames, 1000, None) == sw.SML_ERR_ALIGNMENT
    assert L.sml_quantize_pack_frames(buf, 16, 256, 1, None, 64, ctypes.byref(fp), frames, 1078, None) == sw.SML_ERR_ALIGNMENT
    # no params / batch 0 / W 0
    assert L.sml_quantize_pack_frames(buf, 16, 256, 1, None, 64, None, frames, 1076, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_quantize_pack_frames(buf, 16, 256, 1, None, 0, ctypes.byref(fp), frames, 1076, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_quantize_pack_frames(buf, 16, 256, 0, None, 64, ctypes.byref(fp), frames, 1076, None) == sw.SML_ERR_INVALID_ARG
    # empty slice: nothing to do
    assert L.sml_quantize_pack_frames(None, 0, 256, 1, None, 64, ctypes.byref(fp), None, 1076, None) == sw.SML_OK
    assert L.sml_rdma_imm(None, 0, 64, None, None) == sw.SML_OK
    assert L.sml_rdma_imm(None, 10, 64, None, None) == sw.SML_ERR_INVALID_ARG
    # a null exponent plane is an error for FLOAT32 even with d_imm given
    # (the INT32 immediates have their own entry point)
    assert L.sml_rdma_imm(None, 10, 64, ctypes.c_void_p(16), None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_rdma_imm_int32(0, None, None) == sw.SML_OK
    assert L.sml_rdma_imm_int32(10, None, None) == sw.SML_ERR_INVALID_ARG
    assert L.sml_debug_stall(0, None) == sw.SML_OK
    assert L.sml_debug_stall(60_000_001, None) == sw.SML_ERR_INVALID_ARG


def test_frame_params_layout_matches_header(sw):
    """The ctypes mirror of sml_frame_params has the C layout (offsets per the
    natural alignment of include/switchml_hip.h's struct)."""
    F = sw.FrameParams
    assert F.dst_mac.offset == 0 and F.src_mac.offset == 6
    assert F.src_ip_be.offset == 12 and F.dst_ip_be.offset == 16
    assert F.src_port_be.offset == 20 and F.dst_port_be.offset == 22
    assert F.job_id.offset == 24 and F.pool_index_start.offset == 32
    assert ctypes.sizeof(F) == 48


def test_rx_frames_validation_without_gpu(sw):
    L = sw.lib()
    frames = (ctypes.c_uint8 * 4096)()
    st = (ctypes.c_uint64 * 16)()
    ex = (ctypes.c_int8 * 16)()
    out = (ctypes.c_float * 16)()
    f = L.sml_dequantize_frames
    assert f(frames, 1, 1076, 16, 100, 1, 64, 0, ex, st, out, None, None) == sw.SML_ERR_UNSUPPORTED
    assert f(frames, 1, 1076, 16, 256, 0, 64, 0, ex, st, out, None, None) == sw.SML_ERR_INVALID_ARG
    assert f(frames, 1, 1076, 16, 256, 1, 0, 0, ex, st, out, None, None) == sw.SML_ERR_INVALID_ARG
    assert f(frames, 0, 1076, 16, 256, 1, 64, 0, None, None, None, None, None) == sw.SML_OK
    assert f(frames, 1, 1076, 16, 256, 1, 64, 0, ex, None, out, None, None) == sw.SML_ERR_INVALID_ARG
    assert f(frames, 1, 1000, 16, 256, 1, 64, 0, ex, st, out, None, None) == sw.SML_ERR_ALIGNMENT
    assert f(frames, 1, 1078, 16, 256, 1, 64, 0, ex, st, out, None, None) == sw.SML_ERR_ALIGNMENT
    assert f(frames, 2 ** 32, 1076, 16, 256, 1, 64, 0, ex, st, out, None, None) == sw.SML_ERR_UNSUPPORTED
    cnt = (ctypes.c_uint64 * 3)()
    assert f(frames, 1, 1076, 16, 256, 1, 64, 0, ex, st, out, ctypes.addressof(cnt) + 4, None) == sw.SML_ERR_ALIGNMENT


@pytest.mark.parametrize("header", ["switchml_hip.h", "switchml_client.h"])
def test_public_header_is_plain_c(header, tmp_path):
    """The drop-in boundary is a C ABI: each public header compiles on its own
    as strict C99 (what a cgo / JNI / N-API stub includes) and as C++11, with
    every warning an error."""
    import os
    import shutil
    import subprocess
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "inc.c"
    src.write_text(f'#include "{header}"\nint main(void) {{ return 0; }}\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        if not shutil.which(cc):
            pytest.skip(f"{cc} not found")
        lang = ["-x", "c++"] if cc == "g++" else []
        r = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", *lang, f"-I{inc}",
                            str(src)], capture_output=True, text=True)
        assert r.returncode == 0, (cc, r.stderr[-2000:])
