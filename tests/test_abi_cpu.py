"""switchml_amd/abi.py held to include/switchml_hip.h and
include/switchml_client.h (no GPU needed): every prototype of the signature
table type by type, every constant, the layout of the six structures as the
host C compiler lays them out, and the package's public surface."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

import switchml_amd
from switchml_amd import abi, client
from test_capi_cpu import header_prototypes

INCLUDE = os.path.dirname(abi.HEADER_PATH)
HEADERS = (abi.HEADER_PATH, abi.CLIENT_HEADER_PATH)

STRUCTS = {"sml_slice": abi.Slice, "sml_typed_slice": abi.TypedSlice, "sml_packet_burst": abi.PacketBurst,
           "sml_frame_params": abi.FrameParams, "sml_switch_worker": abi.SwitchWorker,
           "sml_frame_switch_params": abi.FrameSwitchParams}
# what is passed by value
SCALARS = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "uint16_t": ctypes.c_uint16,
           "int": ctypes.c_int, "sml_status_t": ctypes.c_int, "sml_data_type_t": ctypes.c_int}
# what a POINTER(...) of the table may point at, besides the above
POINTEES = dict(SCALARS, uint8_t=ctypes.c_uint8, int8_t=ctypes.c_int8, int32_t=ctypes.c_int32, float=ctypes.c_float)
POINTER_TYPEDEFS = {"sml_job_t"}        # typedef struct sml_job_s* sml_job_t


def stripped(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def c_type(decl, named):
    """(base type, pointer depth) of a parameter (`named`) or return type:
    const dropped, an array parameter decayed to a pointer, a pointer typedef
    counted as the pointer it is."""
    decl = re.sub(r"\bconst\b", " ", decl)
    depth = decl.count("*") + len(re.findall(r"\[[^\]]*\]", decl))
    words = re.sub(r"\[[^\]]*\]|\*", " ", decl).split()
    if named:
        words = words[:-1]
    base = " ".join(w for w in words if w != "struct")
    if base in POINTER_TYPEDEFS:
        depth += 1
    return base, depth


def allowed(base, depth):
    """The ctypes types the table may hold for a C type."""
    if depth == 0:
        return {None} if base == "void" else {SCALARS[base]}
    if depth == 1 and base in STRUCTS:
        return {ctypes.POINTER(STRUCTS[base])}
    if depth == 1 and base == "char":
        return {ctypes.c_char_p, ctypes.c_void_p}
    if depth == 1:
        return {ctypes.c_void_p} | ({ctypes.POINTER(POINTEES[base])} if base in POINTEES else set())
    return {ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)}


def typed_prototypes(path):
    """{function: ((base, depth) of the return type, [(base, depth) per parameter])}."""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?\**)\s*\b(sml_[a-z0-9_]+)\s*\(([^()]*)\)\s*;",
                                        stripped(path)):
        params = params.strip()
        plist = [] if params in ("", "void") else [c_type(p, named=True) for p in params.split(",")]
        protos[name] = (c_type(ret, named=False), plist)
    return protos


def test_c_type_parser():
    assert c_type("const int32_t* const* d_payloads", True) == ("int32_t", 2)
    assert c_type("float lut[256]", True) == ("float", 1)
    assert c_type("sml_job_t* job", True) == ("sml_job_t", 2)
    assert c_type("sml_job_t job", True) == ("sml_job_t", 1)
    assert c_type("const sml_frame_params* params", True) == ("sml_frame_params", 1)
    assert c_type("uint16_t num_workers", True) == ("uint16_t", 0)
    assert c_type("const char*", False) == ("char", 1)
    assert c_type("void", False) == ("void", 0)


def test_signature_table_equals_the_headers_type_by_type():
    """Every function of both headers is in the table, with the header's
    return type and the header's parameter list position by position, and the
    table holds nothing else; lib() has bound what the table says."""
    protos = {}
    for path in HEADERS:
        typed = typed_prototypes(path)
        counted = header_prototypes(path)
        assert sorted(typed) == sorted(counted) == abi.header_symbols(path)
        assert all(len(typed[n][1]) == counted[n][1] for n in typed)
        protos.update(typed)
    assert len(protos) == 67 + 15
    assert sorted(abi.SIGNATURES) == sorted(protos)      # nothing missing, nothing of its own
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = abi.SIGNATURES[name]
        if restype not in allowed(*ret):
            bad.append((name, "returns", ret, restype))
        if len(argtypes) != len(params):
            bad.append((name, "takes", len(params), len(argtypes)))
            continue
        bad += [(name, i, p, a) for i, (p, a) in enumerate(zip(params, argtypes)) if a not in allowed(*p)]
    assert not bad, bad
    L = abi.lib()
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def int_value(text):
    m = re.fullmatch(r"\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?[lL]*\s*\)?", text.strip())
    return None if m is None else int(m.group(1), 0)


def defines(path):
    """{name: value} of the header's #define SML_* with an integer value."""
    out = {}
    for name, text in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SML_\w+)[ \t]+(.+)$", stripped(path), flags=re.M):
        if int_value(text) is not None:
            out[name] = int_value(text)
    return out


def enumerators(path):
    """{name: value} over every enum of the header (an enumerator without a
    value is its predecessor's plus one)."""
    out = {}
    for body in re.findall(r"\benum\s*\w*\s*\{(.*?)\}", stripped(path), flags=re.S):
        nxt = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, text = (s.strip() for s in item.partition("="))
            nxt = int_value(text) if text else nxt
            out[name] = nxt
            nxt += 1
    return out


# a define without a Python constant, and why
NO_COUNTERPART = {
    "SML_ABI_VERSION": "the library reports it: held to sml_abi_version() instead",
    "SML_CTX_OK": "client.py raises ContextError on any non-zero code and puts the code in the message",
    "SML_CTX_ERR_STATE": "as SML_CTX_OK",
    "SML_CTX_ERR_CONFIG": "as SML_CTX_OK",
    "SML_CTX_ERR_ARG": "as SML_CTX_OK",
    "SML_CTX_ERR_FAILED": "as SML_CTX_OK",
}


def python_name(c_name):
    """switchml_hip.h: the status codes keep their names, everything else
    drops SML_ (SML_FLAG_X is FLAG_X, SML_FLOAT16 is FLOAT16)."""
    return c_name if c_name == "SML_OK" or c_name.startswith("SML_ERR_") else c_name[len("SML_"):]


def test_constants_equal_the_headers():
    hip = dict(defines(abi.HEADER_PATH), **enumerators(abi.HEADER_PATH))
    assert len(hip) == (1 + 4 + 5 + 3 + 5) + (5 + 4)      # version, flags, limits, ops, verdicts; status, types
    listed = set()
    for c_name, value in hip.items():
        if c_name in NO_COUNTERPART:
            listed.add(c_name)
            continue
        name = python_name(c_name)
        assert getattr(abi, name) == value, (c_name, value)
        assert getattr(switchml_amd, name) is getattr(abi, name)
    assert hip["SML_ABI_VERSION"] == abi.lib().sml_abi_version()
    # the client header: its defines are listed, its enums are client.py's constants
    for c_name in defines(abi.CLIENT_HEADER_PATH):
        assert c_name in NO_COUNTERPART, c_name
        listed.add(c_name)
    assert listed == set(NO_COUNTERPART)                   # no entry outlives its define
    enums = enumerators(abi.CLIENT_HEADER_PATH)
    assert len(enums) == 5 + 5 + 4 + 1
    for c_name, value in enums.items():
        m = re.fullmatch(r"SML_(?:CTX_|DT_|OP_|(JOB_))(\w+)", c_name)
        assert getattr(client, (m.group(1) or "") + m.group(2)) == value, (c_name, value)


def header_structs():
    """{struct: [field names in order]} of switchml_hip.h."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", stripped(abi.HEADER_PATH),
                                 flags=re.S):
        out[name] = [re.sub(r"\[[^\]]*\]", "", d).replace("*", " ").split()[-1]
                     for decl in filter(None, (s.strip() for s in body.split(";"))) for d in decl.split(",")]
    return out


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    """sizeof, and offsetof and size of every field, of the six structures as
    the host C compiler sees the header, against the ctypes mirrors; the
    fields are the header's, in the header's order (`in` is spelled in_)."""
    fields = header_structs()
    assert sorted(fields) == sorted(STRUCTS)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "switchml_hip.h"', "int main(void) {"]
    for s, names in fields.items():
        assert names == [n.rstrip("_") for n, _ in STRUCTS[s]._fields_], s
        lines.append(f'    printf("{s} %zu 0\\n", sizeof({s}));')
        lines += [f'    printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in names]
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    cc = next(filter(None, map(shutil.which, (os.environ.get("CC", "cc"), "cc", "gcc", "clang"))), None)
    assert cc, "the host C compiler the Makefile builds capi_roundtrip with"
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c11", f"-I{INCLUDE}", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, a, b = line.split()
        seen[key] = (int(a), int(b))
    want = {}
    for s, T in STRUCTS.items():
        want[s] = (ctypes.sizeof(T), 0)
        for n, _ in T._fields_:
            want[f"{s}.{n.rstrip('_')}"] = (getattr(T, n).offset, getattr(T, n).size)
    assert seen == want, {k: (seen.get(k), want.get(k)) for k in set(seen) | set(want) if seen.get(k) != want.get(k)}


PUBLIC = """BFLOAT16 BURST_EXCHANGE BURST_POST BURST_PRE BurstServer FLAG_PAYLOAD_LE FLAG_PEER_PLANES
FLAG_PROCESS_PACKET FLAG_ROUND_RNE FLOAT16 FLOAT32 FrameParams FrameSwitch FrameSwitchParams HEADER_PATH INT32
LIB_PATH MAX_BATCH_SLICES MAX_BURST MAX_FRAME_SWITCH_SLOTS MAX_FRAME_SWITCH_WORKERS MAX_SWITCH_WORKERS PACKET_NUMELS
PacketBurst RxSlice RxSliceInt32 SML_ERR_ALIGNMENT SML_ERR_HIP SML_ERR_INVALID_ARG SML_ERR_UNSUPPORTED SML_OK Slice
SwitchMLError SwitchWorker TypedSlice VERDICT_BROADCAST VERDICT_CONSUMED VERDICT_DEFERRED VERDICT_IGNORED
VERDICT_RETRANSMIT bswap_i32 copy_segments copy_segments_typed copy_words debug_stall dequantize dequantize_frames
exchange_burst exponents fifo_slice frame_bytes frame_params frame_switch_params gather_frames header_symbols lib
loopback_aggregate narrow_i32_u8 num_blocks pack_frames_int32 packet_burst postprocess_burst preprocess_burst
quantize_pack quantize_pack_frames quantize_pack_launcher rdma_imm release_to_peers roundtrip_loopback
roundtrip_loopback_batch scale_lut scale_lut_device set_grid_limit set_payload_nt_threshold set_quantize_tile_slices
set_stream_tile_slices set_xcd_chunk shard_quantize_pack stream_copy switch_aggregate switch_exps
unpack_frames_int32 widen_u8_i32""".split()


def test_public_surface():
    """The package holds the 83 public names, each the object one of its
    submodules defines."""
    from switchml_amd import frame_switch, frames, knobs, packets, planes, switch
    assert len(PUBLIC) == len(set(PUBLIC)) == 83
    owners = (abi, planes, switch, packets, frames, frame_switch, knobs)
    missing = object()
    for name in PUBLIC:
        obj = getattr(switchml_amd, name)
        assert any(getattr(m, name, missing) is obj for m in owners), name
    for name in PUBLIC:
        if callable(getattr(switchml_amd, name)):
            assert getattr(switchml_amd, name).__module__.startswith("switchml_amd."), name


def test_import_loads_neither_torch_nor_numpy_nor_the_library():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import switchml_amd; "
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules, sorted(sys.modules); "
            "assert switchml_amd.abi._lib is None")
    pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(switchml_amd.__file__)))
    r = subprocess.run([sys.executable, "-c", code, pkg_parent], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
