"""Writes tests/golden/ref_vectors.json: results produced by the COMPILED
reference (oracle/_ref/, built by oracle/ref/Makefile where the reference
checkout exists).  Data only: numbers, names and digests, no program text.

    python tests/golden/make_ref_vectors.py          # rewrites the fixture

tests/test_ref_vectors.py calls make() where oracle/_ref/ exists and requires
the committed file to equal it, so the fixture cannot go stale or be edited by
hand.  The reading side, the input specs and the stored form of a plane are in
tests/ref_vectors.py.

Every PPP record runs one job slice through the reference's
CpuExponentQuantizerPPP packet by packet, in its release AND debug builds
(asserted equal here), with the dummy backend's x W between send and receive.
Recorded: the exponent plane, the payload words [0, numel) (under the recorded
global exponents where the record has them), and the output bits.  The
generator asserts that at most 1 % of a record's outputs are NaN, which is
what lets the GPU test compare >= 99 % of the positions by bits.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_vectors as RV  # noqa: E402
from oracle import oracle as O  # noqa: E402

MAX_BYTES = 64 * 1024
KATS = ("ties_half_away", "all_zero_block", "tiny_block_e_minus102", "block_max_e_minus96_97", "denormals",
        "nan_skipped_in_max", "inf_block", "huge_e128_wraps", "W3_nonpow2_scale", "W8_pattern",
        "partial_last_block", "global_exps_smaller_wraps", "global_exps_larger", "W65535", "P256_mixed")


def _kat_case(name):
    with open(os.path.join(HERE, "kat_vectors.json")) as f:
        return [c for c in json.load(f)["cases"] if c["name"] == name][0]


def ppp_specs():
    """(name, P, W, batch, input spec, global exponents: None | list | ("below", k) | ("at", {block: e}))."""
    out = []
    for name in KATS:                        # the hand-derived cases' inputs, now with the reference's answers
        c = _kat_case(name)
        out.append(("kat_" + name, c["P"], c["W"], 64, {"gen": "kat", "name": name}, c["global_exps"]))
    grad = lambda seed, n, **kw: dict({"gen": "splitmix_grad", "seed": seed, "n": n}, **kw)
    rnd = lambda seed, n, **kw: dict({"gen": "ref_random_floats", "seed": seed, "n": n}, **kw)
    specials = [[5, "7fc00000"], [70, "7f800000"], [71, "ff800000"], [130, "00000001"], [131, "807fffff"],
                [200, "7f7fffff"], [201, "00800000"]]
    out += [
        ("one_element", 1024, 8, 64, grad(1, 1), None),
        ("three_elements_W65535", 128, 65535, 2, grad(2, 3), None),
        ("p64_partial_W3", 64, 3, 64, grad(3, 4113), None),
        ("p64_glibc_W1_batch1", 64, 1, 1, rnd(4, 1025), None),
        ("p128_glibc_W1", 128, 1, 64, rnd(5, 8192), None),
        ("p128_below_own_W3", 128, 3, 2, grad(6, 1023), ("below", 7)),
        ("p256_pattern_W8", 256, 8, 64, {"gen": "ref_pattern_floats", "n": 1025}, None),
        ("p256_specials_W3", 256, 3, 64, grad(7, 257, patch=specials), None),
        ("p256_below_own_W8", 256, 8, 64, grad(8, 4113), ("below", 33)),
        ("p512_W65535", 512, 65535, 64, grad(9, 5000), None),
        ("p512_glibc_below_own", 512, 1, 4, rnd(10, 2049), ("below", 3)),
        ("p1024_glibc_W1", 1024, 1, 64, rnd(11, 8191), None),
        ("p1024_tiny_W3", 1024, 3, 64, grad(12, 1025, shift=-90), None),      # blocks around e = -96 / -97
        ("p64_huge_W8", 64, 8, 64, grad(13, 255, shift=129), None),           # e up to 128 -> int8 -128
        # one 64-element block whose scale is 0 (3 * 2^127 overflows float): 64 of 6400 outputs are 0/0
        ("scale_zero_block", 64, 3, 64, grad(14, 6400), ("at", {37: 127})),
    ]
    return out


def global_exps(rule, own):
    if rule is None:
        return None
    if isinstance(rule, list):
        return np.array(rule, dtype=np.int8)
    kind, arg = rule
    e = own.astype(np.int32)
    if kind == "below":                      # 1 .. 40 below the own ones, every third block above
        k = np.arange(e.size)
        e = np.where(k % 3 == 2, e + 1 + k % 4, e - 1 - (k * arg) % 40)
    else:
        for blk, v in arg.items():
            e[int(blk)] = v
    return np.clip(e, -128, 127).astype(np.int8)


def ppp_record(name, P, W, batch, spec, rule):
    x = RV.make_input(spec)
    n = x.size
    ge = global_exps(rule, O.exponents(x, P))
    r = O.ref_packet_stream(x, P, W, batch, debug=False, global_exps=ge, aggregate=True)
    d = O.ref_packet_stream(x, P, W, batch, debug=True, global_exps=ge, aggregate=True)
    B, b = r["B"], r["b"]
    exps = r["tx_extra"][:B, 0].copy()
    payload = r["tx"][b:].reshape(-1)[:n].copy()
    assert np.array_equal(exps, d["tx_extra"][:B, 0]) and np.array_equal(payload, d["tx"][b:].reshape(-1)[:n])
    assert np.array_equal(r["out"].view(np.uint32), d["out"].view(np.uint32)), (name, "release and debug differ")
    assert np.isnan(r["out"]).mean() <= 0.01, (name, "more than 1 % of the reference's outputs are NaN")
    full = n <= RV.FULL_MAX
    assert n <= 8192
    return {"name": name, "P": P, "W": W, "batch": batch, "n": n, "input": spec,
            "global_exps": None if ge is None else [int(v) for v in ge],
            "exps": RV.record_plane(exps, 2, full), "payload": RV.record_plane(payload, 8, full),
            "out": RV.record_plane(r["out"], 8, full, is_float=True)}


def half_bits(T, n):
    """Finite 16-bit patterns over the type's whole exponent range (integer
    arithmetic only), a zero block, denormals, the largest finite value, ties."""
    i = np.arange(n, dtype=np.uint64)
    b = ((i * np.uint64(40503) + np.uint64(977)) * np.uint64(2654435761) >> np.uint64(9)).astype(np.uint16)
    # no inf / NaN; bf16 stays below 2^124, so that 3 * 2^e does not overflow (a scale of 0)
    expmask, limit, top = (0x7C00, 0x7C00, 0x7BFF) if T == "fp16" else (0x7F80, 0x7D00, 0x7CFF)
    b = np.where((b & expmask) >= limit, b & np.uint16(0xBFFF), b).astype(np.uint16)
    b[64:128] = 0
    b[130], b[131], b[132], b[133] = 0x0001, 0x8001, top, 0x8000 | top
    return b


def half_record(T):
    P, W, batch = 64, 3, 2
    spec = {"type": T, "bits16": RV.hexwords(half_bits(T, 200), 4)}
    _, x = RV.half_input(spec)
    r = O.ref_packet_stream(x, P, W, batch, aggregate=True)
    d = O.ref_packet_stream(x, P, W, batch, debug=True, aggregate=True)
    assert np.array_equal(r["out"].view(np.uint32), d["out"].view(np.uint32))
    assert not np.isnan(r["out"]).any()
    B, b, n = r["B"], r["b"], x.size
    return {"name": "exact_in_" + T, "P": P, "W": W, "batch": batch, "n": n, "input": spec, "global_exps": None,
            "exps": RV.record_plane(r["tx_extra"][:B, 0].copy(), 2, True),
            "payload": RV.record_plane(r["tx"][b:].reshape(-1)[:n].copy(), 8, True),
            "out": RV.record_plane(r["out"], 8, True, is_float=True)}


CONTEXT = [
    # name, n, T, mop, P, W, type, inplace, process_packets, input
    ("f32_T4_general_cfg", 100_003, 4, 256, 256, 2, "f32", False, True, {"gen": "splitmix_grad", "seed": 21}),
    ("f32_T1_mop1", 1000, 1, 1, 64, 1, "f32", False, True, {"gen": "ref_random_floats", "seed": 22}),
    ("f32_T3_ragged_inplace", 65_537, 3, 64, 1024, 8, "f32", True, True, {"gen": "splitmix_grad", "seed": 23}),
    ("f32_T8_mop8", 100_003, 8, 8, 64, 3, "f32", True, True, {"gen": "ref_pattern_floats"}),
    ("f32_T2_glibc", 65_537, 2, 256, 256, 1, "f32", False, True, {"gen": "ref_random_floats", "seed": 25}),
    ("f32_T4_n3_empty_slice", 3, 4, 64, 256, 3, "f32", False, True, {"gen": "splitmix_grad", "seed": 26}),
    ("f32_T2_no_process", 1000, 2, 64, 256, 8, "f32", False, False, {"gen": "splitmix_grad", "seed": 27}),
    ("f32_T3_p64_W8", 100_003, 3, 256, 64, 8, "f32", False, True, {"gen": "splitmix_grad", "seed": 28}),
    ("i32_T4_W3", 100_003, 4, 256, 256, 3, "i32", False, True, {"gen": "glibc_i32", "seed": 29}),
    ("i32_T3_inplace_W8", 65_537, 3, 64, 1024, 8, "i32", True, True, {"gen": "glibc_i32", "seed": 30}),
]


def context_record(name, n, T, mop, P, W, typ, inplace, process, spec):
    spec = dict(spec, n=n)
    x = RV.make_input(spec)
    assert x.dtype == (np.float32 if typ == "f32" else np.int32) and n <= 100_003
    out = O.ref_allreduce(x, P=P, num_workers=W, num_worker_threads=T, max_outstanding_packets=mop,
                          process_packets=process, inplace=inplace)
    if typ == "f32":
        assert np.isnan(out).mean() <= 0.01
    return {"name": name, "n": n, "T": T, "mop": mop, "P": P, "W": W, "type": typ, "inplace": inplace,
            "process_packets": process, "input": spec,
            "out": RV.record_plane(out, 8, False, is_float=(typ == "f32"))}


def make():
    return {
        "generator": "tests/golden/make_ref_vectors.py",
        "source": "outputs of the reference's CpuExponentQuantizerPPP (release and debug builds, equal) and of its "
                  "dummy-backend Context, VCL=0",
        "ppp": [ppp_record(*s) for s in ppp_specs()],
        "half": [half_record("bf16"), half_record("fp16")],
        "context": [context_record(*c) for c in CONTEXT],
    }


def dumps(doc):
    """One record per line."""
    one = lambda v: json.dumps(v, separators=(",", ":"))
    parts = [f'"{k}":{one(doc[k])}' for k in ("generator", "source")]
    parts += [f'"{k}":[\n' + ",\n".join(one(r) for r in doc[k]) + "\n]" for k in ("ppp", "half", "context")]
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    if not O.ref_available():
        sys.exit("oracle/_ref/ is not built: the fixture can only be made where the reference checkout exists")
    text = dumps(make())
    assert len(text.encode()) <= MAX_BYTES, f"{len(text.encode())} bytes > {MAX_BYTES}"
    with open(RV.PATH, "w") as f:
        f.write(text)
    print(f"wrote {RV.PATH}: {len(text.encode())} bytes")
