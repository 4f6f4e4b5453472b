"""Reading side of tests/golden/ref_vectors.json: results RECORDED FROM THE
COMPILED REFERENCE (tests/golden/make_ref_vectors.py), shared by
test_ref_vectors.py (the oracle reproduces them; the file is regenerated where
the reference is built) and test_ref_vectors_gpu.py (the HIP kernels and the
client are held to them directly, not through the oracle).

The fixture holds numbers, names and digests only.  Inputs are rebuilt from a
spec: a generator of oracle/oracle.py by name and seed (integer arithmetic
only, the same bytes on every host), a case of kat_vectors.json by name, or
explicit bit patterns; `patch` then overwrites single elements.

A plane is stored in full as one hex string (records of <= 300 elements) or as
its SHA-256 plus its first 16 words.  Float outputs also store where the
reference produced a NaN (`nan_at`, [start, stop) ranges) and `sha256` is taken
with those words set to 0x7fc00000: gfx950 and x86 differ in the sign of the
0/0 NaN (the project's NaN rule), everything else is compared by bits;
`sha256_raw` covers the reference's own words, NaN bits included.
"""
import hashlib
import json
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "ref_vectors.json")
FULL_MAX = 300
CANONICAL_NAN = 0x7FC00000


def load():
    with open(PATH) as f:
        return json.load(f)


def _kat(name):
    with open(os.path.join(GOLDEN, "kat_vectors.json")) as f:
        c = [c for c in json.load(f)["cases"] if c["name"] == name][0]
    return np.array([int(h, 16) for h in c["x_bits"]], dtype=np.uint32).view(np.float32)


def glibc_i32(seed, n):
    """Signed 32-bit integers from glibc's rand() stream (integer arithmetic only)."""
    r = O.c_glibc_rand(seed, n).astype(np.uint64)
    return ((r * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def make_input(spec):
    """float32 / int32 input of a record (16-bit records: see half_input)."""
    g = spec["gen"]
    if g == "splitmix_grad":
        x = O.splitmix_grad(spec["seed"], spec["n"])
        x = np.ldexp(x, spec.get("shift", 0)).astype(np.float32)
    elif g == "ref_random_floats":
        x = O.c_ref_random_floats(spec["seed"], spec["n"])
    elif g == "ref_pattern_floats":
        x = O.ref_pattern_floats(spec["n"])
    elif g == "glibc_i32":
        x = glibc_i32(spec["seed"], spec["n"])
    elif g == "kat":
        x = _kat(spec["name"])
    elif g == "bits":
        x = unhex(spec["bits"], 8).view(np.float32)
    else:
        raise ValueError(g)
    x = np.array(x, copy=True)
    for i, h in spec.get("patch", []):
        x.view(np.uint32)[i] = int(h, 16)
    for lo, hi in spec.get("zero", []):
        x[lo:hi] = 0
    return x


def half_input(spec):
    """(raw uint16 patterns, the exactly widened float32) of a 16-bit record."""
    b = unhex(spec["bits16"], 4).astype(np.uint16)
    if spec["type"] == "fp16":
        return b, b.view(np.float16).astype(np.float32)
    return b, (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def hexwords(a, width):
    a = np.ascontiguousarray(a)
    a = a.view({8: np.uint32, 4: np.uint16, 2: np.uint8}[width])
    return "".join(f"{int(v):0{width}x}" for v in a)


def unhex(s, width):
    dt = {8: np.uint32, 4: np.uint16, 2: np.uint8}[width]
    return np.array([int(s[i:i + width], 16) for i in range(0, len(s), width)], dtype=dt)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def nan_ranges(mask):
    idx = np.flatnonzero(mask)
    out = []
    for i in idx:
        if out and out[-1][1] == i:
            out[-1][1] = int(i) + 1
        else:
            out.append([int(i), int(i) + 1])
    return out


def nan_mask(ranges, n):
    m = np.zeros(n, dtype=bool)
    for lo, hi in ranges:
        m[lo:hi] = True
    return m


def record_plane(a, width, full, is_float=False):
    """The stored form of one plane (see the module docstring)."""
    a = np.ascontiguousarray(a)
    u = a.view({8: np.uint32, 2: np.uint8}[width])
    rec = {}
    if is_float:
        nan = np.isnan(a.view(np.float32))
        canon = np.where(nan, np.uint32(CANONICAL_NAN), u)
        rec["nan_at"] = nan_ranges(nan)
    if full:
        rec["hex"] = hexwords(u, width)
    else:
        rec["first16"] = hexwords(u[:16], width)
        rec["sha256_raw" if is_float else "sha256"] = sha(u)
        if is_float:
            rec["sha256"] = sha(canon)
    return rec


def check_plane(got, rec, width, what, exact_nan=False):
    """Assert that `got` is the recorded plane.  Float planes (those with
    nan_at): a recorded NaN must be a NaN, every other word equal by bits, and
    at least 99 % of the words compared by bits; exact_nan = True (the CPU
    oracle) compares the NaN words by bits too."""
    got = np.ascontiguousarray(got)
    u = got.view({8: np.uint32, 2: np.uint8}[width])
    is_float = "nan_at" in rec
    if is_float:
        nan = nan_mask(rec["nan_at"], u.size)
        assert np.isnan(got.view(np.float32)[nan]).all(), f"{what}: the reference recorded a NaN, got a number"
        assert not np.isnan(got.view(np.float32)[~nan]).any(), f"{what}: NaN where the reference has a number"
        if u.size:
            assert (~nan).mean() >= 0.99, f"{what}: only {(~nan).mean():.4f} of the positions compared by bits"
        cmp_u = u if exact_nan else np.where(nan, np.uint32(CANONICAL_NAN), u)
    else:
        cmp_u = u
    if "hex" in rec:
        want = unhex(rec["hex"], width)
        if is_float and not exact_nan:
            want = np.where(nan, np.uint32(CANONICAL_NAN), want)
        assert cmp_u.size == want.size, f"{what}: {cmp_u.size} words, recorded {want.size}"
        bad = np.flatnonzero(cmp_u != want)
        assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {bad[0]}: got {int(cmp_u[bad[0]]):#x}, "
                               f"recorded {int(want[bad[0]]):#x}")
    else:
        first = unhex(rec["first16"], width)
        k = first.size
        if is_float and not exact_nan:
            first = np.where(nan[:k], np.uint32(CANONICAL_NAN), first)
        assert np.array_equal(cmp_u[:k], first), f"{what}: first words {hexwords(cmp_u[:k], width)}, recorded {rec['first16']}"
        key = "sha256_raw" if (is_float and exact_nan) else "sha256"
        assert sha(cmp_u) == rec[key], f"{what}: digest differs from the recorded one"
