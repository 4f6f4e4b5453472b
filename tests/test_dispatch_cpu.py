"""csrc/sml_dispatch.h on its own (CPU, a host compiler only): every launch
site picks its kernel instance through these helpers, so a constant that
reaches the lambda with another value, or in another position, than the
runtime argument it came from would launch the wrong kernel without any
compile error.

A stand-alone program (its own main) includes the header alone and checks,
for every packet size and every combination of four flags, that the lambda
receives constants equal to the runtime values in argument order; that an
unlisted packet size takes the 1024 branch; and that the slices helper maps
listed values to themselves and anything else to the last listed.  Built
plain and once more with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p4app-switchml_amd", "csrc")

PROGRAM = r"""
#include "sml_dispatch.h"

#include <stdio.h>

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

int main() {
    using namespace sml;
    const uint32_t packets[] = {64, 128, 256, 512, 1024};
    int calls = 0;
    for (uint32_t P : packets)
        for (int m = 0; m < 16; m++) {
            const bool a = m & 1, b = m & 2, c = m & 4, d = m & 8;
            int here = 0;
            dispatch_packet(P, [&](auto Pc) {
                dispatch_bools([&](auto A, auto B, auto C, auto D) {
                    // constants, usable as template arguments
                    constexpr int p = Pc();
                    constexpr bool ca = A(), cb = B(), cc = C(), cd = D();
                    CHECK((uint32_t)p == P);
                    CHECK(ca == a && cb == b && cc == c && cd == d);
                    here++;
                }, a, b, c, d);
            });
            CHECK(here == 1);
            calls += here;
        }
    CHECK(calls == 5 * 16);
    // argument order with flags that differ pairwise
    dispatch_bools([&](auto A, auto B, auto C) { CHECK(A() && !B() && C()); calls++; }, true, false, true);
    dispatch_bools([&](auto A, auto B) { CHECK(!A() && B()); calls++; }, false, true);
    dispatch_bools([&](auto A) { CHECK(A()); calls++; }, true);
    CHECK(calls == 5 * 16 + 3);
    // an invalid packet size takes the 1024 branch
    const uint32_t invalid[] = {0, 1, 63, 100, 2048, 0xFFFFFFFFu};
    for (uint32_t P : invalid) {
        int got = 0;
        dispatch_packet(P, [&](auto Pc) { got = Pc(); });
        CHECK(got == 1024);
    }
    // slices: listed values map to themselves, anything else to the last listed
    for (uint32_t U = 0; U <= 5; U++) {
        int g124 = -1, g24 = -1;
        dispatch_slices<1, 2, 4>(U, [&](auto Uc) { constexpr int u = Uc(); g124 = u; });
        dispatch_slices<2, 4>(U, [&](auto Uc) { g24 = Uc(); });
        CHECK(g124 == (U == 1 || U == 2 ? (int)U : 4));
        CHECK(g24 == (U == 2 ? 2 : 4));
    }
    if (failures) return 1;
    printf("dispatch ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("dispatch")
    src = d / "dispatch_check.cc"
    src.write_text(PROGRAM)
    return cxx, d, src


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_dispatch_header_standalone(source, sanitize):
    cxx, d, src = source
    exe = d / ("check_san" if sanitize else "check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else ["-O2"]
    # the header alone: no HIP include path, no other project header
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                            "-o", str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "dispatch ok"


def test_dispatch_header_needs_no_hip():
    with open(os.path.join(CSRC, "sml_dispatch.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(includes) == ["<stdint.h>", "<type_traits>"]
