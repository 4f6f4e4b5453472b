"""csrc/client/xgmi_shards.h on its own (CPU, a host compiler only): which
blocks of a chunk each of the W workers of the in-node switch aggregates,
pushes and gathers — S = ceil(B / W) blocks per worker, the last shards
shorter or empty — is otherwise reached only by the multi-process GPU runs
(test_xgmi_switch.py), where an off-by-one shows as a bit mismatch on one rank.

A stand-alone program (its own main) includes the header and walks the grid
n x P x W below.  It restates the rules (disjoint shards in rank order that
cover blocks [0, B); element counts that sum to n; offsets b0 P; nothing in an
empty shard; whole-block words nb P; the inbox rows inside what the payload
plane allocates) without calling the plan to check the plan, and prints every
shard.  Built with the host compiler, plain and once more with the address
and undefined-behaviour sanitizers, and run directly.  The Python side reads
the printed shards and holds switchml_amd.p2pswitch.shard_blocks, the same
rule in the p2p switch, against them."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "p4app-switchml_amd")
CLIENT = os.path.join(PKG, "csrc", "client")

PROGRAM = r"""
#include "xgmi_shards.h"

#include <stdio.h>

using namespace switchml;

static int failures = 0;
static uint64_t g_n, g_P, g_W;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            printf("line %d (n %llu P %llu W %llu): %s\n", __LINE__, (unsigned long long)g_n, \
                   (unsigned long long)g_P, (unsigned long long)g_W, #cond);                 \
            failures++;                                                                      \
        }                                                                                    \
    } while (0)

static void check(uint64_t n, uint64_t P, uint64_t W) {
    g_n = n, g_P = P, g_W = W;
    const ShardPlan plan(n, P, W);
    // blocks: the last one may be ragged
    uint64_t B = 0;
    while (B * P < n) B++;
    CHECK(plan.n == n && plan.P == P && plan.W == W && plan.B == B);
    // S: the least block count with which W shards cover B blocks
    CHECK(plan.S * W >= B && (plan.S == 0 || (plan.S - 1) * W < B));
    uint64_t next_block = 0, elements = 0;
    for (uint64_t w = 0; w < W; w++) {
        const Shard sh = plan.shard(w);
        printf("shard %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)P,
               (unsigned long long)W, (unsigned long long)B, (unsigned long long)w, (unsigned long long)sh.b0,
               (unsigned long long)sh.nb);
        // disjoint, in rank order, no gap: each shard starts where the one before ended
        CHECK(sh.b0 == next_block && sh.b0 + sh.nb <= B);
        next_block = sh.b0 + sh.nb;
        // every shard but the last non-empty one is full; none is longer
        CHECK(sh.nb <= plan.S && (sh.nb == plan.S || next_block == B));
        CHECK(sh.offset == sh.b0 * P);
        CHECK(sh.words == sh.nb * P);
        if (sh.nb == 0) {
            CHECK(sh.numel == 0 && sh.words == 0 && sh.b0 == B);
        } else {
            // whole blocks, but for the chunk's ragged last block
            const uint64_t end = next_block == B ? n : next_block * P;
            CHECK(sh.numel == end - sh.b0 * P && sh.numel > 0 && sh.numel <= sh.words);
            CHECK(sh.offset + sh.numel <= n);
        }
        elements += sh.numel;
        CHECK(plan.inbox_row(w) == w * plan.S * P);
    }
    CHECK(next_block == B);
    CHECK(elements == n);
    // the last inbox row's end, against what the payload plane allocates past
    // the chunk: W - 1 packets
    CHECK(W * plan.S * P <= B * P + (W - 1) * P);
}

int main() {
    const uint64_t Ps[] = {64, 256, 1024};
    const uint64_t Ws[] = {1, 2, 3, 5, 16};
    for (uint64_t P : Ps)
        for (uint64_t W : Ws) {
            const uint64_t ns[] = {1, P - 1, P, P + 1, W * P - 1, W * P, W * P + 1, 4 * P * W + 5, 100003};
            for (uint64_t n : ns) check(n, P, W);
        }
    if (failures) return 1;
    printf("xgmi shards ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("xgmi_shards")
    src = d / "xgmi_shards_check.cc"
    src.write_text(PROGRAM)
    return cxx, d, src


def _build_and_run(source, sanitize):
    cxx, d, src = source
    exe = d / ("check_san" if sanitize else "check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else ["-O2"]
    # the header alone: no HIP include path, no kernel C-ABI header
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CLIENT,
                            "-o", str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "xgmi shards ok"
    return [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("shard ")]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_xgmi_shards_standalone(source, sanitize):
    shards = _build_and_run(source, sanitize)
    # the whole grid was walked: 3 P x 9 n x the W shards of W in {1, 2, 3, 5, 16}
    assert len(shards) == 3 * 9 * (1 + 2 + 3 + 5 + 16)
    cases = {s[:3] for s in shards}
    assert len(cases) == 3 * 5 * 9 - 3 * 3    # at W = 1, n = W P - 1, W P, W P + 1 repeat P - 1, P, P + 1
    assert any(B < W for _, _, W, B, _, _, _ in shards)          # trailing shards empty
    assert any(n % P for n, P, _, _, _, _, _ in shards)          # a ragged last block


def test_p2pswitch_shard_blocks_agrees(source):
    """The p2p switch's Python rule gives the same (first block, block count)
    as the header for every worker of every case of the grid."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from switchml_amd.p2pswitch import shard_blocks   # torch only: no GPU, no library load
    shards = _build_and_run(source, False)
    assert shards
    for n, P, W, B, w, b0, nb in shards:
        assert shard_blocks(B, W, w) == (b0, nb), (n, P, W, B, w)


def test_xgmi_shards_header_needs_no_hip():
    with open(os.path.join(CLIENT, "xgmi_shards.h")) as f:
        includes = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<cstdint>"]


def test_shard_rule_lives_in_the_header_only():
    """No file of the client but xgmi_shards.h derives a shard by hand."""
    for name in sorted(os.listdir(CLIENT)):
        if name == "xgmi_shards.h" or not name.endswith((".h", ".cc")):
            continue
        with open(os.path.join(CLIENT, name)) as f:
            text = f.read()
        for formula in ("+ W_ - 1) / W_", "* S * P_", "B - b0", "B - blk0"):
            assert formula not in text, (name, formula)
