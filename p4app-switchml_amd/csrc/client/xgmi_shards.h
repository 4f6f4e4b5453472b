// xgmi_shards.h — how the in-node switch (xgmi_switch.cc) deals a chunk of n
// elements, B = ceil(n / P) blocks of P, to its W workers: worker w owns
// S = ceil(B / W) blocks from block w S on, the last shards shorter or empty
// (switchml_amd/p2pswitch.py, shard_blocks, is the same rule).  No HIP in
// here: the plan is arithmetic, tested on a CPU (tests/test_xgmi_shards_cpu.py).
#ifndef SWITCHML_AMD_XGMI_SHARDS_H_
#define SWITCHML_AMD_XGMI_SHARDS_H_

#include <algorithm>
#include <cstdint>

namespace switchml {

struct Shard {
    uint64_t b0;      // first block
    uint64_t nb;      // blocks; 0: an empty shard, which launches nothing
    uint64_t offset;  // b0 P: its first element, in the chunk and in every plane
    uint64_t numel;   // its elements: whole blocks but for the chunk's ragged last one
    uint64_t words;   // nb P: whole blocks (what the INT32 aggregate sums)
};

struct ShardPlan {
    uint64_t n, P, W;
    uint64_t B;   // blocks of the chunk
    uint64_t S;   // blocks per shard

    ShardPlan(uint64_t numel, uint64_t packet_numel, uint64_t workers)
        : n(numel), P(packet_numel), W(workers), B((n + P - 1) / P), S((B + W - 1) / W) {}

    Shard shard(uint64_t w) const {
        const uint64_t b0 = std::min(w * S, B);
        const uint64_t nb = std::min(S, B - b0);
        return Shard{b0, nb, b0 * P, nb ? std::min(nb * P, n - b0 * P) : 0, nb * P};
    }

    // Push form: where worker r's row starts in an inbox (W rows of S blocks,
    // so its end W S P can pass B P by up to W − 1 blocks).
    uint64_t inbox_row(uint64_t r) const { return r * S * P; }
};

}  // namespace switchml

#endif  // SWITCHML_AMD_XGMI_SHARDS_H_
