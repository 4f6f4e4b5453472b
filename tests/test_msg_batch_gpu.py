"""The batched round trip for long messages on the GPU
(sml_msg_roundtrip_loopback_batch): every slice bit-exact against the CPU
oracle at P = msg_numel, by test_messages_gpu.py's recipe (each slice a view one
element into a guarded allocation of its own, 16-bit types through torch's CPU
narrow)."""
import pytest

from oracle import oracle as O
from test_half_gpu import sw, words_equal
from test_messages_gpu import RNE, assert_out, data, offset1

pytestmark = pytest.mark.gpu

# handed to the packet batch; one masked slice; per_group 2; 3 waves (192 threads); 17 slices on 5 waves; 16 waves
MS = (256, 192, 2048, 2304, 4160, 16384)
# the odd message counts (1, 3) put a dead message at a slice's end at per_group 2 and 4, before the next slice
LENGTHS = (lambda M: 1, lambda M: M - 1, lambda M: 0, lambda M: M + 1, lambda M: 2 * M + 3,
           lambda M: 5 * M + M // 2 + 1, lambda M: 3 * M)
TYPES = ("fp32", "fp16", "bf16")


def run_batch(cuda, M, W, flags, lengths, types, inplace=()):
    """Run one call over slices of `lengths` and `types` and check every slice and its guards."""
    made = []
    for i, (n, T) in enumerate(zip(lengths, types)):
        x, x32 = data(T, n, 7 * M + 31 * i + n)
        buf, xd = offset1(x, cuda)
        obuf, out = (buf, xd) if i in inplace else offset1(x, cuda, fill=False)
        made.append((T, x32, xd, obuf, out))
    sw().msg_roundtrip_loopback_batch([(xd, out) for _, _, xd, _, out in made], M, W, flags=flags)
    for T, x32, _, obuf, _ in made:
        y32 = O.dummy_allreduce(x32, P=M, num_worker_threads=1, num_workers=W, vcl=bool(flags & RNE))
        assert_out(obuf, y32, T)


@pytest.mark.parametrize("rot,W,flags", [(0, 1, 0), (1, 3, RNE), (2, 4, 0)])
@pytest.mark.parametrize("M", MS)
def test_mixed_table(cuda, M, rot, W, flags):
    """Types cycle over the slices, rotated by the path: the type of slices 0, 3
    and 6 and that of slices 1 and 4 run the batch kernel, the third type is
    present once (slice 2 is empty) and takes the single-slice kernel."""
    run_batch(cuda, M, W, flags, [f(M) for f in LENGTHS], [TYPES[(i + rot) % 3] for i in range(7)], inplace=(4,))


@pytest.mark.parametrize("M", [2048, 4160])
def test_two_workgroups_loop_across_slices(cuda, M):
    """16 or 10 groups of six fp32 slices on two workgroups: each crosses at
    least two slice boundaries (the trip double-buffer, load-ahead into the next
    slice), with non-temporal stores."""
    old = sw().set_grid_limit(2), sw().set_payload_nt_threshold(0)
    try:
        run_batch(cuda, M, 3, 0, [f(M) for f in LENGTHS], ["fp32"] * 7, inplace=(1,))
    finally:
        sw().set_grid_limit(old[0])
        sw().set_payload_nt_threshold(old[1])


def test_full_table(cuda):
    M = 2304
    run_batch(cuda, M, 2, RNE, [(1, M + 1, 2 * M + 3, M - 1)[i % 4] for i in range(64)], ["fp16"] * 64)


def test_equals_the_packet_batch_at_1024(cuda):
    import torch
    M = 1024
    xs = [offset1(data(TYPES[i % 3], f(M), i)[0], cuda)[1] for i, f in enumerate(LENGTHS)]
    a, b = [torch.empty_like(x) for x in xs], [torch.empty_like(x) for x in xs]
    sw().roundtrip_loopback_batch(list(zip(xs, a)), M, 3)
    sw().msg_roundtrip_loopback_batch(list(zip(xs, b)), M, 3)
    for x, ya, yb in zip(xs, a, b):
        assert words_equal(ya.float().cpu().numpy(), yb.float().cpu().numpy())
