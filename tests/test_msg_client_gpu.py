"""The client at general.packet_numel = M > 1024 (an LTU that mirrors
backend.rdma.msg_numel): bulk mode, the fused threaded path and the batch
worker, bit-exact against the oracle at P = M over the T FIFO slices."""
import numpy as np
import pytest

from oracle import oracle as O
from test_half_gpu import assert_half_equal, narrow, words_equal
from test_messages_gpu import data

pytestmark = pytest.mark.gpu

MODES = {"bulk": dict(mode="bulk"), "fused-threads": dict(mode="fused", batch_jobs=0),
         # a round with a pinned host job waits coalesce_us for the next job: the jobs posted below share it
         "fused-batch": dict(mode="fused", batch_jobs=16, coalesce_us=5000)}
W = 3


@pytest.fixture
def C(cuda):
    from switchml_amd import client
    yield client
    if client.state() == client.RUNNING:
        client.stop()


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M", [2304, 16384])
def test_allreduce_at_a_long_packet_numel(C, cuda, M, mode, T):
    C.start(C.make_config(packet_numel=M, num_workers=W, num_worker_threads=T, max_outstanding_packets=64 * T,
                          bandwidth=0, **MODES[mode]))
    n = 5 * M + M // 2 + 3                                    # odd: no multiple of T = 4 or of M
    made = [data(typ, n - 2 * i, M + i) for i, typ in enumerate(("fp32", "fp32", "bf16", "fp32", "bf16"))]
    ins = [made[0][0].pin_memory()] + [x.to(cuda) for x, _ in made[1:]]
    outs = [ins[0].clone().pin_memory()] + [x.clone() for x in ins[1:-1]] + [ins[-1]]   # the last job in place
    jobs = [C.allreduce_async(x, o) for x, o in zip(ins, outs)]
    C.wait_for_all_jobs()
    assert all(j.status() == C.JOB_FINISHED for j in jobs)
    bstats = C.batch_stats()
    C.stop()
    for (x, x32), o in zip(made, outs):
        y32 = O.dummy_allreduce(x32, P=M, max_outstanding_packets=64 * T, num_worker_threads=T, num_workers=W)
        if o.element_size() == 4:
            assert words_equal(o.cpu().numpy(), y32)
        else:
            assert_half_equal(o, narrow(y32, "bf16"))
    if mode == "fused-batch":       # every slice went through a batch call, and slices of different jobs shared one
        assert bstats["batched_slices"] == T * len(jobs) and bstats["single_slices"] == 0
        assert 1 <= bstats["launches"] < len(jobs)
    else:
        assert bstats == {"launches": 0, "batched_slices": 0, "single_slices": 0}


def test_int32_job_at_a_long_packet_numel(C):
    M, T = 2304, 4
    C.start(C.make_config(packet_numel=M, num_workers=W, num_worker_threads=T, max_outstanding_packets=64 * T,
                          bandwidth=0, mode="fused"))
    xi = np.random.default_rng(M).integers(-2 ** 31, 2 ** 31, 3 * M + 5, dtype=np.int64).astype(np.int32)
    oi = np.empty_like(xi)
    C.allreduce(xi, oi)
    C.stop()
    assert np.array_equal(oi, (xi.astype(np.int64) * W).astype(np.int32))
