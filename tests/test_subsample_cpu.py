"""CPU-side checks of the random max_train subset (bcbf_subsample_rows, ops.subsample_rows, the learning loop's
subsample="random"): argument checks refuse before any launch, no CPU path, the pool rule, the loop's checks run before it
touches a device."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


# (lo, P, Ntot, ldk, n, m, N) -> the reason bcbf_last_error names; every case fails its host check, so the fake pointers are never used
GOOD = dict(lo=0, P=64, Ntot=100, ldk=64, n=3, m=2, N=32)
BAD = [(dict(N=65), "N <= P"), (dict(P=8193, Ntot=9000, ldk=8193, N=64), "P > 8192"), (dict(lo=40), "lo + P <= Ntot"),
       (dict(ldk=63), "ldk < P"), (dict(n=0), "1 <= n <= 8"), (dict(N=0), "N <= P"), (dict(m=9), "0 <= m <= 8")]


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("change,why", BAD, ids=[w for _, w in BAD])
def test_bad_arguments_return_negative_with_a_reason_and_no_launch(lib, suf, change, why):
    a = dict(GOOD, **change)
    fake = [ctypes.c_void_p(4096 * (k + 1)) for k in range(8)]
    fn = getattr(lib.lib, "bcbf_subsample_rows" + suf)
    rc = fn(fake[0], a["ldk"], a["lo"], a["P"], fake[1], fake[2], fake[3], a["Ntot"], a["n"], a["m"], a["N"], fake[4], fake[5], fake[6],
            fake[7], 5, None)
    assert rc < 0
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_subsample_rows") and why in msg, msg


def test_ops_subsample_rows_refuses_cpu_tensors(lib):
    from bayesian_cbf_amd import ops
    X, UH, Y = torch.zeros(2, 10, 3), torch.zeros(2, 10, 3), torch.zeros(2, 10, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.subsample_rows(torch.rand(2, 10), X, UH, Y, 4)


def test_subsample_pool_window_rule_then_the_whole_own_stream():
    from bayesian_cbf_amd.rollouts import subsample_pool
    W = 64
    for own in (1, 17, 63, 64):
        assert subsample_pool(W, own, W) == (own, W, False)          # the last W stream rows [own, own + W): synthetic start included
    for own in (65, 100, 8192):
        assert subsample_pool(W, own, W) == (W, own, True)           # every own row [W, W + own) is in the pool


def test_loop_refuses_random_subset_with_the_tail_schedule_before_touching_a_device():
    from bayesian_cbf_amd.rollouts import self_learning_closed_loop
    # device="cpu": a loop that got as far as allocating would fail differently (no CPU path / no streams)
    with pytest.raises(ValueError, match="schedule='reference'"):
        self_learning_closed_loop(Bt=4, max_train=64, steps=16, refit_every=16, schedule="online_tail", subsample="random", device="cpu")
    with pytest.raises(ValueError, match="subsample"):
        self_learning_closed_loop(Bt=4, max_train=64, steps=16, refit_every=16, subsample="shuffle", device="cpu")
    with pytest.raises(ValueError, match="8192"):
        self_learning_closed_loop(Bt=4, max_train=64, steps=8192, refit_every=16, subsample="random", device="cpu")
