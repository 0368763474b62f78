"""GPU tests of the reference's random max_train subset in the batched learning loop: bcbf_subsample_rows against torch's stable
sort + indexing (exact), and self_learning_closed_loop(subsample="random") -- the final models against the oracle's refit of the
rows they hold, the subset against the stream it was drawn from and against what LearnedShiftInvariantDynamics.fit hands to the
regressor (unicycle_move_to_pose.py:377-384 of the reference), mixed precision and the hyper-parameter fit on the subset."""
import numpy as np
import pytest
import torch

from _tolreport import rel_close
from oracle import gp_posterior as ogp

pytestmark = pytest.mark.gpu
DEV = "cuda"


def host(t):
    return t.detach().cpu().double().numpy()


def _final_vs_oracle(final, tol, what):
    """Every instance's final model against the ORACLE's from-scratch refit of the rows that model holds (read back from the
    device, in subset order) with the jitter every row was factored with."""
    Mk, Bk = (host(t) for t in final["posterior"])
    hy = {k: host(v) for k, v in final["hyper"].items()}
    xq = host(final["xq_check"])
    worst = [0.0, 0.0]
    for (lo, hi), rows in zip(final["bounds"], final["rows"]):
        X, UH, Y, J = (host(rows[k]) for k in ("X", "UH", "Y", "jitter"))
        for j in range(hi - lo):
            i = lo + j
            st = ogp.refit_state(X[j], UH[j][:, 1:], Y[j], hy["Bm"][i], hy["ell"][i], hy["s2"][i], hy["M0"][i], J[j][None] / 1e-5)
            Mo, Bo = ogp.posterior_step(st["L"][None], st["alpha"][None], X[j][None], st["UHB"][None], hy["ell"][i][None], hy["s2"][i][None],
                                        hy["Bm"][i][None], hy["M0"][i][None], xq[i][None])
            prior = float(hy["s2"][i] * np.abs(hy["Bm"][i]).max())
            rel_close(Mk[i], Mo[0], tol, scale=max(1.0, np.abs(Mo).max()), what=what + " Mk")
            rel_close(Bk[i], Bo[0], tol, scale=prior, what=what + " Bk")
            worst = [max(worst[0], np.abs(Mk[i] - Mo[0]).max() / max(1.0, np.abs(Mo).max())), max(worst[1], np.abs(Bk[i] - Bo[0]).max() / prior)]
    return worst


CASES = [(1, 64, 64, 3, 2), (37, 300, 64, 2, 1), (5, 8192, 512, 3, 2), (4096, 760, 512, 3, 2)]
VARIANTS = ["plain", "offset-lo-and-ldk", "ties", "odd-N"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%d-n%d-m%d" % c for c in CASES])
def test_subsample_rows_equals_torch_stable_sort_and_indexing(case, dtype):
    """Indices and gathered rows == torch.sort(keys[:, :P], stable=True).indices[:, :N] + lo and plain indexing, bit for bit: pools
    at the stream's start and past it (lo > 0) with a key stride beyond P, keys on a 1/16 grid (most keys tie: the lower pool index
    first), N off the 32-row grid."""
    from bayesian_cbf_amd import ops
    B, P, N, n, m = case
    g = torch.Generator(device=DEV)
    g.manual_seed(B * 7 + P)
    for variant in VARIANTS:
        lo, ldk, Nv = (11, P + 13, N) if variant == "offset-lo-and-ldk" else (0, P, N)
        if variant == "odd-N":
            Nv = N - 13 if N > 13 else N - 1
        Ntot = lo + P + 5
        f = dict(dtype=dtype, device=DEV)
        X = torch.randn(B, Ntot, n, generator=g, **f)
        UH = torch.randn(B, Ntot, 1 + m, generator=g, **f)
        Y = torch.randn(B, Ntot, n, generator=g, **f)
        keys = torch.rand(B, ldk, generator=g, device=DEV)
        if variant == "ties":
            keys = (keys * 16).floor() / 16
        Xo, UHo, Yo, idx = ops.subsample_rows(keys, X, UH, Y, Nv, lo=lo, P=P)
        torch.cuda.synchronize()
        ref = torch.sort(keys[:, :P], dim=1, stable=True).indices[:, :Nv] + lo
        assert idx.dtype == torch.int32 and idx.shape == (B, Nv)
        assert torch.equal(idx.long(), ref), (variant, (idx.long() != ref).sum().item())
        take = lambda t_: torch.gather(t_, 1, ref[:, :, None].expand(B, Nv, t_.shape[2]))
        assert torch.equal(Xo, take(X)) and torch.equal(UHo, take(UH)) and torch.equal(Yo, take(Y)), variant
        # the same call into the caller's buffers
        out = (torch.full_like(Xo, 7), torch.full_like(UHo, 7), torch.full_like(Yo, 7), torch.full_like(idx, -1))
        ops.subsample_rows(keys, X, UH, Y, Nv, lo=lo, P=P, out=out)
        assert torch.equal(out[3], idx) and torch.equal(out[0], Xo) and torch.equal(out[1], UHo) and torch.equal(out[2], Yo)


def _record_subsample_calls(monkeypatch):
    """Wrap ops.subsample_rows: every call the loop makes is recorded (stream base pointer, lo, P, indices) and its indices are
    checked against the stable sort of the keys the loop drew."""
    from bayesian_cbf_amd import ops
    calls = []
    inner = ops.subsample_rows

    def rec(keys, X, UH, Y, N, lo=0, P=None, out=None):
        res = inner(keys, X, UH, Y, N, lo=lo, P=P, out=out)
        ref = torch.sort(keys[:, :P], dim=1, stable=True).indices[:, :N] + lo
        assert torch.equal(res[3].long(), ref)
        calls.append((X.data_ptr(), lo, P, res[3].clone()))
        return res
    monkeypatch.setattr(ops, "subsample_rows", rec)
    return calls


def test_random_subset_loop_fp64_vs_oracle_refit_of_the_subset(monkeypatch):
    """fp64, three staggered parts, max_train 64, default warmup (80 steps: every timed refit has more than max_train own rows):
    the subset of every instance is max_train DISTINCT rows of its own observations, the rows the model holds are those stream rows
    bit for bit, instances and consecutive refits draw different subsets, and every final model == the oracle's refit of its rows
    (1e-7)."""
    from bayesian_cbf_amd.rollouts import self_learning_closed_loop, final_model_vs_fp64_refit
    calls = _record_subsample_calls(monkeypatch)
    rep, final = self_learning_closed_loop(Bt=24, max_train=64, refit_every=16, steps=48, parts=3, dtype=torch.float64, subsample="random",
                                           seed=5, device=DEV)
    W = final["stream_rows"]["window"]
    assert rep["subsample"] == "random" and W == 64 and rep["warmup"] >= 64
    assert rep["refit_failures_after_retries"] == 0 and rep["solver_optimal_fraction"] >= 0.9
    assert all(p_ > 64 for p_ in rep["pool_rows_at_last_refit"])
    sidx = final["subset_index"]
    assert sidx.shape == (24, 64) and sidx.dtype == torch.int32
    sr = final["stream_rows"]
    for c, ((lo, hi), rows) in enumerate(zip(final["bounds"], final["rows"])):
        pool = rep["pool_rows_at_last_refit"][c]
        s = sidx[lo:hi].long()
        assert int(s.min()) >= W and int(s.max()) < W + pool
        assert all(torch.unique(s[j]).numel() == 64 for j in range(hi - lo))
        g = lambda t_: torch.gather(t_[lo:hi], 1, s[:, :, None].expand(hi - lo, 64, t_.shape[2]))
        assert torch.equal(rows["X"], g(sr["X"])) and torch.equal(rows["UH"], g(sr["UH"])) and torch.equal(rows["Y"], g(sr["Y"]))
        assert bool((rows["jitter"] > 0).all())
    assert not torch.equal(torch.sort(sidx[0]).values, torch.sort(sidx[1]).values)
    # consecutive refits of one part draw different subsets (every part refits at least twice with more than max_train own rows)
    by_part = {}
    for ptr, lo_, P_, idx in calls:
        assert lo_ == W and P_ > 64
        by_part.setdefault(ptr, []).append(idx)
    assert len(by_part) == 3
    for seq in by_part.values():
        assert len(seq) >= 2
        for a_, b_ in zip(seq, seq[1:]):
            assert not torch.equal(torch.sort(a_, dim=1).values, torch.sort(b_, dim=1).values)
    worst = _final_vs_oracle(final, 1e-7, "random-subset loop fp64")
    chk = final_model_vs_fp64_refit(final)
    assert chk["Mk"] <= 1e-8 and chk["Bk"] <= 1e-8 and chk["refit_failures"] == 0, chk
    print("random-subset loop fp64: worst |dMk| %.2e |dBk| %.2e vs oracle; %d subset draws" % (worst[0], worst[1], len(calls)))


def test_random_subset_is_the_facades_training_set():
    """The façade (LearnedShiftInvariantDynamics.train / fit) run on the recorded trajectory of instance 0 (part 0) and 5 (part 1),
    its random draw replaced by the loop's chosen indices and its schedule set to the part's last refit: the (X, U, Y) it hands to
    the regressor == the rows of the loop's final subset -- inputs and controls bit for bit, targets within the 2-ulp rule of
    tests/test_gpu_learning.py (the kernel divides by dt, torch on the GPU multiplies by its reciprocal)."""
    from bayesian_cbf_amd.rollouts import self_learning_closed_loop
    from bayesian_cbf_amd.unicycle_move_to_pose import LearnedShiftInvariantDynamics, AckermannDrive
    dt, max_train = 0.01, 64
    rep, final = self_learning_closed_loop(Bt=8, max_train=max_train, steps=48, refit_every=16, parts=2, dtype=torch.float64, device=DEV,
                                           seed=3, dt=dt, record_states=True, subsample="random")
    xs = torch.cat([final["states"]["x"], final["x"][:, None]], 1)          # x_0 .. x_T (the state after the last step too)
    us = final["states"]["u"]
    W = final["stream_rows"]["window"]

    class Recorder:
        def __init__(self):
            self.calls = []

        def fit(self, X, U, Y, training_iter=0):
            self.calls.append((X.clone(), U.clone(), Y.clone()))
    for inst in (0, 5):
        c = next(k for k, (lo, hi) in enumerate(final["bounds"]) if lo <= inst < hi)
        rows, lo = final["rows"][c], final["bounds"][c][0]
        count = rep["pool_rows_at_last_refit"][c]                            # own rows at the part's last refit
        assert count > max_train
        chosen = final["subset_index"][inst].long() - W
        rec = Recorder()
        dyn = LearnedShiftInvariantDynamics(dt=dt, learned_dynamics=rec, mean_dynamics=AckermannDrive(L=4.0), max_train=max_train,
                                            training_iter=0, train_every_n_steps=count + 1, device=DEV, dtype=torch.float64)
        asked = []

        def draw(n_, k_, chosen=chosen, asked=asked):
            asked.append((n_, k_))
            return chosen
        dyn._learner.subsample = draw
        for t in range(count + 2):                                           # the refit happens with count + 1 states buffered
            dyn.train(xs[inst, min(t, xs.shape[1] - 1)], us[inst, min(t, us.shape[1] - 1)])   # (the last call's own data are not used)
        assert asked == [(count, max_train)] and len(rec.calls) == 1
        Xf, Uf, Yf = rec.calls[0]
        j = inst - lo
        assert torch.equal(rows["X"][j], Xf)
        assert torch.equal(rows["UH"][j][:, 1:], Uf) and bool((rows["UH"][j][:, 0] == 1).all())
        fd = (xs[inst, chosen + 1] - xs[inst, chosen]).abs() / dt
        Yd = rows["Y"][j]
        assert bool(((Yd - Yf).abs() <= 2.3e-16 * fd.clamp(min=1e-300) * 2).all()), float((Yd - Yf).abs().max())


def test_random_subset_mixed_precision_meets_1e_3():
    """fp64 factors + fp32 passes (jitter floor 1e-3) on the random subsets: every final model == the oracle's fp64 refit of the
    subset it holds to 1e-3, as for the window."""
    from bayesian_cbf_amd.rollouts import self_learning_closed_loop, final_model_vs_fp64_refit
    rep, final = self_learning_closed_loop(Bt=24, max_train=64, refit_every=16, steps=48, parts=3, dtype=torch.float32, subsample="random",
                                           seed=5, device=DEV, factor_dtype=torch.float64, min_jitter_level=1e-3)
    assert rep["refit_failures_after_retries"] == 0 and rep["factor_dtype"] == "torch.float64"
    assert all(p_ > 64 for p_ in rep["pool_rows_at_last_refit"])
    assert final["posterior"][0].dtype == torch.float32 and final["subset_index"].shape == (24, 64)
    worst = _final_vs_oracle(final, 1e-3, "random-subset loop, fp64 factors + fp32 passes")
    chk = final_model_vs_fp64_refit(final)
    assert chk["Mk"] <= 1e-3 and chk["Bk"] <= 1e-3 and chk["refit_failures"] == 0, chk
    print("random-subset mixed precision: worst |dMk| %.2e |dBk| %.2e vs oracle" % (worst[0], worst[1]))


def test_random_subset_with_hyper_parameter_fit_fp64():
    """fit_iters=3 on the random subsets: it runs, the hyper-parameters move, and every final model == the oracle's refit of its
    subset at the final hyper-parameters (1e-7)."""
    from bayesian_cbf_amd.rollouts import self_learning_closed_loop
    from bayesian_cbf_amd.synthetic import make_instances
    rep, final = self_learning_closed_loop(Bt=12, max_train=64, refit_every=16, steps=32, parts=2, dtype=torch.float64, subsample="random",
                                           seed=5, device=DEV, fit_iters=3)
    assert rep["refit_failures_after_retries"] == 0 and rep["fit_iters"] == 3
    assert all(p_ > 64 for p_ in rep["pool_rows_at_last_refit"])
    p0 = make_instances(12, 64, 3, 2, dtype=torch.float64, device=DEV, seed=5, variant="theta")
    for k in ("ell", "s2", "Bm"):
        assert not torch.equal(final["hyper"][k], p0[k]), k
    worst = _final_vs_oracle(final, 1e-7, "random-subset loop + fit fp64")
    print("random-subset loop + 3 Adam iterations per refit: worst |dMk| %.2e |dBk| %.2e vs oracle" % tuple(worst))
