"""GPU tests of the self-triggering interval (bcbf_trigger_interval, ops.trigger_interval, bayesian_cbf_amd/trigger_interval.py):
the 200 steps of the reference's committed learning run as one batch against the results the reference recorded for it; generic
(non-grid) test points against the numpy yardstick tests/_trigger_reference.py; the reference's call surface on an event file; graph
capture; a log written by this project's own loop; the refusal of other data kernels."""
import math
import os

import numpy as np
import pytest
import torch

import _trigger_reference as R
from _tolreport import all_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = [torch.float64, torch.float32]


def host(t):
    return t.detach().cpu().double().numpy()


@pytest.fixture(scope="module")
def saved():
    return np.load(os.path.join(GOLDEN, "saved_run_learning_v1p6p3.npz")), np.load(os.path.join(GOLDEN, "trigger_interval_v1p6p3.npz"))


# ------------------------------------------------------------------------------------------------ 1. the recorded reference
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_recorded_reference_results_as_one_batch_of_200(saved, dtype):
    """Lfh, tau, xvel of the committed run's 200 steps (per-instance hyper-parameters, the default grid of 729 points and the
    default obstacles) against the reference's Lfh.np.txt / tau.np.txt / xvel.np.txt: fp64 1e-6 (the float32 log bounds it: the
    fp64 numpy restatement reaches 1.7e-7 at worst), fp32 1e-5 (the same arithmetic in fp32 on the CPU: 2.7e-7; the rest is room
    for the hardware exponential)."""
    from bayesian_cbf_amd import trigger_interval as ti
    G, F = saved
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)
    out = ti.trigger_interval_batch(t(G["state"]), t(G["xtp1"]), t(G["uopt"]), t(G["knl_lengthscale"]), t(G["knl_scalefactor"]),
                                    t(G["knl_A"]), t(G["knl_B"]), ti._DEFAULT_CBFS(), 0.01)
    tol = 1e-6 if dtype == torch.float64 else 1e-5
    assert out["Lfh"].shape == (200,) and out["Lkd"].shape == (200, 3) and out["Lfh"].dtype == dtype and out["tau"].is_cuda
    for k in ("Lfh", "tau", "xvel"):
        got = host(out[k])
        print("%s %s: worst relative error %.3e (bound %.0e)" % (k, dtype, np.max(np.abs(got - F[k]) / np.abs(F[k])), tol))
    for k in ("Lfh", "tau", "xvel"):
        all_close(host(out[k]), F[k], rtol=tol, atol=1e-300, what="trigger interval vs recorded " + k)


# ------------------------------------------------------------------------------------------------ 2. generic points
CASES = [(1, 1, 1, 1), (3, 2, 2, 1), (5, 63, 3, 2), (4, 64, 3, 2), (7, 65, 2, 1), (2, 257, 3, 2), (3, 729, 3, 2), (2, 1100, 3, 2)]
REGIMES = ["interior", "far", "underflow"]
EXTENT = 0.1


def _inputs(case, regime, shared, seed):
    """fp64 numpy inputs of one case.  Offsets are random (no grid); lengthscales per regime: of the order of the points' extent
    (the maximising pair is in the interior), 100 x the extent (it is the farthest pair: a dropped tile or tail shows), 1e-3 of the
    smallest spacing (every off-diagonal kernel value underflows: Lkd == 0 exactly)."""
    B, Nte, n, m = case
    rng = np.random.default_rng(seed)
    off = rng.normal(size=(Nte, n)) * EXTENT
    Bh = 1 if shared else B
    if regime == "underflow":
        d = np.linalg.norm(off[:, None, :] - off[None, :, :], axis=-1)
        base = 1e-3 * (d[np.triu_indices(Nte, 1)].min() if Nte > 1 else EXTENT)
    else:
        base = EXTENT * (100.0 if regime == "far" else 1.0)
    C = 1 + m
    Bm = rng.normal(size=(Bh, C, C))
    inp = dict(x=rng.normal(size=(B, n)) * 2, u=rng.normal(size=(B, m)), ls=base * rng.uniform(0.5, 1.5, size=(Bh, n)),
               sf=rng.uniform(0.5, 1.5, size=Bh), A=np.stack([np.diag(rng.uniform(0.5, 2.0, size=n)) for _ in range(Bh)]),
               B=Bm @ Bm.transpose(0, 2, 1) + 0.1 * np.eye(C), Lh=rng.uniform(0.5, 3.0, size=B), off=off)
    inp["xtp1"] = inp["x"] + rng.normal(size=(B, n)) * 0.02
    return inp


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shared", [False, True], ids=["per-instance", "shared-model"])
@pytest.mark.parametrize("case", CASES, ids=["B%d-Nte%d-n%d-m%d" % c for c in CASES])
def test_generic_points_against_the_numpy_yardstick(case, shared, dtype):
    """Lkd, Lfh and tau against tests/_trigger_reference.py: fp64 within 1e-12 relative; fp32 within 1e-5 against the yardstick
    evaluated on the fp32-ROUNDED inputs and test points (off + x formed in fp32, as the kernel forms it), so the cancellation
    in the inputs is not charged to the kernel.  Nte = 1: Lkd == 0."""
    from bayesian_cbf_amd import trigger_interval as ti
    B, Nte, n, m = case
    dt, tol = 0.01, (1e-12 if dtype == torch.float64 else 1e-5)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    for ri, regime in enumerate(REGIMES):
        inp = {k: v.astype(npdt) for k, v in _inputs(case, regime, shared, seed=1000 * B + Nte + ri).items()}     # what the device sees
        t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV)
        r = R.whole_norm(inp["off"].astype(np.float64))
        hy = (lambda a: t(a[0])) if shared else t
        out = ti.trigger_interval_batch(t(inp["x"]), t(inp["xtp1"]), t(inp["u"]), hy(inp["ls"]), hy(inp["sf"]), hy(inp["A"]), hy(inp["B"]),
                                        None, dt, off=t(inp["off"]), r=r, Lh=t(inp["Lh"]))
        got = {k: host(v) for k, v in out.items()}
        f64 = {k: v.astype(np.float64) for k, v in inp.items()}
        want = dict(Lkd=np.zeros((B, n)), Lfh=np.zeros(B), tau=np.zeros(B))
        for b in range(B):
            hb = 0 if shared else b
            uh = np.r_[1.0, f64["u"][b]]
            Xtest = (inp["off"] + inp["x"][b]).astype(np.float64)                  # rounded in the working type, then exact
            res = R.step(None, None, f64["ls"][hb], f64["sf"][hb], np.diag(f64["A"][hb]), uh @ f64["B"][hb] @ uh, r, f64["Lh"][b],
                         np.linalg.norm(f64["xtp1"][b] - f64["x"][b]) / dt, Xtest=Xtest)
            for k in want:
                want[k][b] = res[k]
        for k in ("Lkd", "Lfh", "tau"):
            assert np.isfinite(got[k]).all(), (regime, k)
            nz = want[k] != 0
            worst = np.max(np.abs(got[k][nz] - want[k][nz]) / np.abs(want[k][nz])) if nz.any() else 0.0
            print("%s %s %s %s: worst relative error %.3e (bound %.0e)" % (case, regime, dtype, k, worst, tol))
        for k in ("Lkd", "Lfh", "tau"):
            all_close(got[k], want[k], rtol=tol, atol=1e-300, what="trigger interval %s %s" % (regime, k))
        if regime == "underflow" or Nte == 1:
            assert (got["Lkd"] == 0).all() and (want["Lkd"] == 0).all()
        else:
            assert (got["Lkd"] > 0).all()


# ------------------------------------------------------------------------------------------------ 3. the reference's call surface
NAMES = ("xvel.np.txt", "Lfh.np.txt", "Lfh_num.np.txt", "tau.np.txt", "tau_num.np.txt")


def _write_saved_run_as_event_file(G, run_dir):
    from bayesian_cbf_amd import tblog
    log = tblog.TBLogger(["trigger_interval", "saved_run"], runs_dir=str(run_dir))
    for s in range(len(G["state"])):
        log.add_tensors("vis", dict(state=G["state"][s], uopt=G["uopt"][s], xtp1=G["xtp1"][s], knl_lengthscale=G["knl_lengthscale"][s],
                                    knl_scalefactor=G["knl_scalefactor"][s], knl_A=G["knl_A"][s], knl_B=G["knl_B"][s]), s)
    log.summary_writer.close()
    return log.summary_writer.path


def test_reference_call_surface_on_an_event_file(saved, tmp_path):
    """unicycle_trigger_interval_compute(events_file, out_data_files) with the reference's defaults on the committed run written
    back as an event file: five text files of 200 rows; Lfh, tau, xvel agree with the recorded ones at 1e-6; the sampled
    Lfh_num, tau_num (unseeded draws upstream: not reproducible, not pinned) are finite and positive."""
    from bayesian_cbf_amd import trigger_interval as ti
    G, F = saved
    events_file = _write_saved_run_as_event_file(G, tmp_path)
    files = {name: str(tmp_path / name) for name in NAMES}
    ret = ti.unicycle_trigger_interval_compute(events_file, files)
    for name in NAMES:
        arr = np.loadtxt(files[name])
        assert arr.shape == (200,), name
        np.testing.assert_array_equal(arr, ret[name])
        if name.split(".")[0] in ("Lfh", "tau", "xvel"):
            all_close(arr, F[name.split(".")[0]], rtol=1e-6, atol=1e-300, what="call surface " + name)
        else:
            assert np.isfinite(arr).all() and (arr > 0).all(), name


# ------------------------------------------------------------------------------------------------ 4. capture
def test_capture_in_a_graph_and_replay_on_overwritten_inputs():
    from bayesian_cbf_amd import ops
    dtype, (B, Nte, n, m) = torch.float32, (6, 200, 3, 2)

    def device_inputs(seed):
        inp = _inputs((B, Nte, n, m), "interior", False, seed)
        t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV).contiguous()
        return [t(inp["x"]), t(inp["off"]), t(inp["ls"]), t(inp["sf"]), t(np.stack([np.diag(a) for a in inp["A"]])),
                t(np.abs(inp["u"][:, 0]) + 0.5), t(np.abs(inp["u"][:, 1]) + 0.3), t(inp["Lh"])]

    a, b = device_inputs(1), device_inputs(2)
    eager_a = [v.clone() for v in ops.trigger_interval(*a, 3.0)]
    again = ops.trigger_interval(*a, 3.0)
    assert all(torch.equal(p, q) for p, q in zip(eager_a, again))                 # the same inputs: the same bits
    eager_b = [v.clone() for v in ops.trigger_interval(*b, 3.0)]
    assert not torch.equal(eager_a[0], eager_b[0])
    out = tuple(torch.empty_like(v) for v in eager_a)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.trigger_interval(*a, 3.0, out=out)                                     # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.trigger_interval(*a, 3.0, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(out, eager_a))
    for dst, src in zip(a, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(out, eager_b))


# ------------------------------------------------------------------------------------------------ 5. a log of this project's loop
def _run_own_loop(run_dir, **kw):
    from bayesian_cbf_amd import tblog
    from bayesian_cbf_amd import unicycle_move_to_pose as ump
    x0, xg = torch.tensor([-3.0, -1.0, -math.pi / 4], dtype=torch.float64), torch.tensor([0.0, 0.0, math.pi / 4], dtype=torch.float64)
    log = tblog.TBLogger(["unicycle_move_to_pose_fixed", "own_loop"], runs_dir=str(run_dir))
    ump.track_trajectory_ackerman_clf_bayesian(
        x0, xg, dt=0.01, numSteps=5, train_every_n_steps=1000, cbf_gammas=[5.0, 5.0], max_risk=0.01, logger=log, device=DEV,
        cbfs=lambda a, b: ump.obstacles_at_mid_from_start_and_goal(a, b, term_weights=(0.7, 0.3)),
        mean_dynamics_gen=lambda: ump.AckermannDrive(L=12.0), true_dynamics_gen=lambda: ump.AckermannDrive(L=1.0), **kw)
    log.summary_writer.close()
    return log.summary_writer.path


def test_a_log_of_our_own_loop_feeds_the_computation(tmp_path):
    from bayesian_cbf_amd import tblog
    from bayesian_cbf_amd import trigger_interval as ti
    events_file = _run_own_loop(tmp_path / "with", log_model=True)
    tags = set(tblog.load_tensorboard_scalars(events_file))
    assert {"vis/state", "vis/uopt", "vis/xtp1", "vis/knl_lengthscale", "vis/knl_scalefactor", "vis/knl_A", "vis/knl_B"} <= tags
    files = {name: str(tmp_path / name) for name in NAMES}
    ret = ti.unicycle_trigger_interval_compute(events_file, files)
    tau = np.loadtxt(files["tau.np.txt"])
    assert tau.shape == (5,) and np.isfinite(tau).all() and (tau > 0).all(), tau
    assert np.isfinite(ret["Lfh.np.txt"]).all() and (ret["Lfh.np.txt"] > 0).all() and (ret["xvel.np.txt"] > 0).all()
    plain = set(tblog.load_tensorboard_scalars(_run_own_loop(tmp_path / "without")))
    assert "vis/state" in plain and not any("knl_" in tag or "xtp1" in tag for tag in plain), plain


# ------------------------------------------------------------------------------------------------ 6. refusal
def test_other_data_kernels_are_refused():
    from bayesian_cbf_amd import trigger_interval as ti
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    for kind in (1, 2, "matern52"):
        with pytest.raises(ValueError, match="RBF data kernel"):
            ti.trigger_interval_batch(z(2, 3), z(2, 3), z(2, 2), z(3) + 1, z(()) + 1, z(3, 3), z(3, 3), None, 0.01, Lh=z(2) + 1,
                                      kernel_kind=kind)
