"""GPU tests of the control step on a plant drawn from the model's own posterior (bcbf_unicycle_control_step_sampled,
bcbf_rollout_risk, ops.unicycle_control_step_prepare(sampled=...), rollouts.monte_carlo_safety_rollouts(plant="posterior")):
the solve is untouched, the draw against the numpy yardstick tests/_posterior_plant_reference.py, the semidefinite and the
unsolved paths, the risk bookkeeping of a rollout, and -- the point of the feature -- the calibration of the empirical risk against
the max_risk the program was built for."""
import math

import numpy as np
import pytest
import torch

import _posterior_plant_reference as R
from _tolreport import _record

pytestmark = pytest.mark.gpu
DEV = "cuda"
BT, KOB, DT, NTRAIN = 37, 2, 0.05, 40          # 37 instances: two full quad-waves (16 instances each) and a ragged one
L_MEAN = 4.0
NP = {torch.float64: np.float64, torch.float32: np.float32}
BADCONE = 3


def raw(t):
    return t.detach().cpu().numpy()


def bits(t):
    return raw(t.contiguous()).tobytes()


@pytest.fixture(scope="module")
def ops():
    from bayesian_cbf_amd import ops as _ops
    return _ops


_CASES = {}


def case(ops, dtype, model):
    """Inputs of one (precision, model) pair, built once: the task of synthetic.make_unicycle_task, and either the fixed-kernel
    model (Lop = NULL: M_k = 0, B_k = I are inputs) or one learned GP of NTRAIN points per instance."""
    key = (dtype, model)
    if key in _CASES:
        return _CASES[key]
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    task = make_unicycle_task(BT, dtype=dtype, device=DEV, seed=71)
    f = dict(dtype=dtype, device=DEV)
    if model == "fixed":
        gp = dict(A=(1e-2 * torch.eye(3, **f)).expand(BT, 3, 3).contiguous())
    else:
        p = make_instances(BT, NTRAIN, 3, 2, dtype=dtype, device=DEV, seed=72)
        jit = p["jitter"]
        for _ in range(4):                                   # make_psd's x10 retry, as the benchmark refits
            Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit)
            if not bool((info != 0).any()):
                break
            jit = torch.where((info != 0)[:, None], jit * 10, jit).contiguous()
        assert int((info != 0).sum()) == 0
        Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
        gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=(0.01 * p["A"]).contiguous())
    z = torch.randn(BT, 3, generator=torch.Generator(device=DEV).manual_seed(73), **f)
    _CASES[key] = dict(task=task, gp=gp, z=z, dtype=dtype, model=model)
    return _CASES[key]


def workspace(ops, c, Bt=BT):
    ws = ops.control_workspace(Bt, KOB, c["dtype"], DEV)
    if c["model"] == "fixed":
        ws["Mk"].zero_()
        ws["Bk"].copy_(torch.eye(3, dtype=c["dtype"], device=DEV).expand(Bt, 3, 3))
    return ws


def run_sampled(ops, c, z=None, A=None, dt=DT, fill=7.0, obs=None):
    """One sampled step from the case's start states.  xdot_s / cbc_s start from `fill`, so a row the kernel does not write shows."""
    f = dict(dtype=c["dtype"], device=DEV)
    gp = dict(c["gp"], A=A) if A is not None else c["gp"]
    x = c["task"]["x"].clone()
    ws = workspace(ops, c)
    out = dict(z=(c["z"] if z is None else z).clone(), xdot_s=torch.full((BT, 3), fill, **f), cbc_s=torch.full((BT, 1 + KOB), fill, **f))
    step = ops.unicycle_control_step_prepare(gp, c["task"], ws, x, dt=dt, L_true=12.0, L_mean=L_MEAN, clf_gamma=10.0, max_iters=40,
                                             sampled=out)
    step(obs=obs)
    torch.cuda.synchronize()
    return dict(x0=c["task"]["x"], x=x, ws=ws, A=gp["A"], **out)


def reference_of(c, run, z=None):
    ws, t = run["ws"], c["task"]
    return R.step(raw(run["x0"]), raw(ws["y"]), raw(ws["status"]), raw(ws["Mk"]), raw(ws["Bk"]), raw(run["A"]), raw(ws["grad"]),
                  raw(ws["cst"]), raw(ws["fhat"]), raw(ws["ghat"]), raw(t["sign"]), raw(run["z"] if z is None else z), DT,
                  dtype=NP[c["dtype"]])


def close(actual, desired, scale, dtype, what):
    """|actual - desired| <= 1e-12 scale (fp64: a few dozen flops plus sqrt / sin / cos) or 2 ulp at scale (fp32: the reference is
    the same fp64 evaluation of the same fp32 inputs, rounded once).  The worst ratio goes to the tolerance report."""
    err = np.abs(actual.astype(np.float64) - desired.astype(np.float64))
    if dtype == torch.float64:
        tol, name = 1e-12 * scale, "1e-12 scale"
    else:
        tol, name = 2.0 * np.spacing(scale.astype(np.float32)).astype(np.float64), "2 ulp(scale)"
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    _record(what, ratio, 1.0)
    print("%s: worst error / bound (%s) = %.3e" % (what, name, ratio))
    assert (err <= tol).all(), "%s: worst error / bound (%s) = %.3e" % (what, name, ratio)


PAIRS = [(torch.float64, "fixed"), (torch.float64, "learned"), (torch.float32, "fixed"), (torch.float32, "learned")]
PAIR_IDS = ["f64-fixed", "f64-learned", "f32-fixed", "f32-learned"]


# ------------------------------------------------------------------------------------------------ 1. the solve is untouched
@pytest.mark.parametrize("dtype,model", PAIRS, ids=PAIR_IDS)
def test_solve_is_bit_identical_to_the_existing_step(ops, dtype, model):
    c = case(ops, dtype, model)
    x1, ws1 = c["task"]["x"].clone(), workspace(ops, c)
    ops.unicycle_control_step(c["gp"], c["task"], ws1, x1, dt=0.0, L_mean=L_MEAN, clf_gamma=10.0, max_iters=40)
    torch.cuda.synchronize()
    run = run_sampled(ops, c)
    for k in ("y", "status", "iters", "Mk", "Bk", "cones", "grad", "cst"):
        assert bits(ws1[k]) == bits(run["ws"][k]), k
    assert int((run["ws"]["status"] == 0).sum()) >= 0.8 * BT
    assert bits(x1) == bits(c["task"]["x"]) and bits(run["x"]) != bits(c["task"]["x"])


# ------------------------------------------------------------------------------------------------ 2. parity of the draw
@pytest.mark.parametrize("dtype,model", PAIRS, ids=PAIR_IDS)
def test_draw_matches_the_fp64_restatement(ops, dtype, model):
    """x, xdot_s, cbc_s against tests/_posterior_plant_reference.py fed the step's own stored intermediates (outputs of kernels the
    existing parity tests hold to the oracle)."""
    c = case(ops, dtype, model)
    run = run_sampled(ops, c)
    ref = reference_of(c, run)
    tag = "posterior plant %s " % (PAIR_IDS[PAIRS.index((dtype, model))],)
    close(raw(run["xdot_s"]), ref["xdot_s"], ref["scale_xdot"], dtype, tag + "xdot_s")
    close(raw(run["x"]), ref["x_next"], ref["scale_x"], dtype, tag + "x")
    close(raw(run["cbc_s"]), ref["cbc_s"], ref["scale_cbc"], dtype, tag + "cbc_s")
    solved = raw(run["ws"]["status"]) == 0
    assert np.abs(raw(run["xdot_s"])[solved]).min() > 0            # (the fill value is gone, the draw is not degenerate)


def test_observation_rows_record_the_sampled_plant(ops):
    """`observe` composes: the row written with the step is the finite difference of the SAMPLED states minus the prior mean."""
    c = case(ops, torch.float64, "learned")
    f = dict(dtype=torch.float64, device=DEV)
    obs = (torch.zeros(BT, 3, **f), torch.zeros(BT, 3, **f), torch.zeros(BT, 3, **f), 1)
    run = run_sampled(ops, c, obs=obs)
    ws = run["ws"]
    solved = (ws["status"] == 0)[:, None]
    u = torch.where(solved, ws["y"][:, :2], torch.zeros_like(ws["y"][:, :2]))
    want = torch.where(solved, run["xdot_s"] - (ws["ghat"] @ u[:, :, None])[:, :, 0], torch.zeros_like(run["xdot_s"]))
    np.testing.assert_allclose(raw(obs[2]), raw(want), rtol=0, atol=1e-10)
    np.testing.assert_array_equal(raw(obs[1]), raw(torch.cat([torch.ones(BT, 1, **f), u], 1)))
    np.testing.assert_array_equal(raw(obs[0])[:, 2], raw(run["x0"])[:, 2])


# ------------------------------------------------------------------------------------------------ 3. z = 0 and semidefinite A
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_zero_draw_and_semidefinite_kernel_matrix(ops, dtype):
    """z = 0: the step is x + (fhat + ghat u + M_k ubar) dt as the reference computes it.  A = 0: the same result for any z and
    no NaN -- with A = 0 no cone can be factored (a_h = grad' A grad = 0: the oracle's bad_cone branch), so that result is every
    instance keeping its state.  A positive-semidefinite A with a zero pivot (first or last) IS solved: the zeroed column of its
    factor keeps the draw in the range of A, against the reference, finite everywhere."""
    c = case(ops, dtype, "fixed")
    f = dict(dtype=dtype, device=DEV)
    run0 = run_sampled(ops, c, z=torch.zeros(BT, 3, **f))
    ref0 = reference_of(c, run0)
    close(raw(run0["x"]), ref0["x_next"], ref0["scale_x"], dtype, "posterior plant z=0 x")
    close(raw(run0["xdot_s"]), ref0["xdot_s"], ref0["scale_xdot"], dtype, "posterior plant z=0 xdot_s")
    ws0 = run0["ws"]
    solved = (ws0["status"] == 0)[:, None]
    mean = (ws0["ghat"].double() @ ws0["y"][:, :2, None].double())[:, :, 0]                   # fixed-kernel model: M_k = 0, fhat = 0
    want = torch.where(solved, c["task"]["x"].double() + mean * DT, c["task"]["x"].double())
    np.testing.assert_allclose(raw(run0["x"]), raw(want), rtol=0, atol=1e-12 if dtype == torch.float64 else 1e-6)

    Azero = torch.zeros(BT, 3, 3, **f)
    a = run_sampled(ops, c, A=Azero)
    b = run_sampled(ops, c, A=Azero, z=-3.0 * c["z"])
    for k in ("x", "xdot_s", "cbc_s"):
        assert bits(a[k]) == bits(b[k]), k
        assert bool(torch.isfinite(a[k]).all()), k
    assert bits(a["x"]) == bits(c["task"]["x"]) and bool((a["ws"]["status"] == BADCONE).all())

    for diag in ((1e-2, 1e-2, 0.0), (0.0, 1e-2, 1e-2)):
        Apsd = torch.diag(torch.tensor(diag, **f)).expand(BT, 3, 3).contiguous()
        run = run_sampled(ops, c, A=Apsd)
        ref = reference_of(c, run)
        assert int((run["ws"]["status"] == 0).sum()) >= 0.8 * BT
        for k in ("x", "xdot_s", "cbc_s"):
            assert bool(torch.isfinite(run[k]).all()), k
        close(raw(run["xdot_s"]), ref["xdot_s"], ref["scale_xdot"], dtype, "posterior plant psd %s xdot_s" % (diag,))
        close(raw(run["x"]), ref["x_next"], ref["scale_x"], dtype, "posterior plant psd %s x" % (diag,))
        close(raw(run["cbc_s"]), ref["cbc_s"], ref["scale_cbc"], dtype, "posterior plant psd %s cbc_s" % (diag,))
        null = diag.index(0.0)                                     # nothing is drawn along the null direction of A
        runz = run_sampled(ops, c, A=Apsd, z=torch.zeros(BT, 3, **f))
        assert bits(run["xdot_s"][:, null]) == bits(runz["xdot_s"][:, null])


# ------------------------------------------------------------------------------------------------ 4. an unsolved instance
@pytest.mark.parametrize("dtype,model", PAIRS, ids=PAIR_IDS)
def test_unsolved_instance_keeps_its_state_and_its_counters(ops, dtype, model):
    c = case(ops, dtype, model)
    f = dict(dtype=dtype, device=DEV)
    bad = 21
    A = c["gp"]["A"].clone()
    A[bad] = -torch.eye(3, **f)
    run = run_sampled(ops, c, A=A)
    st = run["ws"]["status"]
    assert int(st[bad]) == BADCONE
    assert bits(run["x"][bad]) == bits(c["task"]["x"][bad])
    assert bits(run["xdot_s"][bad]) == bits(torch.zeros(3, **f)) and bits(run["cbc_s"][bad]) == bits(torch.zeros(1 + KOB, **f))
    viol = torch.full((BT, KOB), 5, dtype=torch.int32, device=DEV)
    solved = torch.full((BT,), 9, dtype=torch.int32, device=DEV)
    min_cbc = torch.full((BT, KOB), 1.5, **f)
    ops.rollout_risk(run["cbc_s"], st, viol, solved, min_cbc)
    torch.cuda.synchronize()
    ok = raw(st) == 0
    assert ok.sum() >= 0.8 * BT and not ok[bad]
    cb = raw(run["cbc_s"])[:, 1:]
    np.testing.assert_array_equal(raw(solved), np.where(ok, 10, 9))
    np.testing.assert_array_equal(raw(viol), np.where(ok[:, None], 5 + (cb < 0), 5))
    np.testing.assert_array_equal(raw(min_cbc), np.where(ok[:, None], np.minimum(cb, NP[dtype](1.5)), NP[dtype](1.5)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_rollout_risk_counts_non_finite_values_as_violations(ops, dtype):
    """More than one block (Bt = 300), every kind of value, a mix of statuses."""
    Bt = 300
    rng = np.random.default_rng(5)
    vals = np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 1e-30, -1e-30])
    cb = vals[rng.integers(0, len(vals), size=(Bt, 1 + KOB))].astype(NP[dtype])
    st = rng.integers(0, 4, size=Bt).astype(np.int32) * (rng.random(Bt) < 0.4)
    viol = torch.zeros(Bt, KOB, dtype=torch.int32, device=DEV)
    solved = torch.zeros(Bt, dtype=torch.int32, device=DEV)
    min_cbc = torch.full((Bt, KOB), float("inf"), dtype=dtype, device=DEV)
    for _ in range(2):
        ops.rollout_risk(torch.as_tensor(cb, device=DEV), torch.as_tensor(st.astype(np.int32), device=DEV), viol, solved, min_cbc)
    torch.cuda.synchronize()
    ok = st == 0
    c = np.where(np.isfinite(cb[:, 1:]), cb[:, 1:], -np.inf)
    np.testing.assert_array_equal(raw(solved), 2 * ok)
    np.testing.assert_array_equal(raw(viol), 2 * ((c < 0) & ok[:, None]))
    np.testing.assert_array_equal(raw(min_cbc), np.where(ok[:, None], c, np.inf))


# ------------------------------------------------------------------------------------------------ 5. bookkeeping of a rollout
def test_rollout_risk_block_equals_a_host_recount_eager_and_graph():
    from bayesian_cbf_amd.rollouts import monte_carlo_safety_rollouts
    kw = dict(numSteps=12, start_noise=0.05, seed=3, max_risk=0.2)
    rec = monte_carlo_safety_rollouts(64, plant="posterior", record=True, **kw)
    cbc, st = raw(rec["cbc_s"]), raw(rec["status"])
    assert cbc.shape == (12, 64, 3) and st.shape == (12, 64)
    ok = st == 0
    c = np.where(np.isfinite(cbc[:, :, 1:]), cbc[:, :, 1:], -np.inf)
    per = ((c < 0) & ok[:, :, None]).sum(axis=(0, 1))
    n = int(ok.sum())
    risk = rec["risk"]
    assert n > 0.9 * 12 * 64
    assert risk["instance_steps"] == n and risk["violations"] == int(per.sum()) and risk["max_risk"] == 0.2
    assert risk["rate"] == per.sum() / (n * 2)
    assert [p["violations"] for p in risk["per_obstacle"]] == [int(v) for v in per]
    assert [p["rate"] for p in risk["per_obstacle"]] == [int(v) / n for v in per]
    assert risk["min_cbc"] == [float(v) for v in np.where(ok[:, :, None], c, np.inf).min(axis=(0, 1))]
    # the recorded states are the drawn ones: X[t+1] = X[t] + xdot_s dt is checked by the parity test; here the draw moves them
    eager = monte_carlo_safety_rollouts(64, plant="posterior", **kw)
    graph = monte_carlo_safety_rollouts(64, plant="posterior", use_graph=True, **kw)
    assert bits(eager["x_final"]) == bits(graph["x_final"]) == bits(rec["x_final"])
    assert eager["risk"] == graph["risk"] == risk
    true = monte_carlo_safety_rollouts(64, **kw)
    assert "risk" not in true and bits(true["x_final"]) != bits(eager["x_final"])


def test_true_plant_path_is_the_loop_of_existing_entry_points(ops):
    """plant="true" (the default) is today's path: the same 12 steps restated with the entry points that existed before the
    feature -- plan row, `unicycle_control_step_prepare` without `sampled`, nothing else -- give bit-identical states."""
    from bayesian_cbf_amd.planner import PiecewiseLinearPlanner
    from bayesian_cbf_amd.rollouts import monte_carlo_safety_rollouts, unicycle_task_tensors
    Bt, T, dt = 64, 12, 0.05
    out = monte_carlo_safety_rollouts(Bt, numSteps=T, start_noise=0.05, seed=3, max_risk=0.2, plant="true")
    dflt = monte_carlo_safety_rollouts(Bt, numSteps=T, start_noise=0.05, seed=3, max_risk=0.2)
    assert bits(out["x_final"]) == bits(dflt["x_final"]) and out["stats"] == dflt["stats"]
    f = dict(dtype=torch.float64, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    x0, xg = torch.tensor((-3.0, -1.0, -math.pi / 4), **f), torch.tensor((0.0, 0.0, math.pi / 4), **f)
    task = unicycle_task_tensors(Bt, x0, xg, torch.float64, torch.device(DEV), max_risk=0.2)
    planner = PiecewiseLinearPlanner(x0, xg, T, dt, frac_time_to_reach_goal=0.95)
    x = (x0 + 0.05 * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    ws = ops.control_workspace(Bt, 2, torch.float64, DEV)
    ws["Mk"].zero_()
    ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
    A = torch.diag(torch.tensor((1e-2, 1e-2, 1e-2), **f)).expand(Bt, 3, 3).contiguous()
    task["plan"], task["dot_plan"] = torch.empty(Bt, 3, **f), torch.empty(Bt, 3, **f)
    step = ops.unicycle_control_step_prepare(dict(A=A), task, ws, x, dt=dt, L_true=12.0, L_mean=1.0, max_iters=30)
    for t in range(T):
        task["plan"].copy_(planner.plan(t).to(**f))
        task["dot_plan"].copy_(planner.dot_plan(t).to(**f))
        step()
    torch.cuda.synchronize()
    assert bits(x) == bits(out["x_final"])


# ------------------------------------------------------------------------------------------------ 6. calibration
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("max_risk", [0.2, 0.05])
def test_empirical_risk_matches_the_risk_the_program_was_built_for(ops, dtype, max_risk):
    """ONE step of 4096 independent instances driven at obstacle 0 by the CLF, so that the cone of row 1 is active: the control
    sits where P(CBC_1 < 0) = max_risk under the posterior, and the count of negative drawn conditions is binomial(n, max_risk).
    |v - n delta| <= 5 sqrt(n delta (1 - delta)): a correct build fails this about once in 1e6 runs; a build that ignores z gives
    v = 0, one that scales the draw wrongly fails on one side."""
    from bayesian_cbf_amd.rollouts import unicycle_task_tensors
    Bt = 4096
    f = dict(dtype=dtype, device=DEV)
    f64 = dict(dtype=torch.float64, device="cpu")
    start, goal = torch.tensor((-3.0, -1.0, -math.pi / 4), **f64), torch.tensor((0.0, 0.0, math.pi / 4), **f64)
    task = unicycle_task_tensors(Bt, start, goal, dtype, torch.device(DEV), max_risk=max_risk)
    c0, r0 = raw(task["centers"])[0, 0].astype(np.float64), float(raw(task["radii"])[0, 0])
    rng = np.random.default_rng(2024)
    ang = rng.uniform(0.0, 2 * np.pi, Bt)
    dist = r0 * rng.uniform(1.02, 1.25, Bt)
    head = ang + np.pi + rng.uniform(-0.5, 0.5, Bt)
    ray = np.stack([np.cos(ang), np.sin(ang)], 1)
    xs = np.concatenate([c0 + dist[:, None] * ray, head[:, None]], 1)
    plan = np.concatenate([c0 - dist[:, None] * ray, head[:, None]], 1)           # the mirror point on the far side
    x = torch.as_tensor(xs, **f).contiguous()
    x_start = x.clone()
    task["plan"], task["dot_plan"] = torch.as_tensor(plan, **f).contiguous(), torch.zeros(Bt, 3, **f)
    ws = ops.control_workspace(Bt, KOB, dtype, DEV)
    ws["Mk"].zero_()
    ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
    A = (1e-2 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous()
    out = dict(z=torch.randn(Bt, 3, generator=torch.Generator(device=DEV).manual_seed(11), **f),
               xdot_s=torch.zeros(Bt, 3, **f), cbc_s=torch.zeros(Bt, 1 + KOB, **f))
    ops.unicycle_control_step_prepare(dict(A=A), task, ws, x, dt=DT, L_mean=1.0, clf_gamma=10.0, sampled=out)()
    torch.cuda.synchronize()
    solved = raw(ws["status"]) == 0
    mean, std = R.row_mean_std(raw(ws["y"]), raw(ws["Mk"]), raw(ws["Bk"]), raw(A), raw(ws["grad"]), raw(ws["cst"]), raw(ws["fhat"]),
                               raw(ws["ghat"]), raw(task["sign"]), 1)
    rho = float(task["rho"][0])
    active = solved & (mean - rho * std <= 1e-6 * (1 + np.abs(mean)))
    n, v = int(active.sum()), int((raw(out["cbc_s"])[:, 1][active] < 0).sum())
    print("max_risk %.2f %s: %d / %d solved, %d active, %d negative draws (rate %.4f)" % (max_risk, dtype, solved.sum(), Bt, n, v, v / max(n, 1)))
    assert solved.sum() >= 0.95 * Bt                                    # conditions of the test, not measurements
    assert n >= 0.9 * solved.sum()
    assert abs(v - n * max_risk) <= 5 * math.sqrt(n * max_risk * (1 - max_risk)), (v, n, max_risk)
    assert bits(x[~torch.as_tensor(solved, device=DEV)]) == bits(x_start[~torch.as_tensor(solved, device=DEV)])
