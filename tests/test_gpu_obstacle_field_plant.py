"""GPU tests of the obstacle-field commit on a plant drawn from the model's posterior (bcbf_obstacle_field_commit_sampled,
csrc/field_plant.hip; ops.unicycle_field_control_step_prepare(sampled=...); rollouts.obstacle_field_rollouts(plant="posterior")):
the arithmetic against tests/_obstacle_field_plant_reference.py fed the step's own stored buffers, the instances that must not
move, agreement with the plain sampled step on three discs, the calibration of the tight cone's risk, the joint risk of two active
cones against the union bound, and the rollout's bookkeeping eager / graph / permuted."""
import math

import numpy as np
import pytest
import torch

import _obstacle_field_plant_reference as R
import _obstacle_field_reference as OF
from _tolreport import _record

pytestmark = pytest.mark.gpu
DEV = "cuda"
BT, DT, NTRAIN = R.BT, 0.05, 32
NP = {torch.float64: np.float64, torch.float32: np.float32}
SUMS = ("solved", "viol_tight", "viol_any", "viol_unselected", "viol_discs")
MAX_BORDERLINE = 0.02


@pytest.fixture(scope="module")
def ops():
    from bayesian_cbf_amd import ops as _ops
    return _ops


def raw(t):
    return t.detach().cpu().numpy()


def bits(t):
    return raw(t.contiguous()).tobytes()


def close(actual, desired, scale, dtype, what):
    """The bounds tests/test_gpu_posterior_plant.py applies to xdot_s, x and cbc_s (the arithmetic is specified the same way):
    1e-12 scale in fp64, 2 ulp at scale in fp32 (the reference is the same fp64 evaluation of the same stored inputs, rounded
    once).  The worst ratio goes to the tolerance report."""
    actual, desired = actual.astype(np.float64), desired.astype(np.float64)
    same = (actual == desired) | (np.isnan(actual) & np.isnan(desired))      # (a held instance's non-finite state is itself)
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(actual - desired))
    scale = np.where(same & ~np.isfinite(scale), 1.0, scale)
    if dtype == torch.float64:
        tol, name = 1e-12 * scale, "1e-12 scale"
    else:
        tol, name = 2.0 * np.spacing(scale.astype(np.float32)).astype(np.float64), "2 ulp(scale)"
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    _record(what, ratio, 1.0)
    print("%s: worst error / bound (%s) = %.3e" % (what, name, ratio))
    assert (err <= tol).all(), "%s: worst error / bound (%s) = %.3e" % (what, name, ratio)


_GP = {}


def learned_gp(ops, dtype):
    """A small learned model per instance (N = 32): make_instances' data with a residual a tenth as large and A near 0.01 I."""
    if dtype not in _GP:
        from bayesian_cbf_amd.synthetic import make_instances
        p = make_instances(BT, NTRAIN, 3, 2, dtype=dtype, device=DEV, seed=11)
        g = torch.Generator(device=DEV).manual_seed(11)
        A = (torch.eye(3, dtype=dtype, device=DEV)[None] * (0.01 + 0.005 * torch.rand(BT, 1, 1, generator=g, dtype=dtype, device=DEV))).contiguous()
        Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], (0.05 * p["Bm"]).contiguous(), p["ell"], p["s2"], p["jitter"])
        assert (info == 0).all()
        Vw, _ = ops.potrs(Lop, (0.1 * p["Xdot"]).contiguous(), p["UH"], p["M0"], want_alpha=False)
        _GP[dtype] = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=(0.05 * p["Bm"]).contiguous(), M0=p["M0"], A=A)
    return _GP[dtype]


def field_task(Bt, S, dtype, max_risk=0.01):
    from bayesian_cbf_amd.rollouts import unicycle_task_tensors
    f = dict(dtype=dtype, device=DEV)
    task = unicycle_task_tensors(Bt, torch.tensor(OF.START), torch.tensor(OF.GOAL), dtype, torch.device(DEV), max_risk=max_risk,
                                 cbf_gammas=(5.0,) * S)
    task.update(sign=torch.tensor([-1.0] + [1.0] * S, **f), relax_mask=torch.tensor([1.0] + [0.0] * S, **f))
    return task


def run_field_step(ops, case, S, dtype, model="fixed", max_risk=0.01, rounds=3, dt=DT, prefill=True):
    """One sampled field step on the inputs of `case` (numpy, R.make_case's keys).  The accumulators start from nonzero values, so
    the in-place update shows.  Returns everything the reference needs, as stored."""
    f = dict(dtype=dtype, device=DEV)
    Bt = case["x"].shape[0]
    t = lambda a: torch.as_tensor(np.asarray(a), **f).contiguous()
    task = field_task(Bt, S, dtype, max_risk)
    task["plan"], task["dot_plan"] = t(case["plan"]), t(case["dot_plan"])
    x = t(case["x"])
    x0 = x.clone()
    field = dict(centers=t(case["centers"]), radii=t(case["radii"]))
    ws = ops.control_workspace(Bt, S, dtype, DEV)
    if model == "fixed":
        ws["Mk"].zero_(); ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        gp = dict(A=(0.01 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous())
    else:
        gp = learned_gp(ops, dtype)
    risk = ops.obstacle_field_risk_workspace(Bt, dtype, DEV)
    risk["z"].copy_(t(case["z"]))
    if prefill:
        for i, k in enumerate(SUMS):
            risk[k].fill_(3 + i)
        risk["min_cbc"].fill_(1.5)
        for k in ("xdot_s", "cbc_min", "cbc_tight", "cbc_argmin", "tight_idx", "nneg"):
            risk[k].fill_(7)
    start = {k: raw(risk[k]).copy() for k in SUMS + ("min_cbc",)}
    step = ops.unicycle_field_control_step_prepare(gp, task, field, ws, x, rounds=rounds, dt=dt, L_true=12.0, L_mean=1.0, max_iters=100,
                                                   sampled=dict(z=risk["z"], risk=risk))
    step()
    torch.cuda.synchronize()
    return dict(x0=x0, x=x, ws=ws, fws=step.fws, risk=risk, start=start, task=task, field=field, A=gp["A"], dtype=dtype)


def reference_of(run, dt=DT):
    ws, fws, t = run["ws"], run["fws"], run["task"]
    return R.step(raw(run["x0"]), raw(ws["y"]), raw(fws["status_eff"]), raw(ws["Mk"]), raw(ws["Bk"]), raw(run["A"]), raw(ws["fhat"]),
                  raw(ws["ghat"]), raw(t["rho"]), raw(run["field"]["centers"]), raw(run["field"]["radii"]), raw(t["tw"]),
                  float(t["gammas"][0]), raw(fws["idx"]), raw(run["risk"]["z"]), dt, dtype=NP[run["dtype"]])


def check_against_reference(run, ref, tag):
    dtype, risk, npd = run["dtype"], run["risk"], NP[run["dtype"]]
    close(raw(risk["xdot_s"]), ref["xdot_s"], ref["scale_xdot"], dtype, tag + " xdot_s")
    close(raw(run["x"]), ref["x_next"], ref["scale_x"], dtype, tag + " x")
    close(raw(risk["cbc_min"]), ref["cbc_min"], ref["scale_cbc_min"], dtype, tag + " cbc_min")
    ok = ~ref["borderline"]                          # where an argmin may differ, so may the value it names
    close(raw(risk["cbc_tight"])[ok], ref["cbc_tight"][ok], ref["scale_cbc_tight"][ok], dtype, tag + " cbc_tight")
    taken = ref["solved"] == 1
    assert ref["borderline"].sum() <= MAX_BORDERLINE * max(int(taken.sum()), 1), (int(ref["borderline"].sum()), int(taken.sum()))
    for k in ("cbc_argmin", "tight_idx", "nneg"):
        np.testing.assert_array_equal(raw(risk[k])[ok], ref[k][ok], err_msg=k)
    for k in SUMS:
        np.testing.assert_array_equal(raw(risk[k])[ok], (run["start"][k] + ref[k])[ok], err_msg=k)
    want = np.minimum(run["start"]["min_cbc"], ref["min_cbc"].astype(npd))
    got = raw(risk["min_cbc"])
    close(got[taken], want[taken], ref["scale_cbc_min"][taken], dtype, tag + " min_cbc")
    assert np.array_equal(got[~taken], run["start"]["min_cbc"][~taken])
    assert (raw(run["fws"]["status_eff"]) == 0).tolist() == taken.tolist()
    return int(taken.sum()), int(ref["borderline"].sum())


# ------------------------------------------------------------------------------------------------ 1. the arithmetic
@pytest.mark.parametrize("Kf,S,per,seed", R.SHAPES, ids=["Kf%d-S%d-%s" % (k, s, "own" if p else "shared") for k, s, p, _ in R.SHAPES])
@pytest.mark.parametrize("model", ["fixed", "learned"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_draw_and_every_discs_condition_match_the_reference(ops, dtype, model, Kf, S, per, seed):
    """Bt = 67 (a partial workgroup); Kf = 3, 64, 65, 256 (Kf = S, exactly one lap, one disc past a lap, all laps); S = 1, 3; one
    field or one per instance; both precisions; the fixed-kernel model and a learned one of 32 points.  The reference is fed the
    step's stored buffers.  Values within the posterior-plant bounds relative to the reference's scale_*; integer outputs and
    counters equal except where the reference flags the instance borderline (at most 2 % of the instance-steps; the CPU test shows
    none for these seeds on the oracle's optimum)."""
    if model == "learned":
        seed = R.SEEDS_LEARNED[[s[:3] for s in R.SHAPES].index((Kf, S, per))]
    case = R.make_case(Kf, S, per, seed)
    run = run_field_step(ops, case, S, dtype, model)
    ref = reference_of(run)
    taken, border = check_against_reference(run, ref, "field plant %s-%s Kf%d S%d %s" % (NP[dtype].__name__, model, Kf, S, "own" if per else "shared"))
    print("%d of %d instances stepped, %d borderline" % (taken, BT, border))
    assert taken >= 0.2 * BT
    assert np.abs(raw(run["risk"]["xdot_s"])[ref["solved"] == 1]).min() > 0          # the fill value is gone, the draw is not degenerate


def test_dt_zero_keeps_the_state_and_does_everything_else(ops):
    case = R.make_case(65, 3, False, 1170)
    run = run_field_step(ops, case, 3, torch.float64, dt=0.0)
    assert bits(run["x"]) == bits(run["x0"])
    ref = reference_of(run, dt=0.0)
    check_against_reference(run, ref, "field plant dt=0")
    assert ref["solved"].sum() >= 0.2 * BT


# ------------------------------------------------------------------------------------------------ 2. instances that must not move
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_unsolved_and_uncertified_instances_keep_state_and_counters(ops, dtype):
    """One slot and one round among nearby discs (whoever needs a second cone stays uncertified) and three non-finite start states
    (unsolved): state bit for bit, xdot_s = 0, indices -1, accumulators untouched; status_eff is the plain commit's."""
    from bayesian_cbf_amd.rollouts import random_obstacle_field
    Bt = 67
    fld = random_obstacle_field(16, seed=31, box=((-3.6, -1.4), (-2.1, 0.3)), clear_start=0.35)
    rng = np.random.RandomState(12)
    x = OF.START[None] + rng.randn(Bt, 3) * np.array([0.4, 0.4, 1.0])
    x[5, 0], x[40, 2], x[66, 1] = np.nan, np.inf, np.nan
    plan = np.tile(OF.START + 0.15 * (OF.GOAL - OF.START), (Bt, 1))
    case = dict(x=x, plan=plan, dot_plan=np.tile((OF.GOAL - OF.START) / 5.0, (Bt, 1)), centers=fld["centers"].numpy(),
                radii=fld["radii"].numpy(), z=rng.randn(Bt, 3))
    run = run_field_step(ops, case, 1, dtype, rounds=1)
    ws, fws, risk = run["ws"], run["fws"], run["risk"]
    eff, cert, status = raw(fws["status_eff"]), raw(fws["cert"]), raw(ws["status"])
    print("cert histogram %s, status_eff values %s" % (np.bincount(cert, minlength=4).tolist(), sorted(set(eff.tolist()))))
    # the plain commit on a copy of the same buffers
    plain = {k: v.clone() for k, v in fws.items()}
    plain["status_eff"].fill_(-5)
    ops.obstacle_field_commit(run["x0"].clone(), ws["y"], ws["status"], plain, DT, 12.0)
    torch.cuda.synchronize()
    assert bits(plain["status_eff"]) == bits(fws["status_eff"])
    held = eff != 0
    assert held[[5, 40, 66]].all() and (status[[5, 40, 66]] != 0).all()
    assert ((cert != OF.CERTIFIED) & (status == 0)).sum() >= 1 and (eff[(cert != OF.CERTIFIED) & (status == 0)] == OF.UNCERTIFIED).all()
    assert (~held).sum() >= 10
    h = torch.as_tensor(held, device=DEV)
    assert bits(run["x"][h]) == bits(run["x0"][h])
    word = np.uint64 if dtype == torch.float64 else np.uint32       # bit patterns: a held NaN state is equal to itself
    moved = (raw(run["x"]).view(word) != raw(run["x0"]).view(word)).any(1)
    assert (moved == ~held).all()
    assert bits(risk["xdot_s"][h]) == bits(torch.zeros(int(held.sum()), 3, dtype=dtype, device=DEV))
    for k in ("cbc_min", "cbc_tight"):
        assert bits(risk[k][h]) == bits(torch.zeros(int(held.sum()), dtype=dtype, device=DEV)), k
    assert (raw(risk["cbc_argmin"])[held] == -1).all() and (raw(risk["tight_idx"])[held] == -1).all() and (raw(risk["nneg"])[held] == 0).all()
    for k in SUMS + ("min_cbc",):
        assert np.array_equal(raw(risk[k])[held], run["start"][k][held]), k
        assert (raw(risk["solved"])[~held] == run["start"]["solved"][~held] + 1).all()
    check_against_reference(run, reference_of(run), "field plant held-%s" % NP[dtype].__name__)


# ------------------------------------------------------------------------------------------------ 3. the plain sampled step
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_three_disc_field_agrees_with_the_plain_sampled_step(ops, dtype):
    """Kf = S = 3 and the same z: the field step against `unicycle_control_step_prepare(sampled=...)` on the same three discs in the
    working set's order (the solves are the same kernel on the same inputs).  The drawn condition of each disc comes out of the
    field kernel as cbc_min of a one-disc field, run with dt = 0 on the step's own buffers."""
    f = dict(dtype=dtype, device=DEV)
    case = R.make_case(3, 3, True, 121)
    run = run_field_step(ops, case, 3, dtype, prefill=False)
    ws, fws, task = run["ws"], run["fws"], run["task"]
    eff = raw(fws["status_eff"])
    ptask = dict(task, centers=fws["centers_sel"], radii=fws["radii_sel"])
    x2, ws2 = run["x0"].clone(), ops.control_workspace(BT, 3, dtype, DEV)
    ws2["Mk"].zero_(); ws2["Bk"].copy_(torch.eye(3, **f).expand(BT, 3, 3))
    out = dict(z=run["risk"]["z"].clone(), xdot_s=torch.zeros(BT, 3, **f), cbc_s=torch.zeros(BT, 4, **f))
    ops.unicycle_control_step_prepare(dict(A=run["A"]), ptask, ws2, x2, dt=DT, L_true=12.0, L_mean=1.0, max_iters=100, sampled=out)()
    torch.cuda.synchronize()
    assert bits(ws2["y"]) == bits(ws["y"]) and bits(ws2["status"]) == bits(ws["status"])
    assert ((eff == 0) == (raw(ws["status"]) == 0)).all() and (eff == 0).sum() >= 0.8 * BT      # Kf = S: solved means certified
    ref = R.step(raw(run["x0"]), raw(ws["y"]), eff, raw(ws["Mk"]), raw(ws["Bk"]), raw(run["A"]), raw(ws["fhat"]), raw(ws["ghat"]),
                 raw(task["rho"]), raw(fws["centers_sel"]), raw(fws["radii_sel"]), raw(task["tw"]), 5.0, np.tile(np.arange(3), (BT, 1)),
                 raw(out["z"]), DT, dtype=NP[dtype])
    tag = "field plant vs plain %s" % NP[dtype].__name__
    close(raw(run["risk"]["xdot_s"]), raw(out["xdot_s"]), ref["scale_xdot"], dtype, tag + " xdot_s")
    close(raw(run["x"]), raw(x2), ref["scale_x"], dtype, tag + " x")
    for s in range(3):
        one = ops.obstacle_field_risk_workspace(BT, dtype, DEV)
        one["z"].copy_(out["z"])
        fone = dict(idx=torch.zeros(BT, 1, dtype=torch.int32, device=DEV), cert=fws["cert"], status_eff=torch.zeros(BT, dtype=torch.int32, device=DEV))
        disc = dict(centers=fws["centers_sel"][:, s:s + 1].contiguous(), radii=fws["radii_sel"][:, s:s + 1].contiguous())
        ops.obstacle_field_commit_sampled(run["x0"].clone(), ws, run["A"], task["rho"], disc, task["tw"], 5.0, fone, one, 0.0)
        torch.cuda.synchronize()
        close(raw(one["cbc_min"]), raw(out["cbc_s"])[:, 1 + s], ref["scale_cbc"][:, s], dtype, tag + " cbc of slot %d" % s)


# ------------------------------------------------------------------------------------------------ 4. calibration
@pytest.mark.parametrize("max_risk", [0.2, 0.05])
def test_tight_cone_risk_is_calibrated_on_the_device(ops, max_risk):
    """The recipe of the CPU test at 4096 instances, one step: the negative draws of the tight (active) cone are
    binomial(n, max_risk); |v - n max_risk| <= 5 sigma.  A build that ignores z gives 0, one that scales the draw wrongly fails on
    one side."""
    Bt = 4096
    case = R.calibration_case(Bt)
    run = run_field_step(ops, case, 1, torch.float64, max_risk=max_risk, prefill=False)
    risk = run["risk"]
    ref = reference_of(run)
    solved = raw(risk["solved"]) == 1
    ti = np.where(solved, raw(risk["tight_idx"]), 0)
    m, E = ref["margin"][np.arange(Bt), ti], ref["E"][np.arange(Bt), ti]
    active = solved & (m <= 1e-6 * (1 + np.abs(E)))
    vt, va, vd = raw(risk["viol_tight"]), raw(risk["viol_any"]), raw(risk["viol_discs"])
    n, v = int(active.sum()), int(vt[active].sum())
    print("max_risk %.2f: %d / %d stepped, %d active, %d negative draws of the tight cone (rate %.4f)" % (max_risk, solved.sum(), Bt, n, v, v / max(n, 1)))
    assert solved.sum() >= 0.95 * Bt and n >= 0.9 * solved.sum()                  # conditions of the test, not measurements
    assert (raw(risk["tight_idx"])[solved] == case["near"]).all()
    assert R.binomial_ok(v, n, max_risk), (v, n, max_risk)
    assert (va >= vt).all() and (vd >= va).all()
    assert (vt[active] == (raw(risk["cbc_tight"])[active] < 0)).all()


# ------------------------------------------------------------------------------------------------ 5. joint risk
def test_joint_risk_of_two_active_cones_is_under_the_union_bound(ops):
    """Two equal discs mirrored about the heading, the target straight ahead between them: by symmetry the optimum turns nowhere
    and both cones bind.  Each cone is violated with probability max_risk on the draw; 'any' is bounded by the union, 2 max_risk."""
    Bt, max_risk = 4096, 0.1
    rng = np.random.default_rng(77)
    phi = rng.uniform(0.0, 2 * np.pi, Bt)
    d, a, r = rng.uniform(0.7, 0.9, Bt), rng.uniform(0.5, 0.6, Bt), rng.uniform(0.35, 0.45, Bt)
    p = rng.uniform(-1.0, 1.0, (Bt, 2))
    fwd, left = np.stack([np.cos(phi), np.sin(phi)], 1), np.stack([-np.sin(phi), np.cos(phi)], 1)
    centers = np.stack([p + d[:, None] * fwd + a[:, None] * left, p + d[:, None] * fwd - a[:, None] * left], 1)
    case = dict(x=np.concatenate([p, phi[:, None]], 1), plan=np.concatenate([p + 3.0 * fwd, phi[:, None]], 1),
                dot_plan=np.zeros((Bt, 3)), centers=centers, radii=np.stack([r, r], 1), z=rng.standard_normal((Bt, 3)))
    run = run_field_step(ops, case, 2, torch.float64, max_risk=max_risk, prefill=False)
    risk = run["risk"]
    ref = reference_of(run)
    solved = raw(risk["solved"]) == 1
    both = solved & (ref["margin"] <= 1e-6 * (1 + np.abs(ref["E"]))).all(1)
    vt, va, vd = (raw(risk[k]) for k in ("viol_tight", "viol_any", "viol_discs"))
    n = int(solved.sum())
    print("two active cones: %d / %d stepped, %d with both active; tight %.4f, any %.4f, discs/step %.4f (max_risk %.2f)"
          % (n, Bt, both.sum(), vt.sum() / n, va.sum() / n, vd.sum() / n, max_risk))
    assert n >= 0.95 * Bt and both.sum() >= 0.9 * n                               # conditions of the test, not measurements
    assert (vt <= va).all() and (va <= vd).all()
    pu = 2 * max_risk
    assert va.sum() / n <= pu + 5 * math.sqrt(pu * (1 - pu) / n), (int(va.sum()), n)
    assert va.sum() > vt.sum()                                                    # the joint event is strictly more than the tight cone's


# ------------------------------------------------------------------------------------------------ 6. the rollout
def test_rollout_bookkeeping_eager_graph_and_permuted(ops):
    from bayesian_cbf_amd.rollouts import obstacle_field_rollouts, random_obstacle_field
    Bt, T = 67, 40
    fld = random_obstacle_field(16, seed=2)
    kw = dict(numSteps=T, start_noise=0.05, seed=3, max_risk=0.2, plant="posterior")
    rec = obstacle_field_rollouts(Bt, fld, record=True, **kw)
    eager = obstacle_field_rollouts(Bt, fld, **kw)
    graph = obstacle_field_rollouts(Bt, fld, use_graph=True, **kw)
    assert bits(rec["x_final"]) == bits(eager["x_final"]) == bits(graph["x_final"])
    for k, v in rec["risk_counters"].items():
        assert bits(v) == bits(eager["risk_counters"][k]) == bits(graph["risk_counters"][k]), k
    assert rec["risk"] == eager["risk"] == graph["risk"]
    risk = rec["risk"]
    taken = raw(rec["status_eff"]) == 0
    n = int(taken.sum())
    assert int(rec["solved"].sum()) == n == risk["instance_steps"] and n >= 0.5 * T * Bt
    assert (raw(rec["solved"]) == taken.sum(0)).all()
    nneg, ct = raw(rec["nneg"]), raw(rec["cbc_tight"])
    c = rec["risk_counters"]
    assert (raw(c["viol_any"]) == ((nneg > 0) & taken).sum(0)).all() and (raw(c["viol_discs"]) == np.where(taken, nneg, 0).sum(0)).all()
    assert (raw(c["viol_tight"]) == ((ct < 0) & taken).sum(0)).all()
    assert np.array_equal(raw(c["min_cbc"]), np.where(taken, raw(rec["cbc_min"]), np.inf).min(0))
    assert risk["tight"] == raw(c["viol_tight"]).sum() / n and risk["joint"] == raw(c["viol_any"]).sum() / n
    assert risk["unselected"] == raw(c["viol_unselected"]).sum() / n and risk["mean_discs_violated"] == raw(c["viol_discs"]).sum() / n
    assert risk["tight"] <= risk["joint"] <= risk["mean_discs_violated"] and risk["unselected"] <= risk["joint"]
    assert risk["max_risk"] == 0.2 and risk["min_cbc"] == float(raw(c["min_cbc"]).min())
    true = obstacle_field_rollouts(Bt, fld, numSteps=T, start_noise=0.05, seed=3, max_risk=0.2)
    assert "risk" not in true and bits(true["x_final"]) != bits(eager["x_final"])
    # the caller's start states and normals, and the same ones permuted
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = torch.tensor(OF.START, device=DEV) + 0.05 * torch.randn(Bt, 3, generator=g, dtype=torch.float64, device=DEV)
    zs = torch.randn(T, Bt, 3, generator=g, dtype=torch.float64, device=DEV)
    perm = torch.randperm(Bt, generator=torch.Generator().manual_seed(6)).to(DEV)
    a = obstacle_field_rollouts(Bt, fld, x_start=xs, z_all=zs, **kw)
    b = obstacle_field_rollouts(Bt, fld, x_start=xs[perm], z_all=zs[:, perm], **kw)
    assert bits(a["x_final"][perm]) == bits(b["x_final"]) and bits(a["x_final"]) != bits(eager["x_final"])
    for k, v in a["risk_counters"].items():
        assert bits(v[perm]) == bits(b["risk_counters"][k]), k
    assert a["risk"] == b["risk"]
