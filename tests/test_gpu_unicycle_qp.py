"""The unicycle CLF-CBF quadratic program on the mean model on the device (bcbf_clf_cbf_qp2, bcbf_unicycle_clf_cbf_control,
bcbf_unicycle_clf_cbf_rollout) against the numpy yardstick of tests/_unicycle_qp_reference.py, which tests/test_unicycle_qp_cpu.py
holds to the reference's recorded rows, to oracle.socp.coneqp and to SLSQP.  Bounds: the project's own-relative parity
bounds, 1e-8 (fp64) / 1e-3 (fp32); `status` and `active` are compared on the programs whose decision margin exceeds 1e-9 / 1e-4
(the CPU test caps the share left out)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _unicycle_qp_reference as R
from _tolreport import rel_close
from test_unicycle_qp_cpu import MARGIN, MAX_EXCLUDED, loop_case, solver_programs

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = dict(np.load(os.path.join(ROOT, "tests", "golden", "unicycle_clf_qp_rows.npz")))
NP = {torch.float64: np.float64, torch.float32: np.float32}
RTOL = {torch.float64: 1e-8, torch.float32: 1e-3}          # the project's parity bounds, own-relative
BTS = [1, 63, 64, 130]
# Free-running drift of the device loop against the numpy loop over 300 steps, 130 starts, every second one on a mismatched
# plant: the worst own-relative deviation of x_final, min_h and cost MEASURED on an MI355X (profiles/unicycle_clf_cbf.json,
# "free_running_drift").  The test asserts 100 times the measured worst, floor 1e-10.
FREE_RUN_MEASURED = 7.8e-15         # x_final 7.7e-15, min_h 2.5e-15, cost 1.0e-15
FREE_RUN_BOUND = max(100 * FREE_RUN_MEASURED, 1e-10)


def raw(t):
    return t.detach().cpu().numpy()


def bits(t):
    return raw(t.contiguous()).tobytes()


def T(v, dtype=torch.float64):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV).contiguous()


@pytest.fixture(scope="module")
def ops():
    from bayesian_cbf_amd import ops as _ops
    return _ops


def rnd(v, dtype):
    """The values the device receives in the precision under test, as float64."""
    return np.asarray(v, dtype=NP[dtype]).astype(np.float64)


def task_kw(t, dtype=torch.float64, centers=None, radii=None):
    kw = dict(Kp=t["Kp"], clf_kind=t["clf_kind"], clf_gamma=t["clf_gamma"], relax_weight=t["relax_weight"], lo=t["lo"], hi=t["hi"])
    if centers is not None:
        kw.update(centers=T(centers, dtype), radii=T(radii, dtype), tw=t["tw"], gammas=t["gammas"])
    return kw


def rounded_task(t, dtype):
    return dict(t, Kp=tuple(rnd(t["Kp"], dtype)), lo=rnd(t["lo"], dtype), hi=rnd(t["hi"], dtype), tw=tuple(rnd(t["tw"], dtype)),
                gammas=tuple(rnd(t["gammas"], dtype)))


def compare_solution(got, want, dtype, what, a=None):
    """u and relax on EVERY feasible program; status and active where the decision margin allows."""
    sure = want["margin"] > MARGIN[NP[dtype]]
    assert (~sure).sum() <= max(MAX_EXCLUDED * len(sure), 1), (what, int((~sure).sum()), len(sure))
    st = raw(got["status"])
    assert (st[sure] == want["status"][sure]).all(), what
    both = (st == 0) & (want["status"] == 0)
    assert both.sum() >= 0.5 * (want["status"] == 0).sum()
    if both.any():
        rel_close(raw(got["u"])[both], want["u"][both], RTOL[dtype], what=what + " u")
        rel_close(raw(got["relax"])[both], want["relax"][both], RTOL[dtype], what=what + " relax")
    ok = sure & both
    assert (raw(got["active"])[ok] == want["active"][ok]).all(), what
    return st


# ------------------------------------------------------------------------------------------------ 1. the solver alone
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_solver_alone(ops, dtype, K):
    a, b = solver_programs()[K]
    a, b = rnd(a, dtype), rnd(b, dtype)
    assert len(b) > 130                                       # more than two waves, a ragged last one
    want = R.solve_qp2(a, b, rnd(R.LO, dtype), rnd(R.HI, dtype), 10.0, R.EPS[np.dtype(NP[dtype])])
    assert (want["status"] == 0).any() and ((want["status"] == 1).any() or K == 1)      # (the box alone is never empty)
    got = ops.clf_cbf_qp2(T(a, dtype), T(b, dtype))
    st = compare_solution(got, want, dtype, "qp2 K=%d" % K)
    # nothing is written where status is 1: the wrapper's sentinels (NaN, NaN, -1) are still there
    bad = st == 1
    assert np.isnan(raw(got["u"])[bad]).all() and np.isnan(raw(got["relax"])[bad]).all() and (raw(got["active"])[bad] == -1).all()
    assert np.isfinite(raw(got["u"])[~bad]).all()


@pytest.mark.parametrize("Bt", BTS)
def test_solver_every_output_is_optional_at_every_batch_shape(ops, Bt):
    a, b = solver_programs()[3]
    a, b = T(a[:Bt]), T(b[:Bt])
    full = ops.clf_cbf_qp2(a, b)
    assert full["u"].shape == (Bt, 2)
    for name in ("u", "relax", "active", "status"):
        one = ops.clf_cbf_qp2(a, b, want=(name,))
        assert list(one) == [name] and bits(one[name]) == bits(full[name]), name
    assert ops.clf_cbf_qp2(a, b, want=()) == {}


# ------------------------------------------------------------------------------------------------ 2. one-step parity
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["polar", "cartesian-0", "cartesian-2"])
def test_one_step_parity_on_the_golden_states(ops, dtype, kind):
    g = GOLDEN
    x = rnd(np.tile(g["x"], (3, 1))[:130], dtype)
    if kind == "polar":
        t = rounded_task(R.task(Kp=tuple(g["Kp_polar"]), clf_kind=1), dtype)
        plan, dplan, cen, rad = rnd(g["goal"], dtype), np.zeros(3), None, None
    else:
        t = rounded_task(R.task(Kp=tuple(g["Kp_cart"]) + (0.0,), tw=tuple(g["tw"]), gammas=tuple(g["gammas"])), dtype)
        plan, dplan = rnd(g["cart_plan"][2], dtype), rnd(g["cart_dot_plan"][2], dtype)
        cen, rad = (rnd(g["centers"], dtype), rnd(g["radii"], dtype)) if kind == "cartesian-2" else (None, None)
        if cen is None:
            t = dict(t, gammas=())
    want = R.control(x, plan, dplan, 1.0, cen, rad, t, R.EPS[np.dtype(NP[dtype])])
    B = len(x)
    got = ops.unicycle_clf_cbf_control(T(x, dtype), T(np.broadcast_to(plan, (B, 3)), dtype), T(np.broadcast_to(dplan, (B, 3)), dtype),
                                       L_ctrl=1.0, **task_kw(t, dtype, cen, rad))
    # rows: a state inside an obstacle or 1e-3 from the goal has rows of very different sizes; each row against its own scale
    for name in ("a", "b", "values"):
        w, d = want[name], raw(got[name])
        for k in range(w.shape[1]):
            rel_close(d[:, k], w[:, k], RTOL[dtype], what="%s %s row %d" % (kind, name, k))
    compare_solution(got, want, dtype, kind)


# ------------------------------------------------------------------------------------------------ the closed loops
def dev_rollout(ops, case, steps=None, dtype=torch.float64, record_every=0, t_offset=0, state=None, x0=None, **over):
    """One launch of the loop `case` (tests/test_unicycle_qp_cpu.loop_case's keywords) from fresh statistics, or from `state`."""
    c = dict(case, **over)
    f = dict(dtype=dtype, device=DEV)
    x0 = c["x0"] if x0 is None else x0
    Bt = len(x0)
    steps = c["numSteps"] if steps is None else steps
    if state is None:
        state = dict(x=T(x0, dtype), min_h=torch.full((Bt,), float("inf"), **f), cost=torch.zeros(Bt, **f),
                     status=torch.zeros(Bt, dtype=torch.int32, device=DEV),
                     converged_at=torch.full((Bt,), -1, dtype=torch.int32, device=DEV))
    nrec = ops.unicycle_clf_cbf_records(t_offset, steps, record_every)
    traj = torch.full((nrec, Bt, 3), float("nan"), **f) if record_every > 0 else None
    us = torch.full((nrec, Bt, 2), float("nan"), **f) if record_every > 0 else None
    t = c["t"]
    kw = task_kw(t, dtype, c.get("centers"), c.get("radii"))
    Lt = c["L_true"]
    ops.unicycle_clf_cbf_rollout(
        state["x"], T(np.broadcast_to(c["goal"], (Bt, 3)), dtype), state["cost"], state["status"], steps, dt=c["dt"],
        min_h=state["min_h"], converged_at=state["converged_at"], planner=c.get("planner", 0),
        x0_plan=T(np.broadcast_to(c["x0_plan"], (Bt, 3)), dtype) if c.get("planner", 0) else None,
        numStepsPlan=c.get("numStepsPlan", 0), frac_time_to_reach_goal=c.get("frac", 0.7), L_ctrl=c["L_ctrl"],
        L_true=T(Lt, dtype) if np.ndim(Lt) else Lt, stop_rho=c.get("stop_rho", 0.0), traj=traj, u_rec=us,
        record_every=record_every, t_offset=t_offset, **kw)
    torch.cuda.synchronize()
    return dict(state, traj=traj, u=us)


@pytest.fixture(scope="module")
def case():
    return loop_case()


@pytest.fixture(scope="module")
def dev_loop(ops, case):
    return dev_rollout(ops, case, record_every=1)


def test_teacher_forced_loop(ops, case, dev_loop):
    """From each recorded x_t the yardstick recomputes u_t and x_{t+1}; min_h and cost follow from the records."""
    c = case
    X, U = raw(dev_loop["traj"]), raw(dev_loop["u"])
    n, Bt = X.shape[:2]
    assert n == 300 and Bt == 130 and (raw(dev_loop["status"]) == 0).all()
    Xall = np.concatenate([X, raw(dev_loop["x"])[None]])
    hmin, cost, masks = np.full(Bt, np.inf), np.zeros(Bt), set()
    for s in range(n):
        pl, dp = R.plan(1, c["x0_plan"], np.broadcast_to(c["goal"], (Bt, 3)), s, c["numStepsPlan"], c["dt"], c["frac"])
        w = R.control(X[s], pl, dp, c["L_ctrl"], c["centers"], c["radii"], c["t"])
        assert (w["status"] == 0).all()
        rel_close(U[s], w["u"], 1e-8, what="teacher-forced u")
        rel_close(Xall[s + 1], R.plant_step(X[s], U[s], c["L_true"], c["dt"]), 1e-8, what="teacher-forced x")
        hmin = np.minimum(hmin, w["values"][:, 1:].min(1))
        cost += (U[s] ** 2).sum(1)
        masks |= set(w["active"][w["margin"] > 1e-9].tolist())
    rel_close(raw(dev_loop["min_h"]), hmin, 1e-8, what="min_h from the records")
    rel_close(raw(dev_loop["cost"]), cost, 1e-8, what="cost from the records")
    assert 0 in masks and any(m & 0xF for m in masks) and any(m >> 4 for m in masks)      # unconstrained, box, obstacle


def test_free_running_loop(ops, case, dev_loop):
    ref = R.rollout(**case)
    worst = {}
    for name, got, want in (("x_final", dev_loop["x"], ref["x"]), ("min_h", dev_loop["min_h"], ref["min_h"]),
                            ("cost", dev_loop["cost"], ref["cost"])):
        worst[name] = float(np.abs(raw(got) - want).max() / np.abs(want).max())
    print("free-running drift over 300 steps: %s (bound %.1e)" % (worst, FREE_RUN_BOUND))
    out = os.environ.get("BCBF_UNICYCLE_QP_DRIFT_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(worst, fh)
    assert (raw(dev_loop["status"]) == ref["status"]).all()
    assert max(worst.values()) <= FREE_RUN_BOUND, worst


def polar_case(Bt=130):
    return dict(x0=R.starts(Bt, noise=(0.5, 0.5, 1.0), seed=3), goal=R.GOAL, numSteps=2000, dt=0.01, L_ctrl=1.0, L_true=1.0,
                t=R.task(Kp=R.KP_POLAR, clf_kind=1), stop_rho=1e-3)


def test_polar_move_to_pose(ops):
    """Every instance converges, the step is the yardstick's, the state is frozen afterwards.
    The polar loop at dt = 0.01 overshoots the goal on some starts (rho 0.011 -> 0.089 in one step, alpha turning by pi), and
    from there on its trajectory is not a continuous function of the start: the YARDSTICK's own converged_at moves by up to 257
    steps when its start is perturbed by 1e-15 .. 1e-13 relative (instances 27, 33, 52 of these 63).  Measured on an MI355X: 62 of
    63 free-running convergence steps equal the yardstick's, instance 27 differs by 16.  So the step is held twice:
    on the device's OWN recorded trajectory for every instance (the first t with rho(x_t) < stop_rho, as numpy computes it; exact
    where that rho is further than 1e-9 from stop_rho), and free-running against the yardstick for the instances whose yardstick
    answer survives those perturbations."""
    c = polar_case(63)
    got = dev_rollout(ops, c, record_every=1)
    conv = raw(got["converged_at"])
    assert (raw(got["status"]) == 0).all() and (conv > 0).all() and (conv < 2000).all()
    X, U, xf = raw(got["traj"]), raw(got["u"]), raw(got["x"])
    rho = np.hypot(R.GOAL[0] - X[..., 0], R.GOAL[1] - X[..., 1])                 # [2000, 63]
    clear = np.abs(rho - 1e-3) > 1e-9
    for b in range(63):
        assert clear[:conv[b] + 1, b].all() and (rho[:conv[b], b] >= 1e-3).all() and rho[conv[b], b] < 1e-3, b
        assert (X[conv[b]:, b] == xf[b]).all() and (U[conv[b]:, b] == 0).all()               # frozen afterwards, u = 0
    n = int(conv.max()) + 2
    ref = R.rollout(c["x0"], c["goal"], n, dt=c["dt"], t=c["t"], stop_rho=1e-3)
    stable = np.abs(ref["rho_at"] - 1e-3) > 1e-9
    for eps in (1e-15, -1e-14, 1e-13):
        stable &= R.rollout(c["x0"] * (1 + eps), c["goal"], n, dt=c["dt"], t=c["t"], stop_rho=1e-3)["converged_at"] == ref["converged_at"]
    diff = conv - ref["converged_at"]
    print("polar move_to_pose: converged in %d..%d steps; %d of 63 differ from the free-running yardstick (by %s); %d stable"
          % (conv.min(), conv.max(), (diff != 0).sum(), sorted(set(diff[diff != 0].tolist())), stable.sum()))
    assert stable.sum() >= 55 and (diff[stable] == 0).all()
    # teacher-forced controls on the way, and box rows were active
    for s in range(0, int(conv.min()), 9):
        w = R.control(X[s], np.broadcast_to(R.GOAL, (63, 3)), np.zeros((63, 3)), 1.0, None, None, c["t"])
        rel_close(U[s], w["u"], 1e-8, what="polar teacher-forced u")
    box = (np.abs(U[..., 0]) >= 10.0 * (1 - 1e-12)) | (np.abs(U[..., 1]) >= 5 * math.pi * (1 - 1e-12))
    assert box.any() and any(m & 0xF for m in ref["actives"])


# ------------------------------------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("k,every", [(150, 1), (149, 7)])
def test_two_launches_equal_one_bit_for_bit(ops, case, dtype, k, every):
    one = dev_rollout(ops, case, dtype=dtype, record_every=every)
    first = dev_rollout(ops, case, steps=k, dtype=dtype, record_every=every)
    second = dev_rollout(ops, case, steps=300 - k, dtype=dtype, record_every=every, t_offset=k,
                         state={n: first[n] for n in ("x", "min_h", "cost", "status", "converged_at")})
    for name in ("x", "min_h", "cost", "status", "converged_at"):
        assert bits(second[name]) == bits(one[name]), name
    for name in ("traj", "u"):
        assert bits(torch.cat([first[name], second[name]])) == bits(one[name]), name
        assert not torch.isnan(one[name]).any()


# ------------------------------------------------------------------------------------------------ 7. freeze
def test_an_infeasible_instance_freezes_and_leaves_its_wave_alone(ops, case):
    Bt, lane = 63, 17
    x0 = case["x0"][:Bt]
    cen = np.broadcast_to(case["centers"], (Bt, 2, 2)).copy()
    rad = np.broadcast_to(case["radii"], (Bt, 2)).copy()
    small = dict(case, x0=x0, x0_plan=case["x0_plan"][:Bt], L_true=case["L_true"][:Bt], centers=cen, radii=rad)
    plain = dev_rollout(ops, small, steps=40, record_every=1)
    cen2, rad2 = cen.copy(), rad.copy()
    cen2[lane, 0], rad2[lane, 0] = x0[lane, :2] + [1e-3, 0.0], 100.0          # an obstacle of radius 100 around the instance
    frozen = dict(small, centers=cen2, radii=rad2)
    got = dev_rollout(ops, frozen, steps=40, record_every=1)
    st = raw(got["status"])
    assert st[lane] == 1 and (np.delete(st, lane) == 0).all()
    assert (raw(got["x"])[lane] == x0[lane]).all() and raw(got["min_h"])[lane] == np.inf and raw(got["cost"])[lane] == 0
    assert (raw(got["u"])[:, lane] == 0).all() and (raw(got["traj"])[:, lane] == x0[lane]).all()
    others = np.arange(Bt) != lane
    for name in ("x", "min_h", "cost", "traj", "u"):
        g, p = raw(got[name]), raw(plain[name])
        sel = (slice(None), others) if g.ndim == 3 else (others,)
        assert g[sel].tobytes() == p[sel].tobytes(), name
    # the status carries the global step; an instance that arrives frozen is left alone
    late = dev_rollout(ops, frozen, steps=5, t_offset=150)
    assert raw(late["status"])[lane] == 151
    again = dev_rollout(ops, frozen, steps=5, t_offset=155, state={n: late[n].clone() for n in ("x", "min_h", "cost", "status", "converged_at")})
    assert raw(again["status"])[lane] == 151 and (raw(again["x"])[lane] == x0[lane]).all()
    assert (raw(again["x"])[others] != raw(late["x"])[others]).any()


# ------------------------------------------------------------------------------------------------ 8. strides and NULLs
def test_shared_and_replicated_parameters_are_bit_equal(ops, case):
    Bt = 130
    shared = dict(case, L_true=12.0)
    a = dev_rollout(ops, shared, steps=60)
    b = dev_rollout(ops, dict(shared, L_true=np.full(Bt, 12.0), centers=np.broadcast_to(case["centers"], (Bt, 2, 2)).copy(),
                              radii=np.broadcast_to(case["radii"], (Bt, 2)).copy()), steps=60)
    f = dict(dtype=torch.float64, device=DEV)
    for name in ("x", "min_h", "cost", "status"):
        assert bits(a[name]) == bits(b[name]), name
    # L_ctrl replicated; one recording buffer alone; zero steps changes nothing
    st = lambda: dict(x=T(case["x0"]), cost=torch.zeros(Bt, **f), status=torch.zeros(Bt, dtype=torch.int32, device=DEV),
                      min_h=torch.full((Bt,), float("inf"), **f))
    kw = dict(dt=case["dt"], planner="piecewise", x0_plan=T(np.broadcast_to(case["x0_plan"], (Bt, 3))), numStepsPlan=300,
              frac_time_to_reach_goal=0.95, L_true=12.0, **task_kw(case["t"], torch.float64, case["centers"], case["radii"]))
    goal = T(np.broadcast_to(case["goal"], (Bt, 3)))
    s1, s2 = st(), st()
    traj = torch.full((60, Bt, 3), float("nan"), **f)
    ops.unicycle_clf_cbf_rollout(s1["x"], goal, s1["cost"], s1["status"], 60, min_h=s1["min_h"], L_ctrl=torch.ones(Bt, **f),
                                 traj=traj, record_every=1, **kw)
    for name in ("x", "min_h", "cost", "status"):
        assert bits(s1[name]) == bits(a[name]), name
    assert not torch.isnan(traj).any() and bits(traj[0]) == bits(T(case["x0"]))
    us = torch.full((9, Bt, 2), float("nan"), **f)
    ops.unicycle_clf_cbf_rollout(s2["x"], goal, s2["cost"], s2["status"], 60, min_h=s2["min_h"], L_ctrl=1.0, u_rec=us,
                                 record_every=7, **kw)
    assert bits(s2["x"]) == bits(a["x"]) and not torch.isnan(us).any()
    before = {n: bits(v) for n, v in s2.items()}
    ops.unicycle_clf_cbf_rollout(s2["x"], goal, s2["cost"], s2["status"], 0, min_h=s2["min_h"], L_ctrl=1.0, t_offset=60, **kw)
    torch.cuda.synchronize()
    assert before == {n: bits(v) for n, v in s2.items()}
    # no obstacles: min_h is not needed and not touched
    s3 = st()
    ops.unicycle_clf_cbf_rollout(s3["x"], goal, s3["cost"], s3["status"], 10, dt=case["dt"], L_ctrl=1.0)
    torch.cuda.synchronize()
    assert (raw(s3["status"]) == 0).all() and (raw(s3["cost"]) > 0).all()


# ------------------------------------------------------------------------------------------------ 9. the facade
def test_facade(ops, case):
    from bayesian_cbf_amd import rollouts
    from bayesian_cbf_amd import unicycle_move_to_pose as U
    f = dict(dtype=torch.float64, device=DEV)
    start, goal = T(R.START), T(R.GOAL)
    x = T(case["x0"])
    obs = lambda a, b: U.obstacles_at_mid_from_start_and_goal(a, b, term_weights=(0.7, 0.3))
    mk = lambda solver: U.ControllerCLF(U.PiecewiseLinearPlanner(start, goal, 300, 0.05, 0.95), coordinate_converter=lambda a, b: a,
                                        dynamics=U.CartesianDynamics(), clf=U.CLFCartesian(Kp=(0.9, 1.5, 0.0)), cbfs=obs(start, goal),
                                        cbf_gammas=[5.0, 5.0], solver=solver, device=DEV)
    default = U.ControllerCLF(U.PiecewiseLinearPlanner(start, goal, 300, 0.05, 0.95), coordinate_converter=lambda a, b: a,
                              dynamics=U.CartesianDynamics(), clf=U.CLFCartesian(Kp=(0.9, 1.5, 0.0)), cbfs=obs(start, goal),
                              cbf_gammas=[5.0, 5.0], device=DEV)
    u_default = default.control(x, 7)                  # before any new code path is touched
    u_ipm, u_exact = mk("ipm").control(x, 7), mk("exact").control(x, 7)
    assert bits(u_default) == bits(u_ipm) and default.solver == "ipm"
    ctrl = mk("exact")
    pl, dp = (v.to(**f).expand(130, 3).contiguous() for v in (ctrl.planner.plan(7), ctrl.planner.dot_plan(7)))
    direct = ops.unicycle_clf_cbf_control(x, pl, dp, **ctrl.exact_task(130))
    rel_close(raw(direct["u"]), R.control(case["x0"], raw(pl), raw(dp), 1.0, case["centers"], case["radii"], case["t"])["u"], 1e-8,
              what="facade against the yardstick")
    assert bits(u_exact) == bits(direct["u"]) and (raw(direct["status"]) == 0).all()
    rel_close(raw(u_exact), raw(u_ipm), 1e-6, what="exact against ipm")
    one = mk("exact").control(x[3], 7)
    assert one.shape == (2,) and bits(one) == bits(u_exact[3])
    X, Uc = U.move_to_pose_clf_polar(start + torch.tensor([0.2, -0.1, 0.3], **f), goal, dt=0.01, max_steps=2000)
    assert X.ndim == 2 and X.shape[1] == 3 and Uc.shape == (X.shape[0] - 1, 2) and 50 < Uc.shape[0] < 2000
    assert float((X[-1, :2] - goal[:2]).norm()) < 1e-3
    Xd, Xs, Us = U.track_trajectory_clf_cartesian(start, goal, dt=0.05, cbfs=obs, cbf_gammas=[5.0, 5.0], numSteps=100)
    assert Xd.shape == (100, 3) and Xs.shape == (101, 3) and Us.shape == (100, 2) and bits(Xs[0]) == bits(start)
    rel_close(raw(Xd), raw((Xs[1:] - Xs[:-1]) / 0.05), 1e-8, what="Xdot")
    Xd, Xs, Us = U.move_to_pose_sample_clf_cartesian(start, goal, dt=0.01)
    assert Xs.shape == (201, 3) and Us.shape == (200, 2)
    X2, U2 = U.move_to_pose_clf_cartesian(start, goal, dt=0.01, max_steps=50)
    assert X2.shape == (51, 3) and U2.shape == (50, 2)
    r1 = rollouts.unicycle_clf_cbf_rollouts(130, numSteps=60, record_every=7)
    r2 = rollouts.unicycle_clf_cbf_rollouts(130, numSteps=60, record_every=7, steps_per_launch=13)
    assert set(r1) == {"stats", "x_final", "min_h", "cost", "status", "converged_at", "dist_to_goal", "traj", "u", "loop_seconds"}
    assert set(r1["stats"]) == {"collisions", "mean_cost", "solver_failures", "count", "min_h"} and r1["stats"]["count"] == 130
    for name in ("x_final", "min_h", "cost", "status", "converged_at", "traj", "u"):
        assert bits(r1[name]) == bits(r2[name]), name
    assert r1["traj"].shape == (9, 130, 3) and r1["u"].shape == (9, 130, 2)
    rp = rollouts.unicycle_clf_cbf_rollouts(64, numSteps=800, dt=0.01, L_true=1.0, planner="none", clf="polar", obstacles=None,
                                            stop_rho=1e-3)
    assert (raw(rp["converged_at"]) > 0).all() and rp["stats"]["solver_failures"] == 0


# ------------------------------------------------------------------------------------------------ 10. what it exists for
def test_a_wrong_model_costs_collisions():
    from bayesian_cbf_amd import rollouts
    matched = rollouts.unicycle_clf_cbf_rollouts(64, L_ctrl=1.0, L_true=1.0)
    wrong = rollouts.unicycle_clf_cbf_rollouts(64, L_ctrl=1.0, L_true=12.0)
    print("collisions: matched %d, L_true = 12: %d of 64" % (matched["stats"]["collisions"], wrong["stats"]["collisions"]))
    assert matched["stats"]["solver_failures"] == 0
    assert wrong["stats"]["collisions"] >= matched["stats"]["collisions"]
