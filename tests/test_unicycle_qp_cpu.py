"""CPU side of the unicycle CLF-CBF quadratic program on the mean model: the yardstick (tests/_unicycle_qp_reference.py) against
the recorded rows of the reference's own classes, its enumerator against oracle.socp.coneqp and scipy's SLSQP, the hand-made
programs, the freedoms the GPU tests rely on, the torch side of the facade, and every BCBF_EINVAL refusal of the three
entries through ctypes (they return before any HIP call, so they run without a GPU)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _unicycle_qp_reference as R
from oracle import socp as osocp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "unicycle_clf_qp_rows.npz")
ENTRIES = ["bcbf_%s_%s" % (e, s) for e in ("clf_cbf_qp2", "unicycle_clf_cbf_control", "unicycle_clf_cbf_rollout")
           for s in ("f32", "f64")]
MARGIN = {np.float64: 1e-9, np.float32: 1e-4}           # the decision margins below which status / active are not compared
MAX_EXCLUDED = 0.05


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _close(got, want, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.maximum(np.abs(want), 1.0)
    assert np.isfinite(want).all()
    assert (np.abs(got - want) <= tol * scale).all(), float((np.abs(got - want) / scale).max())


def golden_rows(g, kind):
    """The yardstick's (a, b, values) at the golden states: kind 'polar', or ('cartesian', index into t_steps)."""
    if kind == "polar":
        t = R.task(Kp=tuple(g["Kp_polar"]), clf_kind=1, clf_gamma=float(g["clf_gamma"]))
        return R.rows(g["x"], g["goal"], np.zeros(3), 1.0, None, None, t)
    i = kind[1]
    t = R.task(Kp=tuple(g["Kp_cart"]) + (0.0,), clf_gamma=float(g["clf_gamma"]), tw=tuple(g["tw"]), gammas=tuple(g["gammas"]))
    return R.rows(g["x"], g["cart_plan"][i], g["cart_dot_plan"][i], 1.0, g["centers"], g["radii"], t)


def test_golden_file_holds_the_states_the_issue_names(golden):
    g = golden
    assert g["x"].shape == (64, 3)
    d = np.linalg.norm(g["x"][:, None, :2] - g["centers"][None], axis=2) / g["radii"]
    assert (np.abs(d - 1) < 1e-12).sum() >= 2 and (d < 0.9).sum() >= 2            # on an obstacle's boundary, inside one
    rho = g["polar"][:, 0]
    assert ((rho > 5e-4) & (rho < 2e-3)).sum() >= 2 and ((rho > 5e-3) & (rho < 2e-2)).sum() >= 2
    assert list(g["t_steps"]) == [0, 7, 150, 195] and int(g["numStepsPlan"]) == 200
    assert float(g["clf_gamma"]) == 10.0 and float(g["clf_relax_weight"]) == 10.0    # the constructor ignores its arguments


def test_polar_rows_equal_the_recorded_reference_rows(golden):
    g = golden
    a, b, v = golden_rows(g, "polar")
    _close(a[:, 0], g["polar_bfa"])
    _close(b[:, 0], g["polar_b"])
    _close(v[:, 0], g["polar_terms"].sum(1))
    for i, x in enumerate(g["x"]):
        polar, V, gV, gm = R.polar_terms(x, g["goal"], tuple(g["Kp_polar"]))
        _close(polar, g["polar"][i])
        _close(gV, g["polar_grad"][i])
        _close(gm, g["polar_g"][i])


@pytest.mark.parametrize("i", range(4))
def test_cartesian_rows_equal_the_recorded_reference_rows(golden, i):
    g = golden
    a, b, v = golden_rows(g, ("cartesian", i))
    _close(a, g["cart_bfa"][i])
    _close(b, g["cart_b"][i])
    _close(g["gammas"][None] * v[:, 1:], g["cart_b"][i][:, 1:])
    import oracle.unicycle as ouni
    P = ouni.PiecewiseLinearPlanner(g["start"], g["goal"], 200, 0.05)
    t = int(g["t_steps"][i])
    _close(P.plan(t), g["cart_plan"][i])
    _close(P.dot_plan(t), g["cart_dot_plan"][i])


def test_torch_facade_functions_equal_the_recorded_reference_values(golden):
    """cartesian2polar, polar2cartesian, CLFPolar and PolarDynamics of the facade, batched on the host."""
    import torch
    from bayesian_cbf_amd import unicycle_move_to_pose as U
    g = golden
    x, goal = torch.tensor(g["x"]), torch.tensor(g["goal"])
    polar = U.cartesian2polar(x, goal)
    _close(polar.numpy(), g["polar"])
    _close(U.polar2cartesian(polar, goal).numpy(), g["polar_back"])
    clf = U.CLFPolar(Kp=tuple(g["Kp_polar"]))
    _close(clf.clf_terms(polar, goal).numpy(), g["polar_terms"])
    _close(clf.grad_clf(polar, goal).numpy(), g["polar_grad"])
    assert not clf.grad_clf_wrt_goal(polar, goal).any()
    _close(U.PolarDynamics().g_func(polar).numpy(), g["polar_g"])
    assert clf.isconverged(x, goal).tolist() == (g["polar"][:, 0] < 1e-3).tolist()
    assert U.CLFCartesian().isconverged(x, goal).tolist() == (g["polar"][:, 0] < 1e-3).tolist()
    with pytest.raises(ValueError, match="exact"):
        U.ControllerCLF(U.NoPlanner(goal), coordinate_converter=U.cartesian2polar, dynamics=U.PolarDynamics(), clf=clf,
                        device="cpu")
    with pytest.raises(ValueError, match="come together"):
        U.ControllerCLF(U.NoPlanner(goal), coordinate_converter=U.cartesian2polar, clf=U.CLFCartesian(), solver="exact",
                        device="cpu")
    with pytest.raises(ValueError, match="solver"):
        U.ControllerCLF(U.NoPlanner(goal), solver="simplex", device="cpu")
    c = U.ControllerCLF(U.NoPlanner(goal), coordinate_converter=U.cartesian2polar, dynamics=U.PolarDynamics(), clf=clf,
                        solver="exact", device="cpu")
    assert c.polar and c.exact_task(4)["clf_kind"] == "polar" and c.clf_gamma == 10.0 and c.clf_relax_weight == 10.0
    assert U.ControllerCLF(U.NoPlanner(goal), device="cpu").solver == "ipm"


# ---------------------------------------------------------------------------------------------- the enumerator
def _coneqp(a, b):
    P, q, G, h, dims = R.coneqp_form(a, b)
    return osocp.coneqp(P, q, G, h, dims)


def _agrees_with_coneqp(a, b, tol=1e-6):
    """One program: both optimal and equal to tol (own-relative), or infeasible here and not optimal there."""
    mine = R.solve_qp2(a[None], b[None])
    sol = _coneqp(a, b)
    if mine["status"][0] != 0:
        assert sol["status"] != "optimal", (a, b)
        return False
    assert sol["status"] == "optimal", (a, b, mine["u"])
    want = np.concatenate([mine["u"][0], mine["relax"]])
    assert (np.abs(sol["x"] - want) <= tol * np.maximum(np.abs(want), 1.0)).all(), (a, b, sol["x"], want)
    return True


def test_enumerator_agrees_with_coneqp_on_random_programs():
    progs = R.random_programs(400)
    feasible = sum(_agrees_with_coneqp(a, b) for a, b in progs)
    assert 40 <= 400 - feasible <= 200              # the set holds infeasible programs, and mostly feasible ones


def test_enumerator_agrees_with_coneqp_on_the_golden_programs(golden):
    n = 0
    for kind in ("polar", ("cartesian", 0), ("cartesian", 1), ("cartesian", 2), ("cartesian", 3)):
        a, b, _ = golden_rows(golden, kind)
        for i in range(64):
            n += _agrees_with_coneqp(a[i], b[i])
    assert n >= 250


def test_enumerator_agrees_with_slsqp():
    from scipy.optimize import minimize
    checked = 0
    for a, b in R.random_programs(120, seed=5):
        mine = R.solve_qp2(a[None], b[None])
        if mine["status"][0] != 0:
            continue
        cons = [dict(type="ineq", fun=lambda y, a=a, b=b: -(a[0] @ y[:2] + b[0] - y[2]))]
        cons += [dict(type="ineq", fun=lambda y, k=k, a=a, b=b: a[k] @ y[:2] + b[k]) for k in range(1, len(b))]
        y0 = np.concatenate([mine["u"][0] * 0.9, mine["relax"] + 1.0])
        res = minimize(lambda y: y[0] ** 2 + y[1] ** 2 + 10.0 * y[2], y0, method="SLSQP", constraints=cons,
                       bounds=[(R.LO[0], R.HI[0]), (R.LO[1], R.HI[1]), (None, None)], options=dict(ftol=1e-14, maxiter=500))
        if not res.success:
            continue
        obj = (mine["u"][0] ** 2).sum() + 10.0 * mine["relax"][0]
        assert res.fun >= obj - 1e-6 * max(1.0, abs(obj)), (a, b)          # nothing feasible is better than the enumerator's
        if abs(res.fun - obj) <= 1e-9 * max(1.0, abs(obj)):
            assert np.abs(res.x[:2] - mine["u"][0]).max() <= 1e-4 * max(1.0, np.abs(mine["u"][0]).max())
            checked += 1
    assert checked >= 15


def test_hand_made_programs():
    out = {}
    for a, b, what in R.hand_programs():
        s = R.solve_qp2(a[None], b[None])
        out[what] = {k: v[0] for k, v in s.items()}
        _agrees_with_coneqp(a, b) if not what.startswith("zero-normal") else None   # (a zero row is degenerate for the IPM)
    o = out["a_c = 0: u = 0"]
    assert o["status"] == 0 and o["active"] == 0 and (o["u"] == 0).all() and o["relax"] == 1.0
    o = out["zero-normal hard row, b > 0: ignored"]
    assert o["status"] == 0 and o["active"] == 0 and np.allclose(o["u"], [-5.0, -10.0]) and np.isclose(o["relax"], -24.5)
    assert out["zero-normal hard row, b < 0: infeasible"]["status"] == 1
    o = out["parallel rows: u0 >= -1 and u0 >= -2"]
    assert o["status"] == 0 and o["active"] == 1 << 4 and np.allclose(o["u"], [-1.0, 0.0])
    assert out["parallel rows, empty strip"]["status"] == 1
    o = out["box corner (hi0, hi1)"]
    assert o["status"] == 0 and o["active"] == (1 << 2) | (1 << 3) and np.allclose(o["u"], R.HI)
    o = out["box corner (lo0, hi1) with a slack hard row"]
    assert o["status"] == 0 and o["active"] == (1 << 0) | (1 << 3) and np.allclose(o["u"], [R.LO[0], R.HI[1]])
    o = out["vertex of two hard rows"]
    assert o["status"] == 0 and o["active"] == (1 << 4) | (1 << 5) and np.allclose(o["u"], [1.0, 0.0])
    bad = R.solve_qp2(np.array([[[np.nan, 0.0]]]), np.array([[0.0]]))
    assert bad["status"][0] == 1 and np.isnan(bad["u"]).all()


# ---------------------------------------------------------------------------------------------- what the GPU tests rely on
def solver_programs():
    """The programs of the GPU solver test, per K: random ones, the hand-made ones and infeasible ones."""
    progs = R.random_programs(600, seed=11) + R.hand_programs()
    return {K: R.pack(progs, K) for K in (1, 2, 3, 4)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_share_of_programs_left_out_of_the_active_comparison(dtype):
    left, total, infeasible = 0, 0, 0
    for K, (a, b) in solver_programs().items():
        a, b = a.astype(dtype).astype(np.float64), b.astype(dtype).astype(np.float64)
        s = R.solve_qp2(a, b, R.LO.astype(dtype).astype(np.float64), R.HI.astype(dtype).astype(np.float64), 10.0,
                        R.EPS[np.dtype(dtype)])
        left += int((s["margin"] <= MARGIN[dtype]).sum())
        total += len(b)
        infeasible += int((s["status"] != 0).sum())
    assert left <= MAX_EXCLUDED * total, (left, total)
    assert infeasible >= 20


def loop_case():
    """The closed loop of the GPU loop tests: 130 starts, 300 steps, the two mid obstacles, every second plant at L = 12."""
    x0 = R.starts(130)
    cen, rad = R.mid_obstacles()
    t = R.task(Kp=R.KP_TRACK, tw=(0.7, 0.3), gammas=(5.0, 5.0))
    L_true = np.where(np.arange(130) % 2 == 1, 12.0, 1.0)
    return dict(x0=x0, goal=R.GOAL, numSteps=300, dt=0.05, L_ctrl=1.0, L_true=L_true, centers=cen, radii=rad, t=t, planner=1,
                x0_plan=np.broadcast_to(R.START, (130, 3)), numStepsPlan=300, frac=0.95)


@pytest.fixture(scope="module")
def loop():
    return R.rollout(record_every=1, **loop_case())


def test_the_loop_of_the_gpu_tests_meets_no_infeasible_step_and_every_kind_of_step(loop):
    assert (loop["status"] == 0).all()
    masks = loop["actives"]
    assert 0 in masks                                               # unconstrained
    assert any(m & 0xF for m in masks)                              # box-active
    assert any(m >> 4 for m in masks)                               # obstacle-active
    assert np.isfinite(loop["x"]).all() and np.isfinite(loop["cost"]).all()


def test_polar_move_to_pose_converges_from_the_starts_of_the_gpu_test():
    x0 = R.starts(16, noise=(0.5, 0.5, 1.0), seed=3)
    out = R.rollout(x0, R.GOAL, 600, dt=0.01, t=R.task(Kp=R.KP_POLAR, clf_kind=1), stop_rho=1e-3)
    assert (out["status"] == 0).all() and (out["converged_at"] > 0).all(), (out["status"], out["converged_at"])
    assert any(m & 0xF for m in out["actives"])


def test_freeze_case_is_infeasible():
    """An obstacle of radius 100 around the instance itself: the polygon is empty."""
    x = R.START[None] + np.array([[0.01, 0.0, 0.0]])
    cen = np.array([[[x[0, 0] + 1e-3, x[0, 1]], [5.0, 5.0]]])
    rad = np.array([[100.0, 0.1]])
    c = R.control(x, R.GOAL[None], np.zeros((1, 3)), 1.0, cen, rad, R.task(tw=(0.7, 0.3), gammas=(5.0, 5.0)))
    assert c["status"][0] == 1 and c["b"][0, 1] < -1e4


# ---------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


def test_symbols_are_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRIES:
        assert name in declared and name in exported and name in lib.declared_symbols(), name


def test_rollout_kernels_are_under_the_scratch_guard():
    from bayesian_cbf_amd import build
    assert "unicycle_qp.hip" in build.SOURCES
    guard = build.ZERO_SCRATCH_KERNELS["unicycle_qp.hip"]
    assert len(guard) == 10 and all("unicycle_clf_cbf_rollout_kernel" in k for k in guard)
    assert "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["unicycle_qp.hip"]


FAKE = [ctypes.c_void_p(4096 * (k + 1)) for k in range(20)]
GOOD = dict(Bt=64, K=3, Kob=2, numSteps=10, dt=0.05, relax_weight=10.0, clf_gamma=10.0, clf_kind=0, L_stride=0, Lt_stride=1,
            obs_stride=0, planner=1, t2=95, lookahead=10, numStepsPlan=100, stop_rho=0.0, record_every=1, t_offset=0, null=(),
            host_null=(), lo=(-10.0, -5 * math.pi), hi=(10.0, 5 * math.pi))


def _call(lib, entry, suf, a):
    ct = ctypes.c_float if suf == "f32" else ctypes.c_double
    p = [None if k in a["null"] else FAKE[k] for k in range(20)]
    host = dict(lo=(ct * 2)(*a["lo"]), hi=(ct * 2)(*a["hi"]), Kp=(ct * 4)(0.9, 1.5, 4.0, 0.0), tw=(ct * 2)(0.7, 0.3),
                gammas=(ct * 3)(5.0, 5.0, 5.0))
    host = {k: (None if k in a["host_null"] else v) for k, v in host.items()}
    fn = getattr(lib.lib, "bcbf_%s_%s" % (entry, suf))
    if entry == "clf_cbf_qp2":               # pointers: 0 a, 1 b, 2 u, 3 relax, 4 active, 5 status
        return fn(p[0], p[1], host["lo"], host["hi"], a["relax_weight"], p[2], p[3], p[4], p[5], a["Bt"], a["K"], None)
    if entry == "unicycle_clf_cbf_control":
        # pointers: 0 x, 1 plan, 2 dot_plan, 3 L_ctrl, 4 centers, 5 radii, 6 a, 7 b, 8 values, 9 u, 10 relax, 11 active, 12 status
        return fn(p[0], p[1], p[2], host["Kp"], a["clf_kind"], a["clf_gamma"], a["relax_weight"], host["lo"], host["hi"], p[3],
                  a["L_stride"], p[4], p[5], a["obs_stride"], host["tw"], host["gammas"], p[6], p[7], p[8], p[9], p[10], p[11],
                  p[12], a["Bt"], a["Kob"], None)
    # pointers: 0 x, 1 goal, 2 x0_plan, 3 L_ctrl, 4 L_true, 5 centers, 6 radii, 7 min_h, 8 cost, 9 status, 10 converged_at,
    #           11 traj, 12 u_rec
    return fn(p[0], p[1], p[2], a["planner"], a["t2"], a["lookahead"], a["numStepsPlan"], host["Kp"], a["clf_kind"],
              a["clf_gamma"], a["relax_weight"], host["lo"], host["hi"], p[3], a["L_stride"], p[4], a["Lt_stride"], p[5], p[6],
              a["obs_stride"], host["tw"], host["gammas"], a["dt"], a["stop_rho"], p[7], p[8], p[9], p[10], p[11], p[12],
              a["record_every"], a["t_offset"], a["numSteps"], a["Bt"], a["Kob"], None)


BAD_BOX = [(dict(Bt=0), "Bt <= 0"), (dict(Bt=-3), "Bt <= 0"), (dict(relax_weight=0.0), "relax_weight"),
           (dict(relax_weight=-1.0), "relax_weight"), (dict(relax_weight=math.nan), "relax_weight"),
           (dict(relax_weight=math.inf), "relax_weight"), (dict(host_null=("lo",)), "null lo or hi"),
           (dict(host_null=("hi",)), "null lo or hi"), (dict(lo=(-math.inf, 0.0)), "finite"), (dict(hi=(1.0, math.nan)), "finite")]
BAD_QP2 = [(dict(K=0), "K must be"), (dict(K=5), "K must be"), (dict(null=(0,)), "null a or b"), (dict(null=(1,)), "null a or b")]
BAD_TASK = [(dict(Kob=-1), "Kob"), (dict(Kob=4), "Kob"), (dict(clf_kind=2), "clf_kind"), (dict(clf_kind=-1), "clf_kind"),
            (dict(clf_kind=1), "takes no obstacles"), (dict(host_null=("Kp",)), "null Kp"), (dict(clf_gamma=math.nan), "clf_gamma"),
            (dict(L_stride=2), "L_ctrl stride"), (dict(L_stride=-1), "L_ctrl stride"), (dict(obs_stride=3), "obstacle stride"),
            (dict(host_null=("tw",)), "null centers"), (dict(host_null=("gammas",)), "null centers")]
BAD_CONTROL = [(dict(null=(0,)), "null x"), (dict(null=(1,)), "null x"), (dict(null=(2,)), "null x"), (dict(null=(3,)), "null L_ctrl"),
               (dict(null=(4,)), "null centers"), (dict(null=(5,)), "null centers")]
BAD_ROLLOUT = [(dict(numSteps=-1), "numSteps < 0"), (dict(t_offset=-1), "t_offset"), (dict(t_offset=0x7fffffff, numSteps=5), "t_offset"),
               (dict(dt=0.0), "dt"), (dict(dt=-0.05), "dt"), (dict(dt=math.nan), "dt"), (dict(dt=math.inf), "dt"),
               (dict(stop_rho=-1e-3), "stop_rho"), (dict(stop_rho=math.nan), "stop_rho"),
               (dict(stop_rho=1e-3, null=(10,)), "converged_at"), (dict(null=(0,)), "null x"), (dict(null=(1,)), "null x"),
               (dict(null=(8,)), "null x"), (dict(null=(9,)), "null x"), (dict(null=(7,)), "null min_h"),
               (dict(null=(3,)), "null L_ctrl"), (dict(null=(4,)), "null L_true"), (dict(null=(5,)), "null centers"),
               (dict(null=(6,)), "null centers"), (dict(Lt_stride=2), "L_true stride"), (dict(planner=2), "planner kind"),
               (dict(planner=-1), "planner kind"), (dict(null=(2,)), "x0_plan"), (dict(numStepsPlan=2, t2=1, lookahead=1), "numStepsPlan"),
               (dict(t2=100), "numStepsPlan"), (dict(t2=-1), "numStepsPlan"), (dict(lookahead=0), "numStepsPlan"),
               (dict(record_every=0), "record_every"), (dict(record_every=-2, null=(11,)), "record_every"),
               (dict(record_every=0, null=(12,)), "record_every")]
BAD = ([("clf_cbf_qp2", c, w) for c, w in BAD_BOX + BAD_QP2]
       + [("unicycle_clf_cbf_control", c, w) for c, w in BAD_BOX + BAD_TASK + BAD_CONTROL]
       + [("unicycle_clf_cbf_rollout", c, w) for c, w in BAD_BOX + BAD_TASK + BAD_ROLLOUT])


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry,change,why", BAD, ids=["%s-%d" % (e, i) for i, (e, c, w) in enumerate(BAD)])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, entry, change, why):
    """Every case fails the host check, so the made-up pointers are never used and no GPU is touched."""
    rc = _call(lib, entry, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_%s_%s" % (entry, suf)) and why in msg, msg


def test_ops_refuse_cpu_tensors_and_bad_shapes(lib):
    import torch
    from bayesian_cbf_amd import ops
    x = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.clf_cbf_qp2(torch.zeros(4, 2, 2, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.unicycle_clf_cbf_control(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.unicycle_clf_cbf_rollout(x, x, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32), 10)
    assert [ops.unicycle_clf_cbf_records(t0, n, e) for t0, n, e in ((0, 300, 1), (0, 7, 3), (150, 150, 1), (149, 151, 7), (0, 9, 0))] \
        == [300, 3, 150, 21, 0]
    assert ops.unicycle_planner_steps(300, 0.95) == R.planner_steps(300, 0.95) == (285, 30)
    assert ops.unicycle_planner_steps(3, 0.7) == (2, 1)
