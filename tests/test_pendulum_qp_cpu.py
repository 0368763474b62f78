"""CPU-side checks of the pendulum CLF-CBF quadratic program (bcbf_pendulum_clf_cbf_control_*, bcbf_pendulum_clf_cbf_rollout_*):
the yardstick the GPU tests hold the device to (tests/_pendulum_qp_reference.py) reproduces the rows recorded from the
reference's own classes, its generic active-set enumerator agrees with scipy's SLSQP and satisfies the KKT conditions, its
closed loop reproduces the facts the GPU tests rely on, and the C ABI refuses every bad argument before any HIP call.

The reference solves this program with cvxopt, which is not available here: parity with cvxopt's iterates is not claimed.
The program is strictly convex, so its optimum is unique; SLSQP (to its own accuracy) and the KKT conditions (to rounding)
pin that optimum."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _pendulum_qp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "pendulum_clf_cbf_rows.npz"))
ENTRIES = tuple("bcbf_pendulum_clf_cbf_%s_%s" % (e, s) for e in ("control", "rollout") for s in ("f32", "f64"))


def golden_task(**over):
    g = GOLDEN
    return R.task(clf_c=float(g["clf_c"]), k_alpha=tuple(g["k_alpha"]), theta_c=float(g["theta_c"]), delta_c=float(g["delta_c"]),
                  cbf_gamma=float(g["cbf_gamma"]), **over)


# ---------------------------------------------------------------------------------------------- rows against the reference
@pytest.mark.parametrize("kind,name", [(0, "cbf2"), (1, "cbf1")])
def test_oracle_rows_equal_the_recorded_reference_rows(kind, name):
    g = GOLDEN
    assert g["x"].shape == (64, 2) and tuple(g["model"]) == (1.0, 10.0, 1.0)
    A, b, v = R.rows(g["x"], g["model"], golden_task(cbf_kind=kind))
    for got, key in ((A[:, 0], "clf_A"), (b[:, 0], "clf_b"), (v[:, 0], "clf_value"), (A[:, 1], name + "_A"),
                     (b[:, 1], name + "_b"), (v[:, 1], name + "_value")):
        np.testing.assert_allclose(got, g[key], rtol=0, atol=1e-12 * max(1.0, np.abs(g[key]).max()), err_msg=key)


def test_golden_states_hold_the_cases_the_gpu_tests_need():
    g = GOLDEN
    A, b, _ = R.rows(g["x"], g["model"], golden_task())
    at_c = g["x"][:, 0] == float(g["theta_c"])
    assert at_c.sum() == 2 and np.all(A[at_c, 1] == 0) and sorted(np.sign(b[at_c, 1])) == [-1, 1]      # a1 == 0: b1 < 0 and b1 > 0
    assert (g["x"][:, 0] == 3 * math.pi / 8).sum() == 3 and (g["x"][:, 1] == 0).sum() >= 5


# ---------------------------------------------------------------------------------------------- the enumerator
def _programs():
    """The golden rows of both barriers (feasible ones) and 200 random feasible programs with slack weights in [1, 100]."""
    g = GOLDEN
    As, bs, ws = [], [], []
    for kind in (0, 1):
        A, b, _ = R.rows(g["x"], g["model"], golden_task(cbf_kind=kind))
        keep = ~((A[:, 1] == 0) & (b[:, 1] < 0))
        As.append(A[keep]), bs.append(b[keep]), ws.append(np.full(keep.sum(), 100.0))
    rng = np.random.default_rng(11)
    As.append(3 * rng.standard_normal((200, 2)))
    bs.append(5 * rng.standard_normal((200, 2)))
    ws.append(np.where(rng.random(200) < 0.5, 100.0, rng.uniform(1.0, 100.0, 200)))
    return np.concatenate(As), np.concatenate(bs), np.concatenate(ws)


def _solve_each(A, b, w):
    out = [R.solve_qp(*R.program(A[i:i + 1], b[i:i + 1], w[i])) for i in range(len(w))]
    return (np.concatenate([o[k] for o in out]) for k in range(3))


def test_enumerator_agrees_with_slsqp():
    """scipy.optimize.minimize(method='SLSQP') on every program, started at a feasible point; held to SLSQP's own accuracy,
    1e-6 relative to max(1, |u|).  With ftol = 1e-13 SLSQP ends about a quarter of the programs with status 8 ("positive
    directional derivative for linesearch"): its line search finds no further descent at rounding level, which is convergence,
    not failure; a looser ftol that always ends with status 0 leaves it 2e-5 away from the optimum.  Measured worst: 4e-8."""
    from scipy.optimize import minimize
    A, b, w = _programs()
    z, _, status = _solve_each(A, b, w)
    assert len(w) >= 320 and np.all(status == 0)
    worst = 0.0
    for i in range(len(w)):
        a0, a1, b0, b1 = A[i, 0], A[i, 1], b[i, 0], b[i, 1]
        u0 = 0.0 if a1 == 0 else (b1 - 1.0) / a1
        start = np.array([u0, max(0.0, a0 * u0 - b0) + 1.0])
        res = minimize(lambda v: 0.5 * (v[0] ** 2 + w[i] * v[1] ** 2), start, jac=lambda v: np.array([v[0], w[i] * v[1]]),
                       method="SLSQP", options=dict(ftol=1e-13, maxiter=500),
                       constraints=[dict(type="ineq", fun=lambda v: b0 - a0 * v[0] + v[1], jac=lambda v: np.array([-a0, 1.0])),
                                    dict(type="ineq", fun=lambda v: b1 - a1 * v[0], jac=lambda v: np.array([-a1, 0.0]))])
        assert res.status in (0, 8), (i, res.message)
        err = abs(res.x[0] - z[i, 0]) / max(1.0, abs(z[i, 0]))
        worst = max(worst, err)
        assert err <= 1e-6, (i, res.x, z[i], A[i], b[i], w[i])
    print("enumerator vs SLSQP: worst |du| / max(1, |u|) = %.3e over %d programs" % (worst, len(w)))


def test_enumerator_satisfies_the_kkt_conditions():
    """Stationarity P z + G' lam = 0 and complementarity lam_i (G z - h)_i = 0 to 1e-12 (relative to the magnitudes of their
    own terms), primal feasibility and lam >= 0."""
    A, b, w = _programs()
    z, lam, status = _solve_each(A, b, w)
    assert np.all(status == 0)
    for i in range(len(w)):
        P, G, h = R.program(A[i:i + 1], b[i:i + 1], w[i])
        G, h = G[0], h[0]
        stat = P @ z[i] + G.T @ lam[i]
        stat_scale = np.maximum(1.0, np.abs(P @ z[i]) + np.abs(G.T) @ np.abs(lam[i]))
        assert np.all(np.abs(stat) <= 1e-12 * stat_scale), (i, stat)
        slack = G @ z[i] - h
        mag = np.maximum(1.0, np.abs(h) + np.abs(G) @ np.abs(z[i]))
        assert np.all(np.abs(lam[i] * slack) <= 1e-12 * np.maximum(1.0, np.abs(lam[i])) * mag), (i, lam[i], slack)
        assert np.all(slack <= 1e-12 * mag) and np.all(lam[i] >= -1e-9 * np.maximum(1.0, np.abs(lam[i]).max())), (i, slack, lam[i])


def test_infeasible_exactly_when_the_hard_row_has_no_coefficient_and_a_negative_bound():
    w = 100.0
    cases = [((1.0, 0.0), (-2.0, -1e-300), 1), ((1.0, 0.0), (-2.0, -0.0761), 1), ((0.0, 0.0), (3.0, -1.0), 1),
             ((1.0, 0.0), (-2.0, 0.0), 0), ((1.0, 0.0), (-2.0, 5.0), 0), ((1.0, 1e-8), (-2.0, -5.0), 0),
             ((1.0, -1e-8), (-2.0, -5.0), 0), ((0.0, 2.0), (-1.0, -3.0), 0), ((-4.0, 0.5), (1.0, 1.0), 0)]
    for A, b, want in cases:
        z, _, st = R.solve_qp(*R.program(np.array([A]), np.array([b]), w))
        assert st[0] == want, (A, b, st)
        assert np.all(np.isfinite(z[0])) == (want == 0)
    g = GOLDEN
    A, b, _ = R.rows(g["x"], g["model"], golden_task())
    c = R.control(g["x"], g["model"], golden_task())
    assert np.array_equal(c["status"] != 0, (A[:, 1] == 0) & (b[:, 1] < 0)) and c["status"].sum() == 1


# ---------------------------------------------------------------------------------------------- the closed loop
def test_nominal_run_settles_on_the_boundary_of_the_safe_set():
    """run_pendulum_control_cbf_clf's own run (theta0 = 5 pi / 12, omega0 = -0.01, tau = 0.002, 15 000 steps): ends at
    theta = 3 pi / 8 to 1e-5, min_h >= 0, no infeasible step."""
    r = R.rollout([[5 * math.pi / 12, -0.01]], (1.0, 10.0, 1.0), (1.0, 10.0, 1.0), 15000)
    assert r["status"][0] == 0 and r["min_h"][0] >= 0
    assert abs(r["x"][0, 0] - 3 * math.pi / 8) <= 1e-5, r["x"]
    print("nominal run: theta - 3 pi/8 = %.3e, omega = %.3e, min_h = %.3e" % (r["x"][0, 0] - 3 * math.pi / 8, r["x"][0, 1], r["min_h"][0]))


def test_the_starts_of_the_gpu_tests_never_meet_an_infeasible_step():
    """130 starts, noise 0.05, seed 0, 300 steps, matched plant and the half-mismatched plants of the teacher-forced GPU test:
    zero infeasible steps, so that test compares every instance."""
    x0 = R.starts(130)
    assert R.rollout(x0, (1.0, 10.0, 1.0), (1.0, 10.0, 1.0), 300)["status"].max() == 0
    r = R.rollout(R.loop_starts(130), (1.0, 10.0, 1.0), R_half_mismatched(130), 300)
    assert r["status"].max() == 0 and r["damage"].max() > 0 and (r["min_h"] < 0).any() and np.abs(r["x"][:, 0]).max() < 3.0


def R_half_mismatched(Bt):
    true = np.tile([1.0, 10.0, 1.0], (Bt, 1))
    true[1::2] = [2.0, 10.0, 0.5]
    return true


def test_recording_and_freeze_rules_of_the_loop():
    x0 = np.array([[5 * math.pi / 12, -0.01], [math.pi / 4, 0.0]])
    r = R.rollout(x0, (1.0, 10.0, 1.0), (1.0, 10.0, 1.0), 7, record_every=3)
    assert r["traj"].shape == (3, 2, 2) and r["u"].shape == (3, 2)
    assert r["status"].tolist() == [0, 1] and np.array_equal(r["x"][1], x0[1]) and r["min_h"][1] == np.inf and r["damage"][1] == 0
    assert np.array_equal(r["traj"][0], x0) and np.all(r["u"][:, 1] == 0)


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


def test_rollout_kernel_is_under_the_scratch_guard():
    from bayesian_cbf_amd import build
    assert "pendulum_qp.hip" in build.SOURCES
    assert any("pendulum_clf_cbf_rollout_kernel" in k for k in build.ZERO_SCRATCH_KERNELS["pendulum_qp.hip"])


FAKE = [ctypes.c_void_p(4096 * (k + 1)) for k in range(12)]
GOOD = dict(Bt=64, numSteps=10, dt=0.002, slack_weight=100.0, ctrl_stride=0, true_stride=3, cbf_kind=0, record_every=1,
            t_offset=0, null=(), k_alpha=True)


def _call(lib, entry, suf, a):
    ct = ctypes.c_float if suf == "f32" else ctypes.c_double
    p = [None if k in a["null"] else FAKE[k] for k in range(12)]
    ka = (ct * 2)(1.0, 3.0) if a["k_alpha"] else None
    fn = getattr(lib.lib, "bcbf_pendulum_clf_cbf_%s_%s" % (entry, suf))
    if entry == "control":        # pointers: 0 x, 1 ctrl_params, 2 A, 3 b, 4 values, 5 u, 6 rho, 7 status
        return fn(p[0], p[1], a["ctrl_stride"], 1.0, ka, math.pi / 4, math.pi / 8, 1.0, a["cbf_kind"], a["slack_weight"],
                  p[2], p[3], p[4], p[5], p[6], p[7], a["Bt"], None)
    # pointers: 0 x, 1 ctrl_params, 2 true_params, 3 min_h, 4 damage, 5 status, 6 traj, 7 u_rec
    return fn(p[0], p[1], a["ctrl_stride"], p[2], a["true_stride"], 1.0, ka, math.pi / 4, math.pi / 8, 1.0, a["cbf_kind"],
              a["slack_weight"], a["dt"], p[3], p[4], p[5], p[6], p[7], a["record_every"], a["t_offset"], a["numSteps"],
              a["Bt"], None)


BAD_BOTH = [(dict(Bt=0), "Bt <= 0"), (dict(Bt=-3), "Bt <= 0"), (dict(slack_weight=0.0), "slack_weight"),
            (dict(slack_weight=-1.0), "slack_weight"), (dict(slack_weight=math.nan), "slack_weight"),
            (dict(ctrl_stride=1), "ctrl_stride"), (dict(ctrl_stride=-3), "ctrl_stride"), (dict(cbf_kind=2), "cbf_kind"),
            (dict(cbf_kind=-1), "cbf_kind"), (dict(null=(0,)), "null"), (dict(null=(1,)), "null"), (dict(k_alpha=False), "k_alpha")]
BAD_ROLLOUT = [(dict(numSteps=-1), "numSteps < 0"), (dict(dt=0.0), "dt"), (dict(dt=-0.002), "dt"), (dict(dt=math.nan), "dt"),
               (dict(true_stride=2), "true_stride"), (dict(record_every=0), "record_every"),
               (dict(record_every=-2, null=(6,)), "record_every"), (dict(record_every=0, null=(7,)), "record_every"),
               (dict(t_offset=-1), "t_offset"), (dict(null=(2,)), "null"), (dict(null=(3,)), "null"), (dict(null=(4,)), "null"),
               (dict(null=(5,)), "null")]
BAD = [("control", c, w) for c, w in BAD_BOTH] + [("rollout", c, w) for c, w in BAD_BOTH + BAD_ROLLOUT]


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry,change,why", BAD, ids=["%s-%d" % (e, i) for i, (e, c, w) in enumerate(BAD)])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, entry, change, why):
    """Every case fails the host check, so the made-up pointers are never used and no GPU is touched."""
    rc = _call(lib, entry, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_pendulum_clf_cbf_%s_%s" % (entry, suf)) and why in msg, msg


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry,change", [("control", dict()), ("control", dict(null=(2, 3, 4, 5, 6, 7), ctrl_stride=3)),
                                          ("rollout", dict()), ("rollout", dict(null=(6, 7), record_every=0, numSteps=0)),
                                          ("rollout", dict(cbf_kind=1, true_stride=0, t_offset=150, null=(7,)))],
                         ids=["control", "control-no-outputs", "rollout", "rollout-no-recording", "rollout-radial-offset"])
def test_a_valid_call_passes_the_checks_and_fails_at_the_launch_without_a_gpu(lib, suf, entry, change):
    """Without a device the launch fails: BCBF_ELAUNCH and HIP's message.  Not run where a GPU is present: a launch on these
    made-up pointers must never reach one."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the valid call on made-up pointers is only made where the launch cannot happen")
    rc = _call(lib, entry, suf, dict(GOOD, **change))
    assert rc == -2, (rc, lib.lib.bcbf_last_error().decode())                      # BCBF_ELAUNCH
    assert lib.lib.bcbf_last_error().decode().startswith("bcbf_pendulum_clf_cbf_%s_%s" % (entry, suf))


def test_ops_refuse_cpu_tensors(lib):
    import torch
    from bayesian_cbf_amd import ops
    x = torch.zeros(4, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pendulum_clf_cbf_control(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pendulum_clf_cbf_rollout(x, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32),
                                     torch.zeros(4, dtype=torch.int32), 10)
    assert [ops.pendulum_clf_cbf_records(t0, n, e) for t0, n, e in ((0, 300, 1), (0, 7, 3), (150, 150, 1), (4, 5, 3), (3, 1, 3), (0, 9, 0))] \
        == [300, 3, 150, 1, 1, 0]
