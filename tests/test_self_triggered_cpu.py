"""CPU-side checks of the self-triggered loop's event (bcbf_unicycle_trigger_step): the numpy yardstick
tests/_trigger_step_reference.py against the results the reference recorded for its committed learning run, the clamp rules and the
planner-row index on hand-made cases, and the entry's argument checks (refused before any HIP call)."""
import ctypes
import math
import os

import numpy as np
import pytest

import _trigger_reference as R
import _trigger_step_reference as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


def test_event_reference_reproduces_the_recorded_run(lib):
    """The event yardstick fed the committed log -- the state, the control, the kernel parameters, and the model's logged one-step
    prediction as its velocity (fhat = (xtp1 - x) / dt, ghat = M_k = 0) -- against the reference's Lfh.np.txt / tau.np.txt /
    xvel.np.txt: 1e-6 relative, the bound tests/test_trigger_interval_cpu.py holds the plain yardstick to (the float32 log bounds it).
    Every 8th step (the pair loop of the yardstick is brute force)."""
    G = np.load(os.path.join(GOLDEN, "saved_run_learning_v1p6p3.npz"))
    F = np.load(os.path.join(GOLDEN, "trigger_interval_v1p6p3.npz"))
    off, dt = R.grid(), 0.01
    r = R.whole_norm(off)
    obs = R.default_obstacles()
    centers, tw = [c for c, _, _ in obs], obs[0][2]
    plan_all = np.arange(12.0).reshape(4, 3)
    worst = dict(Lfh=0.0, tau=0.0, xvel=0.0)
    for s in range(0, 200, 8):
        g = lambda k: G[k][s].astype(np.float64)
        x = g("state")
        ev = S.event(x, g("uopt"), 0, (g("xtp1") - x) / dt, np.zeros((3, 2)), np.zeros((3, 3)), centers, tw, off, r, g("knl_lengthscale"),
                     float(G["knl_scalefactor"][s]), np.diag(g("knl_A")), g("knl_B"), 0.0, 0, plan_all, plan_all, 0.05, 1.0, 1e-6, 1.0,
                     1.0)
        for k in worst:
            worst[k] = max(worst[k], abs(ev[k] - F[k][s]) / abs(F[k][s]))
        assert ev["dt_used"] == ev["tau"] and ev["events"] == 1                  # interior: tau itself is held
    print("worst relative errors against the recorded run:", worst)
    for k, e in worst.items():
        assert e <= 1e-6, (k, e)


def test_clamp_rules():
    tmin, tmax, tend = 1e-3, 0.05, 2.0
    h = lambda tau, solved=True, t=0.5: S.hold_time(tau, solved, t, tend, tmin, tmax)
    assert h(0.01) == (0.01, False)                          # interior
    assert h(1e-5) == (tmin, False) and h(0.3) == (tmax, False)
    assert h(math.inf) == (tmax, False)
    assert h(math.nan) == (tmin, False) and h(0.0) == (tmin, False) and h(-1.0) == (tmin, False) and h(-math.inf) == (tmin, False)
    assert h(1e-5, solved=False) == (tmax, False) and h(math.nan, solved=False) == (tmax, False)     # unsolved: tau_max passes
    # the last, partial step lands on t_end
    assert h(0.01, t=tend - 0.004) == (tend - (tend - 0.004), True)
    assert h(math.inf, t=tend - 0.004)[1] and h(0.3, solved=False, t=tend - 0.004)[1]
    left = tend - (tend - 0.004)
    assert h(left, t=tend - 0.004) == (left, True)                               # exactly the remainder counts as the last step
    assert h(1e-5, t=tend - 0.004) == (tmin, False)


def test_event_acts_on_the_clamped_time_and_moves_the_clock():
    off = np.random.default_rng(0).normal(size=(5, 3)) * 0.05
    r = R.whole_norm(off)
    P = 7
    plan_all, dplan_all = np.arange(3.0 * P).reshape(P, 3), -np.arange(3.0 * P).reshape(P, 3)
    x, u = np.array([-2.9, -0.8, 0.3]), np.array([0.7, -0.4])
    common = dict(fhat=np.zeros(3), ghat=np.array([[math.cos(0.3), 0], [math.sin(0.3), 0], [0, 0.25]]), Mk=0.01 * np.ones((3, 3)),
                  centers=[np.array([-4.0, -2.0])], tw=(0.7, 0.3), off=off, r=r, ls=np.array([0.3, 0.4, 0.5]), sf=0.9,
                  Adiag=np.array([0.01, 0.02, 0.03]), Bhyp=np.eye(3), plan_all=plan_all, dplan_all=dplan_all, dt_plan=0.05, L_true=12.0)
    ev = S.event(x, u, 0, t=0.12, events=3, t_end=1.0, tau_min=1e-6, tau_max=10.0, **common)
    assert 1e-6 < ev["tau"] < 10.0 and ev["dt_used"] == ev["tau"] and not ev["last"]
    np.testing.assert_allclose(ev["x"], x + np.array([math.cos(0.3) * 0.7, math.sin(0.3) * 0.7, -0.4 / 12.0]) * ev["tau"], rtol=1e-15)
    assert ev["t"] == 0.12 + ev["tau"] and ev["events"] == 4
    assert abs(ev["uBu"] - (1 + 0.49 + 0.16)) <= 1e-15
    v = common["ghat"] @ u + common["Mk"] @ np.r_[1.0, u]
    assert abs(ev["xvel"] - np.linalg.norm(v)) <= 1e-15
    assert ev["row"] == S.plan_row(ev["t"], 0.05, P) and np.array_equal(ev["plan"], plan_all[ev["row"]])
    # unsolved: the state is kept, tau_max passes, the event counts
    un = S.event(x, u, 2, t=0.12, events=3, t_end=1.0, tau_min=1e-6, tau_max=0.2, **common)
    assert np.array_equal(un["x"], x) and un["dt_used"] == 0.2 and un["events"] == 4 and un["tau"] == ev["tau"]
    # clamped low / high
    assert S.event(x, u, 0, t=0.12, events=0, t_end=1.0, tau_min=0.5, tau_max=0.6, **common)["dt_used"] == 0.5
    assert S.event(x, u, 0, t=0.12, events=0, t_end=1.0, tau_min=1e-9, tau_max=1e-8, **common)["dt_used"] == 1e-8
    # the remainder to t_end, and the clock lands on it
    la = S.event(x, u, 0, t=0.12, events=0, t_end=0.12 + ev["tau"] / 2, tau_min=1e-6, tau_max=10.0, **common)
    assert la["last"] and la["t"] == 0.12 + ev["tau"] / 2 and la["dt_used"] == la["t"] - 0.12
    # finished: nothing
    assert S.event(x, u, 0, t=1.0, events=9, t_end=1.0, tau_min=1e-6, tau_max=10.0, **common) is None
    # a still control: xvel = 0 gives tau = inf, held for tau_max
    still = dict(common, ghat=np.zeros((3, 2)), Mk=np.zeros((3, 3)))
    with np.errstate(divide="ignore"):
        st = S.event(x, np.zeros(2), 0, t=0.0, events=0, t_end=1.0, tau_min=1e-6, tau_max=0.25, **still)
    assert st["tau"] == math.inf and st["dt_used"] == 0.25


def test_plan_row_index():
    assert S.plan_row(0.0, 0.05, 10) == 0 and S.plan_row(0.049, 0.05, 10) == 0 and S.plan_row(0.051, 0.05, 10) == 1
    assert S.plan_row(0.26, 0.05, 10) == 5 and S.plan_row(0.5, 0.05, 10) == 9 and S.plan_row(7.0, 0.05, 10) == 9     # clamped at P - 1
    assert S.plan_row(3.0, 0.05, 1) == 0
    assert S.plan_row(0.15, 0.05, 10) == int(math.floor(0.15 / 0.05))          # the floor of the floating-point quotient, as stated


# ------------------------------------------------------------------------------------------------ the entry's argument checks
NPTR = 35
GOOD = dict(Bt=5, Bh=5, Kob=2, Nte=64, P=10, tau_min=1e-3, tau_max=0.05, dt_plan=0.05)
BAD = [(dict(null=0), "null control-step buffer"), (dict(null=5), "null control-step buffer"), (dict(null=6), "null input pointer"),
       (dict(null=8), "null input pointer"), (dict(null=9), "null hyper-parameter"), (dict(null=12), "null hyper-parameter"),
       (dict(null=13), "null planner table"), (dict(null=15), "null in/out"), (dict(null=18), "null in/out"),
       (dict(Bh=2), "Bh must be 1 or Bt"), (dict(Bt=0, Bh=0), "Bt < 1"), (dict(Nte=0), "Nte < 1"), (dict(Nte=1 << 20), "Nte too large"),
       (dict(Kob=0), "Kob"), (dict(Kob=8), "Kob"), (dict(P=0), "P < 1"), (dict(tau_min=0.1), "tau_min > tau_max"),
       (dict(tau_min=0.0), "tau_min must be positive"), (dict(tau_max=math.inf), "tau_max must be finite"),
       (dict(dt_plan=0.0), "dt_plan must be positive")]


def _call(lib, suf, a):
    """The entry on fake pointers: position 0-5 the control step's, 6-8 centers / tw / off, 9-12 the hyper-parameters, 13-14 the
    planner tables, 15-18 t / events / plan / dot_plan, 19-25 the optional outputs."""
    ptr = [ctypes.c_void_p(4096 * (k + 1)) for k in range(NPTR)]
    if "null" in a:
        ptr[a["null"]] = None
    fn = getattr(lib.lib, "bcbf_unicycle_trigger_step" + suf)
    return fn(*ptr[:9], 96.4, *ptr[9:13], 1e-4, 1e-2, 1.0, a["tau_min"], a["tau_max"], 10.0, 12.0, ptr[13], ptr[14], a["dt_plan"],
              *ptr[15:26], a["Bt"], a["Bh"], a["Kob"], a["Nte"], a["P"], None)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("change,why", BAD, ids=["%s-%s" % (w.split(" (")[0].replace(" ", "_"), "-".join("%s%s" % kv for kv in c.items()))
                                                 for c, w in BAD])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, change, why):
    """Every case fails the host check, so the fake pointers are never used and no GPU is touched."""
    rc = _call(lib, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_unicycle_trigger_step" + suf) and why in msg, msg


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bcbf.h")).read()
    for name in ("bcbf_unicycle_trigger_step_f32", "bcbf_unicycle_trigger_step_f64"):
        assert name + "(" in header and name in lib.declared_symbols() and hasattr(lib.lib, name)


def test_loop_refuses_a_fixed_kernel_model_without_hyper_parameters_and_other_kernels(lib):
    import torch
    from bayesian_cbf_amd import ops, rollouts
    with pytest.raises(ValueError, match="trigger_hyper"):
        rollouts.self_triggered_rollouts(4, horizon=1.0, device="cpu")
    hyper = dict(ls=[1.0, 1.0, 1.0], sf=1.0, A=np.eye(3), B=np.eye(3))
    for kind in ("matern52", "rbf_matern52"):
        with pytest.raises(ValueError, match="RBF data kernel"):
            rollouts.self_triggered_rollouts(4, horizon=1.0, trigger_hyper=dict(hyper, kernel=kind), device="cpu")
        with pytest.raises(ValueError, match="RBF data kernel"):
            rollouts.self_triggered_rollouts(4, horizon=1.0, gp=dict(kernel=kind), device="cpu")
    with pytest.raises(ValueError, match="tau_min <= tau_max"):
        rollouts.self_triggered_rollouts(4, horizon=1.0, trigger_hyper=hyper, tau_min=0.1, tau_max=0.01, device="cpu")
    ws = ops.trigger_workspace(3, torch.float32, "cpu")
    assert ws["t"].dtype == torch.float64 and ws["events"].dtype == torch.int32 and ws["Lkd"].shape == (3, 3) and ws["tau"].dtype == torch.float32
