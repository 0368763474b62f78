"""bcbf_lqr_nominal_f32 / _f64 and bcbf_pendulum_control_step_nominal_f64 on the MI355X: the reference's LQR nominal controller
(LQRController.control, controllers.py:64-115) as one lane per instance, against the numpy restatement
(tests/_lqr_reference.py, itself held to the reference's recorded numbers and to scipy's Riccati solver in test_lqr_cpu.py),
against the reference's recorded controls, and through the pendulum step, the façade and the rollouts.
Tolerances are DESIGN section 4's: 1e-8 (fp64) and 1e-3 (fp32) of the largest reference value of the compared array."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lqr_reference as lqr
from _tolreport import rel_close
from test_lqr_cpu import G as GOLD, JETS, pendulum_jets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
T64 = dict(dtype=torch.float64, device=DEV)
SHAPES = [(n, m) for n in (1, 2, 3, 4) for m in (1, 2, 3)]
BATCHES = (1, 63, 64, 65, 257)
HORIZONS = (1, 2, 3, 64, 1000)
RTOL = {torch.float64: 1e-8, torch.float32: 1e-3}
DT = 0.002


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def host(v):
    return v.detach().cpu().double().numpy()


_PROBLEMS = {}


def problem(n, m):
    """257 random instances of shape (n, m) in fp32-representable numbers (one reference serves both precisions), with the
    helper's (u, u0) per horizon -- computed once and left unchanged.
    The scales keep the PROBLEM well conditioned, so that the tolerance measures the kernel: dt = 0.002 (the pendulum demo's)
    makes the longest horizon 2 time units, over which an uncontrolled mode of a unit-normal Jf grows by e^(2 |lambda|) ~ 1e2,
    not the 1e9 of dt = 0.01; the Jacobians of g are scaled by 0.1 and |x| <= 1, so the second linearisation Jf + Jg u0 stays
    of Jf's size.  With them a relative input perturbation of 1e-13 moves u by < 20 times that (own-relative, measured on this
    restatement alone)."""
    if (n, m) not in _PROBLEMS:
        rng = np.random.default_rng(100 * n + m)
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        C = 1 + m
        Mq, Mr = rng.standard_normal((n, n)), rng.standard_normal((m, m))
        Mj = rng.standard_normal((257, n, 1 + n, C))
        Mj[..., 1:] *= 0.1
        p = dict(Mk=f32(rng.standard_normal((257, n, C))), Mj=f32(Mj.reshape(257, n, C * (1 + n))),
                 x=f32(rng.uniform(-1.0, 1.0, (257, n))), x_goal=f32(rng.uniform(-0.5, 0.5, n)),
                 Q=f32(Mq @ Mq.T + np.eye(n)), R=f32(Mr @ Mr.T + np.eye(m)), ref={})
        for H in HORIZONS:
            u, u0, status = lqr.lqr_nominal(p["Mk"], p["Mj"], p["x"], p["x_goal"], p["Q"], p["R"], DT, H, 0)
            assert not status.any() and np.isfinite(u).all()
            p["ref"][H] = (u, u0)
        _PROBLEMS[(n, m)] = p
    return _PROBLEMS[(n, m)]


def run(ops, p, dtype, H, rows=slice(None), t=0, numSteps=None, t_dev=None):
    Mk, Mj, x = (dev(p[k][rows], dtype) for k in ("Mk", "Mj", "x"))
    u, u0, status = ops.lqr_nominal(Mk, Mj, x, p["x_goal"], p["Q"], p["R"], DT, H + t if numSteps is None else numSteps, t,
                                    t_dev=t_dev, want_u0=True)
    torch.cuda.synchronize()
    return u, u0, status


# ---------------------------------------------------------------- 1. the entry against the helper
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nm", SHAPES, ids=lambda v: "n%dm%d" % v)
def test_entry_matches_numpy_restatement(ops, nm, dtype):
    p = problem(*nm)
    for H in HORIZONS:
        ru, ru0 = p["ref"][H]
        for Bt in BATCHES:
            u, u0, status = run(ops, p, dtype, H, slice(0, Bt))
            assert not status.any()
            what = "n%dm%d H%d Bt%d " % (nm + (H, Bt))
            rel_close(host(u), ru[:Bt], RTOL[dtype], what=what + "u")
            rel_close(host(u0), ru0[:Bt], RTOL[dtype], what=what + "u0")


# ---------------------------------------------------------------- 2. the entry against the reference's recorded controls
@pytest.mark.parametrize("tag", ["b", "c"])
@pytest.mark.parametrize("ci", range(4))
def test_entry_matches_reference_lqr_controller(ops, tag, ci):
    numSteps, t, dt = GOLD["configs"][ci]
    Mk, Mj = JETS[tag](GOLD["x"])
    u, status = ops.lqr_nominal(dev(Mk), dev(Mj), dev(GOLD["x"]), GOLD["x_goal"], GOLD["Q"], GOLD["R"], dt, int(numSteps), int(t))
    torch.cuda.synchronize()
    assert not status.any()
    rel_close(host(u), GOLD["%s_c%d_u" % (tag, ci)], 1e-8, what="golden (%s) config %d" % (tag, ci))


# ---------------------------------------------------------------- 3. position independence
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_result_does_not_depend_on_batch_position(ops, dtype):
    p = problem(4, 3)
    H = 64
    u, u0, _ = run(ops, p, dtype, H)
    for b in (0, 63, 64, 200, 256):
        ub, u0b, _ = run(ops, p, dtype, H, slice(b, b + 1))
        assert torch.equal(ub[0], u[b]) and torch.equal(u0b[0], u0[b])
    perm = np.random.default_rng(3).permutation(257)
    up, u0p, _ = run(ops, p, dtype, H, perm)
    idx = torch.as_tensor(perm, device=DEV)
    assert torch.equal(up, u[idx]) and torch.equal(u0p, u0[idx])


# ---------------------------------------------------------------- 4. the horizon read from the device
def test_device_counter_gives_the_host_horizon(ops):
    p = problem(2, 1)
    for t in (0, 3, 99, 100, 250):                     # numSteps = 100: t >= numSteps clamps the horizon to 1
        want = run(ops, p, torch.float64, None, t=t, numSteps=100)
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        got = run(ops, p, torch.float64, None, t=-7, numSteps=100, t_dev=t_dev)          # the host t is then ignored
        assert all(torch.equal(a, b) for a, b in zip(want, got))
    one = run(ops, p, torch.float64, 1)
    assert torch.equal(one[0], run(ops, p, torch.float64, None, t=100, numSteps=100)[0])


def test_captured_graph_replays_a_shrinking_horizon(ops):
    p = problem(2, 1)
    Mk, Mj, x = (dev(p[k]) for k in ("Mk", "Mj", "x"))
    eager = []
    for t in range(3):
        u, _ = ops.lqr_nominal(Mk, Mj, x, p["x_goal"], p["Q"], p["R"], DT, 40, t)
        eager.append(u.clone())
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = (torch.empty(257, 1, **T64), None, torch.empty(257, dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on the capture stream
        ops.lqr_nominal(Mk, Mj, x, p["x_goal"], p["Q"], p["R"], DT, 40, t_dev=t_dev, out=out)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.lqr_nominal(Mk, Mj, x, p["x_goal"], p["Q"], p["R"], DT, 40, t_dev=t_dev, out=out)
        t_dev.add_(1)
    for t in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[t]), t
    assert int(t_dev) == 3


# ---------------------------------------------------------------- 5. status
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_singular_instance_is_reported_and_leaves_its_wave_alone(ops, dtype):
    p = dict(problem(3, 2))
    p["R"] = np.zeros((2, 2))                              # G = B'PB alone: positive definite unless g = 0
    base = run(ops, p, dtype, 64, slice(0, 65))
    assert not base[2].any()
    q = dict(p, Mk=p["Mk"].copy())
    q["Mk"][7, :, 1:] = 0.0                                # instance 7 has no input matrix
    u, u0, status = run(ops, q, dtype, 64, slice(0, 65))
    want = torch.zeros(65, dtype=torch.int32, device=DEV)
    want[7] = 1
    assert torch.equal(status, want)
    assert not u[7].any() and not u0[7].any()
    keep = torch.arange(65, device=DEV) != 7
    assert torch.equal(u[keep], base[0][keep]) and torch.equal(u0[keep], base[1][keep])


# ---------------------------------------------------------------- 6. the pendulum step
def golden_gp(regime, Bt):
    from test_gpu_pendulum import golden_regressor
    if regime == "none":
        return None
    reg = golden_regressor(np.load(os.path.join(GOLDEN, "controllers_pendulum_N16.npz")))
    st = reg._state()
    gp = {k: st[k] for k in ("Lop", "Vw", "X", "UHB", "ell", "s2", "Bm", "M0", "A")}
    if regime == "I":                  # one copy of the model per instance
        gp = {k: v.expand(Bt, *v.shape[1:]).contiguous() for k, v in gp.items()}
    return gp


def states(Bt, seed=4):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.stack([torch.empty(Bt, **T64).uniform_(-1.0, 2.0, generator=gen),
                        torch.empty(Bt, **T64).uniform_(-1.0, 1.0, generator=gen)], dim=1).contiguous()


COST = dict(x_goal=(0.3, -0.2), Q_goal=((2.0, 0.3), (0.3, 1.0)), R=0.5)
WS_KEYS = ("Mk", "Bk", "G", "Mj", "h", "gh", "Hh", "u_ref", "terms2", "terms", "tstatus", "Gc", "hc", "cstatus", "y", "sstatus",
           "iters", "u", "status")


@pytest.mark.parametrize("horizon", [1, 7, 250])
@pytest.mark.parametrize("regime", ["S", "I", "none"])
@pytest.mark.parametrize("Bt", [1, 65])
def test_step_nominal_control_is_the_lqr_entry_on_the_steps_factors(ops, Bt, regime, horizon):
    gp, x0 = golden_gp(regime, Bt), states(Bt)
    numSteps, t = 250, 250 - horizon
    ws = ops.pendulum_workspace(Bt, torch.float64, DEV)
    x = x0.clone()
    step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=(1.0, 10.0, 1.0), nominal="lqr", numSteps=numSteps, t=t, **COST)
    step()
    torch.cuda.synchronize()
    u, status = ops.lqr_nominal(ws["Mk"], ws["Mj"], x0, COST["x_goal"], COST["Q_goal"], [[COST["R"]]], 0.002, numSteps, t)
    assert torch.equal(ws["u_ref"], u) and torch.equal(step.lstatus, status) and not status.any()
    assert torch.isfinite(ws["u"]).all() and not torch.equal(x, x0)
    # explore and clip on top: the host's formula (EpsilonGreedyController, then clip) on that value
    lo, hi, eps = -1.5, 1.0, 0.5
    ex = torch.rand(Bt, 2, generator=torch.Generator(device=DEV).manual_seed(9), **T64)
    ws2, x2 = ops.pendulum_workspace(Bt, torch.float64, DEV), x0.clone()
    ops.pendulum_control_step_prepare(gp, ws2, x2, mean_model=(1.0, 10.0, 1.0), nominal="lqr", numSteps=numSteps, t=t, explore=ex,
                                      eps=eps, ctrl_range=(lo, hi), **COST)()
    torch.cuda.synchronize()
    want = torch.where(ex[:, :1] < eps, lo + ex[:, 1:] * (hi - lo), u).clamp(lo, hi)
    # (the kernel may contract lo + a (hi - lo) into one fused multiply-add: one rounding of a value of size <= |hi - lo|)
    np.testing.assert_allclose(host(ws2["u_ref"]), host(want), rtol=0, atol=2 * np.finfo(np.float64).eps * (hi - lo))
    assert bool((ex[:, 0] < eps).any()) or Bt == 1


@pytest.mark.parametrize("ci", range(4))
def test_step_no_gp_nominal_control_matches_reference_lqr_controller(ops, ci):
    numSteps, t, dt = GOLD["configs"][ci]
    x = dev(GOLD["x"])
    ws = ops.pendulum_workspace(len(x), torch.float64, DEV)
    ops.pendulum_control_step_prepare(None, ws, x, mean_model=tuple(GOLD["b_model"]), dt=float(dt), nominal="lqr",
                                      numSteps=int(numSteps), t=int(t), x_goal=tuple(GOLD["x_goal"]),
                                      Q_goal=GOLD["Q"].tolist(), R=float(GOLD["R"][0, 0]))()
    torch.cuda.synchronize()
    rel_close(host(ws["u_ref"]), GOLD["b_c%d_u" % ci], 1e-8, what="step, no-GP, config %d" % ci)
    Mk, Mj = pendulum_jets(GOLD["x"])
    np.testing.assert_allclose(host(ws["Mk"]), Mk, rtol=1e-14, atol=1e-14)            # (device sin / cos against numpy's)
    np.testing.assert_allclose(host(ws["Mj"]), Mj, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("plant", ["true", "posterior"])
@pytest.mark.parametrize("regime", ["S", "I", "none"])
@pytest.mark.parametrize("Bt", [1, 65])
def test_step_greedy_through_the_nominal_entry_is_bitwise_the_existing_entry(ops, Bt, regime, plant):
    gp, x0 = golden_gp(regime, Bt), states(Bt, seed=6)
    gen = torch.Generator(device=DEV).manual_seed(12)
    ex, z = torch.rand(Bt, 2, generator=gen, **T64), torch.randn(Bt, 2, 4, generator=gen, **T64)
    outs = []
    for nominal_entry in (False, True):
        ws, x = ops.pendulum_workspace(Bt, torch.float64, DEV), x0.clone()
        draw = dict(z=z.clone(), xdot_s=torch.zeros(Bt, 2, **T64), cbc_s=torch.zeros(Bt, 2, **T64)) if plant == "posterior" else None
        obs = tuple(torch.zeros(Bt, 2, **T64) for _ in range(3))
        stats = (torch.full((Bt,), float("inf"), **T64), torch.zeros(Bt, dtype=torch.int32, device=DEV))
        step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=(1.2, 9.0, 0.9), explore=ex, eps=0.3, ctrl_range=(-15.0, 15.0),
                                                 observe=True, sampled=draw, stats=stats, nominal_entry=nominal_entry, **COST)
        step(obs=obs + (1,))
        torch.cuda.synchronize()
        outs.append([x] + [ws[k] for k in WS_KEYS] + list(obs) + list(stats) + ([draw["xdot_s"], draw["cbc_s"]] if draw else []))
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), k
    assert not torch.equal(outs[0][0], x0)


# ---------------------------------------------------------------- 7. the façade and the rollouts
def test_lqr_controller_single_state_is_a_row_of_the_batch(ops):
    from bayesian_cbf_amd.controllers import LQRController, SumDynamicModels
    from bayesian_cbf_amd.pendulum import PendulumDynamicsModel
    from test_gpu_pendulum import golden_regressor
    reg = golden_regressor(np.load(os.path.join(GOLDEN, "controllers_pendulum_N16.npz")))
    mean = PendulumDynamicsModel(m=1, n=2, mass=1.0, gravity=10.0, length=1.0, dtype=torch.float64)
    Q, R, xg = torch.tensor(COST["Q_goal"], **T64), torch.tensor([[COST["R"]]], **T64), torch.tensor(COST["x_goal"], **T64)
    xs = states(5)
    for model in (reg, SumDynamicModels(reg, mean), mean):
        ctrl = LQRController(model, Q, R, xg, 50, 0.002, None)
        ub = ctrl.control(xs, t=3)
        assert ub.shape == (5, 1) and not ctrl.last_status.any()
        for b in (0, 4):
            assert torch.equal(ctrl.control(xs[b], t=3), ub[b])
        assert torch.equal(ctrl.control(xs), ctrl.control(xs, t=0))           # t = None is t = 0
    # the deterministic pendulum through autograd is golden (b)'s controller
    numSteps, t, dt = GOLD["configs"][2]
    ctrl = LQRController(mean, dev(GOLD["Q"]), dev(GOLD["R"]), dev(GOLD["x_goal"]), int(numSteps), float(dt), None)
    rel_close(host(ctrl.control(dev(GOLD["x"]), t=int(t))), GOLD["b_c2_u"], 1e-8, what="facade on the pendulum")


def test_control_cbf_learned_takes_the_lqr_controller(ops):
    from bayesian_cbf_amd.controllers import ControlCBFLearned, LQRController, SOCPController
    from bayesian_cbf_amd.pendulum import RadialCBFRelDegree2
    from test_gpu_pendulum import golden_regressor
    reg = golden_regressor(np.load(os.path.join(GOLDEN, "controllers_pendulum_N16.npz")))
    ctrl = ControlCBFLearned(x_dim=2, u_dim=1, model=reg, dt=0.002, numSteps=50, unsafe_controller_class=LQRController,
                             cbfs=[RadialCBFRelDegree2(reg, dtype=torch.float64)], controller_class=SOCPController,
                             exploration_controller_class=None, ctrl_range=(-15.0, 15.0))
    assert isinstance(ctrl.unsafe_controller, LQRController)
    u = ctrl.control(states(1), t=0)
    assert u.shape[-1] == 1 and torch.isfinite(u).all()


def test_learning_rollouts_take_the_lqr_controller(ops):
    """Two refits in 25 steps; the explorer wraps the LQR control: where the coin did not explore, the recorded u_ref is the
    clipped LQR control, which differs from the greedy loop's on the same draws from the first step on."""
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    kw = dict(numSteps=25, train_every=10, max_train=16, mean_model=(1.0, 10.0, 1.0), egreedy=(0.5, 0.1), seed=2, record=True)
    r = pendulum_learning_rollouts(8, nominal="lqr", **kw)
    g = pendulum_learning_rollouts(8, draws=r["draws"], x0=r["traj"][0], **kw)
    assert r["lqr_failures"] == 0 and len(r["report"]["refits"]) == 2
    assert torch.isfinite(r["traj"]).all() and torch.isfinite(r["u_ref"]).all()
    assert float(r["u_ref"].abs().max()) <= 15.0
    assert torch.equal(r["traj"][0], g["traj"][0]) and not torch.equal(r["u_ref"][0], g["u_ref"][0])
    # step 0 runs on the prior (Mk = M0', Mj = 0) plus the mean model: the LQR control there, clipped
    kept = r["draws"]["explore"][0, :, 0] >= 0.5
    assert bool(kept.any())
    Mk, Mj = pendulum_jets(host(r["traj"][0]))
    Mk = dev(Mk) + r["final"]["hyper"]["M0"].transpose(1, 2)
    u, status = ops.lqr_nominal(Mk.contiguous(), dev(Mj), r["traj"][0].contiguous(), (0.0, 0.0), np.eye(2), [[1.0]], 0.002, 25, 0)
    # (the step's sin / cos are the device's, these jets numpy's: an ulp apart at most, far inside 1e-8)
    rel_close(host(r["u_ref"][0][kept]), host(u[:, 0].clamp(-15.0, 15.0)[kept]), 1e-8, what="learning loop, step 0 u_ref")


def test_safety_rollouts_with_the_lqr_controller_eager_equals_graph(ops, capsys):
    from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
    kw = dict(numSteps=25, mean_model=(1.0, 10.0, 1.0), nominal="lqr", seed=3)
    e = pendulum_safety_rollouts(64, use_graph=False, **kw)
    g = pendulum_safety_rollouts(64, use_graph=True, **kw)
    assert torch.equal(e["x_final"], g["x_final"]) and torch.equal(e["min_h"], g["min_h"])
    assert e["lqr_failures"] == g["lqr_failures"] == 0
    greedy = pendulum_safety_rollouts(64, numSteps=25, mean_model=(1.0, 10.0, 1.0), seed=3)
    assert not torch.equal(greedy["x_final"], e["x_final"])             # the nominal controller is a different one
    with capsys.disabled():
        print("\npendulum_safety_rollouts(nominal='lqr'), 64 x 25 steps: min_h = %.4f (greedy: %.4f)"
              % (float(e["min_h"].min()), float(greedy["min_h"].min())))
