"""bcbf_pendulum_control_step_f64 / bcbf_pendulum_plant_step on the MI355X: the pendulum's rel-degree-2 safety filter
(SOCPController with cbfs = [RadialCBFRelDegree2], clf = None, greedy nominal control) as one batched device step,
against the executed reference's recorded terms and cone rows, the CPU oracle composition, the host façade and the
reference's plant trajectory; and the batched rollouts built on it."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _pendulum_oracle import oracle_state, oracle_step
from test_pendulum_cpu import cone_close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
T64 = dict(dtype=torch.float64, device=DEV)
KINDS = ("rbf", "matern52", "rbf_matern52")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), **T64)


def host(v):
    return v.detach().cpu().double().numpy()


def golden_regressor(g):
    from bayesian_cbf_amd.control_affine_model import ControlAffineRegressor
    reg = ControlAffineRegressor(2, 1, device=DEV, dtype=torch.float64)
    reg.set_kernel_params(A=g["A"], B=g["B"], lengthscale=g["ell"], scalefactor=float(g["s2"]), M0=g["M0"])
    reg.fit(t(g["X"]), t(g["U"]), t(g["Xdot"]), training_iter=0)
    it = iter([g["jitter_rand"][0]])
    reg.rand_fn = lambda k: t(next(it)[:k])
    return reg


def rows_to_cones(Gc, hc):
    """bcbf_controller_cones rows [objective (3), safety (3)] -> [(A, b, c, d)] (Gq = [-c'; -A], hq = [d; b])."""
    return [(-Gc[r + 1:r + 3], hc[r + 1:r + 3], -Gc[r], hc[r]) for r in (0, 3)]


# ---------------------------------------------------------------- 1. reference goldens, learned model (regime S)
@pytest.mark.parametrize("tag", ["N16", "N40"])
def test_step_terms_and_rows_match_reference_goldens(ops, tag):
    from oracle import controllers as oc
    g = np.load(os.path.join(GOLDEN, "controllers_pendulum_%s.npz" % tag))
    reg = golden_regressor(g)
    gp = dict(reg._state())
    S = len(g["xs"])
    ws = ops.pendulum_workspace(S, torch.float64, DEV)
    x, uref = t(g["xs"]), t(g["urefs"])
    sf = float(g["safety_factor"])
    ops.pendulum_control_step(gp, ws, x, u_ref=uref, k_alpha=tuple(g["k_alpha"]), max_unsafe_prob=1.0 / (1.0 + sf * sf),
                              ctrl_reg=float(g["ctrl_reg"]), relax_weight=float(g["relax_weight"]))
    torch.cuda.synchronize()
    np.testing.assert_allclose(host(ws["terms"])[:, 0], g["t_safety_terms"], rtol=1e-9, atol=1e-11)
    Gc, hc = host(ws["Gc"]), host(ws["hc"])
    for i in range(S):
        bfe, e, V, bfv, v = (g["t_safety_terms"][i][k] for k in range(5))
        indefinite = np.linalg.eigvalsh(oc._asq(np.array([[V]]), np.array([bfv]), v)).min() <= 0
        for cone, key in zip(rows_to_cones(Gc[i], hc[i]), ("obj", "safety")):
            cone_close(cone, tuple(g["t_%s_%s" % (key, k)][i] for k in "Abcd"), key == "safety" and indefinite)
    # the cbc2 fixtures: (mean_A, mean_b, Q, p, r) at u0s
    c2 = np.load(os.path.join(GOLDEN, "cbc2_pendulum_%s.npz" % tag))
    reg2 = golden_regressor(c2)
    S2 = len(c2["xs"])
    ws2 = ops.pendulum_workspace(S2, torch.float64, DEV)
    ops.pendulum_control_step(dict(reg2._state()), ws2, t(c2["xs"]), u_ref=t(c2["u0s"]), k_alpha=tuple(c2["k_alpha"]))
    torch.cuda.synchronize()
    out = host(ws2["terms2"])
    for k, name in enumerate(("mean_A", "mean_b", "Q", "p", "r")):
        np.testing.assert_allclose(out[:, k], c2["t_" + name].reshape(S2), rtol=1e-9, atol=1e-11, err_msg=name)


# ---------------------------------------------------------------- 2. oracle composition
def _instances(ops, Bt, N, kernel, seed):
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(Bt, N, 2, 1, dtype=torch.float64, device=DEV, seed=seed)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], kernel=kernel)
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=p["A"], kernel=kernel)
    h = {k: host(v) for k, v in p.items()}
    states = [oracle_state(h["X"][i], h["UH"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i],
                           h["jitter"][i], h["A"][i], kernel=kernel) for i in range(Bt)]
    return gp, states


@pytest.mark.parametrize("kernel", KINDS)
@pytest.mark.parametrize("mean", [None, (1.2, 9.0, 0.9)])
@pytest.mark.parametrize("regime", ["I", "S"])
def test_step_matches_oracle_composition(ops, regime, mean, kernel):
    B = 32
    gp, states = _instances(ops, 1 if regime == "S" else B, 48, kernel, seed=7 + KINDS.index(kernel))
    if regime == "S":
        states = states * B
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.empty(B, 2, **T64)
    x[:, 0].uniform_(-1.5, 0.2, generator=gen)          # inside the training box of make_instances
    x[:, 1].uniform_(-1.0, 1.0, generator=gen)
    x0 = host(x)
    ws = ops.pendulum_workspace(B, torch.float64, DEV)
    ops.pendulum_control_step(gp, ws, x, mean_model=mean)
    torch.cuda.synchronize()
    u, status, xn, uref = host(ws["u"])[:, 0], ws["status"].cpu().numpy(), host(x), host(ws["u_ref"])[:, 0]
    for i in range(B):
        o = oracle_step(states[i], x0[i], mean_model=mean)
        np.testing.assert_allclose(uref[i], o["u_ref"][0], rtol=1e-9, atol=1e-11)
        assert (status[i] == 0) == (o["status"] == "optimal"), (i, status[i], o["status"])
        np.testing.assert_allclose(u[i], o["u"][0], rtol=1e-7, atol=1e-7 * max(1.0, abs(o["u"][0])))
        np.testing.assert_allclose(xn[i], o["x_next"], rtol=1e-7, atol=1e-9)


# ---------------------------------------------------------------- 3. façade equality
def test_step_equals_socp_controller_facade(ops):
    from bayesian_cbf_amd.controllers import GreedyController, SOCPController, SumDynamicModels
    from bayesian_cbf_amd.pendulum import PendulumDynamicsModel, RadialCBFRelDegree2
    g = np.load(os.path.join(GOLDEN, "controllers_pendulum_N40.npz"))
    reg = golden_regressor(g)
    mean = PendulumDynamicsModel(m=1, n=2, mass=1.0, gravity=10.0, length=1.0, dtype=torch.float64)
    net = SumDynamicModels(reg, mean)
    cbf = RadialCBFRelDegree2(net, dtype=torch.float64)
    dt = 0.002
    greedy = GreedyController(net, torch.eye(2, **T64), torch.eye(1, **T64), torch.zeros(2, **T64), 250, dt, None)
    ctrl = SOCPController(2, 1, 1.0, 100.0, net, [cbf], None, greedy)
    gen = torch.Generator(device=DEV).manual_seed(5)
    xs = torch.stack([torch.empty(24, **T64).uniform_(-1.0, 2.0, generator=gen),
                      torch.empty(24, **T64).uniform_(-1.0, 1.0, generator=gen)], dim=1).contiguous()
    u_f = ctrl.control(xs.clone())
    ws = ops.pendulum_workspace(24, torch.float64, DEV)
    x = xs.clone()
    ops.pendulum_control_step(dict(reg._state()), ws, x, mean_model=(1.0, 10.0, 1.0), dt=dt)
    torch.cuda.synchronize()
    assert torch.equal(ws["status"].cpu(), ctrl.last_status.cpu().to(torch.int32))
    np.testing.assert_allclose(host(ws["u"]), host(u_f), rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------- 4. no-GP mode
def test_no_gp_mode_terms_are_deterministic(ops):
    B = 64
    gen = torch.Generator(device=DEV).manual_seed(2)
    x = torch.stack([torch.empty(B, **T64).uniform_(-math.pi, math.pi, generator=gen),
                     torch.empty(B, **T64).uniform_(-3.0, 3.0, generator=gen)], dim=1).contiguous()
    x0 = host(x)
    ws = ops.pendulum_workspace(B, torch.float64, DEV)
    ws["Bk"].fill_(7.0)                               # no-GP mode owns these buffers: stale contents must not leak in
    ws["G"].fill_(7.0)
    ops.pendulum_control_step(None, ws, x, mean_model=(1.0, 10.0, 1.0))
    torch.cuda.synchronize()
    terms = host(ws["terms"])[:, 0]
    assert np.all(terms[:, 2:] == 0.0), "V, bfv, v must be exactly 0"
    th, om = x0[:, 0], x0[:, 1]
    d = th - math.pi / 4
    h = math.cos(math.pi / 8) - np.cos(d)
    np.testing.assert_allclose(terms[:, 0], np.sin(d), rtol=1e-13, atol=1e-15)                       # -A(x)
    np.testing.assert_allclose(terms[:, 1], om ** 2 * np.cos(d) - 10.0 * np.sin(d) * np.sin(th) + h + 3.0 * om * np.sin(d),
                               rtol=1e-12, atol=1e-12)                                                # b(x)
    for i in range(0, B, 8):
        o = oracle_step(None, x0[i], mean_model=(1.0, 10.0, 1.0))
        assert (int(ws["status"][i]) == 0) == (o["status"] == "optimal")
        np.testing.assert_allclose(host(ws["u"])[i, 0], o["u"][0], rtol=1e-7, atol=1e-7 * max(1.0, abs(o["u"][0])))


# ---------------------------------------------------------------- 5. plant
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_plant_step_replays_reference_trajectory(ops, dtype):
    g = np.load(os.path.join(GOLDEN, "facade_surfaces.npz"))
    X, U = g["pend_X"], g["pend_U"]
    dt = 0.05                                  # the generator's (gen_golden.py: sampling_pendulum_data(dt=0.05))
    x = torch.as_tensor(X[:-1], dtype=dtype, device=DEV).contiguous()
    u = torch.as_tensor(U[:-1], dtype=dtype, device=DEV).contiguous()
    ops.pendulum_plant_step(x, u, 1.0, 10.0, 1.0, dt)
    torch.cuda.synchronize()
    got = host(x)
    assert (np.abs(X[1:, 0] - X[:-1, 0]) > 3.0).any()          # the replay crosses the wrap
    if dtype == torch.float64:
        np.testing.assert_allclose(got, X[1:], rtol=1e-13, atol=1e-13)
    else:                                      # fp32 may land on the other side of +-pi: compare angles modulo 2 pi
        dth = np.angle(np.exp(1j * (got[:, 0] - X[1:, 0])))
        assert np.abs(dth).max() < 1e-4 and np.abs(got[:, 1] - X[1:, 1]).max() < 1e-4 * max(1.0, np.abs(X[:, 1]).max())


# ---------------------------------------------------------------- 6. rollouts
def _model(ops, Bt, kernel="rbf"):
    gp, _ = _instances(ops, Bt, 48, kernel, seed=21)
    return gp


@pytest.mark.parametrize("regime", ["S", "I", "none"])
def test_rollouts_graph_batch_and_min_h(ops, regime):
    from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
    B, steps = 256, 100
    gp = None if regime == "none" else _model(ops, 1 if regime == "S" else B)
    kw = dict(numSteps=steps, gp=gp, shared=regime == "S", mean_model=(1.0, 10.0, 1.0), seed=3)
    eager = pendulum_safety_rollouts(B, **kw)
    graph = pendulum_safety_rollouts(B, use_graph=True, **kw)
    assert torch.equal(eager["x_final"], graph["x_final"]) and torch.equal(eager["min_h"], graph["min_h"])
    assert torch.equal(eager["fails"], graph["fails"])
    rec = pendulum_safety_rollouts(B, record=True, **kw)
    assert torch.equal(rec["x_final"], eager["x_final"])
    th = rec["traj"][:steps, :, 0]
    h = math.cos(math.pi / 8) - torch.cos(th - math.pi / 4)
    assert torch.equal(rec["min_h"], h.min(dim=0).values)
    assert eager["stats"]["count"] == B
    # instance i of the batch == a Bt = 1 run of instance i (same start state)
    x_start = rec["traj"][0]
    for i in (0, 77, 255):
        gp1 = None if gp is None else (gp if regime == "S" else
                                       {k: (v[i:i + 1].contiguous() if torch.is_tensor(v) else v) for k, v in gp.items()})
        one = _single(ops, gp1, x_start[i:i + 1].clone(), steps)
        assert torch.equal(one, rec["traj"][steps, i:i + 1]), i


def _single(ops, gp, x, steps):
    ws = ops.pendulum_workspace(1, torch.float64, DEV)
    step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=(1.0, 10.0, 1.0))
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return x


def test_no_gp_safe_loop_from_reference_start_is_recorded(ops, capsys):
    """Recorded, not asserted: whether the no-GP safe loop keeps min_h >= 0 from theta0 = 7 pi / 12."""
    from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
    r = pendulum_safety_rollouts(256, numSteps=250, gp=None, mean_model=(1.0, 10.0, 1.0), start_noise=0.0)
    with capsys.disabled():
        print("\nno-GP safe loop from 7pi/12, 250 steps: %s" % r["stats"])
    assert r["stats"]["count"] == 256
