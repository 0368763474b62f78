"""bcbf_pendulum_control_step_sampled_f64 on the MI355X: the pendulum's rel-degree-2 safety loop on plants drawn from the
model's own posterior, against the observing entry (everything up to the plant kernel is unchanged), the numpy restatement
of the draw (_pendulum_posterior_plant_reference), the exact quadratic-form moments of the condition, and the rollouts
built on it."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pendulum_posterior_plant_reference as ref
from test_gpu_pendulum import DEV, KINDS, T64, _instances, host, t

DT = 0.002
# Deviation of the device from the numpy restatement with the same z, max |got - want| / max(1, max |want|) per quantity, the
# worst over every comparison of this file (`close_to_restatement`; the device contracts a * b + c into fused multiply-adds,
# numpy does not).  MEASURED on the MI355X; the bound is ten times that, and never more than 1e-8 of the quantity's scale.
MEASURED = dict(xdot_s=3.0e-16, cbc_s=2.85e-16, x_next=3.81e-17)
BOUND = {k: min(10.0 * v, 1e-8) for k, v in MEASURED.items()}


@pytest.fixture(scope="module", autouse=True)
def leave_the_global_generators_alone():
    """A fresh regressor draws its start hyper-parameters from torch's global generator; tests that run after this module must
    find that generator where they would have found it without this module."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def normals(B, seed):
    return torch.randn(B, 2, 4, generator=torch.Generator(device=DEV).manual_seed(seed), **T64)


def states(B, seed, lo=-1.5, hi=0.2):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.empty(B, 2, **T64)
    x[:, 0].uniform_(lo, hi, generator=gen)
    x[:, 1].uniform_(-1.0, 1.0, generator=gen)
    return x


def run_sampled(ops, gp, x0, z, step_kw=None, **kw):
    """One sampled step from x0 (left untouched): (workspace, x_next, the `sampled` dict with its outputs and counters)."""
    B = x0.shape[0]
    ws = ops.pendulum_workspace(B, torch.float64, DEV)
    x = x0.clone()
    i32 = dict(dtype=torch.int32, device=DEV)
    draw = dict(z=z, xdot_s=torch.full((B, 2), float("nan"), **T64), cbc_s=torch.full((B, 2), float("nan"), **T64),
                relaxed=torch.zeros(B, **i32), viol_relaxed=torch.zeros(B, **i32), rho_tol=1e-6)
    ops.pendulum_control_step_prepare(gp, ws, x, dt=DT, sampled=draw, **kw)(**(step_kw or {}))
    torch.cuda.synchronize()
    return ws, x, draw


def hyper_rows(gp, B):
    """(A, ell, s2, Bm) per instance on the host, whatever leading axis gp carries."""
    out = []
    for k in ("A", "ell", "s2", "Bm"):
        v = host(gp[k])
        out.append(np.broadcast_to(v, (B,) + v.shape[1:]))
    return out


def restate(ws, gp, kernel, x0, z, u=None, gp_flag=True, k_alpha=ref.K_ALPHA):
    """The numpy restatement of the sampled plant kernel on the step's own workspace: (xdot_s, cbc_s, x_next), each [B,2]."""
    B = x0.shape[0]
    A, ell, s2, Bm = hyper_rows(gp, B)
    w = {k: host(ws[k]) for k in ("Mk", "Bk", "G", "Mj", "h", "gh", "Hh")}
    u = host(ws["u"])[:, 0] if u is None else u
    xs, zs = host(x0), host(z)
    out = [ref.sampled_step({k: w[k][b] for k in ("Mk", "Bk", "G", "Mj")}, A[b], ell[b], s2[b], Bm[b, 0, 0], ref.KXX[kernel],
                            w["h"][b], w["gh"][b], w["Hh"][b], k_alpha, u[b], zs[b], xs[b], DT, gp=gp_flag) for b in range(B)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def close_to_restatement(draw, x, want, which=("xdot_s", "cbc_s", "x_next")):
    """Hold the step's outputs to restate()'s (xdot_s, cbc_s, x_next); each figure is printed before it is asserted."""
    got = dict(xdot_s=host(draw["xdot_s"]), cbc_s=host(draw["cbc_s"]), x_next=host(x))
    for k, w in zip(("xdot_s", "cbc_s", "x_next"), want):
        if k in which:
            assert np.isfinite(got[k]).all(), k
            d = float(np.abs(got[k] - w).max() / max(1.0, np.abs(w).max()))
            print("%s deviation %.3g (bound %.3g)" % (k, d, BOUND[k]))
            assert d <= BOUND[k], (k, d)


# ---------------------------------------------------------------- 1, 2, 7: one step per (kernel, regime, mean model)
CASES = {}


def case(ops, kernel, regime, mean):
    key = (kernel, regime, mean)
    if key not in CASES:
        B, N = (70, 16) if mean is None else (33, 40)
        gp, _ = _instances(ops, 1 if regime == "S" else B, N, kernel, seed=31 + KINDS.index(kernel))
        x0, z = states(B, 5), normals(B, 6)
        # the observing entry on the same inputs
        wo, xo = ops.pendulum_workspace(B, torch.float64, DEV), x0.clone()
        ops.pendulum_control_step_prepare(gp, wo, xo, mean_model=mean, dt=DT, observe=True)()
        obs = tuple(torch.zeros(B, 2, **T64) for _ in range(3))
        ws, x, draw = run_sampled(ops, gp, x0, z, step_kw=dict(obs=obs + (1,)), mean_model=mean, observe=True)
        CASES[key] = dict(gp=gp, x0=x0, z=z, wo=wo, ws=ws, x=x, draw=draw, obs=obs, B=B)
    return CASES[key]


ALL = pytest.mark.parametrize("kernel,regime,mean", [(k, r, m) for k in KINDS for r in ("I", "S") for m in (None, (1.2, 9.0, 0.9))])


@ALL
def test_program_is_byte_equal_to_the_observing_entry(ops, kernel, regime, mean):
    c = case(ops, kernel, regime, mean)
    for k in ("y", "sstatus", "status", "u", "terms2", "u_ref"):
        assert torch.equal(c["ws"][k], c["wo"][k]), k


@ALL
def test_draw_matches_numpy_restatement(ops, kernel, regime, mean):
    c = case(ops, kernel, regime, mean)
    xd, cbc, xn = restate(c["ws"], c["gp"], kernel, c["x0"], c["z"])
    Mk, u = host(c["ws"]["Mk"]), host(c["ws"]["u"])
    assert np.abs(xd - (Mk[:, :, 0] + Mk[:, :, 1] * u)).max() > 1e-3, "the draw moved the plant off the posterior mean"
    close_to_restatement(c["draw"], c["x"], (xd, cbc, xn))


@ALL
def test_observation_rows_record_the_drawn_plant(ops, kernel, regime, mean):
    c = case(ops, kernel, regime, mean)
    x0, u, xd = host(c["x0"]), host(c["ws"]["u"])[:, 0], host(c["draw"]["xdot_s"])
    assert np.abs(host(c["x"])[:, 0] - x0[:, 0]).max() < 1.0, "no step of this case wraps"
    m = np.zeros_like(xd)
    if mean is not None:
        m = np.stack([x0[:, 1], -(mean[1] / mean[2]) * np.sin(x0[:, 0]) + u / (mean[0] * mean[2])], axis=1)
    ox, ouh, oy = (host(v) for v in c["obs"])
    assert np.array_equal(ox, x0) and np.array_equal(ouh, np.stack([np.ones_like(u), u], axis=1))
    # (x_{t+1} - x_t) / dt from the stored states: one rounding of x_{t+1}, eps |x| / dt ~ 1e-13
    np.testing.assert_allclose(oy, xd - m, rtol=0, atol=1e-11 * max(1.0, np.abs(xd).max()))


# ---------------------------------------------------------------- 3. z = 0 and the no-GP mode
@pytest.mark.parametrize("kernel", KINDS)
def test_zero_draw_is_the_deterministic_form_at_the_mean(ops, kernel):
    B = 48
    gp, _ = _instances(ops, B, 16, kernel, seed=41)
    x0 = states(B, 8)
    ws, x, draw = run_sampled(ops, gp, x0, torch.zeros(B, 2, 4, **T64), mean_model=(1.0, 10.0, 1.0))
    Mk, Mj, u = host(ws["Mk"]), host(ws["Mj"]), host(ws["u"])[:, 0]
    np.testing.assert_allclose(host(draw["xdot_s"]), Mk[:, :, 0] + Mk[:, :, 1] * u[:, None], rtol=1e-14, atol=1e-14)
    h, gh, Hh = host(ws["h"]), host(ws["gh"]), host(ws["Hh"])
    for b in range(B):
        _, lfh, c2 = ref.cbc2_on(ref.jet_mean(Mk[b], Mj[b]), u[b], h[b], gh[b], Hh[b], ref.K_ALPHA)
        np.testing.assert_allclose(host(draw["cbc_s"])[b], [lfh, c2], rtol=1e-13, atol=1e-12)


def test_no_gp_mode_ignores_the_draw(ops):
    B, mean = 64, (1.2, 9.0, 0.9)
    x0 = states(B, 9, lo=-3.0, hi=3.0)
    ws, x, draw = run_sampled(ops, None, x0, normals(B, 10), mean_model=mean)
    terms2, u = host(ws["terms2"]), host(ws["u"])[:, 0]
    want = terms2[:, 0] * u + terms2[:, 1]
    np.testing.assert_allclose(host(draw["cbc_s"])[:, 1], want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))
    xp = x0.clone()
    ops.pendulum_plant_step(xp, ws["u"], *mean, DT)              # the plant of the mean model's parameters
    torch.cuda.synchronize()
    np.testing.assert_allclose(host(x), host(xp), rtol=0, atol=1e-14)


# ---------------------------------------------------------------- 4. prior mode with no data
@pytest.mark.parametrize("kernel", KINDS)
def test_prior_mode_draws_from_the_prior(ops, kernel):
    B = 40
    gp, _ = _instances(ops, B, 16, kernel, seed=43)
    hyper = {k: gp[k] for k in ("ell", "s2", "Bm", "M0", "A")}
    x0, z = states(B, 12), normals(B, 13)
    # (the prior of a regressor without data does not depend on the data kernel's shape, only kxx does: the RBF value is the
    # one the step uses there, as bcbf_cbc2_terms does)
    ws, x, draw = run_sampled(ops, hyper, x0, z, prior=True, mean_model=(1.0, 10.0, 1.0))
    s2, Bm, ell = host(gp["s2"]), host(gp["Bm"]), host(gp["ell"])
    assert np.array_equal(host(ws["Bk"]), s2[:, None, None] * Bm) and not host(ws["G"]).any()
    xd, cbc, xn = restate(ws, hyper, "rbf", x0, z)
    for b in range(0, B, 7):                                     # Sigma4 of the restatement is the closed form
        S4 = ref.jet_covariance(host(ws["Bk"])[b], host(ws["G"])[b], ell[b], s2[b], Bm[b, 0, 0], 1.0)
        want = np.zeros((4, 4))
        want[:2, :2] = s2[b] * Bm[b]
        want[2, 2], want[3, 3] = (s2[b] * Bm[b, 0, 0] / ell[b, d] ** 2 for d in range(2))
        np.testing.assert_allclose(S4, want, rtol=1e-15)
    close_to_restatement(draw, x, (xd, cbc, xn))
    assert np.abs(xd - host(ws["Mk"])[:, :, 0]).max() > 1e-2


# ---------------------------------------------------------------- 5. semidefinite inputs
def test_query_on_a_training_row_at_tiny_jitter_stays_finite(ops):
    from bayesian_cbf_amd.synthetic import make_instances
    B, N = 24, 16
    p = make_instances(B, N, 2, 1, dtype=torch.float64, device=DEV, seed=45)
    jit = torch.full_like(p["jitter"], 1e-10)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit)
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=p["A"])
    x0, z = p["X"][:, 3].clone().contiguous(), normals(B, 14)
    ws, x, draw = run_sampled(ops, gp, x0, z, mean_model=(1.0, 10.0, 1.0))
    for v in (draw["xdot_s"], draw["cbc_s"], x):
        assert torch.isfinite(v).all()
    xd, cbc, xn = restate(ws, gp, "rbf", x0, z)
    assert np.isfinite(xd).all() and np.isfinite(cbc).all()


@pytest.mark.parametrize("A2", [((1.0, 0.0), (0.0, 0.0)), ((4.0, 2.0), (2.0, 1.0))], ids=["diag(1,0)", "rank1"])
def test_a_null_direction_of_A_receives_no_draw(ops, A2):
    B = 40
    gp, _ = _instances(ops, B, 16, "rbf", seed=47)
    gp = dict(gp, A=t(np.array(A2)).expand(B, 2, 2).contiguous())
    x0, z = states(B, 15), normals(B, 16)
    ws, x, draw = run_sampled(ops, gp, x0, z)
    assert all(torch.isfinite(v).all() for v in (draw["xdot_s"], draw["cbc_s"], x))
    Mk, u = host(ws["Mk"]), host(ws["u"])[:, 0]
    d = host(draw["xdot_s"]) - (Mk[:, :, 0] + Mk[:, :, 1] * u[:, None])          # what the draw added to the mean plant
    assert np.abs(d[:, 0]).max() > 1e-3
    if A2[1][1] == 0.0:
        np.testing.assert_allclose(d[:, 1], 0.0, rtol=0, atol=1e-14 * max(1.0, np.abs(Mk).max() * np.abs(u).max()))
    else:                                                       # the range is span{(2, 1)}: its null direction (1, -2) sees nothing
        np.testing.assert_allclose(d[:, 0] - 2.0 * d[:, 1], 0.0, rtol=0, atol=1e-12 * max(1.0, np.abs(d).max()))
    close_to_restatement(draw, x, restate(ws, gp, "rbf", x0, z))


# ---------------------------------------------------------------- 6, 8: one shared model at one state
SAMPLER = dict(x=(0.2, -0.3), mean_model=(1.0, 10.0, 1.0), max_unsafe_prob=0.2, u_ref=ref.U0)
# (chosen on the CPU: _pendulum_oracle.oracle_step solves this program -- u = -0.6195, the safety cone active -- and the exact
# moments of CBC2 there are mean 5.051, variance 6.366, so var / (var + mean^2) = 0.1997)


def small_model_on_device(ops):
    m = ref.small_model()
    X, UH, Xdot = (t(m[k])[None] for k in ("X", "UH", "Xdot"))
    Bm, ell, s2, M0, A = t(m["Bm"])[None], t(m["ell"])[None], t(np.array([m["s2"]])), t(m["M0"])[None], t(m["A"])[None]
    Lop, UHB, info, _ = ops.refit(X, UH, Bm, ell, s2, t(m["jitter"])[None])
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, Xdot, UH, M0, want_alpha=False)
    return m, dict(Lop=Lop, Vw=Vw, X=X, UHB=UHB, ell=ell, s2=s2, Bm=Bm, M0=M0, A=A)


def sampler_run(ops, B, seed, **kw):
    m, gp = small_model_on_device(ops)
    x0 = t(np.array(SAMPLER["x"])).expand(B, 2).contiguous()
    uref = torch.full((B, 1), SAMPLER["u_ref"], **T64)
    ws, x, draw = run_sampled(ops, gp, x0, normals(B, seed), mean_model=SAMPLER["mean_model"], u_ref=uref,
                              max_unsafe_prob=SAMPLER["max_unsafe_prob"], **kw)
    return m, gp, x0, ws, x, draw


def risk_counters(ops, draw, ws):
    B = ws["status"].shape[0]
    viol, solved = torch.zeros(B, 1, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    min_cbc = torch.full((B, 1), float("inf"), **T64)
    ops.rollout_risk(draw["cbc_s"], ws["status"], viol, solved, min_cbc)
    torch.cuda.synchronize()
    return viol, solved, min_cbc


def test_sampler_on_the_device_has_the_exact_moments(ops):
    from _pendulum_oracle import oracle_step, pendulum_fg
    B = 4096
    m, gp, x0, ws, x, draw = sampler_run(ops, B, 21)
    xs = np.array(SAMPLER["x"])
    o = oracle_step(m, xs, dt=DT, u_ref=np.array([SAMPLER["u_ref"]]), mean_model=SAMPLER["mean_model"],
                    safety_factor=math.sqrt((1 - SAMPLER["max_unsafe_prob"]) / SAMPLER["max_unsafe_prob"]))
    assert o["status"] == "optimal" and (ws["status"] == 0).all(), "the program of this state is solved"
    u = host(ws["u"])[:, 0]
    assert (u == u[0]).all() and abs(u[0] - o["u"][0]) < 1e-6
    _, _, mean, S4, (h, gh, Hh) = ref.model_at(m, xs)
    f, g, J = pendulum_fg(xs, *SAMPLER["mean_model"])
    mean = mean + np.stack([f, g, J[:, 0], J[:, 1]], axis=1)
    m_ex, v_ex = ref.exact_moments(mean, m["A"], S4, u[0], h, gh, Hh, ref.K_ALPHA)
    assert m_ex > 0
    c = host(draw["cbc_s"])[:, 1]
    # standard errors: the mean's from the exact variance; the variance's from the fourth central moment of the same
    # quadratic form, taken from 200 000 draws of the numpy restatement (not from the device sample)
    cr = ref.cbc2_on(ref.draw(mean, m["A"], S4, np.random.default_rng(3).standard_normal((200000, 2, 4))), u[0], h, gh, Hh,
                     ref.K_ALPHA)[2]
    mu4 = float(((cr - cr.mean()) ** 4).mean())
    se_m, se_v = math.sqrt(v_ex / B), math.sqrt((mu4 - v_ex ** 2) / B)
    print("cbc2_s mean %.4f (exact %.4f, se %.4f)  var %.4f (exact %.4f, se %.4f)" % (c.mean(), m_ex, se_m, c.var(), v_ex, se_v))
    assert abs(c.mean() - m_ex) <= 6.0 * se_m and abs(c.var() - v_ex) <= 6.0 * se_v
    # one-sided Chebyshev (Cantelli) on the EXACT moments: holds for any distribution
    p = v_ex / (v_ex + m_ex ** 2)
    rate = float((c < 0).mean())
    print("violation rate %.4f, Cantelli bound %.4f (+ 4 sd %.4f)" % (rate, p, 4 * math.sqrt(p * (1 - p) / B)))
    assert rate <= p + 4.0 * math.sqrt(p * (1 - p) / B)
    viol, solved, min_cbc = risk_counters(ops, draw, ws)
    assert (solved == 1).all() and int(viol.sum()) == int((c < 0).sum()) and float(min_cbc.min()) == c.min()
    rho = host(ws["y"])[:, 1]
    assert torch.equal(draw["relaxed"].cpu(), torch.as_tensor(rho > 1e-6).to(torch.int32))
    assert torch.equal(draw["viol_relaxed"].cpu(), torch.as_tensor((rho > 1e-6) & ~(c >= 0)).to(torch.int32))


def test_unsolved_instance_is_driven_by_u_ref_on_the_draw(ops):
    B = 64
    m, gp, x0, ws, x, draw = sampler_run(ops, B, 22, max_iters=1)
    assert (ws["status"] != 0).all(), "one iteration does not solve the program"
    assert (ws["u"] == SAMPLER["u_ref"]).all()
    z = normals(B, 22)
    xd, cbc, xn = restate(ws, gp, "rbf", x0, z, u=np.full(B, SAMPLER["u_ref"]))
    close_to_restatement(draw, x, (xd, cbc, xn))
    assert np.abs(xd - host(ws["Mk"])[:, :, 0]).max() > 1e-3
    viol, solved, min_cbc = risk_counters(ops, draw, ws)
    assert not solved.any() and not viol.any() and torch.isinf(min_cbc).all()
    assert not draw["relaxed"].any() and not draw["viol_relaxed"].any()


def test_rollout_risk_counts_a_nan_condition_as_a_violation(ops):
    cbc = t(np.array([[0.0, 1.0], [0.0, float("nan")], [0.0, -2.0], [0.0, float("nan")]]))
    status = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=DEV)
    viol, solved, min_cbc = risk_counters(ops, dict(cbc_s=cbc), dict(status=status))
    assert viol[:, 0].tolist() == [0, 1, 1, 0] and solved.tolist() == [1, 1, 1, 0]
    assert min_cbc[:, 0].tolist() == [1.0, float("-inf"), -2.0, float("inf")]


# ---------------------------------------------------------------- 9. rollouts
def test_posterior_rollouts_graph_equals_eager_and_counters_recount(ops):
    from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
    _, gp = small_model_on_device(ops)
    B, steps = 64, 30
    kw = dict(numSteps=steps, gp=gp, shared=True, mean_model=(1.0, 10.0, 1.0), max_unsafe_prob=0.2, theta0=0.2, omega0=-0.3,
              seed=4, plant="posterior")
    eager = pendulum_safety_rollouts(B, **kw)
    graph = pendulum_safety_rollouts(B, use_graph=True, **kw)
    for k in ("x_final", "min_h", "fails"):
        assert torch.equal(eager[k], graph[k]), k
    assert eager["risk"] == graph["risk"]
    rec = pendulum_safety_rollouts(B, record=True, **kw)
    assert torch.equal(rec["x_final"], eager["x_final"]) and rec["risk"] == eager["risk"]
    ok = rec["status"] == 0
    c2 = rec["cbc_s"][:, :, 1]
    bad = ~(c2 >= 0)
    rel = ok & (rec["rho"] > 1e-6)
    r = rec["risk"]
    assert r["instance_steps"] == int(ok.sum()) > 0 and r["violations"] == int((ok & bad).sum())
    assert r["relaxed_steps"] == int(rel.sum()) and r["violations_relaxed"] == int((rel & bad).sum())
    assert r["min_cbc2"] == float(c2[ok].min()) and r["max_unsafe_prob"] == 0.2
    assert r["rate"] == r["violations"] / r["instance_steps"]
    assert r["rate_unrelaxed"] == (r["violations"] - r["violations_relaxed"]) / max(r["instance_steps"] - r["relaxed_steps"], 1)
    assert int(rec["fails"].sum()) == int((~ok).sum())
    other = pendulum_safety_rollouts(B, **dict(kw, seed=5))
    assert not torch.equal(other["x_final"], eager["x_final"])


def test_true_plant_rollouts_equal_a_loop_of_the_existing_entry(ops):
    from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
    _, gp = small_model_on_device(ops)
    B, steps = 48, 25
    r = pendulum_safety_rollouts(B, numSteps=steps, gp=gp, shared=True, mean_model=(1.0, 10.0, 1.0), seed=6)
    assert "risk" not in r
    gen = torch.Generator(device=DEV).manual_seed(6)
    x = (torch.tensor([7 * math.pi / 12, -0.01], **T64) + 0.05 * torch.randn(B, 2, generator=gen, **T64)).contiguous()
    ws = ops.pendulum_workspace(B, torch.float64, DEV)
    min_h = torch.full((B,), float("inf"), **T64)
    fails = torch.zeros(B, dtype=torch.int32, device=DEV)
    step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=(1.0, 10.0, 1.0), stats=(min_h, fails))
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    assert torch.equal(r["x_final"], x) and torch.equal(r["min_h"], min_h) and torch.equal(r["fails"], fails)


def test_learning_rollouts_learn_from_the_drawn_plant(ops):
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    B, steps = 16, 30
    m = ref.small_model()
    hyper = dict(ell=t(m["ell"])[None], s2=t(np.array([m["s2"]])), Bm=t(m["Bm"])[None], M0=t(m["M0"])[None], A=t(m["A"])[None])
    r = pendulum_learning_rollouts(B, numSteps=steps, train_every=20, plant="posterior", record=True, seed=2, hyper=hyper)
    assert r["report"]["refits"] == [(20, 19)] and r["risk"]["instance_steps"] == int((r["status"] == 0).sum())
    traj, Y, UH = r["traj"], r["rows"]["Y"], r["rows"]["UH"]
    assert torch.isfinite(traj).all() and torch.isfinite(r["cbc_s"]).all()
    xdot = ((traj[1:] - traj[:-1]) / DT).permute(1, 0, 2)                 # [B, T, 2]; no mean model: the rows are these
    still = (traj[1:, :, 0] - traj[:-1, :, 0]).abs().T < 1.0               # steps that do not wrap
    # (the kernel divides by dt; torch may multiply by its reciprocal: one rounding apart)
    assert torch.allclose(Y[still], xdot[still], rtol=1e-15, atol=0) and torch.equal(UH[:, :, 1], r["u"].T)
    true = torch.stack([traj[:-1, :, 1], -10.0 * torch.sin(traj[:-1, :, 0]) + r["u"]], dim=-1).permute(1, 0, 2)
    assert (Y - true)[still].abs().max() > 1e-2, "the rows record the drawn plant, not the true pendulum"
