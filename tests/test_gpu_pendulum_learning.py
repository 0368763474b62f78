"""bcbf_pendulum_control_step_observe_f64 / rollouts.pendulum_learning_rollouts on the MI355X: the pendulum's safety loop
that learns its dynamics online (ControlPendulumCBFLearned).  Observation rows, epsilon-greedy exploration, the GP prior
before the first refit, parity with the one-instance façade (ControlPendulumCBFLearned with replayed draws), the final
models against the CPU oracle, batch = single-instance runs, and a run at scale."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _pendulum_oracle import greedy, oracle_state

DEV = "cuda"
T64 = dict(dtype=torch.float64, device=DEV)
PEND = (1.0, 10.0, 1.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def host(v):
    return v.detach().cpu().double().numpy()


def _fixed_gp(ops, Bt, N=48, seed=21):
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(Bt, N, 2, 1, dtype=torch.float64, device=DEV, seed=seed)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    return dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=p["A"])


def _start_reg(seed=0):
    from bayesian_cbf_amd.control_affine_model import ControlAffineRegressor
    torch.manual_seed(seed)
    return ControlAffineRegressor(2, 1, device=DEV, dtype=torch.float64, gamma_length_scale_prior=(math.pi / 100, math.pi / 100))


def _crossing_starts(Bt, seed=3):
    """Half near theta0 = 7 pi / 12, half just below pi spinning up: those wrap across +-pi within a few steps."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.empty(Bt, 2, **T64)
    x[:, 0] = 7 * math.pi / 12 + 0.05 * torch.randn(Bt, generator=g, **T64)
    x[:, 1] = -0.01 + 0.05 * torch.randn(Bt, generator=g, **T64)
    h = Bt // 2
    x[h:, 0] = math.pi - 0.03 * torch.rand(Bt - h, generator=g, **T64)
    x[h:, 1] = 4.0 + torch.rand(Bt - h, generator=g, **T64)
    return x


# ---------------------------------------------------------------- 1. observation rows
@pytest.mark.parametrize("mean", [None, PEND], ids=["zero_mean", "pendulum_mean"])
def test_rows_are_the_recorded_finite_differences(mean):
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    B, T = 64, 40
    r = pendulum_learning_rollouts(B, numSteps=T, train_every=10, max_train=24, mean_model=mean, record=True,
                                   x0=_crossing_starts(B), seed=1)
    traj, u = r["traj"], r["u"]
    th0 = traj[:T, :, 0]
    assert int(((traj[1:, :, 0] - th0).abs() > math.pi).sum()) >= 1                     # some instance wrapped at +-pi
    X, UH, Y = (r["rows"][k].transpose(0, 1) for k in ("X", "UH", "Y"))                   # [T, B, 2]
    assert torch.equal(X, traj[:T])
    assert torch.equal(UH[..., 0], torch.ones_like(u)) and torch.equal(UH[..., 1], u)
    fd = (traj[1:] - traj[:T]) / 0.002
    mean_rows = torch.zeros_like(fd)
    if mean is not None:
        m, g, l = mean
        mean_rows[..., 0] = traj[:T, :, 1]
        mean_rows[..., 1] = -(g / l) * torch.sin(th0) + u / (m * l)
    np.testing.assert_allclose(host(Y), host(fd - mean_rows), rtol=1e-13, atol=1e-12)
    assert float(Y[..., 0].abs().max()) > 2 * math.pi / 0.002 * 0.9                      # the wrap's ~2 pi / dt target


# ---------------------------------------------------------------- 2. exploration
def test_exploration_wraps_the_greedy_control(ops):
    B = 512
    gp = _fixed_gp(ops, B)
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.stack([torch.empty(B, **T64).uniform_(-1.5, 0.2, generator=g),
                     torch.empty(B, **T64).uniform_(-1.0, 1.0, generator=g)], dim=1).contiguous()
    x0 = host(x)
    explore = torch.rand(B, 2, generator=g, **T64)
    lo, hi, eps = -0.5, 0.7, 0.4
    ws = ops.pendulum_workspace(B, torch.float64, DEV)
    step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=PEND, explore=explore, eps=eps, ctrl_range=(lo, hi))
    step()
    torch.cuda.synchronize()
    Mk, uref, ex = host(ws["Mk"]), host(ws["u_ref"])[:, 0], host(explore)
    coin = ex[:, 0] < eps
    assert 0 < coin.sum() < B
    n_clipped = 0
    for i in range(B):
        gr = greedy(x0[i], Mk[i][:, 0], Mk[i][:, 1], 0.002)[0]
        want = lo + ex[i, 1] * (hi - lo) if coin[i] else gr
        n_clipped += int(not coin[i] and not (lo <= gr <= hi))
        want = max(min(want, hi), lo)
        np.testing.assert_allclose(uref[i], want, rtol=1e-12, atol=1e-12, err_msg=str(i))
    assert n_clipped > 0


def test_observe_entry_without_exploration_equals_safety_rollouts(ops):
    from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
    B, T = 128, 60
    gp = _fixed_gp(ops, B)
    ref = pendulum_safety_rollouts(B, numSteps=T, gp=gp, mean_model=PEND, seed=4, record=True)
    x = ref["traj"][0].clone()
    ws = ops.pendulum_workspace(B, torch.float64, DEV)
    min_h = torch.full((B,), float("inf"), **T64)
    fails = torch.zeros(B, dtype=torch.int32, device=DEV)
    step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=PEND, stats=(min_h, fails), observe=True)
    rows = [torch.zeros(B, T, 2, **T64) for _ in range(3)]
    for t in range(T):
        step(obs=(rows[0][:, t], rows[1][:, t], rows[2][:, t], T))
        assert torch.equal(x, ref["traj"][t + 1]), t
    torch.cuda.synchronize()
    assert torch.equal(min_h, ref["min_h"]) and torch.equal(fails, ref["fails"])
    assert torch.equal(ws["u"][:, 0], ref["u"][T - 1])
    assert torch.equal(rows[0], ref["traj"][:T].transpose(0, 1))


# ---------------------------------------------------------------- 3. prior mode
@pytest.mark.parametrize("mean", [None, PEND], ids=["zero_mean", "pendulum_mean"])
def test_prior_mode_equals_socp_facade_on_untrained_regressor(ops, mean):
    from bayesian_cbf_amd.controllers import GreedyController, SOCPController, SumDynamicModels
    from bayesian_cbf_amd.pendulum import PendulumDynamicsModel, RadialCBFRelDegree2
    from bayesian_cbf_amd.unicycle_move_to_pose import ZeroDynamicsModel
    reg = _start_reg(seed=2)
    md = ZeroDynamicsModel(m=1, n=2) if mean is None else PendulumDynamicsModel(m=1, n=2, mass=1.0, gravity=10.0,
                                                                                 length=1.0, dtype=torch.float64)
    net = SumDynamicModels(reg, md)
    cbf = RadialCBFRelDegree2(net, dtype=torch.float64)
    dt = 0.002
    gr = GreedyController(net, torch.eye(2, **T64), torch.eye(1, **T64), torch.zeros(2, **T64), 250, dt, None)
    ctrl = SOCPController(2, 1, 1.0, 100.0, net, [cbf], None, gr)
    g = torch.Generator(device=DEV).manual_seed(6)
    xs = torch.stack([torch.empty(32, **T64).uniform_(-2.0, 3.0, generator=g),
                      torch.empty(32, **T64).uniform_(-2.0, 2.0, generator=g)], dim=1).contiguous()
    u_f = ctrl.control(xs.clone())
    ws = ops.pendulum_workspace(32, torch.float64, DEV)
    x = xs.clone()
    step = ops.pendulum_control_step_prepare(reg._hyper(), ws, x, mean_model=mean, dt=dt, prior=True)
    step()
    torch.cuda.synchronize()
    assert torch.equal(ws["status"].cpu(), ctrl.last_status.cpu().to(torch.int32))
    np.testing.assert_allclose(host(ws["u"]), host(u_f), rtol=1e-9, atol=1e-9)
    hp = reg._hyper()
    np.testing.assert_allclose(host(ws["Bk"]), host((hp["s2"][:, None, None] * hp["Bm"]).expand(32, 2, 2)), rtol=1e-15)


# ---------------------------------------------------------------- 4. façade parity
def _facade_run(i, r, T, train_every, max_train, fit_iters, start):
    """Instance i of the batched run `r`, replayed through ControlPendulumCBFLearned(enable_learning=True) with the same
    draws: explore through a test-local epsilon-greedy subclass, the subset through `_learner.subsample`, the jitter (and
    the fit's draws) through the regressor's `rand_fn` / `target_rand_fn`."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.controllers import EpsilonGreedyController, clip, epsilon
    from bayesian_cbf_amd.pendulum import ControlPendulumCBFLearned
    from bayesian_cbf_amd.rollouts import pendulum_learning_schedule
    dr = r["draws"]
    ex = host(dr["explore"][:, i])

    class Replay(EpsilonGreedyController):
        def control(self, x, t=None):
            lo, hi = (float(v) for v in self.ctrl_range)
            eps = epsilon(t, interpolate={0: self.egreedy_scheme[0], self.numSteps: self.egreedy_scheme[1]})
            u0 = self.base_controller.control(x, t=t)
            ue = torch.full_like(u0, lo + ex[t, 1] * (hi - lo)) if ex[t, 0] < eps else u0
            return clip(ue, torch.as_tensor(lo).to(u0), torch.as_tensor(hi).to(u0))

    reg = _start_reg(seed=0)
    reg.model.load_state_dict(start.model.state_dict())
    sched = pendulum_learning_schedule(T, train_every, max_train)
    jit, tgt, idx = [], [], []
    for (t, count, wr), rd in zip(sched, dr["refits"]):
        for it in range(fit_iters):
            jit.append(rd["fit_jitter"][it][i])
            tgt.append(rd["fit_target"][it][i])
        jit.append(rd["jitter"][i])
        if wr:
            idx.append(rd["idx"][i])
    jit_it, tgt_it, idx_it = iter(jit), iter(tgt), iter(idx)
    reg.rand_fn = lambda k: next(jit_it)[:k].to(**T64)
    reg.target_rand_fn = lambda Y: next(tgt_it).to(**T64)
    fac = ControlPendulumCBFLearned(dt=0.002, numSteps=T, train_every_n_steps=train_every, max_train=max_train,
                                    iterations=fit_iters, enable_learning=True, model=reg, exploration_controller_class=Replay,
                                    device=DEV)
    fac.net_model._learner.subsample = lambda count, k: next(idx_it)
    x = r["traj"][0, i:i + 1].clone()
    xs, us, st = [x.clone()], [], []
    for t in range(T):
        u = fac.control(x.clone(), t=t).reshape(1, 1).contiguous()
        st.append(int(fac.last_status[0]))
        us.append(float(u[0, 0]))
        ops.pendulum_plant_step(x, u, *PEND, 0.002)
        xs.append(x.clone())
    torch.cuda.synchronize()
    assert next(jit_it, None) is None and next(idx_it, None) is None          # every recorded draw was consumed
    return torch.cat(xs).cpu().numpy(), np.array(us), np.array(st), reg


@pytest.mark.parametrize("fit_iters", [0, 3])
def test_batched_loop_equals_learning_facade(fit_iters):
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    B, T, every, mt = 8, 40, 10, 24
    start = _start_reg(seed=0)
    r = pendulum_learning_rollouts(B, numSteps=T, train_every=every, max_train=mt, fit_iters=fit_iters, hyper=start,
                                   record=True, seed=12)
    rep = r["report"]
    assert rep["refits"] == [(10, 9), (20, 19), (30, 24)]
    assert rep["instances_factored_per_retry_level"][1:] == [0] * (len(rep["instances_factored_per_retry_level"]) - 1)
    assert rep["refit_failures_after_retries"] == 0
    traj, u, status = host(r["traj"]), host(r["u"]), r["status"].cpu().numpy()
    # Tolerances: the models hold 9 .. 24 consecutive states 2 ms apart with make_psd's 1e-5 jitter, cond(K_b) ~ 1e9 .. 1e10,
    # so two implementations of the posterior (jets kernel here, the façade's prediction there) agree to ~1e-16 cond only;
    # at a few near-degenerate programs the cone solver then moves u by up to ~2e-3 for one step, and the instance drifts
    # (measured: trajectories within 5e-5 over the 40 steps; in prior mode, steps 0 .. 10, u agrees to 1e-14).
    for i in range(B):
        xs, us, st = _facade_run(i, r, T, every, mt, fit_iters, start)[:3]
        assert (status[:, i] == st).all(), i
        du = np.abs(u[:, i] - us)
        assert du[:11].max() < 1e-9, (i, du)
        np.testing.assert_allclose(traj[:, i], xs, rtol=2e-4, atol=2e-4, err_msg="trajectory %d" % i)
        assert np.quantile(du, 0.75) < 1e-4, (i, du)
    if fit_iters:
        # the batched fit carried the hyper-parameters from refit to refit like the façade's module: compare the last
        # instance's (reg of the last façade run) raw parameters through their derived values
        _, _, _, reg = _facade_run(B - 1, r, T, every, mt, fit_iters, start)
        hp = reg._hyper()
        fin = r["final"]["hyper"]
        for k in ("ell", "s2", "Bm", "M0", "A"):
            np.testing.assert_allclose(host(fin[k][B - 1]), host(hp[k][0]), rtol=1e-5, atol=1e-7, err_msg=k)
        assert float((fin["ell"] - start._hyper()["ell"]).abs().max()) > 1e-3                # the fit moved them


# ---------------------------------------------------------------- 5. final model
def test_final_models_equal_oracle_posterior_of_their_rows(capsys):
    from bayesian_cbf_amd import ops
    from oracle import cbc2 as oc2
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    B, T = 1024, 100
    r = pendulum_learning_rollouts(B, numSteps=T, record=True, seed=5)
    assert r["report"]["refits"][-1] == (90, 89)
    fin, gp = r["final"]["rows"], r["final"]["gp"]
    pick = torch.randperm(B, generator=torch.Generator().manual_seed(0))[:16].tolist()
    xq = torch.tensor([[7 * math.pi / 12, -0.01], [0.3, 0.5], [2.0, -1.0]], **T64)
    worst = 0.0
    for i in pick:
        h = {k: host(v[i]) for k, v in fin.items()}
        hp = {k: host(v[i]) for k, v in r["final"]["hyper"].items()}
        st = oracle_state(h["X"], h["UH"], h["Y"], hp["Bm"], hp["ell"], float(hp["s2"]), hp["M0"], h["jitter"], hp["A"])
        gi = {k: v[i:i + 1].contiguous() for k, v in gp.items()}
        for q in host(xq):
            jets = oc2.posterior_jets(st["L"], st["Y"], st["X"], st["UHB"], st["ell"], st["s2"], st["Bm"], st["M0"], q)
            xb = torch.tensor(q, **T64)[None].contiguous()
            Mk, Bk, _, _ = ops.posterior_jets(gi["Lop"], gi["Vw"], gi["X"], gi["UHB"], gi["ell"], gi["s2"], gi["Bm"],
                                              gi["M0"], xb, shared=True)
            # the rows are consecutive states 2 ms apart: cond(K_b) reaches ~1e10, and two factorisations of the same
            # system agree to ~eps cond(K_b) relative to the prior scale, not better (1e-9 where K_b is well conditioned)
            tol = max(1e-9, 10 * np.finfo(np.float64).eps * np.linalg.cond(st["L"]) ** 2)
            scale = max(1.0, float(np.abs(jets["Mk"]).max()))
            np.testing.assert_allclose(host(Mk[0]), jets["Mk"], rtol=tol, atol=tol * scale, err_msg="Mk %d" % i)
            np.testing.assert_allclose(host(Bk[0]), jets["Bk"], rtol=tol, atol=tol * float(hp["s2"]), err_msg="Bk %d" % i)
            worst = max(worst, float(np.abs(host(Mk[0]) - jets["Mk"]).max() / scale))
    with capsys.disabled():
        print("\nfinal models vs oracle: worst |dMk| / scale %.2e" % worst)


# ---------------------------------------------------------------- 6. batch = single
def test_batch_instance_equals_single_instance_run():
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    B, T = 256, 60
    kw = dict(numSteps=T, train_every=10, max_train=24, hyper=_start_reg(seed=0))
    r = pendulum_learning_rollouts(B, record=True, seed=8, **kw)
    dr = r["draws"]
    for i in (0, 101, 255):
        sl = dict(explore=dr["explore"][:, i:i + 1],
                  refits=[dict(idx=None if d["idx"] is None else d["idx"][i:i + 1], jitter=d["jitter"][i:i + 1]) for d in dr["refits"]])
        one = pendulum_learning_rollouts(1, record=True, draws=sl, x0=r["traj"][0, i:i + 1], **kw)
        assert torch.equal(one["traj"][:, 0], r["traj"][:, i]), i
        assert torch.equal(one["u"][:, 0], r["u"][:, i]) and torch.equal(one["status"][:, 0], r["status"][:, i]), i


# ---------------------------------------------------------------- 7. scale
def test_scale_run_4096(capsys):
    from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts
    B = 4096
    on = pendulum_learning_rollouts(B, numSteps=250, fit_iters=0, seed=0)
    off = pendulum_learning_rollouts(B, numSteps=250, learning=False, seed=0)
    for r in (on, off):
        assert torch.isfinite(r["x_final"]).all()
        assert r["stats"]["count"] == B
        assert isinstance(r["report"]["refit_failures_after_retries"], int)
    assert len(on["report"]["refits"]) == 24 and off["report"]["refits"] == []
    with capsys.disabled():
        print("\npendulum learning loop, 4096 x 250: learning on %s / %s;  off %s / %s"
              % (on["stats"], {k: on["report"][k] for k in ("instance_steps_per_s", "refit_ms_per_refit",
                                                            "refit_failures_after_retries", "solver_optimal_fraction")},
                 off["stats"], {k: off["report"][k] for k in ("instance_steps_per_s", "solver_optimal_fraction")}))
