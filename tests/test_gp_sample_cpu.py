"""CPU tests of the sampling surface: GaussianProcessBase.sample / DeterministicGP.sample (gp_algebra.py:33-34, :99-100 of the
reference) draw for draw against torch's MultivariateNormal, the one-instance posterior-sampled plant for
`sample_generator_trajectory`, the reduction of the risk statistics, and the C ABI of the batched counterpart."""
import math
import os

import numpy as np
import pytest
import torch

from bayesian_cbf_amd import gp_algebra as ga

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = dict(dtype=torch.float64)
K3 = torch.tensor([[2.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 0.5]], **F64)
X = torch.tensor([0.1, 0.2, 0.3], **F64)


def _leaf():
    return ga.GaussianProcess(mean=lambda x: torch.sin(x), knl=lambda x, xp: K3 * torch.exp(-0.5 * ((x - xp) ** 2).sum()),
                              shape=(3,), name="leaf")


def _processes():
    leaf = _leaf()
    grad = ga.DeterministicGP(lambda x: torch.tensor([1.0, 2.0, -1.0], **F64) * x, shape=(3,))
    off = ga.DeterministicGP(lambda x: 2.0 * x[:1], shape=(1,))
    return dict(leaf=leaf, add=leaf + leaf * 0.5, matmul=grad.t() @ leaf + off)


@pytest.mark.parametrize("shape", [(), (5,)], ids=["one", "five"])
@pytest.mark.parametrize("which", ["leaf", "add", "matmul"])
def test_sample_is_torchs_multivariate_normal_draw_for_draw(which, shape):
    gp = _processes()[which]
    mean, knl = torch.as_tensor(gp.mean(X)), torch.as_tensor(gp.knl(X, X))
    k = 1 if mean.dim() == 0 else mean.shape[0]
    torch.manual_seed(17)
    want = torch.distributions.MultivariateNormal(mean.reshape(k), knl.reshape(k, k)).sample(torch.Size(shape))
    torch.manual_seed(17)
    got = gp.sample(X, torch.Size(shape))
    assert got.shape == torch.Size(shape) + (k,)
    assert torch.equal(got, want)
    if shape == ():
        torch.manual_seed(17)
        assert torch.equal(gp.sample(X), want)                          # the default sample_shape


@pytest.mark.parametrize("shape", [(), (5,)], ids=["one", "five"])
def test_deterministic_gp_sample_is_the_expanded_mean(shape):
    det = ga.DeterministicGP(lambda x: torch.cos(x), shape=(3,))
    state = torch.get_rng_state()
    got = det.sample(X, torch.Size(shape))
    assert torch.equal(torch.get_rng_state(), state)                    # nothing is drawn
    assert got.shape == torch.Size(shape) + (3,)
    assert torch.equal(got, torch.cos(X).expand(*shape, 3))


def _model():
    from bayesian_cbf_amd.unicycle_move_to_pose import AckermannDrive
    return AckermannDrive(L=1.5, kernel_diag_A=(1e-2, 4e-2, 0.0))      # positive SEMIdefinite: no draw along theta


def test_posterior_sampled_dynamics_step_is_mean_plus_factor_times_the_draw():
    from bayesian_cbf_amd.unicycle_move_to_pose import PosteriorSampledDynamics, semidefinite_cholesky
    model = _model()
    plant = PosteriorSampledDynamics(model, x0=X, generator=torch.Generator().manual_seed(5))
    assert (plant.ctrl_size, plant.state_size) == (2, 3)
    assert torch.equal(plant.f_func(X), model.f_func(X)) and torch.equal(plant.g_func(X), model.g_func(X))
    u, dt = torch.tensor([0.7, -0.3], **F64), 0.05
    obs = plant.step(u, dt)
    z = torch.randn(3, generator=torch.Generator().manual_seed(5), **F64)
    gp = model.fu_func_gp(u)
    Kx = gp.knl(X, X)
    L = semidefinite_cholesky(Kx)
    assert torch.equal(L, torch.tril(L)) and float(L[2, 2]) == 0.0
    np.testing.assert_allclose((L @ L.t()).numpy(), Kx.numpy(), rtol=0, atol=1e-15)
    s = 1.0 + float(u @ u)                                              # ubar' I ubar
    np.testing.assert_allclose(torch.diagonal(L).numpy(), np.sqrt(s * np.array([1e-2, 4e-2, 0.0])), rtol=1e-14)
    want = gp.mean(X) + L @ z
    np.testing.assert_allclose(obs["xdot"].numpy(), want.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(obs["x"].numpy(), (X + want * dt).numpy(), rtol=0, atol=1e-12)
    assert float(obs["xdot"][2]) == float(gp.mean(X)[2])                # the null direction of A carries the mean alone
    assert torch.equal(plant.current_state, obs["x"])
    full = semidefinite_cholesky(K3)                                    # positive definite: the ordinary factor
    np.testing.assert_allclose(full.numpy(), torch.linalg.cholesky(K3).numpy(), rtol=0, atol=1e-14)
    lead = semidefinite_cholesky(torch.diag(torch.tensor([0.0, 1.0, 4.0], **F64)))          # a zero FIRST pivot
    assert torch.equal(lead, torch.diag(torch.tensor([0.0, 1.0, 2.0], **F64)))


def test_posterior_sampled_dynamics_under_sample_generator_trajectory():
    from bayesian_cbf_amd.sampling import sample_generator_trajectory
    from bayesian_cbf_amd.unicycle_move_to_pose import PosteriorSampledDynamics
    D, dt = 5, 0.02
    ctrl = lambda x, t=0: torch.tensor([0.5 + 0.1 * t, math.sin(0.3 * t)], **F64)
    run = lambda seed: sample_generator_trajectory(PosteriorSampledDynamics(_model(), generator=torch.Generator().manual_seed(seed)),
                                                   D, dt=dt, x0=X, controller=ctrl)
    Xdot, Xs, U = run(9)
    assert Xdot.shape == (D, 3) and Xs.shape == (D + 1, 3) and U.shape == (D, 2)
    assert torch.equal(Xs[0], X)
    for t in range(D):
        assert torch.equal(Xs[t + 1], Xs[t] + Xdot[t] * dt)
    Xdot2, Xs2, _ = run(9)
    assert torch.equal(Xs, Xs2) and torch.equal(Xdot, Xdot2)            # the supplied generator decides the draws
    assert not torch.equal(run(10)[1], Xs)
    mean = torch.stack([_model().g_func(Xs[t]) @ U[t] for t in range(D)])
    assert float((Xdot - mean)[:, :2].abs().min()) > 0 and torch.equal(Xdot[:, 2], mean[:, 2])


def test_reduce_risk_stats_single_process():
    from bayesian_cbf_amd.distributed import reduce_risk_stats
    out = reduce_risk_stats(torch.tensor(200), torch.tensor([7, 13], dtype=torch.int32), torch.tensor([-0.5, 0.25]), 0.05)
    assert out == dict(instance_steps=200, violations=20, rate=20 / 400, max_risk=0.05,
                       per_obstacle=[dict(violations=7, rate=7 / 200), dict(violations=13, rate=13 / 200)], min_cbc=[-0.5, 0.25])
    empty = reduce_risk_stats(0, [0, 0], [float("inf")] * 2, 0.2)
    assert empty["rate"] == 0.0 and empty["instance_steps"] == 0 and empty["min_cbc"] == [float("inf")] * 2


def test_sampled_step_and_risk_entries_are_declared_exported_and_refuse_bad_arguments():
    import re
    import subprocess
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for base in ("bcbf_unicycle_control_step_sampled", "bcbf_rollout_risk"):
        for suf in ("_f32", "_f64"):
            name = base + suf
            assert name + "(" in header and name in _lib.declared_symbols() and name in exported
    # Bt > 0 with z == NULL / a kernel_kind that does not exist / no counters: refused before anything is launched
    n = [None] * 13 + [0.0] + [None] * 4 + [1.0] + [None] * 16 + [0.05, 1.0, 4, 0, 2, 10, 0] + [None] * 4 + [1, None, 1]
    assert _lib.lib.bcbf_unicycle_control_step_sampled_f64(*n, 0, None, None, None, None, None, None) == -1
    assert _lib.lib.bcbf_rollout_risk_f32(None, None, None, None, None, 4, 2, None) == -1
    assert _lib.lib.bcbf_rollout_risk_f32(None, None, None, None, None, 0, 2, None) == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rollout_risk(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32),
                         torch.zeros(4, dtype=torch.int32), torch.zeros(4, 2))
