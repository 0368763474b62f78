"""CPU-side checks of the self-triggering interval (bayesian_cbf_amd/trigger_interval.py, bcbf_trigger_interval): the numpy
yardstick tests/_trigger_reference.py against the results the reference recorded for its committed learning run, the reference's
helper functions, ObstacleCBF.cbf / grad_cbf, and the entry points' argument checks (refused before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _trigger_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ti(lib):
    from bayesian_cbf_amd import trigger_interval
    return trigger_interval


def test_numpy_restatement_reproduces_the_recorded_results_at_all_200_steps():
    """Lfh, xvel and tau of the helper, fed the committed log, against the reference's own Lfh.np.txt / xvel.np.txt / tau.np.txt:
    1e-6 relative (the float32-logged inputs bound what can agree)."""
    G = np.load(os.path.join(GOLDEN, "saved_run_learning_v1p6p3.npz"))
    F = np.load(os.path.join(GOLDEN, "trigger_interval_v1p6p3.npz"))
    for k in ("Lfh", "tau", "xvel", "Lfh_num", "tau_num"):
        assert F[k].shape == (200,) and F[k].dtype == np.float64
    got = R.saved_run(G)
    for k in ("Lfh", "xvel", "tau"):
        err = np.max(np.abs(got[k] - F[k]) / np.abs(F[k]))
        print("%s: worst relative error %.3e" % (k, err))
        assert err <= 1e-6, (k, err)


def test_grid_and_its_norm(ti):
    grid = ti.ndgridj([-0.1, -0.1, -np.pi / 100], [0.1, 0.1, np.pi / 100], 9 * np.ones(3))
    assert grid.shape == (729, 3)
    assert np.array_equal(grid, ti.default_test_grid(3)) and np.allclose(grid, R.grid(), rtol=0, atol=1e-16)
    np.testing.assert_array_equal(grid[0], [-0.1, -0.1, -np.pi / 100])
    np.testing.assert_array_equal(grid[1, :2], [-0.1, -0.1])                 # the last axis runs fastest
    assert abs(ti.pdist(grid) - 96.40769006) <= 1e-9
    assert abs(ti._grid_norm(grid) - ti.pdist(grid)) <= 1e-12 * 96.4
    pts = np.random.default_rng(0).normal(size=(37, 2))
    assert abs(ti._grid_norm(pts) - ti.pdist(pts)) <= 1e-12 * ti.pdist(pts)


def test_kernel_derivative_helpers(ti):
    rng = np.random.default_rng(1)
    x, xp, ls, sf = rng.normal(size=(50, 3)), rng.normal(size=(50, 3)), np.array([0.7, 1.3, 2.1]), 0.9
    k = sf ** 2 * np.exp(-0.5 * (((x - xp) / ls) ** 2).sum(1))
    np.testing.assert_allclose(ti.rbf_knl(x, xp, sf, ls), k, rtol=1e-14)
    for i in range(3):
        d1 = ti.rbf_d_knl_d_x_xp_i(x, xp, i, sf, ls)
        np.testing.assert_allclose(d1, -(x[:, i] - xp[:, i]) / ls[i] ** 2 * k, rtol=1e-14)
        np.testing.assert_allclose(ti.rbf_d3_knl_d_x_xp_i(x, xp, i, sf, ls), -2 * ls[i] ** (-2) * d1, rtol=1e-15)
        # d1 is the derivative in x_i; d2 is MINUS the second derivative in x_i (= d^2 k / dx_i dx'_i): central differences
        h = 1e-5
        e = np.zeros(3)
        e[i] = h
        np.testing.assert_allclose(d1, (ti.rbf_knl(x + e, xp, sf, ls) - ti.rbf_knl(x - e, xp, sf, ls)) / (2 * h), rtol=1e-6, atol=1e-9)
        fd2 = (ti.rbf_d_knl_d_x_xp_i(x + e, xp, i, sf, ls) - ti.rbf_d_knl_d_x_xp_i(x - e, xp, i, sf, ls)) / (2 * h)
        np.testing.assert_allclose(ti.rbf_d2_knl_d_x_xp_i(x, xp, i, sf, ls), -fd2, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(ti.rbf_d2_knl_d_x_xp_i(x, x, i, sf, ls), sf ** 2 / ls[i] ** 2, rtol=1e-15)


def test_numerical_lipschitz_estimate_with_given_draws(ti):
    rng = np.random.default_rng(2)
    X, ls, sf, w = rng.normal(size=(40, 3)), np.array([0.5, 0.8, 1.1]), 1.3, rng.normal(size=40)
    Lf, prob = ti.numerical_lipschitz_estimate(X, 1, sf, ls, 0.7, 2.5, w=w)
    sigma = 0.7 * 2.5 * sf ** 2 / ls[1] ** 2                       # the same at every point: x == x'
    i = np.argmax(np.abs(w))
    assert abs(Lf - abs(w[i]) * sigma) <= 1e-14 * Lf
    assert abs(prob - np.exp(-w[i] ** 2 / 2) / np.sqrt(2 * np.pi) * 1e-2) <= 1e-16
    Lf2, prob2 = ti.numerical_lipschitz_estimate(X, 1, sf, ls, 0.7, 2.5)        # unseeded draws: finite and positive
    assert np.isfinite(Lf2) and Lf2 > 0 and 0 < prob2 <= 1e-2 / np.sqrt(2 * np.pi)


def test_obstacle_cbf_gradient_single_state_and_batch(lib):
    from bayesian_cbf_amd.unicycle_move_to_pose import ObstacleCBF
    c, rad, w = np.array([-1.2, 0.4]), 0.6, (0.7, 0.3)
    h = ObstacleCBF(c, rad, term_weights=w)
    s = np.array([-2.9, -0.8, 0.3])
    assert abs(float(h.cbf(torch.from_numpy(s))) - R.cbf(c, rad, w, s)) <= 1e-14
    g = h.grad_cbf(torch.from_numpy(s)).numpy()
    assert g.shape == (3,)
    e = 1e-6
    fd = np.array([(R.cbf(c, rad, w, s + e * np.eye(3)[k]) - R.cbf(c, rad, w, s - e * np.eye(3)[k])) / (2 * e) for k in range(3)])
    np.testing.assert_allclose(g, fd, rtol=1e-7, atol=1e-9)
    # a batch [Nte, 3]: rho over the whole batch, as the reference's torch.norm takes it
    X = R.grid() + s
    np.testing.assert_allclose(h.grad_cbf(torch.from_numpy(X)).numpy(), R.grad_cbf(c, w, X), rtol=1e-13, atol=1e-15)
    assert not np.allclose(h.grad_cbf(torch.from_numpy(X)).numpy()[0], h.grad_cbf(torch.from_numpy(X[0])).numpy(), rtol=1e-3)
    # [B, Nte, 3]: rho per instance
    X2 = np.stack([X, R.grid() + np.array([-1.0, 0.2, -0.4])])
    G2 = h.grad_cbf(torch.from_numpy(X2)).numpy()
    for b in range(2):
        np.testing.assert_allclose(G2[b], R.grad_cbf(c, w, X2[b]), rtol=1e-13, atol=1e-15)
    assert h.cbf(torch.from_numpy(X2)).shape == (2, 729)


def test_default_obstacles_match_the_yardstick(ti):
    for h, (c, rad, w) in zip(ti._DEFAULT_CBFS(), R.default_obstacles()):
        np.testing.assert_allclose(h.center.numpy(), c, rtol=2e-7)
        assert h.center.dtype == torch.float64 and tuple(h.term_weights) == w


GOOD = dict(B=5, Bh=5, Nte=64, n=3)
BAD = [(dict(Nte=0), "Nte < 1"), (dict(Nte=-3), "Nte < 1"), (dict(n=0), "1 <= n <= 3"), (dict(n=4), "1 <= n <= 3"), (dict(B=0, Bh=0), "B < 1"),
       (dict(Bh=2), "Bh must be 1 or B"), (dict(null=12), "null output"), (dict(null=14), "null output"), (dict(null=1), "null input"),
       (dict(Nte=1 << 20), "Nte too large")]


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("change,why", BAD, ids=["%s-%s" % (w, "-".join("%s%s" % kv for kv in c.items())) for c, w in BAD])
def test_bad_arguments_are_refused_with_a_reason_and_no_launch(lib, suf, change, why):
    """Every case fails the host check, so the fake pointers are never used and no GPU is touched."""
    a = dict(GOOD, **change)
    ptr = [ctypes.c_void_p(4096 * (k + 1)) for k in range(15)]           # argument positions 0-7 inputs, 12-14 outputs
    if "null" in a:
        ptr[a["null"]] = None
    fn = getattr(lib.lib, "bcbf_trigger_interval" + suf)
    rc = fn(*ptr[:8], 96.4, 1e-4, 1e-2, 1.0, ptr[12], ptr[13], ptr[14], a["B"], a["Bh"], a["Nte"], a["n"], None)
    assert rc < 0
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_trigger_interval" + suf) and why in msg, msg


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bcbf.h")).read()
    for name in ("bcbf_trigger_interval_f32", "bcbf_trigger_interval_f64"):
        assert name + "(" in header and name in lib.declared_symbols() and hasattr(lib.lib, name)


def test_ops_and_module_refuse_cpu_tensors_and_other_kernels(ti):
    from bayesian_cbf_amd import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.trigger_interval(z(2, 3), z(8, 3), z(1, 3), z(1), z(1, 3), z(2), z(2), z(2), 1.0)
    for kind in (1, 2, "matern52", "rbf_matern52"):
        with pytest.raises(ValueError, match="RBF data kernel"):
            ti.trigger_interval_batch(z(2, 3), z(2, 3), z(2, 2), z(3), z(()), z(3, 3), z(3, 3), None, 0.01, kernel_kind=kind)
        with pytest.raises(ValueError, match="RBF data kernel"):
            ti.unicycle_trigger_interval_compute("no-such-file", {}, kernel_kind=kind)
