"""CPU-side checks of the LQR nominal controller (bcbf_lqr_nominal_f32 / _f64, bcbf_pendulum_control_step_nominal_f64): the
numpy restatement the GPU tests hold the kernel to (tests/_lqr_reference.py) reproduces what the reference's own code recorded
(tests/golden/lqr_nominal.npz) and, at a long horizon, the stabilising solution of the discrete algebraic Riccati equation
(scipy -- the check of the formula that shares nothing with the reference); the header declares and the library exports the
entry points; every bad argument is refused with BCBF_EINVAL before any HIP call."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _lqr_reference as lqr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "lqr_nominal.npz"))
NEW = ("bcbf_lqr_nominal_f32", "bcbf_lqr_nominal_f64", "bcbf_pendulum_control_step_nominal_f64")


def own_rel(actual, desired, rtol, what):
    sc = max(np.abs(desired).max(), 1e-300)
    err = np.abs(np.asarray(actual) - desired).max()
    assert err <= rtol * sc, "%s: %.3e > %.1e * %.3e" % (what, err, rtol, sc)


# ---------------------------------------------------------------- the helper against the reference's recorded numbers
@pytest.mark.parametrize("nm", [(2, 1), (3, 2), (4, 3)], ids=lambda v: "n%dm%d" % v)
@pytest.mark.parametrize("T", [1, 2, 3, 64])
def test_recursion_matches_reference_affine_backpropagation(nm, T):
    tag = "a_%d%d_" % nm
    P, o, K, k, ok = lqr.recursion(G[tag + "A"], G[tag + "B"], G[tag + "Q"], G[tag + "R"], G[tag + "s"], T)
    assert ok
    for name, v in (("P", P), ("o", o), ("K", K), ("k", k)):
        own_rel(v, G["%sT%d_%s" % (tag, T, name)], 1e-12, name)


def pendulum_jets(x, mass=1.0, gravity=10.0, length=1.0):
    """Mk[Bt,2,2], Mj[Bt,2,6] of the pendulum (what the step's task kernel writes in the no-GP mode)."""
    th, om = x[:, 0], x[:, 1]
    Mk, Mj = np.zeros((len(x), 2, 2)), np.zeros((len(x), 2, 6))
    Mk[:, 0, 0], Mk[:, 1, 0], Mk[:, 1, 1] = om, -(gravity / length) * np.sin(th), 1.0 / (mass * length)
    Mj[:, 0, 4] = 1.0
    Mj[:, 1, 2] = -(gravity / length) * np.cos(th)
    return Mk, Mj


def xdependent_jets(x):
    """The jets of golden (c)'s model: the pendulum's f (g/l = 10), g = [0.1 sin theta, 1 + 0.2 omega]'."""
    th, om = x[:, 0], x[:, 1]
    Mk, Mj = pendulum_jets(x)
    Mk[:, 0, 1], Mk[:, 1, 1] = 0.1 * np.sin(th), 1.0 + 0.2 * om
    Mj[:, 0, 2 + 1] = 0.1 * np.cos(th)          # d g_0 / d theta at column (1+0) C + 1
    Mj[:, 1, 4 + 1] = 0.2                       # d g_1 / d omega at column (1+1) C + 1
    return Mk, Mj


JETS = dict(b=pendulum_jets, c=xdependent_jets)


@pytest.mark.parametrize("tag", ["b", "c"])
@pytest.mark.parametrize("ci", range(4))
def test_helper_matches_reference_lqr_controller(tag, ci):
    numSteps, t, dt = G["configs"][ci]
    x = G["x"]
    Mk, Mj = JETS[tag](x)
    pre = "%s_c%d_" % (tag, ci)
    assert int(G[pre + "T"]) == max(int(numSteps) - int(t), 1)
    # the linearisations the reference handed to its solver, both passes
    g, Jf, Jg = lqr.unpack_jets(Mk, Mj, 2, 1)
    u, u0, status = lqr.lqr_nominal(Mk, Mj, x, G["x_goal"], G["Q"], G["R"], dt, int(numSteps), int(t))
    assert not status.any()
    own_rel(g * dt, G[pre + "B"], 1e-12, "B")
    own_rel(np.eye(2) + dt * Jf, G[pre + "A1"], 1e-12, "A, first pass")
    own_rel(np.eye(2) + dt * (Jf + Jg[:, 0] * u0[:, 0, None, None]), G[pre + "A2"], 1e-12, "A, second pass")
    if tag == "c":
        assert np.abs(G[pre + "A2"] - G[pre + "A1"]).max() > 1e-6          # the second linearisation is a different one
    own_rel(u, G[pre + "u"], 1e-12, "u")


def test_long_horizon_is_the_discrete_algebraic_riccati_solution():
    """dt = 0.05, T = 5000 on the pendulum linearised at the bottom: P and K have converged to the stabilising solution of
    P = Q + A'PA - A'PB (R + B'PB)^-1 B'PA.  1e-10: the recursion is contractive there (rounding does not accumulate) and
    scipy's Schur solver is itself good to a few 1e-12 on this 2 x 2 problem."""
    import scipy.linalg as scipy_linalg
    dt = 0.05
    Mk, Mj = pendulum_jets(np.array([[0.0, 0.0]]))
    g, Jf, _ = lqr.unpack_jets(Mk, Mj, 2, 1)
    A, B = np.eye(2) + dt * Jf[0], g[0] * dt
    Q, R = G["Q"], G["R"]
    P, o, K, k, ok = lqr.recursion(A, B, Q, R, -Q @ G["x_goal"], 5000)
    assert ok
    Pinf = scipy_linalg.solve_discrete_are(A, B, Q, R)
    Kinf = np.linalg.solve(R + B.T @ Pinf @ B, B.T @ Pinf @ A)
    own_rel(P, Pinf, 1e-10, "P")
    own_rel(K, Kinf, 1e-10, "K")


def test_singular_input_cost_is_reported():
    u, u0, status = lqr.lqr_nominal(np.zeros((1, 2, 2)), np.zeros((1, 2, 6)), np.ones((1, 2)), [0.0, 0.0], np.eye(2),
                                    np.zeros((1, 1)), 0.01, 5)
    assert status.tolist() == [1] and not u.any() and not u0.any()


# ---------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


def test_header_declares_and_library_exports_lqr_entry_points(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in declared and name in exported and name in lib.declared_symbols(), name


# Every call below passes Bt = 0: the argument checks run first, so a refused call returns BCBF_EINVAL, and a call that passes
# its checks returns at once without touching the device (the fake pointers are never dereferenced).
FAKE = ctypes.c_void_p(4096)


def _lqr_args(ct, **over):
    a = dict(Mk=FAKE, Mj=FAKE, x=FAKE, x_goal=(ct * 4)(), Q=(ct * 16)(), R=(ct * 9)(), dt=0.01, numSteps=10, t=0, t_dev=None,
             u=FAKE, u0=FAKE, status=FAKE, Bt=0, n=2, m=1, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    return list(a.values())


LQR_OK = [dict(), dict(u0=None), dict(n=4, m=3), dict(n=1, m=1), dict(t=25), dict(t=-1, t_dev=FAKE), dict(numSteps=1)]
LQR_BAD = [dict(n=0), dict(n=5), dict(m=0), dict(m=4), dict(Mk=None), dict(Mj=None), dict(x=None), dict(x_goal=None),
           dict(Q=None), dict(R=None), dict(u=None), dict(status=None), dict(dt=0.0), dict(dt=-0.01), dict(dt=float("nan")),
           dict(numSteps=0), dict(t=-1), dict(Bt=-1)]
# (a ctypes array prints with its address, which would give the case a different id in every process)
_ids = lambda d: ",".join("%s=%s" % (k, "ptr" if isinstance(v, ctypes.c_void_p) else "array" if isinstance(v, ctypes.Array) else v)  # noqa: E731
                          for k, v in d.items()) or "default"


@pytest.mark.parametrize("suf, ct", [("_f32", ctypes.c_float), ("_f64", ctypes.c_double)], ids=["f32", "f64"])
@pytest.mark.parametrize("ok", LQR_OK, ids=_ids)
def test_lqr_nominal_valid_arguments_pass_the_checks(lib, suf, ct, ok):
    assert getattr(lib.lib, "bcbf_lqr_nominal" + suf)(*_lqr_args(ct, **ok)) == 0


@pytest.mark.parametrize("suf, ct", [("_f32", ctypes.c_float), ("_f64", ctypes.c_double)], ids=["f32", "f64"])
@pytest.mark.parametrize("bad", LQR_BAD, ids=_ids)
def test_lqr_nominal_refuses_bad_arguments(lib, suf, ct, bad):
    assert getattr(lib.lib, "bcbf_lqr_nominal" + suf)(*_lqr_args(ct, **bad)) == -1


def _step_args(**over):
    a = dict(Lop=FAKE, Vw=FAKE, X=FAKE, UHB=FAKE, ell=FAKE, s2=FAKE, Bm=FAKE, M0=FAKE, A=FAKE, N=16, shared=0,
             kernel_kind=0, mean_model=1, mean_mass=1.0, mean_gravity=10.0, mean_length=1.0, theta_c=math.pi / 4,
             delta_c=math.pi / 8, kalpha=FAKE, x_goal=(ctypes.c_double * 2)(0.0, 0.0),
             Q_goal=(ctypes.c_double * 4)(1.0, 0.0, 0.0, 1.0), R=1.0, u_ref_in=None, safety_factor=math.sqrt(99.0),
             ctrl_reg=1.0, relax_weight=100.0, hessian_mode=0, max_iters=100, true_mass=1.0, true_gravity=10.0,
             true_length=1.0, dt=0.002)
    a.update((k, FAKE) for k in ("x", "Mk", "Bk", "G", "Mj", "h", "gh", "Hh", "u_ref", "terms2", "terms", "tstatus", "Gc", "hc",
                                 "cstatus", "P", "q", "y", "sstatus", "iters", "u", "status", "min_h", "fails"))
    a.update(prior=0, explore=None, eps=0.0, ctrl_range=None, obs_x=None, obs_uh=None, obs_y=None, obs_ld=1, z=None,
             xdot_s=None, cbc_s=None, relaxed=None, viol_relaxed=None, rho_tol=1e-6, nominal=1, numSteps=250, t=0, t_dev=None,
             lstatus=FAKE, Bt=0, n=2, m=1)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    return list(a.values()) + [None, None, None]


RANGE = (ctypes.c_double * 2)(-10.0, 10.0)
STEP_OK = [dict(), dict(nominal=0), dict(nominal=0, lstatus=None, numSteps=0, t=-1), dict(nominal=0, u_ref_in=FAKE),
           dict(z=FAKE), dict(t=-1, t_dev=FAKE), dict(explore=FAKE, eps=0.1, ctrl_range=RANGE), dict(t=400),
           dict(Lop=None, Vw=None, X=None, UHB=None, M0=None, N=0)]
STEP_BAD = [dict(nominal=2), dict(nominal=-1), dict(u_ref_in=FAKE), dict(lstatus=None), dict(numSteps=0), dict(t=-1),
            dict(n=3), dict(dt=0.0), dict(R=0.0), dict(x_goal=None), dict(eps=2.0), dict(explore=FAKE),
            dict(z=FAKE, rho_tol=-1.0), dict(z=FAKE, relaxed=FAKE)]


@pytest.mark.parametrize("ok", STEP_OK, ids=_ids)
def test_pendulum_nominal_step_valid_arguments_pass_the_checks(lib, ok):
    assert lib.lib.bcbf_pendulum_control_step_nominal_f64(*_step_args(**ok)) == 0


@pytest.mark.parametrize("bad", STEP_BAD, ids=_ids)
def test_pendulum_nominal_step_refuses_bad_arguments(lib, bad):
    assert lib.lib.bcbf_pendulum_control_step_nominal_f64(*_step_args(**bad)) == -1
