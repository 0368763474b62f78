"""CPU-side checks of the pendulum safety loop (bcbf_pendulum_control_step_f64, bcbf_pendulum_plant_step_*): the header
declares and the library exports the entry points, every bad argument is refused with BCBF_EINVAL before any HIP call,
and the oracle composition the GPU tests hold the device step to reproduces the reference's recorded controller rows."""
import ctypes
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

from _pendulum_oracle import barrier, oracle_state, oracle_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("bcbf_pendulum_control_step_f64", "bcbf_pendulum_plant_step_f32", "bcbf_pendulum_plant_step_f64")


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


def test_header_declares_and_library_exports_pendulum_entry_points(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in declared and name in exported and name in lib.declared_symbols(), name
    assert "#define BCBF_PENDULUM_BADHESSIAN 5" in open(os.path.join(ROOT, "include", "bcbf.h")).read()


# Every call below passes Bt = 0: the argument checks run first, so a refused call returns BCBF_EINVAL, and a call that
# passes its checks returns at once without touching the device (the fake pointers are never dereferenced).
FAKE = ctypes.c_void_p(4096)


def _args(**over):
    a = dict(Lop=FAKE, Vw=FAKE, X=FAKE, UHB=FAKE, ell=FAKE, s2=FAKE, Bm=FAKE, M0=FAKE, A=FAKE, N=16, shared=0,
             kernel_kind=0, mean_model=1, mean_mass=1.0, mean_gravity=10.0, mean_length=1.0, theta_c=math.pi / 4,
             delta_c=math.pi / 8, kalpha=FAKE, x_goal=(ctypes.c_double * 2)(0.0, 0.0),
             Q_goal=(ctypes.c_double * 4)(1.0, 0.0, 0.0, 1.0), R=1.0, u_ref_in=None, safety_factor=math.sqrt(99.0),
             ctrl_reg=1.0, relax_weight=100.0, hessian_mode=0, max_iters=100, true_mass=1.0, true_gravity=10.0,
             true_length=1.0, dt=0.002)
    ws = dict((k, FAKE) for k in ("x", "Mk", "Bk", "G", "Mj", "h", "gh", "Hh", "u_ref", "terms2", "terms", "tstatus",
                                  "Gc", "hc", "cstatus", "P", "q", "y", "sstatus", "iters", "u", "status", "min_h", "fails"))
    a.update(ws)
    a.update(dict(Bt=0, n=2, m=1))
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    return list(a.values()) + [None, None, None]


def test_pendulum_control_step_valid_arguments_pass_the_checks(lib):
    assert lib.lib.bcbf_pendulum_control_step_f64(*_args()) == 0
    assert lib.lib.bcbf_pendulum_control_step_f64(*_args(Lop=None, Vw=None, X=None, UHB=None, M0=None, N=0)) == 0
    assert lib.lib.bcbf_pendulum_control_step_f64(*_args(iters=None, min_h=None, fails=None, shared=1, kernel_kind=2)) == 0


BAD = [dict(n=3), dict(m=2), dict(x=None), dict(ell=None), dict(s2=None), dict(A=None), dict(kalpha=None),
       dict(x_goal=None), dict(Mk=None), dict(G=None), dict(terms=None), dict(y=None), dict(status=None), dict(u=None),
       dict(min_h=None), dict(fails=None), dict(Vw=None), dict(N=0), dict(shared=2), dict(kernel_kind=3),
       dict(kernel_kind=-1), dict(hessian_mode=2), dict(max_iters=0), dict(dt=0.0), dict(dt=float("nan")), dict(R=0.0),
       dict(mean_length=0.0), dict(true_mass=0.0), dict(ctrl_reg=0.0), dict(relax_weight=-1.0),
       dict(safety_factor=-1.0), dict(Bt=-1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_pendulum_control_step_refuses_bad_arguments(lib, bad):
    assert lib.lib.bcbf_pendulum_control_step_f64(*_args(**bad)) == -1


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_pendulum_plant_step_refuses_bad_arguments(lib, suf):
    fn = getattr(lib.lib, "bcbf_pendulum_plant_step" + suf)
    assert fn(FAKE, FAKE, 1.0, 10.0, 1.0, 0.002, 0, None) == 0
    assert fn(None, FAKE, 1.0, 10.0, 1.0, 0.002, 0, None) == -1
    assert fn(FAKE, None, 1.0, 10.0, 1.0, 0.002, 0, None) == -1
    assert fn(FAKE, FAKE, 0.0, 10.0, 1.0, 0.002, 0, None) == -1
    assert fn(FAKE, FAKE, 1.0, 10.0, 1.0, 0.002, -1, None) == -1


# ---------------------------------------------------------------- the yardstick itself against the reference
CONTROLLER_FILES = sorted(glob.glob(os.path.join(GOLDEN, "controllers_pendulum_*.npz")))


def golden_state(g):
    from oracle import gp_posterior as ogp
    UH = ogp.homogeneous_controls(g["U"])
    return oracle_state(g["X"], UH, g["Xdot"], g["B"], g["ell"], float(g["s2"]), g["M0"], 1e-5 * g["jitter_rand"][0],
                        g["A"])


def cone_close(got, ref, indefinite, rtol=1e-9, atol=1e-11):
    A, b, c, d = got
    rA, rb, rc, rd = ref
    if indefinite:         # eigen fallback: rows sqrt(lambda_a) v_a', defined up to the sign of each eigenvector
        Mg, Mr = np.column_stack([b, A[:, 2:]]), np.column_stack([rb, rA[:, 2:]])
        np.testing.assert_allclose(Mg.T @ Mg, Mr.T @ Mr, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(np.abs(Mg), np.abs(Mr), rtol=1e-7, atol=1e-9)
    else:
        np.testing.assert_allclose(A, rA, rtol=rtol, atol=atol)
        np.testing.assert_allclose(b, rb, rtol=rtol, atol=atol)
    np.testing.assert_allclose(c, rc, rtol=rtol, atol=atol)
    np.testing.assert_allclose(d, rd, rtol=rtol, atol=atol)


@pytest.mark.parametrize("path", CONTROLLER_FILES, ids=os.path.basename)
def test_oracle_composition_reproduces_reference_controller_rows(path):
    g = np.load(path)
    st = golden_state(g)
    from oracle import controllers as oc
    for i in range(len(g["xs"])):
        o = oracle_step(st, g["xs"][i], u_ref=g["urefs"][i], k_alpha=g["k_alpha"], safety_factor=float(g["safety_factor"]),
                        ctrl_reg=float(g["ctrl_reg"]), relax_weight=float(g["relax_weight"]))
        bfe, e, V, bfv, v = o["terms"]
        packed = np.concatenate([bfe, [e], V.ravel(), bfv, [v]])
        np.testing.assert_allclose(packed, g["t_safety_terms"][i], rtol=1e-9, atol=1e-11)
        indefinite = np.linalg.eigvalsh(oc._asq(V, bfv, v)).min() <= 0
        assert [c[0] for c in o["cons"]] == ["Objective", "Safety_0 gt 0"]
        for (name, cone), key in zip(o["cons"], ("obj", "safety")):
            cone_close(cone, tuple(g["t_%s_%s" % (key, k)][i] for k in "Abcd"), key == "safety" and indefinite)


def test_oracle_no_gp_terms_are_the_reference_closed_form():
    """No-GP mode (ControlCBFCLFGroundTruth): variance terms exactly 0, (bfe, e) = (-A(x), b(x)) of RadialCBFRelDegree2
    on the true pendulum (pendulum.py:713-746): -A = L_g L_f h = sin(theta - theta_c) / (m l),
    b = L_f^2 h + k_alpha . [h, L_f h]."""
    rng = np.random.default_rng(3)
    for _ in range(16):
        x = np.array([rng.uniform(-math.pi, math.pi), rng.uniform(-3, 3)])
        o = oracle_step(None, x, mean_model=(1.0, 10.0, 1.0))
        bfe, e, V, bfv, v = o["terms"]
        assert np.all(V == 0) and np.all(bfv == 0) and v == 0
        th, om = x
        d = th - math.pi / 4
        h, _, _ = barrier(x)
        np.testing.assert_allclose(bfe[0], math.sin(d), rtol=1e-13, atol=1e-15)
        b = om ** 2 * math.cos(d) - 10.0 * math.sin(d) * math.sin(th) + 1.0 * h + 3.0 * om * math.sin(d)
        np.testing.assert_allclose(e, b, rtol=1e-12, atol=1e-13)
