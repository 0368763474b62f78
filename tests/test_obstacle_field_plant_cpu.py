"""CPU side of the obstacle-field commit on a posterior-drawn plant (bcbf_obstacle_field_commit_sampled, csrc/field_plant.hip): the
ABI and every BCBF_EINVAL refusal through ctypes (they return before any HIP call), the yardstick
tests/_obstacle_field_plant_reference.py against the posterior-plant yardstick, the calibration of the tight cone's empirical risk
on the CPU oracle, and the borderline condition of the seeded inputs the GPU tests use."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _obstacle_field_plant_reference as R
import _obstacle_field_reference as OF
import _posterior_plant_reference as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["bcbf_obstacle_field_commit_sampled_f32", "bcbf_obstacle_field_commit_sampled_f64"]


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRIES:
        assert name in declared and name in exported and name in lib.declared_symbols(), name


def test_the_new_source_is_under_the_scratch_guard_with_no_allowance(lib):
    from bayesian_cbf_amd import build
    assert "field_plant.hip" in build.SOURCES
    assert build.ZERO_SCRATCH_KERNELS["field_plant.hip"] == ["field_plant_kernel<float>", "field_plant_kernel<double>"]
    assert "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["field_plant.hip"]
    assert not any("field_plant" in k for k in build.SCRATCH_ALLOWANCE)
    assert len(build.ZERO_SCRATCH_KERNELS["obstacle_field.hip"]) == 6          # no instantiation went into the existing file


NPTR = 28
FAKE = [ctypes.c_void_p(4096 * (k + 1)) for k in range(NPTR)]
GOOD = dict(Bt=5, Kf=16, S=3, stride=0, gamma=5.0, dt=0.05, null=())
# pointers: 0 x, 1 y, 2 status, 3 cert, 4 Mk, 5 Bk, 6 A, 7 fhat, 8 ghat, 9 rho, 10 centers_f, 11 radii_f, 12 tw, 13 idx, 14 z,
#           15 status_eff, 16 xdot_s, 17 cbc_min, 18 cbc_argmin, 19 tight_idx, 20 cbc_tight, 21 nneg, 22 solved, 23 viol_tight,
#           24 viol_any, 25 viol_unselected, 26 viol_discs, 27 min_cbc


def _call(lib, suf, a):
    p = [None if k in a["null"] else FAKE[k] for k in range(NPTR)]
    fn = getattr(lib.lib, "bcbf_obstacle_field_commit_sampled_" + suf)
    return fn(*p[0:12], a["stride"], p[12], a["gamma"], *p[13:28], a["dt"], a["Bt"], a["Kf"], a["S"], None)


BAD = ([(dict(Bt=0), "Bt <= 0"), (dict(Bt=-2), "Bt <= 0"), (dict(S=0), "S must be"), (dict(S=4), "S must be"),
        (dict(Kf=2), "Kf must be"), (dict(Kf=257), "Kf must be"), (dict(Kf=0, S=1), "Kf must be"),
        (dict(stride=2), "field_stride"), (dict(stride=-1), "field_stride"),
        (dict(gamma=math.nan), "gamma"), (dict(gamma=math.inf), "gamma"), (dict(gamma=-math.inf), "gamma"),
        (dict(dt=math.nan), "dt"), (dict(dt=math.inf), "dt"), (dict(dt=-0.05), "dt")]
       + [(dict(null=(k,)), "null") for k in range(NPTR)])


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("change,why", BAD, ids=["bad-%d" % i for i in range(len(BAD))])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, change, why):
    """Every case fails the host check, so the made-up pointers are never used and no GPU is touched."""
    rc = _call(lib, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_obstacle_field_commit_sampled_" + suf) and why in msg, msg


def test_facade_refuses_on_the_host(lib):
    import torch
    from bayesian_cbf_amd import ops
    f64 = torch.float64
    risk = ops.obstacle_field_risk_workspace(4, f64, "cpu")
    assert risk["z"].shape == (4, 3) and risk["xdot_s"].shape == (4, 3) and bool(torch.isinf(risk["min_cbc"]).all())
    for k in ("cbc_argmin", "tight_idx", "nneg", "solved", "viol_tight", "viol_any", "viol_unselected", "viol_discs"):
        assert risk[k].dtype == torch.int32 and risk[k].shape == (4,) and int(risk[k].abs().sum()) == 0
    x = torch.zeros(4, 3, dtype=f64)
    ws = ops.control_workspace(4, 2, f64, "cpu")
    fws = ops.obstacle_field_workspace(4, 2, f64, "cpu")
    field = dict(centers=torch.zeros(8, 2, dtype=f64), radii=torch.ones(8, dtype=f64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.obstacle_field_commit_sampled(x, ws, torch.zeros(4, 3, 3, dtype=f64), torch.ones(4, dtype=f64), field,
                                          torch.tensor([0.7, 0.3], dtype=f64), 5.0, fws, risk, 0.05)
    from bayesian_cbf_amd.rollouts import obstacle_field_rollouts
    with pytest.raises(ValueError, match="plant must be"):
        obstacle_field_rollouts(4, field, plant="drawn", device="cpu")


# ---------------------------------------------------------------------------------------------- the yardstick against itself
def test_reference_with_three_discs_is_the_posterior_plant_reference():
    """Kf = S = 3: cbc_k of the field yardstick = the obstacle rows of _posterior_plant_reference.step for the same inputs."""
    rng = np.random.RandomState(12)
    Bt = 9
    case = R.make_case(3, 3, True, 31, Bt=Bt)
    tw, gamma = (0.7, 0.3), 5.0
    y = rng.randn(Bt, 3)
    Mk = 0.1 * rng.randn(Bt, 3, 3)
    Bq = rng.randn(Bt, 3, 3)
    Bk = Bq @ Bq.transpose(0, 2, 1) + 0.1 * np.eye(3)
    A = np.tile(np.diag([0.01, 0.02, 0.0]), (Bt, 1, 1))                  # a zero pivot: the semidefinite rule
    fhat, ghat = 0.05 * rng.randn(Bt, 3), rng.randn(Bt, 3, 2)
    eff = np.zeros(Bt, np.int32)
    eff[4] = 6
    idx = np.tile(np.arange(3), (Bt, 1))
    out = R.step(case["x"], y, eff, Mk, Bk, A, fhat, ghat, np.full(Bt, 2.3), case["centers"], case["radii"], tw, gamma, idx,
                 case["z"], 0.05)
    grad, cst = np.zeros((Bt, 3, 3)), np.zeros((Bt, 3))
    for b in range(Bt):
        g, h = OF.rows(case["x"][b], case["centers"][b], case["radii"][b], tw)
        grad[b], cst[b] = g, gamma * h
    pp = PP.step(case["x"], y, eff, Mk, Bk, A, grad, cst, fhat, ghat, np.ones(3), case["z"], 0.05)
    np.testing.assert_allclose(out["cbc"], pp["cbc_s"], rtol=0, atol=1e-13 * out["scale_cbc"].max())
    np.testing.assert_array_equal(out["xdot_s"], pp["xdot_s"])
    np.testing.assert_array_equal(out["x_next"], pp["x_next"])
    assert out["solved"].tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1] and out["cbc_argmin"][4] == -1 and (out["xdot_s"][4] == 0).all()
    assert (out["scale_cbc"] >= np.abs(out["cbc"])).all() and (out["xdot_s"][:, 2] == pp["xdot_s"][:, 2]).all()
    for b in (0, 8):
        assert out["cbc_argmin"][b] == np.argmin(out["cbc"][b]) and out["nneg"][b] == (out["cbc"][b] < 0).sum()
        assert out["cbc_min"][b] == out["cbc"][b].min() and out["cbc_tight"][b] == out["cbc"][b, out["tight_idx"][b]]


# ---------------------------------------------------------------------------------------------- calibration on the CPU oracle
@pytest.mark.parametrize("max_risk", [0.2, 0.05])
def test_tight_cone_risk_is_calibrated_on_the_cpu_oracle(max_risk):
    Bt = 1500
    case = R.calibration_case(Bt)
    o = R.oracle_field_inputs(case, 1, max_risk=max_risk, rounds=1)
    c = o["consts"]
    out = R.step(case["x"], o["y"], o["status_eff"], o["Mk"], o["Bk"], o["A"], o["fhat"], o["ghat"], o["rho"], case["centers"],
                 case["radii"], c["tw"], c["gamma"], o["idx"], case["z"], 0.05)
    solved = out["solved"] == 1
    ti = np.where(solved, out["tight_idx"], 0)
    m, E = out["margin"][np.arange(Bt), ti], out["E"][np.arange(Bt), ti]
    active = solved & (m <= 1e-6 * (1 + np.abs(E)))
    n, v = int(active.sum()), int(out["viol_tight"][active].sum())
    print("max_risk %.2f: %d / %d solved, %d active, %d negative draws of the tight cone (rate %.4f)" % (max_risk, solved.sum(), Bt, n, v, v / max(n, 1)))
    assert solved.sum() >= 0.95 * Bt and n >= 0.9 * solved.sum()                  # conditions of the test, not measurements
    assert (out["tight_idx"][solved] == case["near"]).all()
    assert R.binomial_ok(v, n, max_risk), (v, n, max_risk)
    assert (out["viol_any"] >= out["viol_tight"]).all() and (out["viol_discs"] >= out["viol_any"]).all()
    assert out["viol_unselected"].sum() == 0                                      # the far discs never go negative


# ---------------------------------------------------------------------------------------------- the borderline condition
@pytest.mark.parametrize("Kf,S,per,seed", R.SHAPES, ids=["Kf%d-S%d-%s" % (k, s, "own" if p else "shared") for k, s, p, _ in R.SHAPES])
def test_seeded_inputs_of_the_gpu_tests_are_not_borderline(Kf, S, per, seed):
    """Every (shape, seed) of the GPU arithmetic test, with the working-set optimum of the CPU oracle in the place of the device's
    (they differ by the solvers' 1e-8), and at tol = 1e-9, a hundred times the band the GPU test uses: no instance is within tol of a
    sign change of a cbc_k or of a tie of the two smallest -- the 2 % cap of the GPU test hides nothing."""
    case = R.make_case(Kf, S, per, seed)
    o = R.oracle_field_inputs(case, S)
    c = o["consts"]
    out = R.step(case["x"], o["y"], o["status_eff"], o["Mk"], o["Bk"], o["A"], o["fhat"], o["ghat"], o["rho"], case["centers"],
                 case["radii"], c["tw"], c["gamma"], o["idx"], case["z"], 0.05, tol=1e-9)
    print("Kf=%d S=%d per=%s: %d / %d taken, %d borderline" % (Kf, S, per, out["solved"].sum(), R.BT, out["borderline"].sum()))
    assert out["solved"].sum() >= 0.25 * R.BT
    assert int(out["borderline"].sum()) == 0
