"""CPU side of the obstacle-field working set: the rule's unit cases on the yardstick (tests/_obstacle_field_reference.py), the
certificate on four seeded fields against the oracle's full program, the sampler, the host-side checks of the facade, and every
BCBF_EINVAL refusal of the three entries through ctypes (they return before any HIP call, so they run without a GPU)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _obstacle_field_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["bcbf_obstacle_field_%s_%s" % (e, s) for e in ("select", "audit", "commit") for s in ("f32", "f64")]
# the four fields of the issue: (discs, seed) of rollouts.random_obstacle_field, 40 steps each
FIELDS = [(16, 0), (64, 1), (32, 2), (48, 3)]
STEPS = 40
MAX_NOT_COMPARED, MAX_UNCERTIFIED = 0.15, 0.10


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops(lib):
    from bayesian_cbf_amd import ops
    assert (ops.FIELD_CERTIFIED, ops.FIELD_FULL, ops.FIELD_UNSOLVED, ops.FIELD_UNCERTIFIED) == \
        (R.CERTIFIED, R.FULL, R.UNSOLVED, R.UNCERTIFIED)
    assert ops.FIELD_TOLERANCES[__import__("torch").float64] == (R.TOL_F, R.TOL_A)
    return ops


# ---------------------------------------------------------------------------------------------- the rule
X = np.array([-1.0, -0.5, 0.3])
TW = (0.7, 0.3)


def test_select_duplicate_discs_tie_to_the_lower_index(ops):
    cen = np.array([[0.0, 0.0], [-0.2, -0.1], [0.0, 0.0], [-0.2, -0.1], [2.0, 2.0], [-0.2, -0.1]])
    rad = np.array([0.3, 0.2, 0.3, 0.2, 0.1, 0.2])
    _, h = R.rows(X, cen, rad, TW)
    assert h[1] == h[3] == h[5] and h[0] == h[2]                    # bit-equal: the tie rule is exact
    order = np.argsort(h, kind="stable")
    for S in (1, 2, 3):
        s = R.select(X, cen, rad, TW, S)
        assert s["idx"].tolist() == order[:S].tolist()
        assert s["min_h"] == h.min()
    assert R.select(X, cen, rad, TW, 3)["idx"].tolist() == [1, 3, 5] and R.select(X, cen, rad, TW, 3)["margin"] > 1e-3
    assert R.select(X, cen, rad, TW, 2)["margin"] == 0.0            # the third duplicate is as small: an undecided set


def test_select_nan_radius_is_lowest_and_min_h_is_minus_inf(ops):
    cen = np.array([[0.0, 0.0], [-0.2, -0.1], [1.0, 1.0], [0.5, 0.5]])
    rad = np.array([0.3, 0.2, np.nan, np.nan])
    s = R.select(X, cen, rad, TW, 3)
    assert s["idx"].tolist() == [2, 3, 1] and s["min_h"] == -np.inf
    assert R.select(X, cen[:2], rad[:2], TW, 2)["margin"] == np.inf  # Kf = S: nothing to decide


def _audit_case(m, idx, scale=None, cert=0, status=0, **kw):
    m = np.array(m, dtype=np.float64)
    return R.audit(cert, status, np.array(idx), R._lowest(m), np.ones_like(m) if scale is None else np.array(scale), **kw)


def test_audit_certifies_when_no_unselected_cone_is_violated(ops):
    a = _audit_case([-3e-10, 0.5, 2.0, -5e-8, 0.1], [0, 1, 2])
    assert a["cert"] == ops.FIELD_CERTIFIED and a["nviol"] == 0 and a["swapped"] == -1 and a["idx"].tolist() == [0, 1, 2]
    assert a["worst_idx"] == 3 and a["worst_margin"] == -5e-8       # inside tol_f: not a violator
    assert abs(a["decision"] - 5e-8) < 1e-12
    a = _audit_case([-3e-10, 0.5, 2.0, -5e-5, 0.1], [0, 1, 2], scale=[1, 1, 1, 1e3, 1])
    assert a["cert"] == ops.FIELD_CERTIFIED                         # the threshold scales with max(1, |E|, rho s)


def test_audit_evicts_the_slackest_slot_for_the_worst_violator(ops):
    a = _audit_case([-3e-10, 0.5, 2.0, -0.2, -0.7, -0.7, 0.3, np.nan], [0, 2, 1])
    assert a["cert"] == 0 and a["nviol"] == 4 and a["rounds_inc"] == 1
    assert a["swapped"] == 1 and a["violator"] == 7 and a["idx"].tolist() == [0, 7, 1]          # NaN counts as -inf
    a = _audit_case([-3e-10, 0.5, 2.0, -0.2, -0.7, -0.7, 0.3], [0, 2, 1])
    assert a["violator"] == 4 and a["decision"] == 0.0              # bit-equal violators: the lower index, an undecided choice
    a = _audit_case([2.0, 2.0, -1.0], [0, 1])
    assert a["swapped"] == 0 and a["idx"].tolist() == [2, 1]        # bit-equal slots: the lower slot


def test_audit_full_set_exit(ops):
    a = _audit_case([-3e-10, 5e-7, -2e-9, -0.2, 0.4], [0, 1, 2])
    assert a["cert"] == ops.FIELD_FULL and a["nviol"] == 1 and a["idx"].tolist() == [0, 1, 2] and a["rounds_inc"] == 0
    a = _audit_case([-3e-10, 5e-6, -2e-9, -0.2, 0.4], [0, 1, 2])
    assert a["cert"] == 0 and a["swapped"] == 1                     # 5e-6 > tol_a: that slot is slack


def test_audit_is_idempotent_on_a_decided_instance_and_flags_unsolved(ops):
    for cert in (ops.FIELD_CERTIFIED, ops.FIELD_FULL, ops.FIELD_UNSOLVED):
        a = _audit_case([0.1, 0.2, -5.0], [0, 1], cert=cert)
        assert a["cert"] == cert and a["idx"].tolist() == [0, 1] and a["rounds_inc"] == 0 and a["nviol"] is None
    a = _audit_case([0.1, 0.2, -5.0], [0, 1], status=2)
    assert a["cert"] == ops.FIELD_UNSOLVED and a["idx"].tolist() == [0, 1] and a["worst_idx"] == -1


def test_margin_is_the_cone_of_the_oracle(ops):
    """margin_k of the yardstick = c'u + d - rho |A u + b| of oracle.cbc's cone, on a learned-model-like (Mk, Bk, A)."""
    from oracle import cbc as ocbc, unicycle as ouni
    rng = np.random.RandomState(4)
    cen, rad = R.random_obstacle_field(12, seed=9)
    Mk = 0.1 * rng.randn(3, 3)
    Bq = rng.randn(3, 3)
    Bk, A = Bq @ Bq.T + 0.1 * np.eye(3), np.diag([0.01, 0.02, 0.03])
    u, rho = np.array([0.7, -0.4]), 2.3
    fhat, ghat = ouni.ackermann_f(X), ouni.ackermann_g(X, 1.0)
    m, E, rs, scale = R.margins(X, u, Mk, Bk, A, fhat, ghat, rho, cen, rad, TW, 5.0)
    for k in range(12):
        ob = ouni.ObstacleCBF(cen[k], rad[k], TW)
        Ac, b, c, d = ocbc.convert_cbc_terms_to_socp_terms(*ocbc.reldeg1_terms(Mk, Bk, A, ob.grad_cbf(X), 5.0 * ob.cbf(X), fhat, ghat), 0)
        want = c @ u + d - rho * np.linalg.norm(Ac @ u + b)
        assert abs(m[k] - want) <= 1e-12 * scale[k], (k, m[k], want)


# ---------------------------------------------------------------------------------------------- the certificate
def test_sampler_of_the_package_is_the_yardsticks(ops):
    from bayesian_cbf_amd.rollouts import random_obstacle_field
    for Kf, seed in FIELDS:
        f = random_obstacle_field(Kf, seed=seed)
        cen, rad = R.random_obstacle_field(Kf, seed=seed)
        assert np.array_equal(f["centers"].numpy(), cen) and np.array_equal(f["radii"].numpy(), rad)
        assert (np.linalg.norm(cen - R.START[:2], axis=1) >= rad + 0.5).all()
        assert (np.linalg.norm(cen - R.GOAL[:2], axis=1) >= rad + 0.4).all()
        assert (rad >= 0.1).all() and (rad <= 0.35).all() and cen.shape == (Kf, 2)


@pytest.mark.parametrize("Kf,seed", FIELDS)
def test_certified_steps_are_feasible_and_optimal_for_the_whole_field(ops, Kf, seed):
    from bayesian_cbf_amd.rollouts import random_obstacle_field
    f = random_obstacle_field(Kf, seed=seed)
    cen, rad = f["centers"].numpy(), f["radii"].numpy()
    steps, c = R.closed_loop(cen, rad, STEPS)
    from oracle import unicycle as ouni, cbc as ocbc
    certified = compared = 0
    worst_obj = worst_feas = 0.0
    for s in steps:
        fs = s["fs"]
        if fs["cert"] != ops.FIELD_CERTIFIED:
            assert fs["status_eff"] != 0
            continue
        certified += 1
        assert fs["status_eff"] == 0 and fs["rounds"] <= 2
        # every cone of the field, recomputed independently of the yardstick's vectorised rows: oracle.cbc's cone per disc
        x, u = s["x"], fs["y"][:2]
        fhat, ghat = ouni.ackermann_f(x), ouni.ackermann_g(x, c["L_mean"])
        for k in range(Kf):
            ob = ouni.ObstacleCBF(cen[k], rad[k], c["tw"])
            Ac, b, cc, d = ocbc.convert_cbc_terms_to_socp_terms(
                *ocbc.reldeg1_terms(np.zeros((3, 3)), np.eye(3), 0.01 * np.eye(3), ob.grad_cbf(x), c["gamma"] * ob.cbf(x), fhat, ghat), 0)
            E, rs = cc @ u + d, c["rho"] * np.linalg.norm(Ac @ u + b)
            assert E - rs >= -R.TOL_F * max(1.0, abs(E), rs), (k, E - rs)
            worst_feas = max(worst_feas, -(E - rs) / max(1.0, abs(E), rs))
        if s["full"]["status"] != "optimal":
            continue
        compared += 1
        yf = np.concatenate([s["full"]["u"], [s["full"]["relax"]]])
        fo, fw = R.objective(yf, c["w"]), R.objective(fs["y"], c["w"])
        worst_obj = max(worst_obj, abs(fo - fw) / max(1.0, abs(fo)))
        assert abs(fo - fw) <= R.EPS_G * max(1.0, abs(fo)), (fo, fw)
    print("Kf=%d seed=%d: certified %d / %d, compared %d, worst objective gap %.2e, worst infeasibility %.2e"
          % (Kf, seed, certified, STEPS, compared, worst_obj, worst_feas))
    assert STEPS - certified <= MAX_UNCERTIFIED * STEPS, certified
    assert certified - compared <= MAX_NOT_COMPARED * STEPS, (certified, compared)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcbf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bcbf_\w+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ENTRIES:
        assert name in declared and name in exported and name in lib.declared_symbols(), name
    assert re.search(r"#define BCBF_MAX_FIELD 256\b", header) and re.search(r"#define BCBF_FIELD_UNCERTIFIED 6\b", header)


def test_field_kernels_are_under_the_scratch_guard(lib):
    from bayesian_cbf_amd import build
    assert "obstacle_field.hip" in build.SOURCES
    guard = build.ZERO_SCRATCH_KERNELS["obstacle_field.hip"]
    assert len(guard) == 6 and all(k.startswith("obstacle_field_") for k in guard)
    assert "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["obstacle_field.hip"]
    assert not any(k.startswith("obstacle_field") for k in build.SCRATCH_ALLOWANCE)


FAKE = [ctypes.c_void_p(4096 * (k + 1)) for k in range(24)]
GOOD = dict(Bt=5, Kf=16, S=3, stride=0, gamma=5.0, tol_f=1e-7, tol_a=1e-6, dt=0.05, L_true=12.0, null=())
# pointers -- select: 0 x, 1 centers_f, 2 radii_f, 3 tw, 4 idx, 5 centers_sel, 6 radii_sel, 7 min_h, 8 cert, 9 rounds
#             audit:  0 x, 1 y, 2 status, 3 Mk, 4 Bk, 5 A, 6 fhat, 7 ghat, 8 rho, 9 centers_f, 10 radii_f, 11 tw, 12 idx,
#                     13 centers_sel, 14 radii_sel, 15 cert, 16 rounds, 17 worst_margin, 18 worst_idx, 19 nviol
#             commit: 0 x, 1 y, 2 status, 3 cert, 4 status_eff
NPTR = dict(select=10, audit=20, commit=5)


def _call(lib, entry, suf, a):
    p = [None if k in a["null"] else FAKE[k] for k in range(24)]
    fn = getattr(lib.lib, "bcbf_obstacle_field_%s_%s" % (entry, suf))
    if entry == "select":
        return fn(p[0], p[1], p[2], a["stride"], *p[3:10], a["Bt"], a["Kf"], a["S"], None)
    if entry == "audit":
        return fn(*p[0:11], a["stride"], p[11], a["gamma"], a["tol_f"], a["tol_a"], *p[12:20], a["Bt"], a["Kf"], a["S"], None)
    return fn(*p[0:5], a["dt"], a["L_true"], a["Bt"], None)


BAD_SHAPE = [(dict(Bt=0), "Bt <= 0"), (dict(Bt=-2), "Bt <= 0"), (dict(S=0), "S must be"), (dict(S=4), "S must be"),
             (dict(Kf=2), "Kf must be"), (dict(Kf=257), "Kf must be"), (dict(Kf=0, S=1), "Kf must be"),
             (dict(stride=2), "field_stride"), (dict(stride=-1), "field_stride")]
BAD_TOL = [(dict(tol_f=-1e-9), "tol_f"), (dict(tol_f=math.nan), "tol_f"), (dict(tol_f=math.inf), "tol_f"),
           (dict(tol_a=-1.0), "tol_a"), (dict(tol_a=math.nan), "tol_a"), (dict(tol_a=math.inf), "tol_a")]
BAD_COMMIT = [(dict(Bt=0), "Bt <= 0"), (dict(dt=-0.05), "dt"), (dict(dt=math.nan), "dt"), (dict(dt=math.inf), "dt"),
              (dict(L_true=0.0), "L_true"), (dict(L_true=math.nan), "L_true"), (dict(L_true=math.inf), "L_true")]
BAD = ([("select", c, w) for c, w in BAD_SHAPE] + [("select", dict(null=(k,)), "null") for k in range(NPTR["select"])]
       + [("audit", c, w) for c, w in BAD_SHAPE + BAD_TOL] + [("audit", dict(null=(k,)), "null") for k in range(NPTR["audit"])]
       + [("commit", c, w) for c, w in BAD_COMMIT] + [("commit", dict(null=(k,)), "null") for k in range(NPTR["commit"])])


@pytest.mark.parametrize("suf", ["f32", "f64"])
@pytest.mark.parametrize("entry,change,why", BAD, ids=["%s-%d" % (e, i) for i, (e, c, w) in enumerate(BAD)])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, entry, change, why):
    """Every case fails the host check, so the made-up pointers are never used and no GPU is touched."""
    rc = _call(lib, entry, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_obstacle_field_%s_%s" % (entry, suf)) and why in msg, msg


def test_facade_refuses_on_the_host(ops):
    import torch
    f64 = torch.float64
    x = torch.zeros(4, 3, dtype=f64)
    field = dict(centers=torch.zeros(8, 2, dtype=f64), radii=torch.ones(8, dtype=f64))
    task = dict(sign=torch.tensor([-1.0, 1.0, 1.0], dtype=f64), gammas=torch.tensor([5.0, 4.0], dtype=f64))
    with pytest.raises(ValueError, match="one gamma"):
        ops.unicycle_field_control_step_prepare(dict(A=None), task, field, {}, x)
    with pytest.raises(ValueError, match="1..3 obstacle slots"):
        ops.unicycle_field_control_step_prepare(dict(A=None), dict(task, sign=torch.ones(5, dtype=f64)), field, {}, x)
    with pytest.raises(ValueError, match="rounds"):
        ops.unicycle_field_control_step_prepare(dict(A=None), task, field, {}, x, rounds=0)
    task["gammas"] = torch.tensor([5.0, 5.0], dtype=f64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.unicycle_field_control_step_prepare(dict(A=None), task, field, {}, x)
    fws = ops.obstacle_field_workspace(4, 2, f64, "cpu")
    assert fws["idx"].shape == (4, 2) and fws["centers_sel"].shape == (4, 2, 2) and bool(torch.isinf(fws["min_h"]).all())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.obstacle_field_select(x, field, torch.tensor([0.7, 0.3], dtype=f64), fws)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.obstacle_field_commit(x, x, fws["cert"], fws)
