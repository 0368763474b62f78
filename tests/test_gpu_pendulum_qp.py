"""GPU tests of the pendulum CLF-CBF quadratic program on the known model (bcbf_pendulum_clf_cbf_control_*,
bcbf_pendulum_clf_cbf_rollout_*, ops.pendulum_clf_cbf_*, the PendulumCBFCLFDirect façade, rollouts.pendulum_clf_cbf_rollouts)
against the numpy yardstick tests/_pendulum_qp_reference.py: one-step parity on the states recorded from the reference's own
classes, the closed loop teacher-forced and free-running, composition of launches, the freeze of an infeasible instance,
strides and optional buffers, and the host façade.  Batch sizes 1, 63 and 130: one lane, a ragged wave, more than two waves.

The reference solves the program with cvxopt; parity with its iterates is not claimed -- the device is held to the unique
optimum of the strictly convex program, which the yardstick's generic enumerator is held to on the CPU
(tests/test_pendulum_qp_cpu.py)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _pendulum_qp_reference as R
from _tolreport import _record, rel_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "pendulum_clf_cbf_rows.npz"))
NP = {torch.float64: np.float64, torch.float32: np.float32}
RTOL = {torch.float64: 1e-8, torch.float32: 1e-3}          # the project's parity bounds, own-relative
CTRL = (1.0, 10.0, 1.0)
STEPS, DT = 300, 0.002
# Free-running drift of the device loop against the numpy loop over 300 steps, 130 starts, half of them on a mismatched
# plant: the worst |x_final - x_ref| / max |x_ref| and |min_h - min_h_ref| / max |min_h_ref| MEASURED on an MI355X
# (profiles/pendulum_clf_cbf.json, "free_running_drift").  The test asserts 100 times the measured worst, floor 1e-10.
FREE_RUN_MEASURED = 7.4e-16          # x_final 2.4e-16, min_h 7.4e-16
FREE_RUN_BOUND = max(100 * FREE_RUN_MEASURED, 1e-10)


def raw(t):
    return t.detach().cpu().numpy()


def bits(t):
    return raw(t.contiguous()).tobytes()


@pytest.fixture(scope="module")
def ops():
    from bayesian_cbf_amd import ops as _ops
    return _ops


def half_mismatched(Bt):
    """Every second instance runs on a plant (2, 10, 0.5) its controller, which believes (1, 10, 1), does not know."""
    true = np.tile(np.array(CTRL), (Bt, 1))
    true[1::2] = [2.0, 10.0, 0.5]
    return true


def dev_rollout(ops, x0, steps, dtype=torch.float64, ctrl=CTRL, true=None, record_every=0, t_offset=0, state=None, **task):
    """One launch from fresh statistics (or from `state`, the dict of an earlier call); everything comes back as tensors."""
    f = dict(dtype=dtype, device=DEV)
    Bt = len(x0)
    if state is None:
        state = dict(x=torch.tensor(np.asarray(x0), **f).contiguous(), min_h=torch.full((Bt,), float("inf"), **f),
                     damage=torch.zeros(Bt, dtype=torch.int32, device=DEV), status=torch.zeros(Bt, dtype=torch.int32, device=DEV))
    to_t = lambda m: m if m is None or isinstance(m, tuple) else torch.tensor(np.asarray(m), **f).contiguous()
    nrec = ops.pendulum_clf_cbf_records(t_offset, steps, record_every)
    traj = torch.full((nrec, Bt, 2), float("nan"), **f) if record_every > 0 else None
    us = torch.full((nrec, Bt), float("nan"), **f) if record_every > 0 else None
    ops.pendulum_clf_cbf_rollout(state["x"], state["min_h"], state["damage"], state["status"], steps, dt=DT, ctrl_model=to_t(ctrl),
                                 true_model=to_t(true), traj=traj, u_rec=us, record_every=record_every, t_offset=t_offset, **task)
    torch.cuda.synchronize()
    return dict(state, traj=traj, u=us)


# ------------------------------------------------------------------------------------------------ 1. one-step parity
def golden_oracle(dtype, kind, Bt):
    """The golden states (tiled to Bt) in the precision under test and the yardstick's answer ON THOSE inputs: in fp32 the
    states and the two angles of the barrier are the rounded ones the device receives, so theta = theta_c stays exact."""
    g = GOLDEN
    rnd = lambda v: np.asarray(v, dtype=NP[dtype]).astype(np.float64)
    x = rnd(g["x"][np.arange(Bt) % 64])
    t = R.task(clf_c=float(g["clf_c"]), k_alpha=tuple(g["k_alpha"]), theta_c=float(rnd(g["theta_c"])),
               delta_c=float(rnd(g["delta_c"])), cbf_gamma=float(g["cbf_gamma"]), cbf_kind=kind)
    return x, t, R.control(x, g["model"], t)


@pytest.mark.parametrize("Bt", [1, 63, 64, 130])
@pytest.mark.parametrize("kind", [0, 1], ids=["reldeg2", "radial"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_one_step_parity_on_the_golden_states(ops, dtype, kind, Bt):
    """A, b, values, u, rho against the yardstick to 1e-8 (fp64) / 1e-3 (fp32) of each output's own scale; status exact, the
    theta = theta_c states included (a1 == 0: infeasible where b1 < 0, the hard row vacuous where b1 > 0); u and rho are not
    written where status != 0 (the entry is called on buffers holding a sentinel)."""
    from bayesian_cbf_amd import _lib
    x, t, want = golden_oracle(dtype, kind, Bt)
    f = dict(dtype=dtype, device=DEV)
    xd = torch.tensor(x, **f).contiguous()
    model = torch.tensor(GOLDEN["model"], **f)
    out = dict(A=torch.empty(Bt, 2, **f), b=torch.empty(Bt, 2, **f), values=torch.empty(Bt, 2, **f),
               u=torch.full((Bt,), 777.0, **f), rho=torch.full((Bt,), 777.0, **f),
               status=torch.full((Bt,), -5, dtype=torch.int32, device=DEV))
    ct = ctypes.c_float if dtype == torch.float32 else ctypes.c_double
    fn = getattr(_lib.lib, "bcbf_pendulum_clf_cbf_control" + ("_f32" if dtype == torch.float32 else "_f64"))
    rc = fn(ops._p(xd), ops._p(model), 0, t["clf_c"], (ct * 2)(*t["k_alpha"]), t["theta_c"], t["delta_c"], t["cbf_gamma"], kind,
            t["slack_weight"], *(ops._p(out[k]) for k in ("A", "b", "values", "u", "rho", "status")), Bt, ops._stream(xd))
    assert rc == 0, _lib.lib.bcbf_last_error()
    torch.cuda.synchronize()
    got = {k: raw(v).astype(np.float64) if v.dtype != torch.int32 else raw(v) for k, v in out.items()}
    if kind == 1:
        # RadialCBF's two coefficients are both proportional to cos Delta_c - cos d, which at the three states ON the boundary
        # theta = 3 pi / 8 is a difference of equal numbers: its sign -- and with it which of a1 == 0, b1 < 0 holds -- is
        # below the rounding of either precision there.  Those states are compared for RadialCBFRelDegree2 only.
        gap = math.cos(t["delta_c"]) - np.cos(x[:, 0] - t["theta_c"])
        keep = np.abs(gap) > 16 * np.finfo(NP[dtype]).eps
        assert (~keep).sum() == 3 * (Bt // 64) + (Bt % 64 > 40) * 3
        got = {k: v[keep] for k, v in got.items()}
        want = {k: v[keep] for k, v in want.items()}
    assert np.array_equal(got["status"], want["status"])
    if Bt >= 64 and kind == 0:
        assert want["status"].sum() >= 1 and (want["status"] == 0).sum() >= 63
    for k in ("A", "b", "values"):
        for col in (0, 1):
            rel_close(got[k][:, col], want[k][:, col], RTOL[dtype], what="%s[:, %d]" % (k, col))
    ok = want["status"] == 0
    full_ok = torch.tensor(raw(out["status"]) == 0, device=DEV)
    if ok.any():
        rel_close(got["u"][ok], want["u"][ok], RTOL[dtype], what="u")
        rel_close(got["rho"][ok], want["rho"][ok], RTOL[dtype], what="rho")
    assert np.all(got["u"][~ok] == 777.0) and np.all(got["rho"][~ok] == 777.0)
    # the wrapper: the same numbers, NaN where nothing was written, and every output optional at the ABI
    o = ops.pendulum_clf_cbf_control(xd, ctrl_model=tuple(GOLDEN["model"]), clf_c=t["clf_c"], k_alpha=t["k_alpha"],
                                     theta_c=t["theta_c"], delta_c=t["delta_c"], cbf_gamma=t["cbf_gamma"],
                                     cbf_kind=("reldeg2", "radial")[kind])
    assert bits(o["A"]) == bits(out["A"]) and bits(o["status"]) == bits(out["status"]) and bits(o["u"][full_ok]) == bits(out["u"][full_ok])
    assert bool(torch.isnan(o["u"][~full_ok]).all()) and bool(torch.isnan(o["rho"][~full_ok]).all())
    only_u = torch.full((Bt,), 777.0, **f)
    rc = fn(ops._p(xd), ops._p(model), 0, t["clf_c"], (ct * 2)(*t["k_alpha"]), t["theta_c"], t["delta_c"], t["cbf_gamma"], kind,
            t["slack_weight"], None, None, None, ops._p(only_u), None, None, Bt, ops._stream(xd))
    assert rc == 0
    torch.cuda.synchronize()
    assert bits(only_u) == bits(out["u"])


# ------------------------------------------------------------------------------------------------ 2./3. the closed loop
_LOOP = {}


def loop_case(ops):
    """130 starts (ten of them inside the band the damage counter sees), 300 steps, every step recorded, fp64, every second plant mismatched (per-instance rows): the device run and
    the free-running numpy loop, each computed once."""
    if not _LOOP:
        x0, true = R.loop_starts(130), half_mismatched(130)
        _LOOP.update(x0=x0, true=true, dev=dev_rollout(ops, x0, STEPS, true=true, record_every=1),
                     ref=R.rollout(x0, CTRL, true, STEPS, dt=DT))
    return _LOOP


def test_teacher_forced_trajectory(ops):
    """From every device-recorded x_t the yardstick recomputes u_t and x_{t+1}: both to 1e-8 of their own scale; min_h and
    damage recomputed from the recorded states equal the outputs (damage exactly).  No instance is left out: none meets
    an infeasible step (held on the CPU for these starts)."""
    c = loop_case(ops)
    d = c["dev"]
    assert raw(d["status"]).max() == 0
    traj, us = raw(d["traj"]), raw(d["u"])
    assert traj.shape == (STEPS, 130, 2) and us.shape == (STEPS, 130) and np.isfinite(traj).all() and np.isfinite(us).all()
    assert np.array_equal(traj[0], c["x0"])
    flat = traj.reshape(-1, 2)
    ctrl = np.tile(np.array(CTRL), (len(flat), 1))
    want = R.control(flat, ctrl)
    assert want["status"].max() == 0
    rel_close(us.reshape(-1), want["u"], 1e-8, what="u_t from the recorded x_t")
    nxt = R.plant_step(flat, want["u"], np.tile(c["true"], (STEPS, 1)), DT).reshape(STEPS, 130, 2)
    got_next = np.concatenate([traj[1:], raw(d["x"])[None]])
    for col, name in ((0, "theta"), (1, "omega")):
        rel_close(got_next[:, :, col], nxt[:, :, col], 1e-8, what="x_{t+1} from the recorded x_t: " + name)
    h = want["values"][:, 1].reshape(STEPS, 130)
    rel_close(raw(d["min_h"]), h.min(0), 1e-8, what="min_h over the recorded states")
    assert np.array_equal(raw(d["damage"]), ((0 < traj[:, :, 0]) & (traj[:, :, 0] < math.pi / 4)).sum(0))
    assert (raw(d["min_h"]) < 0).any() and (raw(d["min_h"]) > 0).any() and raw(d["damage"]).max() > 0    # every outcome is in the comparison


def test_free_running_fp64_against_the_numpy_loop(ops):
    """The same 300 steps without teacher forcing: final state and min_h of the device loop against the numpy loop.  The loop
    contracts towards the boundary of the safe set, so rounding differences (libm against the device's sin / cos, fused
    multiply-adds) do not grow.  MEASURED on an MI355X: worst relative deviation 2.4e-16 (x_final), 7.4e-16 (min_h), a few
    ulp; asserted at 100 times the measured worst with a floor of 1e-10, so the floor is the bound in force."""
    c = loop_case(ops)
    d, r = c["dev"], c["ref"]
    assert raw(d["status"]).max() == 0 and r["status"].max() == 0
    ex = np.abs(raw(d["x"]) - r["x"]).max() / np.abs(r["x"]).max()
    eh = np.abs(raw(d["min_h"]) - r["min_h"]).max() / np.abs(r["min_h"]).max()
    print("free-running drift over %d steps: x_final %.3e, min_h %.3e (bound %.1e)" % (STEPS, ex, eh, FREE_RUN_BOUND))
    _record("free-running x_final", ex, FREE_RUN_BOUND)
    _record("free-running min_h", eh, FREE_RUN_BOUND)
    assert np.array_equal(raw(d["damage"]), r["damage"])
    assert ex <= FREE_RUN_BOUND and eh <= FREE_RUN_BOUND, (ex, eh)


# ------------------------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("split,every", [((150, 150), 1), ((149, 151), 7)], ids=["150+150", "149+151-every7"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_two_launches_equal_one_bit_for_bit(ops, dtype, split, every):
    """k + (300 - k) steps, the second call with t_offset = k and the record pointers moved on, equal one 300-step call in
    x, min_h, damage, status, traj and u -- bit for bit.  One instance starts on the infeasible state (status 1 in both)."""
    x0, true = R.starts(130).astype(NP[dtype]), half_mismatched(130)
    x0[77] = [NP[dtype](math.pi / 4), 0.0]
    one = dev_rollout(ops, x0, STEPS, dtype=dtype, true=true, record_every=every)
    a = dev_rollout(ops, x0, split[0], dtype=dtype, true=true, record_every=every)
    b = dev_rollout(ops, x0, split[1], dtype=dtype, true=true, record_every=every, t_offset=split[0],
                    state={k: a[k] for k in ("x", "min_h", "damage", "status")})
    assert a["traj"].shape[0] + b["traj"].shape[0] == one["traj"].shape[0] == ops.pendulum_clf_cbf_records(0, STEPS, every)
    for k in ("x", "min_h", "damage", "status"):
        assert bits(b[k]) == bits(one[k]), k
    assert bits(torch.cat([a["traj"], b["traj"]])) == bits(one["traj"])
    assert bits(torch.cat([a["u"], b["u"]])) == bits(one["u"])
    st = raw(one["status"])
    assert st[77] == 1 and np.count_nonzero(st) == 1 and not bool(torch.isnan(one["traj"]).any())


# ------------------------------------------------------------------------------------------------ 5. freeze
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_an_infeasible_instance_freezes_and_leaves_its_wave_alone(ops, dtype):
    """theta = theta_c, omega = 0 (a1 == 0, b1 = cos Delta_c - 1 < 0) among healthy starts in one wave: status 1, state and
    statistics exactly as they came in after 50 steps, u recorded as 0; the other lanes equal a run without it."""
    x0 = R.starts(63).astype(NP[dtype])
    bad = x0.copy()
    bad[5] = [NP[dtype](math.pi / 4), 0.0]
    a = dev_rollout(ops, bad, 50, dtype=dtype, record_every=1)
    b = dev_rollout(ops, x0, 50, dtype=dtype, record_every=1)
    assert raw(a["status"])[5] == 1 and np.count_nonzero(raw(a["status"])) == 1 and raw(b["status"]).max() == 0
    assert np.array_equal(raw(a["x"])[5], bad[5]) and raw(a["min_h"])[5] == np.inf and raw(a["damage"])[5] == 0
    assert np.all(raw(a["traj"])[:, 5] == bad[5]) and np.all(raw(a["u"])[:, 5] == 0)
    keep = torch.tensor([i for i in range(63) if i != 5], device=DEV)
    for k in ("x", "min_h", "damage", "status"):
        assert bits(a[k][keep]) == bits(b[k][keep]), k
    assert bits(a["traj"][:, keep]) == bits(b["traj"][:, keep]) and bits(a["u"][:, keep]) == bits(b["u"][:, keep])
    # the step index in status is global: the same instance in a call that continues a run at step 150
    c = dev_rollout(ops, bad, 20, dtype=dtype, t_offset=150)
    assert raw(c["status"])[5] == 151
    # and an instance that arrives frozen stays as it is
    d = dev_rollout(ops, x0, 20, dtype=dtype, state=dict(
        x=torch.tensor(x0, dtype=dtype, device=DEV), min_h=torch.full((63,), 0.25, dtype=dtype, device=DEV),
        damage=torch.full((63,), 3, dtype=torch.int32, device=DEV), status=torch.full((63,), 9, dtype=torch.int32, device=DEV)))
    assert np.array_equal(raw(d["x"]), x0) and np.all(raw(d["min_h"]) == 0.25) and np.all(raw(d["damage"]) == 3) and np.all(raw(d["status"]) == 9)


# ------------------------------------------------------------------------------------------------ 6. strides and NULLs
@pytest.mark.parametrize("Bt", [1, 63, 130])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_shared_row_equals_replicated_rows_and_recording_is_optional(ops, dtype, Bt):
    x0 = R.starts(Bt).astype(NP[dtype])
    plant = (2.0, 10.0, 0.5)
    shared = dev_rollout(ops, x0, 100, dtype=dtype, ctrl=CTRL, true=plant, record_every=1)
    rows = dev_rollout(ops, x0, 100, dtype=dtype, ctrl=np.tile(np.array(CTRL), (Bt, 1)), true=np.tile(np.array(plant), (Bt, 1)),
                       record_every=1)
    quiet = dev_rollout(ops, x0, 100, dtype=dtype, ctrl=CTRL, true=plant, record_every=0)
    assert quiet["traj"] is None and quiet["u"] is None
    for k in ("x", "min_h", "damage", "status"):
        assert bits(shared[k]) == bits(rows[k]) == bits(quiet[k]), k
    assert bits(shared["traj"]) == bits(rows["traj"]) and bits(shared["u"]) == bits(rows["u"])
    only_u = dev_rollout(ops, x0, 100, dtype=dtype, ctrl=CTRL, true=plant, record_every=0)       # one recording buffer alone
    us = torch.full((100, Bt), float("nan"), dtype=dtype, device=DEV)
    ops.pendulum_clf_cbf_rollout(*(torch.tensor(x0, dtype=dtype, device=DEV), torch.full((Bt,), float("inf"), dtype=dtype, device=DEV),
                                   torch.zeros(Bt, dtype=torch.int32, device=DEV), torch.zeros(Bt, dtype=torch.int32, device=DEV)),
                                 100, dt=DT, ctrl_model=CTRL, true_model=plant, u_rec=us, record_every=1)
    torch.cuda.synchronize()
    assert bits(us) == bits(shared["u"]) and bits(only_u["x"]) == bits(shared["x"])
    # zero steps: nothing moves
    z = dev_rollout(ops, x0, 0, dtype=dtype)
    assert np.array_equal(raw(z["x"]), x0) and np.all(raw(z["min_h"]) == np.inf)


# ------------------------------------------------------------------------------------------------ 7. the façade
def test_facade_controller_equals_the_batched_entry(ops):
    from bayesian_cbf_amd import pendulum as P
    ctrl = P.PendulumCBFCLFDirect(mass=1.0, gravity=10.0, length=1.0, dt=DT, dtype=torch.float64)
    g = GOLDEN
    batch = ops.pendulum_clf_cbf_control(torch.tensor(g["x"], dtype=torch.float64, device=DEV))
    clf, cbf1 = P.EnergyCLF(ctrl.model), P.RadialCBF(ctrl.model)
    for i in (0, 7, 38, 40, 50, 63):
        x = torch.tensor(g["x"][i], dtype=torch.float64)
        u = ctrl.control(x)
        assert u.shape == (1,) and u.dtype == torch.float64 and float(u[0]) == float(batch["u"][i])
        rel_close([float(clf.A(x)[0]), float(clf.b(x)), float(clf.value(x))], [g["clf_A"][i], g["clf_b"][i], g["clf_value"][i]], 1e-8,
                  what="EnergyCLF")
        rel_close([float(cbf1.A(x)[0]), float(cbf1.b(x)), float(cbf1.value(x))], [g["cbf1_A"][i], g["cbf1_b"][i], g["cbf1_value"][i]],
                  1e-8, what="RadialCBF")
        assert abs(float(clf(x, u)) - (g["clf_A"][i] * float(u[0]) - g["clf_b"][i])) <= 1e-8 * max(1.0, abs(g["clf_b"][i]))
    x32 = torch.tensor(g["x"][7], dtype=torch.float32)
    assert ctrl.control(x32).dtype == torch.float32
    with pytest.raises(RuntimeError, match="QP is infeasible"):
        P.control_QP_cbf_clf(torch.tensor([math.pi / 4, 0.0], dtype=torch.float64), ctrl.aff_constraints, [100])
    with pytest.raises(NotImplementedError):
        P.control_QP_cbf_clf(torch.tensor([1.0, 0.0], dtype=torch.float64), ctrl.aff_constraints, [100, 100])
    with pytest.raises(NotImplementedError):
        P.control_QP_cbf_clf(torch.tensor([1.0, 0.0], dtype=torch.float64), ctrl.aff_constraints[:1], [100])
    ctrl.set_model_params(mass=2.0, gravity=10.0, length=0.5)
    want = R.control(g["x"][7:8], (2.0, 10.0, 0.5))
    rel_close(raw(ctrl.control(torch.tensor(g["x"][7], dtype=torch.float64))), want["u"], 1e-8, what="set_model_params")


def test_run_pendulum_control_cbf_clf_returns_upstreams_five_vectors():
    from bayesian_cbf_amd import pendulum as P
    damage, time_vec, theta, omega, u = P.run_pendulum_control_cbf_clf(numSteps=200)
    assert all(v.shape == (200,) for v in (time_vec, theta, omega, u)) and damage.ndim == 0
    assert bool(((theta >= -math.pi) & (theta <= math.pi)).all()) and bool(torch.isfinite(u).all())
    assert float(theta[0]) == 5 * math.pi / 12 and float(omega[0]) == -0.01 and abs(float(time_vec[-1]) - 199 * 0.002) < 1e-12
    ref = R.rollout([[5 * math.pi / 12, -0.01]], CTRL, CTRL, 200, dt=0.002, record_every=1)
    rel_close(raw(theta), ref["traj"][:, 0, 0], 1e-8, what="theta_vec")
    rel_close(raw(u), ref["u"][:, 0], 1e-8, what="u_vec")
    assert float(damage) == 100.0 * ref["damage"][0] / 200
    d32 = P.run_pendulum_control_cbf_clf(numSteps=50, dtype=torch.float32)
    assert d32[2].dtype == torch.float32 and d32[2].shape == (50,)


def test_rollouts_driver_keys_and_launch_splitting():
    from bayesian_cbf_amd.rollouts import pendulum_clf_cbf_rollouts
    r = pendulum_clf_cbf_rollouts(Bt=130, numSteps=300)
    assert {"stats", "x_final", "min_h", "fails", "traj", "u", "loop_seconds", "damage", "status"} <= set(r)
    assert set(r["stats"]) == {"collisions", "mean_cost", "solver_failures", "count", "min_h"} and r["stats"]["count"] == 130
    assert r["x_final"].shape == (130, 2) and r["min_h"].shape == (130,) and r["fails"].dtype == torch.bool
    assert r["traj"] is None and r["u"] is None and r["damage"].dtype == torch.int32 and r["status"].dtype == torch.int32
    assert r["stats"]["collisions"] == int((~(r["min_h"] >= 0)).sum()) and r["stats"]["solver_failures"] == int(r["fails"].sum())
    one = pendulum_clf_cbf_rollouts(Bt=130, numSteps=300, record_every=5, true_model=(2.0, 10.0, 0.5))
    cut = pendulum_clf_cbf_rollouts(Bt=130, numSteps=300, record_every=5, true_model=(2.0, 10.0, 0.5), steps_per_launch=77)
    assert one["traj"].shape == (60, 130, 2) and one["u"].shape == (60, 130)
    for k in ("x_final", "min_h", "damage", "status", "traj", "u"):
        assert bits(one[k]) == bits(cut[k]), k
    per = pendulum_clf_cbf_rollouts(Bt=130, numSteps=300, record_every=5,
                                    true_model=torch.tensor([2.0, 10.0, 0.5], dtype=torch.float64, device=DEV).expand(130, 3).contiguous())
    assert bits(per["x_final"]) == bits(one["x_final"])
    r32 = pendulum_clf_cbf_rollouts(Bt=63, numSteps=100, dtype=torch.float32)
    assert r32["x_final"].dtype == torch.float32 and bool(torch.isfinite(r32["x_final"]).all())


def test_a_wrong_model_collides_more_often_than_the_right_one():
    """The question the controller exists for: (1, 10, 1) believed on a plant (2, 10, 0.5), 64 starts, 3000 steps, fp64."""
    from bayesian_cbf_amd.rollouts import pendulum_clf_cbf_rollouts
    matched = pendulum_clf_cbf_rollouts(Bt=64, numSteps=3000)
    wrong = pendulum_clf_cbf_rollouts(Bt=64, numSteps=3000, true_model=(2.0, 10.0, 0.5))
    print("collisions of 64: matched %d, mismatched %d" % (matched["stats"]["collisions"], wrong["stats"]["collisions"]))
    assert wrong["stats"]["collisions"] > matched["stats"]["collisions"]
    assert matched["stats"]["solver_failures"] == 0
