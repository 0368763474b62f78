"""CPU-side checks of the self-triggered event with the posterior-drawn plant and the held-control audit
(bcbf_unicycle_trigger_step_audit): the numpy yardstick tests/_trigger_audit_reference.py against the two yardsticks it is built on,
its NaN / first-event / after-unsolved rules, the entry's argument checks (refused before any HIP call) and the ValueErrors of the
`ops` binding."""
import ctypes
import math
import os

import numpy as np
import pytest

import _posterior_plant_reference as P
import _trigger_audit_reference as TA
import _trigger_reference as R
import _trigger_step_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


KOB, PROWS = 2, 7


def random_instance(seed):
    """One instance with every input of the event random: (base arguments of S.event, the rows of the solve)."""
    rng = np.random.default_rng(seed)
    off = rng.normal(size=(6, 3)) * 0.05
    th = rng.uniform(-1, 1)
    Bm, Am = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
    base = dict(x=np.array([-2.9, -0.8, th]) + 0.1 * rng.normal(size=3), u=rng.normal(size=2), fhat=0.05 * rng.normal(size=3),
                ghat=np.array([[math.cos(th), 0], [math.sin(th), 0], [0, 0.25]]), Mk=0.05 * rng.normal(size=(3, 3)),
                centers=[np.array([-4.0, -2.0]), np.array([-1.0, 0.5])], tw=(0.7, 0.3), off=off, r=R.whole_norm(off),
                ls=rng.uniform(0.3, 0.6, size=3), sf=0.9, Adiag=rng.uniform(0.01, 0.03, size=3), Bhyp=np.eye(3) + 0.1,
                plan_all=np.arange(3.0 * PROWS).reshape(PROWS, 3), dplan_all=-np.arange(3.0 * PROWS).reshape(PROWS, 3), dt_plan=0.05,
                L_true=12.0, t=0.12, events=3, t_end=1.0, tau_min=1e-6, tau_max=10.0)
    rows = dict(Bk=Bm @ Bm.T + 0.1 * np.eye(3), A=1e-2 * (Am @ Am.T + 0.1 * np.eye(3)), grad=rng.normal(size=(1 + KOB, 3)),
                cst=rng.normal(size=1 + KOB), sign=np.array([-1.0, 1.0, 1.0]), rho=1.7)
    return base, rows


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("status", [0, 2])
def test_without_draws_the_reference_is_the_trigger_step_yardstick_exactly(seed, status):
    base, rows = random_instance(seed)
    want = S.event(status=status, **base)
    got = TA.event(status=status, **base, **rows)
    assert set(got) == set(want)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    # ... and with the audit alone the event itself is still that one
    held = TA.event(status=status, u_held=np.array([0.3, -0.2]), held=1, **base, **rows)
    for k, v in want.items():
        assert np.array_equal(np.asarray(held[k]), np.asarray(v)), k
    assert TA.event(status=status, **dict(base, t=1.0), **rows, z=np.ones(3), u_held=np.zeros(2), held=1) is None      # finished


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_with_draws_the_plant_is_the_posterior_plant_yardstick_over_the_hold(seed, dtype):
    base, rows = random_instance(seed)
    z = np.random.default_rng(100 + seed).normal(size=3)
    plain = S.event(status=0, **base)
    c = TA.new_counters(KOB, dtype)
    ev = TA.event(status=0, z=z, counters=c, dtype=dtype, **base, **rows)
    one = lambda a: np.asarray(a, dtype=np.float64)[None]
    st = P.step(one(base["x"]), one(np.r_[base["u"], 0.0]), np.array([0]), one(base["Mk"]), one(rows["Bk"]), one(rows["A"]),
                one(rows["grad"]), one(rows["cst"]), one(base["fhat"]), one(base["ghat"]), rows["sign"], one(z), plain["dt_used"], dtype=dtype)
    for k, r in (("x", "x_next"), ("xdot_s", "xdot_s"), ("cbc_s", "cbc_s")):
        assert ev[k].dtype == dtype and np.array_equal(ev[k], st[r][0]), k
    for k in ("tau", "dt_used", "t", "events", "row", "uBu", "xvel", "Lh", "Lfh"):          # none of them depends on the plant
        assert np.array_equal(ev[k], plain[k]), k
    assert not np.array_equal(ev["x"], plain["x"].astype(dtype))
    # the hold as the device's working type holds it overrides the yardstick's own
    half = TA.event(status=0, z=z, dtype=dtype, dt_used=plain["dt_used"] / 2, **base, **rows)
    # (each state is rounded to `dtype` once, half an ulp of |x| each: one ulp bounds the difference of the two displacements)
    np.testing.assert_allclose(half["x"] - base["x"], (ev["x"] - base["x"]) / 2, rtol=0, atol=float(np.spacing(dtype(np.abs(ev["x"]).max()))))
    # the counters: one solved event, the obstacle rows only
    cb = ev["cbc_s"][1:]
    assert c["solved"] == 1 and np.array_equal(c["viol"], (cb < 0).astype(int)) and np.array_equal(c["min_cbc"], cb)
    # unsolved: the state is kept, zero draw, zero conditions, no counter moves
    un = TA.event(status=2, z=z, counters=c, dtype=dtype, **base, **rows)
    assert np.array_equal(un["x"], base["x"].astype(dtype)) and not un["xdot_s"].any() and not un["cbc_s"].any()
    assert c["solved"] == 1 and un["dt_used"] == min(base["tau_max"], base["t_end"] - base["t"]) and un["last"]


@pytest.mark.parametrize("seed", range(6))
def test_audit_is_the_cone_of_the_held_control(seed):
    base, rows = random_instance(seed)
    u_held = np.random.default_rng(200 + seed).normal(size=2)
    c = TA.new_counters(KOB)
    ev = TA.event(status=0, u_held=u_held, held=1, counters=c, **base, **rows)
    assert ev["audited"] and c["audit_n"] == 1
    one = lambda a: np.asarray(a, dtype=np.float64)[None]
    for k in (1, 2):
        mean, std = P.row_mean_std(one(np.r_[u_held, 0.0]), one(base["Mk"]), one(rows["Bk"]), one(rows["A"]), one(rows["grad"]),
                                   one(rows["cst"]), one(base["fhat"]), one(base["ghat"]), rows["sign"], k)
        assert ev["held_mean"][k - 1] == mean[0] and ev["held_margin"][k - 1] == mean[0] - rows["rho"] * std[0]
        assert ev["scale_mean"][k - 1] >= abs(mean[0]) and ev["scale_margin"][k - 1] >= abs(ev["held_margin"][k - 1])
    assert np.array_equal(c["audit_neg"], np.stack([~(ev["held_mean"] >= 0), ~(ev["held_margin"] >= 0)], 1).astype(int))
    assert np.array_equal(c["audit_min"], np.stack([ev["held_mean"], ev["held_margin"]], 1))
    assert np.array_equal(ev["u_held_next"], base["u"]) and ev["held_next"] == 1
    # it is the HELD control that is audited, not this event's, and the status of this event does not matter
    other = TA.event(status=2, u_held=u_held, held=1, **base, **rows)
    assert np.array_equal(other["held_mean"], ev["held_mean"]) and other["held_next"] == 0
    assert not np.array_equal(TA.event(status=0, u_held=base["u"], held=1, **base, **rows)["held_mean"], ev["held_mean"])


def test_first_event_after_unsolved_and_nan_rules():
    base, rows = random_instance(3)
    c = TA.new_counters(KOB)
    # an instance's first event (held = 0): nothing is audited, no output rows, the flag is set for the next one
    e1 = TA.event(status=0, u_held=np.zeros(2), held=0, counters=c, **base, **rows)
    assert not e1["audited"] and "held_mean" not in e1 and c["audit_n"] == 0 and e1["held_next"] == 1
    # the chain: solved -> audited; unsolved -> the NEXT event is not audited
    e2 = TA.event(status=2, u_held=e1["u_held_next"], held=e1["held_next"], counters=c, **base, **rows)
    assert e2["audited"] and c["audit_n"] == 1 and e2["held_next"] == 0
    e3 = TA.event(status=0, u_held=e2["u_held_next"], held=e2["held_next"], counters=c, **base, **rows)
    assert not e3["audited"] and c["audit_n"] == 1 and e3["held_next"] == 1
    # NaN counts as negative and takes the minimum; +inf does neither
    c = TA.new_counters(KOB)
    TA.count_audit(c, np.array([np.nan, 1.0]), np.array([np.inf, -2.0]))
    assert c["audit_neg"].tolist() == [[1, 0], [0, 1]] and c["audit_min"].tolist() == [[-np.inf, np.inf], [1.0, -2.0]]
    TA.count_audit(c, np.array([3.0, 0.5]), np.array([4.0, -0.0]))
    assert c["audit_n"] == 2 and c["audit_neg"].tolist() == [[1, 0], [0, 1]] and c["audit_min"].tolist() == [[-np.inf, 4.0], [0.5, -2.0]]
    # the drawn conditions: any non-finite value is a violation (rollout_risk's rule); the CLC row is not counted
    c = TA.new_counters(KOB)
    TA.count_risk(c, np.array([-5.0, np.inf, 0.25]))
    TA.count_risk(c, np.array([-5.0, 1.0, np.nan]))
    assert c["solved"] == 2 and c["viol"].tolist() == [1, 1] and c["min_cbc"].tolist() == [-np.inf, -np.inf]


# ------------------------------------------------------------------------------------------------ the entry's argument checks
NPTR = 45
ROWS0, Z, XDOT, CBC, VIOL, SOLVED, MINCBC, UHELD, HELD = 26, 32, 33, 34, 35, 36, 37, 38, 39
GOOD = dict(Bt=5, Bh=5, Kob=2, Nte=64, P=10, tau_min=1e-3, tau_max=0.05, dt_plan=0.05, null=())
GROUP_P, GROUP_H = tuple(range(Z, MINCBC + 1)), tuple(range(UHELD, NPTR))
BAD = [(dict(null=(0,)), "null control-step buffer"), (dict(null=(15,)), "null in/out"), (dict(null=(13,)), "null planner table")] \
    + [(dict(null=(k,)), "null row of the solve") for k in range(ROWS0, ROWS0 + 6)] \
    + [(dict(null=(Z,)), "need the draws z"), (dict(null=(Z, XDOT, CBC)), "need the draws z"), (dict(null=(Z, CBC, VIOL, SOLVED, MINCBC)), "need the draws z"),
       (dict(null=(VIOL,)), "given together"), (dict(null=(SOLVED, MINCBC)), "given together"), (dict(null=GROUP_H + (MINCBC,)), "given together")] \
    + [(dict(null=(k,)), "the audit buffers") for k in GROUP_H] \
    + [(dict(null=GROUP_H[1:]), "the audit buffers"), (dict(null=GROUP_P + (HELD,)), "the audit buffers"),
       (dict(Kob=0), "Kob"), (dict(Kob=4), "BCBF_MAX_QUAD_CONSTRAINTS"), (dict(Kob=7), "BCBF_MAX_QUAD_CONSTRAINTS"), (dict(Kob=8), "Kob"),
       (dict(tau_min=0.1), "tau_min > tau_max"), (dict(Bh=2), "Bh must be 1 or Bt"), (dict(Nte=0), "Nte < 1")]


def _call(lib, suf, a):
    """The entry on fake pointers: positions 0-25 as bcbf_unicycle_trigger_step takes them (tests/test_self_triggered_cpu.py),
    26-31 Bk / A / grad / cst / sign / rho, 32-37 z / xdot_s / cbc_s / viol / solved / min_cbc, 38-44 the audit's seven."""
    ptr = [ctypes.c_void_p(4096 * (k + 1)) for k in range(NPTR)]
    for k in a["null"]:
        ptr[k] = None
    fn = getattr(lib.lib, "bcbf_unicycle_trigger_step_audit" + suf)
    return fn(*ptr[:9], 96.4, *ptr[9:13], 1e-4, 1e-2, 1.0, a["tau_min"], a["tau_max"], 10.0, 12.0, ptr[13], ptr[14], a["dt_plan"],
              *ptr[15:NPTR], a["Bt"], a["Bh"], a["Kob"], a["Nte"], a["P"], None)


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("change,why", BAD, ids=["%d-%s" % (i, "-".join("%s%s" % (k, "_".join(map(str, v)) if isinstance(v, tuple) else v)
                                                                         for k, v in c.items())) for i, (c, w) in enumerate(BAD)])
def test_bad_arguments_are_refused_with_a_reason_and_no_hip_call(lib, suf, change, why):
    """Every case fails the host check, so the fake pointers are never used and no GPU is touched."""
    rc = _call(lib, suf, dict(GOOD, **change))
    assert rc == -1                                                                # BCBF_EINVAL
    msg = lib.lib.bcbf_last_error().decode()
    assert msg.startswith("bcbf_unicycle_trigger_step_audit" + suf) and why in msg, msg


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("null", [(), GROUP_P, GROUP_H, GROUP_P + GROUP_H, (XDOT, CBC), (VIOL, SOLVED, MINCBC)],
                         ids=["all", "no-P", "no-H", "neither", "no-xdot-cbc", "no-counters"])
def test_a_valid_call_passes_the_checks_and_fails_at_the_launch_without_a_gpu(lib, suf, null):
    """With every group complete or absent the host check passes; without a device the launch then fails: BCBF_ELAUNCH and HIP's
    message.  Not run where a GPU is present: a launch on these made-up pointers must never reach one."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the valid call on made-up pointers is only made where the launch cannot happen")
    rc = _call(lib, suf, dict(GOOD, null=null))
    assert rc == -2, (rc, lib.lib.bcbf_last_error().decode())                      # BCBF_ELAUNCH
    assert lib.lib.bcbf_last_error().decode().startswith("bcbf_unicycle_trigger_step_audit" + suf)


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "bcbf.h")).read()
    for name in ("bcbf_unicycle_trigger_step_audit_f32", "bcbf_unicycle_trigger_step_audit_f64"):
        assert name + "(" in header and name in lib.declared_symbols() and hasattr(lib.lib, name)


# ------------------------------------------------------------------------------------------------ the ops binding
def _binding_inputs(Bt=4, Kob=2, Nte=5):
    import torch
    from bayesian_cbf_amd import ops
    f = dict(dtype=torch.float64)
    task = dict(centers=torch.zeros(Bt, Kob, 2, **f), tw=torch.ones(2, **f), plan=torch.zeros(Bt, 3, **f), dot_plan=torch.zeros(Bt, 3, **f),
                sign=torch.ones(1 + Kob, **f), rho=torch.ones(Bt, **f))
    ws = ops.control_workspace(Bt, Kob, torch.float64, "cpu")
    tws = ops.trigger_workspace(Bt, torch.float64, "cpu")
    hyper = dict(ls=torch.ones(1, 3, **f), sf=torch.ones(1, **f), Adiag=torch.ones(1, 3, **f), B=torch.eye(3, **f)[None].contiguous())
    pos = (task, ws, tws, torch.zeros(Bt, 3, **f), torch.zeros(Nte, 3, **f), 1.0, hyper, torch.zeros(3, 3, **f), torch.zeros(3, 3, **f), 0.05,
           1.0, 1e-3, 0.05)
    return pos, ops.trigger_audit_workspace(Bt, Kob, torch.float64, "cpu"), torch.eye(3, **f).expand(Bt, 3, 3).contiguous()


def test_workspace_shapes_and_starting_values(lib):
    import torch
    from bayesian_cbf_amd import ops
    aws = ops.trigger_audit_workspace(3, 2, torch.float32, "cpu")
    s, a = aws["sampled"], aws["audit"]
    assert list(s) == ["z", "xdot_s", "cbc_s", "viol", "solved", "min_cbc"]
    assert list(a) == ["u_held", "held", "held_mean", "held_margin", "audit_n", "audit_neg", "audit_min"]
    shapes = dict(z=(3, 3), xdot_s=(3, 3), cbc_s=(3, 3), viol=(3, 2), solved=(3,), min_cbc=(3, 2), u_held=(3, 2), held=(3,), held_mean=(3, 2),
                  held_margin=(3, 2), audit_n=(3,), audit_neg=(3, 2, 2), audit_min=(3, 2, 2))
    for k, v in {**s, **a}.items():
        assert tuple(v.shape) == shapes[k], k
        assert v.dtype == (torch.int32 if k in ("viol", "solved", "held", "audit_n", "audit_neg") else torch.float32), k
        assert bool((v == (math.inf if k in ("min_cbc", "audit_min") else 0)).all()), k


def test_binding_refuses_wrong_buffers_with_value_errors(lib):
    """The checks of the new arguments come before the device check, so they can be exercised on host tensors; a call that passes
    them then meets the refusal of host tensors (there is no CPU path)."""
    import torch
    from bayesian_cbf_amd import ops
    pos, aws, A = _binding_inputs()
    prep = ops.unicycle_trigger_step_prepare
    s, a = aws["sampled"], aws["audit"]
    with pytest.raises(ValueError, match="gp_A"):
        prep(*pos, sampled=s)
    with pytest.raises(ValueError, match="gp_A"):
        prep(*pos, gp_A=A[:2], audit=a)
    with pytest.raises(ValueError, match=r"sampled\['z'\] is required"):
        prep(*pos, gp_A=A, sampled=dict(s, z=None))
    with pytest.raises(ValueError, match=r"sampled\['z'\]"):
        prep(*pos, gp_A=A, sampled=dict(s, z=s["z"][:3]))
    with pytest.raises(ValueError, match=r"sampled\['cbc_s'\]"):
        prep(*pos, gp_A=A, sampled=dict(s, cbc_s=torch.zeros(4, 2, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"sampled\['xdot_s'\]"):
        prep(*pos, gp_A=A, sampled=dict(s, xdot_s=s["xdot_s"].float()))
    with pytest.raises(ValueError, match=r"sampled\['viol'\]"):
        prep(*pos, gp_A=A, sampled=dict(s, viol=s["viol"].long()))
    with pytest.raises(ValueError, match="given together"):
        prep(*pos, gp_A=A, sampled=dict(s, solved=None))
    with pytest.raises(ValueError, match="no buffer"):
        prep(*pos, gp_A=A, sampled=dict(s, held=a["held"]))
    with pytest.raises(ValueError, match=r"audit\['audit_min'\] is required"):
        prep(*pos, gp_A=A, audit={k: v for k, v in a.items() if k != "audit_min"})
    with pytest.raises(ValueError, match=r"audit\['audit_neg'\]"):
        prep(*pos, gp_A=A, audit=dict(a, audit_neg=torch.zeros(4, 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"audit\['u_held'\]"):
        prep(*pos, gp_A=A, audit=dict(a, u_held=torch.zeros(4, 4, dtype=torch.float64)[:, :2]))
    task, ws = pos[0], pos[1]
    with pytest.raises(ValueError, match=r"ws\['grad'\]"):
        prep(*((task, dict(ws, grad=ws["grad"][:, :2])) + pos[2:]), gp_A=A, audit=a)
    with pytest.raises(ValueError, match="sign"):
        prep(*((dict(task, sign=torch.ones(2, dtype=torch.float64)), ws) + pos[2:]), gp_A=A, audit=a)
    for kw in (dict(sampled=s), dict(audit=a), dict(sampled=s, audit=a), {}):
        with pytest.raises(RuntimeError, match="ROCm device tensors"):
            prep(*pos, gp_A=A, **kw)


def test_loop_refuses_an_unknown_plant(lib):
    from bayesian_cbf_amd import rollouts
    hyper = dict(ls=[1.0, 1.0, 1.0], sf=1.0, A=np.eye(3), B=np.eye(3))
    with pytest.raises(ValueError, match="plant must be"):
        rollouts.self_triggered_rollouts(4, horizon=1.0, trigger_hyper=hyper, plant="drawn", device="cpu")
