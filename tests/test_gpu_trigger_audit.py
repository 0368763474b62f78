"""GPU tests of the self-triggered event on a posterior-drawn plant with the held-control audit (bcbf_unicycle_trigger_step_audit,
ops.unicycle_trigger_step_prepare(sampled=..., audit=...), rollouts.self_triggered_rollouts(plant="posterior", audit=True)): one
event against the existing entry (bit for bit where the plant does not enter), the numpy yardstick tests/_trigger_audit_reference.py
and the sampled control step; unsolved and finished instances; the audit across two events; the calibration of the empirical risk;
the loop, event by event; eager against graph and the defaults against the old binding."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _trigger_audit_reference as TA
import test_gpu_self_triggered as G                      # the solved states (built once, shared with that module's tests) and loop settings
from test_gpu_posterior_plant import close               # the project's bound for this arithmetic: 1e-12 scale (fp64), 2 ulp(scale) (fp32)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP = G.NP
KOB = 2
OLD_OUT = ("tau", "Lfh", "Lkd", "Lh", "xvel", "uBu", "dt_used")


def raw(t):
    return t.detach().cpu().numpy()


def bits(t):
    return raw(t.contiguous()).tobytes()


def filled_workspace(Bt, dtype, fill=7):
    """The buffers of groups P and H, every one filled with 7 so that a row the kernel does not write shows."""
    from bayesian_cbf_amd import ops
    aws = ops.trigger_audit_workspace(Bt, KOB, dtype, DEV)
    for grp in aws.values():
        for v in grp.values():
            v.fill_(fill)
    return aws


def run_event(st, hyper, off, dtype, entry="old", z=None, aws=None, groups="", status=None, t0=None, t_end=10.0, tau_min=1e-9, tau_max=10.0,
              zeta=1e-2):
    """One trigger step on a copy of the solved state, with the inputs of test_gpu_self_triggered.run_event.  entry: "old" (the
    existing binding), "raw" (the new entry through ctypes with every optional group NULL) or "new" (the new binding with the
    groups named in `groups`: "P", "H" or "PH", buffers from `aws`, z copied into them)."""
    from bayesian_cbf_amd import _lib, ops
    from bayesian_cbf_amd import trigger_interval as ti
    Bt = st["x"].shape[0]
    f = dict(dtype=dtype, device=DEV)
    x = st["x"].clone()
    ws = dict(st["ws"])
    if status is not None:
        ws["status"] = status.clone()
    task = dict(st["task"], plan=torch.full((Bt, 3), -5.0, **f), dot_plan=torch.full((Bt, 3), -6.0, **f))
    tws = ops.trigger_workspace(Bt, dtype, DEV)
    for k in OLD_OUT:
        tws[k].fill_(7.0)
    if t0 is not None:
        tws["t"].copy_(torch.as_tensor(t0, dtype=torch.float64))
    tws["events"].copy_(torch.arange(Bt, dtype=torch.int32))
    before = dict(t=tws["t"].clone(), events=tws["events"].clone())
    plan_all = torch.arange(3.0 * G.P_ROWS, **f).reshape(G.P_ROWS, 3).contiguous()
    dplan_all = (-plan_all - 1).contiguous()
    r = ti._grid_norm(G.host(off))
    pos = (task, ws, tws, x, off, r, hyper, plan_all, dplan_all, G.DT_PLAN, t_end, tau_min, tau_max)
    kw = dict(L_true=G.L_TRUE, zeta=zeta)
    A = st["gp"]["A"]
    if entry == "old":
        ops.unicycle_trigger_step_prepare(*pos, **kw)()
    elif entry == "new":
        if "P" in groups:
            aws["sampled"]["z"].copy_(z)
        ops.unicycle_trigger_step_prepare(*pos, gp_A=A, sampled=aws["sampled"] if "P" in groups else None,
                                          audit=aws["audit"] if "H" in groups else None, **kw)()
    else:
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        fn = getattr(_lib.lib, "bcbf_unicycle_trigger_step_audit" + ("_f64" if dtype == torch.float64 else "_f32"))
        rc = fn(p(x), p(ws["y"]), p(ws["status"]), p(ws["fhat"]), p(ws["ghat"]), p(ws["Mk"]), p(task["centers"]), p(task["tw"]), p(off), float(r),
                p(hyper["ls"]), p(hyper["sf"]), p(hyper["Adiag"]), p(hyper["B"]), 1e-4, float(zeta), 1.0, float(tau_min), float(tau_max), float(t_end),
                float(G.L_TRUE), p(plan_all), p(dplan_all), float(G.DT_PLAN), p(tws["t"]), p(tws["events"]), p(task["plan"]), p(task["dot_plan"]),
                *[p(tws[k]) for k in ("tau", "dt_used", "Lfh", "Lkd", "Lh", "xvel", "uBu")], p(ws["Bk"]), p(A), p(ws["grad"]), p(ws["cst"]),
                p(task["sign"]), p(task["rho"]), *([None] * 13), Bt, hyper["ls"].shape[0], KOB, off.shape[0], G.P_ROWS,
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _lib.lib.bcbf_last_error().decode()
    torch.cuda.synchronize()
    return dict(x=x, task=task, tws=tws, ws=ws, r=r, plan_all=plan_all, dplan_all=dplan_all, before=before, t_end=t_end, tau_min=tau_min,
                tau_max=tau_max, zeta=zeta, aws=aws, A=A)


def reference_events(st, run, hyper, off, dtype, z=None, u_held=None, held=None, counters=None):
    """The numpy yardstick on what the device saw (test_gpu_self_triggered.reference_events with the rows of the solve): the inputs as
    the working type holds them, the test points formed in it, the hold the device's plant saw."""
    Bt = st["x"].shape[0]
    ws, task = run["ws"], st["task"]
    x0, offn = raw(st["x"]), raw(off)
    shared = hyper["ls"].shape[0] == 1 and Bt > 1
    h = G.host
    dtu = h(run["tws"]["dt_used"])
    out = []
    for b in range(Bt):
        hb = 0 if shared else b
        Xtest = (offn + x0[b]).astype(NP[dtype]).astype(np.float64)
        out.append(TA.event(h(st["x"])[b], h(ws["y"])[b, :2], int(raw(ws["status"])[b]), h(ws["fhat"])[b], h(ws["ghat"])[b], h(ws["Mk"])[b],
                            h(task["centers"])[b], h(task["tw"]), offn, run["r"], h(hyper["ls"])[hb], float(h(hyper["sf"])[hb]),
                            h(hyper["Adiag"])[hb], h(hyper["B"])[hb], float(run["before"]["t"][b]), int(run["before"]["events"][b]),
                            h(run["plan_all"]), h(run["dplan_all"]), G.DT_PLAN, run["t_end"], run["tau_min"], run["tau_max"], G.L_TRUE,
                            Bk=h(ws["Bk"])[b], A=h(run["A"])[b], grad=h(ws["grad"])[b], cst=h(ws["cst"])[b], sign=h(task["sign"]),
                            rho=float(h(task["rho"])[b]), z=None if z is None else h(z)[b], u_held=None if u_held is None else u_held[b],
                            held=0 if held is None else held[b], counters=None if counters is None else counters[b], dtype=NP[dtype],
                            dt_used=dtu[b], zeta=run["zeta"], Xtest=Xtest))
    return out


def draws(Bt, dtype, seed):
    return torch.randn(Bt, 3, generator=torch.Generator(device=DEV).manual_seed(seed), dtype=dtype, device=DEV)


def stack(ref, key, live):
    return np.stack([ref[b][key] for b in live])


# ------------------------------------------------------------------------------------------------ 1. one event
SHAPES = [(Bt, Nte) for Bt in (1, 5, 67) for Nte in (1, 27, 65)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shared", [False, True], ids=["per-instance", "shared-model"])
@pytest.mark.parametrize("Bt,Nte", SHAPES, ids=["B%d-Nte%d" % s for s in SHAPES])
def test_one_event_against_the_existing_entry_the_yardstick_and_the_sampled_step(Bt, Nte, shared, dtype):
    """No optional group: every output, x, t, events and the planner rows are the existing entry's, bit for bit.  With z (and the
    audit): what does not depend on the plant still is; xdot_s, cbc_s, x against the numpy yardstick and xdot_s, cbc_s against
    bcbf_unicycle_control_step_sampled run with the same z and dt > 0 on a copy of the state, both at the bound of
    tests/test_gpu_posterior_plant.py (1e-12 scale / 2 ulp(scale): the reference is the same fp64 evaluation of the same stored
    inputs, rounded once)."""
    from bayesian_cbf_amd import ops
    st = G.solved_state(dtype, Bt)
    hyper, off = G.hyper_and_points(dtype, Bt, Nte, shared, seed=100 * Bt + Nte)
    old = run_event(st, hyper, off, dtype)
    plain = run_event(st, hyper, off, dtype, entry="raw")
    for k in OLD_OUT + ("t", "events"):
        assert bits(plain["tws"][k]) == bits(old["tws"][k]), k
    assert bits(plain["x"]) == bits(old["x"])
    assert bits(plain["task"]["plan"]) == bits(old["task"]["plan"]) and bits(plain["task"]["dot_plan"]) == bits(old["task"]["dot_plan"])
    # the audit alone leaves the true plant in place
    only_h = run_event(st, hyper, off, dtype, entry="new", aws=filled_workspace(Bt, dtype), groups="H")
    assert bits(only_h["x"]) == bits(old["x"]) and bits(only_h["tws"]["tau"]) == bits(old["tws"]["tau"])

    z = draws(Bt, dtype, 300 + Bt + Nte)
    new = run_event(st, hyper, off, dtype, entry="new", z=z, aws=filled_workspace(Bt, dtype), groups="PH")
    for k in OLD_OUT + ("t", "events"):
        assert bits(new["tws"][k]) == bits(old["tws"][k]), k
    assert bits(new["task"]["plan"]) == bits(old["task"]["plan"]) and bits(new["task"]["dot_plan"]) == bits(old["task"]["dot_plan"])
    solved = raw(st["ws"]["status"]) == 0
    ts = torch.as_tensor(solved, device=DEV)
    assert bits(new["x"][~ts]) == bits(st["x"][~ts]) and bits(new["x"][ts]) != bits(old["x"][ts])
    ref = reference_events(st, new, hyper, off, dtype, z=z)
    live = list(range(Bt))
    tag = "trigger audit B%d Nte%d %s %s " % (Bt, Nte, "shared" if shared else "per-inst", "f64" if dtype == torch.float64 else "f32")
    s = new["aws"]["sampled"]
    close(raw(s["xdot_s"]), stack(ref, "xdot_s", live), stack(ref, "scale_xdot", live), dtype, tag + "xdot_s")
    close(raw(s["cbc_s"]), stack(ref, "cbc_s", live), stack(ref, "scale_cbc", live), dtype, tag + "cbc_s")
    close(raw(new["x"]), stack(ref, "x", live), stack(ref, "scale_x", live), dtype, tag + "x")
    assert np.abs(raw(s["xdot_s"])[solved]).min() > 0
    # the sampled control step on a copy of the state: the same draw, made by the kernel this one restates
    x2, ws2 = st["x"].clone(), ops.control_workspace(Bt, KOB, dtype, DEV)
    f = dict(dtype=dtype, device=DEV)
    out = dict(z=z.clone(), xdot_s=torch.full((Bt, 3), 7.0, **f), cbc_s=torch.full((Bt, 1 + KOB), 7.0, **f))
    ops.unicycle_control_step_prepare(st["gp"], st["task"], ws2, x2, dt=0.05, L_true=G.L_TRUE, L_mean=G.L_MEAN, clf_gamma=10.0, max_iters=40,
                                      sampled=out)()
    torch.cuda.synchronize()
    assert bits(ws2["y"]) == bits(st["ws"]["y"]) and bits(ws2["status"]) == bits(st["ws"]["status"])
    close(raw(s["xdot_s"]), raw(out["xdot_s"]), stack(ref, "scale_xdot", live), dtype, tag + "xdot_s vs sampled step")
    close(raw(s["cbc_s"]), raw(out["cbc_s"]), stack(ref, "scale_cbc", live), dtype, tag + "cbc_s vs sampled step")


# ------------------------------------------------------------------------------------------------ 2. unsolved and finished
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_unsolved_and_finished_instances(dtype):
    """Two solved instances are made unsolved by rewriting the status buffer between the two launches: state kept bit for bit, zero
    xdot_s / cbc_s, not counted, held becomes 0 (they are still audited: held was 7).  One instance is finished: every buffer of it
    still holds the 7 it was filled with."""
    Bt, Nte = 13, 27
    st = G.solved_state(dtype, Bt)
    hyper, off = G.hyper_and_points(dtype, Bt, Nte, False, seed=7)
    ok = np.flatnonzero(raw(st["ws"]["status"]) == 0)
    assert len(ok) >= 6
    unsolved, done_b = ok[:2], ok[2]
    t_end = 5.0
    t0 = np.zeros(Bt)
    t0[done_b] = t_end
    status = st["ws"]["status"].clone()
    status[torch.as_tensor(unsolved, device=DEV)] = 2
    z = draws(Bt, dtype, 5)
    run = run_event(st, hyper, off, dtype, entry="new", z=z, aws=filled_workspace(Bt, dtype), groups="PH", status=status, t0=t0, t_end=t_end,
                    tau_min=1e-4, tau_max=0.05)
    s, a = run["aws"]["sampled"], run["aws"]["audit"]
    x0, x1 = raw(st["x"]), raw(run["x"])
    stat = raw(status)
    for b in unsolved:
        assert x1[b].tobytes() == x0[b].tobytes()
        assert not raw(s["xdot_s"])[b].any() and not raw(s["cbc_s"])[b].any()
        assert raw(s["solved"])[b] == 7 and (raw(s["viol"])[b] == 7).all() and (raw(s["min_cbc"])[b] == 7).all()
        assert raw(a["held"])[b] == 0 and raw(a["audit_n"])[b] == 8
        assert raw(run["tws"]["dt_used"])[b] == NP[dtype](0.05)
    for b in range(Bt):
        if b == done_b:
            continue
        assert raw(a["held"])[b] == int(stat[b] == 0) and raw(a["u_held"])[b].tobytes() == raw(st["ws"]["y"])[b, :2].tobytes()
        assert raw(s["solved"])[b] == 7 + int(stat[b] == 0)
    moved = [b for b in range(Bt) if stat[b] == 0 and b != done_b]
    assert all(x1[b].tobytes() != x0[b].tobytes() for b in moved)
    cb = raw(s["cbc_s"])[moved][:, 1:]
    np.testing.assert_array_equal(raw(s["viol"])[moved], 7 + (cb < 0))
    np.testing.assert_array_equal(raw(s["min_cbc"])[moved], np.minimum(cb, NP[dtype](7)))
    # the finished instance
    assert x1[done_b].tobytes() == x0[done_b].tobytes() and raw(run["tws"]["t"])[done_b] == t_end and raw(run["tws"]["events"])[done_b] == done_b
    for grp in (s, a):
        for k, v in grp.items():
            if k != "z":
                assert (raw(v)[done_b] == 7).all(), k
    for k in OLD_OUT:
        assert (raw(run["tws"][k])[done_b] == 7).all(), k


# ------------------------------------------------------------------------------------------------ 3. the audit across two events
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_audit_across_two_events_on_the_same_batch(dtype):
    """Event 1 (fresh workspace: held = 0) audits nothing.  The batch is solved again at the states event 1 left; event 2's
    held_mean, held_margin, counters and minima are the yardstick's on event 2's rows with event 1's control (bound: 1e-12 scale /
    2 ulp(scale), scale of margin = scale of mean + rho std).  Two instances made unsolved at event 1 are not audited at event 2."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd import trigger_interval as ti
    Bt, Nte = 13, 27
    st = G.solved_state(dtype, Bt)
    hyper, off = G.hyper_and_points(dtype, Bt, Nte, False, seed=11)
    f = dict(dtype=dtype, device=DEV)
    x = st["x"].clone()
    ws = {k: v.clone() for k, v in st["ws"].items()}
    task = dict(st["task"], plan=st["task"]["plan"].clone(), dot_plan=st["task"]["dot_plan"].clone())
    tws = ops.trigger_workspace(Bt, dtype, DEV)
    aws = ops.trigger_audit_workspace(Bt, KOB, dtype, DEV)
    s, a = aws["sampled"], aws["audit"]
    a["held_mean"].fill_(7.0)
    a["held_margin"].fill_(7.0)
    plan_all = torch.stack([st["task"]["plan"][0], st["task"]["plan"][0]]).contiguous()       # the planner stands still: both rows are
    dplan_all = torch.stack([st["task"]["dot_plan"][0], st["task"]["dot_plan"][0]]).contiguous()   # instance 0's; every instance gets them
    A = st["gp"]["A"]
    solve = ops.unicycle_control_step_prepare(st["gp"], task, ws, x, dt=0.0, L_true=G.L_TRUE, L_mean=G.L_MEAN, clf_gamma=10.0, max_iters=40)
    trig = ops.unicycle_trigger_step_prepare(task, ws, tws, x, off, ti._grid_norm(G.host(off)), hyper, plan_all, dplan_all, G.DT_PLAN, 10.0,
                                             1e-3, 0.05, L_true=G.L_TRUE, gp_A=A, sampled=s, audit=a)
    ok = np.flatnonzero(raw(ws["status"]) == 0)
    unsolved = ok[:2]
    ws["status"][torch.as_tensor(unsolved, device=DEV)] = 2
    status1, u1 = raw(ws["status"]).copy(), raw(ws["y"])[:, :2].copy()
    s["z"].copy_(draws(Bt, dtype, 21))
    trig()
    torch.cuda.synchronize()
    assert not raw(a["audit_n"]).any() and not raw(a["audit_neg"]).any() and np.isinf(raw(a["audit_min"])).all()
    assert (raw(a["held_mean"]) == 7).all() and (raw(a["held_margin"]) == 7).all()
    np.testing.assert_array_equal(raw(a["held"]), (status1 == 0).astype(np.int32))
    assert raw(a["u_held"]).tobytes() == u1.tobytes()
    solve()
    s["z"].copy_(draws(Bt, dtype, 22))
    trig()
    torch.cuda.synchronize()
    audited = status1 == 0
    assert audited.sum() >= 4 and not audited[unsolved].any()
    np.testing.assert_array_equal(raw(a["audit_n"]), audited.astype(np.int32))
    h = G.host
    tag = "trigger audit two events %s " % ("f64" if dtype == torch.float64 else "f32")
    want_neg, want_min = np.zeros((Bt, KOB, 2), dtype=np.int64), np.full((Bt, KOB, 2), np.inf)
    for b in range(Bt):
        if not audited[b]:
            assert (raw(a["held_mean"])[b] == 7).all() and (raw(a["held_margin"])[b] == 7).all()
            continue
        ref = TA.held_audit(u1[b], h(ws["fhat"])[b], h(ws["ghat"])[b], h(ws["Mk"])[b], h(ws["Bk"])[b], h(A)[b], h(ws["grad"])[b], h(ws["cst"])[b],
                            h(task["sign"]), float(h(task["rho"])[b]), dtype=NP[dtype])
        close(raw(a["held_mean"])[b], ref["held_mean"], ref["scale_mean"], dtype, tag + "held_mean")
        close(raw(a["held_margin"])[b], ref["held_margin"], ref["scale_margin"], dtype, tag + "held_margin")
        # the counters look at the values as stored
        c = TA.new_counters(KOB, NP[dtype])
        TA.count_audit(c, raw(a["held_mean"])[b], raw(a["held_margin"])[b])
        want_neg[b], want_min[b] = c["audit_neg"], c["audit_min"]
    np.testing.assert_array_equal(raw(a["audit_neg"]), want_neg)
    np.testing.assert_array_equal(raw(a["audit_min"]), want_min)
    assert raw(a["u_held"]).tobytes() == raw(ws["y"])[:, :2].tobytes()
    np.testing.assert_array_equal(raw(a["held"]), (raw(ws["status"]) == 0).astype(np.int32))


# ------------------------------------------------------------------------------------------------ 4. calibration
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("max_risk", [0.2, 0.05])
def test_empirical_risk_of_the_trigger_step_matches_the_risk_the_program_was_built_for(dtype, max_risk):
    """The recipe of tests/test_gpu_posterior_plant.py's calibration test -- 4096 instances driven at obstacle 0 on the fixed-kernel
    model, so that the cone of row 1 is active and the count of negative drawn conditions is binomial(n, max_risk) -- with the draw
    made by the trigger step after a dt = 0 solve.  Nte = 1 and tau_min = tau_max = 0.05: the hold does not depend on tau.
    |v - n delta| <= 5 sqrt(n delta (1 - delta))."""
    import _posterior_plant_reference as R
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.rollouts import unicycle_task_tensors
    Bt = 4096
    f = dict(dtype=dtype, device=DEV)
    f64 = dict(dtype=torch.float64, device="cpu")
    start, goal = torch.tensor((-3.0, -1.0, -math.pi / 4), **f64), torch.tensor((0.0, 0.0, math.pi / 4), **f64)
    task = unicycle_task_tensors(Bt, start, goal, dtype, torch.device(DEV), max_risk=max_risk)
    c0, r0 = raw(task["centers"])[0, 0].astype(np.float64), float(raw(task["radii"])[0, 0])
    rng = np.random.default_rng(2024)
    ang = rng.uniform(0.0, 2 * np.pi, Bt)
    dist = r0 * rng.uniform(1.02, 1.25, Bt)
    head = ang + np.pi + rng.uniform(-0.5, 0.5, Bt)
    ray = np.stack([np.cos(ang), np.sin(ang)], 1)
    xs = np.concatenate([c0 + dist[:, None] * ray, head[:, None]], 1)
    plan = np.concatenate([c0 - dist[:, None] * ray, head[:, None]], 1)
    x = torch.as_tensor(xs, **f).contiguous()
    x_start = x.clone()
    task["plan"], task["dot_plan"] = torch.as_tensor(plan, **f).contiguous(), torch.zeros(Bt, 3, **f)
    ws = ops.control_workspace(Bt, KOB, dtype, DEV)
    ws["Mk"].zero_()
    ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
    A = (1e-2 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous()
    ops.unicycle_control_step_prepare(dict(A=A), task, ws, x, dt=0.0, L_mean=1.0, clf_gamma=10.0)()
    tws = ops.trigger_workspace(Bt, dtype, DEV)
    aws = ops.trigger_audit_workspace(Bt, KOB, dtype, DEV)
    s = aws["sampled"]
    s["z"].copy_(torch.randn(Bt, 3, generator=torch.Generator(device=DEV).manual_seed(11), **f))
    hyper = dict(ls=torch.tensor([[0.5, 0.6, 0.7]], **f), sf=torch.tensor([0.8], **f), Adiag=torch.full((1, 3), 1e-2, **f),
                 B=torch.eye(3, **f)[None].contiguous())
    rows = torch.zeros(2, 3, **f)
    ops.unicycle_trigger_step_prepare(task, ws, tws, x, torch.zeros(1, 3, **f), 1.0, hyper, rows, rows.clone(), 0.05, 10.0, 0.05, 0.05,
                                      L_true=12.0, gp_A=A, sampled=s)()
    torch.cuda.synchronize()
    solved = raw(ws["status"]) == 0
    assert (raw(tws["dt_used"]) == NP[dtype](0.05)).all()
    mean, std = R.row_mean_std(raw(ws["y"]), raw(ws["Mk"]), raw(ws["Bk"]), raw(A), raw(ws["grad"]), raw(ws["cst"]), raw(ws["fhat"]),
                               raw(ws["ghat"]), raw(task["sign"]), 1)
    rho = float(task["rho"][0])
    active = solved & (mean - rho * std <= 1e-6 * (1 + np.abs(mean)))
    n, v = int(active.sum()), int((raw(s["cbc_s"])[:, 1][active] < 0).sum())
    print("max_risk %.2f %s: %d / %d solved, %d active, %d negative draws (rate %.4f)" % (max_risk, dtype, solved.sum(), Bt, n, v, v / max(n, 1)))
    assert solved.sum() >= 0.95 * Bt                                    # conditions of the test, not measurements
    assert n >= 0.9 * solved.sum()
    assert abs(v - n * max_risk) <= 5 * math.sqrt(n * max_risk * (1 - max_risk)), (v, n, max_risk)
    ts = torch.as_tensor(solved, device=DEV)
    assert bits(x[~ts]) == bits(x_start[~ts]) and int(raw(s["solved"]).sum()) == int(solved.sum())
    np.testing.assert_array_equal(raw(s["viol"])[:, 0], (raw(s["cbc_s"])[:, 1] < 0) & solved)


# ------------------------------------------------------------------------------------------------ 5. the loop
def _loop_kw(model, Bt):
    LOOP = G.LOOPS[model]
    return dict(LOOP, gp=G._learned_gp(Bt)) if model == "learned" else dict(LOOP, trigger_hyper=G.FIXED_HYPER)


@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_loop_event_by_event(model):
    """self_triggered_rollouts(8, record=True, plant="posterior", audit=True), fp64, the settings of the existing loop test.  Every
    event an instance took is replayed by the numpy yardstick from the recorded x_before, u, status, Mk, Bk and z, with grad, cst,
    fhat, ghat recomputed by the oracle's task functions: x_after, cbc_s and the audited rows within 1e-12 scale; t the running sum
    of dt_used, landing on the horizon; x_before[e+1] == x_after[e].  risk and audit equal a host recount of the record."""
    from bayesian_cbf_amd import rollouts, trigger_interval as ti
    from bayesian_cbf_amd.planner import PiecewiseLinearPlanner
    from oracle import control_step as ostep, unicycle as ouni
    import _trigger_reference as R
    Bt, LOOP = 8, G.LOOPS[model]
    kw = _loop_kw(model, Bt)
    out = rollouts.self_triggered_rollouts(Bt, record=True, dtype=torch.float64, device=DEV, plant="posterior", audit=True, **kw)
    rec = {k: (v.cpu().numpy() if v.dtype in (torch.int32, torch.bool) else G.host(v)) for k, v in out["rec"].items()}
    task = {k: G.host(v) for k, v in out["task"].items()}
    horizon, E = LOOP["horizon"], LOOP["max_events"]
    for k in ("z", "xdot_s", "cbc_s", "held", "held_mean", "held_margin"):
        assert rec[k].shape[:2] == (E, Bt), k
    if model == "learned":
        g = kw["gp"]
        hy = dict(ls=G.host(g["ell"]), sf=G.host(g["s2"]), Adiag=np.diagonal(G.host(g["A"]), axis1=-2, axis2=-1), B=G.host(g["Bm"]), A=G.host(g["A"]))
    else:
        one = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (Bt,) + np.shape(v))
        FH = G.FIXED_HYPER
        hy = dict(ls=one(FH["ls"]), sf=one(FH["sf"]), Adiag=one(np.diag(FH["A"])), B=one(FH["B"]), A=one(np.diag([1e-2, 1e-2, 1e-2])))
    x0, xg = torch.tensor([-3.0, -1.0, -math.pi / 4], dtype=torch.float64), torch.tensor([0.0, 0.0, math.pi / 4], dtype=torch.float64)
    numSteps = 3
    planner = PiecewiseLinearPlanner(x0, xg, numSteps, LOOP["dt"], frac_time_to_reach_goal=0.95)
    plan_all = np.stack([planner.plan(s).numpy() for s in range(numSteps)])
    dplan_all = np.stack([planner.dot_plan(s).numpy() for s in range(numSteps)])
    off = ti.default_test_grid(3, LOOP["Nte"])
    r = R.whole_norm(off)
    events, t_fin = out["events"].cpu().numpy(), G.host(out["t"])
    eps = np.finfo(np.float64).eps
    checked, audited_n = 0, 0
    counters = [TA.new_counters(KOB) for _ in range(Bt)]
    for b in range(Bt):
        t, n_ev, u_held, held = 0.0, 0, np.zeros(2), 0
        for e in range(E):
            if not rec["active"][e, b]:
                assert t == horizon and not rec["active"][e:, b].any()
                break
            xb, u, status = rec["x_before"][e, b], rec["u"][e, b], int(rec["status"][e, b])
            assert rec["held"][e, b] == held, (b, e)
            grad, cst, sign = ostep.constraint_rows(xb, rec["plan"][e, b], rec["dot_plan"][e, b], task["Kp"], 10.0, task["centers"][b],
                                                    task["radii"][b], task["tw"], task["gammas"])
            assert np.array_equal(sign, task["sign"])
            ev = TA.event(xb, u, status, ouni.ackermann_f(xb), ouni.ackermann_g(xb, LOOP["L_mean"]), rec["Mk"][e, b], task["centers"][b],
                          task["tw"], off, r, hy["ls"][b], float(hy["sf"][b]), hy["Adiag"][b], hy["B"][b], t, n_ev, plan_all, dplan_all,
                          LOOP["dt"], horizon, LOOP["tau_min"], LOOP["tau_max"], LOOP["L_true"], Bk=rec["Bk"][e, b], A=hy["A"][b], grad=grad,
                          cst=cst, sign=sign, rho=float(task["rho"][b]), z=rec["z"][e, b], u_held=u_held, held=held, counters=counters[b],
                          dt_used=rec["dt_used"][e, b], zeta=LOOP["zeta"])
            tag = "trigger audit loop %s " % model
            close(rec["x_after"][e, b], ev["x"], ev["scale_x"], torch.float64, tag + "x_after")
            close(rec["cbc_s"][e, b], ev["cbc_s"], ev["scale_cbc"], torch.float64, tag + "cbc_s")
            if status != 0:
                assert np.array_equal(rec["x_after"][e, b], xb) and not rec["cbc_s"][e, b].any()
            if ev["audited"]:
                close(rec["held_mean"][e, b], ev["held_mean"], ev["scale_mean"], torch.float64, tag + "held_mean")
                close(rec["held_margin"][e, b], ev["held_margin"], ev["scale_margin"], torch.float64, tag + "held_margin")
                audited_n += 1
            dtu = rec["dt_used"][e, b]
            assert 0 < dtu <= LOOP["tau_max"]
            t_next = t + dtu
            if rec["t"][e, b] == horizon and abs(t_next - horizon) <= 4 * eps * horizon:
                t_next = horizon                                          # the last, partial step lands on the horizon itself
            assert rec["t"][e, b] == t_next, (b, e, rec["t"][e, b], t_next)
            t, n_ev, checked = t_next, n_ev + 1, checked + 1
            u_held, held = ev["u_held_next"], ev["held_next"]
            if e + 1 < E:
                np.testing.assert_array_equal(rec["x_before"][e + 1, b], rec["x_after"][e, b])
        assert events[b] == n_ev and t_fin[b] == t
    assert checked >= Bt * 3 and audited_n >= Bt
    assert out["done"] == 1.0 and (t_fin == horizon).all() and (events <= math.ceil(horizon / LOOP["tau_min"])).all()
    # risk and audit: a host recount of the record (the device's own stored values)
    act = rec["active"]
    ok = act & (rec["status"] == 0)
    c = np.where(np.isfinite(rec["cbc_s"][:, :, 1:]), rec["cbc_s"][:, :, 1:], -np.inf)
    per = ((c < 0) & ok[:, :, None]).sum(axis=(0, 1))
    n = int(ok.sum())
    risk = out["risk"]
    assert risk["instance_steps"] == n and risk["violations"] == int(per.sum()) and risk["rate"] == per.sum() / (n * KOB)
    assert risk["max_risk"] == 0.01 and [p["violations"] for p in risk["per_obstacle"]] == [int(v) for v in per]
    assert risk["min_cbc"] == [float(v) for v in np.where(ok[:, :, None], c, np.inf).min(axis=(0, 1))]
    aud = act & (rec["held"] != 0)
    vals = np.stack([rec["held_mean"], rec["held_margin"]], -1)                      # [E, Bt, Kob, 2]
    neg = (~(vals >= 0) & aud[:, :, None, None]).sum(axis=(0, 1))
    mins = np.where(aud[:, :, None, None], np.where(np.isnan(vals), -np.inf, vals), np.inf).min(axis=(0, 1))
    a = out["audit"]
    na = int(aud.sum())
    assert a["events"] == na == audited_n == sum(cn["audit_n"] for cn in counters)
    assert a["neg_mean"] == [int(v) for v in neg[:, 0]] and a["neg_margin"] == [int(v) for v in neg[:, 1]]
    assert a["rate_mean"] == neg[:, 0].sum() / (na * KOB) and a["rate_margin"] == neg[:, 1].sum() / (na * KOB)
    assert a["min_mean"] == [float(v) for v in mins[:, 0]] and a["min_margin"] == [float(v) for v in mins[:, 1]]


# ------------------------------------------------------------------------------------------------ 6. eager, graph and defaults
@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_loop_eager_and_graph_agree(model):
    from bayesian_cbf_amd import rollouts
    Bt = 8
    kw = dict(_loop_kw(model, Bt), plant="posterior", audit=True)
    a = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, **kw)
    b = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, use_graph=True, **kw)
    for k in ("x_final", "t", "events", "min_h"):
        assert torch.equal(a[k], b[k]), k
    assert a["risk"] == b["risk"] and a["audit"] == b["audit"] and a["done"] == b["done"] == 1.0
    assert a["risk"]["instance_steps"] > 0 and a["audit"]["events"] > 0
    true = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, **_loop_kw(model, Bt))
    assert "risk" not in true and "audit" not in true and not torch.equal(true["x_final"], a["x_final"])


def test_defaults_are_the_loop_of_the_old_binding():
    """plant="true", audit=False (the defaults) against the same events restated with the entry points as they were called before
    the feature -- the solve with dt = 0, `unicycle_trigger_step_prepare` without the new arguments, nothing else: bit-identical
    states, clocks and event counts."""
    from bayesian_cbf_amd import ops, rollouts, trigger_interval as ti
    from bayesian_cbf_amd.planner import PiecewiseLinearPlanner
    Bt, LOOP = 8, G.LOOPS["fixed"]
    kw = _loop_kw("fixed", Bt)
    dflt = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, **kw)
    expl = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, plant="true", audit=False, **kw)
    f = dict(dtype=torch.float64, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(LOOP["seed"])
    x0, xg = torch.tensor((-3.0, -1.0, -math.pi / 4), **f), torch.tensor((0.0, 0.0, math.pi / 4), **f)
    task = rollouts.unicycle_task_tensors(Bt, x0, xg, torch.float64, torch.device(DEV), max_risk=0.01)
    numSteps = max(3, int(round(LOOP["horizon"] / LOOP["dt"])))
    planner = PiecewiseLinearPlanner(x0, xg, numSteps, LOOP["dt"], frac_time_to_reach_goal=0.95)
    x = (x0 + 0.05 * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    ws = ops.control_workspace(Bt, 2, torch.float64, DEV)
    tws = ops.trigger_workspace(Bt, torch.float64, DEV)
    ws["Mk"].zero_()
    ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
    A = torch.diag(torch.tensor((1e-2, 1e-2, 1e-2), **f)).expand(Bt, 3, 3).contiguous()
    FH = G.FIXED_HYPER
    hyper = rollouts._trigger_hyper(FH["ls"], FH["sf"], FH["A"], FH["B"], Bt, f)
    off_np = ti.default_test_grid(3, LOOP["Nte"])
    off = torch.as_tensor(off_np).to(**f).contiguous()
    plan_all = torch.stack([planner.plan(s).to(torch.float64) for s in range(numSteps)]).to(DEV).contiguous()
    dplan_all = torch.stack([planner.dot_plan(s).to(torch.float64) for s in range(numSteps)]).to(DEV).contiguous()
    task["plan"], task["dot_plan"] = plan_all[0].expand(Bt, 3).contiguous(), dplan_all[0].expand(Bt, 3).contiguous()
    solve = ops.unicycle_control_step_prepare(dict(A=A), task, ws, x, dt=0.0, L_true=LOOP["L_true"], L_mean=LOOP["L_mean"], max_iters=30)
    trig = ops.unicycle_trigger_step_prepare(task, ws, tws, x, off, ti._grid_norm(off_np), hyper, plan_all, dplan_all, LOOP["dt"],
                                             LOOP["horizon"], LOOP["tau_min"], LOOP["tau_max"], L_true=LOOP["L_true"], zeta=LOOP["zeta"])
    for _ in range(LOOP["max_events"]):
        solve()
        trig()
    torch.cuda.synchronize()
    for run in (dflt, expl):
        assert bits(run["x_final"]) == bits(x) and bits(run["t"]) == bits(tws["t"]) and bits(run["events"]) == bits(tws["events"])
        assert "risk" not in run and "audit" not in run


# ------------------------------------------------------------------------------------------------ 7. the shared definitions
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_risk_counters_are_those_of_rollout_risk(dtype):
    """The trigger step's risk counters and bcbf_rollout_risk call one rule.  A launch with draws and fresh counters on a batch with
    one instance made unsolved, one already at t_end and one with a NaN in an obstacle row's cst; then `ops.rollout_risk` on that
    launch's cbc_s and status into fresh counters: viol, solved and min_cbc agree bit for bit on the live instances (the NaN row a
    violation with minimum -inf in both), and the finished instance's counters are as the workspace made them."""
    from bayesian_cbf_amd import ops
    Bt, Nte = 5, 27
    st = G.solved_state(dtype, Bt)
    hyper, off = G.hyper_and_points(dtype, Bt, Nte, False, seed=31)
    ok = np.flatnonzero(raw(st["ws"]["status"]) == 0)
    assert len(ok) >= 2
    nan_b = int(ok[0])
    unsolved_b, done_b = [b for b in range(Bt) if b not in ok[:2]][:2]
    status, cst = st["ws"]["status"].clone(), st["ws"]["cst"].clone()
    status[unsolved_b] = 2
    cst[nan_b, 1] = float("nan")
    t_end, t0 = 5.0, np.zeros(Bt)
    t0[done_b] = t_end
    aws = ops.trigger_audit_workspace(Bt, KOB, dtype, DEV)
    run = run_event(dict(st, ws=dict(st["ws"], cst=cst)), hyper, off, dtype, entry="new", z=draws(Bt, dtype, 41), aws=aws, groups="P",
                    status=status, t0=t0, t_end=t_end, tau_min=1e-4, tau_max=0.05)
    s = aws["sampled"]
    fresh = ops.trigger_audit_workspace(Bt, KOB, dtype, DEV)["sampled"]
    ops.rollout_risk(s["cbc_s"], run["ws"]["status"], fresh["viol"], fresh["solved"], fresh["min_cbc"])
    torch.cuda.synchronize()
    live = torch.as_tensor([b != done_b for b in range(Bt)], device=DEV)
    for k in ("viol", "solved", "min_cbc"):
        assert bits(s[k][live]) == bits(fresh[k][live]), k
    assert np.isnan(raw(s["cbc_s"])[nan_b, 1]) and raw(s["viol"])[nan_b, 0] == 1 and raw(s["min_cbc"])[nan_b, 0] == -np.inf
    assert raw(s["solved"])[nan_b] == 1 and raw(s["solved"])[unsolved_b] == 0 and not raw(s["viol"])[unsolved_b].any()
    assert raw(s["solved"])[done_b] == 0 and not raw(s["viol"])[done_b].any() and (raw(s["min_cbc"])[done_b] == np.inf).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_plant_step_is_that_of_unicycle_step(dtype):
    """The plain entry's Euler step and bcbf_unicycle_step are one definition.  Nte = 1 and tau_min = tau_max = 0.01: every live
    solved instance holds the same dt, so `ops.unicycle_step` on a copy of the state with u = y[:, :2] and that dt gives the same x
    bit for bit on the solved instances; the instance made unsolved keeps its state."""
    from bayesian_cbf_amd import ops
    Bt, hold = 5, 0.01
    st = G.solved_state(dtype, Bt)
    hyper, off = G.hyper_and_points(dtype, Bt, 1, False, seed=32)
    ok = np.flatnonzero(raw(st["ws"]["status"]) == 0)
    assert len(ok) >= 2
    unsolved_b = int(ok[-1])
    status = st["ws"]["status"].clone()
    status[unsolved_b] = 2
    run = run_event(st, hyper, off, dtype, status=status, tau_min=hold, tau_max=hold)
    solved = torch.as_tensor(raw(status) == 0, device=DEV)
    assert (raw(run["tws"]["dt_used"][solved]) == NP[dtype](hold)).all()
    x2 = ops.unicycle_step(st["x"].clone(), st["ws"]["y"][:, :2].contiguous(), hold, G.L_TRUE)
    torch.cuda.synchronize()
    assert int(solved.sum()) >= 1 and bits(run["x"][solved]) == bits(x2[solved]) and bits(run["x"][solved]) != bits(st["x"][solved])
    assert bits(run["x"][unsolved_b]) == bits(st["x"][unsolved_b])
