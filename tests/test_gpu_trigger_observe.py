"""GPU tests of the self-triggered event that observes itself (bcbf_unicycle_trigger_step_observe,
ops.unicycle_trigger_step_prepare(observe=...)) and of the loop that learns from it (rollouts.self_triggered_learning_rollouts): one
event against the audit entry (bit for bit) and the numpy yardstick tests/_trigger_observe_reference.py; the three groups together;
the loop row by row, its final model against the oracle's refit of the rows it holds; eager against graph; fp32; the audit."""
import ctypes

import numpy as np
import pytest
import torch

import _trigger_observe_reference as TO
import test_gpu_self_triggered as G                      # hyper-parameters and test points of the one-event tests, loop conventions
from test_gpu_learning import _final_vs_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP = G.NP
OLD_OUT = ("tau", "Lfh", "Lkd", "Lh", "xvel", "uBu", "dt_used")
SENTINEL = 7.0
L_MEAN = G.L_MEAN


def raw(t):
    return t.detach().cpu().numpy()


def bits(t):
    return raw(t.contiguous()).tobytes()


_STATES = {}


def solved_state(dtype, Bt, Kob):
    """test_gpu_self_triggered.solved_state with Kob of the task's two obstacles: the batch after the fused solve with dt = 0 on a
    learned model.  Built once per (precision, batch, Kob)."""
    key = (dtype, Bt, Kob)
    if key in _STATES:
        return _STATES[key]
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    task = make_unicycle_task(Bt, dtype=dtype, device=DEV, seed=81)
    for k, n in (("centers", Kob), ("radii", Kob)):
        task[k] = task[k][:, :n].contiguous()
    for k, n in (("gammas", Kob), ("sign", 1 + Kob), ("relax_mask", 1 + Kob)):
        task[k] = task[k][:n].contiguous()
    p = make_instances(Bt, G.NTRAIN, 3, 2, dtype=dtype, device=DEV, seed=82)
    jit = p["jitter"]
    for _ in range(4):
        Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit)
        if not bool((info != 0).any()):
            break
        jit = torch.where((info != 0)[:, None], jit * 10, jit).contiguous()
    assert int((info != 0).sum()) == 0
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=(0.01 * p["A"]).contiguous())
    ws = ops.control_workspace(Bt, Kob, dtype, DEV)
    x = task["x"].clone()
    ops.unicycle_control_step_prepare(gp, task, ws, x, dt=0.0, L_true=G.L_TRUE, L_mean=L_MEAN, clf_gamma=10.0, max_iters=40)()
    torch.cuda.synchronize()
    assert torch.equal(x, task["x"])
    _STATES[key] = dict(task=task, ws=ws, x=x, gp=gp, Kob=Kob)
    return _STATES[key]


def run_event(st, hyper, off, dtype, events, t0, status, t_end, observe=None, groups="", z=None, tau_min=1e-9, tau_max=10.0):
    """One trigger step on a copy of the solved state.  observe = None: bcbf_unicycle_trigger_step_audit (through ctypes when no group
    is named, so that the entry runs with every optional pointer NULL); else dict(ld, row0, every, shift_invariant): the observing
    entry through the binding, stream buffers and xq_next pre-filled with the sentinel.  groups: "", "P", "H" or "PH"."""
    from bayesian_cbf_amd import _lib, ops
    from bayesian_cbf_amd import trigger_interval as ti
    Bt, Kob = st["x"].shape[0], st["Kob"]
    f = dict(dtype=dtype, device=DEV)
    x = st["x"].clone()
    ws = dict(st["ws"], status=status.clone())
    task = dict(st["task"], plan=torch.full((Bt, 3), -5.0, **f), dot_plan=torch.full((Bt, 3), -6.0, **f))
    tws = ops.trigger_workspace(Bt, dtype, DEV)
    for k in OLD_OUT:
        tws[k].fill_(SENTINEL)
    tws["t"].copy_(torch.as_tensor(t0, dtype=torch.float64))
    tws["events"].copy_(torch.as_tensor(events, dtype=torch.int32))
    plan_all = torch.arange(3.0 * G.P_ROWS, **f).reshape(G.P_ROWS, 3).contiguous()
    dplan_all = (-plan_all - 1).contiguous()
    r = ti._grid_norm(G.host(off))
    A = st["gp"]["A"]
    aws = None
    if groups:
        aws = ops.trigger_audit_workspace(Bt, Kob, dtype, DEV)
        for grp in aws.values():
            for v in grp.values():
                v.fill_(7)
        if "P" in groups:
            aws["sampled"]["z"].copy_(z)
    kw = dict(gp_A=A, sampled=aws["sampled"] if "P" in groups else None, audit=aws["audit"] if "H" in groups else None)
    pos = (task, ws, tws, x, off, r, hyper, plan_all, dplan_all, G.DT_PLAN, t_end, tau_min, tau_max)
    ow = None
    if observe is not None:
        ow = ops.trigger_observe_workspace(Bt, observe["ld"], dtype, DEV)
        for v in ow["obs"] + (ow["xq_next"],):
            v.fill_(SENTINEL)
        ow.update(row0=observe["row0"], every=observe["every"], shift_invariant=observe["shift_invariant"], L_mean=L_MEAN)
        ops.unicycle_trigger_step_prepare(*pos, L_true=G.L_TRUE, observe=ow, **kw)()
    elif groups:
        ops.unicycle_trigger_step_prepare(*pos, L_true=G.L_TRUE, **kw)()
    else:
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        fn = getattr(_lib.lib, "bcbf_unicycle_trigger_step_audit" + ("_f64" if dtype == torch.float64 else "_f32"))
        rc = fn(p(x), p(ws["y"]), p(ws["status"]), p(ws["fhat"]), p(ws["ghat"]), p(ws["Mk"]), p(task["centers"]), p(task["tw"]), p(off), float(r),
                p(hyper["ls"]), p(hyper["sf"]), p(hyper["Adiag"]), p(hyper["B"]), 1e-4, 1e-2, 1.0, float(tau_min), float(tau_max), float(t_end),
                float(G.L_TRUE), p(plan_all), p(dplan_all), float(G.DT_PLAN), p(tws["t"]), p(tws["events"]), p(task["plan"]), p(task["dot_plan"]),
                *[p(tws[k]) for k in ("tau", "dt_used", "Lfh", "Lkd", "Lh", "xvel", "uBu")], p(ws["Bk"]), p(A), p(ws["grad"]), p(ws["cst"]),
                p(task["sign"]), p(task["rho"]), *([None] * 13), Bt, hyper["ls"].shape[0], Kob, off.shape[0], G.P_ROWS,
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _lib.lib.bcbf_last_error().decode()
    torch.cuda.synchronize()
    return dict(x=x, task=task, tws=tws, ws=ws, aws=aws, ow=ow)


def same_event(a, b):
    """Everything the audit entry writes, bit for bit."""
    for k in OLD_OUT + ("t", "events"):
        assert bits(a["tws"][k]) == bits(b["tws"][k]), k
    assert bits(a["x"]) == bits(b["x"])
    assert bits(a["task"]["plan"]) == bits(b["task"]["plan"]) and bits(a["task"]["dot_plan"]) == bits(b["task"]["dot_plan"])
    if a["aws"] is not None:
        for grp in ("sampled", "audit"):
            for k, v in a["aws"][grp].items():
                assert bits(v) == bits(b["aws"][grp][k]), (grp, k)


def check_row(got_x, got_uh, got_y, ref, what):
    """obs_x, obs_uh bit for bit; obs_y within the yardstick's derived bound (printed first)."""
    err = np.abs(got_y.astype(np.float64) - ref["obs_y"].astype(np.float64))
    print("MEASURED %s: |obs_y - reference| %s, bound %s" % (what, err.tolist(), ref["bound"].tolist()))
    assert got_x.tobytes() == ref["obs_x"].tobytes(), (what, got_x, ref["obs_x"])
    assert got_uh.tobytes() == ref["obs_uh"].tobytes(), (what, got_uh, ref["obs_uh"])
    assert (err <= ref["bound"]).all(), (what, err, ref["bound"])


# ------------------------------------------------------------------------------------------------ 1. one event, group O alone
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("si", [True, False], ids=["shift-invariant", "raw-inputs"])
@pytest.mark.parametrize("Kob", [1, 2])
@pytest.mark.parametrize("Nte", [27, 65])
def test_one_event_group_o_alone(Nte, Kob, si, dtype):
    """Six instances: a solved one (event 0 -> the first stream row), one made unsolved by rewriting the status buffer, a finished
    one, one whose event count is no multiple of obs_every, one whose row index is past obs_ld, and one more writer.  Everything the
    audit entry writes: bit-identical to the audit entry on the same inputs.  obs_x, obs_uh, xq_next: bit-identical to the yardstick
    on the device's own x_before, x_after, u; obs_y within 8 eps (|dx_d / dt_b| + |u_0| + |u_1| / L_mean) of the yardstick evaluated
    in the working type from the stored x_after and dt_used.  Every other row of the streams still holds the sentinel."""
    Bt, every, row0, ld, t_end = 6, 3, 2, 8, 5.0
    st = solved_state(dtype, Bt, Kob)
    hyper, off = G.hyper_and_points(dtype, Bt, Nte, False, seed=100 * Kob + Nte)
    ok = np.flatnonzero(raw(st["ws"]["status"]) == 0)
    assert len(ok) >= 2, raw(st["ws"]["status"])
    solved_b, unsolved_b = int(ok[0]), int(ok[1])
    finished_b, skip_b, past_b, other_b = [b for b in range(Bt) if b not in (solved_b, unsolved_b)]
    events = np.zeros(Bt, dtype=np.int32)
    events[[solved_b, unsolved_b, finished_b, skip_b, past_b, other_b]] = [0, 3, 6, 4, 30, 9]
    t0 = np.zeros(Bt)
    t0[finished_b] = t_end
    status = st["ws"]["status"].clone()
    status[unsolved_b] = 2
    base = run_event(st, hyper, off, dtype, events, t0, status, t_end)
    new = run_event(st, hyper, off, dtype, events, t0, status, t_end, observe=dict(ld=ld, row0=row0, every=every, shift_invariant=si))
    same_event(new, base)
    assert raw(new["tws"]["events"]).tolist() == [int(e) + (b != finished_b) for b, e in enumerate(events)]
    X, UH, Y = (raw(v) for v in new["ow"]["obs"])
    xq = raw(new["ow"]["xq_next"])
    x0, x1, u, dtu, stat = raw(st["x"]), raw(new["x"]), raw(st["ws"]["y"])[:, :2], raw(new["tws"]["dt_used"]), raw(status)
    want_rows = {solved_b: row0, unsolved_b: row0 + 1, other_b: row0 + 3}
    assert {b: TO.row_index(int(events[b]), every, row0, ld) for b in range(Bt) if b != finished_b} == {**want_rows, skip_b: None, past_b: None}
    tag = "trigger observe Nte%d Kob%d %s %s " % (Nte, Kob, "si" if si else "raw", "f64" if dtype == torch.float64 else "f32")
    for b in range(Bt):
        written = np.zeros(ld, dtype=bool)
        if b == finished_b:
            assert (xq[b] == SENTINEL).all() and x1[b].tobytes() == x0[b].tobytes()
        else:
            ref = TO.observation(x0[b], x1[b], u[b], stat[b] == 0, dtu[b], L_MEAN, shift_invariant=si, dtype=NP[dtype])
            assert xq[b].tobytes() == ref["xq_next"].tobytes(), (b, xq[b], ref["xq_next"])
            if b in want_rows:
                k = want_rows[b]
                written[k] = True
                check_row(X[b, k], UH[b, k], Y[b, k], ref, tag + "instance %d" % b)
        for v in (X, UH, Y):
            assert (v[b][~written] == SENTINEL).all(), b
    assert UH[unsolved_b, row0 + 1].tolist() == [1, 0, 0] and Y[unsolved_b, row0 + 1].tolist() == [0, 0, 0]
    assert x1[unsolved_b].tobytes() == x0[unsolved_b].tobytes() and x1[solved_b].tobytes() != x0[solved_b].tobytes()
    assert np.abs(Y[solved_b, row0]).max() > 0 and np.abs(UH[solved_b, row0, 1:]).max() > 0


# ------------------------------------------------------------------------------------------------ 2. all three groups together
def test_all_three_groups_together_the_row_records_the_drawn_plant():
    """fp64, Bt = 4, Nte = 27, groups P, H and O on.  The outputs of P and H, and everything else the audit entry writes, are
    bit-identical to the audit entry on the same inputs.  The row is that of the yardstick on the stored states, and it records the
    DRAWN plant: obs_y = xdot_s - g_mean u within the same bound.  The hold is pinned to tau_min = tau_max = 1: the bound is derived
    for the arithmetic of the row, and obs_y is formed from the STORED new state, whose rounding (half an ulp of |x| <= 8, at most
    4 eps) enters divided by dt_b -- at dt_b = 1 that is below the bound as soon as |xdot_s| + |u_0| + |u_1| / L_mean >= 1/2."""
    dtype, Bt, Nte, Kob = torch.float64, 4, 27, 2
    st = solved_state(dtype, Bt, Kob)
    hyper, off = G.hyper_and_points(dtype, Bt, Nte, False, seed=31)
    status = st["ws"]["status"].clone()
    solved = raw(status) == 0
    assert solved.sum() >= 2
    z = torch.randn(Bt, 3, generator=torch.Generator(device=DEV).manual_seed(9), dtype=dtype, device=DEV)
    events, t0 = np.arange(Bt, dtype=np.int32), np.zeros(Bt)
    kw = dict(groups="PH", z=z, tau_min=1.0, tau_max=1.0)
    base = run_event(st, hyper, off, dtype, events, t0, status, 50.0, **kw)
    new = run_event(st, hyper, off, dtype, events, t0, status, 50.0, observe=dict(ld=Bt, row0=0, every=1, shift_invariant=True), **kw)
    same_event(new, base)
    assert (raw(new["tws"]["dt_used"]) == 1.0).all() and raw(new["aws"]["sampled"]["solved"]).tolist() == (7 + solved).tolist()
    X, UH, Y = (raw(v) for v in new["ow"]["obs"])
    x0, x1, u, xdot = raw(st["x"]), raw(new["x"]), raw(st["ws"]["y"])[:, :2], raw(new["aws"]["sampled"]["xdot_s"])
    for b in range(Bt):
        ref = TO.observation(x0[b], x1[b], u[b], solved[b], 1.0, L_MEAN, dtype=np.float64)
        check_row(X[b, b], UH[b, b], Y[b, b], ref, "trigger observe P+H+O instance %d" % b)
        rest = np.arange(Bt) != b
        assert all((v[b][rest] == SENTINEL).all() for v in (X, UH, Y))
        ub = u[b] if solved[b] else np.zeros(2)
        th = x0[b, 2]
        drawn = xdot[b] - np.array([np.cos(th) * ub[0], np.sin(th) * ub[0], ub[1] / L_MEAN])
        err = np.abs(Y[b, b] - drawn)
        print("MEASURED trigger observe P+H+O instance %d: |obs_y - (xdot_s - g_mean u)| %s, bound %s" % (b, err.tolist(), ref["bound"].tolist()))
        assert (err <= ref["bound"]).all(), (b, err, ref["bound"])
        if solved[b]:
            assert np.abs(xdot[b]).sum() + np.abs(ub[0]) + np.abs(ub[1]) / L_MEAN >= 0.5         # the condition the docstring states
        else:
            assert not xdot[b].any() and not Y[b, b].any() and x1[b].tobytes() == x0[b].tobytes()


# ------------------------------------------------------------------------------------------------ 3-6. the loop
# zeta: on the synthetic start model Lfh is of the order of 1e3, and with the default zeta = 1e-2 every tau is far below tau_min = 0.02
# (measured on the device, seeds 0-2, zeta 1e-2 and 1: all eight instances take all 60 events at tau_min, so no seed lets one finish
# early).  tau grows with log(zeta); at zeta = 1e8, seed 0, a few taus of instance 4 exceed tau_min and it finishes after 59 events,
# one iteration before the last refit (measured: events [60, 60, 60, 60, 59, 60, 60, 60]).
LOOP = dict(max_train=48, refit_every=12, obs_every=1, tau_min=0.02, tau_max=0.05, horizon=1.2, Nte=27, seed=0, zeta=1e8)
L_MEAN_LOOP = 1.0                                          # the loop's default prior wheelbase (the true one is 12)
E_LOOP = 60                                                # ceil(horizon / tau_min) iterations >= max_train + refit_every
_RUNS = {}


def loop(dtype, **kw):
    from bayesian_cbf_amd import rollouts
    key = (dtype,) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        _RUNS[key] = rollouts.self_triggered_learning_rollouts(8, dtype=dtype, device=DEV, **LOOP, **kw)
    return _RUNS[key]


def test_loop_rows_final_model_and_finished_instances_fp64():
    """fp64, record=True.  Every row an active instance wrote is the yardstick's row for the recorded states of that event (criteria of
    the one-event test).  The final model holds stream rows [r - 48, r), r = 48 + 60; no refit failed; every instance's final
    (Mk, Bk) is the oracle's from-scratch refit of the rows it holds with the jitter they were factored with, 1e-7 (the bound of
    tests/test_gpu_learning.py for this comparison).  At least one instance finishes before the last refit: from then on its state,
    clock, event count and statistics stand still, and the stream rows it never wrote are still the plant at rest."""
    out = loop(torch.float64, record=True)
    rec = {k: raw(v) for k, v in out["rec"].items()}
    Bt, W, E = 8, LOOP["max_train"], E_LOOP
    assert rec["active"].shape == (E, Bt) and out["learning"]["refits"] == E // LOOP["refit_every"] == 5
    events = raw(out["events"])
    print("MEASURED learning loop fp64: events per instance %s, share_at_tau_min %s, refits %s" % (events.tolist(), out["share_at_tau_min"], out["learning"]))
    checked = 0
    for e in range(E):
        for b in range(Bt):
            if not rec["active"][e, b]:
                continue
            ref = TO.observation(rec["x_before"][e, b], rec["x_after"][e, b], rec["u"][e, b], rec["status"][e, b] == 0, rec["dt_used"][e, b],
                                 L_MEAN_LOOP, dtype=np.float64)
            err = np.abs(rec["obs_y"][e, b] - ref["obs_y"])
            assert rec["obs_x"][e, b].tobytes() == ref["obs_x"].tobytes() and rec["obs_uh"][e, b].tobytes() == ref["obs_uh"].tobytes(), (e, b)
            assert (err <= ref["bound"]).all(), (e, b, err, ref["bound"])
            assert rec["xq"][e, b].tolist() == [0, 0, rec["x_before"][e, b, 2]]
            checked += 1
    assert checked == events.sum() and np.array_equal(raw(out["learning"]["rows_written"]), events)
    fin = out["final"]
    sr = fin["stream_rows"]
    r = W + E
    assert sr["row0"] == W and sr["X"].shape[1] == r and fin["window_lo"] == r - W
    rows = fin["rows"][0]
    for k in ("X", "UH", "Y"):
        assert torch.equal(rows[k], sr[k][:, r - W:r]), k
        assert np.array_equal(raw(sr[k])[:, W:].transpose(1, 0, 2)[rec["active"]], rec["obs_" + {"X": "x", "UH": "uh", "Y": "y"}[k]][rec["active"]]), k
    assert out["learning"]["refit_failures_after_retries"] == 0
    worst = _final_vs_oracle(fin, 1e-7, "self-triggered learning loop fp64")
    print("MEASURED learning loop fp64: worst |dMk| %.2e |dBk| %.2e vs the oracle's refit" % tuple(worst))
    # the instances that finished before the last refit (it follows iteration E - 1)
    early = np.flatnonzero(events < E)
    assert len(early) >= 1, events
    rest = TO.rest_row(np.float64)
    for b in early:
        n = int(events[b])
        assert rec["active"][:n, b].all() and not rec["active"][n:, b].any()
        assert (rec["t"][n - 1:, b] == LOOP["horizon"]).all() and raw(out["t"])[b] == LOOP["horizon"]
        for e in range(n, E):
            assert rec["x_before"][e, b].tobytes() == rec["x_after"][n - 1, b].tobytes() == rec["x_after"][e, b].tobytes()
            for k in ("cost", "fails", "min_h"):
                assert rec[k][e, b].tobytes() == rec[k][n - 1, b].tobytes(), (k, e, b)
        assert raw(out["x_final"])[b].tobytes() == rec["x_after"][n - 1, b].tobytes()
        for k, name in (("X", "obs_x"), ("UH", "obs_uh"), ("Y", "obs_y")):
            assert np.array_equal(raw(sr[k])[b, W + n:], np.broadcast_to(rest[name], (E - n, 3))), (k, b)


def test_loop_eager_and_graph_agree_bit_for_bit():
    a, b = loop(torch.float64), loop(torch.float64, use_graph=True)
    for k in ("x_final", "t", "events"):
        assert bits(a[k]) == bits(b[k]), k
    assert bits(a["learning"]["rows_written"]) == bits(b["learning"]["rows_written"])
    for k in ("refits", "refit_failures_after_retries", "instances_factored_per_retry_level", "jitter_level_max"):
        assert a["learning"][k] == b["learning"][k], k
    fa, fb = a["final"], b["final"]
    for k in ("X", "UH", "Y", "jitter"):
        assert bits(fa["rows"][0][k]) == bits(fb["rows"][0][k]), k
    assert bits(fa["posterior"][0]) == bits(fb["posterior"][0]) and bits(fa["posterior"][1]) == bits(fb["posterior"][1])
    assert fa["window_lo"] == fb["window_lo"] and bits(fa["stream_rows"]["Y"]) == bits(fb["stream_rows"]["Y"])
    # ... and the record does not change the run
    c = loop(torch.float64, record=True)
    assert bits(c["x_final"]) == bits(a["x_final"]) and bits(c["final"]["posterior"][0]) == bits(fa["posterior"][0])


def test_loop_fp32_runs_and_reports_its_deviation():
    """fp32 on self-generated rows is not a parity path (tests/test_gpu_learning.py): the loop runs, every output is finite, no
    refit failed after the retries; the deviation of the final model from the fp64 refit of the same rows is recorded, not asserted."""
    from _tolreport import _record
    from bayesian_cbf_amd.rollouts import final_model_vs_fp64_refit
    out = loop(torch.float32)
    assert out["learning"]["refit_failures_after_retries"] == 0 and out["learning"]["refits"] == 5
    print("MEASURED learning loop fp32: done %s (0.02 rounds DOWN in fp32, so an instance held at tau_min for all 60 iterations ends an ulp "
          "short of the horizon), events %s" % (out["done"], raw(out["events"]).tolist()))
    for k in ("x_final", "t", "min_h", "dist_to_goal"):
        assert bool(torch.isfinite(out[k]).all()), k
    fin = out["final"]
    assert all(bool(torch.isfinite(v).all()) for v in fin["posterior"]) and all(bool(torch.isfinite(v).all()) for v in fin["rows"][0].values())
    assert fin["posterior"][0].dtype == torch.float32
    chk = final_model_vs_fp64_refit(fin)
    assert chk["refit_failures"] == 0 and np.isfinite(chk["Mk"]) and np.isfinite(chk["Bk"]), chk
    _record("self-triggered learning loop fp32 vs fp64 refit of the same rows (measured, not asserted)", max(chk["Mk"], chk["Bk"]), float("inf"))
    print("MEASURED learning loop fp32: vs fp64 refit of the same rows Mk %.2e Bk %.2e; %s" % (chk["Mk"], chk["Bk"], out["learning"]))


def test_loop_audit_counts_the_events_taken_with_a_held_control():
    out = loop(torch.float64, record=True, audit=True)
    rec = out["rec"]
    held = raw(rec["active"]) & (raw(rec["held"]) != 0)
    assert out["audit"]["events"] == int(held.sum()) > 0
    plain = loop(torch.float64, record=True)
    assert bits(plain["x_final"]) == bits(out["x_final"]) and "audit" not in plain
