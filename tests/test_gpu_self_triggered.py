"""GPU tests of the self-triggered closed loop (bcbf_unicycle_trigger_step, ops.unicycle_trigger_step_prepare,
rollouts.self_triggered_rollouts): one event against the existing path (trigger_interval_batch on the same state) and against the
numpy yardstick tests/_trigger_step_reference.py; the clamp classes; finished instances; the loop, event by event; and the periodic
loop, which must not notice any of it."""
import math

import numpy as np
import pytest
import torch

import _trigger_reference as R
import _trigger_step_reference as S
from _tolreport import all_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP = {torch.float64: np.float64, torch.float32: np.float32}
L_MEAN, L_TRUE, NTRAIN = 4.0, 12.0, 24
# fp32 bounds of the quantities this kernel adds, relative: 4 x the worst error measured against the fp64 yardstick over all the
# one-event cases below on the first green run (profiles/self_triggered_tol_report.txt); fp64: the floor of
# tests/test_gpu_trigger_interval.py
TOL32 = dict(uBu=2.4e-7, xvel=2.2e-7, Lh=2.4e-7, x=1.9e-7)         # measured 5.91e-8, 5.34e-8, 5.78e-8, 4.70e-8
FLOOR64 = 1e-12


def host(t):
    return t.detach().cpu().double().numpy()


_STATES = {}


def solved_state(dtype, Bt):
    """A batch after `bcbf_unicycle_control_step` with dt = 0 on a learned model of NTRAIN points per instance (so M_k != 0): the
    task, the workspace the trigger step reads, and the states.  Built once per (precision, batch)."""
    if (dtype, Bt) in _STATES:
        return _STATES[(dtype, Bt)]
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    task = make_unicycle_task(Bt, dtype=dtype, device=DEV, seed=81)
    p = make_instances(Bt, NTRAIN, 3, 2, dtype=dtype, device=DEV, seed=82)
    jit = p["jitter"]
    for _ in range(4):
        Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit)
        if not bool((info != 0).any()):
            break
        jit = torch.where((info != 0)[:, None], jit * 10, jit).contiguous()
    assert int((info != 0).sum()) == 0
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=(0.01 * p["A"]).contiguous())
    ws = ops.control_workspace(Bt, 2, dtype, DEV)
    x = task["x"].clone()
    ops.unicycle_control_step_prepare(gp, task, ws, x, dt=0.0, L_true=L_TRUE, L_mean=L_MEAN, clf_gamma=10.0, max_iters=40)()
    torch.cuda.synchronize()
    assert torch.equal(x, task["x"])                                   # dt = 0: solve only
    # the bearing of every obstacle is defined: the states stay at least 0.5 away from every centre
    dist = (task["x"][:, None, :2] - task["centers"]).norm(dim=-1)
    assert float(dist.min()) >= 0.5, float(dist.min())
    assert int((ws["status"] == 0).sum()) >= max(1, Bt // 2)
    _STATES[(dtype, Bt)] = dict(task=task, ws=ws, x=x, gp=gp)
    return _STATES[(dtype, Bt)]


def hyper_and_points(dtype, Bt, Nte, shared, seed):
    """Hyper-parameters of the bound (one set or one per instance) and the test offsets: the reference's grid for Nte = 729, else
    random points of the same extent; lengthscales of the order of the extent, so the maximising pair is in the interior."""
    rng = np.random.default_rng(seed)
    Bh = 1 if shared else Bt
    off = R.grid() if Nte == 729 else rng.normal(size=(Nte, 3)) * np.array([0.06, 0.06, 0.02])
    Bm = rng.normal(size=(Bh, 3, 3))
    h = dict(ls=0.1 * rng.uniform(0.5, 1.5, size=(Bh, 3)), sf=rng.uniform(0.5, 1.5, size=Bh), Adiag=1e-2 * rng.uniform(0.5, 2.0, size=(Bh, 3)),
             B=Bm @ Bm.transpose(0, 2, 1) + 0.1 * np.eye(3))
    t = lambda a: torch.as_tensor(a.astype(NP[dtype]), device=DEV).contiguous()
    return {k: t(v) for k, v in h.items()}, t(off)


P_ROWS, DT_PLAN = 7, 0.05


def run_event(st, hyper, off, dtype, t0=None, t_end=10.0, tau_min=1e-9, tau_max=10.0, zeta=1e-2, status=None):
    """One trigger step on a copy of the solved state.  Outputs start from 7, so a row the kernel does not write shows."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd import trigger_interval as ti
    Bt = st["x"].shape[0]
    f = dict(dtype=dtype, device=DEV)
    x = st["x"].clone()
    ws = dict(st["ws"])
    if status is not None:                       # (the status buffer rewritten between the two launches)
        ws["status"] = status.clone()
    task = dict(st["task"], plan=torch.full((Bt, 3), -5.0, **f), dot_plan=torch.full((Bt, 3), -6.0, **f))
    tws = ops.trigger_workspace(Bt, dtype, DEV)
    for k in ("tau", "dt_used", "Lfh", "Lkd", "Lh", "xvel", "uBu"):
        tws[k].fill_(7.0)
    if t0 is not None:
        tws["t"].copy_(torch.as_tensor(t0, dtype=torch.float64))
    tws["events"].copy_(torch.arange(Bt, dtype=torch.int32))
    before = dict(t=tws["t"].clone(), events=tws["events"].clone())
    plan_all = torch.arange(3.0 * P_ROWS, **f).reshape(P_ROWS, 3).contiguous()
    dplan_all = (-plan_all - 1).contiguous()
    r = ti._grid_norm(host(off))
    step = ops.unicycle_trigger_step_prepare(task, ws, tws, x, off, r, hyper, plan_all, dplan_all, DT_PLAN, t_end, tau_min, tau_max,
                                             L_true=L_TRUE, zeta=zeta)
    step()
    torch.cuda.synchronize()
    return dict(x=x, task=task, tws=tws, ws=ws, r=r, plan_all=plan_all, dplan_all=dplan_all, before=before, t_end=t_end, tau_min=tau_min,
                tau_max=tau_max, zeta=zeta)


def reference_events(st, run, hyper, off, dtype):
    """The numpy yardstick on what the device saw: the inputs as the working type holds them, the test points formed in it."""
    Bt = st["x"].shape[0]
    ws, task = run["ws"], st["task"]
    npdt = NP[dtype]
    raw = lambda v: v.detach().cpu().numpy()
    x0, offn = raw(st["x"]), raw(off)
    shared = hyper["ls"].shape[0] == 1 and Bt > 1
    out = []
    for b in range(Bt):
        hb = 0 if shared else b
        Xtest = (offn + x0[b]).astype(npdt).astype(np.float64)
        out.append(S.event(host(st["x"])[b], host(ws["y"])[b, :2], int(raw(ws["status"])[b]), host(ws["fhat"])[b], host(ws["ghat"])[b],
                           host(ws["Mk"])[b], host(task["centers"])[b], host(task["tw"]), offn, run["r"], host(hyper["ls"])[hb],
                           float(host(hyper["sf"])[hb]), host(hyper["Adiag"])[hb], host(hyper["B"])[hb], float(run["before"]["t"][b]),
                           int(run["before"]["events"][b]), host(run["plan_all"]), host(run["dplan_all"]), DT_PLAN, run["t_end"],
                           run["tau_min"], run["tau_max"], L_TRUE, zeta=run["zeta"], Xtest=Xtest))
    return out


def worst_rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. one event
SHAPES = [(Bt, Nte) for Bt in (1, 5, 67) for Nte in (1, 27, 65, 125, 729)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shared", [False, True], ids=["per-instance", "shared-model"])
@pytest.mark.parametrize("Bt,Nte", SHAPES, ids=["B%d-Nte%d" % s for s in SHAPES])
def test_one_event_against_the_existing_path_and_the_yardstick(Bt, Nte, shared, dtype):
    """uBu, xvel, Lh, Lkd, Lfh, tau of the fused event against trigger_interval_batch on the same state (its xtp1 formed over dt = 64,
    a power of two large enough that x + v dt - x loses nothing of v) and against the numpy yardstick, then the state after the step.
    Lkd, Lfh, tau: 1e-12 (fp64) / 1e-5 (fp32), the bounds of tests/test_gpu_trigger_interval.py.  The quantities the kernel adds and
    the new state: fp64 1e-12 against the yardstick; fp32 TOL32.  tau_min / tau_max are out of the way here: the raw tau is held."""
    from bayesian_cbf_amd import trigger_interval as ti
    from bayesian_cbf_amd.unicycle_move_to_pose import ObstacleCBF
    st = solved_state(dtype, Bt)
    hyper, off = hyper_and_points(dtype, Bt, Nte, shared, seed=100 * Bt + Nte)
    run = run_event(st, hyper, off, dtype)
    tws, ws, task = run["tws"], run["ws"], st["task"]
    got = {k: host(tws[k]) for k in ("uBu", "xvel", "Lh", "Lkd", "Lfh", "tau", "dt_used")}
    solved = host(ws["status"]) == 0                  # (an unsolved program's y is no control: only what happens to the state is held)
    for k, v in got.items():
        assert np.isfinite(v[solved]).all() and not (v == 7.0).any(), k
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    # the existing path
    u = ws["y"][:, :2].contiguous()
    ub = torch.cat([torch.ones(Bt, 1, dtype=dtype, device=DEV), u], dim=1)
    v = ws["fhat"] + torch.einsum("bdi,bi->bd", ws["ghat"], u) + torch.einsum("bdc,bc->bd", ws["Mk"], ub)
    sq = (lambda a: a[0]) if (shared and Bt > 1) else (lambda a: a)
    cbfs = [ObstacleCBF(task["centers"][:, k], task["radii"][:, k], tuple(float(w) for w in task["tw"])) for k in range(2)]
    batch = ti.trigger_interval_batch(st["x"], st["x"] + v * 64.0, u, sq(hyper["ls"]), sq(hyper["sf"]), sq(torch.diag_embed(hyper["Adiag"])),
                                      sq(hyper["B"]), cbfs, 64.0, off=off, r=run["r"])
    ref = reference_events(st, run, hyper, off, dtype)
    want = {k: np.array([e[k] for e in ref]) for k in ("uBu", "xvel", "Lh", "Lkd", "Lfh", "tau", "dt_used", "x", "t")}
    tag = "B%d Nte%d %s %s" % (Bt, Nte, "shared" if shared else "per-inst", "f64" if dtype == torch.float64 else "f32")
    for k in ("uBu", "xvel", "Lh", "Lkd", "Lfh", "tau"):
        print("MEASURED %s %s: worst relative error vs batch %.3e, vs yardstick %.3e" % (
            tag, k, worst_rel(got[k][solved], host(batch[k])[solved]), worst_rel(got[k][solved], want[k][solved])))
    xa = host(run["x"])
    print("MEASURED %s x: worst error / max(1, |x|) vs yardstick %.3e" % (tag, float(np.max(np.abs(xa - want["x"])) / max(1.0, np.abs(want["x"]).max()))))
    for k in ("Lkd", "Lfh", "tau"):
        all_close(got[k][solved], host(batch[k])[solved], rtol=tol, atol=1e-300, what="trigger step vs batch " + k)
        all_close(got[k][solved], want[k][solved], rtol=tol, atol=1e-300, what="trigger step vs yardstick " + k)
    if Nte == 1:
        assert (got["Lkd"] == 0).all()
    new_tol = dict.fromkeys(TOL32, FLOOR64) if dtype == torch.float64 else TOL32
    for k in ("uBu", "xvel", "Lh"):
        all_close(got[k][solved], want[k][solved], rtol=new_tol[k], atol=1e-300, what="trigger step vs yardstick " + k)
        # the batch path forms these three with torch in the working type: held at the bound of the outputs they feed
        all_close(got[k][solved], host(batch[k])[solved], rtol=tol, atol=1e-300, what="trigger step vs batch " + k)
    # the act: the clamp is out of the way, so a solved instance holds its control for tau itself; an unsolved one keeps its state
    assert np.array_equal(got["dt_used"][solved], got["tau"][solved]) and (got["dt_used"][~solved] == run["tau_max"]).all()
    assert xa[~solved].tobytes() == host(st["x"])[~solved].tobytes()
    np.testing.assert_allclose(xa[solved], want["x"][solved], rtol=0, atol=new_tol["x"] * max(1.0, np.abs(want["x"]).max()))
    np.testing.assert_allclose(host(tws["t"])[solved], want["t"][solved], rtol=tol, atol=0)
    assert (host(tws["t"])[~solved] == run["tau_max"]).all()
    assert np.array_equal(host(tws["events"]), np.arange(Bt) + 1)
    rows = np.array([S.plan_row(t, DT_PLAN, P_ROWS) for t in host(tws["t"])])
    assert np.array_equal(host(run["task"]["plan"]), host(run["plan_all"])[rows]) and np.array_equal(host(run["task"]["dot_plan"]), host(run["dplan_all"])[rows])


# ------------------------------------------------------------------------------------------------ 2. the clamp classes
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_clamp_classes_unsolved_last_step_and_finished(dtype):
    """tau_min and tau_max are put BETWEEN the yardstick's own taus, so that it yields instances clamped low, clamped high and interior
    (asserted on the yardstick, with a margin of 1e-3 to the nearest tau).  By class: low -> dt_used == tau_min, high -> tau_max,
    interior -> the raw tau itself, all exactly (as the working type holds them).  Two solved instances are made unsolved by
    rewriting the status buffer between the two launches: their state is kept bit for bit and tau_max passes.  One instance is 1e-4
    before t_end: it takes the remainder and its clock lands on t_end.  One is finished: nothing of it changes."""
    Bt, Nte = 13, 27
    st = solved_state(dtype, Bt)
    hyper, off = hyper_and_points(dtype, Bt, Nte, False, seed=7)
    T = lambda v: float(NP[dtype](v))
    probe = reference_events(st, run_event(st, hyper, off, dtype), hyper, off, dtype)
    ok = np.array([e is not None and host(st["ws"]["status"])[b] == 0 for b, e in enumerate(probe)])
    idx = np.flatnonzero(ok)
    assert len(idx) >= 8
    unsolved, last_b, done_b, cls = idx[:2], idx[2], idx[3], idx[4:]
    taus = np.sort(np.array([probe[b]["tau"] for b in cls]))
    assert len(taus) >= 3 and (taus > 0).all(), taus
    tau_min, tau_max = math.sqrt(taus[0] * taus[1]), math.sqrt(taus[-2] * taus[-1])     # the smallest is clamped low, the largest high
    t_end = 5.0
    t0 = np.zeros(Bt)
    t0[last_b], t0[done_b] = t_end - tau_min / 2, t_end
    status = st["ws"]["status"].clone()
    status[torch.as_tensor(unsolved, device=DEV)] = 2
    run = run_event(st, hyper, off, dtype, t0=t0, t_end=t_end, tau_min=tau_min, tau_max=tau_max, status=status)
    ref = reference_events(st, run, hyper, off, dtype)
    klass = {b: ("low" if ref[b]["tau"] < tau_min else "high" if ref[b]["tau"] > tau_max else "interior") for b in cls}
    assert {"low", "high", "interior"} <= set(klass.values()), klass
    for b in cls:
        assert min(abs(ref[b]["tau"] / tau_min - 1), abs(ref[b]["tau"] / tau_max - 1)) > 1e-3          # no instance sits on a clamp
    tws = run["tws"]
    dt_used, tau, t1, ev = host(tws["dt_used"]), host(tws["tau"]), host(tws["t"]), host(tws["events"])
    xa, xb = run["x"].cpu().numpy(), st["x"].cpu().numpy()
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    for b in cls:
        want = dict(low=T(tau_min), high=T(tau_max), interior=tau[b])[klass[b]]
        assert dt_used[b] == want, (b, klass[b], dt_used[b], want)
        assert abs(tau[b] - ref[b]["tau"]) <= tol * ref[b]["tau"]
        assert t1[b] == want and ev[b] == b + 1                                                          # from t = 0
        assert not np.array_equal(xa[b], xb[b])
    for b in unsolved:
        assert xa[b].tobytes() == xb[b].tobytes() and dt_used[b] == T(tau_max) and t1[b] == T(tau_max) and ev[b] == b + 1
        assert ref[b]["dt_used"] == tau_max and np.array_equal(ref[b]["x"], host(st["x"])[b])
    assert ref[last_b]["last"] and t1[last_b] == t_end and dt_used[last_b] == T(t_end - t0[last_b]) and ev[last_b] == last_b + 1
    assert host(run["task"]["plan"])[last_b].tolist() == host(run["plan_all"])[P_ROWS - 1].tolist()
    # the finished instance: state, clock, count, planner rows and every output row as they were
    assert ref[done_b] is None
    assert xa[done_b].tobytes() == xb[done_b].tobytes() and t1[done_b] == t_end and ev[done_b] == done_b
    assert (host(run["task"]["plan"])[done_b] == -5.0).all() and (host(run["task"]["dot_plan"])[done_b] == -6.0).all()
    for k in ("tau", "dt_used", "Lfh", "Lkd", "Lh", "xvel", "uBu"):
        assert (host(tws[k])[done_b] == 7.0).all(), k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_finished_instances_are_bit_identical_before_and_after(dtype):
    """t >= t_end (at it and past it), every second instance: x, t, events and plan do not change by a bit; the others do."""
    Bt = 5
    st = solved_state(dtype, Bt)
    hyper, off = hyper_and_points(dtype, Bt, 65, True, seed=3)
    t0 = np.array([2.0, 0.12, 2.5, 0.0, 2.0])
    run = run_event(st, hyper, off, dtype, t0=t0, t_end=2.0, tau_min=1e-4, tau_max=0.05)
    done = t0 >= 2.0
    x0, x1 = st["x"].cpu().numpy(), run["x"].cpu().numpy()
    assert x1[done].tobytes() == x0[done].tobytes()
    assert np.array_equal(host(run["tws"]["t"])[done], t0[done]) and np.array_equal(host(run["tws"]["events"])[done], np.arange(Bt)[done])
    assert (host(run["task"]["plan"])[done] == -5.0).all() and (host(run["task"]["dot_plan"])[done] == -6.0).all()
    rows = [S.plan_row(t, DT_PLAN, P_ROWS) for t in host(run["tws"]["t"])]
    assert rows[1] in (2, 3) and rows[3] in (0, 1)                         # 0.12 + dt_b, dt_b <= 0.05: past the second planner step
    assert np.array_equal(host(run["task"]["plan"])[~done], host(run["plan_all"])[rows][~done])
    assert (host(run["tws"]["t"])[~done] > t0[~done]).all() and np.array_equal(host(run["tws"]["events"])[~done], np.arange(Bt)[~done] + 1)
    assert not (host(run["task"]["plan"])[~done] == -5.0).any()


# ------------------------------------------------------------------------------------------------ 3. the loop
def _learned_gp(Bt):
    from bayesian_cbf_amd.control_affine_model import BatchedControlAffineGP
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(Bt, NTRAIN, 3, 2, dtype=torch.float64, device=DEV, seed=91)
    return BatchedControlAffineGP(p["X"], p["U"], 0.05 * p["Xdot"], 1e-2 * p["A"], 1e-2 * p["Bm"], p["ell"], p["s2"], p["M0"]).as_dict()


# two settings: on the learned model the clock crosses planner rows (horizon 0.12 = 2.4 planner steps); on the fixed-kernel model,
# whose taus over the first 0.008 s lie between 2.46e-4 and 3.0e-4, tau_min and tau_max sit inside that range (2 % away from the
# nearest instance), so all three clamp classes occur
LOOP = dict(horizon=0.12, dt=0.05, tau_min=4e-3, tau_max=0.05, max_events=40, zeta=1.0, Nte=28, L_mean=1.0, L_true=12.0, seed=4)
LOOPS = dict(learned=LOOP, fixed=dict(LOOP, horizon=0.008, tau_min=2.6e-4, tau_max=2.85e-4))
FIXED_HYPER = dict(ls=[0.5, 0.6, 0.7], sf=0.8, A=np.diag([1e-2, 2e-2, 3e-2]), B=np.eye(3) + 0.1)


@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_loop_event_by_event(model):
    """self_triggered_rollouts(Bt = 8, record = True, max_events = 40), fp64.  Every recorded event that an instance took is checked on
    its own from the recorded x_before: the planner rows it solved with against the planner at its clock; u against the oracle's
    control step (1e-6 of the control's scale, the project's fp64 bound, statuses agreeing unless the instance sits in the oracle's
    feasibility band; where the oracle's own solver breaks down -- status 'unknown', seen once in 240 events: a failed factorisation one
    iteration short of its tolerances -- there is no control to compare with, and at most max(2, 1 %) of the events may be such); tau against the numpy yardstick (1e-12); x_after against Euler (a few ulp); t the running sum of dt_used, the
    last step landing on the horizon; events stop there."""
    from bayesian_cbf_amd import rollouts, trigger_interval as ti
    from bayesian_cbf_amd.planner import PiecewiseLinearPlanner
    from oracle import control_step as ostep
    Bt, LOOP = 8, LOOPS[model]
    kw = dict(LOOP, gp=_learned_gp(Bt)) if model == "learned" else dict(LOOP, trigger_hyper=FIXED_HYPER)
    out = rollouts.self_triggered_rollouts(Bt, record=True, dtype=torch.float64, device=DEV, **kw)
    rec = {k: (v.cpu().numpy() if v.dtype in (torch.int32, torch.bool) else host(v)) for k, v in out["rec"].items()}
    task = {k: host(v) for k, v in out["task"].items()}
    horizon, E = LOOP["horizon"], LOOP["max_events"]
    if model == "learned":
        g = kw["gp"]
        hy = dict(ls=host(g["ell"]), sf=host(g["s2"]), Adiag=np.diagonal(host(g["A"]), axis1=-2, axis2=-1), B=host(g["Bm"]), A=host(g["A"]))
    else:
        one = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (Bt,) + np.shape(v))
        hy = dict(ls=one(FIXED_HYPER["ls"]), sf=one(FIXED_HYPER["sf"]), Adiag=one(np.diag(FIXED_HYPER["A"])), B=one(FIXED_HYPER["B"]),
                  A=one(np.diag([1e-2, 1e-2, 1e-2])))
    x0, xg = torch.tensor([-3.0, -1.0, -math.pi / 4], dtype=torch.float64), torch.tensor([0.0, 0.0, math.pi / 4], dtype=torch.float64)
    numSteps = 3
    planner = PiecewiseLinearPlanner(x0, xg, numSteps, LOOP["dt"], frac_time_to_reach_goal=0.95)
    plan_all = np.stack([planner.plan(s).numpy() for s in range(numSteps)])
    dplan_all = np.stack([planner.dot_plan(s).numpy() for s in range(numSteps)])
    off = ti.default_test_grid(3, LOOP["Nte"])
    r = R.whole_norm(off)
    assert off.shape == (27, 3)                       # floor(28^(1/3)) = 3 points per axis, as the reference counts them
    events, t_fin = out["events"].cpu().numpy(), host(out["t"])
    checked, no_verdict, classes = 0, 0, set()
    for b in range(Bt):
        t, n_ev = 0.0, 0
        for e in range(E):
            if not rec["active"][e, b]:
                assert t == horizon                                       # idle only once finished, and then for good
                assert not rec["active"][e:, b].any()
                break
            xb, u, status = rec["x_before"][e, b], rec["u"][e, b], int(rec["status"][e, b])
            row = S.plan_row(t, LOOP["dt"], numSteps)
            np.testing.assert_allclose(rec["plan"][e, b], plan_all[row], rtol=1e-14, atol=1e-15)
            np.testing.assert_allclose(rec["dot_plan"][e, b], dplan_all[row], rtol=1e-14, atol=1e-15)
            o = ostep.control_step(xb, rec["plan"][e, b], rec["dot_plan"][e, b], rec["Mk"][e, b], rec["Bk"][e, b], hy["A"][b], task["Kp"], 10.0,
                                   task["centers"][b], task["radii"][b], task["tw"], task["gammas"], LOOP["L_mean"], task["w"][b],
                                   task["r"][b], task["rho"][b], task["relax_mask"], dt=0.0)
            if o["status"] == "unknown":             # the ORACLE's solver broke down (iteration limit or a failed factorisation,
                no_verdict += 1                      # oracle/socp.py): it has no control to compare with; counted and bounded below
            elif (o["status"] == "optimal") != (status == 0):
                loose, tight = ostep.shifted_status(o, task["w"][b], task["r"][b], task["rho"][b], task["relax_mask"], 1e-6)
                assert (loose == "optimal") != (tight == "optimal"), (b, e, status, o["status"])
            elif status == 0:
                sol = o["sol"]["x"]
                assert np.abs(u - sol[:2]).max() <= 1e-6 * max(1.0, np.abs(sol).max()), (b, e, u, sol)
            th = xb[2]
            ghat = np.array([[math.cos(th), 0.0], [math.sin(th), 0.0], [0.0, 1.0 / LOOP["L_mean"]]])
            ev = S.event(xb, u, status, np.zeros(3), ghat, rec["Mk"][e, b], task["centers"][b], task["tw"], off, r, hy["ls"][b], float(hy["sf"][b]),
                         hy["Adiag"][b], hy["B"][b], t, n_ev, plan_all, dplan_all, LOOP["dt"], horizon, LOOP["tau_min"], LOOP["tau_max"],
                         LOOP["L_true"], zeta=LOOP["zeta"])
            if np.isfinite(ev["tau"]) and ev["tau"] != 0:
                assert abs(rec["tau"][e, b] - ev["tau"]) <= 1e-12 * abs(ev["tau"]), (b, e, rec["tau"][e, b], ev["tau"])
            else:
                assert rec["tau"][e, b] == ev["tau"] or (np.isnan(ev["tau"]) and np.isnan(rec["tau"][e, b]))
            near = min(abs(ev["tau"] / LOOP["tau_min"] - 1), abs(ev["tau"] / LOOP["tau_max"] - 1)) if np.isfinite(ev["tau"]) else 1.0
            dtu = rec["dt_used"][e, b]
            if status == 0 and not ev["last"]:
                classes.add("low" if ev["dt_used"] == LOOP["tau_min"] else "high" if ev["dt_used"] == LOOP["tau_max"] else "interior")
            if near > 1e-9 and not ev["last"]:                             # (on a clamp to rounding either side is right)
                assert dtu == (ev["dt_used"] if ev["dt_used"] in (LOOP["tau_min"], LOOP["tau_max"]) else rec["tau"][e, b]), (b, e)
            if near > 1e-9 and ev["last"]:
                assert dtu == horizon - t, (b, e)
            euler = xb + (np.array([math.cos(th) * u[0], math.sin(th) * u[0], u[1] / LOOP["L_true"]]) * dtu if status == 0 else 0.0)
            np.testing.assert_allclose(rec["x_after"][e, b], euler, rtol=0, atol=4 * np.finfo(np.float64).eps * max(1.0, np.abs(xb).max()))
            if status != 0:
                assert np.array_equal(rec["x_after"][e, b], xb)
            t_next = t + dtu
            if rec["t"][e, b] == horizon and abs(t_next - horizon) <= 4 * np.finfo(np.float64).eps * horizon:
                t_next = horizon                                          # the last, partial step lands on the horizon itself
            assert rec["t"][e, b] == t_next, (b, e, rec["t"][e, b], t_next)
            t, n_ev, checked = t_next, n_ev + 1, checked + 1
            if e + 1 < E:
                np.testing.assert_array_equal(rec["x_before"][e + 1, b], rec["x_after"][e, b])
        assert events[b] == n_ev and t_fin[b] == t
    assert checked >= Bt * 3 and no_verdict <= max(2, checked // 100), (checked, no_verdict)
    if model == "fixed":
        assert classes == {"low", "interior", "high"}, classes
    # at most ceil(horizon / tau_min) <= 31 events: every instance is done within the 40 and has idled since
    assert out["done"] == 1.0 and (t_fin == horizon).all()
    assert (events <= math.ceil(horizon / LOOP["tau_min"])).all() and (events >= math.floor(horizon / LOOP["tau_max"])).all()
    assert out["dt_used"]["min"] >= 0 and out["dt_used"]["max"] <= LOOP["tau_max"]
    np.testing.assert_allclose(host(out["events_per_second"]), events / horizon, rtol=1e-15)
    assert out["stats"]["count"] == Bt and np.isfinite(out["stats"]["mean_cost"])


@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_loop_eager_and_graph_agree(model):
    from bayesian_cbf_amd import rollouts
    Bt, LOOP = 8, LOOPS[model]
    kw = dict(LOOP, gp=_learned_gp(Bt)) if model == "learned" else dict(LOOP, trigger_hyper=FIXED_HYPER)
    a = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, **kw)
    b = rollouts.self_triggered_rollouts(Bt, dtype=torch.float64, device=DEV, use_graph=True, **kw)
    for k in ("x_final", "t", "events", "min_h"):
        assert torch.equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["dt_used"] == b["dt_used"] and a["done"] == b["done"] == 1.0


# ------------------------------------------------------------------------------------------------ 4. the periodic loop
def test_periodic_loop_is_untouched():
    """monte_carlo_safety_rollouts(Bt = 64, seed = 0) before and after the new code has run in the same process: the same x_final, bit
    for bit (the new entry shares no state with it)."""
    from bayesian_cbf_amd import rollouts
    before = rollouts.monte_carlo_safety_rollouts(64, numSteps=20, seed=0, device=DEV)["x_final"].clone()
    rollouts.self_triggered_rollouts(8, dtype=torch.float64, device=DEV, **dict(LOOP, trigger_hyper=FIXED_HYPER, max_events=5))
    after = rollouts.monte_carlo_safety_rollouts(64, numSteps=20, seed=0, device=DEV)["x_final"]
    assert torch.equal(before, after)
