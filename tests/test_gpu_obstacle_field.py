"""The obstacle-field working set on the device (bayesian_cbf_amd/csrc/obstacle_field.hip) against the numpy yardstick
(tests/_obstacle_field_reference.py): select and audit at every lap shape of the lane stride, one step against the device's own
composed path with every disc, and the closed loop -- certificate recomputed in numpy, objectives against the oracle's full
program, graph replay and a permuted batch bit for bit."""
import math

import numpy as np
import pytest
import torch

import _obstacle_field_reference as R

pytestmark = pytest.mark.gpu

BTS, KFS, SS = (1, 5, 67), (3, 4, 63, 64, 65, 130, 256), (1, 2, 3)
MARGIN = {torch.float64: 1e-9, torch.float32: 1e-4}      # decisions closer than this are not compared
MAX_EXCLUDED = 0.05
DEV = "cuda"
TW = (0.7, 0.3)
# instances of the closed loop whose every step is also solved with all 16 cones by the oracle (chosen before any run)
ORACLE_INSTANCES = (0, 13, 26, 39, 52, 65)
MAX_NOT_COMPARED, MAX_UNCERTIFIED = 0.15, 0.10


@pytest.fixture(scope="module")
def ops():
    from bayesian_cbf_amd import ops
    return ops


def _np(t):
    return t.detach().double().cpu().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def _field(Bt, Kf, shared, dtype, seed):
    """A field of the sampler's discs around states near the start; instance 0 sees duplicate discs, instance 1 a NaN radius."""
    rng = np.random.RandomState(seed)
    Bf = 1 if shared else Bt
    cen = np.stack([R.random_obstacle_field(Kf, seed=seed + 7 * b)[0] for b in range(Bf)])
    rad = np.stack([R.random_obstacle_field(Kf, seed=seed + 7 * b)[1] for b in range(Bf)])
    if Kf >= 4 and (Bt == 1 or not shared):
        o = np.argsort(R.rows(R.START, cen[0], rad[0], TW)[1])          # copies of the nearest discs, at other lanes and laps:
        cen[0, Kf - 1], rad[0, Kf - 1] = cen[0, o[0]], rad[0, o[0]]     # bit-equal h, the tie rule decides
        cen[0, Kf // 2], rad[0, Kf // 2] = cen[0, o[1]], rad[0, o[1]]
        if Bt > 1:
            rad[1, Kf - 2] = np.nan
    x = R.START[None] + rng.randn(Bt, 3) * np.array([0.4, 0.4, 1.0])
    f = dict(dtype=dtype, device=DEV)
    return torch.tensor(x, **f), dict(centers=torch.tensor(cen, **f), radii=torch.tensor(rad, **f))


def _field_of(field, b):
    cen, rad = _np(field["centers"]), _np(field["radii"])
    return (cen[0], rad[0]) if cen.shape[0] == 1 else (cen[b], rad[b])


# ---------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-instance"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_select_equals_the_yardstick(ops, dtype, shared):
    eps = torch.finfo(dtype).eps
    tw = torch.tensor(TW, dtype=dtype, device=DEV)
    twn = _np(tw)
    total = left = 0
    for Bt in BTS:
        for Kf in KFS:
            x, field = _field(Bt, Kf, shared, dtype, seed=Kf)
            for S in SS:
                fws = ops.obstacle_field_workspace(Bt, S, dtype, DEV)
                fws["cert"].fill_(7); fws["rounds"].fill_(7)
                fws["min_h"][::2] = -100.0                                   # in place: an earlier minimum survives
                ops.obstacle_field_select(x, field, tw, fws)
                idx, mh = _np(fws["idx"]), _np(fws["min_h"])
                assert not fws["cert"].any() and not fws["rounds"].any()
                xn = _np(x)
                for b in range(Bt):
                    cen, rad = _field_of(field, b)
                    ref = R.select(xn[b], cen, rad, twn, S)
                    total += 1
                    if ref["margin"] > MARGIN[dtype] or ref["exact_tie"]:
                        assert idx[b].tolist() == ref["idx"].tolist(), (Bt, Kf, S, b, idx[b], ref["idx"])
                    else:
                        left += 1
                        assert len(set(idx[b].tolist())) == S and idx[b].min() >= 0 and idx[b].max() < Kf
                    assert np.array_equal(_np(fws["centers_sel"])[b], cen[idx[b]])
                    assert np.array_equal(_np(fws["radii_sel"])[b], rad[idx[b]], equal_nan=True)
                    want = min(ref["min_h"], -100.0) if b % 2 == 0 else ref["min_h"]
                    if np.isfinite(want):
                        gh = xn[b, :2] - cen
                        mag = np.nanmax(twn[0] * ((gh ** 2).sum(1) + rad ** 2) + twn[1])
                        assert abs(mh[b] - want) <= 64 * eps * mag, (Bt, Kf, S, b, mh[b], want)
                    else:
                        assert mh[b] == want
    print("select %s: %d of %d decisions left out" % (dtype, left, total))
    assert left <= MAX_EXCLUDED * total, (left, total)


# ---------------------------------------------------------------------------------------------- audit
def _audit_inputs(ops, Bt, Kf, S, shared, dtype, seed):
    x, field = _field(Bt, Kf, shared, dtype, seed)
    rng = np.random.RandomState(1000 + seed)
    f = dict(dtype=dtype, device=DEV)
    tw = torch.tensor(TW, **f)
    fws = ops.obstacle_field_workspace(Bt, S, dtype, DEV)
    ops.obstacle_field_select(x, field, tw, fws)
    ws = ops.control_workspace(Bt, S, dtype, DEV)
    Bq = rng.randn(Bt, 3, 3)
    ws["y"].copy_(torch.tensor(rng.randn(Bt, 3) * np.array([1.5, 1.5, 1.0]) * (rng.rand(Bt, 1) < 0.8), **f))   # some u = 0
    ws["status"].copy_(torch.tensor((rng.rand(Bt) < 0.15) * rng.randint(1, 4, Bt), dtype=torch.int32))
    ws["Mk"].copy_(torch.tensor(0.05 * rng.randn(Bt, 3, 3), **f))
    ws["Bk"].copy_(torch.tensor(Bq @ Bq.transpose(0, 2, 1) / 3 + 0.05 * np.eye(3), **f))
    ws["fhat"].copy_(torch.tensor(0.01 * rng.randn(Bt, 3), **f))
    th = _np(x)[:, 2]
    gh = np.zeros((Bt, 3, 2)); gh[:, 0, 0] = np.cos(th); gh[:, 1, 0] = np.sin(th); gh[:, 2, 1] = 1.0
    ws["ghat"].copy_(torch.tensor(gh, **f))
    A = torch.tensor(np.eye(3)[None] * (0.002 + 0.02 * rng.rand(Bt, 1, 1)), **f)
    rho = torch.tensor(2.0 + rng.rand(Bt), **f)
    fws["cert"].copy_(torch.tensor((rng.rand(Bt) < 0.15) * rng.randint(1, 4, Bt), dtype=torch.int32))        # decided earlier
    return x, field, tw, ws, A, rho, fws


@pytest.mark.parametrize("tols", [None, (1e-7, 1e6), (1e6, 1e-6)], ids=["default", "all-active", "all-feasible"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-instance"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_audit_equals_the_yardstick(ops, dtype, shared, tols):
    eps = torch.finfo(dtype).eps
    tol_f, tol_a = tols if tols is not None else ops.FIELD_TOLERANCES[dtype]
    gamma = 5.0
    total = left = swaps = certs = fulls = 0
    worst_rel = 0.0
    shapes = [(Bt, Kf, S) for Bt in BTS for Kf in KFS for S in SS] if tols is None else \
        [(67, Kf, S) for Kf in (4, 65, 256) for S in (1, 3)]
    for Bt, Kf, S in shapes:
        x, field, tw, ws, A, rho, fws = _audit_inputs(ops, Bt, Kf, S, shared, dtype, seed=Kf + S)
        before = {k: _np(v).copy() for k, v in fws.items()}
        for k in ("worst_margin", "worst_idx", "nviol"):
            fws[k].fill_(-77)
        ops.obstacle_field_audit(x, ws, A, rho, field, tw, gamma, fws, *(tols or (None, None)))
        after = {k: _np(v) for k, v in fws.items()}
        h = {k: _np(v) for k, v in ws.items()}
        xn, An, rhon, twn = _np(x), _np(A), _np(rho), _np(tw)
        for b in range(Bt):
            cen, rad = _field_of(field, b)
            m, E, rs, scale = R.margins(xn[b], h["y"][b, :2], h["Mk"][b], h["Bk"][b], An[b], h["fhat"][b], h["ghat"][b], rhon[b],
                                        cen, rad, twn, gamma)
            ref = R.audit(int(before["cert"][b]), int(h["status"][b]), before["idx"][b], m, scale, tol_f, tol_a)
            if before["cert"][b] != 0:                                        # idempotent: nothing is touched
                assert after["cert"][b] == before["cert"][b] and after["rounds"][b] == 0 and after["nviol"][b] == -77
                assert after["worst_idx"][b] == -77 and after["worst_margin"][b] == -77
                assert np.array_equal(after["idx"][b], before["idx"][b])
                assert np.array_equal(after["centers_sel"][b], before["centers_sel"][b])
                continue
            if h["status"][b] != 0:
                assert after["cert"][b] == ops.FIELD_UNSOLVED and after["worst_idx"][b] == -1 and after["nviol"][b] == 0
                assert np.isnan(after["worst_margin"][b]) and np.array_equal(after["idx"][b], before["idx"][b])
                continue
            total += 1
            # the reported margin against the float64 formula on the same stored inputs, at the disc the device names
            wi = int(after["worst_idx"][b])
            if Kf == S:
                assert wi == -1 and after["worst_margin"][b] == np.inf
            else:
                assert 0 <= wi < Kf and wi not in before["idx"][b].tolist()
                if np.isfinite(m[wi]):
                    mag = R.margin_magnitude(xn[b], h["y"][b, :2], h["Mk"][b], h["Bk"][b], An[b], h["fhat"][b], h["ghat"][b],
                                             rhon[b], cen, rad, twn, gamma)[wi]
                    rel = abs(after["worst_margin"][b] - m[wi]) / mag
                    worst_rel = max(worst_rel, rel)
                    assert rel <= 64 * eps, (Bt, Kf, S, b, after["worst_margin"][b], m[wi])
                else:
                    assert after["worst_margin"][b] == m[wi]
            if not ref["decision"] > MARGIN[dtype]:
                left += 1
                continue
            assert after["cert"][b] == ref["cert"], (Bt, Kf, S, b, after["cert"][b], ref["cert"], ref["decision"])
            assert after["nviol"][b] == ref["nviol"] and wi == ref["worst_idx"]
            assert np.array_equal(after["idx"][b], ref["idx"]), (Bt, Kf, S, b, after["idx"][b], ref["idx"])
            assert after["rounds"][b] == ref["rounds_inc"]
            assert np.array_equal(after["centers_sel"][b], cen[ref["idx"]])
            assert np.array_equal(after["radii_sel"][b], rad[ref["idx"]], equal_nan=True)
            swaps += ref["swapped"] >= 0
            certs += ref["cert"] == R.CERTIFIED
            fulls += ref["cert"] == R.FULL
    print("audit %s tols=%s: %d audited, %d left out, %d swaps, %d certified, %d full; worst |margin - float64 margin| / "
          "magnitudes summed = %.3e" % (dtype, tols, total, left, swaps, certs, fulls, worst_rel))
    assert left <= MAX_EXCLUDED * total, (left, total)
    if tols is None:
        assert swaps >= 10 and certs >= 10                                    # both branches were taken
    elif tols[1] > 1:
        assert fulls >= 20 and swaps == 0
    else:
        assert certs == total


# ---------------------------------------------------------------------------------------------- the loop
def _gp(Bt, N, dtype, seed):
    """A small learned model per instance: make_instances' data with a residual a tenth as large and A near 0.01 I."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(Bt, N, 3, 2, dtype=dtype, device=DEV, seed=seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    p["A"] = (torch.eye(3, dtype=dtype, device=DEV)[None] * (0.01 + 0.005 * torch.rand(Bt, 1, 1, generator=g, dtype=dtype, device=DEV))).contiguous()
    p["Xdot"] = (0.1 * p["Xdot"]).contiguous()
    p["Bm"] = (0.05 * p["Bm"]).contiguous()
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    return dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=p["A"])


def _loop(ops, model, dtype=torch.float64, Bt=67, Kf=16, steps=40, graph=False, perm=None, field_seed=2, S=3, rounds=3):
    """The closed loop of the GPU tests, driven step by step so that every step's inputs and outputs are recorded.  Field seed 2:
    of the seeds 0..23 one of the two (with 18) on which the numpy loop from the unperturbed start swaps a disc in within 40 steps."""
    from bayesian_cbf_amd.rollouts import random_obstacle_field, unicycle_task_tensors
    from bayesian_cbf_amd.planner import PiecewiseLinearPlanner
    f = dict(dtype=dtype, device=DEV)
    x0, xg = torch.tensor(R.START, **f), torch.tensor(R.GOAL, **f)
    task = unicycle_task_tensors(Bt, x0, xg, dtype, DEV, cbf_gammas=(5.0,) * S)
    task["sign"] = torch.tensor([-1.0] + [1.0] * S, **f)
    task["relax_mask"] = torch.tensor([1.0] + [0.0] * S, **f)
    fld = random_obstacle_field(Kf, seed=field_seed, dtype=dtype, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = (x0 + 0.05 * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    ws = ops.control_workspace(Bt, S, dtype, DEV)
    if model == "fixed":
        ws["Mk"].zero_(); ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        gp = dict(A=(0.01 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous())
    else:
        gp = _gp(Bt, 40, dtype, seed=11)
    if perm is not None:
        x = x[perm].contiguous()
        gp = {k: v[perm].contiguous() for k, v in gp.items()}
    planner = PiecewiseLinearPlanner(x0, xg, 120, 0.05, frac_time_to_reach_goal=0.95)
    plan_all = torch.stack([planner.plan(t).to(dtype=dtype) for t in range(steps)]).to(DEV)
    dplan_all = torch.stack([planner.dot_plan(t).to(dtype=dtype) for t in range(steps)]).to(DEV)
    task["plan"], task["dot_plan"] = torch.empty(Bt, 3, **f), torch.empty(Bt, 3, **f)
    step = ops.unicycle_field_control_step_prepare(gp, task, fld, ws, x, rounds=rounds, dt=0.05, L_true=12.0, L_mean=1.0, max_iters=30)
    fws = step.fws
    tctr = torch.zeros(1, dtype=torch.long, device=DEV)

    def one():
        task["plan"].copy_(plan_all.index_select(0, tctr))
        task["dot_plan"].copy_(dplan_all.index_select(0, tctr))
        step()
        tctr.add_(1)

    g = None
    if graph:
        state = [x, fws["min_h"], fws["cost"], fws["fails"], tctr]
        saved = [v.clone() for v in state]
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            one()
        side.synchronize()
        for d, s in zip(state, saved):
            d.copy_(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            one()
        for d, s in zip(state, saved):
            d.copy_(s)
        torch.cuda.synchronize()
    rec = []
    for t in range(steps):
        xb = x.clone()
        g.replay() if g is not None else one()
        rec.append(dict(x=_np(xb), xn=_np(x), y=_np(ws["y"]), status=_np(ws["status"]), cert=_np(fws["cert"]),
                        rounds=_np(fws["rounds"]), eff=_np(fws["status_eff"]), idx=_np(fws["idx"]), Mk=_np(ws["Mk"]),
                        Bk=_np(ws["Bk"]), plan=_np(plan_all[t]), dplan=_np(dplan_all[t])))
    out = dict(rec=rec, x=x.clone(), min_h=fws["min_h"].clone(), cost=fws["cost"].clone(), fails=fws["fails"].clone(),
               A=_np(gp["A"]), cen=_np(fld["centers"]), rad=_np(fld["radii"]), rho=float(task["rho"][0]))
    return out


@pytest.fixture(scope="module")
def loops(ops):
    return {m: _loop(ops, m) for m in ("fixed", "learned")}


@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_closed_loop_certificate_holds_in_numpy_and_objectives_equal_the_oracles(ops, loops, model):
    from oracle import unicycle as ouni
    L = loops[model]
    c = R.task_constants()
    assert abs(c["rho"] - L["rho"]) < 1e-12
    cen, rad = L["cen"], L["rad"]
    n = certified = frozen = asked = compared = 0
    hist = np.zeros(3, dtype=int)
    worst_feas = worst_obj = worst_active = 0.0
    for s in L["rec"]:
        for b in range(67):
            n += 1
            x = s["x"][b]
            if s["eff"][b] != 0:                                     # uncertified and unsolved instances keep their state
                frozen += 1
                assert s["cert"][b] != R.CERTIFIED and np.array_equal(s["xn"][b], x)
                assert s["eff"][b] == (s["status"][b] if s["status"][b] != 0 else R.UNCERTIFIED)
                continue
            certified += 1
            hist[s["rounds"][b]] += 1
            assert s["cert"][b] == R.CERTIFIED and s["status"][b] == 0
            fhat, ghat = ouni.ackermann_f(x), ouni.ackermann_g(x, 1.0)
            m, E, rs, scale = R.margins(x, s["y"][b, :2], s["Mk"][b], s["Bk"][b], L["A"][b], fhat, ghat, c["rho"], cen, rad, c["tw"], c["gamma"])
            worst_feas = max(worst_feas, float((-m / scale).max()))
            worst_active = max(worst_active, float(np.abs(m[s["idx"][b]] / scale[s["idx"][b]]).min()))
            assert (m >= -R.TOL_F * scale).all(), (b, m.min())       # all 16 cones, recomputed from the recorded inputs
            want = ouni.ackermann_step(x, s["y"][b, :2], 0.05, 12.0)
            assert np.abs(s["xn"][b] - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
            if b in ORACLE_INSTANCES:
                asked += 1
                o = R.full_step(x, s["plan"], s["dplan"], s["Mk"][b], s["Bk"][b], L["A"][b], c, cen, rad)
                if o["status"] != "optimal":
                    continue
                compared += 1
                fo = R.objective(np.concatenate([o["u"], [o["relax"]]]), c["w"])
                fw = R.objective(s["y"][b], c["w"])
                worst_obj = max(worst_obj, abs(fo - fw) / max(1.0, abs(fo)))
                assert abs(fo - fw) <= R.EPS_G * max(1.0, abs(fo)), (b, fo, fw)
    print("%s: %d instance-steps, %d certified (after 0/1/2 swaps: %s), %d kept their state; worst infeasibility %.2e, "
          "tightest slot |margin| / scale up to %.2e; oracle: %d of %d compared, worst objective gap %.2e"
          % (model, n, certified, hist.tolist(), frozen, worst_feas, worst_active, compared, asked, worst_obj))
    assert n - certified <= MAX_UNCERTIFIED * n, (certified, n)
    assert asked - compared <= MAX_NOT_COMPARED * asked and compared >= 100, (asked, compared)
    if model == "fixed":
        assert hist[1:].sum() > 0                                   # the swap path ran (the numpy loop swaps on this field too)


@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_graph_replay_equals_eager_bit_for_bit(ops, loops, model):
    G, E = _loop(ops, model, graph=True), loops[model]
    for k in ("x", "min_h", "cost", "fails"):
        assert torch.equal(G[k], E[k]), k
    for a, b in zip(G["rec"], E["rec"]):
        for k in ("xn", "y", "cert", "rounds", "eff", "idx"):
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


@pytest.mark.parametrize("model", ["fixed", "learned"])
def test_permuted_batch_is_bit_identical(ops, loops, model):
    perm = torch.randperm(67, generator=torch.Generator().manual_seed(5)).to(DEV)
    P, E = _loop(ops, model, perm=perm), loops[model]
    p = perm.cpu().numpy()
    assert torch.equal(P["x"], E["x"][perm]) and torch.equal(P["min_h"], E["min_h"][perm])
    for a, b in zip(P["rec"], E["rec"]):
        for k in ("xn", "cert", "rounds"):
            assert np.array_equal(a[k], b[k][p]), k


def test_f32_loop_certifies_at_its_measured_tolerances(ops):
    """The fp32 entries: rows formed in fp32 by the solver, audited in fp64 from the same stored inputs."""
    from oracle import unicycle as ouni
    L = _loop(ops, "fixed", dtype=torch.float32)
    c = R.task_constants()
    tol_f, _ = ops.FIELD_TOLERANCES[torch.float32]
    n = certified = 0
    worst_active = worst_feas = 0.0
    for s in L["rec"]:
        for b in range(67):
            n += 1
            if s["eff"][b] != 0:
                assert np.array_equal(s["xn"][b], s["x"][b])
                continue
            certified += 1
            x = s["x"][b]
            m, E, rs, scale = R.margins(x, s["y"][b, :2], s["Mk"][b], s["Bk"][b], L["A"][b], ouni.ackermann_f(x),
                                        ouni.ackermann_g(x, 1.0), np.float64(np.float32(c["rho"])), L["cen"], L["rad"],
                                        np.float32(c["tw"]).astype(np.float64), c["gamma"])
            un = np.setdiff1d(np.arange(16), s["idx"][b])
            worst_feas = max(worst_feas, float((-m[un] / scale[un]).max()))
            worst_active = max(worst_active, float((-m[s["idx"][b]] / scale[s["idx"][b]]).max()))
            assert (m[un] >= -tol_f * scale[un]).all()
    print("f32: %d of %d certified; unselected infeasibility %.2e; the working set's own cones as the fp64 audit sees them: "
          "down to %.2e below zero (relative)" % (certified, n, worst_feas, worst_active))
    assert n - certified <= MAX_UNCERTIFIED * n


def test_instances_that_are_not_certified_keep_their_state(ops):
    """One slot and one round among nearby discs: whoever needs a second cone stays uncertified and must not move."""
    from bayesian_cbf_amd.rollouts import random_obstacle_field, unicycle_task_tensors
    Bt, dtype = 67, torch.float64
    f = dict(dtype=dtype, device=DEV)
    x0, xg = torch.tensor(R.START, **f), torch.tensor(R.GOAL, **f)
    fld = random_obstacle_field(16, seed=31, dtype=dtype, device=DEV, box=((-3.6, -1.4), (-2.1, 0.3)), clear_start=0.35)
    gen = torch.Generator(device=DEV).manual_seed(12)
    x = (x0 + torch.tensor([0.4, 0.4, 1.0], **f) * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    task = unicycle_task_tensors(Bt, x0, xg, dtype, DEV, cbf_gammas=(5.0,))
    task.update(sign=torch.tensor([-1.0, 1.0], **f), relax_mask=torch.tensor([1.0, 0.0], **f),
                plan=(x0 + 0.15 * (xg - x0)).expand(Bt, 3).contiguous(), dot_plan=((xg - x0) / 5.0).expand(Bt, 3).contiguous())
    ws = ops.control_workspace(Bt, 1, dtype, DEV)
    ws["Mk"].zero_(); ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
    step = ops.unicycle_field_control_step_prepare(dict(A=(0.01 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous()), task, fld, ws, x,
                                                   rounds=1, dt=0.05, L_true=12.0, max_iters=100)
    before = x.clone()
    step()
    torch.cuda.synchronize()
    fws = step.fws
    eff, cert, status = _np(fws["status_eff"]), _np(fws["cert"]), _np(ws["status"])
    moved = (x != before).any(1).cpu().numpy()
    print("one slot, one round: cert histogram %s, status_eff values %s" % (np.bincount(cert, minlength=4).tolist(), sorted(set(eff.tolist()))))
    assert (moved == (eff == 0)).all()
    assert ((eff == 0) == (cert == R.CERTIFIED)).all()
    assert (eff[(cert != R.CERTIFIED) & (status == 0)] == R.UNCERTIFIED).all()
    assert (eff[status != 0] == status[status != 0]).all() and (cert[status != 0] == R.UNSOLVED).all()
    assert (cert == 0).sum() >= 1 and (cert == R.CERTIFIED).sum() >= 1
    assert _np(fws["fails"]).tolist() == (eff != 0).astype(int).tolist()


# ---------------------------------------------------------------------------------------------- against the composed path
@pytest.mark.parametrize("Kf", [4, 7])
def test_one_step_equals_the_composed_path_with_every_disc(ops, Kf):
    from bayesian_cbf_amd.rollouts import random_obstacle_field, unicycle_task_tensors
    from oracle import unicycle as ouni
    Bt, dtype = 67, torch.float64
    f = dict(dtype=dtype, device=DEV)
    x0, xg = torch.tensor(R.START, **f), torch.tensor(R.GOAL, **f)
    fld = random_obstacle_field(Kf, seed=20 + Kf, dtype=dtype, device=DEV, box=((-3.4, -1.6), (-1.9, 0.1)))   # discs near the start
    gen = torch.Generator(device=DEV).manual_seed(8)
    x = (x0 + torch.tensor([0.3, 0.3, 0.8], **f) * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    plan = (x0 + 0.15 * (xg - x0)).expand(Bt, 3).contiguous()
    dplan = ((xg - x0) / 5.0).expand(Bt, 3).contiguous()
    A = (0.01 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous()

    def task_for(K, centers, radii):
        t = unicycle_task_tensors(Bt, x0, xg, dtype, DEV, cbf_gammas=(5.0,) * K)
        t.update(sign=torch.tensor([-1.0] + [1.0] * K, **f), relax_mask=torch.tensor([1.0] + [0.0] * K, **f), plan=plan,
                 dot_plan=dplan, centers=centers, radii=radii)
        return t

    def fixed_ws(K):
        ws = ops.control_workspace(Bt, K, dtype, DEV)
        ws["Mk"].zero_(); ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        return ws
    # the composed path: every disc in one program
    wsc, xc = fixed_ws(Kf), x.clone()
    ops.unicycle_control_step(dict(A=A), task_for(Kf, fld["centers"].expand(Bt, Kf, 2).contiguous(), fld["radii"].expand(Bt, Kf).contiguous()),
                              wsc, xc, dt=0.0, max_iters=100)
    # the working set
    wsf, xf = fixed_ws(3), x.clone()
    step = ops.unicycle_field_control_step_prepare(dict(A=A), task_for(3, None, None), fld, wsf, xf, rounds=3, dt=0.0, max_iters=100)
    step()
    torch.cuda.synchronize()
    assert torch.equal(xf, x)                                               # dt = 0: nobody moves
    yc, stc, yf, cert = _np(wsc["y"]), _np(wsc["status"]), _np(wsf["y"]), _np(step.fws["cert"])
    c = R.task_constants()
    cen, rad, xn = _np(fld["centers"]), _np(fld["radii"]), _np(x)
    compared = 0
    worst_obj = worst_feas = 0.0
    for b in range(Bt):
        if cert[b] != R.CERTIFIED or stc[b] != 0:
            continue
        compared += 1
        fc, fw = R.objective(yc[b], c["w"]), R.objective(yf[b], c["w"])
        worst_obj = max(worst_obj, abs(fc - fw) / max(1.0, abs(fc)))
        assert abs(fc - fw) <= R.EPS_G * max(1.0, abs(fc)), (b, fc, fw)
        m, E, rs, scale = R.margins(xn[b], yf[b, :2], np.zeros((3, 3)), np.eye(3), 0.01 * np.eye(3), ouni.ackermann_f(xn[b]),
                                    ouni.ackermann_g(xn[b], 1.0), c["rho"], cen, rad, c["tw"], c["gamma"])
        worst_feas = max(worst_feas, float((-m / scale).max()))
        assert (m >= -R.EPS_F * scale).all(), (b, (m / scale).min())
    print("Kf=%d: %d of %d compared with the composed path; worst objective gap %.2e, worst infeasibility %.2e; cert histogram %s"
          % (Kf, compared, Bt, worst_obj, worst_feas, np.bincount(cert, minlength=4).tolist()))
    assert compared >= Bt // 2
