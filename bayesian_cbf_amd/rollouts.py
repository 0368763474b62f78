"""Monte-Carlo safety rollouts (BASELINE config 4) and online-GP growth (config 5) drivers.

Batched counterpart of the reference's `unicycle_bayes_cbf_safe_obstacle` recipe
(unicycle_move_to_pose.py:1887-1928: fixed-kernel Ackermann model, CLFCartesian Kp=[.9,1.5,0],
two obstacles at mid path with weights [.7,.3], gamma 5, max_risk 0.01) run as Bt independent
closed loops from perturbed start states: `sample_generator_trajectory` (sampling.py:68-74) for
every trajectory at once, sharded over GPUs by `distributed.shard_range`, statistics reduced once
at the end."""
import math
import os
import time
from types import SimpleNamespace as types_ns

import torch

from . import ops
from .cbc2 import cbc1_safety_factor
from .distributed import reduce_cbc2_risk_stats, reduce_risk_stats, reduce_rollout_stats
from .planner import PiecewiseLinearPlanner


def unicycle_task_tensors(Bt, x0, xg, dtype, device, term_weights=(0.7, 0.3), cbf_gammas=(5.0, 5.0),
                          Kp=(0.9, 1.5, 0.0), cost_weights=(0.33, 0.33, 0.33), max_risk=0.01):
    f = dict(dtype=dtype, device=device)
    x0, xg = x0.to(**f), xg.to(**f)
    R90 = torch.tensor([[0.0, -1.0], [1.0, 0.0]], **f)
    d = x0[:2] - xg[:2]
    mid = (x0[:2] + xg[:2]) / 2
    centers = torch.stack([mid + R90 @ d / 3, mid - R90 @ d / 3]).expand(Bt, 2, 2).contiguous()
    radii = (d.norm() / 4).expand(Bt, 2).contiguous()
    rho = 0.0 if max_risk == 0.5 else cbc1_safety_factor(max_risk)
    return dict(centers=centers, radii=radii, Kp=torch.tensor(Kp, **f), tw=torch.tensor(term_weights, **f),
                gammas=torch.tensor(cbf_gammas, **f), sign=torch.tensor([-1.0, 1.0, 1.0], **f),
                relax_mask=torch.tensor([1.0, 0.0, 0.0], **f), w=torch.tensor(cost_weights, **f).expand(Bt, 3).contiguous(),
                r=torch.zeros(Bt, 2, **f), rho=torch.full((Bt,), rho, **f))


def monte_carlo_safety_rollouts(Bt, numSteps=200, dt=0.05, gp=None, kernel_diag_A=(1e-2, 1e-2, 1e-2),
                                L_mean=1.0, L_true=12.0, start=(-3.0, -1.0, -math.pi / 4), goal=(0.0, 0.0, math.pi / 4),
                                start_noise=0.05, max_risk=0.01, dtype=torch.float64, device="cuda", seed=0,
                                record=False, max_iters=30, use_graph=False, plant="true"):
    """Run Bt closed loops for numSteps steps.  `gp`: dict from BatchedControlAffineGP.as_dict() (learned
    residual, one GP per trajectory) or None (fixed-kernel model M_k = 0, B_k = I, A = diag(kernel_diag_A)).
    Returns dict(stats..., x_final[Bt,3], traj (if record)).  Collectives: one, at the end.
    use_graph: capture one closed-loop step (plan row gather, the fused control step, the safety bookkeeping) in a HIP
    graph and replay it numSteps times -- the loop is launch bound for small batches (about ten launches per step).
    plant: "true" (default) -- the deterministic Ackermann drive x += g(x; L_true) u dt -- or "posterior": every step's plant is a
    draw from the model's OWN posterior, xdot ~ N(fhat + ghat u + M_k ubar, (ubar' B_k ubar) A) (`ops.unicycle_control_step_prepare`
    with `sampled`; L_true is ignored), which is the distribution the controller's chance constraint P(CBC_k >= 0) >= 1 - max_risk
    is stated under.  The standard normals z_all[numSteps,Bt,3] are drawn once from the seeded device generator, after the start
    noise; row t is gathered like the plan row, so the same seed gives the same trajectories eager and under use_graph.  The
    result gains risk = dict(instance_steps, violations, rate, max_risk, per_obstacle, min_cbc) (`distributed.reduce_risk_stats`):
    over the solved instance-steps, how often an obstacle row's condition was negative ON THE DRAW -- the empirical risk to hold
    against max_risk -- and, with record, cbc_s[numSteps,Bt,1+Kob] and status[numSteps,Bt], the drawn conditions and the solver's
    status of every step.  Draws of different steps
    are independent: each step's marginal at the visited (x_t, u_t) is exact, which is all the per-step constraint speaks about; a
    trajectory is NOT one function drawn from the GP (that would mean conditioning on the earlier draws, `ops.gp_append`)."""
    if plant not in ("true", "posterior"):
        raise ValueError("plant must be 'true' or 'posterior', got %r" % (plant,))
    sampled = plant == "posterior"
    dev = torch.device(device)
    f = dict(dtype=dtype, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x0 = torch.tensor(start, **f)
    xg = torch.tensor(goal, **f)
    task = unicycle_task_tensors(Bt, x0, xg, dtype, dev, max_risk=max_risk)
    planner = PiecewiseLinearPlanner(x0, xg, numSteps, dt, frac_time_to_reach_goal=0.95)
    x = (x0 + start_noise * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    ws = ops.control_workspace(Bt, 2, dtype, dev)
    if gp is None:
        A = torch.diag(torch.tensor(kernel_diag_A, **f)).expand(Bt, 3, 3).contiguous()
        ws["Mk"].zero_()                                   # fixed-kernel model: M_k = 0, B_k = I are inputs of the step
        ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        fixed = dict(A=A)
    min_h = torch.full((Bt,), float("inf"), **f)
    cost = torch.zeros(Bt, **f)
    fails = torch.zeros(Bt, dtype=torch.int32, device=dev)
    gam = task["gammas"]
    traj = torch.empty(numSteps + 1, Bt, 3, **f) if record else None
    if record:
        traj[0] = x
    # the whole plan goes to the device once; per step two broadcast copies into the task buffers
    plan_all = torch.stack([planner.plan(t).to(dtype=dtype) for t in range(numSteps)]).to(dev)
    dplan_all = torch.stack([planner.dot_plan(t).to(dtype=dtype) for t in range(numSteps)]).to(dev)
    task["plan"], task["dot_plan"] = torch.empty(Bt, 3, **f), torch.empty(Bt, 3, **f)
    state = [x, min_h, cost, fails]                        # what a step changes (saved / restored around the graph capture)
    draw = None
    if sampled:
        z_all = torch.randn(numSteps, Bt, 3, generator=gen, **f)
        draw = dict(z=torch.empty(Bt, 3, **f), xdot_s=torch.zeros(Bt, 3, **f), cbc_s=torch.zeros(Bt, 3, **f))
        viol = torch.zeros(Bt, 2, dtype=torch.int32, device=dev)
        solved = torch.zeros(Bt, dtype=torch.int32, device=dev)
        min_cbc = torch.full((Bt, 2), float("inf"), **f)
        cbc_traj = torch.empty(numSteps, Bt, 3, **f) if record else None
        status_traj = torch.empty(numSteps, Bt, dtype=torch.int32, device=dev) if record else None
        state += [viol, solved, min_cbc]
    step = ops.unicycle_control_step_prepare(gp if gp is not None else fixed, task, ws, x, dt=dt, L_true=L_true,
                                             L_mean=L_mean, max_iters=max_iters, sampled=draw)
    import time
    w_cost = task["w"]

    def one_step(t):
        # plan row t -> task buffers (t is a python int, or a device index tensor inside the captured graph)
        if torch.is_tensor(t):
            task["plan"].copy_(plan_all.index_select(0, t))
            task["dot_plan"].copy_(dplan_all.index_select(0, t))
            if sampled:
                draw["z"].copy_(z_all.index_select(0, t)[0])
        else:
            task["plan"].copy_(plan_all[t])
            task["dot_plan"].copy_(dplan_all[t])
            if sampled:
                draw["z"].copy_(z_all[t])
        step()       # one host call, two launches (one for the fixed-kernel model): rows -> terms -> SOCP -> plant step
        # safety bookkeeping in ONE launch: min_h over the obstacle rows h_k(x_t) = cst_k / gamma_k (before the step; a
        # non-finite h counts as a collision), and -- only where the program was solved: an unsolved program (MAXITER /
        # infeasible / bad cone) is where the reference raises ValueError (unicycle_move_to_pose.py:954-964), the kernel
        # leaves that instance's state untouched for the step and its y is not a control -- the cost; else a failure count
        ops.rollout_stats(ws["cst"], ws["y"], ws["status"], w_cost, gam, min_h, cost, fails)
        if sampled:      # ... and the risk bookkeeping on the drawn conditions, one more launch
            ops.rollout_risk(draw["cbc_s"], ws["status"], viol, solved, min_cbc)

    torch.cuda.synchronize(dev)
    graph = None
    if use_graph and not record:
        tctr = torch.zeros(1, dtype=torch.long, device=dev)
        side = torch.cuda.Stream(device=dev)
        saved = [v.clone() for v in state]
        with torch.cuda.stream(side):                   # warm-up on the capture stream (allocator, lazy module load)
            one_step(tctr)
        side.synchronize()
        for dst, src in zip(state, saved):
            dst.copy_(src)
        tctr.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one_step(tctr)
            tctr.add_(1)
        for dst, src in zip(state, saved):    # capture does not execute, but keep the state explicit
            dst.copy_(src)
        tctr.zero_()
        torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    for t in range(numSteps):
        if graph is not None:
            graph.replay()
        else:
            one_step(t)
        if record:
            traj[t + 1] = x
            if sampled:
                cbc_traj[t] = draw["cbc_s"]
                status_traj[t] = ws["status"]
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter() - t_loop
    collided = ~(min_h >= 0)                       # NaN-safe: anything that is not provably >= 0 is a collision
    stats = reduce_rollout_stats(collided.sum(), min_h.min(), cost.sum() / numSteps, (fails > 0).sum(), Bt)
    dist_to_goal = (x[:, :2] - xg[:2]).norm(dim=1)
    out = dict(stats=stats, x_final=x, min_h=min_h, dist_to_goal=dist_to_goal, traj=traj, loop_seconds=t_loop)
    if sampled:
        out.update(risk=reduce_risk_stats(solved.sum(), viol.sum(0), min_cbc.min(0).values, max_risk), cbc_s=cbc_traj, status=status_traj)
    return out


def random_obstacle_field(Kf, start=(-3.0, -1.0, -math.pi / 4), goal=(0.0, 0.0, math.pi / 4), seed=0,
                          box=((-3.5, 0.5), (-2.0, 1.0)), radius=(0.1, 0.35), clear_start=0.5, clear_goal=0.4,
                          dtype=torch.float64, device="cpu"):
    """Kf discs for `obstacle_field_rollouts`: centres uniform in `box`, radii uniform in `radius`; a disc is rejected when its
    centre is closer than radius + clear_start to the start or radius + clear_goal to the goal.  Drawn on the host from
    numpy's seeded RandomState (the same discs on every device).  Returns dict(centers[Kf,2], radii[Kf])."""
    import numpy as np
    rng = np.random.RandomState(seed)
    cen, rad = [], []
    while len(rad) < Kf:
        c = (rng.uniform(*box[0]), rng.uniform(*box[1]))
        r = rng.uniform(*radius)
        if math.hypot(c[0] - start[0], c[1] - start[1]) < r + clear_start or math.hypot(c[0] - goal[0], c[1] - goal[1]) < r + clear_goal:
            continue
        cen.append(c)
        rad.append(r)
    return dict(centers=torch.tensor(np.array(cen).reshape(Kf, 2), dtype=dtype, device=device),
                radii=torch.tensor(np.array(rad), dtype=dtype, device=device))


def obstacle_field_rollouts(Bt, field, numSteps=200, dt=0.05, gp=None, kernel_diag_A=(1e-2, 1e-2, 1e-2), L_mean=1.0, L_true=12.0,
                            start=(-3.0, -1.0, -math.pi / 4), goal=(0.0, 0.0, math.pi / 4), start_noise=0.05, max_risk=0.01,
                            dtype=torch.float64, device="cuda", seed=0, slots=3, rounds=3, record=False, max_iters=30,
                            use_graph=False, tol_f=None, tol_a=None, plant="true", x_start=None, z_all=None):
    """`monte_carlo_safety_rollouts` among the discs of `field` = dict(centers[Kf,2] or [Bt,Kf,2], radii) -- up to 256 of them
    (`random_obstacle_field`): every step solves the program on a working set of `slots` discs and certifies it against the whole
    field (`ops.unicycle_field_control_step_prepare`, at most `rounds` solves).  A step that is not certified, or not solved, is
    not taken: that instance keeps its state for the step and counts as a failure, as an unsolved program does there.
    The result of `monte_carlo_safety_rollouts` (min_h over the WHOLE field), plus over all instance-steps:
    certified_steps, rounds_hist[rounds] (certified after r swaps), uncertified_steps (rounds ran out), full_set_steps (every slot
    active and a disc still violated), unsolved_steps (the working-set program was not solved); with record, traj[numSteps+1,Bt,3],
    y[numSteps,Bt,3], cert, rounds_rec, status_eff [numSteps,Bt] and idx[numSteps,Bt,slots].
    plant: "true" (default) -- the Ackermann drive with L_true -- or "posterior": every certified step is taken on a draw from the
    model's own posterior (`ops.obstacle_field_commit_sampled`; L_true is ignored) and the condition of EVERY disc of the field is
    evaluated on that draw.  The normals z_all[numSteps,Bt,3] are drawn once from the seeded device generator, after the start
    noise, and row t is gathered like the plan row: the same bits eager and under use_graph.  The result gains
    risk = dict(tight, joint, unselected -- rates over the solved (certified) instance-steps: the drawn condition of the tightest
    cone was negative (what max_risk promises, per cone), ANY disc's was (which only the union bound covers), a disc's outside the
    working set was; mean_discs_violated, min_cbc, instance_steps, max_risk) (`distributed.reduce_risk_stats`), solved[Bt] and the
    per-instance counters risk_counters; with record also cbc_min, cbc_tight, cbc_argmin, tight_idx, nneg [numSteps,Bt].  Draws of
    different steps are independent (exact per-step marginals, not one function drawn along the trajectory).
    x_start[Bt,3] / z_all[numSteps,Bt,3]: the caller's start states / normals in place of the seeded ones (a study that pairs or
    permutes instances)."""
    if plant not in ("true", "posterior"):
        raise ValueError("plant must be 'true' or 'posterior', got %r" % (plant,))
    sampled = plant == "posterior"
    dev = torch.device(device)
    f = dict(dtype=dtype, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x0 = torch.tensor(start, **f)
    xg = torch.tensor(goal, **f)
    S = int(slots)
    task = unicycle_task_tensors(Bt, x0, xg, dtype, dev, max_risk=max_risk, cbf_gammas=(5.0,) * S)
    task["sign"] = torch.tensor([-1.0] + [1.0] * S, **f)
    task["relax_mask"] = torch.tensor([1.0] + [0.0] * S, **f)
    field = dict(centers=field["centers"].to(**f).contiguous(), radii=field["radii"].to(**f).contiguous())
    planner = PiecewiseLinearPlanner(x0, xg, numSteps, dt, frac_time_to_reach_goal=0.95)
    x = (x0 + start_noise * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    if x_start is not None:
        x = x_start.to(**f).reshape(Bt, 3).clone().contiguous()
    ws = ops.control_workspace(Bt, S, dtype, dev)
    fws = ops.obstacle_field_workspace(Bt, S, dtype, dev)
    if gp is None:
        A = torch.diag(torch.tensor(kernel_diag_A, **f)).expand(Bt, 3, 3).contiguous()
        ws["Mk"].zero_()
        ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        gp = dict(A=A)
    plan_all = torch.stack([planner.plan(t).to(dtype=dtype) for t in range(numSteps)]).to(dev)
    dplan_all = torch.stack([planner.dot_plan(t).to(dtype=dtype) for t in range(numSteps)]).to(dev)
    task["plan"], task["dot_plan"] = torch.empty(Bt, 3, **f), torch.empty(Bt, 3, **f)
    # counters of the certificate, accumulated on the device: [certified after 0 .. rounds-1 swaps | uncertified | full | unsolved]
    counts = torch.zeros(rounds + 3, dtype=torch.long, device=dev)
    bin_ids = torch.arange(rounds + 3, **i32)
    state =[x, fws["min_h"], fws["cost"], fws["fails"], counts]
    risk = draw = None
    if sampled:
        z_all = torch.randn(numSteps, Bt, 3, generator=gen, **f) if z_all is None else z_all.to(**f).reshape(numSteps, Bt, 3).contiguous()
        risk = ops.obstacle_field_risk_workspace(Bt, dtype, dev)
        draw = dict(z=risk["z"], risk=risk)
        state += [risk[k] for k in ops._FIELD_RISK_SUMS]
    step = ops.unicycle_field_control_step_prepare(gp, task, field, ws, x, rounds=rounds, dt=dt, L_true=L_true, L_mean=L_mean,
                                                   max_iters=max_iters, fws=fws, tol_f=tol_f, tol_a=tol_a, sampled=draw)
    rec = None
    if record:
        rec = dict(traj=torch.empty(numSteps + 1, Bt, 3, **f), y=torch.empty(numSteps, Bt, 3, **f),
                   cert=torch.empty(numSteps, Bt, **i32), rounds_rec=torch.empty(numSteps, Bt, **i32),
                   status_eff=torch.empty(numSteps, Bt, **i32), idx=torch.empty(numSteps, Bt, S, **i32))
        rec["traj"][0] = x
        if sampled:
            rec.update({k: torch.empty(numSteps, Bt, dtype=risk[k].dtype, device=dev) for k in ops._FIELD_RISK_STEP[1:]})

    def one_step(t):
        if torch.is_tensor(t):
            task["plan"].copy_(plan_all.index_select(0, t))
            task["dot_plan"].copy_(dplan_all.index_select(0, t))
            if sampled:
                risk["z"].copy_(z_all.index_select(0, t)[0])
        else:
            task["plan"].copy_(plan_all[t])
            task["dot_plan"].copy_(dplan_all[t])
            if sampled:
                risk["z"].copy_(z_all[t])
        step()
        cert, eff = fws["cert"], fws["status_eff"]
        # bin per instance: certified -> its number of swaps; else rounds (uncertified), rounds + 1 (full), rounds + 2 (unsolved)
        other = rounds + 2 - 2 * (eff == ops.FIELD_UNCERTIFIED).to(torch.int32) + (cert == ops.FIELD_FULL).to(torch.int32)
        bins = torch.where(cert == ops.FIELD_CERTIFIED, fws["rounds"].clamp(max=rounds - 1), other)
        counts.add_((bins[:, None] == bin_ids[None]).sum(0))          # (no bincount: its output size is a host look)

    torch.cuda.synchronize(dev)
    graph = None
    if use_graph and not record:
        tctr = torch.zeros(1, dtype=torch.long, device=dev)
        side = torch.cuda.Stream(device=dev)
        saved = [v.clone() for v in state]
        with torch.cuda.stream(side):
            one_step(tctr)
        side.synchronize()
        for dst, src in zip(state, saved):
            dst.copy_(src)
        tctr.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one_step(tctr)
            tctr.add_(1)
        for dst, src in zip(state, saved):
            dst.copy_(src)
        tctr.zero_()
        torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    for t in range(numSteps):
        if graph is not None:
            graph.replay()
        else:
            one_step(t)
        if record:
            rec["traj"][t + 1] = x
            rec["y"][t] = ws["y"]
            rec["cert"][t], rec["rounds_rec"][t], rec["status_eff"][t] = fws["cert"], fws["rounds"], fws["status_eff"]
            rec["idx"][t] = fws["idx"]
            if sampled:
                for k in ops._FIELD_RISK_STEP[1:]:
                    rec[k][t] = risk[k]
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter() - t_loop
    min_h, cost, fails = fws["min_h"], fws["cost"], fws["fails"]
    collided = ~(min_h >= 0)
    stats = reduce_rollout_stats(collided.sum(), min_h.min(), cost.sum() / numSteps, (fails > 0).sum(), Bt)
    c = counts.tolist()
    out = dict(stats=stats, x_final=x, min_h=min_h, dist_to_goal=(x[:, :2] - xg[:2]).norm(dim=1), loop_seconds=t_loop,
               certified_steps=sum(c[:rounds]), rounds_hist=c[:rounds], uncertified_steps=c[rounds], full_set_steps=c[rounds + 1],
               unsolved_steps=c[rounds + 2], traj=None)
    if sampled:
        sums = torch.stack([risk[k].sum() for k in ("viol_tight", "viol_any", "viol_unselected", "viol_discs")])
        r = reduce_risk_stats(risk["solved"].sum(), sums, risk["min_cbc"].min().reshape(1), max_risk)
        tight, joint, unsel, discs = (v["violations"] for v in r["per_obstacle"])
        n = r["instance_steps"]
        out.update(risk=dict(tight=tight / max(n, 1), joint=joint / max(n, 1), unselected=unsel / max(n, 1),
                             mean_discs_violated=discs / max(n, 1), min_cbc=r["min_cbc"][0], instance_steps=n,
                             max_risk=float(max_risk)),
                   solved=risk["solved"], risk_counters={k: risk[k] for k in ops._FIELD_RISK_SUMS})
    if record:
        out.update(rec)
    return out


def _trigger_hyper(ls, sf, A, B, Bt, f):
    """ls, sf, A, B of one model or of Bt models -> dict(ls[Bh,3], sf[Bh], Adiag[Bh,3], B[Bh,3,3]) for the trigger step, Bh = 1 or Bt
    (mixed leading extents are expanded to Bt)."""
    ls, sf, A, B = (torch.as_tensor(v, **f) for v in (ls, sf, A, B))       # (python numbers go straight to the working type)
    ls, sf, A, B = ls.reshape(-1, 3), sf.reshape(-1), A.reshape(-1, 3, 3), B.reshape(-1, 3, 3)
    ext = {v.shape[0] for v in (ls, sf, A, B)}
    if not ext <= {1, Bt}:
        raise ValueError("trigger hyper-parameters: ls %s, sf %s, A %s, B %s: one model or one per instance (Bt = %d)"
                         % (tuple(ls.shape), tuple(sf.shape), tuple(A.shape), tuple(B.shape), Bt))
    Bh = max(ext)
    ex = lambda v: v.expand(Bh, *v.shape[1:]).contiguous()
    return dict(ls=ex(ls), sf=ex(sf), Adiag=ex(torch.diagonal(A, dim1=-2, dim2=-1)), B=ex(B))


def self_triggered_rollouts(Bt, horizon=10.0, dt=0.05, gp=None, trigger_hyper=None, tau_min=1e-3, tau_max=0.05, max_events=None,
                            kernel_diag_A=(1e-2, 1e-2, 1e-2), L_mean=1.0, L_true=12.0, start=(-3.0, -1.0, -math.pi / 4),
                            goal=(0.0, 0.0, math.pi / 4), start_noise=0.05, max_risk=0.01, dtype=torch.float64, device="cuda",
                            seed=0, record=False, max_iters=30, use_graph=False, Nte=1e3, off=None, deltaL=1e-4, zeta=1e-2,
                            L_alpha=1.0, plant="true", audit=False):
    """The closed loop that ACTS on the self-triggering time: Bt instances of the recipe of `monte_carlo_safety_rollouts` (same
    task, same start states for the same seed, true plant), but every instance re-solves when its model says the last control stops
    being safe, not every dt.  One EVENT is the control step with dt = 0 (solve only), the trigger step
    (`ops.unicycle_trigger_step_prepare`: tau on the test grid around x, the control held for dt_b = min(clamp(tau, tau_min,
    tau_max), horizon - t) on the plant, the instance's clock and the planner rows of its new time) and `ops.rollout_stats`.
    The planner keeps its step-indexed definition: `dt` is ITS step, round(horizon / dt) rows, row min(floor(t / dt), P - 1) at
    time t.  `max_events` iterations run with no device read (default ceil(horizon / tau_min), by which every instance is done).
    Instances run on their own clocks; one that has reached `horizon` IDLES through the remaining iterations: its control step is
    still solved (skipping it is not done here), its state, clock, event count and statistics no longer change.
    gp: dict from BatchedControlAffineGP.as_dict() -- ls, sf, A, B of the bound are its ell, s2 (the output scale the reference
    logs as knl_scalefactor), A, Bm -- or None: the fixed-kernel model, whose data kernel the bound needs from
    trigger_hyper = dict(ls, sf, A, B) (one model or one per instance).  Any data kernel but RBF is refused.  Nte / off: the test
    grid (`trigger_interval.default_test_grid`).  use_graph: capture one event and replay it (ignored with record).
    Returns dict(stats (`reduce_rollout_stats`; mean_cost is per event), x_final, t[Bt], events[Bt], events_per_second[Bt] =
    events / t, done = share of instances with t == horizon, dt_used = dict(min, median, max) over all events taken,
    share_at_tau_min = the share of those events held for exactly tau_min (clamped up to it: tau's promise is not in force), min_h,
    dist_to_goal, loop_seconds, task (the task tensors), and with record: rec = dict(x_before, u, status, tau, dt_used, t, x_after,
    active, and what the solve of the event read and formed: plan, dot_plan, Mk, Bk) of [max_events, Bt, ...] tensors, `active`
    telling which instances took that event (the rows of the others are stale)).
    dt_used of every event is kept on the device ([max_events, Bt] in the working type) for the three figures.
    plant: "true" (default) or "posterior": every event's plant is a draw from the model's OWN posterior at (x_e, u_e), xdot_s ~
    N(fhat + ghat u + M_k ubar, (ubar' B_k ubar) A), held for the event's dt_b (`ops.unicycle_trigger_step_prepare` with `sampled`;
    L_true is ignored): the distribution the chance constraint P(CBC_k >= 0) >= 1 - max_risk is stated under.  The standard
    normals z_all[max_events, Bt, 3] are drawn once from the seeded generator, after the start noise; row e is gathered by the
    device event counter, so the same seed gives the same run eager and under use_graph.  Each event's plant is ONE posterior draw
    at (x_e, u_e) held for dt_b: exact per-event marginals, not one function drawn along the trajectory.  A held draw moves the
    state by xdot_s dt_b, so the noise a trajectory accumulates depends on its event rate (n events of length h add a
    displacement of standard deviation ~ sqrt(n) h; the same time in one event adds n h).  The result gains risk =
    `distributed.reduce_risk_stats` over the SOLVED events of LIVE instances (an idle instance is not counted): how often an
    obstacle row's condition was negative on the draw, to hold against max_risk.
    audit: the control of every solved event is looked at again where it is released -- at the next event's state, on the rows that
    event's solve wrote -- (`ops.unicycle_trigger_step_prepare` with `audit`): mean_k and margin_k = mean_k - rho std_k of every
    obstacle row's condition under the HELD control.  tau promises margin_k >= 0 there; where the hold was clamped up to tau_min
    the promise is not in force, and this is the measurement of what that costs.  The result gains audit = dict(events (audited),
    neg_mean, neg_margin (per obstacle), rate_mean, rate_margin (over events x obstacles), min_mean, min_margin (per obstacle)).
    With record, rec gains z, xdot_s, cbc_s (plant="posterior") and held (the flag BEFORE the event), held_mean, held_margin
    (audit=True; rows are stale where held == 0 or the instance was idle).  The defaults are the loop as it was, bit for bit."""
    from . import trigger_interval as ti
    if plant not in ("true", "posterior"):
        raise ValueError("plant must be 'true' or 'posterior', got %r" % (plant,))
    sampled = plant == "posterior"
    f = dict(dtype=dtype, device=torch.device(device))
    if gp is not None:
        ti._require_rbf(gp.get("kernel", "rbf"))
        hyper = _trigger_hyper(gp["ell"], gp["s2"], gp["A"], gp["Bm"], Bt, f)
    else:
        if trigger_hyper is None or not {"ls", "sf", "A", "B"} <= set(trigger_hyper):
            raise ValueError("self_triggered_rollouts: the fixed-kernel model has no data kernel of its own: pass "
                             "trigger_hyper=dict(ls, sf, A, B)")
        ti._require_rbf(trigger_hyper.get("kernel", "rbf"))
        hyper = _trigger_hyper(trigger_hyper["ls"], trigger_hyper["sf"], trigger_hyper["A"], trigger_hyper["B"], Bt, f)
    c = _self_triggered_setup("self_triggered_rollouts", Bt, horizon, dt, tau_min, tau_max, max_events, start, goal, start_noise,
                              max_risk, dtype, device, seed, Nte, off, sampled, audit)
    ws, task, x = c.ws, c.task, c.x
    if gp is None:
        A = torch.diag(torch.tensor(kernel_diag_A, **f)).expand(Bt, 3, 3).contiguous()
        ws["Mk"].zero_()
        ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        gp = dict(A=A)
    solve = ops.unicycle_control_step_prepare(gp, task, ws, x, dt=0.0, L_true=L_true, L_mean=L_mean, max_iters=max_iters)
    trigger = ops.unicycle_trigger_step_prepare(task, ws, c.tws, x, c.off, c.r, hyper, c.plan_all, c.dplan_all, dt, horizon, tau_min,
                                                tau_max, L_true=L_true, deltaL=deltaL, zeta=zeta, L_alpha=L_alpha,
                                                **(dict(gp_A=gp["A"], sampled=c.draw, audit=c.hold) if c.aws is not None else {}))
    rec, before, after = _self_triggered_record(c) if record else (None, None, None)
    c.loop_seconds = _self_triggered_run(c, [lambda: _self_triggered_event(c, solve, trigger)], c.state, use_graph and not record,
                                         before=before, after=after)
    return _self_triggered_result(c, rec)


def _self_triggered_setup(who, Bt, horizon, dt, tau_min, tau_max, max_events, start, goal, start_noise, max_risk, dtype, device, seed,
                          Nte, off, sampled, audit):
    """What the self-triggered loops share before their model enters: the task, the start states (the generator's first draws),
    the posterior plant's normals (its next), the planner's tables, the test grid, the workspaces and the statistics buffers, as
    one namespace.  `state`: what an event changes (saved and restored around a graph capture)."""
    import types
    from . import trigger_interval as ti
    dev = torch.device(device)
    f = dict(dtype=dtype, device=dev)
    if not (0 < tau_min <= tau_max < math.inf) or not horizon > 0:
        raise ValueError("%s: need 0 < tau_min <= tau_max < inf and horizon > 0" % who)
    numSteps = max(3, int(round(horizon / dt)))
    if max_events is None:
        max_events = int(math.ceil(horizon / tau_min))
    gen = torch.Generator(device=dev).manual_seed(seed)
    x0, xg = torch.tensor(start, **f), torch.tensor(goal, **f)
    task = unicycle_task_tensors(Bt, x0, xg, dtype, dev, max_risk=max_risk)
    planner = PiecewiseLinearPlanner(x0, xg, numSteps, dt, frac_time_to_reach_goal=0.95)
    x = (x0 + start_noise * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    z_all = torch.randn(max_events, Bt, 3, generator=gen, **f) if sampled else None
    ws = ops.control_workspace(Bt, 2, dtype, dev)
    tws = ops.trigger_workspace(Bt, dtype, dev)
    aws = ops.trigger_audit_workspace(Bt, 2, dtype, dev) if (sampled or audit) else None
    draw = aws["sampled"] if sampled else None
    hold = aws["audit"] if audit else None
    off_np = ti.default_test_grid(3, Nte) if off is None else (off.detach().cpu().numpy() if torch.is_tensor(off) else off)
    r = ti._grid_norm(off_np)
    off = torch.as_tensor(off_np).to(**f).contiguous()
    plan_all = torch.stack([planner.plan(s).to(dtype=dtype) for s in range(numSteps)]).to(dev).contiguous()
    dplan_all = torch.stack([planner.dot_plan(s).to(dtype=dtype) for s in range(numSteps)]).to(dev).contiguous()
    task["plan"], task["dot_plan"] = plan_all[0].expand(Bt, 3).contiguous(), dplan_all[0].expand(Bt, 3).contiguous()
    min_h = torch.full((Bt,), float("inf"), **f)
    cost, cost_prev = torch.zeros(Bt, **f), torch.zeros(Bt, **f)
    fails, fails_prev = (torch.zeros(Bt, dtype=torch.int32, device=dev) for _ in range(2))
    active = torch.empty(Bt, dtype=torch.bool, device=dev)
    dt_hist = torch.zeros(max_events, Bt, **f)
    act_hist = torch.zeros(max_events, Bt, dtype=torch.bool, device=dev)
    ectr = torch.zeros(1, dtype=torch.long, device=dev)
    t, events = tws["t"], tws["events"]
    state = [x, min_h, cost, fails, t, events, task["plan"], task["dot_plan"], dt_hist, act_hist, ectr]
    if sampled:
        state += [draw["viol"], draw["solved"], draw["min_cbc"]]
    if audit:
        state += [hold[k] for k in ("u_held", "held", "audit_n", "audit_neg", "audit_min")]
    return types.SimpleNamespace(Bt=Bt, horizon=horizon, tau_min=tau_min, max_events=max_events, max_risk=max_risk, dtype=dtype, dev=dev,
                                 f=f, gen=gen, xg=xg, task=task, x=x, z_all=z_all, ws=ws, tws=tws, aws=aws, draw=draw, hold=hold, off=off,
                                 r=r, plan_all=plan_all, dplan_all=dplan_all, min_h=min_h, min_h_prev=torch.empty_like(min_h), cost=cost, cost_prev=cost_prev, fails=fails,
                                 fails_prev=fails_prev, active=active, dt_hist=dt_hist, act_hist=act_hist, ectr=ectr, t=t, events=events,
                                 state=state, sampled=sampled, audit=audit)


def _self_triggered_event(c, solve, trigger, freeze_min_h=False):
    """One event of a self-triggered loop on the buffers of `_self_triggered_setup`: no device read, capturable.
    freeze_min_h: an idle instance's min_h is put back too.  The bookkeeping launch evaluates h at the state BEFORE the step, so
    without it the first idle iteration of an instance that finished early adds h of its final state to its minimum -- a state
    that an instance finishing at the last iteration never has evaluated (`self_triggered_rollouts` keeps that, as it always did)."""
    ws = c.ws
    torch.lt(c.t, c.horizon, out=c.active)      # who takes this event (the trigger step leaves the others alone)
    solve()                                     # rows -> terms -> SOCP at the current state, no plant
    if c.sampled:                               # this event's draws, by the device event counter
        c.draw["z"].copy_(c.z_all.index_select(0, c.ectr)[0])
    trigger()                                   # tau, the plant over the time the control is held, clock, planner rows
    # the bookkeeping of `monte_carlo_safety_rollouts`, per event; an idle instance's cost and failure count are put back
    # (its min_h cannot change: its state does not)
    c.cost_prev.copy_(c.cost)
    c.fails_prev.copy_(c.fails)
    if freeze_min_h:
        c.min_h_prev.copy_(c.min_h)
    ops.rollout_stats(ws["cst"], ws["y"], ws["status"], c.task["w"], c.task["gammas"], c.min_h, c.cost, c.fails)
    torch.where(c.active, c.cost, c.cost_prev, out=c.cost)
    torch.where(c.active, c.fails, c.fails_prev, out=c.fails)
    if freeze_min_h:
        torch.where(c.active, c.min_h, c.min_h_prev, out=c.min_h)
    c.dt_hist.index_copy_(0, c.ectr, c.tws["dt_used"][None])
    c.act_hist.index_copy_(0, c.ectr, c.active[None])
    c.ectr.add_(1)


def _self_triggered_record(c):
    """(rec, before(e), after(e)): the per-event record of a self-triggered loop and the two hooks that fill it around an event."""
    Bt, f, dev, E = c.Bt, c.f, c.dev, c.max_events
    ws, tws, task, x, draw, hold = c.ws, c.tws, c.task, c.x, c.draw, c.hold
    rec = dict(x_before=torch.empty(E, Bt, 3, **f), u=torch.empty(E, Bt, 2, **f), status=torch.empty(E, Bt, dtype=torch.int32, device=dev),
               tau=torch.empty(E, Bt, **f), dt_used=c.dt_hist, t=torch.empty(E, Bt, dtype=torch.float64, device=dev),
               x_after=torch.empty(E, Bt, 3, **f), active=c.act_hist, plan=torch.empty(E, Bt, 3, **f), dot_plan=torch.empty(E, Bt, 3, **f),
               Mk=torch.empty(E, Bt, 3, 3, **f), Bk=torch.empty(E, Bt, 3, 3, **f))
    if c.sampled:
        rec.update(z=c.z_all, xdot_s=torch.empty(E, Bt, 3, **f), cbc_s=torch.empty(E, Bt, 3, **f))
    if c.audit:
        rec.update(held=torch.empty(E, Bt, dtype=torch.int32, device=dev), held_mean=torch.empty(E, Bt, 2, **f),
                   held_margin=torch.empty(E, Bt, 2, **f))

    def before(e):
        rec["x_before"][e], rec["plan"][e], rec["dot_plan"][e] = x, task["plan"], task["dot_plan"]
        if c.audit:
            rec["held"][e] = hold["held"]

    def after(e):
        rec["u"][e], rec["Mk"][e], rec["Bk"][e] = ws["y"][:, :2], ws["Mk"], ws["Bk"]
        rec["status"][e] = ws["status"]
        rec["tau"][e] = tws["tau"]
        rec["t"][e] = c.t
        rec["x_after"][e] = x
        if c.sampled:
            rec["xdot_s"][e], rec["cbc_s"][e] = draw["xdot_s"], draw["cbc_s"]
        if c.audit:
            rec["held_mean"][e], rec["held_margin"][e] = hold["held_mean"], hold["held_margin"]
    return rec, before, after


def _self_triggered_run(c, event_fns, state, use_graph, which=None, between=None, before=None, after=None):
    """The max_events iterations of a self-triggered loop; returns the seconds they took.  event_fns: one event closure per set of
    bound buffers (one for a frozen model; the learning loop has one per operator buffer), which(e) -> the index of the one
    iteration e runs.  use_graph: every closure is captured once (warm-up on the capture stream, `state` saved and restored around
    it) and replayed.  between(e): eager work after iteration e (the refits).  before(e) / after(e): the record's hooks (eager)."""
    dev = c.dev
    torch.cuda.synchronize(dev)
    graphs = None
    if use_graph:
        side = torch.cuda.Stream(device=dev)
        saved = [v.clone() for v in state]
        graphs = []
        for fn in event_fns:
            with torch.cuda.stream(side):               # warm-up on the capture stream (allocator, lazy module load)
                fn()
            side.synchronize()
            for dst, src in zip(state, saved):
                dst.copy_(src)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                fn()
            for dst, src in zip(state, saved):
                dst.copy_(src)
            graphs.append(graph)
        torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    for e in range(c.max_events):
        k = which(e) if which is not None else 0
        if graphs is not None:
            graphs[k].replay()
        else:
            if before is not None:
                before(e)
            event_fns[k]()
            if after is not None:
                after(e)
        if between is not None:
            between(e)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t_loop


def _self_triggered_result(c, rec):
    """The statistics every self-triggered loop returns (see `self_triggered_rollouts`)."""
    Bt, f, x, t, events, draw, hold = c.Bt, c.f, c.x, c.t, c.events, c.draw, c.hold
    collided = ~(c.min_h >= 0)
    per_event_cost = c.cost / events.clamp(min=1).to(c.dtype)
    stats = reduce_rollout_stats(collided.sum(), c.min_h.min(), per_event_cost.sum(), (c.fails > 0).sum(), Bt)
    taken = c.dt_hist[c.act_hist]
    dt_used = dict(min=float(taken.min()), median=float(taken.median()), max=float(taken.max())) if taken.numel() else None
    at_min = float((taken == torch.tensor(c.tau_min, **f)).double().mean()) if taken.numel() else None
    out = dict(stats=stats, x_final=x, t=t, events=events, events_per_second=events.double() / t, done=float((t >= c.horizon).double().mean()),
               dt_used=dt_used, min_h=c.min_h, dist_to_goal=(x[:, :2] - c.xg[:2]).norm(dim=1), loop_seconds=c.loop_seconds, task=c.task, rec=rec,
               share_at_tau_min=at_min)
    if c.sampled:
        out["risk"] = reduce_risk_stats(draw["solved"].sum(), draw["viol"].sum(0), draw["min_cbc"].min(0).values, c.max_risk)
    if c.audit:
        n = int(hold["audit_n"].sum())
        neg = hold["audit_neg"].sum(0).tolist()                        # [Kob][mean, margin]
        mins = hold["audit_min"].min(0).values.double().tolist()
        rows = max(len(neg), 1)
        out["audit"] = dict(events=n, neg_mean=[int(v[0]) for v in neg], neg_margin=[int(v[1]) for v in neg],
                            rate_mean=sum(v[0] for v in neg) / max(n * rows, 1), rate_margin=sum(v[1] for v in neg) / max(n * rows, 1),
                            min_mean=[float(v[0]) for v in mins], min_margin=[float(v[1]) for v in mins])
    return out


def self_triggered_learning_rollouts(Bt, horizon=10.0, dt=0.05, max_train=512, refit_every=40, obs_every=1, tau_min=1e-3, tau_max=0.05,
                                     max_events=None, L_mean=1.0, L_true=12.0, retry_levels=3, min_jitter_level=1e-5, level_decay_every=4,
                                     start=(-3.0, -1.0, -math.pi / 4), goal=(0.0, 0.0, math.pi / 4), start_noise=0.05, max_risk=0.01,
                                     dtype=torch.float64, device="cuda", seed=0, record=False, max_iters=30, use_graph=False, Nte=1e3,
                                     off=None, deltaL=1e-4, zeta=1e-2, L_alpha=1.0, plant="true", audit=False):
    """The self-triggered closed loop that LEARNS ITS DYNAMICS ONLINE: the two halves of the paper's algorithm in one loop, as the
    reference's controller runs them (unicycle_move_to_pose.py:326-386, :970-978).  The events are those of
    `self_triggered_rollouts` -- same task, start states for the same seed, planner, trigger and statistics -- on a model that is
    refitted from the loop's own (x_e, u_e, x_{e+1}) rows with the host-free refits of `self_learning_closed_loop`.
    Start model: `synthetic.make_instances(Bt, max_train, 3, 2, variant="theta")`, one GP per instance; the trigger bound reads its
    ell, s2, A, Bm, which stay as they are (no hyper-parameter fit here).  The prior mean is AckermannDrive(L_mean) against a true
    wheelbase L_true, so there is a residual to learn.
    One EVENT: the solve with dt = 0 at the shift-invariant query xq = (0, 0, theta) (bcbf_unicycle_control_step_observe), the
    OBSERVING trigger step (bcbf_unicycle_trigger_step_observe: tau, the hold dt_b on the plant, the clock, the event as an
    observation row with ITS OWN dt_b, and xq at the new state) and the bookkeeping.  Stream layout, per instance: rows
    0 .. max_train - 1 the synthetic start, row max_train + e // obs_every the observation of event e when e % obs_every == 0.
    Live instances take events in lockstep, so after iteration e each of them has written 1 + e // obs_every rows; an instance
    that has reached the horizon writes no more, and the rows it never writes stay the plant at rest (`ops.trigger_observe_workspace`),
    true and uninformative.  When (e + 1) % refit_every == 0 the last max_train stream rows are refactored
    (`ops.refit_with_retries` + `ops.potrs`, a fresh level * rand jitter per factorisation, an instance starting at the level that
    last worked and going one level down every `level_decay_every`-th refit, never below `min_jitter_level`: the rules of
    `self_learning_closed_loop`) into the operator buffer that is not being read, and the buffers swap; nothing waits for the
    host.  use_graph: one captured event per operator buffer, the refits launched eagerly between the replays (ignored with record).
    plant="posterior" is refused: learning from draws of the model's own posterior teaches nothing.  audit: as in
    `self_triggered_rollouts`.  Once an instance has reached the horizon none of its statistics changes any more, min_h included
    (it is the minimum over the states at which the instance took an event).
    Returns what `self_triggered_rollouts` returns, and
      learning = dict(refits, refit_failures_after_retries, instances_factored_per_retry_level, jitter_level_max, rows_written[Bt],
                      window, obs_every);
      final = dict(rows = [dict(X, UH, Y, jitter)] ([Bt, max_train, .]: the raw rows the final model holds, with the jitter they were
              factored with), bounds = [(0, Bt)], hyper, posterior = (Mk, Bk) of the final model at xq_check, xq_check, window_lo (the
              stream row the window starts at), stream_rows = dict(X, UH, Y, row0)) -- the layout of `self_learning_closed_loop`'s;
      with record, rec gains obs_x, obs_uh, obs_y (the stream row of index max_train + e // obs_every after event e: this event's
      where e % obs_every == 0 and the instance was active, else an older or the rest row), xq (the query of the event's solve) and
      the running statistics cost, fails, min_h after the event."""
    from .synthetic import make_instances
    if plant != "true":
        raise ValueError("self_triggered_learning_rollouts: plant must be 'true' (got %r): learning from draws of the model's own "
                         "posterior teaches nothing" % (plant,))
    if max_train < 1 or refit_every < 1 or obs_every < 1:
        raise ValueError("self_triggered_learning_rollouts: need max_train >= 1, refit_every >= 1, obs_every >= 1")
    c = _self_triggered_setup("self_triggered_learning_rollouts", Bt, horizon, dt, tau_min, tau_max, max_events, start, goal,
                              start_noise, max_risk, dtype, device, seed, Nte, off, False, audit)
    f, dev, ws, task, x, W, E = c.f, c.dev, c.ws, c.task, c.x, max_train, c.max_events
    p = make_instances(Bt, W, 3, 2, dtype=dtype, device=dev, seed=seed, variant="theta")
    hp = {k: p[k] for k in ("ell", "s2", "Bm", "M0", "A")}
    hyper = _trigger_hyper(hp["ell"], hp["s2"], hp["A"], hp["Bm"], Bt, f)
    # the observation stream: the synthetic start, then one row per observed event
    ow = ops.trigger_observe_workspace(Bt, W + (E + obs_every - 1) // obs_every, dtype, dev)
    Xall, UHall, Yall = ow["obs"]
    Xall[:, :W], UHall[:, :W], Yall[:, :W] = p["X"], p["UH"], p["Xdot"]
    xq = ow["xq_next"]
    xq.copy_(x)
    xq[:, :2] = 0
    ow.update(row0=W, every=obs_every, L_mean=L_mean)
    E_ = ops.lop_elems(W, dtype)
    mk = lambda: dict(Lop=torch.empty(Bt, E_, **f), UHB=torch.empty(Bt, W, 3, **f), Vw=torch.empty(Bt, W, 3, **f), X=torch.empty(Bt, W, 3, **f))
    bufs = [mk(), mk()]
    info, info2 = (torch.zeros(Bt, dtype=torch.int32, device=dev) for _ in range(2))
    fail_count = torch.zeros((), dtype=torch.int64, device=dev)
    level = torch.full((Bt,), float(min_jitter_level), **f)          # make_psd's level per instance (x10 per failed attempt)
    retry_counts = torch.zeros(retry_levels + 1, dtype=torch.int64, device=dev)
    L = types_ns(cur=0, refits=0, lo=0, J=p["jitter"].clone())

    def factor_into(buf, Xw, UHw, Yw, Jw):
        ops.refit_with_retries(Xw, UHw, hp["Bm"], hp["ell"], hp["s2"], Jw, (buf["Lop"], buf["UHB"], info), levels=retry_levels,
                               scratch=info2, level=level, counts=retry_counts)
        ops.potrs(buf["Lop"], Yw, UHw, hp["M0"], want_alpha=False, out_Vw=buf["Vw"])
        buf["X"].copy_(Xw)
        fail_count.add_((info != 0).sum())

    factor_into(bufs[0], p["X"], p["UH"], p["Xdot"], L.J)
    for k, v in bufs[0].items():                                   # (both buffers hold a model from the start: a graph is captured on each)
        bufs[1][k].copy_(v)
    solves = [ops.unicycle_control_step_prepare(dict(b_, **hp), task, ws, x, dt=0.0, L_true=L_true, L_mean=L_mean, max_iters=max_iters,
                                                observe=dict(xq=xq, xq_next=None, shift_invariant=True)) for b_ in bufs]
    trigger = ops.unicycle_trigger_step_prepare(task, ws, c.tws, x, c.off, c.r, hyper, c.plan_all, c.dplan_all, dt, horizon, tau_min,
                                                tau_max, L_true=L_true, deltaL=deltaL, zeta=zeta, L_alpha=L_alpha, gp_A=hp["A"],
                                                audit=c.hold, observe=ow)

    def between(e):
        """After iteration e: every `refit_every`-th time, refactor the last W stream rows into the buffer that is not being read."""
        if (e + 1) % refit_every:
            return
        lo = 1 + e // obs_every                                     # live instances have written rows W .. W + e // obs_every
        cut = lambda t_: t_[:, lo:lo + W].contiguous()
        L.refits += 1
        if level_decay_every and L.refits % level_decay_every == 0:
            level.div_(10).clamp_(min=float(min_jitter_level))
        # a fresh jitter draw per factorisation, at the instance's level: one below the one that last worked (make_psd, :903-919)
        Jw = (level[:, None] * torch.rand(Bt, W, generator=c.gen, **f)).contiguous()
        factor_into(bufs[1 - L.cur], cut(Xall), cut(UHall), cut(Yall), Jw)
        L.cur, L.lo, L.J = 1 - L.cur, lo, Jw

    rec, before, after = None, None, None
    if record:
        rec, before0, after0 = _self_triggered_record(c)
        rec.update(obs_x=torch.empty(E, Bt, 3, **f), obs_uh=torch.empty(E, Bt, 3, **f), obs_y=torch.empty(E, Bt, 3, **f),
                   xq=torch.empty(E, Bt, 3, **f), cost=torch.empty(E, Bt, **f), fails=torch.empty(E, Bt, dtype=torch.int32, device=dev),
                   min_h=torch.empty(E, Bt, **f))

        def before(e):
            before0(e)
            rec["xq"][e] = xq

        def after(e):
            after0(e)
            row = W + e // obs_every
            rec["obs_x"][e], rec["obs_uh"][e], rec["obs_y"][e] = Xall[:, row], UHall[:, row], Yall[:, row]
            rec["cost"][e], rec["fails"][e], rec["min_h"][e] = c.cost, c.fails, c.min_h
    state = c.state + [Xall, UHall, Yall, xq]
    c.loop_seconds = _self_triggered_run(c, [lambda s_=s_: _self_triggered_event(c, s_, trigger, freeze_min_h=True) for s_ in solves], state,
                                         use_graph and not record, which=lambda e: L.cur, between=between, before=before, after=after)
    out = _self_triggered_result(c, rec)
    out["learning"] = dict(refits=L.refits, refit_failures_after_retries=int(fail_count),
                           instances_factored_per_retry_level=[int(v) for v in retry_counts.tolist()], jitter_level_max=float(level.max()),
                           rows_written=(c.events + (obs_every - 1)) // obs_every, window=W, obs_every=obs_every)
    b_ = bufs[L.cur]
    Mk, Bk = ops.posterior_step(b_["Lop"], b_["Vw"], b_["X"], b_["UHB"], hp["ell"], hp["s2"], hp["Bm"], hp["M0"], p["xq"])
    sl = slice(L.lo, L.lo + W)
    out["final"] = dict(rows=[dict(X=Xall[:, sl].clone(), UH=UHall[:, sl].clone(), Y=Yall[:, sl].clone(), jitter=L.J.clone())],
                        bounds=[(0, Bt)], hyper={k: v.clone() for k, v in hp.items()}, posterior=(Mk, Bk), xq_check=p["xq"],
                        window_lo=L.lo, stream_rows=dict(X=Xall, UH=UHall, Y=Yall, row0=W))
    torch.cuda.synchronize(dev)
    return out


def online_pass_bytes(N, n, m, itemsize):
    """Algorithmic HBM bytes of ONE instance's append (+ control query) pass at N live points: the packed factor
    N(N+1)/2, the whitened targets and inputs N n each, the UH B rows N (1+m) -- read once -- and what the append writes:
    the new factor row (N + 1), one row of Vw / X / UH B."""
    return itemsize * (N * (N + 1) // 2 + 2 * N * n + N * (1 + m) + (N + 1) + 2 * n + (1 + m))


def online_gp_growth(Bt, N0=128, N1=2048, dtype=torch.float64, device="cuda", seed=5, with_control=True, check=True,
                     reserved=True, fused=True, window=None, tail=False):
    """BASELINE configs[4]: every instance starts from an N0-point GP and takes one observation per control step
    until it holds N1 points -- the reference refits from scratch every `train_every_n_steps`
    (unicycle_move_to_pose.py:340-386).  reserved=True (default): capacity-reserving storage (`ops.ReservedGP`,
    capacity N1): an observation enters IN PLACE -- one streaming forward solve + O(N) bytes written, no allocation, no
    copies, no re-packing; the control step's posterior reads the same storage -- fused=True (default): on the SAME pass
    over the factors as the append's forward solve (`append(..., query=x)`; per segment `append_ms` is then that one pass
    + the in-place row writes, `control_step_ms` the solve launch alone).  reserved=False: `ops.gp_append` on the
    packed layout of exactly N points (every per-instance array copied per append, the operator re-packed every 32).
    window = W (reserved storage only): a sliding window over the most recent points (`ops.ReservedGP(window=W)`): the GP
    grows from N0 to W, then every 32nd append drops the oldest 32 points and refits the window (the drop is inside that
    step's `append_ms`); N1 is then the number of observations seen, the final check is against a from-scratch refit of the
    LAST window.
    tail=True (reserved storage, no window; N0 a multiple of 32): the appends since the last commit are contiguous rows beside the
    operator (`bcbf_gp_tail_step`), committed to the column layout 32 rows at a time (`bcbf_gp_tail_commit`: full-line writes) --
    the in-place append's one element per 128-byte line and step is what the next streaming pass waited for.
    Returns per-octave timings (HIP events) and the deviation of the final posterior from a from-scratch refit of all
    N1 points."""
    from .synthetic import make_instances, make_unicycle_task
    dev = torch.device(device)
    n, m = 3, 2
    p = make_instances(Bt, N1, n, m, dtype=dtype, device=dev, seed=seed)
    task = make_unicycle_task(Bt, dtype=dtype, device=dev, seed=seed + 1)
    cut = lambda t, N: t[:, :N].contiguous()
    Lop, UHB, info, _ = ops.refit(cut(p["X"], N0), cut(p["UH"], N0), p["Bm"], p["ell"], p["s2"], cut(p["jitter"], N0))
    assert int((info != 0).sum()) == 0
    Vw, _ = ops.potrs(Lop, cut(p["Xdot"], N0), cut(p["UH"], N0), p["M0"], want_alpha=False)
    X = cut(p["X"], N0)
    A = (0.01 * p["A"]).contiguous()
    ws = ops.control_workspace(Bt, 2, dtype, dev)
    x = task["x"].clone()
    if window is not None:
        assert reserved and N0 <= window, "a sliding window runs on reserved storage, from at most `window` points"
        rgp = ops.ReservedGP(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], window + 32, window=window,
                             UH=cut(p["UH"], N0), Xdot=cut(p["Xdot"], N0), jitter=cut(p["jitter"], N0))
    else:
        rgp = ops.ReservedGP(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], N1, tail=tail) if reserved else None
    if reserved:
        del Lop, Vw, UHB
    # pre-slice the observation stream (contiguous [N1][Bt,.]) so the timed loop holds only the path's own launches
    obs = [t.transpose(0, 1).contiguous() for t in (p["X"], p["UH"], p["Xdot"], p["jitter"])]
    edges = sorted({N0, N1} | {k for k in (256, 512, 1024, 2048) if N0 < k < N1} | ({window} if window and N0 < window < N1 else set()))
    segs = []
    fails = torch.zeros((), dtype=torch.int64, device=dev)
    for lo, hi in zip(edges[:-1], edges[1:]):
        k = hi - lo
        e = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(k)]
        torch.cuda.synchronize()
        for N in range(lo, hi):
            ev = e[N - lo]
            ev[0].record()
            if with_control and reserved and fused:
                # ONE pass over every instance's factor answers the control step's posterior query (on the N points) and the
                # forward solve of the append; (M_k, B_k) are then INPUTS of the fused task-rows / terms / SOCP launch
                info, _, _ = rgp.append(obs[0][N], obs[1][N], obs[2][N], obs[3][N], query=x, out=(ws["Mk"], ws["Bk"]))
                ev[1].record()
                ops.unicycle_control_step(dict(A=A), task, ws, x, dt=0.0, L_mean=4.0, max_iters=20)
                ev[2].record()
                fails += (info != 0).sum()
                continue
            if with_control and reserved:
                rgp.posterior(x, out=(ws["Mk"], ws["Bk"]))
                ops.unicycle_control_step(dict(A=A), task, ws, x, dt=0.0, L_mean=4.0, max_iters=20)
            elif with_control:
                gp = dict(Lop=Lop, Vw=Vw, X=X, UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=A)
                ops.unicycle_control_step(gp, task, ws, x, dt=0.0, L_mean=4.0, max_iters=20)
            ev[1].record()
            if reserved:
                info = rgp.append(obs[0][N], obs[1][N], obs[2][N], obs[3][N])
            else:
                Lop, Vw, X, UHB, info = ops.gp_append(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], obs[0][N],
                                                      obs[1][N], obs[2][N], obs[3][N])
            ev[2].record()
            fails += (info != 0).sum()             # stays on the device: the loop never waits for the host
        torch.cuda.synchronize()
        t_step = sum(ev[0].elapsed_time(ev[1]) for ev in e)
        t_app = sum(ev[1].elapsed_time(ev[2]) for ev in e)
        isz = p["X"].element_size()
        if with_control and reserved and fused:
            t_step, t_app = t_app, t_step              # (events: [0,1] = posterior + append, [1,2] = solve)
        seg = dict(N_from=lo, N_to=hi, control_step_ms=t_step / k, append_ms=t_app / k, step_ms=(t_step + t_app) / k,
                   append_GBs_algorithmic=Bt * isz * ((lo + hi) / 2) ** 2 / 2 / (t_app / k * 1e-3) / 1e9)
        if reserved and window is None:
            # roofline of the pass that dominates an append (+ the control query riding on it): every instance's packed factor,
            # whitened targets, inputs and UH B rows read once (SURVEY 8d's per-instance figure at the live N), summed over the
            # segment's appends; the O(N) bytes an append writes are counted too
            byt = sum(online_pass_bytes(N, n, m, isz) for N in range(lo, hi)) * Bt
            passes = 1 if (with_control and fused) or not with_control else 2
            gbs = byt * passes / (t_app * 1e-3) / 1e9 if passes == 1 else None
            seg["roofline"] = dict(bound="hbm", kernel="posterior_step_kernel<%s, %d, 4, 0, 1, false, 1> (query columns + the append's column on "
                                   "one pass) + %s" % ("double" if isz == 8 else "float", 1 + m,
                                                       "gp_tail_step_kernel (+ gp_tail_commit_kernel every 32nd step)" if tail else "gp_append_rows"),
                                   algorithmic_bytes_per_launch=byt / k, achieved=gbs, peak=8000.0, unit="GB/s",
                                   frac=None if gbs is None else gbs / 8000.0, traffic=None,
                                   how="sum over the segment's appends of Bt x online_pass_bytes(N) / sum of the HIP-event "
                                       "intervals around append(+query) [ms = append_ms]")
        segs.append(seg)
    out = dict(batch=Bt, N0=N0, N1=N1, dtype=str(dtype),
               storage=("reserved (" + ("row-major tail, committed 32 rows at a time" if tail else "in place") + ")"
                        + (", posterior query and append on one pass" if (fused and with_control) else ""))
               if reserved else "packed (copy per append)",
               segments=segs, append_failures=int(fails))
    if window is not None:
        out.update(window=window, drops=rgp.drops, live_points=rgp.N)
    if check:
        if window is not None:                           # the last window: points N1 - live .. N1 - 1 of the stream
            lo = N1 - rgp.N
            p = {k: (v[:, lo:N1].contiguous() if k in ("X", "UH", "Xdot", "jitter") else v) for k, v in p.items()}
        Lr, UHBr, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
        Vr, _ = ops.potrs(Lr, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
        if reserved:
            Mk, Bk = rgp.posterior(p["xq"])
        else:
            Mk, Bk = ops.posterior_step(Lop, Vw, X, UHB, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
        Mr, Br = ops.posterior_step(Lr, Vr, p["X"], UHBr, p["ell"], p["s2"], p["Bm"], p["M0"], p["xq"])
        prior = float((p["s2"][:, None, None] * p["Bm"]).abs().max())
        out["refit_failures"] = int((info != 0).sum())
        out["final_vs_refit"] = dict(Mk=float((Mk - Mr).abs().max() / max(1.0, float(Mr.abs().max()))),
                                     Bk=float((Bk - Br).abs().max() / prior))
    return out


class _PartsReserved:
    """The part batches' `ops.ReservedGP` objects of `learning_closed_loop(parts > 1)` seen as one (what the parity checks read)."""

    def __init__(self, rgps, bounds):
        self.rgps, self.bounds = rgps, bounds

    N = property(lambda self: self.rgps[0].N)
    tail = property(lambda self: self.rgps[0].tail)
    drops = property(lambda self: self.rgps[0].drops)
    drop_failures = property(lambda self: sum(g.drop_failures for g in self.rgps))
    _rJ = property(lambda self: torch.cat([g._rJ for g in self.rgps], 0))

    def posterior(self, xq):
        out = [g.posterior(xq[lo:hi].contiguous()) for g, (lo, hi) in zip(self.rgps, self.bounds)]
        return torch.cat([o[0] for o in out], 0), torch.cat([o[1] for o in out], 0)


def learning_closed_loop(Bt=4096, max_train=512, steps=200, refit_every=40, warmup=40, dtype=torch.float32, device="cuda",
                         seed=1234, schedule="online", n=3, m=2, barrier=None, parts=1, mid_period_steps=0):
    """The reference's REAL workload at BASELINE configs[2] scale: a control loop that keeps learning
    (`LearnedShiftInvariantDynamics.train`, unicycle_move_to_pose.py:340-386: buffer (x, u) every step, refit every
    `train_every_n_steps` = 40 on at most `max_train` points) -- Bt independent instances, each with its own GP over the most
    recent observations, never more than `max_train` of them.

    schedule = "online" (default): every step ONE pass over every instance's factor answers the control step's posterior
        query AND the forward solve of the new observation's in-place append (`ReservedGP.append(query=...)`), then the fused
        task rows / terms / SOCP / plant-step launch; when the model holds `max_train` points the oldest `refit_every` leave
        and the remaining window is refactored from the data (`ReservedGP(window=max_train - refit_every, drop=refit_every)`:
        the live size runs from max_train - refit_every to max_train - 1, so the padded size -- and with it the workgroup
        shape of the streaming kernel -- never exceeds max_train's): the model the controller queries is never more than zero
        steps old.
    schedule = "online_tail": the same schedule with the points observed since the last window refit kept as contiguous ROWS beside
        the window's factor (`ReservedGP(tail=True)`, `bcbf_gp_tail_step`): the streaming pass runs over the static window, a small
        tail kernel finishes the posterior over the newer points and appends the observation as one contiguous row -- no
        element-per-column writes into the operator, whose dirty lines cost the next pass a quarter of its time.
    schedule = "reference": the reference's cadence -- the GP is STATIC between refits (the headline control step,
        `bcbf_unicycle_control_step`: posterior pass + solve), observations only land in a buffer, every `refit_every`-th step
        the last `max_train` buffered points are refactored (`bcbf_refit` + `bcbf_potrs`).  `parts` > 1: the control steps
        run as `ops.ConcurrentControlLoop(parts=...)` (part batches on their own HIP streams, bench.py's default schedule: one
        part's latency-bound solve beside another part's HBM-bound posterior); a refit waits for all part streams (one host
        synchronisation per refit) and the part streams wait for it.

    Observations are PRE-DRAWN synthetic rows (`synthetic.make_instances`: well-conditioned random inputs) -- the cost of the
    learning loop on data that does not depend on the loop; `self_learning_closed_loop` below is the loop that learns from its own
    (x_t, u_t, x_{t+1}).  mid_period_steps: untimed extra steps after the timed region (fewer than refit_every), so that the final
    model the parity checks look at is MID-PERIOD -- a window plus appended / tail rows, not a model that was just refitted.

    `warmup` untimed steps (rounded up to whole refit periods so that the timed region starts right after a refit), then
    `steps` timed steps (a multiple of refit_every: every timed period holds exactly one refit) between two device
    synchronisations.  Returns the timings (wall clock for the total; HIP events for the shares), a roofline entry per
    kernel, and the final state for the parity checks: `final` = dict(rgp | gp tensors, raw window rows, query states)."""
    import time
    from .synthetic import make_instances, make_unicycle_task
    dev = torch.device(device)
    if steps % refit_every or steps <= 0:
        raise ValueError("steps must be a positive multiple of refit_every")
    warmup = -(-warmup // refit_every) * refit_every
    if not 0 <= mid_period_steps < refit_every:
        raise ValueError("mid_period_steps must be in [0, refit_every)")
    total = warmup + steps + int(mid_period_steps)
    window = max_train - refit_every if schedule in ("online", "online_tail") else max_train      # points the model holds right after a refit
    if window < 1:
        raise ValueError("max_train must exceed refit_every")
    p = make_instances(Bt, window + total, n, m, dtype=dtype, device=dev, seed=seed)
    task = make_unicycle_task(Bt, dtype=dtype, device=dev, seed=seed + 99)
    cut = lambda t, N: t[:, :N].contiguous()
    jit0 = cut(p["jitter"], window)
    for attempt in range(4):                                   # make_psd's retry (control_affine_model.py:899-921)
        Lop, UHB, info, _ = ops.refit(cut(p["X"], window), cut(p["UH"], window), p["Bm"], p["ell"], p["s2"], jit0)
        bad = info != 0
        if not bool(bad.any()):
            break
        jit0 = torch.where(bad[:, None], jit0 * 10, jit0).contiguous()
    assert int((info != 0).sum()) == 0, "initial refit failed"
    Vw, _ = ops.potrs(Lop, cut(p["Xdot"], window), cut(p["UH"], window), p["M0"], want_alpha=False)
    isz = p["X"].element_size()
    A = p["A"]
    ws = ops.control_workspace(Bt, 2, dtype, dev)
    x = task["x"].clone()
    dt_plant, L_true, L_mean = 1e-3, 1.0, 4.0
    obs = [t.transpose(0, 1).contiguous() for t in (p["X"], p["UH"], p["Xdot"], p["jitter"])]     # [N][Bt, .]
    fails = torch.zeros((), dtype=torch.int64, device=dev)
    fails_vec = torch.zeros(Bt, dtype=torch.int32, device=dev)
    online = schedule in ("online", "online_tail")
    if online and parts > 1:
        # part batches on their own streams (instances never interact): one part's latency-bound solve and its small tail / row
        # kernels run beside another part's streaming pass, as ops.ConcurrentControlLoop does for the static model; a part's window
        # refit runs on its own stream too (its jitter-retry check waits for that stream only)
        base, rem = divmod(Bt, parts)
        bounds = [(c * base + min(c, rem), (c + 1) * base + min(c + 1, rem)) for c in range(parts)]
        streams = [torch.cuda.Stream(device=dev) for _ in range(parts)]
        cur = torch.cuda.current_stream(dev)
        X0, UH0, Y0 = cut(p["X"], window), cut(p["UH"], window), cut(p["Xdot"], window)
        tkeys = ops.ConcurrentControlLoop.TASK_INSTANCE_KEYS
        rgps, solves = [], []
        for c in range(parts):
            sl = slice(*bounds[c])
            streams[c].wait_stream(cur)
            with torch.cuda.stream(streams[c]):
                rgps.append(ops.ReservedGP(Lop[sl], Vw[sl], X0[sl], UHB[sl], p["ell"][sl], p["s2"][sl], p["Bm"][sl], p["M0"][sl],
                                           window + refit_every, window=window, drop=refit_every, UH=UH0[sl], Xdot=Y0[sl],
                                           jitter=jit0[sl], tail=schedule == "online_tail"))
            taskc = {k: (v[sl] if (torch.is_tensor(v) and k in tkeys) else v) for k, v in task.items()}
            Ac = A[sl] if (A.dim() == 3 and A.shape[0] == Bt and Bt > 1) else A
            solves.append(ops.unicycle_control_step_prepare(dict(A=Ac), taskc, {k: v[sl] for k, v in ws.items()}, x[sl], dt=dt_plant,
                                                            L_true=L_true, L_mean=L_mean, clf_gamma=10.0, max_iters=20,
                                                            stream=streams[c]))
        for s_ in streams:
            s_.synchronize()
        del Lop, Vw, UHB, X0, UH0, Y0
        rgp = _PartsReserved(rgps, bounds)
        # per-part views, made once (the loop's host side is what bounds three and four part batches)
        obs_c = [[o[:, slice(*bounds[c])] for o in obs] for c in range(parts)]
        x_c = [x[slice(*bounds[c])] for c in range(parts)]
        out_c = [(ws["Mk"][slice(*bounds[c])], ws["Bk"][slice(*bounds[c])]) for c in range(parts)]
        fails_c = [fails_vec[slice(*bounds[c])] for c in range(parts)]
    elif online:
        rgp = ops.ReservedGP(Lop, Vw, cut(p["X"], window), UHB, p["ell"], p["s2"], p["Bm"], p["M0"], window + refit_every,
                             window=window, drop=refit_every, UH=cut(p["UH"], window), Xdot=cut(p["Xdot"], window), jitter=jit0,
                             tail=schedule == "online_tail")
        del Lop, Vw, UHB
        solve = ops.unicycle_control_step_prepare(dict(A=A), task, ws, x, dt=dt_plant, L_true=L_true, L_mean=L_mean,
                                                  clf_gamma=10.0, max_iters=20)
    elif schedule == "reference":
        gp = dict(Lop=Lop, Vw=Vw, X=cut(p["X"], window), UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=A)
        jit_w = jit0
        lo = 0
        if parts > 1:
            loop = ops.ConcurrentControlLoop(gp, task, x, parts=parts, dt=dt_plant, L_true=L_true, L_mean=L_mean, clf_gamma=10.0,
                                             max_iters=20)
            ws = loop.ws
        else:
            step_fn = ops.unicycle_control_step_prepare(gp, task, ws, x, dt=dt_plant, L_true=L_true, L_mean=L_mean,
                                                        clf_gamma=10.0, max_iters=20)
    else:
        raise ValueError("schedule: 'online', 'online_tail' or 'reference'")
    E = lambda: torch.cuda.Event(enable_timing=True)
    ev = [[E(), E(), E(), E()] for _ in range(total)]          # step start / pass end / solve end / (refit end)
    for row in ev:                                             # (torch creates the hipEvent handle at the first record; the
        for e_ in row:                                         #  reference schedule hands raw handles to the C entry point)
            e_.record()
    concurrent = parts > 1
    evp = None
    if concurrent:                                             # per part: events around its posterior launch, on its stream
        if not online:
            streams = loop.streams
        evp = [[(E(), E()) for _ in range(parts)] for _ in range(total)]
        for row in evp:
            for c, (a_, b_) in enumerate(row):
                a_.record(streams[c]); b_.record(streams[c])
        ev_base = E()
    refit_steps = []
    t0 = elapsed = None
    for t in range(total):
        if t == warmup:
            if barrier is not None:
                barrier()
            torch.cuda.synchronize(dev)
            if concurrent:
                for s_ in streams:
                    s_.synchronize()
                ev_base.record(streams[0])
            t0 = time.perf_counter()
        if t == warmup + steps:                                  # (mid_period_steps > 0: the timed region ends here)
            torch.cuda.synchronize(dev)
            if barrier is not None:
                barrier()
            elapsed = time.perf_counter() - t0
        N_obs = window + t
        e = ev[t]
        e[0].record()
        if online and concurrent:
            drops_before = rgp.drops
            for c in range(parts):
                oc = obs_c[c]
                with torch.cuda.stream(streams[c]):
                    evp[t][c][0].record(streams[c])
                    info, _, _ = rgps[c].append(oc[0][N_obs], oc[1][N_obs], oc[2][N_obs], oc[3][N_obs], query=x_c[c], out=out_c[c])
                    evp[t][c][1].record(streams[c])
                    solves[c]()
                    fails_c[c] += info != 0
            if rgp.drops != drops_before:
                refit_steps.append(t)
        elif online:
            drops_before = rgp.drops
            info, _, _ = rgp.append(obs[0][N_obs], obs[1][N_obs], obs[2][N_obs], obs[3][N_obs], query=x, out=(ws["Mk"], ws["Bk"]))
            # (the window's drop + refit, when this append filled it, ran inside append -- timed below as its own share)
            e[1].record()
            solve()
            e[2].record()
            fails_vec += info != 0                       # (stays on the device: the loop never waits for the host)
            if rgp.drops != drops_before:
                refit_steps.append(t)
        else:
            if concurrent:
                loop.step(evp[t])
            else:
                step_fn(e[0], e[1])                              # (events around the posterior launch, on its stream)
                e[2].record()
            if (t + 1) % refit_every == 0:
                if concurrent:
                    loop.synchronize()                           # the refit overwrites what the part streams read
                    e[2].record()
                lo = t + 1
                sl = slice(lo, lo + window)
                Xw, UHw, Yw = (p[k][:, sl].contiguous() for k in ("X", "UH", "Xdot"))
                jit_w = p["jitter"][:, sl].contiguous()
                for attempt in range(4):
                    ops.refit(Xw, UHw, p["Bm"], p["ell"], p["s2"], jit_w, out=(gp["Lop"], gp["UHB"], info))
                    bad = info != 0
                    if not bool(bad.any()):
                        break
                    jit_w = torch.where(bad[:, None], jit_w * 10, jit_w).contiguous()
                ops.potrs(gp["Lop"], Yw, UHw, p["M0"], want_alpha=False, out_Vw=gp["Vw"])
                gp["X"].copy_(Xw)
                fails += (info != 0).sum()
                e[3].record()
                if concurrent:
                    for st_ in loop.streams:
                        st_.wait_stream(torch.cuda.current_stream(dev))
                refit_steps.append(t)
    torch.cuda.synchronize(dev)
    if elapsed is None:
        if barrier is not None:
            barrier()
        elapsed = time.perf_counter() - t0
    timed = range(warmup, warmup + steps)
    if online and concurrent:
        # the parts drift apart, so shares are taken over the whole timed region: the time during which at least one part's pass
        # (on a refit step: pass + window refit) ran, and a refit's own share from each part's refit-step interval minus that part's
        # mean plain interval
        spans = sorted((ev_base.elapsed_time(a_), ev_base.elapsed_time(b_)) for t in timed for a_, b_ in evp[t])
        busy, ca, cb = 0.0, spans[0][0], spans[0][1]
        for a_, b_ in spans[1:]:
            if a_ > cb:
                busy += cb - ca
                ca, cb = a_, b_
            else:
                cb = max(cb, b_)
        busy += cb - ca
        tr = set(refit_steps)
        dur = lambda t, c: evp[t][c][0].elapsed_time(evp[t][c][1])
        plain_c = [sum(dur(t, c) for t in timed if t not in tr) / max(1, sum(1 for t in timed if t not in tr)) for c in range(parts)]
        rs = [t for t in timed if t in tr]
        n_refits = len(rs)
        refit_ms = (sum(dur(t, c) - plain_c[c] for t in rs for c in range(parts)) / (n_refits * parts)) if rs else 0.0
        pass_ms = busy / steps - refit_ms * n_refits / steps / parts      # (a part's refit occupies the device for ~1/parts of the batch)
    elif online:
        # the append (+ the drop/refit on refit steps) sits between e[0] and e[1]; a refit step's own share = its interval minus
        # the mean interval of the other steps at a comparable N
        tr = set(refit_steps)
        plain = [ev[t][0].elapsed_time(ev[t][1]) for t in timed if t not in tr]
        withr = [ev[t][0].elapsed_time(ev[t][1]) for t in timed if t in tr]
        pass_ms = sum(plain) / max(1, len(plain))
        refit_ms = (sum(withr) / max(1, len(withr)) - pass_ms) if withr else 0.0
        n_refits = len(withr)
    elif concurrent:
        # the part batches' posterior launches overlap one another: the time during which at least one of them ran (bench.py)
        spans = sorted((ev_base.elapsed_time(a_), ev_base.elapsed_time(b_)) for t in timed for a_, b_ in evp[t])
        busy, ca, cb = 0.0, spans[0][0], spans[0][1]
        for a_, b_ in spans[1:]:
            if a_ > cb:
                busy += cb - ca
                ca, cb = a_, b_
            else:
                cb = max(cb, b_)
        pass_ms = (busy + cb - ca) / steps
        rs = [t for t in refit_steps if warmup <= t < warmup + steps]
        refit_ms = sum(ev[t][2].elapsed_time(ev[t][3]) for t in rs) / max(1, len(rs))
        n_refits = len(rs)
    else:
        pass_ms = sum(ev[t][0].elapsed_time(ev[t][1]) for t in timed) / steps
        rs = [t for t in refit_steps if warmup <= t < warmup + steps]
        refit_ms = sum(ev[t][2].elapsed_time(ev[t][3]) for t in rs) / max(1, len(rs))
        n_refits = len(rs)
    if os.environ.get("BCBF_LEARN_DUMP"):          # development: per-step pass / solve intervals with the live size
        import json as _json
        _json.dump([dict(t=t, N=(window + (t % refit_every)) if online else window, pass_ms=ev[t][0].elapsed_time(ev[t][1]),
                         solve_ms=ev[t][1].elapsed_time(ev[t][2])) for t in timed], open(os.environ["BCBF_LEARN_DUMP"], "w"))
    solve_ms = 0.0 if concurrent else sum(ev[t][1].elapsed_time(ev[t][2]) for t in timed) / steps     # (concurrent: hidden beside the passes)
    ms_step = elapsed / steps * 1e3
    # roofline entries.  pass: every instance's packed factor + whitened targets + inputs + UH B rows read once at the live N
    if online:
        live = [window + (t % refit_every) for t in timed if t not in set(refit_steps)]
        pass_bytes = sum(online_pass_bytes(N, n, m, isz) for N in live) / max(1, len(live)) * Bt
        pass_kernel = "posterior_step_kernel<%s, %d, 4, 0, 1, false, 1> + %s" % ("float" if isz == 4 else "double", 1 + m,
                                                                                   "gp_tail_step_kernel" if rgp.tail else "gp_append_inplace_kernel")
    else:
        pass_bytes = isz * (window * (window + 1) // 2 + 2 * window * n + window * (1 + m)) * Bt
        pass_kernel = "posterior_step_kernel<%s, %d, 4, 0, 1, false, 0>" % ("float" if isz == 4 else "double", 1 + m)
    peak_t = 157.3 if isz == 4 else 78.6
    refit_flops = (Bt / parts if (online and concurrent) else Bt) * window ** 3 / 3.0     # (online on part batches: a refit is one part's)
    roof = {"pass": dict(bound="hbm", kernel=pass_kernel, algorithmic_bytes_per_launch=pass_bytes,
                         achieved=pass_bytes / (pass_ms * 1e-3) / 1e9, peak=8000.0, unit="GB/s",
                         frac=pass_bytes / (pass_ms * 1e-3) / 1e9 / 8000.0, kernel_ms=pass_ms, traffic=None),
            "refit": dict(bound="mfma", kernel="refit_wave_kernel<%s, ...> (+ bcbf_potrs%s)" % ("float" if isz == 4 else "double",
                                                                                                ", row moves, bcbf_gp_reserve" if online else ""),
                          algorithmic_flops_per_launch=refit_flops, achieved=refit_flops / (refit_ms * 1e-3) / 1e12 if refit_ms > 0 else None,
                          peak=peak_t, unit="TFLOP/s", frac=refit_flops / (refit_ms * 1e-3) / 1e12 / peak_t if refit_ms > 0 else None,
                          kernel_ms=refit_ms, traffic=None,
                          note="over the WHOLE refit share of a refit step (every launch of it), a lower bound on the kernel's own rate")}
    out = dict(schedule=schedule, batch=Bt, max_train=max_train, points_after_refit=window, steps=steps, warmup=warmup, refit_every=refit_every, dtype=str(dtype),
               seconds=elapsed, ms_per_step=ms_step, instance_steps_per_s=Bt * steps / elapsed,
               shares=dict(pass_ms_per_step=pass_ms, solve_ms_per_step=solve_ms, refit_ms_per_refit=refit_ms,
                           refit_ms_per_step=refit_ms * n_refits / steps, refits_in_timed_region=n_refits,
                           other_ms_per_step=ms_step - pass_ms - solve_ms - refit_ms * n_refits / steps),
               roofline=roof, append_or_refit_failures=int(fails) + int((fails_vec != 0).sum()), parts=parts, solver_optimal_fraction=float((ws["status"] == 0).float().mean()))
    if online:
        out["drop_failures"] = rgp.drop_failures
        lo = window + total - rgp.N
        final = dict(rgp=rgp, lo=lo, N=rgp.N, jitter=rgp._rJ[:, :rgp.N])
    else:
        final = dict(gp=gp, lo=lo, N=window, jitter=jit_w)
    final.update(p=p, x=x, ws=ws)
    return out, final


def final_window_vs_device_refit(final, sample=64):
    """Self-check of a learning loop's final model (any dtype) against a from-scratch fp64 refit ON THE DEVICE of the same
    window rows with the jitter every point ended up with: max deviation of the posterior at the instances' query points over
    `sample` instances spread over the batch, relative to max(1, |M_k|) and to the prior scale.  (The parity check against
    the CPU oracle lives in tests/.)"""
    p, lo, N = final["p"], final["lo"], final["N"]
    Bt = p["X"].shape[0]
    idx = torch.linspace(0, Bt - 1, min(sample, Bt), device=p["X"].device).long()
    f64 = lambda t: t.double().contiguous()
    sel = lambda k: f64(p[k][idx, lo:lo + N])
    hp = {k: f64(p[k][idx]) for k in ("Bm", "ell", "s2", "M0", "xq")}
    Lr, UHBr, info, _ = ops.refit(sel("X"), sel("UH"), hp["Bm"], hp["ell"], hp["s2"], f64(final["jitter"][idx]))
    Vr, _ = ops.potrs(Lr, sel("Xdot"), sel("UH"), hp["M0"], want_alpha=False)
    Mr, Br = ops.posterior_step(Lr, Vr, sel("X"), UHBr, hp["ell"], hp["s2"], hp["Bm"], hp["M0"], hp["xq"])
    if "rgp" in final:
        Mk, Bk = final["rgp"].posterior(p["xq"])
    else:
        g = final["gp"]
        Mk, Bk = ops.posterior_step(g["Lop"], g["Vw"], g["X"], g["UHB"], g["ell"], g["s2"], g["Bm"], g["M0"], p["xq"])
    prior = (hp["s2"][:, None, None] * hp["Bm"]).abs().amax(dim=(1, 2))
    return dict(instances=int(idx.numel()), refit_failures=int((info != 0).sum()),
                Mk=float(((f64(Mk[idx]) - Mr).abs().amax(dim=(1, 2)) / Mr.abs().amax(dim=(1, 2)).clamp(min=1.0)).max()),
                Bk=float(((f64(Bk[idx]) - Br).abs().amax(dim=(1, 2)) / prior).max()))


def subsample_pool(window, own_rows, max_train):
    """Which stream rows a refit of `self_learning_closed_loop(subsample="random")` learns from, when the instance has made
    `own_rows` observations (stream rows window .. window + own_rows - 1; rows 0 .. window-1 are the synthetic start).
    Returns (lo, P, random): up to max_train own rows, the last `window` rows [lo, lo + P) themselves (synthetic start rows
    included, as subsample="window"); beyond, the reference's `XdotTrain.shape[0] > max_train` branch
    (unicycle_move_to_pose.py:377-384): a random max_train-subset of ALL own rows, the pool [window, window + own_rows)."""
    if own_rows <= max_train:
        return own_rows, window, False
    return window, own_rows, True


def self_learning_closed_loop(Bt=4096, max_train=512, steps=200, refit_every=40, warmup=None, dtype=torch.float32, device="cuda",
                              seed=1234, schedule="reference", parts=4, stagger=True, shift_invariant=True, dt=0.01,
                              retry_levels=3, fit_iters=0, fit_lr=0.1, fit_dtype=torch.float64, record_states=False, barrier=None,
                              mid_period_steps=0, query_shift_invariant=True, level_decay_every=4, factor_dtype=None,
                              min_jitter_level=1e-5, subsample="window"):
    """The reference's learning loop for MANY instances, fed BY ITSELF (LearnedShiftInvariantDynamics.train / fit,
    unicycle_move_to_pose.py:326-386): every control step's observation row is built on the device from the loop's own
    (x_t, u_t, x_{t+1}) -- inside the solve / plant launch (`bcbf_unicycle_control_step_observe`): regressor input = the state
    before the step, shift invariant (0, 0, theta) (:326-330), target = (x_{t+1} - x_t) / dt minus the mean model
    `AckermannDrive(L_mean)` (:364-372) -- and is what the next refit / append learns from.  query_shift_invariant (default):
    the controller queries the learned model at the shift-invariant input of the current state too, which the kernel keeps in
    `xq` (xq_next).  The reference's `fu_func_gp` (:388-397) does NOT go through the wrapper -- its controller queries a model
    trained on (0, 0, theta) at the raw (x, y, theta), far from every training input, so the posterior is the prior and most
    chance constraints are infeasible (measured here: 13 % of the programs solve, against 87 % with consistent inputs);
    query_shift_invariant=False reproduces that.
    Jitter (make_psd, :899-921): every factorisation draws level * rand per point, x10 per failed attempt; an instance starts a
    refit at the level that last worked and goes one level down every `level_decay_every`-th refit (the reference restarts at
    1e-5 every time; in fp32 on a trajectory's near-collinear rows that level fails for three instances in four, each failure
    a whole factorisation).

    Bt instances in `parts` part batches, each on its own HIP stream with its own model buffers; NOTHING waits for the host:
    a refit is `bcbf_refit` + `retry_levels` unconditional `bcbf_refit_retry` launches (make_psd's x10 schedule on the failed
    instances) + `bcbf_potrs` into the operator buffer that is not being read, then the buffers swap.  `stagger`: part c refits
    at steps = c * refit_every / parts (mod refit_every), so one part's matrix-core refit runs beside the other parts' HBM-bound
    passes instead of stopping the device.
      schedule "reference":   the model is static between refits (posterior pass + solve); every `refit_every` steps the last
                              `max_train` observations are refactored -- the reference's cadence (train_every_n_steps).
      schedule "online_tail": every observation enters the model the step after it was made (`ReservedGP(tail=True)`:
                              streaming pass over the window + tail kernel), window refit every `refit_every` appends.
    The windows start filled with synthetic rows (the model the run starts from); `warmup` (default: enough periods to flush
    them, >= window + refit_every steps) makes the timed region learn from the loop's own rows only.
    fit_iters > 0 (schedule "reference"): every refit first runs `fit_iters` Adam iterations of the marginal likelihood on the
    part's window for every instance (`BatchedHyperFit`, in `fit_dtype`) -- the reference's `fit(..., training_iter=100)`;
    the hyper-parameters the control path reads are updated in place.
    mid_period_steps: untimed extra steps after the timed region, so that the final model is mid-period (tail / window not
    just refitted) for the parity checks.
    factor_dtype = torch.float64 with dtype = torch.float32 (schedule "reference"): MIXED precision -- the window is factored in
    fp64 (`bcbf_refit` + `bcbf_potrs` on the rows cast up: cond(K_b) ~ N s2 / jitter is beyond fp32 on a trajectory's rows, the
    fp64 factorisation succeeds at make_psd's base level with no retry) and the operator, `UH B`, `Vw` are ROUNDED to fp32 for
    the streaming passes, which are HBM bound and move half the bytes.  The error the passes then add is cond(L) eps32 =
    sqrt(cond K_b) eps32 ~ 1e-4, not cond(K_b) eps32: the loop runs at fp32's pass rate with models that agree with the fp64
    refit of their rows to ~1e-3 (reported: final_vs_fp64_refit_on_device).
    min_jitter_level (default make_psd's 1e-5): the floor of every instance's jitter level.  fp32 PASSES cannot resolve a posterior
    variance below ~sqrt(cond K_b) eps32 of the prior: with fp64 factors at the 1e-5 level B_k = s2 B - W'W is rounding noise (it
    goes indefinite and the cone conversion refuses the program); 1e-3 keeps it resolvable.

    subsample (schedule "reference"): which rows a refit learns from.
      "window" (default): the last `max_train` observations, a sliding window (the figures in DESIGN 3.4 are this mode's).
      "random": the reference's training set (LearnedShiftInvariantDynamics.fit, unicycle_move_to_pose.py:377-384): while an
                instance has made at most max_train observations, the window as above; beyond, a FRESH random max_train-subset
                of all its own observations at every refit (`subsample_pool`) -- keys rand(Bt_c, P) from the loop's generator,
                `bcbf_subsample_rows` sorts them and gathers the chosen rows into per-part subset buffers on the device (no host
                round trip), which the refit (and the fit) reads.  The draws come from the loop's torch generator, not from
                numpy's global RNG: the distribution of the subset is the reference's, the sample is not.  The pool holds at
                most warmup + steps + mid_period_steps rows, which the kernel limits to 8192.

    Returns (report, final): final = dict(rows = the raw observation rows each instance's model holds, oldest first
    (X, UH, Y, jitter [Bt, N, .]; subsample="random": in subset order, with `subset_index` [Bt, N] int32 = their stream rows),
    posterior = (Mk, Bk) of the final model at `xq_check`, xq_check, hyper-parameters; states
    (record_states): the visited (x_t, u_t) of every step)."""
    import time
    from .synthetic import make_instances, make_unicycle_task
    dev = torch.device(device)
    n, m = 3, 2
    if schedule not in ("reference", "online_tail"):
        raise ValueError("schedule: 'reference' or 'online_tail'")
    if steps % refit_every or steps <= 0:
        raise ValueError("steps must be a positive multiple of refit_every")
    if fit_iters and schedule != "reference":
        raise ValueError("fit_iters: the hyper-parameter fit rides on the reference schedule's refits")
    if subsample not in ("window", "random"):
        raise ValueError("subsample: 'window' or 'random'")
    if subsample == "random" and schedule != "reference":
        raise ValueError("subsample='random' needs schedule='reference' (a bordered factor cannot drop rows)")
    randsub = subsample == "random"
    online = schedule == "online_tail"
    window = max_train - refit_every if online else max_train
    if window < 1:
        raise ValueError("max_train must exceed refit_every")
    if warmup is None:
        warmup = window + refit_every
    warmup = -(-warmup // refit_every) * refit_every
    total = warmup + steps + int(mid_period_steps)
    Ntot = window + total + 1
    if randsub and total > ops.SUBSAMPLE_MAX_POOL:
        raise ValueError("subsample='random': a refit's pool (up to warmup + steps + mid_period_steps = %d rows) exceeds the "
                         "kernel's %d" % (total, ops.SUBSAMPLE_MAX_POOL))
    p = make_instances(Bt, window, n, m, dtype=dtype, device=dev, seed=seed, variant="theta" if shift_invariant else "dense")
    task = make_unicycle_task(Bt, dtype=dtype, device=dev, seed=seed + 99)
    f = dict(dtype=dtype, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed + 7)
    # the observation stream of every instance: rows 0 .. window-1 = the synthetic start, row window + t = step t's observation
    Xall, UHall, Yall = torch.zeros(Bt, Ntot, n, **f), torch.zeros(Bt, Ntot, 1 + m, **f), torch.zeros(Bt, Ntot, n, **f)
    # make_psd's draws (:907-910): reference schedule -- the jitter every row was last factored with (filled in per refit); online --
    # one rand per step, scaled by the instance's level when the point enters
    Jall = torch.rand(Bt, Ntot, generator=gen, **f).contiguous()
    Jall[:, :window] = p["jitter"]
    Xall[:, :window], UHall[:, :window], Yall[:, :window] = p["X"], p["UH"], p["Xdot"]
    x = task["x"].clone()
    # the planner's target moves along the straight line start -> goal at constant speed and reaches the goal when the run ends
    # (PiecewiseLinearPlanner, planner.py:54-64); the solve / plant launch advances it (flags bit 1)
    task["dot_plan"] = ((task["xg"] - task["x"]) / (total * dt)).contiguous()
    task["plan"] = (task["x"] + 20 * dt * task["dot_plan"]).contiguous()        # (a look-ahead: at the state itself the CLF's polar terms are singular)
    L_true, L_mean = 1.0, 4.0
    base, rem = divmod(Bt, parts)
    bounds = [(c * base + min(c, rem), (c + 1) * base + min(c + 1, rem)) for c in range(parts)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(parts)]
    cur = torch.cuda.current_stream(dev)
    ws = ops.control_workspace(Bt, 2, dtype, dev)
    rnd = lambda *shape: torch.rand(*shape, generator=gen, **f)
    tkeys = ops.ConcurrentControlLoop.TASK_INSTANCE_KEYS
    offsets = [(c * refit_every) // parts if stagger else 0 for c in range(parts)]
    hyper = {k: p[k] for k in ("ell", "s2", "Bm", "M0", "A")}                       # updated in place by the fit
    xs_log, us_log = ([], []) if record_states else (None, None)

    class Part:
        pass
    P = []
    for c in range(parts):
        lo, hi = bounds[c]
        sl = slice(lo, hi)
        pt = Part()
        pt.sl, pt.Bt = sl, hi - lo
        pt.X, pt.UH, pt.Y, pt.J = Xall[sl], UHall[sl], Yall[sl], Jall[sl]             # contiguous [Bt_c, Ntot, .] views
        pt.hp = {k: v[sl] for k, v in hyper.items()}
        pt.x = x[sl]
        pt.n_refits = 0
        # the learned model's query: the shift-invariant input of the current state, kept by the solve / plant launch (xq_next)
        pt.xq = None
        if query_shift_invariant and shift_invariant:
            pt.xq = pt.x.clone()
            pt.xq[:, :2] = 0
        obs_kw = dict(xq=pt.xq, xq_next=pt.xq, shift_invariant=shift_invariant, advance_plan=True)
        taskc = {k: (v[sl] if (torch.is_tensor(v) and k in tkeys) else v) for k, v in task.items()}
        wsc = {k: v[sl] for k, v in ws.items()}
        pt.ws = wsc
        streams[c].wait_stream(cur)
        with torch.cuda.stream(streams[c]):
            cutw = lambda t_: t_[:, :window].contiguous()
            Xw, UHw, Yw, Jw = cutw(pt.X), cutw(pt.UH), cutw(pt.Y), cutw(pt.J)
            E = ops.lop_elems(window, dtype)
            mk = lambda: dict(Lop=torch.empty(pt.Bt, E, **f), UHB=torch.empty(pt.Bt, window, 1 + m, **f), Vw=torch.empty(pt.Bt, window, n, **f),
                              X=torch.empty(pt.Bt, window, n, **f))
            pt.info, pt.info2 = torch.zeros(pt.Bt, dtype=torch.int32, device=dev), torch.zeros(pt.Bt, dtype=torch.int32, device=dev)
            pt.fail_count = torch.zeros((), dtype=torch.int64, device=dev)
            pt.level = torch.full((pt.Bt,), float(min_jitter_level), **f)     # make_psd's level per instance (x10 per failed attempt)
            pt.retry_counts = torch.zeros(retry_levels + 1, dtype=torch.int64, device=dev)

            mixed = factor_dtype is not None and factor_dtype != dtype
            if mixed:
                fw = dict(dtype=factor_dtype, device=dev)
                pt.wide = dict(Lop=torch.empty(pt.Bt, ops.lop_elems(window, factor_dtype), **fw), UHB=torch.empty(pt.Bt, window, 1 + m, **fw),
                               Vw=torch.empty(pt.Bt, window, n, **fw))

            def factor_into(buf, Xw, UHw, Yw, Jw, pt=pt, mixed=mixed):
                if mixed:
                    # factor in the wide precision, round the results into the buffers the passes read (the packed layout is the
                    # same element for element in both precisions: a cast, no re-layout)
                    up = lambda t_: t_.to(factor_dtype)
                    hpw = {k: up(v) for k, v in pt.hp.items()}
                    Xd, UHd, Yd, Jd = up(Xw), up(UHw), up(Yw), up(Jw)
                    w = pt.wide
                    ops.refit_with_retries(Xd, UHd, hpw["Bm"], hpw["ell"], hpw["s2"], Jd, (w["Lop"], w["UHB"], pt.info),
                                           levels=retry_levels, scratch=pt.info2, level=pt.level, counts=pt.retry_counts)
                    ops.potrs(w["Lop"], Yd, UHd, hpw["M0"], want_alpha=False, out_Vw=w["Vw"])
                    buf["Lop"].copy_(w["Lop"]); buf["UHB"].copy_(w["UHB"]); buf["Vw"].copy_(w["Vw"])
                    Jw.copy_(Jd)
                else:
                    ops.refit_with_retries(Xw, UHw, pt.hp["Bm"], pt.hp["ell"], pt.hp["s2"], Jw, (buf["Lop"], buf["UHB"], pt.info),
                                           levels=retry_levels, scratch=pt.info2, level=pt.level, counts=pt.retry_counts)
                    ops.potrs(buf["Lop"], Yw, UHw, pt.hp["M0"], want_alpha=False, out_Vw=buf["Vw"])
                buf["X"].copy_(Xw)
                pt.fail_count += (pt.info != 0).sum()
            pt.factor_into = factor_into
            if online:
                b0 = mk()
                factor_into(b0, Xw, UHw, Yw, Jw)
                # stagger: part c starts `offset` rows into its period (N_init = window + offset): its drops come that much earlier
                pt.rgp = ops.ReservedGP(b0["Lop"], b0["Vw"], Xw, b0["UHB"], pt.hp["ell"], pt.hp["s2"], pt.hp["Bm"], pt.hp["M0"],
                                        window + refit_every, window=window, drop=refit_every, UH=UHw, Xdot=Yw, jitter=Jw, tail=True,
                                        retry_levels=retry_levels, factor_dtype=factor_dtype, min_jitter_level=min_jitter_level)
                pt.rgp.level_decay_every = level_decay_every
                pt.obs = [tuple(torch.zeros(pt.Bt, 3, **f) for _ in range(3)) for _ in range(2)]
                pt.solve = ops.unicycle_control_step_prepare(dict(A=pt.hp["A"]), taskc, wsc, pt.x, dt=dt, L_true=L_true, L_mean=L_mean,
                                                             clf_gamma=10.0, max_iters=20, stream=streams[c],
                                                             observe=obs_kw)
            else:
                pt.bufs = [mk(), mk()]
                factor_into(pt.bufs[0], Xw, UHw, Yw, Jw)
                pt.cur = 0
                pt.step = [ops.unicycle_control_step_prepare(dict(b_, **pt.hp), taskc, wsc, pt.x, dt=dt, L_true=L_true, L_mean=L_mean,
                                                             clf_gamma=10.0, max_iters=20, stream=streams[c],
                                                             observe=obs_kw)
                           for b_ in pt.bufs]
                pt.lo = 0
                pt.pool_rows = window
                if randsub:
                    # the rows the current model was factored from, in subset order, with their jitter (pt.J stays per stream row)
                    pt.sX, pt.sUH, pt.sY, pt.sJ = Xw, UHw, Yw, Jw
                    pt.sidx = torch.arange(window, dtype=torch.int32, device=dev).expand(pt.Bt, window).contiguous()
                if fit_iters:
                    from .batched_fit import BatchedHyperFit
                    pt.bf = BatchedHyperFit.from_values(pt.hp["A"], pt.hp["Bm"], pt.hp["ell"], pt.hp["s2"], pt.hp["M0"], dtype=fit_dtype)
        P.append(pt)
    for s_ in streams:
        s_.synchronize()
    if online:
        # bootstrap: the first append needs an observation -- one control step on the start model (posterior, solve + observe)
        for c, pt in enumerate(P):
            with torch.cuda.stream(streams[c]):
                pt.q = pt.xq if pt.xq is not None else pt.x
                pt.rgp.posterior(pt.q, out=(pt.ws["Mk"], pt.ws["Bk"]))
                pt.solve(obs=(*pt.obs[0], 1))
                # stagger the parts' drops: part c enters `offset` more observations before the loop (untimed)
                for k in range(offsets[c]):
                    o = pt.obs[k % 2]
                    pt.rgp.append(o[0], o[1], o[2], pt.rgp.jitter_level * pt.J[:, window + total - 1 - k], query=pt.q, out=(pt.ws["Mk"], pt.ws["Bk"]))
                    pt.solve(obs=(*pt.obs[(k + 1) % 2], 1))
                pt.k0 = offsets[c]
        for s_ in streams:
            s_.synchronize()
    E_ = lambda: torch.cuda.Event(enable_timing=True)
    evp = [[(E_(), E_()) for _ in range(parts)] for _ in range(total)]
    evr = {}
    for row in evp:
        for c, (a_, b_) in enumerate(row):
            a_.record(streams[c]); b_.record(streams[c])
    ev_base = E_()
    refit_log = []

    def do_refit(c, pt, t):
        """Part c, after step t: refactor the last `window` observations (subsample="random": the rows `subsample_pool` picks)
        into the buffer that is not being read; swap."""
        lo = t + 1
        if randsub:
            lo, pt.pool_rows, drawn = subsample_pool(window, t + 1, max_train)
        cutw = lambda t_: t_[:, lo:lo + window].contiguous()
        if not randsub:
            Xw, UHw, Yw = cutw(pt.X), cutw(pt.UH), cutw(pt.Y)
        # a fresh jitter draw per factorisation, at the instance's level: one below the one that last worked (make_psd, :903-919)
        pt.n_refits += 1
        if level_decay_every and pt.n_refits % level_decay_every == 0:
            pt.level.div_(10).clamp_(min=float(min_jitter_level))
        Jw = (pt.level[:, None] * rnd(pt.Bt, window)).contiguous()
        if randsub:
            if drawn:
                keys = torch.rand(pt.Bt, pt.pool_rows, generator=gen, dtype=torch.float32, device=dev)
                ops.subsample_rows(keys, pt.X, pt.UH, pt.Y, window, lo=lo, P=pt.pool_rows, out=(pt.sX, pt.sUH, pt.sY, pt.sidx))
            else:
                pt.sX.copy_(pt.X[:, lo:lo + window]); pt.sUH.copy_(pt.UH[:, lo:lo + window]); pt.sY.copy_(pt.Y[:, lo:lo + window])
                pt.sidx.copy_(torch.arange(lo, lo + window, dtype=torch.int32, device=dev).expand(pt.Bt, window))
            pt.sJ.copy_(Jw)
            Xw, UHw, Yw, Jw = pt.sX, pt.sUH, pt.sY, pt.sJ
        if fit_iters:
            wd = fit_dtype
            pt.bf.fit(Xw.to(wd), UHw[:, :, 1:].to(wd).contiguous(), Yw.to(wd), training_iter=fit_iters, lr=fit_lr)
            hp = pt.bf.derive()
            for k in ("ell", "s2", "Bm", "M0", "A"):
                pt.hp[k].copy_(hp[k].to(dtype))
        nxt = 1 - pt.cur
        pt.factor_into(pt.bufs[nxt], Xw, UHw, Yw, Jw)
        if not randsub:
            pt.J[:, lo:lo + window] = Jw                              # the level every point was finally factored with
        pt.cur, pt.lo = nxt, lo

    t0 = None
    for t in range(total):
        if t == warmup:
            if barrier is not None:
                barrier()
            torch.cuda.synchronize(dev)
            ev_base.record(streams[0])
            t0 = time.perf_counter()
        if t == warmup + steps:
            torch.cuda.synchronize(dev)
            if barrier is not None:
                barrier()
            elapsed = time.perf_counter() - t0
        if record_states:
            torch.cuda.synchronize(dev)
            xs_log.append(x.clone())
        for c, pt in enumerate(P):
            row = window + t
            if online:
                with torch.cuda.stream(streams[c]):
                    k = pt.k0 + t
                    o_prev, o_next = pt.obs[k % 2], pt.obs[(k + 1) % 2]
                    drops_before = pt.rgp.drops
                    evp[t][c][0].record(streams[c])
                    jit = pt.rgp.jitter_level * pt.J[:, row]                  # (J holds rand draws here: the new point's jitter at the instance's level)
                    pt.rgp.append(o_prev[0], o_prev[1], o_prev[2], jit, query=pt.q, out=(pt.ws["Mk"], pt.ws["Bk"]))
                    evp[t][c][1].record(streams[c])
                    pt.solve(obs=(*o_next, 1))
                    if pt.rgp.drops != drops_before:
                        refit_log.append((t, c))
            else:
                pt.step[pt.cur](evp[t][c][0], evp[t][c][1], obs=(pt.X[:, row], pt.UH[:, row], pt.Y[:, row], Ntot))
                if (t + 1 - offsets[c]) % refit_every == 0 and t + 1 >= refit_every:
                    with torch.cuda.stream(streams[c]):
                        a_, b_ = E_(), E_()
                        a_.record(streams[c])
                        do_refit(c, pt, t)
                        b_.record(streams[c])
                        evr[(t, c)] = (a_, b_)
                    refit_log.append((t, c))
        if record_states:
            torch.cuda.synchronize(dev)
            # the control that was APPLIED: the program's solution, or zero for an instance whose program was not solved (frozen)
            us_log.append(torch.where((ws["status"] == 0)[:, None], ws["y"][:, :2], torch.zeros_like(ws["y"][:, :2])))
    torch.cuda.synchronize(dev)
    if total == warmup + steps:
        if barrier is not None:
            barrier()
        elapsed = time.perf_counter() - t0
    timed = range(warmup, warmup + steps)
    spans = sorted((ev_base.elapsed_time(a_), ev_base.elapsed_time(b_)) for t in timed for a_, b_ in evp[t])
    busy, ca, cb = 0.0, spans[0][0], spans[0][1]
    for a_, b_ in spans[1:]:
        if a_ > cb:
            busy += cb - ca
            ca, cb = a_, b_
        else:
            cb = max(cb, b_)
    busy += cb - ca
    rts = [evr[k][0].elapsed_time(evr[k][1]) for k in evr if warmup <= k[0] < warmup + steps]
    isz = p["X"].element_size()
    n_refits = sum(1 for (t, c) in refit_log if warmup <= t < warmup + steps)
    report = dict(schedule=schedule, data="loop", batch=Bt, parts=parts, stagger=bool(stagger), max_train=max_train, points_after_refit=window,
                  steps=steps, warmup=warmup, refit_every=refit_every, dt=dt, shift_invariant=bool(shift_invariant), dtype=str(dtype),
                  retry_levels=retry_levels, query_shift_invariant=bool(query_shift_invariant and shift_invariant), fit_iters=fit_iters,
                  factor_dtype=str(factor_dtype) if factor_dtype is not None else str(dtype), min_jitter_level=min_jitter_level, seconds=elapsed, ms_per_step=elapsed / steps * 1e3,
                  instance_steps_per_s=Bt * steps / elapsed, part_refits_in_timed_region=n_refits,
                  pass_busy_ms_per_step=busy / steps, refit_ms_per_part_refit=(sum(rts) / len(rts)) if rts else None,
                  refit_failures_after_retries=int(sum(int(pt.fail_count) for pt in P)) + (sum(g.rgp.count_drop_failures() for g in P) if online else 0),
                  instances_factored_per_retry_level=[int(v) for v in sum((pt.rgp.retry_counts if online else pt.retry_counts) for pt in P).tolist()],
                  jitter_level_max=float(max(float((pt.rgp.jitter_level if online else pt.level).max()) for pt in P)),
                  solver_optimal_fraction=float((ws["status"] == 0).float().mean()), subsample=subsample,
                  pool_rows_at_last_refit=[pt.pool_rows for pt in P] if not online else None)
    if not online:
        pass_bytes = isz * (window * (window + 1) // 2 + 2 * window * n + window * (1 + m)) * Bt
        report["roofline"] = {"pass": dict(bound="hbm", kernel="posterior_step_kernel<%s, 3, 4, 0, 1, false, 0>" % ("float" if isz == 4 else "double"),
                                           algorithmic_bytes_per_step=pass_bytes, achieved=pass_bytes / (busy / steps * 1e-3) / 1e9, peak=8000.0,
                                           unit="GB/s", frac=pass_bytes / (busy / steps * 1e-3) / 1e9 / 8000.0, traffic=None,
                                           note="union of the part batches' pass intervals (HIP events on their streams); a part's refit on its own "
                                                "stream runs beside the other parts' passes and slows them -- this is the loop's rate, not the kernel's alone")}
    # ---- the final model, for the parity checks
    final = dict(hyper={k: v.clone() for k, v in hyper.items()}, xq_check=p["xq"], x=x, ws=ws)
    rowsX, rowsUH, rowsY, rowsJ, Mks, Bks = [], [], [], [], [], []
    for c, pt in enumerate(P):
        xqc = p["xq"][pt.sl].contiguous()
        with torch.cuda.stream(streams[c]):
            if online:
                g = pt.rgp
                rowsX.append(g.X[:, :g.N].clone()); rowsUH.append(g._rUH[:, :g.N].clone())
                rowsY.append(g._rY[:, :g.N].clone()); rowsJ.append(g._rJ[:, :g.N].clone())
                Mk, Bk = g.posterior(xqc)
            elif randsub:
                rowsX.append(pt.sX.clone()); rowsUH.append(pt.sUH.clone()); rowsY.append(pt.sY.clone()); rowsJ.append(pt.sJ.clone())
                b_ = pt.bufs[pt.cur]
                Mk, Bk = ops.posterior_step(b_["Lop"], b_["Vw"], b_["X"], b_["UHB"], pt.hp["ell"], pt.hp["s2"], pt.hp["Bm"], pt.hp["M0"], xqc)
            else:
                sl_ = slice(pt.lo, pt.lo + window)
                rowsX.append(pt.X[:, sl_].clone()); rowsUH.append(pt.UH[:, sl_].clone())
                rowsY.append(pt.Y[:, sl_].clone()); rowsJ.append(pt.J[:, sl_].clone())
                b_ = pt.bufs[pt.cur]
                Mk, Bk = ops.posterior_step(b_["Lop"], b_["Vw"], b_["X"], b_["UHB"], pt.hp["ell"], pt.hp["s2"], pt.hp["Bm"], pt.hp["M0"], xqc)
            Mks.append(Mk); Bks.append(Bk)
    torch.cuda.synchronize(dev)
    final["rows"] = [dict(X=rowsX[c], UH=rowsUH[c], Y=rowsY[c], jitter=rowsJ[c]) for c in range(parts)]   # (parts may hold different N)
    final["bounds"] = bounds
    final["posterior"] = (torch.cat(Mks, 0), torch.cat(Bks, 0))
    final["stream_rows"] = dict(X=Xall, UH=UHall, Y=Yall, jitter=Jall, window=window)
    if randsub:
        final["subset_index"] = torch.cat([pt.sidx for pt in P], 0)
    if record_states:
        final["states"] = dict(x=torch.stack(xs_log, 1), u=torch.stack(us_log, 1))
    return report, final


def final_model_vs_fp64_refit(final, sample=64):
    """Self-check of `self_learning_closed_loop`'s final model: per part, a from-scratch fp64 refit ON THE DEVICE of the rows the
    model holds (with the jitter every point ended up with) against the model's own posterior at `xq_check`; max deviation over
    `sample` instances per part, relative to max(1, |M_k|) and the prior scale.  (The CPU-oracle check lives in tests/.)"""
    hyper, xq = final["hyper"], final["xq_check"]
    Mk_all, Bk_all = final["posterior"]
    worst = dict(Mk=0.0, Bk=0.0, refit_failures=0, instances=0)
    f64 = lambda t: t.double().contiguous()
    for (lo, hi), rows in zip(final["bounds"], final["rows"]):
        Bt = hi - lo
        idx = torch.linspace(0, Bt - 1, min(sample, Bt), device=xq.device).long()
        hp = {k: f64(hyper[k][lo:hi][idx]) for k in ("Bm", "ell", "s2", "M0")}
        X, UH, Y, J = (f64(rows[k][idx]) for k in ("X", "UH", "Y", "jitter"))
        Lr, UHBr, info, _ = ops.refit(X, UH, hp["Bm"], hp["ell"], hp["s2"], J)
        Vr, _ = ops.potrs(Lr, Y, UH, hp["M0"], want_alpha=False)
        Mr, Br = ops.posterior_step(Lr, Vr, X, UHBr, hp["ell"], hp["s2"], hp["Bm"], hp["M0"], f64(xq[lo:hi][idx]))
        prior = (hp["s2"][:, None, None] * hp["Bm"]).abs().amax(dim=(1, 2))
        ok = info == 0
        worst["refit_failures"] += int((~ok).sum())
        worst["instances"] += int(idx.numel())
        if bool(ok.any()):
            dM = ((f64(Mk_all[lo:hi][idx]) - Mr).abs().amax(dim=(1, 2)) / Mr.abs().amax(dim=(1, 2)).clamp(min=1.0))[ok].max()
            dB = ((f64(Bk_all[lo:hi][idx]) - Br).abs().amax(dim=(1, 2)) / prior)[ok].max()
            worst["Mk"], worst["Bk"] = max(worst["Mk"], float(dM)), max(worst["Bk"], float(dB))
    return worst


def pendulum_safety_rollouts(Bt, numSteps=250, dt=0.002, theta0=7 * math.pi / 12, omega0=-0.01, start_noise=0.05,
                             gp=None, shared=False, mean_model=None, true_model=(1.0, 10.0, 1.0), max_unsafe_prob=0.01,
                             k_alpha=(1.0, 3.0), cbf_col_theta=math.pi / 4, cbf_col_delta=math.pi / 8,
                             dtype=torch.float64, device="cuda", use_graph=False, record=False, seed=0, max_iters=100,
                             hessian_mode="reference", plant="true", rho_tol=1e-6, nominal="greedy",
                             lqr_numSteps=None):
    """Bt closed loops of the pendulum's rel-degree-2 safety filter (SOCPController with cbfs = [RadialCBFRelDegree2] and
    the greedy nominal controller, bcbf_pendulum_control_step) from perturbed start states, numSteps steps each.  The
    defaults are run_pendulum_control_online_learning's (pendulum.py:1041-1048: theta0 = 7 pi/12, tau = 0.002, 250 steps,
    float64) with the barrier of RadialCBFRelDegree2 (:643-661).

    gp: None (no-GP mode: the mean model is the whole model, ControlCBFCLFGroundTruth) or the state dict of a learned model
    (`ControlAffineRegressor.gp_dict()` layout: Lop, Vw, X, UHB, ell, s2, Bm, M0, A[, kernel]); shared=True queries ONE
    model (instance 0 of gp, regime S) from every instance, otherwise gp carries Bt models (regime I).
    mean_model: None or the pendulum (mass, gravity, length) added to the learned mean.  A trajectory collides when
    min_h < 0 (NaN-safe: anything not provably >= 0 counts).  Statistics go through `reduce_rollout_stats` (one
    collective at the end, as C4); use_graph replays one captured step on one stream.  Returns dict(stats, x_final[Bt,2],
    min_h[Bt], fails[Bt], traj[numSteps+1,Bt,2] (record), u[numSteps,Bt] (record), loop_seconds).

    plant: "true" (default) -- the pendulum true_model -- or "posterior": every step's plant is a draw from the model's OWN
    posterior at the visited state (`ops.pendulum_control_step_prepare` with `sampled`; true_model is ignored), the distribution
    the program's chance constraint P(CBC2 >= 0) >= 1 - max_unsafe_prob is stated under.  For relative degree 2 the moments the
    program works with are the reference's approximation of a quadratic form's, so whether the loop holds that probability is
    a measurement.  The standard normals z_all[numSteps,Bt,2,4] are drawn once from the seeded device generator, after the
    start noise; row t is gathered per step, so the same seed gives the same trajectories eager and under use_graph.  The result
    gains risk = dict(instance_steps, violations, rate, max_unsafe_prob, min_cbc2, relaxed_steps, violations_relaxed,
    rate_unrelaxed) (`distributed.reduce_cbc2_risk_stats`): over the solved instance-steps, how often CBC2 was negative ON THE
    DRAW, and the same over the steps whose slack rho = y[1] stayed <= rho_tol (the safety cone is soft: a step that bought slack
    was never promised the risk); with record also cbc_s[numSteps,Bt,2] = (L_f h, CBC2) on the draw, status[numSteps,Bt] and
    rho[numSteps,Bt], the slack of every step.
    Draws of different steps are independent (the marginal at each visited (x_t, u_t) is exact); a trajectory is not one
    function drawn from the GP.

    nominal: "greedy" (default) or "lqr" -- the reference's LQRController (its default for the learned pendulum controller,
    controllers.py:64-115, 681) with the horizon numSteps - t at step t: eager passes the host t, use_graph a device step
    counter the captured step increments.  The result gains lqr_failures, the number of instance-steps whose LQR recursion met
    a non-positive pivot (`ops.lqr_nominal`'s status; the nominal control is 0 there).  lqr_numSteps: the controller's numSteps
    when the loop runs fewer steps than the controller plans for (default: numSteps)."""
    if plant not in ("true", "posterior"):
        raise ValueError("plant must be 'true' or 'posterior', got %r" % (plant,))
    if nominal not in ("greedy", "lqr"):
        raise ValueError("nominal must be 'greedy' or 'lqr', got %r" % (nominal,))
    sampled = plant == "posterior"
    lqr = nominal == "lqr"
    dev = torch.device(device)
    f = dict(dtype=dtype, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x0 = torch.tensor([theta0, omega0], **f)
    x = (x0 + start_noise * torch.randn(Bt, 2, generator=gen, **f)).contiguous()
    if gp is not None and shared:
        gp = {k: (v[:1].contiguous() if torch.is_tensor(v) and k in ("Lop", "Vw", "X", "UHB", "M0") else v)
              for k, v in gp.items()}
    ws = ops.pendulum_workspace(Bt, dtype, dev)
    min_h = torch.full((Bt,), float("inf"), **f)
    fails = torch.zeros(Bt, dtype=torch.int32, device=dev)
    state = [x, min_h, fails]                        # what a step changes (saved / restored around the graph capture)
    draw = risk = None
    if sampled:
        z_all = torch.randn(numSteps, Bt, 2, 4, generator=gen, **f)
        draw, risk = _pendulum_risk_buffers(Bt, rho_tol, f)
        state += [risk[k] for k in ("viol", "solved", "min_cbc")] + [draw["relaxed"], draw["viol_relaxed"]]
        tctr = torch.zeros(1, dtype=torch.long, device=dev)
        cbc_traj = torch.empty(numSteps, Bt, 2, **f) if record else None
        status_traj = torch.empty(numSteps, Bt, dtype=torch.int32, device=dev) if record else None
        rho_traj = torch.empty(numSteps, Bt, **f) if record else None
    nom = {}
    if lqr:                # the horizon's step counter lives on the device under use_graph; lstatus failures accumulate per step
        t_dev = torch.zeros(1, dtype=torch.int32, device=dev) if use_graph and not record else None
        lfails = torch.zeros(Bt, dtype=torch.int32, device=dev)
        state += [lfails] + ([t_dev] if t_dev is not None else [])
        nom = dict(nominal="lqr", numSteps=numSteps if lqr_numSteps is None else lqr_numSteps, t_dev=t_dev)
    step = ops.pendulum_control_step_prepare(gp, ws, x, mean_model=mean_model, true_model=true_model, dt=dt,
                                             theta_c=cbf_col_theta, delta_c=cbf_col_delta, k_alpha=k_alpha,
                                             max_unsafe_prob=max_unsafe_prob, max_iters=max_iters,
                                             hessian_mode=hessian_mode, stats=(min_h, fails), sampled=draw, **nom)

    def one_step(t=None):
        if sampled:      # this step's draws (t: a python int, or the device counter inside the captured graph), then the risk counters
            draw["z"].copy_(z_all.index_select(0, t)[0] if torch.is_tensor(t) else z_all[t])
        if lqr:
            step(t=None if t_dev is not None else t)
            lfails.add_(step.lstatus)
            if t_dev is not None:
                t_dev.add_(1)
        else:
            step()
        if sampled:
            ops.rollout_risk(draw["cbc_s"], ws["status"], risk["viol"], risk["solved"], risk["min_cbc"])

    traj = torch.empty(numSteps + 1, Bt, 2, **f) if record else None
    us = torch.empty(numSteps, Bt, **f) if record else None
    if record:
        traj[0] = x
    torch.cuda.synchronize(dev)
    graph = None
    if use_graph and not record:
        side = torch.cuda.Stream(device=dev)
        saved = [v.clone() for v in state]
        with torch.cuda.stream(side):                   # warm-up on the capture stream
            one_step(tctr if sampled else None)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one_step(tctr if sampled else None)
            if sampled:
                tctr.add_(1)
        for dst, src in zip(state, saved):      # the warm-up advanced the state: restore it
            dst.copy_(src)
        torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    for t in range(numSteps):
        if graph is not None:
            graph.replay()
        else:
            one_step(t)
        if record:
            traj[t + 1] = x
            us[t] = ws["u"][:, 0]
            if sampled:
                cbc_traj[t] = draw["cbc_s"]
                status_traj[t] = ws["status"]
                rho_traj[t] = ws["y"][:, 1]
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter() - t_loop
    collided = ~(min_h >= 0)
    stats = reduce_rollout_stats(collided.sum(), min_h.min(), 0.0, (fails > 0).sum(), Bt)
    out = dict(stats=stats, x_final=x, min_h=min_h, fails=fails, traj=traj, u=us, loop_seconds=t_loop, ws=ws)
    if sampled:
        out.update(risk=_pendulum_risk_result(draw, risk, max_unsafe_prob), cbc_s=cbc_traj, status=status_traj, rho=rho_traj)
    if lqr:
        out["lqr_failures"] = int(lfails.sum())
    return out


def _pendulum_risk_buffers(Bt, rho_tol, f):
    """(`sampled` of `ops.pendulum_control_step_prepare`, the counters of `ops.rollout_risk` with Kob = 1) of a pendulum loop
    on a posterior-drawn plant."""
    i = dict(dtype=torch.int32, device=f["device"])
    draw = dict(z=torch.empty(Bt, 2, 4, **f), xdot_s=torch.zeros(Bt, 2, **f), cbc_s=torch.zeros(Bt, 2, **f),
                relaxed=torch.zeros(Bt, **i), viol_relaxed=torch.zeros(Bt, **i), rho_tol=float(rho_tol))
    risk = dict(viol=torch.zeros(Bt, 1, **i), solved=torch.zeros(Bt, **i), min_cbc=torch.full((Bt, 1), float("inf"), **f))
    return draw, risk


def _pendulum_risk_result(draw, risk, max_unsafe_prob):
    return reduce_cbc2_risk_stats(risk["solved"].sum(), risk["viol"].sum(), risk["min_cbc"].min(), draw["relaxed"].sum(),
                                  draw["viol_relaxed"].sum(), max_unsafe_prob)


def pendulum_learning_schedule(numSteps, train_every=10, max_train=200):
    """The refits of the pendulum's learning loop as (t, count, with_replacement): MeanAdjustedModel.train /
    OnlineLearner.observe (controllers.py:336-378) refit after the control of step t when t > 0 and t % train_every == 0, on
    the count = t - 1 rows the buffer then holds (0 .. t-2: x_t is not in it yet); beyond max_train rows a refit draws
    max_train of them WITH replacement (torch.randint, :360-362).  A count of 0 refits nothing (_refit_from_scratch)."""
    out = []
    for t in range(1, numSteps):
        if t % train_every == 0 and t - 1 > 0:
            out.append((t, t - 1, max_train is not None and t - 1 > max_train))
    return out


def pendulum_learning_rollouts(Bt, numSteps=250, dt=0.002, train_every=10, max_train=200, fit_iters=0, learning=True,
                               egreedy=(1.0, 0.01), ctrl_range=(-15.0, 15.0), mean_model=None, hyper=None, retry_levels=3,
                               seed=0, record=False, draws=None, x0=None, theta0=7 * math.pi / 12, omega0=-0.01,
                               start_noise=0.05, true_model=(1.0, 10.0, 1.0), max_unsafe_prob=0.01, k_alpha=(1.0, 3.0),
                               cbf_col_theta=math.pi / 4, cbf_col_delta=math.pi / 8, fit_lr=0.1,
                               gamma_length_scale_prior=(math.pi / 100, math.pi / 100), max_iters=100,
                               hessian_mode="reference", device="cuda", plant="true", rho_tol=1e-6, nominal="greedy"):
    """Bt closed loops of the pendulum that LEARN their dynamics while the safety filter drives them
    (ControlPendulumCBFLearned, pendulum.py:909-961, through ControlCBFLearned / MeanAdjustedModel, controllers.py:320-378,
    665-736; the settings of run_pendulum_control_online_learning, pendulum.py:1041-1048), fp64, regime I: every instance
    learns its own model from its own rows.  Per step, one call of `bcbf_pendulum_control_step_observe_f64`:
      - the learned part is the GP prior of the start hyper-parameters until the first refit (cbc2.posterior_for), then the
        instance's own model; mean_model (None = ZeroDynamicsModel, or the pendulum (mass, gravity, length)) is added;
      - u_ref = EpsilonGreedyController around the greedy control (controllers.py:269-285): eps_t = epsilon(t, {0: egreedy[0],
        numSteps: egreedy[1]}), the uniform action lo + a (hi - lo) with probability eps_t, clipped to ctrl_range;
      - the SOCP safety filter (cbfs = [RadialCBFRelDegree2], clf = None) as `pendulum_safety_rollouts`; an unsolved program
        keeps u_ref;
      - the row (x_t, (1, u_t), (x_{t+1} - x_t)/dt - mean) goes to column t of [Bt, numSteps, 2] stream buffers.  The states
        are the stored, theta-wrapped ones (as the reference's buffer holds them): a step across theta = +-pi gives a target
        of size ~2 pi / dt, as upstream.
    Refits (`pendulum_learning_schedule`): after the control of step t, on rows 0 .. t-2 (all of them up to max_train, else
    torch.randint(count, (max_train,)) rows WITH replacement, gathered on the device); jitter = 1e-5 * rand(N) per refit
    (make_psd), x10 on the failed instances through `ops.refit_with_retries` (the SAME draw scaled, not a fresh one);
    fit_iters > 0 first runs that many Adam iterations of the marginal likelihood (`BatchedHyperFit`, gamma length-scale
    prior, lr fit_lr), hyper-parameters carried from refit to refit; fit_iters = 0 keeps the start values.  hyper: the
    start, a `ControlAffineRegressor(2, 1)` (its values, and its raw parameters for the fit) or dict(ell, s2, Bm, M0, A)
    with a leading axis of 1 or Bt; default a fresh regressor's.  The model serves
    from step t+1 on.  learning=False: no refits, the prior all along (upstream's class as written never learns).
    Deviations from upstream: its class cannot run (QPController with clf=None by default, enable_learning never set); the
    draws come from the loop's torch generator (start noise, then explore[T,Bt,2], then per refit the subset indices and
    the jitter rand), not from Python's `random` / torch's global RNG.

    Eager on one stream; allocation at set-up only (two flat factor buffers at lop_elems(max_train), viewed as
    [Bt, lop_elems(N)], the step re-bound after each refit); no host read of device values between the first and the last
    step (fit_iters > 0: the batched fit looks at its factorisation status once per iteration).  draws = the `draws` of an
    earlier record=True run (explore[T,Bt,2], refits[k] = dict(idx [Bt,max_train] | None, jitter [Bt,N] rand; fit_iters > 0:
    fit_jitter / fit_target, one [Bt,N] / [Bt,N,2] rand per iteration)): replayed
    instead of drawn (a column slice of them is a sub-batch's).  x0: [Bt,2] start states (default (theta0, omega0) +
    start_noise randn).
    plant="posterior" (as `pendulum_safety_rollouts`): every step's plant is a draw from the model the instance holds at that
    step -- the prior until the first refit -- so the rows the loop learns from record the drawn plant; z_all[T,Bt,2,4] is drawn
    after explore (and is not part of `draws`); the result gains `risk`, with record also cbc_s[T,Bt,2].
    nominal="lqr" (as `pendulum_safety_rollouts`): the explorer wraps the reference's LQRController -- upstream's default for this
    class -- instead of the greedy control, horizon numSteps - t at step t; the result gains lqr_failures.
    Returns dict(stats (`reduce_rollout_stats`), report, x_final, min_h, fails; record: traj[T+1,Bt,2], u[T,Bt],
    u_ref[T,Bt], status[T,Bt], draws, rows = the stream buffers (X, UH, Y [Bt,T,2]), final = dict(X, UH, Y, jitter [Bt,N,.]
    of the last refit, hyper, gp = the model the loop ended with))."""
    from .controllers import epsilon
    if plant not in ("true", "posterior"):
        raise ValueError("plant must be 'true' or 'posterior', got %r" % (plant,))
    if nominal not in ("greedy", "lqr"):
        raise ValueError("nominal must be 'greedy' or 'lqr', got %r" % (nominal,))
    sampled = plant == "posterior"
    lqr = nominal == "lqr"
    dev = torch.device(device)
    f = dict(dtype=torch.float64, device=dev)
    n, C = 2, 2
    gen = torch.Generator(device=dev).manual_seed(seed)
    if x0 is None:
        x = (torch.tensor([theta0, omega0], **f) + start_noise * torch.randn(Bt, 2, generator=gen, **f)).contiguous()
    else:
        x = x0.to(**f).clone().contiguous()
        if x.shape != (Bt, 2):
            raise ValueError("x0 must be [Bt, 2]")
    schedule = pendulum_learning_schedule(numSteps, train_every, max_train) if learning else []
    # ---- the draws, made (or replayed) at set-up: explore, then per refit the subset indices and the jitter rand
    if draws is None:
        explore = torch.rand(numSteps, Bt, 2, generator=gen, **f)
        refit_draws = []
        for (t, count, wr) in schedule:
            idx = torch.randint(count, (Bt, max_train), generator=gen, device=dev) if wr else None
            refit_draws.append(dict(idx=idx, jitter=torch.rand(Bt, min(count, max_train), generator=gen, **f)))
    else:
        explore = draws["explore"].to(**f).contiguous()
        refit_draws = draws["refits"]
        if explore.shape != (numSteps, Bt, 2) or len(refit_draws) != len(schedule):
            raise ValueError("draws do not match (numSteps, Bt) or the refit schedule")
    start = hyper
    if start is None:
        from .control_affine_model import ControlAffineRegressor
        start = ControlAffineRegressor(n, 1, device=dev, dtype=torch.float64)
    hyper = start._hyper() if hasattr(start, "_hyper") else start
    hyper = {k: hyper[k].to(**f).expand(Bt, *hyper[k].shape[1:]).clone().contiguous() for k in ("ell", "s2", "Bm", "M0", "A")}
    # ---- stream rows, subset buffers, the two flat factor buffers
    Nmax = min(max_train, max(numSteps - 2, 1))
    Xall, UHall, Yall = (torch.zeros(Bt, numSteps, 2, **f) for _ in range(3))
    flat = lambda k: torch.empty(Bt * k, **f)
    sX, sUH, sY, sJ = flat(Nmax * n), flat(Nmax * C), flat(Nmax * n), flat(Nmax)
    bufs = [dict(Lop=flat(ops.lop_elems(Nmax, torch.float64)), UHB=flat(Nmax * C), Vw=flat(Nmax * n)) for _ in range(2)]
    info, info2 = (torch.zeros(Bt, dtype=torch.int32, device=dev) for _ in range(2))
    fail_count = torch.zeros((), dtype=torch.int64, device=dev)
    retry_counts = torch.zeros(retry_levels + 1, dtype=torch.int64, device=dev)
    ws = ops.pendulum_workspace(Bt, torch.float64, dev)
    min_h = torch.full((Bt,), float("inf"), **f)
    fails = torch.zeros(Bt, dtype=torch.int32, device=dev)
    bf = None
    if fit_iters and schedule:
        from .batched_fit import BatchedHyperFit
        if hasattr(start, "model"):             # a regressor: its raw parameters (the façade's parametrisation)
            theta = BatchedHyperFit.from_models([start.model], dtype=torch.float64, device=dev).theta
            bf = BatchedHyperFit(theta.expand(Bt, -1).contiguous(), n, 1, gamma_length_scale_prior=gamma_length_scale_prior)
        else:
            bf = BatchedHyperFit.from_values(hyper["A"], hyper["Bm"], hyper["ell"], hyper["s2"], hyper["M0"], dtype=torch.float64)
            bf.gamma_length_scale_prior = gamma_length_scale_prior
    kw = dict(mean_model=mean_model, true_model=true_model, dt=dt, theta_c=cbf_col_theta, delta_c=cbf_col_delta,
              k_alpha=k_alpha, max_unsafe_prob=max_unsafe_prob, max_iters=max_iters, hessian_mode=hessian_mode,
              stats=(min_h, fails), ctrl_range=ctrl_range, observe=True)
    if sampled:
        z_all = torch.randn(numSteps, Bt, 2, 4, generator=gen, **f)
        draw, risk = _pendulum_risk_buffers(Bt, rho_tol, f)
        kw["sampled"] = draw
    if lqr:
        lstatus, lfails = (torch.zeros(Bt, dtype=torch.int32, device=dev) for _ in range(2))
        kw.update(nominal="lqr", numSteps=numSteps, lstatus=lstatus)
    ex = explore[0] if egreedy is not None else None          # (each call passes its step's [Bt,2] slice)
    step = ops.pendulum_control_step_prepare(dict(hyper), ws, x, prior=True, explore=ex, **kw)
    model = None
    rec = None
    if record:
        rec = dict(traj=torch.empty(numSteps + 1, Bt, 2, **f), u=torch.empty(numSteps, Bt, **f),
                   u_ref=torch.empty(numSteps, Bt, **f), status=torch.empty(numSteps, Bt, dtype=torch.int32, device=dev))
        rec["traj"][0] = x
        if sampled:
            rec["cbc_s"] = torch.empty(numSteps, Bt, 2, **f)
    E_ = lambda: torch.cuda.Event(enable_timing=True)
    ev_refit = [(E_(), E_()) for _ in schedule]
    refits, final = [], None
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    k = 0
    for t in range(numSteps):
        eps = epsilon(t, interpolate={0: egreedy[0], numSteps: egreedy[1]}) if egreedy is not None else 0.0
        if sampled:
            draw["z"].copy_(z_all[t])
        step(eps=eps, explore=explore[t] if ex is not None else None, obs=(Xall[:, t], UHall[:, t], Yall[:, t], numSteps),
             **(dict(t=t) if lqr else {}))
        if lqr:
            lfails.add_(lstatus)
        if sampled:
            ops.rollout_risk(draw["cbc_s"], ws["status"], risk["viol"], risk["solved"], risk["min_cbc"])
            if record:
                rec["cbc_s"][t] = draw["cbc_s"]
        if record:
            rec["traj"][t + 1] = x
            rec["u"][t] = ws["u"][:, 0]
            rec["u_ref"][t] = ws["u_ref"][:, 0]
            rec["status"][t] = ws["status"]
        if k < len(schedule) and schedule[k][0] == t:
            _, count, wr = schedule[k]
            N = min(count, max_train)
            ev_refit[k][0].record()
            X, UH, Y, J = sX[:Bt * N * n].view(Bt, N, n), sUH[:Bt * N * C].view(Bt, N, C), sY[:Bt * N * n].view(Bt, N, n), sJ[:Bt * N].view(Bt, N)
            if wr:
                idx = refit_draws[k]["idx"].to(dev)[:, :, None].expand(Bt, N, 2)
                torch.gather(Xall[:, :count], 1, idx, out=X)
                torch.gather(UHall[:, :count], 1, idx, out=UH)
                torch.gather(Yall[:, :count], 1, idx, out=Y)
            else:
                X.copy_(Xall[:, :N]); UH.copy_(UHall[:, :N]); Y.copy_(Yall[:, :N])
            torch.mul(refit_draws[k]["jitter"].to(**f), 1e-5, out=J)                  # make_psd: 1e-5 * rand(N)
            if bf is not None:
                # the fit's draws (make_psd's jitter, the 1 + 1e-6 rand target perturbation): the loop's generator, replayed
                # from `draws` or logged into them (record) per iteration
                rd, log = refit_draws[k], None
                if "fit_jitter" in rd:
                    jt, tt = iter(rd["fit_jitter"]), iter(rd["fit_target"])
                    bf.jitter_rand = lambda idx, N_, jt=jt: next(jt).to(**f)[idx]
                    bf.target_rand = lambda Y_, tt=tt: next(tt).to(**f)
                else:
                    if record:
                        log = dict(fit_jitter=[], fit_target=[])

                    def draw(key, *shape, log=log):
                        r = torch.rand(*shape, generator=gen, **f)
                        if log is not None:
                            log[key].append(r)
                        return r
                    bf.jitter_rand = lambda idx, N_: draw("fit_jitter", Bt, N_)[idx]
                    bf.target_rand = lambda Y_: draw("fit_target", *Y_.shape)
                bf.fit(X, UH[:, :, 1:].contiguous(), Y, training_iter=fit_iters, lr=fit_lr)
                if log is not None:
                    rd.update(log)
                hp = bf.derive()
                for key in ("ell", "s2", "Bm", "M0", "A"):
                    hyper[key].copy_(hp[key])
            b_ = bufs[k % 2]
            E = ops.lop_elems(N, torch.float64)
            Lop, UHB, Vw = b_["Lop"][:Bt * E].view(Bt, E), b_["UHB"][:Bt * N * C].view(Bt, N, C), b_["Vw"][:Bt * N * n].view(Bt, N, n)
            ops.refit_with_retries(X, UH, hyper["Bm"], hyper["ell"], hyper["s2"], J, (Lop, UHB, info), levels=retry_levels,
                                   scratch=info2, counts=retry_counts)
            ops.potrs(Lop, Y, UH, hyper["M0"], want_alpha=False, out_Vw=Vw)
            fail_count += (info != 0).sum()
            model = dict(Lop=Lop, Vw=Vw, X=X, UHB=UHB, **hyper)
            step = ops.pendulum_control_step_prepare(model, ws, x, explore=ex, **kw)
            ev_refit[k][1].record()
            refits.append((t, N))
            final = dict(X=X, UH=UH, Y=Y, jitter=J)
            k += 1
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter() - t_loop
    collided = ~(min_h >= 0)
    stats = reduce_rollout_stats(collided.sum(), min_h.min(), 0.0, (fails > 0).sum(), Bt)
    refit_ms = [a_.elapsed_time(b_) for a_, b_ in ev_refit]
    report = dict(batch=Bt, steps=numSteps, dt=dt, train_every=train_every, max_train=max_train, fit_iters=fit_iters,
                  learning=bool(learning), mean_model=mean_model, seconds=t_loop, ms_per_step=t_loop / numSteps * 1e3,
                  instance_steps_per_s=Bt * numSteps / t_loop,
                  refit_ms_per_refit=(sum(refit_ms) / len(refit_ms)) if refit_ms else None,
                  solver_optimal_fraction=1.0 - float(fails.sum()) / (Bt * numSteps),
                  refit_failures_after_retries=int(fail_count),
                  instances_factored_per_retry_level=[int(v) for v in retry_counts.tolist()], refits=refits)
    out = dict(stats=stats, report=report, x_final=x, min_h=min_h, fails=fails, ws=ws)
    if sampled:
        out["risk"] = _pendulum_risk_result(draw, risk, max_unsafe_prob)
    if lqr:
        out["lqr_failures"] = int(lfails.sum())
    if record:
        out.update(rec)
        out["draws"] = dict(explore=explore, refits=refit_draws)
        out["rows"] = dict(X=Xall, UH=UHall, Y=Yall)
        if final is not None:
            final = {key: v.clone() for key, v in final.items()}
        out["final"] = dict(rows=final, hyper={key: v.clone() for key, v in hyper.items()},
                            gp=None if model is None else {key: v.clone() for key, v in model.items()})
    return out


def pendulum_clf_cbf_rollouts(Bt, numSteps=15000, dt=0.002, theta0=5 * math.pi / 12, omega0=-0.01, start_noise=0.05,
                              ctrl_model=(1.0, 10.0, 1.0), true_model=None, record_every=0, dtype=torch.float64, seed=0,
                              steps_per_launch=None, clf_c=1.0, k_alpha=(1.0, 3.0), cbf_col_theta=math.pi / 4,
                              cbf_col_delta=math.pi / 8, cbf_gamma=1.0, cbf_kind="reldeg2", slack_weight=100.0, x0=None,
                              device="cuda"):
    """Bt closed loops of the pendulum's CLF-CBF quadratic program on a KNOWN model (PendulumCBFCLFDirect; the defaults are
    run_pendulum_control_cbf_clf's, pendulum.py:1019-1024: theta0 = 5 pi / 12, tau = 0.002, 15 000 steps) from perturbed
    starts, every step of every loop inside the library's rollout kernel (bcbf_pendulum_clf_cbf_rollout): one launch, or
    ceil(numSteps / steps_per_launch) launches that compose bit for bit.

    ctrl_model: the (mass, gravity, length) the controller believes.  true_model: the plant -- None (= ctrl_model), a
    triple, or a tensor[Bt,3] (one plant per instance): a plant that differs from the controller's model is the
    model-mismatch study.  x0: explicit starts [Bt,2] instead of the perturbed ones.  A trajectory collides when
    min_h < 0 (NaN-safe: anything not provably >= 0 counts); an instance whose program became infeasible is frozen at that
    step (`status` = its 1-based step, `fails` = status > 0) and contributes the statistics it had until then.
    In float32 h at the boundary the nominal run settles on (theta = 3 pi / 8, h ~ 2e-6) is below the rounding of
    cos Delta_c - cos d: the float32 collision count is noise around that boundary, only the float64 count is meaningful.
    Returns dict(stats (`reduce_rollout_stats`), x_final[Bt,2], min_h[Bt], fails[Bt], damage[Bt], status[Bt],
    traj[nrec,Bt,2] and u[nrec,Bt] (record_every > 0: the steps that are multiples of it, before the step), loop_seconds)."""
    dev = torch.device(device)
    f = dict(dtype=dtype, device=dev)
    if x0 is None:
        gen = torch.Generator(device=dev).manual_seed(seed)
        x = (torch.tensor([theta0, omega0], **f) + start_noise * torch.randn(Bt, 2, generator=gen, **f)).contiguous()
    else:
        x = torch.as_tensor(x0).to(**f).reshape(Bt, 2).clone().contiguous()
    ctrl = torch.tensor([float(v) for v in ctrl_model], **f)
    true = ctrl if true_model is None else (true_model.to(**f).contiguous() if torch.is_tensor(true_model)
                                            else torch.tensor([float(v) for v in true_model], **f))
    min_h = torch.full((Bt,), float("inf"), **f)
    damage = torch.zeros(Bt, dtype=torch.int32, device=dev)
    status = torch.zeros(Bt, dtype=torch.int32, device=dev)
    nrec = ops.pendulum_clf_cbf_records(0, numSteps, record_every)
    traj = torch.empty(nrec, Bt, 2, **f) if record_every > 0 else None
    us = torch.empty(nrec, Bt, **f) if record_every > 0 else None
    chunk = numSteps if not steps_per_launch else int(steps_per_launch)
    if chunk < 1 and numSteps > 0:
        raise ValueError("steps_per_launch must be >= 1")
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    t = 0
    while t < numSteps:
        k = min(chunk, numSteps - t)
        r0 = ops.pendulum_clf_cbf_records(0, t, record_every)
        ops.pendulum_clf_cbf_rollout(x, min_h, damage, status, k, dt=dt, ctrl_model=ctrl, true_model=true, clf_c=clf_c,
                                     k_alpha=k_alpha, theta_c=cbf_col_theta, delta_c=cbf_col_delta, cbf_gamma=cbf_gamma,
                                     cbf_kind=cbf_kind, slack_weight=slack_weight,
                                     traj=traj[r0:] if traj is not None else None, u_rec=us[r0:] if us is not None else None,
                                     record_every=record_every, t_offset=t)
        t += k
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter() - t_loop
    collided = ~(min_h >= 0)
    fails = status > 0
    stats = reduce_rollout_stats(collided.sum(), min_h.min(), 0.0, fails.sum(), Bt)
    return dict(stats=stats, x_final=x, min_h=min_h, fails=fails, damage=damage, status=status, traj=traj, u=us,
                loop_seconds=t_loop)


def unicycle_clf_cbf_rollouts(Bt, numSteps=200, dt=0.05, L_ctrl=1.0, L_true=12.0, start=(-3.0, -1.0, -math.pi / 4),
                              goal=(0.0, 0.0, math.pi / 4), start_noise=(0.3, 0.3, 0.5), planner="piecewise", clf="cartesian",
                              obstacles="mid", record_every=0, steps_per_launch=None, dtype=torch.float64, device="cuda", seed=0,
                              Kp=None, term_weights=(0.7, 0.3), cbf_gammas=(5.0, 5.0), frac_time_to_reach_goal=0.95,
                              stop_rho=0.0, x0=None):
    """Bt closed loops of the unicycle's CLF-CBF quadratic program on the MEAN model (ControllerCLF, the controller of the
    reference's model-based demos) from perturbed starts, every step of every loop inside the library's rollout kernel
    (bcbf_unicycle_clf_cbf_rollout): one launch, or ceil(numSteps / steps_per_launch) launches that compose bit for bit.

    L_ctrl: the wheelbase the controller believes.  L_true: the plant's -- a number or a tensor[Bt] (one plant per instance):
    a plant that differs from the controller's model is the model-mismatch study (the defaults are those of
    unicycle_mean_cbf_collides_obstacle: 1 against 12).  planner 'piecewise': PiecewiseLinearPlanner(start, goal, numSteps, dt,
    frac_time_to_reach_goal) -- ONE plan from the nominal start for every instance, as the Monte-Carlo drivers do -- with
    Kp = (0.9, 1.5, 0) (track_trajectory_clf_cartesian); 'none': the goal itself, Kp = (0.9, 1.5, 4).  clf 'polar': CLFPolar
    through cartesian2polar (Kp = (0.6, 1.5, 4, 0); no obstacles, planner 'none').  obstacles 'mid':
    obstacles_at_mid_from_start_and_goal(start, goal, term_weights) with cbf_gammas; None: none.  stop_rho > 0: an instance
    stops once it is within stop_rho of the goal (`converged_at` = that step, -1 = still running).  x0: explicit starts [Bt,3].
    A trajectory collides when min_h < 0 (NaN-safe: anything not provably >= 0 counts); an instance whose program became
    infeasible is frozen at that step (`status` = its 1-based step) and contributes the statistics it had until then.
    Returns dict(stats (`reduce_rollout_stats`), x_final[Bt,3], min_h[Bt], cost[Bt] (sum |u|^2), status[Bt], converged_at[Bt],
    dist_to_goal[Bt], traj[nrec,Bt,3] and u[nrec,Bt,2] (record_every > 0: the steps that are multiples of it, before the step),
    loop_seconds)."""
    from .unicycle_move_to_pose import obstacles_at_mid_from_start_and_goal
    dev = torch.device(device)
    f = dict(dtype=dtype, device=dev)
    start_t, goal_t = torch.tensor([float(v) for v in start], **f), torch.tensor([float(v) for v in goal], **f)
    if x0 is None:
        gen = torch.Generator(device=dev).manual_seed(seed)
        x = (start_t + torch.tensor([float(v) for v in start_noise], **f) * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    else:
        x = torch.as_tensor(x0).to(**f).reshape(Bt, 3).clone().contiguous()
    if clf == "polar" and (obstacles is not None or planner != "none"):
        raise ValueError("clf='polar' runs with planner='none' and obstacles=None")
    if Kp is None:
        Kp = (0.6, 1.5, 4.0, 0.0) if clf == "polar" else (0.9, 1.5, 0.0) if planner == "piecewise" else (0.9, 1.5, 4.0)
    kw = dict(Kp=Kp, clf_kind=clf, L_ctrl=L_ctrl, L_true=L_true.to(**f).contiguous() if torch.is_tensor(L_true) else L_true,
              planner=planner, stop_rho=stop_rho)
    if planner == "piecewise":
        kw.update(x0_plan=start_t.expand(Bt, 3).contiguous(), numStepsPlan=numSteps, frac_time_to_reach_goal=frac_time_to_reach_goal)
    if obstacles == "mid":
        obs = obstacles_at_mid_from_start_and_goal(start_t, goal_t, term_weights=tuple(term_weights))
        kw.update(centers=torch.stack([o.center.to(**f) for o in obs]).contiguous(),
                  radii=torch.stack([o.radius.to(**f) for o in obs]).contiguous(), tw=tuple(term_weights), gammas=tuple(cbf_gammas))
    elif obstacles is not None:
        raise ValueError("obstacles must be 'mid' or None, got %r" % (obstacles,))
    goal_b = goal_t.expand(Bt, 3).contiguous()
    min_h, cost = torch.full((Bt,), float("inf"), **f), torch.zeros(Bt, **f)
    status = torch.zeros(Bt, dtype=torch.int32, device=dev)
    conv = torch.full((Bt,), -1, dtype=torch.int32, device=dev)
    nrec = ops.unicycle_clf_cbf_records(0, numSteps, record_every)
    traj = torch.empty(nrec, Bt, 3, **f) if record_every > 0 else None
    us = torch.empty(nrec, Bt, 2, **f) if record_every > 0 else None
    chunk = numSteps if not steps_per_launch else int(steps_per_launch)
    if chunk < 1 and numSteps > 0:
        raise ValueError("steps_per_launch must be >= 1")
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter()
    t = 0
    while t < numSteps:
        k = min(chunk, numSteps - t)
        r0 = ops.unicycle_clf_cbf_records(0, t, record_every)
        ops.unicycle_clf_cbf_rollout(x, goal_b, cost, status, k, dt=dt, min_h=min_h, converged_at=conv,
                                     traj=traj[r0:] if traj is not None else None, u_rec=us[r0:] if us is not None else None,
                                     record_every=record_every, t_offset=t, **kw)
        t += k
    torch.cuda.synchronize(dev)
    t_loop = time.perf_counter() - t_loop
    collided = ~(min_h >= 0)
    fails = status > 0
    dist = (x[:, :2] - goal_b[:, :2]).norm(dim=-1)
    stats = reduce_rollout_stats(collided.sum(), min_h.min(), cost.sum() / max(numSteps, 1), fails.sum(), Bt)
    return dict(stats=stats, x_final=x, min_h=min_h, cost=cost, status=status, converged_at=conv, dist_to_goal=dist, traj=traj,
                u=us, loop_seconds=t_loop)
