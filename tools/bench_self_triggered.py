#!/usr/bin/env python3
"""Time one event of the self-triggered loop: the fused trigger step (bcbf_unicycle_trigger_step) against today's sequence on the
same inputs -- the model's one-step prediction in torch, `trigger_interval_batch` (uBu, xvel, Lh in torch, then
bcbf_trigger_interval) and `bcbf_unicycle_step` -- at Bt = 4096, Nte = 729, fp32 and fp64; then one whole event (control step with
dt = 0, trigger step, bcbf_rollout_stats), eager and replayed from a captured graph.

    python tools/bench_self_triggered.py [--B 4096] [--Nte 729] [--out profiles/self_triggered.json]

Fixed-kernel model of the Monte-Carlo recipe, start states of `monte_carlo_safety_rollouts`.  Both forms' tau are compared before
anything is timed.  The sequence cannot hold every instance's control for its OWN time (bcbf_unicycle_step takes one dt for the
batch): it is timed with one dt, which flatters it.  tau_max = 1e-6 keeps the state where it is over the timed repetitions, so
every repetition of either form sees the same inputs to six digits.  HIP events around back-to-back calls after a warm-up that
raises the clocks (tools/_timing.py); the fused step, the sequence and the pair kernel alone are timed three times in alternation and
the medians reported (all nine figures are kept).

    python tools/bench_self_triggered.py --plant posterior --audit [--out profiles/self_triggered_posterior.json]

times, in the same alternating scheme, the plain trigger step against bcbf_unicycle_trigger_step_audit on the same inputs (the plant
drawn from the posterior with its risk counters, the audit of the held control, or both, as the flags say) and nothing else: the
medians of three, all six figures, and the plain step's own run-to-run spread (max - min over its three) beside the difference.

    python tools/bench_self_triggered.py --observe [--max-train 512] [--refit-every 20] [--out profiles/self_triggered_learning.json]

times, in the same alternating scheme, bcbf_unicycle_trigger_step_audit with no optional group against
bcbf_unicycle_trigger_step_observe with group O alone (every instance writes a row and its next query at every launch), then the
loop that learns (`rollouts.self_triggered_learning_rollouts` at --max-train points per instance, eager): one whole learning event
(posterior at the query, solve, observing trigger step, bookkeeping) from a run without refits, and one refit period
(--refit-every events and the refit that ends it) from a run with two; each run is made twice and the second is kept."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import timeit  # noqa: E402


def observe_timings(args, ops, task, ws, tws, x, off, r, hyper, plan_all, dplan_all, A, L_true, L_mean, dtype):
    """--observe, one precision: the two entries on the inputs of the other modes, then the loop that learns."""
    import ctypes
    from bayesian_cbf_amd import _lib
    from bayesian_cbf_amd.rollouts import self_triggered_learning_rollouts
    Bt, Nte, P = x.shape[0], off.shape[0], plan_all.shape[0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fn = getattr(_lib.lib, "bcbf_unicycle_trigger_step_audit" + ("_f64" if dtype == torch.float64 else "_f32"))
    bound = (p(x), p(ws["y"]), p(ws["status"]), p(ws["fhat"]), p(ws["ghat"]), p(ws["Mk"]), p(task["centers"]), p(task["tw"]), p(off), float(r),
             p(hyper["ls"]), p(hyper["sf"]), p(hyper["Adiag"]), p(hyper["B"]), 1e-4, 1e-2, 1.0, 1e-9, 1e-6, 1e9, float(L_true), p(plan_all),
             p(dplan_all), 0.05, p(tws["t"]), p(tws["events"]), p(task["plan"]), p(task["dot_plan"]),
             *[p(tws[k]) for k in ("tau", "dt_used", "Lfh", "Lkd", "Lh", "xvel", "uBu")], p(ws["Bk"]), p(A), p(ws["grad"]), p(ws["cst"]),
             p(task["sign"]), p(task["rho"]), *([None] * 13), Bt, hyper["ls"].shape[0], 2, Nte, P)

    def audit_no_group():
        rc = fn(*bound, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _lib.lib.bcbf_last_error().decode()

    # every launch is an observed event: the row index stays inside the stream over all timed launches (3 x (warm-up + reps) each)
    ow = ops.trigger_observe_workspace(Bt, 64, dtype, "cuda")
    ow.update(every=1 << 20, L_mean=L_mean)
    observing = ops.unicycle_trigger_step_prepare(task, ws, tws, x, off, r, hyper, plan_all, dplan_all, 0.05, 1e9, 1e-9, 1e-6, L_true=L_true,
                                                  gp_A=A, observe=ow)
    tws["events"].zero_()

    def observe_row0():
        tws["events"].zero_()                   # (one small fill per launch, in both timed forms, so that e % every == 0: a row is written)
        observing()

    def audit_row0():
        tws["events"].zero_()
        audit_no_group()

    audit_row0()
    observe_row0()
    torch.cuda.synchronize()
    ok = ws["status"] == 0                      # (a solved instance's row holds its control; the streams start with u = 0)
    rows_written = bool((ow["obs"][1][:, 0, 1:][ok] == ws["y"][:, :2][ok]).all()) and bool((ow["xq_next"][:, 2] == x[:, 2]).all())
    runs = [[timeit(f_, reps=args.reps) for f_ in (audit_row0, observe_row0)] for _ in range(3)]      # alternating; the medians count
    audit_ms, obs_ms = (sorted(col)[1] for col in zip(*runs))
    audit_runs = [q[0] for q in runs]
    out = dict(audit_entry_no_group_ms=audit_ms, observing_trigger_step_ms=obs_ms, added_ms=obs_ms - audit_ms, added_over_audit=obs_ms / audit_ms - 1.0,
               audit_spread_ms=max(audit_runs) - min(audit_runs), every_instance_wrote_its_row=rows_written,
               alternating_runs_ms=dict(audit_entry=audit_runs, observe_entry=[q[1] for q in runs]),
               note="both forms zero the event counters before the launch (one small fill) so that every timed launch is an observed event")
    # the loop that learns: events without refits, then two refit periods
    R, W = args.refit_every, args.max_train
    kw = dict(horizon=100.0, dt=0.05, max_train=W, tau_min=1e-3, tau_max=0.05, dtype=dtype, device="cuda", Nte=args.Nte)
    for _ in range(2):
        ev = self_triggered_learning_rollouts(Bt, refit_every=10 * R, max_events=2 * R, **kw)
    for _ in range(2):
        per = self_triggered_learning_rollouts(Bt, refit_every=R, max_events=2 * R, **kw)
    event_ms = ev["loop_seconds"] / (2 * R) * 1e3
    period_ms = per["loop_seconds"] / 2 * 1e3
    out.update(max_train=W, refit_every=R, learning_event_eager_ms=event_ms, refit_period_ms=period_ms, refit_ms=period_ms - R * event_ms,
               refits_in_timed_run=per["learning"]["refits"], refit_failures_after_retries=per["learning"]["refit_failures_after_retries"],
               instances_factored_per_retry_level=per["learning"]["instances_factored_per_retry_level"],
               solved_share_last_event=float((ws["status"] == 0).double().mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--Nte", type=float, default=1e3, help="rounded down to a cube, as the reference does (1e3 -> 729)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--plant", choices=["true", "posterior"], default="true",
                    help="posterior: time the trigger step on the posterior-drawn plant against the plain one (with --audit: both groups)")
    ap.add_argument("--audit", action="store_true", help="time the trigger step with the held-control audit against the plain one")
    ap.add_argument("--observe", action="store_true",
                    help="time the observing trigger step against the audit entry with no group, a whole learning event and a refit period")
    ap.add_argument("--max-train", type=int, default=512, help="--observe: points per instance of the loop that learns")
    ap.add_argument("--refit-every", type=int, default=20, help="--observe: events per refit period")
    ap.add_argument("--out", default=None, help="default profiles/self_triggered.json, self_triggered_posterior.json with --plant posterior / --audit, "
                                                "self_triggered_learning.json with --observe")
    args = ap.parse_args()
    compare_new = args.plant == "posterior" or args.audit
    if args.observe and compare_new:
        sys.exit("--observe times group O alone: drop --plant posterior / --audit")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "self_triggered_learning.json" if args.observe else
                                "self_triggered_posterior.json" if compare_new else "self_triggered.json")
    if not torch.cuda.is_available():
        sys.exit("bench_self_triggered needs the GPU: nothing is measured without it")
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd import trigger_interval as ti
    from bayesian_cbf_amd.rollouts import _trigger_hyper, unicycle_task_tensors
    from bayesian_cbf_amd.unicycle_move_to_pose import ObstacleCBF
    grid = ti.default_test_grid(3, args.Nte)
    Nte, Bt = grid.shape[0], args.B
    r = ti._grid_norm(grid)
    res = dict(B=Bt, Nte=Nte, device=torch.cuda.get_device_name(0), reps=args.reps)
    if not compare_new and not args.observe:
        res["pair_part_alone_ms_f32_recorded"] = 0.372            # profiles/trigger_interval.json, the only figure measured before
    L_true, L_mean, dt_ref = 12.0, 1.0, 0.01
    for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        f = dict(dtype=dtype, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(0)
        x0, xg = torch.tensor([-3.0, -1.0, -math.pi / 4], **f), torch.tensor([0.0, 0.0, math.pi / 4], **f)
        task = unicycle_task_tensors(Bt, x0, xg, dtype, torch.device("cuda"))
        x = (x0 + 0.05 * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
        task["plan"] = (x0 + 0.1 * (xg - x0)).expand(Bt, 3).contiguous()
        task["dot_plan"] = ((xg - x0) / 10.0).expand(Bt, 3).contiguous()
        ws = ops.control_workspace(Bt, 2, dtype, "cuda")
        ws["Mk"].zero_()
        ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
        gp = dict(A=(1e-2 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous())
        solve = ops.unicycle_control_step_prepare(gp, task, ws, x, dt=0.0, L_true=L_true, L_mean=L_mean, max_iters=30)
        solve()
        ls = 0.05 + 0.1 * torch.rand(Bt, 3, generator=gen, **f)
        sf = 0.5 + torch.rand(Bt, generator=gen, **f)
        A = torch.diag_embed(1e-2 * (0.5 + torch.rand(Bt, 3, generator=gen, **f)))
        Bh = torch.eye(3, **f).expand(Bt, 3, 3) * (0.5 + torch.rand(Bt, 1, 1, generator=gen, **f))
        hyper = _trigger_hyper(ls, sf, A, Bh, Bt, f)
        off = torch.as_tensor(grid, **f).contiguous()
        tws = ops.trigger_workspace(Bt, dtype, "cuda")
        P = 200
        plan_all, dplan_all = task["plan"][:1].expand(P, 3).contiguous(), task["dot_plan"][:1].expand(P, 3).contiguous()
        fused = ops.unicycle_trigger_step_prepare(task, ws, tws, x, off, r, hyper, plan_all, dplan_all, 0.05, 1e9, 1e-9, 1e-6,
                                                  L_true=L_true)
        if args.observe:
            res[name] = observe_timings(args, ops, task, ws, tws, x, off, r, hyper, plan_all, dplan_all, gp["A"], L_true, L_mean, dtype)
            print(json.dumps({name: res[name]}))
            continue
        if compare_new:
            aws = ops.trigger_audit_workspace(Bt, 2, dtype, "cuda")
            aws["sampled"]["z"].copy_(torch.randn(Bt, 3, generator=gen, **f))
            new = ops.unicycle_trigger_step_prepare(task, ws, tws, x, off, r, hyper, plan_all, dplan_all, 0.05, 1e9, 1e-9, 1e-6, L_true=L_true,
                                                    gp_A=gp["A"], sampled=aws["sampled"] if args.plant == "posterior" else None,
                                                    audit=aws["audit"] if args.audit else None)
            fused()
            new()                                   # (from here on every solved instance has a held control to audit)
            torch.cuda.synchronize()
            runs = [[timeit(fn, reps=args.reps) for fn in (fused, new)] for _ in range(3)]      # alternating; the medians count
            plain_ms, new_ms = (sorted(col)[1] for col in zip(*runs))
            plain_runs = [q[0] for q in runs]
            res[name] = dict(plain_trigger_step_ms=plain_ms, audit_trigger_step_ms=new_ms, plant=args.plant, audit=bool(args.audit),
                             added_ms=new_ms - plain_ms, added_over_plain=new_ms / plain_ms - 1.0,
                             plain_spread_ms=max(plain_runs) - min(plain_runs), solved=int((ws["status"] == 0).sum()),
                             audited_events=int(aws["audit"]["audit_n"].sum()), counted_events=int(aws["sampled"]["solved"].sum()),
                             alternating_runs_ms=dict(plain=plain_runs, audit_entry=[q[1] for q in runs]))
            print(json.dumps({name: res[name]}))
            continue
        cbfs = [ObstacleCBF(task["centers"][:, k], task["radii"][:, k], (0.7, 0.3)) for k in range(2)]
        x_seq = x.clone()
        u = ws["y"][:, :2].contiguous()

        def sequence():
            ub = torch.cat([torch.ones(Bt, 1, **f), u], dim=1)
            xtp1 = x_seq + (ws["fhat"] + torch.einsum("bdi,bi->bd", ws["ghat"], u) + torch.einsum("bdc,bc->bd", ws["Mk"], ub)) * dt_ref
            out = ti.trigger_interval_batch(x_seq, xtp1, u, ls, sf, A, Bh, cbfs, dt_ref, off=off, r=r)
            ops.unicycle_step(x_seq, u, 1e-6, L_true)
            return out

        # the same numbers first
        fused()
        seq = sequence()
        torch.cuda.synchronize()
        ok = ws["status"] == 0
        dev = float(((tws["tau"] - seq["tau"]).abs() / seq["tau"].abs())[ok].max())
        pair = lambda: ops.trigger_interval(x_seq, off, ls, sf, hyper["Adiag"], seq["uBu"], seq["xvel"], seq["Lh"], r)
        runs = [[timeit(fn, reps=args.reps) for fn in (fused, sequence, pair)] for _ in range(3)]      # alternating; the medians count
        fused_ms, seq_ms, pair_ms = (sorted(col)[1] for col in zip(*runs))
        # one whole event
        min_h, cost = torch.full((Bt,), float("inf"), **f), torch.zeros(Bt, **f)
        fails = torch.zeros(Bt, dtype=torch.int32, device="cuda")

        def event():
            solve()
            fused()
            ops.rollout_stats(ws["cst"], ws["y"], ws["status"], task["w"], task["gammas"], min_h, cost, fails)

        solve_ms = timeit(solve, reps=args.reps)
        eager_ms = timeit(event, reps=args.reps)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            event()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            event()
        torch.cuda.synchronize()
        graph_ms = timeit(graph.replay, reps=args.reps)
        res[name] = dict(fused_trigger_step_ms=fused_ms, sequence_ms=seq_ms, sequence_over_fused=seq_ms / fused_ms,
                         pair_kernel_alone_ms=pair_ms, fused_over_pair_kernel_alone=fused_ms / pair_ms, tau_max_rel_dev_vs_sequence=dev,
                         solved=int(ok.sum()), control_step_dt0_ms=solve_ms, event_eager_ms=eager_ms, event_graph_ms=graph_ms,
                         events_per_s_graph=Bt / (graph_ms * 1e-3), fused_is_faster_than_sequence=bool(fused_ms < seq_ms),
                         alternating_runs_ms=dict(fused=[q[0] for q in runs], sequence=[q[1] for q in runs], pair_kernel=[q[2] for q in runs]))
        print(json.dumps({name: res[name]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
