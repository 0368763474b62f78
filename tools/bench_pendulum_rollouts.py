#!/usr/bin/env python3
"""The pendulum's rel-degree-2 safety loop (bcbf_pendulum_control_step_f64: jets -> task rows -> cbc2 terms -> cones ->
coneqp -> plant step), fp64, N = 512 training points, 250 closed-loop steps per configuration: regime S (one model
queried by every instance) at Bt = 4096 and 32768, regime I (one model per instance) at Bt = 4096.  One JSON line per
configuration: instance-steps/s of the eager loop (one host call per step) and of the HIP-graph replay, and the share of
the step the jets launch takes (events around it, eager loop).
--plant posterior: the same loops on plants drawn from the model's own posterior (bcbf_pendulum_control_step_sampled_f64); each
line then carries the step time next to the true-plant loop's and the empirical risk of the drawn rel-degree-2 condition.
--nominal lqr [--lqr-numsteps K]: the same loops with the reference's LQRController as the nominal controller
(bcbf_pendulum_control_step_nominal_f64), alternated with the greedy loop; each line carries both step times and the LQR
kernel's own time at the full horizon (events around bcbf_lqr_nominal_f64 on the step's factors)."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bayesian_cbf_amd import ops
from bayesian_cbf_amd.rollouts import pendulum_safety_rollouts
from bayesian_cbf_amd.synthetic import make_instances


def model(n_models, N):
    """Models of the pendulum itself: training states over theta in [-3, 3], omega in [-pi, pi], targets the true
    dynamics [omega, -10 sin theta + u] (mass 1, gravity 10, length 1), zero prior mean; the hyper-parameters are
    make_instances' (a throughput benchmark: the model must be good enough that the programs are solvable)."""
    p = make_instances(n_models, N, 2, 1, dtype=torch.float64, device="cuda", seed=3)
    X = p["X"]
    X[..., 0] = (X[..., 0] + 1.5) * 2.0
    th, om, u = X[..., 0], X[..., 1], p["UH"][..., 1]
    p["Xdot"] = torch.stack([om, -10.0 * torch.sin(th) + u], dim=-1).contiguous()
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"])
    assert (info == 0).all()
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    return dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=p["A"])


def jets_share(gp, Bt, steps=50):
    """Fraction of the eager step spent in the jets launch (hipEvents around it, recorded by the entry point)."""
    x = torch.zeros(Bt, 2, dtype=torch.float64, device="cuda")
    x[:, 0] = 7 * math.pi / 12
    ws = ops.pendulum_workspace(Bt, torch.float64, "cuda")
    step = ops.pendulum_control_step_prepare(gp, ws, x)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in evs:                 # torch creates the HIP event at its first record; the library records it afterwards
        a.record()
        b.record()
    for _ in range(10):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for a, b in evs:
        step(a, b)
    e1.record()
    torch.cuda.synchronize()
    jets = sum(a.elapsed_time(b) for a, b in evs)
    return jets / e0.elapsed_time(e1), jets / steps


def posterior_line(regime, Bt, N, steps, kw, repeats=3):
    """One JSON line: the loop on posterior-drawn plants against the same loop on the true plant, the two alternated `repeats`
    times in this process (medians, with every repeat beside them), eager and graph, and the posterior loop's risk."""
    for plant in ("true", "posterior"):
        pendulum_safety_rollouts(Bt, **dict(kw, numSteps=20, plant=plant))         # warm-up (clocks, lazy loads)
    ms = {(plant, how): [] for plant in ("true", "posterior") for how in ("eager", "graph")}
    for _ in range(repeats):
        for plant in ("true", "posterior"):
            eager = pendulum_safety_rollouts(Bt, plant=plant, **kw)
            graph = pendulum_safety_rollouts(Bt, plant=plant, use_graph=True, **kw)
            ms[plant, "eager"].append(eager["loop_seconds"] * 1e3 / steps)
            ms[plant, "graph"].append(graph["loop_seconds"] * 1e3 / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    line = dict(regime=regime, Bt=Bt, N=N, dtype="float64", steps=steps, plant="posterior", repeats=repeats,
                eager_ms_per_step=med["posterior", "eager"], graph_ms_per_step=med["posterior", "graph"],
                true_plant_eager_ms_per_step=med["true", "eager"], true_plant_graph_ms_per_step=med["true", "graph"],
                graph_ms_added=med["posterior", "graph"] - med["true", "graph"],
                all_ms_per_step={"%s_%s" % k: v for k, v in ms.items()},
                risk=eager["risk"], collisions=eager["stats"]["collisions"],
                instances_with_failed_programs=eager["stats"]["solver_failures"],
                graph_equals_eager=bool(torch.equal(eager["x_final"], graph["x_final"])))
    print(json.dumps(line), flush=True)
    return line


def lqr_kernel_ms(gp, Bt, numSteps, launches=20):
    """Milliseconds per launch of bcbf_lqr_nominal_f64 on the factors one step leaves, at the horizon numSteps (events)."""
    x = torch.zeros(Bt, 2, dtype=torch.float64, device="cuda")
    x[:, 0] = 7 * math.pi / 12
    x0 = x.clone()
    ws = ops.pendulum_workspace(Bt, torch.float64, "cuda")
    ops.pendulum_control_step_prepare(gp, ws, x)()
    out = (torch.empty(Bt, 1, dtype=torch.float64, device="cuda"), None, torch.empty(Bt, dtype=torch.int32, device="cuda"))
    call = lambda: ops.lqr_nominal(ws["Mk"], ws["Mj"], x0, (0.0, 0.0), ((1.0, 0.0), (0.0, 1.0)), ((1.0,),), 0.002, numSteps, out=out)
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def nominal_line(regime, Bt, N, steps, kw, lqr_numSteps, repeats=3):
    """One JSON line: the loop with the LQR nominal controller against the greedy loop, alternated `repeats` times in this
    process (medians, with every repeat beside them), eager and graph."""
    lq = dict(nominal="lqr", lqr_numSteps=lqr_numSteps)
    for extra in ({}, lq):
        pendulum_safety_rollouts(Bt, **dict(kw, numSteps=20, **extra))         # warm-up (clocks, lazy loads)
    ms = {(nom, how): [] for nom in ("greedy", "lqr") for how in ("eager", "graph")}
    iters = {}                  # the cone solver's iteration counts at the last step: its launch time follows the slowest lane
    for _ in range(repeats):
        for nom, extra in (("greedy", {}), ("lqr", lq)):
            eager = pendulum_safety_rollouts(Bt, **kw, **extra)
            it = eager["ws"]["iters"].double()
            iters[nom] = dict(mean=float(it.mean()), max=int(it.max()), u_ref_abs_max=float(eager["ws"]["u_ref"].abs().max()))
            graph = pendulum_safety_rollouts(Bt, use_graph=True, **kw, **extra)
            ms[nom, "eager"].append(eager["loop_seconds"] * 1e3 / steps)
            ms[nom, "graph"].append(graph["loop_seconds"] * 1e3 / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    line = dict(regime=regime, Bt=Bt, N=N, dtype="float64", steps=steps, nominal="lqr", lqr_numSteps=lqr_numSteps, repeats=repeats,
                eager_ms_per_step=med["lqr", "eager"], graph_ms_per_step=med["lqr", "graph"],
                greedy_eager_ms_per_step=med["greedy", "eager"], greedy_graph_ms_per_step=med["greedy", "graph"],
                graph_ms_added=med["lqr", "graph"] - med["greedy", "graph"],
                lqr_kernel_ms_full_horizon=lqr_kernel_ms(kw["gp"], Bt, lqr_numSteps),
                last_step_solver_iters=iters, all_ms_per_step={"%s_%s" % k: v for k, v in ms.items()}, lqr_failures=eager["lqr_failures"],
                collisions=eager["stats"]["collisions"], instances_with_failed_programs=eager["stats"]["solver_failures"],
                min_h=eager["stats"]["min_h"], graph_equals_eager=bool(torch.equal(eager["x_final"], graph["x_final"])))
    print(json.dumps(line), flush=True)
    return line


def main(configs=(("S", 4096), ("S", 32768), ("I", 4096)), plant="true", nominal="greedy", lqr_numSteps=None):
    N, steps = 512, int(os.environ.get("BCBF_PEND_STEPS", "250"))
    for regime, Bt in configs:
        gp = model(1 if regime == "S" else Bt, N)
        kw = dict(numSteps=steps, gp=gp, shared=regime == "S")
        if nominal == "lqr":
            nominal_line(regime, Bt, N, steps, dict(kw, plant=plant), lqr_numSteps or steps)
            del gp
            torch.cuda.empty_cache()
            continue
        if plant == "posterior":
            posterior_line(regime, Bt, N, steps, kw)
            del gp
            torch.cuda.empty_cache()
            continue
        pendulum_safety_rollouts(Bt, **dict(kw, numSteps=20))                     # warm-up (clocks, lazy loads)
        eager = pendulum_safety_rollouts(Bt, **kw)
        graph = pendulum_safety_rollouts(Bt, use_graph=True, **kw)
        share, jets_ms = jets_share(gp, Bt)
        print(json.dumps(dict(regime=regime, Bt=Bt, N=N, dtype="float64", steps=steps,
                              eager_instance_steps_per_s=Bt * steps / eager["loop_seconds"],
                              graph_instance_steps_per_s=Bt * steps / graph["loop_seconds"],
                              eager_ms_per_step=eager["loop_seconds"] * 1e3 / steps,
                              graph_ms_per_step=graph["loop_seconds"] * 1e3 / steps,
                              jets_share=share, jets_ms=jets_ms, collisions=eager["stats"]["collisions"],
                              instances_with_failed_programs=eager["stats"]["solver_failures"], min_h=eager["stats"]["min_h"],
                              graph_equals_eager=bool(torch.equal(eager["x_final"], graph["x_final"])))), flush=True)
        del gp, eager, graph
        torch.cuda.empty_cache()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--only", nargs="+", metavar="REGIME:BT", help="a subset of the configurations, e.g. S:4096 (profiling runs)")
    ap.add_argument("--plant", choices=("true", "posterior"), default="true")
    ap.add_argument("--nominal", choices=("greedy", "lqr"), default="greedy")
    ap.add_argument("--lqr-numsteps", type=int, default=None, help="the LQR controller's numSteps (default: the loop's steps)")
    args = ap.parse_args()
    only = [a.split(":") for a in args.only] if args.only else None
    main(tuple((r, int(b)) for r, b in only) if only else ((("S", 4096), ("S", 32768), ("I", 4096))), plant=args.plant,
         nominal=args.nominal, lqr_numSteps=args.lqr_numsteps)
