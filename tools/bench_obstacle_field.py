#!/usr/bin/env python3
"""The chance-constrained unicycle loop among an obstacle FIELD (`rollouts.obstacle_field_rollouts`: a working set of three
discs in the fused solver, certified against every disc, at most three solves per step): 4096 instances x 200 steps of
dt = 0.05, fixed-kernel model, fields of Kf = 3, 7, 16, 64 and 256 discs (`rollouts.random_obstacle_field`, seed = Kf), eager and
as one captured graph per step.  Beside it, in the same process and alternating with it, the two paths the project had:
the fused control step with the first three discs as its whole program, and the composed path (task rows ->
terms -> generic cone solver -> plant step) with the seven discs of the Kf = 7 field.  One JSON line per configuration: the
median, minimum and maximum wall time of `--repeat` runs after a warm-up run, each run ending in a device synchronise, per
step and per instance-step; the certificate's counts.  `--plant posterior` adds, alternating with the others in the same rounds,
the field loop on a plant drawn from the model's posterior (`plant="posterior"`: the commit evaluates every disc on the draw) with
its risk rates -- tight, joint, unselected -- and writes profiles/obstacle_field_posterior_plant.json.

    python tools/bench_obstacle_field.py [--quick] [--repeat 3] [--dtype float64] [--plant posterior] [--out profiles/obstacle_field.json]
"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bayesian_cbf_amd import ops
from bayesian_cbf_amd.planner import PiecewiseLinearPlanner
from bayesian_cbf_amd.rollouts import obstacle_field_rollouts, random_obstacle_field, unicycle_task_tensors

START, GOAL = (-3.0, -1.0, -math.pi / 4), (0.0, 0.0, math.pi / 4)
DT, L_TRUE = 0.05, 12.0


def plain_loop(Bt, field, steps, dtype, use_graph):
    """The loop of `monte_carlo_safety_rollouts` with EVERY disc of `field` in the program: `ops.unicycle_control_step` -- the fused
    kernel up to three discs, the composed path beyond.  Returns (loop seconds, solver failures, collisions)."""
    dev = torch.device("cuda")
    f = dict(dtype=dtype, device=dev)
    K = field["radii"].shape[0]
    x0, xg = torch.tensor(START, **f), torch.tensor(GOAL, **f)
    task = unicycle_task_tensors(Bt, x0, xg, dtype, dev, cbf_gammas=(5.0,) * K)
    task.update(sign=torch.tensor([-1.0] + [1.0] * K, **f), relax_mask=torch.tensor([1.0] + [0.0] * K, **f),
                centers=field["centers"].to(**f).expand(Bt, K, 2).contiguous(), radii=field["radii"].to(**f).expand(Bt, K).contiguous())
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (x0 + 0.05 * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    ws = ops.control_workspace(Bt, K, dtype, dev)
    ws["Mk"].zero_()
    ws["Bk"].copy_(torch.eye(3, **f).expand(Bt, 3, 3))
    gp = dict(A=(0.01 * torch.eye(3, **f)).expand(Bt, 3, 3).contiguous())
    planner = PiecewiseLinearPlanner(x0, xg, steps, DT, frac_time_to_reach_goal=0.95)
    plan_all = torch.stack([planner.plan(t).to(dtype=dtype) for t in range(steps)]).to(dev)
    dplan_all = torch.stack([planner.dot_plan(t).to(dtype=dtype) for t in range(steps)]).to(dev)
    task["plan"], task["dot_plan"] = torch.empty(Bt, 3, **f), torch.empty(Bt, 3, **f)
    min_h, cost = torch.full((Bt,), float("inf"), **f), torch.zeros(Bt, **f)
    fails = torch.zeros(Bt, dtype=torch.int32, device=dev)
    tctr = torch.zeros(1, dtype=torch.long, device=dev)
    fused = K + 1 <= 4
    step = ops.unicycle_control_step_prepare(gp, task, ws, x, dt=DT, L_true=L_TRUE, max_iters=30) if fused else None

    def one():
        task["plan"].copy_(plan_all.index_select(0, tctr))
        task["dot_plan"].copy_(dplan_all.index_select(0, tctr))
        if fused:
            step()
        else:
            ops.unicycle_control_step(gp, task, ws, x, dt=DT, L_true=L_TRUE, max_iters=30)
        ops.rollout_stats(ws["cst"], ws["y"], ws["status"], task["w"], task["gammas"], min_h, cost, fails)
        tctr.add_(1)

    graph = None
    state = [x, min_h, cost, fails, tctr]
    if use_graph:
        if not fused:
            raise ValueError("the composed path allocates per step: eager only")
        saved = [v.clone() for v in state]
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            one()
        side.synchronize()
        for d, s in zip(state, saved):
            d.copy_(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one()
        for d, s in zip(state, saved):
            d.copy_(s)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        if graph is not None:
            graph.replay()
        else:
            one()
    torch.cuda.synchronize(dev)
    secs = time.perf_counter() - t0
    return secs, int((fails > 0).sum()), int((~(min_h >= 0)).sum())


def row(name, Bt, steps, Kf, mode, secs, extra):
    secs = sorted(secs)
    med = statistics.median(secs)
    return dict(path=name, Bt=Bt, steps=steps, Kf=Kf, mode=mode, seconds_median=med, seconds_min=secs[0], seconds_max=secs[-1],
                us_per_step=med * 1e6 / steps, ns_per_instance_step=med * 1e9 / (Bt * steps), repeat=len(secs), **extra)


def main():
    quick = "--quick" in sys.argv
    repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 3
    dtype = getattr(torch, sys.argv[sys.argv.index("--dtype") + 1]) if "--dtype" in sys.argv else torch.float64
    plant = sys.argv[sys.argv.index("--plant") + 1] if "--plant" in sys.argv else "true"
    if plant not in ("true", "posterior"):
        sys.exit("--plant true | posterior")
    default_out = "obstacle_field_posterior_plant.json" if plant == "posterior" else "obstacle_field.json"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", default_out)
    Bt, steps = (256, 20) if quick else (4096, 200)
    fields = {Kf: random_obstacle_field(Kf, seed=Kf) for Kf in (3, 7, 16, 64, 256)}
    # every configuration once (warm-up: code objects, allocator, clocks), then `repeat` rounds that alternate all of them
    configs = [("field", Kf, mode) for Kf in fields for mode in ("eager", "graph")]
    if plant == "posterior":
        configs += [("field-posterior", Kf, mode) for Kf in fields for mode in ("eager", "graph")]
    configs += [("fused-3", 3, "eager"), ("fused-3", 3, "graph"), ("composed-7", 7, "eager")]
    times = {c: [] for c in configs}
    extra = {}
    for rnd in range(repeat + 1):
        for c in configs:
            name, Kf, mode = c
            if name in ("field", "field-posterior"):
                r = obstacle_field_rollouts(Bt, fields[Kf], numSteps=steps, dt=DT, L_true=L_TRUE, dtype=dtype, use_graph=mode == "graph",
                                            plant="posterior" if name == "field-posterior" else "true")
                secs = r["loop_seconds"]
                n = Bt * steps
                extra[c] = dict(certified_share=r["certified_steps"] / n, rounds_hist=r["rounds_hist"],
                                uncertified_steps=r["uncertified_steps"], full_set_steps=r["full_set_steps"],
                                unsolved_steps=r["unsolved_steps"], collisions=r["stats"]["collisions"],
                                instances_with_a_step_not_taken=r["stats"]["solver_failures"], min_h=r["stats"]["min_h"])
                if name == "field-posterior":
                    extra[c].update(risk_tight=r["risk"]["tight"], risk_joint=r["risk"]["joint"], risk_unselected=r["risk"]["unselected"],
                                    mean_discs_violated=r["risk"]["mean_discs_violated"], risk_instance_steps=r["risk"]["instance_steps"],
                                    max_risk=r["risk"]["max_risk"])
            else:
                secs, failures, collisions = plain_loop(Bt, fields[Kf], steps, dtype, mode == "graph")
                extra[c] = dict(instances_with_a_step_not_taken=failures, collisions=collisions)
            if rnd > 0:
                times[c].append(secs)
    rows = []
    for c in configs:
        rows.append(row(c[0], Bt, steps, c[1], c[2], times[c], extra[c]))
        print(json.dumps(rows[-1]), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), dtype=str(dtype).replace("torch.", ""), dt=DT, L_true=L_TRUE, slots=3, rounds=3,
                  model="fixed kernel: M_k = 0, B_k = I, A = 0.01 I, max_risk = 0.01", rows=rows,
                  note="wall time of the loop (plan row copies, the step, the bookkeeping) ending in a device synchronise; "
                       "fused-3 and composed-7 are the project's earlier paths with every disc in the program")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
