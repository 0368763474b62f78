#!/usr/bin/env python3
"""The unicycle's CLF-CBF quadratic program on the mean model, every step of every rollout inside one launch
(`rollouts.unicycle_clf_cbf_rollouts`, bcbf_unicycle_clf_cbf_rollout): 512 steps of dt = 0.05 from perturbed starts, tracking
PiecewiseLinearPlanner past the two mid obstacles, matched plant (L = 1) and a mismatched one (L = 12 against a controller
that believes 1), Bt = 4096 and 262144, fp64 and fp32.  One JSON line per configuration: the kernel alone by device events and
the wall time of the driver, both per instance-step (the median of `--repeat` timed runs after one warm-up run), the collision
rate, the instances whose program became infeasible.

In the same process, the path this replaces: `sampling.sample_generator_trajectory` over
`ControllerCLF(solver="ipm").control` -- one task-row launch, host einsums and one generic fp64 interior-point solve per step,
driven from Python -- on the same task at 4096 instances and 512 steps.  Also measured: the free-running drift of the device
loop against the numpy loop of tests/_unicycle_qp_reference.py (300 steps, 130 starts, every second plant mismatched -- the
quantity tests/test_gpu_unicycle_qp.py bounds).

    python tools/bench_unicycle_clf_cbf.py [--quick] [--repeat 3] [--out profiles/unicycle_clf_cbf.json]
"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from bayesian_cbf_amd import ops
from bayesian_cbf_amd import unicycle_move_to_pose as U
from bayesian_cbf_amd.rollouts import unicycle_clf_cbf_rollouts
from bayesian_cbf_amd.sampling import sample_generator_trajectory

START, GOAL = (-3.0, -1.0, -math.pi / 4), (0.0, 0.0, math.pi / 4)
STEPS, DT = 512, 0.05


def kernel_ms(Bt, steps, dtype, L_true, repeat):
    """The launch alone, by device events: median ms over `repeat` launches from the same starts."""
    f = dict(dtype=dtype, device="cuda")
    start, goal = torch.tensor(START, **f), torch.tensor(GOAL, **f)
    obs = U.obstacles_at_mid_from_start_and_goal(start, goal, term_weights=(0.7, 0.3))
    kw = dict(dt=DT, planner="piecewise", x0_plan=start.expand(Bt, 3).contiguous(), numStepsPlan=steps, frac_time_to_reach_goal=0.95,
              Kp=(0.9, 1.5, 0.0), L_ctrl=1.0, L_true=L_true, centers=torch.stack([o.center.to(**f) for o in obs]).contiguous(),
              radii=torch.stack([o.radius.to(**f) for o in obs]).contiguous(), tw=(0.7, 0.3), gammas=(5.0, 5.0))
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = start + torch.tensor([0.3, 0.3, 0.5], **f) * torch.randn(Bt, 3, generator=gen, **f)
    goal_b = goal.expand(Bt, 3).contiguous()
    ms = []
    for _ in range(repeat + 1):
        x, min_h, cost = x0.clone(), torch.full((Bt,), float("inf"), **f), torch.zeros(Bt, **f)
        status = torch.zeros(Bt, dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.unicycle_clf_cbf_rollout(x, goal_b, cost, status, steps, min_h=min_h, **kw)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[1:])


def timed(Bt, steps, dtype, L_true, repeat):
    kw = dict(numSteps=steps, dt=DT, dtype=dtype, L_ctrl=1.0, L_true=L_true)
    unicycle_clf_cbf_rollouts(Bt, **kw)                                                  # warm-up (clocks, lazy loads)
    runs = [unicycle_clf_cbf_rollouts(Bt, **kw) for _ in range(repeat)]
    secs = sorted(r["loop_seconds"] for r in runs)
    s = runs[0]["stats"]
    k_ms = kernel_ms(Bt, steps, dtype, L_true, repeat)
    return dict(Bt=Bt, steps=steps, dtype=str(dtype).replace("torch.", ""), plant="matched" if L_true == 1.0 else "mismatched",
                kernel_ms=k_ms, kernel_ns_per_instance_step=k_ms * 1e6 / (Bt * steps),
                wall_ns_per_instance_step=statistics.median(secs) * 1e9 / (Bt * steps), seconds_median=statistics.median(secs),
                seconds_min=secs[0], seconds_max=secs[-1], repeat=repeat, collisions=s["collisions"],
                collision_rate=s["collisions"] / Bt, infeasible_instances=s["solver_failures"], min_h=s["min_h"])


def replaced_path(Bt=4096, steps=STEPS, L_true=12.0):
    """The same trajectories the parent's way: one Python-driven control evaluation (rows, einsums, generic interior point) and one
    plant launch per step."""
    f = dict(dtype=torch.float64, device="cuda")
    start, goal = torch.tensor(START, **f), torch.tensor(GOAL, **f)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = (start + torch.tensor([0.3, 0.3, 0.5], **f) * torch.randn(Bt, 3, generator=gen, **f)).contiguous()
    ctrl = U.ControllerCLF(U.PiecewiseLinearPlanner(start, goal, steps, DT, 0.95), coordinate_converter=lambda x, xg: x,
                           dynamics=U.CartesianDynamics(), clf=U.CLFCartesian(Kp=(0.9, 1.5, 0.0)),
                           cbfs=U.obstacles_at_mid_from_start_and_goal(start, goal, term_weights=(0.7, 0.3)), cbf_gammas=[5.0, 5.0],
                           solver="ipm")
    sample_generator_trajectory(U.AckermannDrive(L=L_true), 8, dt=DT, x0=x0.clone(), controller=ctrl.control)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, X, _ = sample_generator_trajectory(U.AckermannDrive(L=L_true), steps, dt=DT, x0=x0.clone(), controller=ctrl.control)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    one = unicycle_clf_cbf_rollouts(Bt, numSteps=steps, dt=DT, L_ctrl=1.0, L_true=L_true, x0=x0)
    dev = float((X[-1] - one["x_final"]).abs().max() / X[-1].abs().max())
    return dict(Bt=Bt, steps=steps, dtype="float64", plant="mismatched", seconds=secs, ms_per_step=secs * 1e3 / steps,
                wall_ns_per_instance_step=secs * 1e9 / (Bt * steps), one_launch_seconds=one["loop_seconds"],
                x_final_deviation_from_the_one_launch_loop=dev,
                note="sample_generator_trajectory over ControllerCLF(solver='ipm').control: the parent's way to the same "
                     "trajectories (interior-point tolerance apart)")


def free_running_drift():
    import _unicycle_qp_reference as R
    from test_unicycle_qp_cpu import loop_case
    c = loop_case()
    dev = unicycle_clf_cbf_rollouts(130, numSteps=300, dt=0.05, x0=c["x0"], L_ctrl=1.0,
                                    L_true=torch.tensor(c["L_true"], dtype=torch.float64, device="cuda"), term_weights=(0.7, 0.3))
    ref = R.rollout(**c)
    out = dict(steps=300, Bt=130, note="max abs deviation over max abs reference, device fp64 loop against the numpy fp64 loop")
    for name, key in (("x_final", "x"), ("min_h", "min_h"), ("cost", "cost")):
        out[name] = float(np.abs(dev[name].cpu().numpy() - ref[key]).max() / np.abs(ref[key]).max())
    return out


def main():
    quick = "--quick" in sys.argv
    repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 3
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "unicycle_clf_cbf.json")
    rows = []
    for dtype in (torch.float64, torch.float32):
        for Bt in (4096,) if quick else (4096, 262144):
            for L_true in (1.0, 12.0):
                rows.append(timed(Bt, STEPS, dtype, L_true, repeat))
                print(json.dumps(rows[-1]), flush=True)
    drift = free_running_drift()
    print(json.dumps(dict(free_running_drift=drift)), flush=True)
    old = replaced_path(steps=64 if quick else STEPS)
    print(json.dumps(dict(replaced_path=old)), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), dt=DT, start=list(START), goal=list(GOAL), start_noise=[0.3, 0.3, 0.5],
                  L_ctrl=1.0, L_mismatched=12.0, rollouts=rows, free_running_drift=drift, replaced_path=old,
                  limits=["the program's unique optimum in closed form; parity with GUROBI's iterates is not claimed"])
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
