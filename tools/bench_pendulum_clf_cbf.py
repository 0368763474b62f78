#!/usr/bin/env python3
"""The pendulum's CLF-CBF quadratic program on the known model, every step of every rollout inside one launch
(`rollouts.pendulum_clf_cbf_rollouts`, bcbf_pendulum_clf_cbf_rollout): 15 000 steps of tau = 0.002 from perturbed starts,
matched plant and a mismatched one ((1, 10, 1) believed, (2, 10, 0.5) true), Bt = 4096 and 262144, fp64 and fp32.
One JSON line per configuration: instance-steps/s (the median of `--repeat` timed runs after one warm-up run), the collision
rate, the instances whose program became infeasible.  The fp32 collision rate is printed but is noise around the boundary the
matched run settles on (h ~ 2e-6 there, below fp32 rounding): only the fp64 rate means something.

Also measured: the free-running drift of the device loop against the numpy loop of tests/_pendulum_qp_reference.py (300
steps, 130 starts, every second plant mismatched -- the quantity tests/test_gpu_pendulum_qp.py bounds), and, for context
only, the per-step cost of the existing per-launch loop `pendulum_safety_rollouts(gp=None)`: a different, heavier
controller (a cone program per step), so the two are not a comparison and nothing is asserted on either.

    python tools/bench_pendulum_clf_cbf.py [--quick] [--repeat 3] [--out profiles/pendulum_clf_cbf.json]
"""
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from bayesian_cbf_amd.rollouts import pendulum_clf_cbf_rollouts, pendulum_safety_rollouts

MISMATCHED = (2.0, 10.0, 0.5)


def timed(Bt, steps, dtype, true_model, repeat):
    kw = dict(numSteps=steps, dtype=dtype, true_model=true_model)
    pendulum_clf_cbf_rollouts(Bt, **dict(kw, numSteps=min(steps, 500)))                    # warm-up (clocks, lazy loads)
    runs = [pendulum_clf_cbf_rollouts(Bt, **kw) for _ in range(repeat)]
    secs = sorted(r["loop_seconds"] for r in runs)
    s = runs[0]["stats"]
    return dict(Bt=Bt, steps=steps, dtype=str(dtype).replace("torch.", ""), plant="matched" if true_model is None else "mismatched",
                instance_steps_per_s=Bt * steps / statistics.median(secs), seconds_median=statistics.median(secs),
                seconds_min=secs[0], seconds_max=secs[-1], repeat=repeat, collisions=s["collisions"],
                collision_rate=s["collisions"] / Bt, infeasible_instances=s["solver_failures"], min_h=s["min_h"])


def free_running_drift():
    import _pendulum_qp_reference as R
    x0 = R.loop_starts(130)
    true = np.tile([1.0, 10.0, 1.0], (130, 1))
    true[1::2] = MISMATCHED
    dev = pendulum_clf_cbf_rollouts(130, numSteps=300, x0=x0, true_model=torch.tensor(true, dtype=torch.float64, device="cuda"))
    ref = R.rollout(x0, (1.0, 10.0, 1.0), true, 300)
    x, mh = dev["x_final"].cpu().numpy(), dev["min_h"].cpu().numpy()
    return dict(steps=300, Bt=130, x_final=float(np.abs(x - ref["x"]).max() / np.abs(ref["x"]).max()),
                min_h=float(np.abs(mh - ref["min_h"]).max() / np.abs(ref["min_h"]).max()),
                note="max abs deviation over max abs reference, device fp64 loop against the numpy fp64 loop")


def per_launch_context(Bt=4096, steps=250):
    pendulum_safety_rollouts(Bt, numSteps=20, gp=None, mean_model=(1.0, 10.0, 1.0))
    r = pendulum_safety_rollouts(Bt, numSteps=steps, gp=None, mean_model=(1.0, 10.0, 1.0))
    return dict(Bt=Bt, steps=steps, ms_per_step=r["loop_seconds"] * 1e3 / steps,
                instance_steps_per_s=Bt * steps / r["loop_seconds"],
                note="pendulum_safety_rollouts(gp=None): the rel-degree-2 cone program, one host call per step -- a different, "
                     "heavier controller; context, not a comparison")


def main():
    quick = "--quick" in sys.argv
    repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 3
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "pendulum_clf_cbf.json")
    steps = 1500 if quick else 15000
    rows = []
    for dtype in (torch.float64, torch.float32):
        for Bt in (4096,) if quick else (4096, 262144):
            for true_model in (None, MISMATCHED):
                rows.append(timed(Bt, steps, dtype, true_model, repeat))
                print(json.dumps(rows[-1]), flush=True)
    drift = free_running_drift()
    print(json.dumps(dict(free_running_drift=drift)), flush=True)
    context = per_launch_context()
    print(json.dumps(dict(per_launch_loop_context=context)), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), tau=0.002, theta0=5 * math.pi / 12, start_noise=0.05,
                  ctrl_model=[1.0, 10.0, 1.0], mismatched_plant=list(MISMATCHED), rollouts=rows, free_running_drift=drift,
                  per_launch_loop_context=context,
                  limits=["the program's unique optimum in closed form; parity with cvxopt's iterates is not claimed",
                          "fp32 collision counts are not meaningful at the boundary the matched run settles on (h ~ 2e-6)"])
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
