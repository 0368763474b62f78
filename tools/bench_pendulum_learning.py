#!/usr/bin/env python3
"""The pendulum's safety loop that learns its dynamics online (rollouts.pendulum_learning_rollouts on
bcbf_pendulum_control_step_observe_f64, fp64, regime I, 250 steps of dt = 0.002 from theta0 = 7 pi / 12, refits every 10
steps on at most 200 rows): Bt = 4096 with fit_iters = 0, Bt = 4096 with learning off (the GP prior all along), Bt = 256
and 1024 with fit_iters = 100 (the reference's training_iter).  One JSON line per configuration: instance-steps/s, ms per
step, refit ms per refit (events), solver_optimal_fraction, refit failures, instances per retry level, collisions.
`--only 4096:0 4096:off` picks configurations (Bt:fit_iters | Bt:off); BCBF_PEND_STEPS sets the step count."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bayesian_cbf_amd.rollouts import pendulum_learning_rollouts

CONFIGS = ("4096:0", "4096:off", "256:100", "1024:100")


def run(tag, steps):
    bt, fit = tag.split(":")
    kw = dict(learning=False) if fit == "off" else dict(fit_iters=int(fit))
    pendulum_learning_rollouts(int(bt), numSteps=20, seed=1, **kw)                   # warm-up (first launches, allocator)
    r = pendulum_learning_rollouts(int(bt), numSteps=steps, seed=0, **kw)
    rep = r["report"]
    keys = ("instance_steps_per_s", "ms_per_step", "refit_ms_per_refit", "solver_optimal_fraction",
            "refit_failures_after_retries", "instances_factored_per_retry_level")
    out = dict(config=tag, batch=int(bt), steps=steps, learning=fit != "off", fit_iters=0 if fit == "off" else int(fit),
               refits=len(rep["refits"]), collisions=r["stats"].get("collisions"), min_h=r["stats"].get("min_h"),
               device=torch.cuda.get_device_name(0))
    out.update({k: rep[k] for k in keys})
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    only = args[args.index("--only") + 1:] if "--only" in args else list(CONFIGS)
    steps = int(os.environ.get("BCBF_PEND_STEPS", "250"))
    for tag in only:
        run(tag, steps)


if __name__ == "__main__":
    main()
