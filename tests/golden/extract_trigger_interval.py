#!/usr/bin/env python3
"""Extract the trigger-interval results the reference recorded for its committed learning run into a small .npz fixture.

docs/saved-runs/unicycle_move_to_pose_fixed_learning_helps_avoid_getting_stuck_v1.6.3-1-g5fa08e8/ holds, next to the event
file that tests/golden/saved_run_learning_v1p6p3.npz was extracted from, the five text files unicycle_trigger_interval_compute
wrote for it with np.savetxt (bayes_cbf/trigger_interval.py:173-177): Lfh, tau, xvel and the sampled Lfh_num, tau_num, one row
per logged step.  These are data files of the reference (recorded results, not source).
Build-container only:  python tests/golden/extract_trigger_interval.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("BCBF_REFERENCE", "/root/reference")
LEARNING_RUN = "unicycle_move_to_pose_fixed_learning_helps_avoid_getting_stuck_v1.6.3-1-g5fa08e8"
NAMES = ("Lfh", "tau", "xvel", "Lfh_num", "tau_num")


def main():
    rdir = os.path.join(REFERENCE, "docs", "saved-runs", LEARNING_RUN)
    out = {name: np.loadtxt(os.path.join(rdir, name + ".np.txt")).astype(np.float64) for name in NAMES}
    assert all(v.shape == (200,) for v in out.values()), {k: v.shape for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "trigger_interval_v1p6p3.npz"), **out)
    print("trigger_interval_v1p6p3", {k: (v.shape, float(v.min()), float(v.max())) for k, v in out.items()})


if __name__ == "__main__":
    main()
