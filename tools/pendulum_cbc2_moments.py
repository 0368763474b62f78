#!/usr/bin/env python3
"""Exact moments of the pendulum's rel-degree-2 condition against the moments the program works with, on the CPU.

CBC2(x,u) is a quadratic form in the joint posterior of (f, g, df/dx).  For the small model of the tests (16 training rows,
ell = (0.8, 1.1), s2 = 1.5, Bm = [[1, .2], [.2, .8]], A = [[.7, .1], [.1, 1.3]], k_alpha = (1, 3), u0 = 0.7) this prints, per
state: mean / variance of CBC2 over draws of the jet posterior (the construction of bcbf_pendulum_control_step_sampled_f64,
restated in tests/_pendulum_posterior_plant_reference.py), the exact quadratic-form moments, and (mean, var) of
oracle.cbc2.cbc2_terms -- the reference's approximation the program is built from.  One markdown table row per state; DESIGN.md
holds the output.

    python tools/pendulum_cbc2_moments.py [--draws 400000] [--kernel rbf]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _pendulum_posterior_plant_reference as ref  # noqa: E402
from oracle import cbc2 as oc2  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=400000)
    ap.add_argument("--kernel", choices=sorted(ref.KXX), default="rbf")
    ap.add_argument("--seed", type=int, default=12345)
    args = ap.parse_args()
    model = ref.small_model(kernel=args.kernel)
    Z = np.random.default_rng(args.seed).standard_normal((args.draws, 2, 4))
    print("| State (theta, omega) | Draw mean / var | Exact quadratic-form mean / var | `cbc2_terms` mean / var |")
    print("|---|---|---|---|")
    for x in ref.STATES:
        jets, _, mean, S4, (h, gh, Hh) = ref.model_at(model, x)
        _, _, c = ref.cbc2_on(ref.draw(mean, model["A"], S4, Z), ref.U0, h, gh, Hh, ref.K_ALPHA)
        m_ex, v_ex = ref.exact_moments(mean, model["A"], S4, ref.U0, h, gh, Hh, ref.K_ALPHA)
        _, _, m_p, v_p = oc2.cbc2_terms(jets, model["A"], model["Bm"], model["ell"], model["s2"], h, gh, Hh,
                                        np.array(ref.K_ALPHA), np.array([ref.U0]), kernel=args.kernel)
        print("| (%g, %g) | %.3f / %.3f | %.3f / %.3f | %.3f / %.3f |" % (x[0], x[1], c.mean(), c.var(), m_ex, v_ex,
                                                                        float(m_p), float(v_p)))


if __name__ == "__main__":
    main()
