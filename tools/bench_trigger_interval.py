#!/usr/bin/env python3
"""Time the trigger-interval kernel (bcbf_trigger_interval) at B = 4096 instances, Nte = 729 test points, n = 3, fp32 and fp64,
against a chunked torch implementation of the same pairwise maximum on the device.

    python tools/bench_trigger_interval.py [--B 4096] [--Nte 729] [--out profiles/trigger_interval.json]

HIP events around `reps` back-to-back launches after a warm-up that raises the clocks (tools/_timing.py).  The torch form
materialises the [chunk, Nte, Nte, 3] differences of `chunk` instances at a time (all ORDERED pairs: it is what one writes
without a kernel); both forms' Lkd are compared at the timed size before anything is timed.  Per precision the JSON holds:
kernel_ms, torch_ms, their ratio, the exponentials the kernel issues per second (64 lanes per tile row, idle lanes of the last
tile included) and the ordered-pair-equivalent rate B Nte^2 / t (what the reference's loop would have had to evaluate)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import timeit  # noqa: E402


def issued_exponentials(Nte):
    """Lane-level exponentials of one instance: every work unit (tile pair) runs nb(Bt) iterations on 64 lanes."""
    T = (Nte + 63) // 64
    units = T * ((T - 1) // 2 + 1) + (T // 2 if T % 2 == 0 else 0)
    total = 0
    for u in range(units):
        S, A = divmod(u, T)
        Bt = (A + S) % T
        total += 64 * min(64, Nte - 64 * Bt)
    return total


def torch_pair_max(x, off, ls, chunk):
    """max over ordered pairs of |d_j| exp(-1/2 |d / ls|^2), [B, n]: chunk instances at a time."""
    out = torch.empty_like(x)
    for lo in range(0, x.shape[0], chunk):
        X = off[None] + x[lo:lo + chunk, None, :]
        d = X[:, :, None, :] - X[:, None, :, :]
        k = torch.exp(-0.5 * ((d / ls[lo:lo + chunk, None, None, :]) ** 2).sum(-1))
        out[lo:lo + chunk] = (d.abs() * k[..., None]).amax(dim=(1, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--Nte", type=float, default=1e3, help="rounded down to a cube, as the reference does (1e3 -> 729)")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trigger_interval.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trigger_interval needs the GPU: nothing is measured without it")
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd import trigger_interval as ti
    grid = ti.default_test_grid(3, args.Nte)
    Nte, B, n = grid.shape[0], args.B, 3
    r = ti._grid_norm(grid)
    res = dict(B=B, Nte=Nte, n=n, device=torch.cuda.get_device_name(0), reps=args.reps, torch_chunk=args.chunk,
               issued_exponentials_per_instance=issued_exponentials(Nte))
    for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        f = dict(dtype=dtype, device="cuda")
        rnd = lambda *s: torch.rand(*s, generator=g, **f)
        x = (rnd(B, n) - 0.5) * 6
        off = torch.as_tensor(grid, **f)
        ls = 0.05 + 0.1 * rnd(B, n)                        # of the order of the grid's extent: no early saturation of the maximum
        sf, Adiag, uBu, xvel, Lh = 0.5 + rnd(B), 0.5 + rnd(B, n), 0.5 + rnd(B), 0.5 + rnd(B), 0.5 + rnd(B)
        out = tuple(torch.empty(s, **f) for s in ((B,), (B,), (B, n)))
        run = lambda: ops.trigger_interval(x, off, ls, sf, Adiag, uBu, xvel, Lh, r, out=out)
        run()
        torch.cuda.synchronize()
        # the same numbers first (measuring guide: faster and different is not faster)
        want = torch_pair_max(x, off, ls, args.chunk) * (uBu.abs() * sf ** 2)[:, None] * 2 / ls ** 4
        dev = float(((out[2] - want).abs() / want.abs()).max())
        kernel_ms = timeit(run, reps=args.reps)
        torch_ms = timeit(lambda: torch_pair_max(x, off, ls, args.chunk), reps=max(2, args.reps // 10), warm_ms=0.0, min_warm=1)
        res[name] = dict(kernel_ms=kernel_ms, torch_ms=torch_ms, torch_over_kernel=torch_ms / kernel_ms,
                         exp_issued_per_s=B * res["issued_exponentials_per_instance"] / (kernel_ms * 1e-3),
                         ordered_pairs_equiv_per_s=B * Nte * Nte / (kernel_ms * 1e-3), Lkd_max_rel_dev_vs_torch=dev,
                         finite=bool(torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()))
        print(json.dumps({name: res[name]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
