"""Development soak: one-wave refit, super-panel instantiation against the plain one over random shapes, with an order-1 jitter
(well conditioned: the two must agree to rounding in both precisions)."""
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
from bayesian_cbf_amd import ops
from bayesian_cbf_amd.synthetic import make_instances
rng = np.random.default_rng(7)
worst = {torch.float32: 0.0, torch.float64: 0.0}
for case in range(24):
    dt = torch.float64 if case % 3 == 0 else torch.float32
    N = int(rng.integers(64, 1400)); n = int(rng.integers(1, 5)); m = int(rng.integers(1, 4)); Bt = int(rng.integers(1, 9))
    p = make_instances(Bt, N, n, m, dtype=dt, device="cuda", seed=2000 + case)
    big = (p["jitter"] * 5e4).contiguous()
    Ls, Us, is_, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], big, form=ops.REFIT_WAVE | ops.REFIT_SUPER_ON)
    Lp, Up, ip, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], big, form=ops.REFIT_WAVE | ops.REFIT_SUPER_OFF)
    torch.cuda.synchronize()
    assert torch.equal(is_, ip) and int((is_ != 0).sum()) == 0, (case, N, n, m, is_.tolist(), ip.tolist())
    err = float((Ls - Lp).abs().max() / Lp.abs().max())
    worst[dt] = max(worst[dt], err)
    if err > (1e-11 if dt == torch.float64 else 3e-4):      # (fp32: cond x eps -- 1390 points on a line with an order-1 jitter: 7e-5)
        print("MISMATCH", case, dt, N, n, m, Bt, err)
print("worst relative difference fp64 %.2e fp32 %.2e" % (worst[torch.float64], worst[torch.float32]))
