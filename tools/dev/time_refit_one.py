"""Latency of ONE model's refit (the facade's fit / clear_cache path), fp32 and fp64 (development).  argv[1]: workgroup | wave | pair |
team4 | team8 forces the form."""
import sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from bayesian_cbf_amd import ops
from bayesian_cbf_amd.synthetic import make_instances
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit
NAME = sys.argv[1] if len(sys.argv) > 1 else "auto"
FORM = None if NAME == "auto" else getattr(ops, "REFIT_" + NAME.upper())
for dtype in (torch.float32, torch.float64):
    out = []
    for N in (128, 256, 512, 1024):
        p = make_instances(1, N, 3, 2, dtype=dtype, device="cuda", seed=5)
        p["X"] = (2.0 * p["X"]).contiguous()
        t = timeit(lambda: ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], form=FORM), reps=20)
        r = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], want_dense=True, form=FORM)
        out.append("%d: %.0f us%s" % (N, t * 1e3, "" if int(r[2][0]) == 0 else " FAIL"))
    print("form=%s" % NAME, str(dtype)[6:], "Bt=1 refit", "  ".join(out))
