import sys, os, torch, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from bayesian_cbf_amd import ops
from bayesian_cbf_amd.synthetic import make_instances
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit
# argv[1]: 1 / 0 forces the super-panels on / off
SUP = {"1": ops.REFIT_SUPER_ON, "0": ops.REFIT_SUPER_OFF}.get(sys.argv[1] if len(sys.argv) > 1 else "", 0)
FORM = ops.REFIT_WAVE | SUP
out = {}
for Bt, N in ((1024, 512), (4096, 512), (1024, 1024)):
    p = make_instances(Bt, N, 3, 2, dtype=torch.float64, device="cuda", seed=5)
    out["%dx%d" % (Bt, N)] = round(timeit(lambda: ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], form=FORM), reps=5), 4)
    Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], p["jitter"], form=FORM)
    out["fails%dx%d" % (Bt, N)] = int((info != 0).sum())
print("super", sys.argv[1] if len(sys.argv) > 1 else "auto", json.dumps(out))
