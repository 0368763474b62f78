"""The fp32 control-step form of the posterior stream at every boundary of its block loops (csrc/posterior_step.hip,
BCBF_PS_TAIL): both sides at 8 columns per stage while a wave's A-side rows are live, then the B side alone with the whole
block (32 columns) in flight.  The shapes are the smallest at which each loop boundary exists or can be mis-indexed:

    N = 32    one block, nothing streamed              N = 288, 320   the A / B split lands inside the matrix (4 two-sided
    N = 64    first block with rows below it                          blocks; the last A-side rows fill half / all of block 4)
    N = 160   two two-sided blocks, then fewer than    N = 416        an odd block count (13)
              128 rows below every B-only block        N = 500        Np = 512, identity padding inside the last block
                                                       N = 512        the headline shape

`ops.posterior_step` and `bcbf_unicycle_control_step` (through the C ABI) against the CPU oracle (oracle/gp_posterior.py, fp64) at
the tolerances tests/test_gpu_parity.py and tests/test_gpu_configs.py apply to the same entry points (fp32: 1e-3 of the quantity's
scale).  The oracle's refactorisation is computed once per N for three instances (first, third, last of the batch of 65; the
batch of 3 is its first three instances) and shared; every instance of both batches is also held, at the same tolerance, to the
library's fp64 stream on the same data (whose kernel has one stage depth throughout).  fp64 keeps its schedule, so it has no
cases of its own here."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import control_step as ostep
from oracle import gp_posterior as ogp

DEV = "cuda"
n_, m_ = 3, 2
BT = 65
ORACLE_INSTANCES = (0, 2, 64)
SIZES = [32, 64, 160, 288, 320, 416, 500, 512]
TOL = 1e-3                      # fp32, relative to the scale of the quantity (BASELINE.json north_star; test_gpu_parity.TOL)
PLANT = dict(dt=1e-3, L_true=1.0, L_mean=4.0, clf_gamma=10.0, max_iters=20)       # bench.py's arguments


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bayesian_cbf_amd import ops as _ops
    return _ops


def host(t):
    return t.detach().cpu().double().numpy()


from _tolreport import rel_close  # noqa: E402


def _refit_with_retry(ops, p):
    """make_psd's x10 retry on the failing instances (control_affine_model.py:899-921), as bench.py does."""
    jit = p["jitter"]
    for _ in range(4):
        Lop, UHB, info, _ = ops.refit(p["X"], p["UH"], p["Bm"], p["ell"], p["s2"], jit)
        bad = info != 0
        if not bool(bad.any()):
            break
        jit = torch.where(bad[:, None], jit * 10, jit).contiguous()
    assert int((info != 0).sum()) == 0
    return Lop, UHB, jit


@functools.lru_cache(maxsize=None)
def _state(N):
    """Per N, once: 65 fp32 instances, their device factor, the same data factored in fp64 on the device, and the oracle's
    refactorisation of ORACLE_INSTANCES."""
    from bayesian_cbf_amd import ops
    from bayesian_cbf_amd.synthetic import make_instances
    p = make_instances(BT, N, n_, m_, dtype=torch.float32, device=DEV, seed=300 + N)
    Lop, UHB, jit = _refit_with_retry(ops, p)
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    p64 = {k: v.double().contiguous() for k, v in p.items()}
    Lop64, UHB64, info64, _ = ops.refit(p64["X"], p64["UH"], p64["Bm"], p64["ell"], p64["s2"], jit.double().contiguous())
    assert (info64 == 0).all()
    Vw64, _ = ops.potrs(Lop64, p64["Xdot"], p64["UH"], p64["M0"], want_alpha=False)
    h = {k: host(v) for k, v in p.items()}
    hj = host(jit)
    st = {i: ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i], hj[i][None] / 1e-5)
          for i in ORACLE_INSTANCES}
    return dict(p=p, p64=p64, h=h, Lop=Lop, UHB=UHB, Vw=Vw, Lop64=Lop64, UHB64=UHB64, Vw64=Vw64, st=st)


def _cut(d, Bt, keys):
    return {k: d[k][:Bt].contiguous() for k in keys}


def _oracle_posterior(s, i, xq):
    h, st = s["h"], s["st"][i]
    return ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][i][None], st["UHB"][None], h["ell"][i][None],
                              h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None], xq[None])


def _check_posterior(s, Bt, Mk, Bk, xq, Mk64, Bk64, own_relative):
    """Mk, Bk of the first Bt instances: ORACLE_INSTANCES against the oracle, all against the fp64 stream."""
    h = s["h"]
    Mk_d, Bk_d, Mk_r, Bk_r, xq_h = host(Mk), host(Bk), host(Mk64), host(Bk64), host(xq)
    assert np.isfinite(Mk_d).all() and np.isfinite(Bk_d).all()
    for i in range(Bt):
        prior = float(h["s2"][i] * np.abs(h["Bm"][i]).max())
        rel_close(Mk_d[i], Mk_r[i], TOL, scale=max(1.0, np.abs(Mk_r[i]).max()), what="Mk[%d] vs fp64 stream" % i)
        rel_close(Bk_d[i], Bk_r[i], TOL, scale=prior, what="Bk[%d] vs fp64 stream" % i)
    out = {}
    for i in ORACLE_INSTANCES:
        if i >= Bt:
            continue
        Mk_o, Bk_o = _oracle_posterior(s, i, xq_h[i])
        prior = float(h["s2"][i] * np.abs(h["Bm"][i]).max())
        rel_close(Mk_d[i], Mk_o[0], TOL, scale=max(1.0, np.abs(Mk_o).max()), what="Mk[%d]" % i)
        rel_close(Bk_d[i], Bk_o[0], TOL, scale=prior, what="Bk[%d]" % i)
        if own_relative:       # the control step's check in test_gpu_configs: relative to B_k's own magnitude
            rel_close(Bk_d[i], Bk_o[0], TOL, scale=float(np.abs(Bk_o[0]).max()), what="Bk own-relative[%d]" % i)
        out[i] = (Mk_o[0], Bk_o[0])
    return out


@pytest.mark.parametrize("Bt", [3, BT])
@pytest.mark.parametrize("N", SIZES)
def test_posterior_step_at_every_loop_boundary_vs_oracle(ops, N, Bt):
    s = _state(N)
    keys = ("X", "ell", "s2", "Bm", "M0", "xq")
    p, p64 = _cut(s["p"], Bt, keys), _cut(s["p64"], Bt, keys)
    Mk, Bk = ops.posterior_step(s["Lop"][:Bt].contiguous(), s["Vw"][:Bt].contiguous(), p["X"], s["UHB"][:Bt].contiguous(), p["ell"],
                                p["s2"], p["Bm"], p["M0"], p["xq"])
    Mk64, Bk64 = ops.posterior_step(s["Lop64"][:Bt].contiguous(), s["Vw64"][:Bt].contiguous(), p64["X"], s["UHB64"][:Bt].contiguous(),
                                    p64["ell"], p64["s2"], p64["Bm"], p64["M0"], p64["xq"])
    _check_posterior(s, Bt, Mk, Bk, p["xq"], Mk64, Bk64, own_relative=False)


@pytest.mark.parametrize("Bt", [3, BT])
@pytest.mark.parametrize("N", SIZES)
def test_control_step_at_every_loop_boundary_vs_oracle(ops, N, Bt):
    """`bcbf_unicycle_control_step`: its posterior launch (query = the state) and, for the oracle's instances, the control, the
    solver status in both directions and the next state, as tests/test_gpu_configs.py checks them at N = 512."""
    from bayesian_cbf_amd.synthetic import make_unicycle_task
    s = _state(N)
    keys = ("X", "ell", "s2", "Bm", "M0", "A")
    p, p64 = _cut(s["p"], Bt, keys), _cut(s["p64"], Bt, keys)
    task = make_unicycle_task(Bt, dtype=torch.float32, device=DEV, seed=99)
    gp = dict(Lop=s["Lop"][:Bt].contiguous(), Vw=s["Vw"][:Bt].contiguous(), UHB=s["UHB"][:Bt].contiguous(), **p)
    x = task["x"].clone()
    ws = ops.control_workspace(Bt, 2, torch.float32, DEV)
    ops.unicycle_control_step(gp, task, ws, x, **PLANT)
    torch.cuda.synchronize()
    Mk64, Bk64 = ops.posterior_step(s["Lop64"][:Bt].contiguous(), s["Vw64"][:Bt].contiguous(), p64["X"], s["UHB64"][:Bt].contiguous(),
                                    p64["ell"], p64["s2"], p64["Bm"], p64["M0"], task["x"].double().contiguous())
    post = _check_posterior(s, Bt, ws["Mk"], ws["Bk"], task["x"], Mk64, Bk64, own_relative=True)
    h = {**s["h"], **{k: host(v) for k, v in task.items()}}
    y, st, xn = host(ws["y"]), ws["status"].cpu().numpy(), host(x)
    for i, (Mk_o, Bk_o) in post.items():
        o = ostep.control_step(h["x"][i], h["plan"][i], h["dot_plan"][i], Mk_o, Bk_o, h["A"][i], h["Kp"], 10.0, h["centers"][i],
                               h["radii"][i], h["tw"], h["gammas"], PLANT["L_mean"], h["w"][i], h["r"][i], h["rho"][i],
                               h["relax_mask"], dt=PLANT["dt"], L_true=PLANT["L_true"])
        dev_ok, ora_ok = st[i] == 0, o["status"] == "optimal"
        if dev_ok != ora_ok:        # allowed only on the numerical feasibility boundary (test_gpu_configs: band 2e-3 in fp32)
            assert o["cones"] is not None, "instance %d: the oracle cannot factor a cone the device accepted" % i
            loose, tight = ostep.shifted_status(o, h["w"][i], h["r"][i], h["rho"][i], h["relax_mask"], 2e-3)
            assert (loose == "optimal") != (tight == "optimal"), (i, int(st[i]), o["status"], loose, tight)
            continue
        if not ora_ok:
            np.testing.assert_array_equal(xn[i], h["x"][i].astype(np.float32), err_msg="unsolved instance %d must keep its state" % i)
            continue
        scale = max(1.0, np.abs(o["sol"]["x"]).max())
        err = np.abs(y[i] - o["sol"]["x"]).max() / scale
        assert err <= TOL, "instance %d: |y - y_oracle| = %.3e of scale %.2f" % (i, err, scale)
        np.testing.assert_allclose(xn[i], o["x_next"], rtol=0, atol=4e-6 * max(1.0, np.abs(o["x_next"]).max()))


def test_reserved_layout_300_live_points_in_capacity_512_vs_oracle(ops):
    """Capacity-reserving storage (`ops.ReservedGP`): the operator is laid out for 512 points, 300 are live (Nl > Np, ldN > N) --
    the column addressing follows the layout, the loop bounds the live size (Np = 320: 4 two-sided blocks, 6 B-only)."""
    from bayesian_cbf_amd.synthetic import make_instances
    Bt, N, cap = 3, 300, 512
    p = make_instances(Bt, N, n_, m_, dtype=torch.float32, device=DEV, seed=41)
    Lop, UHB, jit = _refit_with_retry(ops, p)
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    g = ops.ReservedGP(Lop, Vw, p["X"], UHB, p["ell"], p["s2"], p["Bm"], p["M0"], cap)
    assert g.N == N and g.capacity == cap
    Mk, Bk = g.posterior(p["xq"])
    h = {k: host(v) for k, v in p.items()}
    hj = host(jit)
    for i in range(Bt):
        st = ogp.refit_state(h["X"][i], h["U"][i], h["Xdot"][i], h["Bm"][i], h["ell"][i], h["s2"][i], h["M0"][i], hj[i][None] / 1e-5)
        Mk_o, Bk_o = ogp.posterior_step(st["L"][None], st["alpha"][None], h["X"][i][None], st["UHB"][None], h["ell"][i][None],
                                        h["s2"][i][None], h["Bm"][i][None], h["M0"][i][None], h["xq"][i][None])
        prior = float(h["s2"][i] * np.abs(h["Bm"][i]).max())
        rel_close(host(Mk)[i], Mk_o[0], TOL, scale=max(1.0, np.abs(Mk_o).max()), what="Mk[%d]" % i)
        rel_close(host(Bk)[i], Bk_o[0], TOL, scale=prior, what="Bk[%d]" % i)


def test_part_batches_equal_single_stream_entry(ops):
    """`ConcurrentControlLoop(parts=3)` and the single-stream entry run the same launches on slices of the batch: after 5
    closed-loop steps at Bt = 65, N = 96 states, statuses, iteration counts and the solved controls are identical."""
    from bayesian_cbf_amd.synthetic import make_instances, make_unicycle_task
    Bt, N, steps = BT, 96, 5
    p = make_instances(Bt, N, n_, m_, dtype=torch.float32, device=DEV, seed=21)
    task = make_unicycle_task(Bt, dtype=torch.float32, device=DEV, seed=22)
    Lop, UHB, _ = _refit_with_retry(ops, p)
    Vw, _ = ops.potrs(Lop, p["Xdot"], p["UH"], p["M0"], want_alpha=False)
    gp = dict(Lop=Lop, Vw=Vw, X=p["X"], UHB=UHB, ell=p["ell"], s2=p["s2"], Bm=p["Bm"], M0=p["M0"], A=(0.05 * p["A"]).contiguous())
    kw = dict(dt=0.02, L_true=2.0, L_mean=4.0, clf_gamma=10.0, max_iters=30)
    x1, x2 = task["x"].clone(), task["x"].clone()
    ws = ops.control_workspace(Bt, 2, torch.float32, DEV)
    for _ in range(steps):
        ops.unicycle_control_step(gp, task, ws, x1, **kw)
    torch.cuda.synchronize()
    loop = ops.ConcurrentControlLoop(gp, task, x2, parts=3, **kw)
    for _ in range(steps):
        loop.step()
    loop.synchronize()
    assert torch.equal(x1, x2)
    assert torch.equal(ws["status"], loop.status) and torch.equal(ws["iters"], loop.iters)
    ok = ws["status"] == 0
    assert int(ok.sum()) > Bt // 2 and torch.equal(ws["y"][ok], loop.y[ok])
    assert float((x1 - task["x"]).abs().max()) > 1e-3            # the loops did move
