"""The refit's launch form (bcbf.h: bcbf_refit_plan, a host function) on literal rows, both sides of every threshold of the
automatic rules and the forced-form semantics -- and the argument checks of the general entry bcbf_refit_form.  No GPU."""
import ctypes

import pytest

AUTO, WORKGROUP, WAVE, PAIR, TEAM4, TEAM8 = range(6)
SUPER_ON, SUPER_OFF, OCC1, OCC2 = 0x10, 0x20, 0x40, 0x80
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from bayesian_cbf_amd.build import build
    build()
    from bayesian_cbf_amd import _lib
    return _lib


def test_form_constants_match_the_header_and_ops(lib):
    import os
    import re
    from bayesian_cbf_amd import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bcbf.h")).read()
    defs = {k: int(v, 0) for k, v in re.findall(r"#define BCBF_FORM_(\w+) (\w+)", header)}
    assert defs == dict(AUTO=AUTO, WORKGROUP=WORKGROUP, WAVE=WAVE, PAIR=PAIR, TEAM4=TEAM4, TEAM8=TEAM8, SUPER_ON=SUPER_ON,
                        SUPER_OFF=SUPER_OFF, OCC1=OCC1, OCC2=OCC2)
    assert defs == {k[6:]: v for k, v in vars(ops).items() if k.startswith("REFIT_")}


def plan(lib, f64, Bt, N, cus=256, Kdense=0, Ldense=0, kind=0, form=AUTO):
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = lib.lib.bcbf_refit_plan(int(f64), Bt, N, cus, Kdense, Ldense, kind, form, out)
    return rc if rc != 0 else dict(form=out[0], waves=out[1], occ=out[2], sup=out[3])


# (f64, Bt, N, extra arguments) -> the fields of the plan that the row pins
ROWS = [
    # fp32, 256 CUs
    ((0, 1, 100, {}), dict(form=PAIR, waves=2)),
    ((0, 1, 512, {}), dict(form=TEAM8, waves=8)),
    ((0, 256, 256, {}), dict(form=TEAM8)),                            # one round of workgroups ...
    ((0, 257, 256, {}), dict(form=TEAM4, waves=4)),                   # ... one more instance: two workgroups per CU
    ((0, 512, 512, {}), dict(form=TEAM4)),
    ((0, 513, 512, {}), dict(form=WAVE, waves=1, occ=1, sup=1)),
    ((0, 2047, 256, {}), dict(form=WAVE, occ=1)),
    ((0, 2048, 256, {}), dict(form=WAVE, occ=2, sup=0)),              # 8 x cus instances: two waves per SIMD
    ((0, 4096, 512, {}), dict(form=WAVE, occ=2, sup=1)),
    ((0, 4096, 1024, {}), dict(form=WAVE, occ=1, sup=1)),             # N >= 1024: one wave with all registers
    ((0, 1024, 128, {}), dict(form=PAIR)),
    ((0, 1025, 128, {}), dict(form=WAVE)),
    ((0, 1024, 1024, {}), dict(form=WAVE)),
    ((0, 1024, 1024, dict(Ldense=1)), dict(form=TEAM8)),              # dense side: four rounds of the team
    ((0, 600, 544, {}), dict(form=WAVE)),
    ((0, 100, 2080, {}), dict(form=WORKGROUP, waves=8)),              # 65 block columns: past the team
    ((0, 200, 2080, {}), dict(form=WORKGROUP, waves=4)),
    ((0, 2, 40, dict(Ldense=1)), dict(form=WORKGROUP, waves=4)),
    ((0, 300, 256, dict(Kdense=1)), dict(form=WAVE, sup=0)),          # (the team of four never runs from a dense K_b)
    # both sides of the remaining fp32 thresholds
    ((0, 64, 512, dict(cus=64)), dict(form=TEAM8)),
    ((0, 128, 512, dict(cus=64)), dict(form=TEAM4)),                  # two rounds of 64 CUs hold 128: the team of four
    ((0, 128, 544, dict(cus=64)), dict(form=TEAM8)),                  # ... 17 block columns: of eight
    ((0, 129, 512, dict(cus=64)), dict(form=PAIR)),                   # the fp32 window 128 <= Bt <= 256 at N = 512
    ((0, 257, 512, dict(cus=64)), dict(form=WAVE, sup=1)),
    ((0, 127, 128, {}), dict(form=PAIR)),
    ((0, 127, 2080, {}), dict(form=WORKGROUP, waves=8)),              # workgroup width: Bt < 128 and N >= 128 (N, not Np)
    ((0, 128, 2080, {}), dict(form=WORKGROUP, waves=4)),
    ((0, 100, 127, dict(Ldense=1)), dict(form=WAVE)),                 # Np = 128: Bt >= 64
    ((0, 63, 127, dict(Ldense=1)), dict(form=WORKGROUP, waves=4)),    # N = 127 < 128
    ((0, 63, 128, dict(Ldense=1)), dict(form=WORKGROUP, waves=8)),
    ((0, 128, 2080, dict(cus=8)), dict(form=WORKGROUP)),
    ((0, 128, 512, dict(cus=8, Ldense=1)), dict(form=WAVE, sup=0)),   # Bt >= 128 and Np <= 512; dense output: plain panels
    ((0, 127, 544, dict(cus=8)), dict(form=WORKGROUP)),
    ((0, 256, 1024, dict(cus=8)), dict(form=WAVE)),                   # Bt >= 256 and Np <= 1024
    ((0, 255, 1024, dict(cus=8)), dict(form=WORKGROUP)),
    ((0, 1023, 1056, dict(cus=8)), dict(form=WORKGROUP)),
    ((0, 1024, 1056, dict(cus=8)), dict(form=WAVE)),
    ((0, 512, 2048, {}), dict(form=TEAM8)),                           # 64 block columns: the last the team takes
    ((0, 513, 1024, {}), dict(form=WAVE)),
    ((0, 513, 480, {}), dict(form=WAVE, sup=0)),                      # Np = 480 < 512: no super-panels
    # fp64
    ((1, 600, 300, {}), dict(form=WAVE, occ=1, sup=0)),
    ((1, 600, 544, {}), dict(form=WORKGROUP, waves=4)),
    ((1, 200, 200, {}), dict(form=PAIR)),
    ((1, 1024, 1024, {}), dict(form=WAVE, sup=1)),
    ((1, 4096, 512, {}), dict(form=WAVE, occ=1, sup=0)),              # fp64: one wave per SIMD, super-panels from 1024
    ((1, 60, 300, {}), dict(form=TEAM8)),
    ((1, 129, 512, dict(cus=64)), dict(form=WORKGROUP, waves=4)),     # no N = 512 window of the pair form in fp64
    ((1, 127, 255, dict(Ldense=1, cus=8)), dict(form=WORKGROUP, waves=4)),   # workgroup width in fp64: N >= 256
    ((1, 127, 256, dict(Ldense=1, cus=8)), dict(form=WORKGROUP, waves=8)),
    ((1, 511, 512, dict(cus=8)), dict(form=WORKGROUP)),
    ((1, 512, 512, dict(cus=8)), dict(form=WAVE)),
    ((1, 1023, 544, dict(cus=8)), dict(form=WORKGROUP)),
    ((1, 1024, 544, dict(cus=8)), dict(form=WAVE, sup=0)),
    ((1, 64, 128, dict(Ldense=1)), dict(form=WAVE)),
    ((1, 63, 128, dict(Ldense=1)), dict(form=WORKGROUP)),
    ((1, 1025, 256, {}), dict(form=WAVE)),
    ((1, 1024, 256, {}), dict(form=PAIR)),
    ((1, 1024, 257, {}), dict(form=WAVE)),                            # Np = 288 > 256
    # another CU count
    ((0, 200, 500, dict(cus=64)), dict(form=PAIR)),
    ((1, 200, 500, dict(cus=64)), dict(form=WORKGROUP, waves=4)),
    # the opt-in data kernels: always the team of eight
    ((0, 4096, 512, dict(kind=1)), dict(form=TEAM8, waves=8)),
    ((1, 4096, 512, dict(kind=2, Ldense=1)), dict(form=TEAM8)),
    ((0, 4096, 512, dict(kind=1, form=TEAM8)), dict(form=TEAM8)),
    ((0, 1, 8192, dict(kind=1)), dict(form=TEAM8)),
    # forced forms
    ((0, 4096, 512, dict(form=WORKGROUP)), dict(form=WORKGROUP, waves=4)),
    ((0, 1, 100, dict(form=WORKGROUP)), dict(form=WORKGROUP, waves=4)),      # (the pair rule does not override it)
    ((0, 1, 512, dict(form=WAVE)), dict(form=WAVE, occ=1, sup=1)),
    ((0, 1, 100, dict(form=PAIR)), dict(form=PAIR)),
    ((0, 9, 512, dict(form=PAIR)), dict(form=PAIR)),
    ((0, 9, 513, dict(form=PAIR)), dict(form=WAVE)),                  # 17 block columns
    ((0, 9, 100, dict(form=PAIR, Ldense=1)), dict(form=WAVE)),
    ((1, 9, 100, dict(form=PAIR, Kdense=1)), dict(form=WAVE)),
    ((0, 9, 100, dict(form=TEAM4, Kdense=1)), dict(form=TEAM8, waves=8)),
    ((0, 9, 100, dict(form=TEAM4, Ldense=1)), dict(form=TEAM4, waves=4)),
    ((0, 1, 8192, dict(form=TEAM8)), dict(form=TEAM8)),
    ((1, 6, 512, dict(form=WAVE | SUPER_ON)), dict(form=WAVE, sup=1)),
    ((1, 6, 512, dict(form=WAVE | SUPER_ON, Ldense=1)), dict(form=WAVE, sup=1)),
    ((1, 6, 512, dict(form=WAVE | SUPER_ON, Kdense=1)), dict(form=WAVE, sup=0)),
    ((1, 6, 1024, dict(form=WAVE | SUPER_OFF)), dict(form=WAVE, sup=0)),
    ((0, 6, 512, dict(form=WAVE | OCC2)), dict(form=WAVE, occ=2)),
    ((0, 4096, 512, dict(form=WAVE | OCC1)), dict(form=WAVE, occ=1)),
    ((1, 6, 512, dict(form=WAVE | OCC2)), dict(form=WAVE, occ=1)),    # fp64 runs one wave per SIMD
    ((0, 4096, 512, dict(form=AUTO | OCC1 | SUPER_OFF)), dict(form=WAVE, occ=1, sup=0)),   # sub-forms of whatever is chosen
]
REFUSED = [
    (0, 1, 8200, dict(kind=1)),                    # 257 block columns
    (0, 1, 8200, dict(form=TEAM8)),
    (1, 1, 8200, dict(form=TEAM4)),
    (0, 9, 100, dict(kind=1, form=WAVE)),
    (0, 9, 100, dict(kind=2, form=TEAM4)),
    (0, 9, 100, dict(kind=1, Kdense=1)),
    (0, 9, 100, dict(kind=3)),
    (0, 9, 100, dict(kind=-1)),
    (0, 9, 100, dict(form=6)),
    (0, 9, 100, dict(form=-1)),
    (0, 9, 100, dict(form=WAVE | SUPER_ON | SUPER_OFF)),
    (0, 9, 100, dict(form=WAVE | OCC1 | OCC2)),
    (0, 9, 100, dict(form=0x100)),
    (0, 9, 0, {}),
]
_rid = lambda r: "%s-%dx%d-%s" % ("f64" if r[0] else "f32", r[1], r[2], ",".join("%s=%s" % kv for kv in r[3].items()) or "auto")  # noqa: E731


@pytest.mark.parametrize("row, want", ROWS, ids=[_rid(r) for r, _ in ROWS])
def test_refit_plan_rows(lib, row, want):
    f64, Bt, N, extra = row
    got = plan(lib, f64, Bt, N, **extra)
    assert isinstance(got, dict), "refused (rc=%s): %s" % (got, lib.lib.bcbf_last_error())
    assert {k: got[k] for k in want} == want, got
    assert got["form"] != AUTO and (got["form"] == WAVE or (got["occ"], got["sup"]) == (0, 0))


@pytest.mark.parametrize("row", REFUSED, ids=[_rid(r) for r in REFUSED])
def test_refit_plan_refuses(lib, row):
    f64, Bt, N, extra = row
    assert plan(lib, f64, Bt, N, **extra) == EINVAL
    assert lib.lib.bcbf_last_error().startswith(b"refit: ")


def test_refit_plan_refuses_a_null_output(lib):
    assert lib.lib.bcbf_refit_plan(0, 1, 100, 256, 0, 0, 0, AUTO, None) == EINVAL


# ---------------------------------------------------------------- bcbf_refit_form: the argument checks
# Every call below passes Bt = 0: the argument checks of this entry run first, so a refused call returns BCBF_EINVAL, and a
# call that passes its checks returns at once without touching the device (the fake pointers are never dereferenced).
FAKE, FAKE2 = ctypes.c_void_p(4096), ctypes.c_void_p(8192)


def _form_args(**over):
    a = dict(X=FAKE, UH=FAKE, Bm=FAKE, ell=FAKE, s2=FAKE, jitter=FAKE, Kdense=None, Lop=FAKE, UHB=FAKE, Ldense=None,
             prev_info=None, info=FAKE, Bt=0, N=100, n=3, m=2, kernel_kind=0, form=AUTO, stream=None)
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    return list(a.values())


_DENSE = dict(X=None, UH=None, Bm=None, ell=None, s2=None, jitter=None, UHB=None, n=0, m=0, Kdense=FAKE)     # bcbf_potrf's call
FORM_OK = [dict(), dict(jitter=None), dict(Ldense=FAKE), dict(prev_info=FAKE2), dict(n=1, m=1), dict(n=8, m=3), dict(N=1),
           dict(N=8192, form=TEAM8), dict(kernel_kind=1), dict(kernel_kind=2, form=TEAM8), dict(kernel_kind=2, Ldense=FAKE),
           dict(form=WORKGROUP), dict(form=WAVE | SUPER_ON | OCC2), dict(form=PAIR), dict(form=TEAM4), dict(Bt=-1),
           _DENSE, dict(_DENSE, Ldense=FAKE, form=WAVE), dict(_DENSE, form=TEAM4)]
FORM_BAD = [dict(X=None), dict(UH=None), dict(Bm=None), dict(ell=None), dict(s2=None), dict(UHB=None), dict(Lop=None),
            dict(info=None), dict(N=0), dict(N=-3), dict(n=0), dict(n=9), dict(m=0), dict(m=4), dict(prev_info=FAKE),   # prev_info == info
            dict(kernel_kind=3), dict(kernel_kind=-1), dict(form=6), dict(form=-1), dict(form=0x100), dict(form=WAVE | 0x30),
            dict(form=WAVE | 0xc0), dict(kernel_kind=1, form=WAVE), dict(kernel_kind=2, form=PAIR), dict(kernel_kind=1, Kdense=FAKE),
            dict(N=8200, form=TEAM8), dict(N=8200, form=TEAM4), dict(N=8200, kernel_kind=1), dict(_DENSE, Lop=None),
            dict(_DENSE, info=None), dict(_DENSE, N=0)]
_ids = lambda d: ",".join("%s=%s" % (k, "ptr" if isinstance(v, ctypes.c_void_p) else v) for k, v in d.items()) or "default"  # noqa: E731


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("ok", FORM_OK, ids=_ids)
def test_refit_form_valid_arguments_pass_the_checks(lib, suf, ok):
    assert getattr(lib.lib, "bcbf_refit_form" + suf)(*_form_args(**ok)) == 0


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
@pytest.mark.parametrize("bad", FORM_BAD, ids=_ids)
def test_refit_form_refuses_bad_arguments(lib, suf, bad):
    assert getattr(lib.lib, "bcbf_refit_form" + suf)(*_form_args(**bad)) == EINVAL


@pytest.mark.parametrize("suf", ["_f32", "_f64"])
def test_named_refit_entries_return_ok_for_an_empty_batch_before_any_check(lib, suf):
    """bcbf_refit, bcbf_refit_retry[_kind], bcbf_refit_matern52 / _rbfm52 and bcbf_potrf have always answered Bt <= 0 with
    BCBF_OK without looking at another argument; callers hand them the null pointers of empty tensors."""
    L = lib.lib
    for name in ("bcbf_refit", "bcbf_refit_matern52", "bcbf_refit_rbfm52"):
        assert getattr(L, name + suf)(*[None] * 10, 0, 0, 0, 0, None) == 0
    assert getattr(L, "bcbf_refit_retry" + suf)(*[None] * 10, 0, 0, 0, 0, None) == 0
    assert getattr(L, "bcbf_refit_retry_kind" + suf)(*[None] * 10, -1, 0, 0, 0, 7, None) == 0
    assert getattr(L, "bcbf_potrf" + suf)(None, None, None, None, 0, 0, None) == 0
