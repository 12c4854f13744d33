"""The GEMM argument check and the exact-sum GEMM cases without a GPU.

aigv_gemm_check (aigv_op_gemm / _rows / _splitk*) and run_skinny's check refuse, with AIGV_ERR_ARG and a message naming the problem, every
row stride their kernels cannot take - before anything reaches the device (the pointers below have no memory behind them; the
_check entry points launch nothing).  Every layout tests/test_gpu_gemm_layouts.py runs is accepted up to the point of launch, the
cost-model shapes show their feature in aigv_plan_gemm, and every case of that file is exact (tests/gemm_exact_reference.py)."""
import ctypes
import os
import re

import pytest
import torch

import gemm_exact_reference as GX
from aigv_assessor_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = native._P, native._I
FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it
NEW = ("aigv_op_gemm_check", "aigv_op_skinny_gemm_check", "aigv_gemm_route")


@pytest.fixture(scope="module")
def lib():
    return native.load()


def test_the_check_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in native.PROTOTYPES, name
        getattr(lib, name)
    assert "multiples of 8" in header.split("int aigv_op_gemm(")[0][-900:]          # the rule stands next to the prototype


def gemm_check(lib, M=300, N=256, K=128, epi=0, lda=None, ldw=None, ldc=None, ldr=None, resid=None, A=FAKE, C=FAKE):
    no = GX.n_out(N, epi)
    if epi in (2, 3) and resid is None:
        resid = FAKE
    return lib.aigv_op_gemm_check(A, K if lda is None else lda, FAKE, K if ldw is None else ldw, C, no if ldc is None else ldc, None,
                                  FAKE if epi == 2 else None, resid, (no if ldr is None else ldr) if resid else 0,
                                  FAKE if epi == 5 else None, M if epi == 5 else 0, M, N, K, epi)


def refused(lib, rc, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG
    assert msg.startswith("gemm:") or msg.startswith("skinny gemm:"), msg
    assert re.search(what, msg), msg


def test_gemm_check_refuses_what_the_kernels_cannot_take(lib):
    assert gemm_check(lib) == 0
    refused(lib, gemm_check(lib, ldc=248), r"ldc is below N \(rows would overlap\)")
    refused(lib, gemm_check(lib, ldc=0), r"ldc is below N")
    refused(lib, gemm_check(lib, epi=4, ldc=120), r"swiglu output is N/2 wide: ldc is below it")
    assert gemm_check(lib, epi=4, ldc=128) == 0
    refused(lib, gemm_check(lib, ldc=260), r"ldc must be a multiple of 8")        # 8-byte aligned rows: enough for the 128 kernel only
    refused(lib, gemm_check(lib, ldc=257), r"ldc must be a multiple of 8")
    for epi in (2, 3):
        assert gemm_check(lib, epi=epi) == 0
        refused(lib, gemm_check(lib, epi=epi, ldr=248), r"ldr is below the width of the residual rows")
        refused(lib, gemm_check(lib, epi=epi, ldr=0), r"ldr is below")
        refused(lib, gemm_check(lib, epi=epi, ldr=260), r"ldr must be a multiple of 8")
    refused(lib, gemm_check(lib, epi=0, resid=FAKE, ldr=100), r"ldr is below")    # a residual that is given is checked, whatever the epilogue
    assert gemm_check(lib, epi=0, ldr=0) == 0                                      # none given: ldr is not looked at
    refused(lib, gemm_check(lib, lda=120), r"lda and ldw: at least K, multiples of 8")
    refused(lib, gemm_check(lib, ldw=132), r"lda and ldw")
    refused(lib, gemm_check(lib, N=200), r"N must be a multiple of 128")
    refused(lib, gemm_check(lib, K=96), r"K must be a multiple of 64")
    refused(lib, gemm_check(lib, A=None), r"null operand")
    refused(lib, lib.aigv_op_gemm_check(FAKE, 128, FAKE, 128, FAKE, 256, None, None, None, 0, None, 0, 300, 256, 128, 3), r"residual epilogue needs resid")
    # the same refusal through the operators themselves, before any launch
    for op in (lib.aigv_op_gemm_splitk, lib.aigv_op_gemm_splitk256):
        refused(lib, op(FAKE, 128, FAKE, 128, FAKE, 260, None, None, None, 0, 300, 256, 128, 0, 2, FAKE, None), r"ldc must be a multiple of 8")
    refused(lib, lib.aigv_op_gemm(FAKE, 128, FAKE, 128, FAKE, 256, None, None, FAKE, 252, None, 0, 300, 256, 128, 3, None), r"ldr is below")


def skinny_check(lib, R=5, N=288, K=512, epi=0, ldx=None, ldw=None, ldo=None, ldr=None, resid=None, x=FAKE):
    no = N // 2 if epi == 2 else N
    if epi == 1 and resid is None:
        resid = FAKE
    return lib.aigv_op_skinny_gemm_check(x, K if ldx is None else ldx, R, FAKE, K if ldw is None else ldw, N, K, resid,
                                         (no if ldr is None else ldr) if resid else 0, FAKE, no if ldo is None else ldo, epi)


def test_skinny_check_refuses_what_the_kernel_cannot_take(lib):
    for epi in (0, 1, 2, 3):
        assert skinny_check(lib, epi=epi) == 0
    refused(lib, skinny_check(lib, ldo=284), r"ldo is below the output width")
    refused(lib, skinny_check(lib, epi=2, ldo=140), r"ldo is below the output width")
    refused(lib, skinny_check(lib, ldo=290), r"ldo must be a multiple of 4")
    assert skinny_check(lib, ldo=292) == 0                                           # 8-byte rows are enough for this kernel
    refused(lib, skinny_check(lib, epi=1, ldr=284), r"ldr is below the width of the residual rows")
    refused(lib, skinny_check(lib, epi=1, ldr=290), r"ldr must be a multiple of 4")
    refused(lib, skinny_check(lib, ldx=504), r"ldx and ldw: at least K, multiples of 8")
    refused(lib, skinny_check(lib, ldw=516), r"ldx and ldw")
    refused(lib, skinny_check(lib, x=None), r"null operand")
    refused(lib, skinny_check(lib, R=65), r"more than 64 rows")
    refused(lib, skinny_check(lib, K=576), r"K must be a multiple of 128")
    refused(lib, lib.aigv_op_skinny_gemm_check(FAKE, 512, 5, FAKE, 512, 288, 512, None, 0, FAKE, 288, 1), r"residual epilogue needs resid")
    refused(lib, lib.aigv_op_skinny_gemm(FAKE, 512, 5, FAKE, 512, 288, 512, None, FAKE, 284, FAKE, 288, 1, None), r"ldr is below")


tile_cases, skinny_cases = GX.tile_cases, GX.skinny_cases


def test_the_route_record_is_empty_until_something_is_launched(lib):
    """aigv_gemm_route: host only; a refused call launches nothing and leaves no mark."""
    lib.aigv_gemm_route(1)
    refused(lib, lib.aigv_op_gemm(FAKE, 128, FAKE, 128, FAKE, 260, None, None, None, 0, None, 0, 300, 256, 128, 0, None), r"ldc must be a multiple of 8")
    assert lib.aigv_gemm_route(0) == 0 and lib.aigv_gemm_route(1) == 0
    names = re.findall(r"AIGV_ROUTE_\w+ = (\d+)", open(os.path.join(ROOT, "include", "aigv_amd.h")).read())
    assert [int(v) for v in names] == [1 << i for i in range(15)]                   # the values tests/test_gpu_gemm_layouts.py spells out


def test_the_layouts_of_the_gpu_tests_are_accepted(lib):
    for M, N, K, epi in tile_cases():
        no = GX.n_out(N, epi)
        lda, ldw, ldc, ldr = GX.strides(no, K)
        resid = FAKE if epi in (2, 3) else None
        for r, ld_r in ((resid, ldr), (FAKE + 64 if resid else None, ldc)):                                   # its own buffer; in place (the address only has to be non-null)
            rc = lib.aigv_op_gemm_check(FAKE, lda, FAKE, ldw, FAKE + 64, ldc, FAKE if epi in (0, 1, 2, 5) else None, FAKE if epi == 2 else None, r,
                                        ld_r if r else 0, FAKE if epi == 5 else None, GX.patch_np(M) if epi == 5 else 0, M, N, K, epi)
            assert rc == 0, (M, N, K, epi, lib.aigv_last_error(None))
    for R, N, K, epi in skinny_cases():
        no = GX.n_out(N, epi)
        ldx, ldw, ldo, ldr = GX.strides(no, K, ldo_pad=12)
        resid = FAKE if epi == 3 else None
        rc = lib.aigv_op_skinny_gemm_check(FAKE, ldx, R, FAKE, ldw, N, K, resid, ldr if resid else 0, FAKE, ldo, GX.SK_OF[epi])
        assert rc == 0, (R, N, K, epi, lib.aigv_last_error(None))


def test_the_cost_model_still_plans_every_feature(lib):
    """Host only (aigv_plan_gemm): the GPU test asserts the same before it runs; here a change of the model fails without a GPU too."""
    for feature, (M, N, K, epi, shows) in GX.COST_MODEL.items():
        plan = (ctypes.c_int * 7)()
        assert lib.aigv_plan_gemm(M, N, K, epi, plan, None) == 0
        assert shows(list(plan)), (feature, list(plan))


SMALL = [c for c in tile_cases() if c[0] * c[1] * c[2] <= 1 << 28]
LARGE = [c for c in tile_cases() if c[0] * c[1] * c[2] > 1 << 28]


def test_every_small_case_is_exact_and_distinguishes_positions():
    for M, N, K, epi in SMALL:
        case = GX.exact_case(M, N, K, epi)
        assert GX.is_exact(case), (M, N, K, epi)
        assert GX.distinguishes_positions(case, case["want"]), (M, N, K, epi)
        assert case["want"].shape == (M, GX.n_out(N, epi)) and case["want"].dtype == torch.bfloat16
    for R, N, K, epi in skinny_cases():
        assert GX.is_exact(GX.exact_case(R, N, K, epi)), (R, N, K, epi)


def test_the_cross_route_cases_are_exact():
    """The GELU and the SwiGLU case every route must agree on bit for bit, and the rows of them the skinny kernel takes."""
    assert sum(GX.CROSS_ROUTE_LENS) == GX.CROSS_ROUTE[0][0] and [c[3] for c in GX.CROSS_ROUTE] == [1, 4]
    assert sum(GX.CROSS_ROUTE_TAIL_LENS) == GX.CROSS_ROUTE[0][0] and GX.CROSS_ROUTE_TAIL_LENS[-1] % 256 > 128          # a tile tail above 128 rows
    for M, N, K, epi in GX.CROSS_ROUTE:
        assert (M, N, K, epi) in tile_cases()
        case = GX.exact_case(M, N, K, epi)
        assert GX.is_exact(case), (M, N, K, epi)
        sub = GX.first_rows(case, GX.CROSS_ROUTE_SKINNY_ROWS)
        assert GX.is_exact(sub) and sub["want"].shape == (GX.CROSS_ROUTE_SKINNY_ROWS, GX.n_out(N, epi))
        assert torch.equal(GX.want(sub), sub["want"])


@pytest.mark.parametrize("M,N,K,epi", LARGE)
def test_every_large_case_is_exact(M, N, K, epi):
    case = GX.exact_case(M, N, K, epi)
    assert GX.is_exact(case)


def test_an_exact_case_has_one_result_in_every_order_of_summation():
    """The point of the bound: fp32 sums over any split of K, in either direction, give ``want``'s bits."""
    for epi in (0, 2, 3):
        case = GX.exact_case(300, 384, 192, epi)
        A, W = case["A"].float(), case["W"].float()
        acc = torch.zeros(300, 384)
        for k0 in (128, 0, 64):                                                      # three slabs, out of order
            acc = acc + A[:, k0:k0 + 64].flip(1) @ W[:, k0:k0 + 64].flip(1).t()
        y = acc + (case["bias"].float() if case["bias"] is not None else 0)
        assert torch.equal(y.to(torch.bfloat16).float(), y) and torch.equal(y.double(), GX.linear(case))


def test_is_exact_refuses_an_inexact_case():
    case = dict(GX.exact_case(129, 128, 64, 0))
    assert GX.is_exact(case)
    bad = dict(case)
    bad["A"] = case["A"].clone()
    bad["A"][5, :] = 2.0                                                             # a row whose sums of magnitudes pass 2^8 quanta
    bad["W"] = case["W"].clone()
    bad["W"][7, :] = 2.0
    assert not GX.is_exact(bad)
    odd = dict(case)
    odd["bias"] = case["bias"].clone()
    odd["bias"][3] = 0.125                                                           # off the grid of the products
    assert not GX.is_exact(odd)
    wide = dict(GX.exact_case(129, 128, 64, 1))
    wide["bias"] = wide["bias"].clone()
    wide["bias"][:] = 4.0                                                            # GELU arguments beyond |x| <= 4
    assert not GX.is_exact(wide)
    r = dict(GX.exact_case(129, 128, 64, 3))
    r["resid"] = r["resid"].clone()
    r["resid"][0, 0] = 100.0
    assert not GX.is_exact(r)


def test_want_distinguishes_positions_and_the_generator_says_when_it_does_not():
    case = GX.exact_case(300, 384, 192, 3)
    w = case["want"]
    assert GX.distinguishes_positions(case, w)
    shifted = w.clone()
    shifted[1] = w[0]
    assert not GX.distinguishes_positions(case, shifted)                             # two equal neighbouring rows
    same_seg = w.clone()
    same_seg[:, 4:8] = w[:, 0:4]
    assert not GX.distinguishes_positions(case, same_seg)
    assert not GX.distinguishes_positions(case, case["resid"].clone())               # a row equal to its residual row


def test_the_fp8_form_of_every_case_is_exact_and_an_odd_scale_is_not():
    for M, N, K in GX.SHAPES_FP8:
        for epi in range(5):
            case = GX.exact_case(M, N, K, epi)
            ops = GX.fp8_operands(case)
            assert GX.fp8_is_exact(case, ops), (M, N, K, epi)
            # what the kernel computes, in float64: the scaled sum of the e4m3 products IS the bf16 case's sum
            acc = (ops["A8"].double() @ ops["W8"].double().t()) * ops["row_scale"].double()[:, None] * ops["col_scale"].double()[None, :]
            assert torch.equal(acc, case["A"].double() @ case["W"].double().t())
            assert len(set(ops["row_scale"].tolist())) == min(3, M) and len(set(ops["col_scale"].tolist())) == 3
    case = GX.exact_case(257, 256, 128, 0)
    bad = dict(GX.fp8_operands(case))
    bad["row_scale"] = bad["row_scale"].clone()
    bad["row_scale"][4] = 3.0                                                        # no power of two
    assert not GX.fp8_is_exact(case, bad)
    off = dict(GX.fp8_operands(case))
    off["W8"] = (off["W8"].float() * 2).to(torch.float8_e4m3fn)                      # operands that are not the case's
    assert not GX.fp8_is_exact(case, off)
