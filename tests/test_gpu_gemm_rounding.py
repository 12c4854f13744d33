"""The rounding points of the GEMM family, on every dispatch route (MI355X only).  tests/test_gpu_gemm_layouts.py pins addressing with sums
that never round, tests/test_gpu_ops.py allows two ulps on a few per cent of random elements: neither sees a wrong rounding DECISION -
truncation, round-half-up, a layer-scale or residual stage fused onto the unrounded accumulator, a packed pair whose halves round
differently, a split-K slab that is rounded, flushed subnormals, saturation instead of Inf, a lost sign of zero.

The cases are those of tests/gemm_rounding_reference.py: every accumulator is exact in any summation order (asserted here and in
tests/test_gemm_rounding_cpu.py), is NOT a bf16 number and sits at a chosen distance from a rounding boundary - exact ties with an even and
an odd neighbour, ties +- a sticky term, carries into the exponent, ties that only appear at the second rounding, fp32 subnormals reached by
cancellation, the tie below 2^128, signed zeros.  For the store, layer-scale, residual and patch epilogues the WHOLE fenced allocation
must equal the CPU image of IEEE round-to-nearest-even at each rounding point of csrc/epilogue.h, bit for bit; GELU and SwiGLU are judged
on the live elements by tests/test_gpu_gemm_layouts.py's rule AND bit for bit against the 128-tile route (their argument is rounded the
same way on every route or not at all).  The layouts (four different strides, NaN padding, fenced outputs) and the route forcing and
proving - the dispatcher's plan before the call, its launch record after it - are tests/test_gpu_gemm_layouts.py's, unchanged.

Out of scope: the decode-step kernels with a fused RMSNorm or RoPE (head8.hip) and the lm-head argmax, whose arithmetic before the epilogue
is not exact - of aigv_op_skinny_gemm_fp8 that leaves the norm-free form, which its launcher has for the residual epilogue only (SwiGLU and
rope exist with the fused RMSNorm alone); a GELU case of the fp8 form (|x| <= 4 leaves no room for a sticky term made of two normal e4m3
numbers under scales of 2); the SlowFast conv epilogue (tests/test_gpu_slowfast_ops.py)."""
import ctypes
import functools

import pytest
import torch

import gemm_rounding_reference as GR
from test_gpu_ops import BF, dev, lib, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import FENCE, SENTINEL, fenced, sentinel_like, same_bits
from test_gpu_gemm_layouts import (Layout, Fp8Layout, padded_rows, padded_vec, FENCE_ROWS, op_gemm, op_splitk, op_gemm_rows, proved, on_128, on_256, ran, restore, live_bits, VARIANT_WORDS,  # noqa: F401
                                   ROW_KNOBS, ROW_LISTS, DEFAULT_ROUTES, DEFAULT_WORD, R_128, R_256, R_CO, R_TAB_FUSED, R_TAB_LONE)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def checked_case(M, N, K, epi, fp8=False, pilot=False):
    case = GR.fp8_case(M, N, K, epi, pilot) if fp8 else GR.rounding_case(M, N, K, epi)
    bad = {k: v for k, v in GR.exactness(case).items() if v}
    assert not bad, f"the case is not exact ({bad}): the test itself is wrong"
    if fp8:                                                          # the e4m3 operands times their scales ARE the case's A and W
        assert not GR.fp8_holes(case), f"the fp8 form is not the case ({GR.fp8_holes(case)}): the test itself is wrong"
    return case


def layout(M, N, K, epi, inplace=False, ldo_pad=8):
    return Layout(checked_case(M, N, K, epi), inplace, ldo_pad)


def explain(L):
    """Which classes the differing live elements belong to (an element carries the class of its Linear rounding and, where a later rounding
    decides, ``second_point``)."""
    case = L.case
    diff = (live_bits(L) != case["want"].view(torch.int16)).numpy()
    if case["epi"] == 4:
        return f"{int(diff.sum())} of {diff.size} live elements differ from the CPU image"
    by_class = {name: f"{int((diff & t).sum())}/{int(t.sum())}" for name, t in GR.tags(case).items() if t.any()}
    return f"{int(diff.sum())} of {diff.size} live elements differ from the CPU image; differing/all by class: {by_class}"


def run(lib, L, op, what):
    """``op`` runs the route on layout L, proves it and compares the whole allocation (tests/test_gpu_gemm_layouts.py); a failure also says
    which classes it is made of."""
    try:
        op(lib, L)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}\n{explain(L)}") from e


# ---------------------------------------------------------------------------------------------------------
# one case per epilogue over every route
# ---------------------------------------------------------------------------------------------------------
M_ALL, N_ALL, K_ALL = GR.EVERY_ROUTE[0][:3]
LENS, TAIL_LENS = GR.CROSS_ROUTE_LENS, GR.CROSS_ROUTE_TAIL_LENS
assert sum(LENS) == M_ALL == sum(TAIL_LENS) and ROW_LISTS[ROW_KNOBS["tail_slices_1"][5]] == LENS == ROW_LISTS[ROW_KNOBS["co_resident"][5]]


def rows_knob(knob):
    *knobs, _, route = ROW_KNOBS[knob]
    return lambda lib, L: op_gemm_rows(lib, L, LENS, route, knobs)


TILE_ROUTES = {
    "128": lambda lib, L: op_gemm(lib, L, 1, proved(on_128(L.case["M"]), "mode 1 runs every row on the 128x128 kernel"), R_128),
    **{f"256-word{v}": (lambda v: lambda lib, L: op_gemm(lib, L, 2 + v, proved(on_256(L.case["M"]), "mode 2 runs every row on the 256x256 kernel"), R_256))(v)
       for v in VARIANT_WORDS},                                      # direct, LDS-staged with residual prefetch, balanced reads
    **{f"co-word{v}": (lambda v: lambda lib, L: op_gemm(lib, L, 4 + v, lambda p: None, R_CO))(v) for v in VARIANT_WORDS[:2]},   # no plan in mode 4: the record proves it
}
SPLITK_ROUTES = {f"splitk{'256' if t else '128'}-S{S}": (lambda t, S: lambda lib, L: op_splitk(lib, L, S, t))(t, S) for t in (False, True) for S in (2, 4)}
ROW_ROUTES = {
    "rows-default": lambda lib, L: op_gemm_rows(lib, L, LENS, DEFAULT_ROUTES["tiny_tails"]),
    "rows-tail_slices_1": rows_knob("tail_slices_1"),
    "rows-co_resident": rows_knob("co_resident"),
    # the fused body + tail-slice launch and the lone body need a tile tail: the same rows as another list of sequences
    "rows-fused-tails": lambda lib, L: op_gemm_rows(lib, L, TAIL_LENS, R_TAB_FUSED, (DEFAULT_WORD, 2, 2, 1, 0)),
    "rows-lone-body": lambda lib, L: op_gemm_rows(lib, L, TAIL_LENS, R_TAB_LONE, (DEFAULT_WORD, 0, 0, 2, 0)),
}
ROUTES = {**TILE_ROUTES, **SPLITK_ROUTES, **ROW_ROUTES}
# The patch epilogue runs where a launcher takes it: the tile kernels (with_epi<EPI_MASK_ALL> in gemm.hip, gemm256.hip, gemmco.hip).
# test_the_other_launchers_refuse_the_patch_epilogue asks the split-K and the row-plan launchers themselves.
ROUTES_OF = {epi: (TILE_ROUTES if epi == 5 else ROUTES) for epi in range(6)}

_reference_bits = {}


def reference_bits(lib, epi):
    """The live bits of the GELU / SwiGLU case on the plain 128-tile route (itself checked by the rule of Layout.check)."""
    if epi not in _reference_bits:
        L = layout(M_ALL, N_ALL, K_ALL, epi)
        run(lib, L, TILE_ROUTES["128"], "the 128-tile route")
        _reference_bits[epi] = live_bits(L)
    return _reference_bits[epi]


def agrees_with_128(lib, L, what):
    ref = reference_bits(lib, L.case["epi"])[:L.case["M"]]
    differ = int((live_bits(L) != ref).sum())
    assert differ == 0, f"{what}: {differ} of {ref.numel()} elements differ from the 128-tile route's bits"


@pytest.mark.parametrize("epi,route", [(epi, route) for epi in range(6) for route in sorted(ROUTES_OF[epi])])
def test_every_rounding_point_on_every_route(lib, epi, route):
    L = layout(M_ALL, N_ALL, K_ALL, epi)
    run(lib, L, ROUTES[route], route)
    if epi in (1, 4):
        agrees_with_128(lib, L, route)


@pytest.mark.parametrize("route", sorted(set(ROUTES) - set(ROUTES_OF[5])))
def test_the_other_launchers_refuse_the_patch_epilogue(lib, route):
    """ROUTES_OF[5] is not a guess: every route it leaves out is asked here, through the very call the other epilogues run on it, and refuses
    on the host - nothing is launched, the output keeps its sentinel."""
    from aigv_assessor_amd import native
    L = layout(M_ALL, N_ALL, K_ALL, 5)
    lib.aigv_gemm_route(1)
    with pytest.raises(native.NativeError):
        ROUTES[route](lib, L)
    torch.cuda.synchronize()
    ran(lib, 0, "a refused call")
    assert bool((L.whole.cpu().view(torch.int16) == SENTINEL[BF]).all())


@pytest.mark.parametrize("route", ["128", "256-word32", "co-word32", "splitk128-S2", "splitk256-S4", "rows-default", "rows-fused-tails"])
@pytest.mark.parametrize("epi", [2, 3])
def test_in_place_residual_on_every_kind_of_route(lib, epi, route):
    """resid == C with ldr == ldc, as the layers have it: the residual is read from the element the result overwrites."""
    run(lib, layout(M_ALL, N_ALL, K_ALL, epi, inplace=True), ROUTES[route], f"{route}, in place")


# ---------------------------------------------------------------------------------------------------------
# ragged small shapes: the scalar and tail paths (M = 1; a last row alone in its tile)
# ---------------------------------------------------------------------------------------------------------
def ragged_routes(M, N, K):
    out = ["128"] + ([f"256-word{v}" for v in VARIANT_WORDS] if N % 256 == 0 else [])
    for S in (2, 3):
        if K // 64 >= S and (K // 64) % S == 0:
            out += [f"splitk128-S{S}"] + ([f"splitk256-S{S}"] if N % 256 == 0 else [])
    return out


RAGGED_SPLITK = {f"splitk{'256' if t else '128'}-S3": (lambda t: lambda lib, L: op_splitk(lib, L, 3, t))(t) for t in (False, True)}


@pytest.mark.parametrize("epi", [0, 2, 3])
@pytest.mark.parametrize("M,N,K", sorted({c[:3] for c in GR.RAGGED}))
def test_ragged_shapes(lib, M, N, K, epi):
    assert (M, N, K, epi) in GR.RAGGED
    for route in ragged_routes(M, N, K):
        run(lib, layout(M, N, K, epi), {**ROUTES, **RAGGED_SPLITK}[route], route)
    if epi != 0:
        run(lib, layout(M, N, K, epi, inplace=True), ROUTES["128"], "128, in place")


# ---------------------------------------------------------------------------------------------------------
# the weight-streaming kernel: its own copy of the chain, a cross-lane reduction for p > 1
# ---------------------------------------------------------------------------------------------------------
def op_skinny(p, resid=True):
    def op(lib, L):
        from aigv_assessor_amd import native
        c = L.case
        epi = GR.SK_OF[c["epi"]]
        rc = lib.aigv_op_skinny_gemm_check(L.dA.data_ptr(), L.lda, c["M"], L.dW.data_ptr(), L.ldw, c["N"], c["K"], L.resid_ptr, L.ldr if L.resid_ptr else 0,
                                           L.C_ptr, L.ldc, epi)
        assert rc == 0, lib.aigv_last_error(None)
        try:
            native.check(lib.aigv_tune_skinny(p))
            sync(lib.aigv_op_skinny_gemm(L.dA.data_ptr(), L.lda, c["M"], L.dW.data_ptr(), L.ldw, c["N"], c["K"], L.bias_ptr, L.resid_ptr,
                                         L.ldr if L.resid_ptr else 0, L.C_ptr, L.ldc, epi, None), lib)
        finally:
            restore(lib)
        L.check()
    return op


@pytest.mark.parametrize("R,p,epi", GR.SKINNY)
def test_skinny_kernel(lib, R, p, epi):
    assert (GR.N_SKINNY, R, p, epi) in GR.SKINNY_CASES or (R, p) == (4, 4)          # (4 rows: the most the p = 4 form takes)
    run(lib, layout(R, GR.N_SKINNY, GR.K_SKINNY, epi, ldo_pad=12), op_skinny(p), f"skinny kernel, {R} rows, p = {p}")
    if epi == 3:
        run(lib, layout(R, GR.N_SKINNY, GR.K_SKINNY, epi, inplace=True, ldo_pad=12), op_skinny(p), f"skinny kernel in place, {R} rows, p = {p}")


@pytest.mark.parametrize("epi,R,p", [(1, 64, 1), (4, 64, 1), (4, 5, 2), (4, 4, 4)])       # (the sub-slab forms p > 1 have no GELU epilogue)
def test_skinny_kernel_agrees_with_the_tile_kernels(lib, epi, R, p):
    """GELU (p = 1) and SwiGLU on the first rows of the every-route case: the same bits as the 128-tile route."""
    whole = checked_case(M_ALL, N_ALL, K_ALL, epi)
    sub = GR.first_rows(whole, R)
    assert GR.is_exact(sub), "the case is not exact: the test itself is wrong"
    S = Layout(sub, False, 12)
    run(lib, S, op_skinny(p), f"skinny kernel, first {R} rows")
    agrees_with_128(lib, S, f"skinny kernel, p = {p}")


# ---------------------------------------------------------------------------------------------------------
# the fp8 form: the e4m3 tile kernel and its split-K form
# ---------------------------------------------------------------------------------------------------------
def fp8_reference_bits(lib, case):
    """The case's A and W are bf16 numbers too: the bf16 128-tile kernel on them gives the bits the e4m3 kernel must give for SwiGLU."""
    L = Layout(case)
    run(lib, L, TILE_ROUTES["128"], "the bf16 128-tile route on the fp8 case's operands")
    return live_bits(L)


@pytest.mark.parametrize("k_slices", [0, 2])
@pytest.mark.parametrize("M,N,K,epi,inplace", [c + (i,) for c in GR.FP8 for i in (False, True) if not i or c[3] in (2, 3)])
def test_fp8_gemm(lib, M, N, K, epi, inplace, k_slices):
    case = checked_case(M, N, K, epi, True)
    L = Fp8Layout(case, inplace)
    ws_ptr = None
    if k_slices:
        n_ws = k_slices * M * N
        ws_whole, ws = fenced(sentinel_like((n_ws,), torch.float32))
        ws_ptr = ws.data_ptr()
    run(lib, L, lambda lib, L: L.run(lib, k_slices, ws_ptr), f"fp8, {k_slices} K slices")
    if k_slices:
        got = ws_whole.cpu().view(torch.int32)
        fence = torch.full((FENCE,), SENTINEL[torch.float32], dtype=torch.int32)
        assert torch.equal(got[:FENCE], fence), "written in front of the split-K workspace"
        assert torch.equal(got[FENCE + n_ws:], fence), "written past the split-K workspace"
    if epi == 4:
        differ = int((live_bits(L) != fp8_reference_bits(lib, case)).sum())
        assert differ == 0, f"{differ} elements differ from the bf16 128-tile route's bits"


# ---------------------------------------------------------------------------------------------------------
# the e4m3 weight-streaming kernel without a norm: its own row quantisation, (acc * row scale) * channel scale, K quarters per wave and a
# cross-lane reduction for p > 1, its own call of the residual epilogue
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,K,p", GR.SKINNY_FP8)
def test_fp8_skinny_kernel(lib, R, N, K, p):
    """aigv_op_skinny_gemm_fp8 quantises its bf16 rows by 448 / amax.  Every row carries a pilot element of 448 x its row scale where all of W
    is zero, so the kernel's own bytes and scale are the case's A8 and row scale, exactly (tests/gemm_rounding_reference.py), and the whole
    fenced allocation must equal the CPU image.  Layout as tests/test_gpu_gemm_layouts.py's test_fp8_decode_gemv_layout: ldx = K + 8,
    ldw = K + 16 bytes, ldo = N + 12, ldr = N + 24, NaN padding in x and the residual, NaN bytes behind W's rows, the scales inside a
    NaN-filled vector."""
    case = checked_case(R, N, K, 3, True, True)
    ops = case["fp8"]
    ldx, ldw, ldo, ldr = K + 8, K + 16, N + 12, N + 24
    dx = dev(padded_rows(case["A"], ldx, 2))
    w8 = torch.full((N, ldw), 0x7f, dtype=torch.uint8)
    w8[:, :K] = ops["W8"].view(torch.uint8)
    dw8 = dev(w8)
    dsw, sw_ptr = padded_vec(ops["col_scale"])
    dr = dev(padded_rows(case["resid"], ldr, 2))
    before = sentinel_like((FENCE_ROWS + R + FENCE_ROWS, ldo), BF)
    whole, view = fenced(before)
    sync(lib.aigv_op_skinny_gemm_fp8(dx.data_ptr(), ldx, R, dw8.data_ptr(), ldw, ctypes.cast(sw_ptr, ctypes.POINTER(ctypes.c_float)), N, K, dr.data_ptr(), ldr,
                                     view.data_ptr() + FENCE_ROWS * ldo * 2, ldo, 1, None, 0.0, p, None), lib)
    image = before.clone()
    image[FENCE_ROWS:FENCE_ROWS + R, :N] = case["want"]
    try:
        same_bits(whole, image)
    except AssertionError as e:
        got = whole.cpu()[FENCE:FENCE + before.numel()].view(before.shape)[FENCE_ROWS:FENCE_ROWS + R, :N]
        diff = (got.contiguous().view(torch.int16) != case["want"].view(torch.int16)).numpy()
        by_class = {name: f"{int((diff & t).sum())}/{int(t.sum())}" for name, t in GR.tags(case).items() if t.any()}
        raise AssertionError(f"{e}\ndiffering/all live elements by class: {by_class}") from e
