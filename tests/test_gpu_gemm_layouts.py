"""The GEMM family on strided, fenced layouts with exact sums (MI355X only): every dispatch route of the C ABI - the 128x128, the 256x256
and the co-resident tile kernels, the cost-model row and column bands, split-K with its finalize pass, the per-sequence row plans with
their tiny tails, the weight-streaming skinny kernel - does its own pointer arithmetic on four independent strides, and none of the
random-data tests of tests/test_gpu_ops.py could see an error in it (there lda = ldw = K, ldc = ldr = n_out, and a stray store lands in
allocator slack).

Here the four strides of a case differ from each other and from N and K; A and W carry NaN padding columns (A two NaN rows behind its
last one); bias, layer scale and position rows are pointers into the middle of NaN-filled vectors; the output sits between fences of two
whole rows plus the fixed fence of tests/test_gpu_row_ops.py, all holding a sentinel, like its padding columns.  The inputs are those of
tests/gemm_exact_reference.py: every partial sum in any order is a bf16 number, so for the store, residual, layer-scale and patch
epilogues the WHOLE allocation must equal one CPU image bit for bit, whichever kernel, slice or row plan ran.  GELU keeps an exact
argument and must be within one bf16 ulp of torch's GELU of it; SwiGLU is judged by test_gemm_epilogues' rule; for both, padding and
fences are still compared bit for bit.

Every route is forced and then PROVED: before the call on the dispatcher's own plan (aigv_plan_gemm), after it on the dispatcher's record of the
launches it made (aigv_gemm_route) - a change that sends a case to another kernel fails here instead of passing on that kernel.  The fp8 form
(row quantisation, the e4m3 tile kernel with its split-K form, the e4m3 decode GEMV) gets the same layouts at the end of the file."""
import ctypes

import pytest
import torch

import gemm_exact_reference as GX
from test_gpu_ops import BF, dev, lib, sync, ulp_check, gemm_ref, _quant_ref, _epilogue_ref, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import FENCE, SENTINEL, INT_OF, fenced, sentinel_like, same_bits
from gemm_exact_reference import strides, SHAPES_128, SHAPES_256, COST_MODEL, ROW_LISTS, K_ROWS, SK_OF, K_SKINNY, SKINNY_CASES

pytestmark = pytest.mark.gpu

NAN = float("nan")
VEC_PAD = 16                     # elements of NaN in front of and behind bias / ls / pos (keeps their 16-byte alignment)
FENCE_ROWS = 2                   # whole sentinel rows in front of and behind every output: a one-row overrun lands inside the allocation
TUNE_TAIL_SLICES, TUNE_FUSE_TAILS, TUNE_LONE_BODY = 7, 12, 13          # AIGV_TUNE_* (include/aigv_amd.h)
DEFAULT_WORD = 0 + 32            # aigv_tune_gemm: cost-model dispatch, the shipped schedule of the 256 kernel
# aigv_gemm_route: one bit per kind of launch the dispatcher made (AIGV_ROUTE_* of include/aigv_amd.h)
R_128, R_256, R_CO, R_SPLITK_128, R_SPLITK_256, R_SKINNY, R_COLUMN_BAND = 1, 2, 4, 8, 16, 32, 64
R_TAB_256, R_TAB_SPLITK, R_TAB_FUSED, R_TAB_LONE, R_TAB_128, R_TAB_CO, R_TINY, R_TINY_STRIDED = 128, 256, 512, 1024, 2048, 4096, 8192, 16384


def padded_rows(t, ld, extra_rows=0):
    out = torch.full((t.shape[0] + extra_rows, ld), NAN, dtype=t.dtype)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def padded_vec(t):
    if t is None:
        return None, None
    flat = t.reshape(-1)
    out = torch.full((flat.numel() + 2 * VEC_PAD,), NAN, dtype=t.dtype)
    out[VEC_PAD:VEC_PAD + flat.numel()] = flat
    d = dev(out)
    return d, d.data_ptr() + VEC_PAD * out.element_size()


class Layout:
    """The device buffers of one case and the CPU image its output allocation must equal."""

    def __init__(self, case, inplace=False, ldo_pad=8):
        self.case, M, N, K, epi = case, case["M"], case["N"], case["K"], case["epi"]
        self.no = no = GX.n_out(N, epi)
        _, _, self.ldc, self.ldr = strides(no, K, ldo_pad)
        self.put_operands(ldo_pad)
        self.rows = GX.patch_rows(M, case["np"]) if epi == 5 else torch.arange(M)
        self.rows_out = M + M // case["np"] if epi == 5 else M
        before = sentinel_like((FENCE_ROWS + self.rows_out + FENCE_ROWS, self.ldc), BF)
        self.resid_ptr = None
        if inplace:                                                # resid == C, ldr == ldc, as the layers have it
            assert case["resid"] is not None
            before[FENCE_ROWS:FENCE_ROWS + M, :no] = case["resid"]
            self.ldr = self.ldc
        elif case["resid"] is not None:
            self.dR = dev(padded_rows(case["resid"], self.ldr, 2))
            self.resid_ptr = self.dR.data_ptr()
        self.whole, view = fenced(before)
        self.C_ptr = view.data_ptr() + FENCE_ROWS * self.ldc * 2
        if inplace:
            self.resid_ptr = self.C_ptr
        self.image = before.clone()
        self.image[FENCE_ROWS + self.rows, :no] = case["want"]
        self.live = torch.zeros_like(self.image, dtype=torch.bool)
        self.live[FENCE_ROWS + self.rows, :no] = True
        (self.dbias, self.bias_ptr), (self.dls, self.ls_ptr), (self.dpos, self.pos_ptr) = (padded_vec(case[k]) for k in ("bias", "ls", "pos"))

    def put_operands(self, ldo_pad):
        """A and W on the device with NaN padding columns, A with two NaN rows behind its last one; lda / ldw in bf16 elements."""
        c = self.case
        self.lda, self.ldw, _, _ = strides(self.no, c["K"], ldo_pad)
        self.dA, self.dW = dev(padded_rows(c["A"], self.lda, 2)), dev(padded_rows(c["W"], self.ldw))

    def operands(self):
        """(A, lda, W, ldw, C, ldc, bias, ls, resid, ldr): the leading arguments of aigv_op_gemm and its siblings."""
        return (self.dA.data_ptr(), self.lda, self.dW.data_ptr(), self.ldw, self.C_ptr, self.ldc, self.bias_ptr, self.ls_ptr, self.resid_ptr,
                self.ldr if self.resid_ptr else 0)

    def accepted(self, lib):
        c = self.case
        rc = lib.aigv_op_gemm_check(*self.operands(), self.pos_ptr, c["np"], c["M"], c["N"], c["K"], c["epi"])
        assert rc == 0, lib.aigv_last_error(None)

    def check(self):
        """Exact epilogues: the whole allocation against the image.  GELU / SwiGLU: everything but the live elements bit for bit, the live
        elements by their rule."""
        epi = self.case["epi"]
        if epi in GX.EXACT_EPILOGUES:
            same_bits(self.whole, self.image)
            return
        n = self.image.numel()
        got = self.whole.cpu()[FENCE:FENCE + n].view(self.image.shape)
        image = torch.where(self.live, got, self.image)
        same_bits(self.whole, image)
        got, want = got[FENCE_ROWS + self.rows, :self.no].float(), self.case["want"].float()
        if epi == 1:
            assert torch.isfinite(got).all()
            ulp = want.abs().clamp_min(1e-38).log2().floor().exp2() * 2.0 ** -7
            worst = ((got - want).abs() / ulp).max().item()
            print(f"gelu: worst error {worst:.3f} ulp, {int((got != want).sum())} of {got.numel()} elements differ")
            assert bool(((got - want).abs() <= ulp).all()), f"worst error {worst:.2f} ulp"
        else:
            c = self.case
            ulp_check(got, gemm_ref(c["A"], c["W"], 4), frac=0.03, max_ulps=4, atol_rel=2e-5)


def exact_layout(M, N, K, epi, inplace=False, seed=0, ldo_pad=8):
    case = GX.exact_case(M, N, K, epi, seed)
    assert GX.is_exact(case), "the case is not exact: the test itself is wrong"
    return Layout(case, inplace, ldo_pad)


def plan_of(lib, M, N, K, epi):
    """aigv_plan_gemm under the CURRENT process mode: (top_tiles, mid_tiles, mid_slices, last_rows, last_kind, last_slices, right band)."""
    from aigv_assessor_amd import native
    plan = (ctypes.c_int * 7)()
    native.check(lib.aigv_plan_gemm(M, N, K, epi, plan, None))
    return list(plan)


def restore(lib):
    from aigv_assessor_amd import native
    native.check(lib.aigv_tune_gemm(DEFAULT_WORD, 0.0))            # also the body tile and the tile order
    native.check(lib.aigv_tune_co_gemm(0))
    native.check(lib.aigv_tune_default(TUNE_TAIL_SLICES, 0))
    native.check(lib.aigv_tune_default(TUNE_FUSE_TAILS, 0))
    native.check(lib.aigv_tune_default(TUNE_LONE_BODY, 1))
    native.check(lib.aigv_tune_skinny(0))


def ran(lib, route, what=""):
    """The launches the dispatcher made since the record was cleared are exactly ``route``."""
    got = lib.aigv_gemm_route(1)
    assert got == route, f"{what}: the dispatcher launched route bits {got:#x}, the case is meant to run {route:#x}"


def op_gemm(lib, L, word, prove, route):
    """aigv_op_gemm on layout ``L`` under aigv_tune_gemm(word).  ``prove(plan)`` asserts on the dispatcher's own plan that the route is the
    one meant; ``route`` (AIGV_ROUTE_* bits, or a function of the plan) is what the dispatcher must then report to have LAUNCHED.  Every
    tune call is undone."""
    from aigv_assessor_amd import native
    c = L.case
    L.accepted(lib)
    try:
        native.check(lib.aigv_tune_gemm(word, 0.0))
        plan = plan_of(lib, c["M"], c["N"], c["K"], c["epi"])
        prove(plan)
        lib.aigv_gemm_route(1)
        sync(lib.aigv_op_gemm(*L.operands(), L.pos_ptr, c["np"], c["M"], c["N"], c["K"], c["epi"], None), lib)
        ran(lib, route(plan) if callable(route) else route, f"word {word}, plan {plan}")
    finally:
        restore(lib)
    L.check()


# ---------------------------------------------------------------------------------------------------------
# one tile kernel for every row
# ---------------------------------------------------------------------------------------------------------
def on_128(M):
    return lambda p: p[0] == 0 and p[1] == 0 and p[3:6] == [M, 2, 1] and p[6] == 0


def on_256(M):
    return lambda p: p[0] == -1 and p[6] == 0


def proved(f, what):
    def prove(p):
        assert f(p), f"{what}: the dispatcher plans {p}"
    return prove


VARIANT_WORDS = (16, 32, 64)     # aigv_tune_gemm bits 4..6: the first schedule (direct 8-byte epilogue), the shipped one (LDS-staged 16-byte row
                                 # segments, residual prefetch), balanced reads with the direct epilogue - three epilogue code paths


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("M,N,K", SHAPES_128)
def test_128_kernel(lib, M, N, K, epi):
    op_gemm(lib, exact_layout(M, N, K, epi), 1, proved(on_128(M), "mode 1 runs every row on the 128x128 kernel"), R_128)


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("i", range(len(SHAPES_256)), ids=lambda i: "-".join(map(str, SHAPES_256[i])))
def test_256_kernel(lib, i, epi):
    """The three schedule variants take turns over shapes x epilogues: every epilogue and every shape meets each of them."""
    M, N, K = SHAPES_256[i]
    op_gemm(lib, exact_layout(M, N, K, epi), 2 + VARIANT_WORDS[(i + epi) % 3], proved(on_256(M), "mode 2 runs every row on the 256x256 kernel"), R_256)


@pytest.mark.parametrize("variant", VARIANT_WORDS)
def test_256_kernel_variants_on_one_ragged_shape(lib, variant):
    for epi in range(6):
        op_gemm(lib, exact_layout(514, 512, 128, epi), 2 + variant, proved(on_256(514), "mode 2"), R_256)


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("M,N,K", SHAPES_256)
def test_co_resident_kernel(lib, M, N, K, epi):
    """Mode 4: use_co() sends the call to gemmco.hip before any plan is made (dispatch.hip), so there is no plan to assert on; the
    dispatcher's record must show the co-resident launch and nothing else."""
    op_gemm(lib, exact_layout(M, N, K, epi), 4 + 32, lambda p: None, R_CO)


@pytest.mark.parametrize("word,M,N,K,epi", [(1, 300, 384, 192, 3), (1, 129, 128, 64, 2), (2 + 16, 514, 512, 128, 3), (2 + 32, 257, 256, 64, 2),
                                            (2 + 64, 514, 256, 128, 2), (4 + 32, 514, 512, 128, 3), (4 + 32, 255, 256, 64, 2)])
def test_tile_kernels_in_place_residual(lib, word, M, N, K, epi):
    """resid == C with ldr == ldc: the image holds the residual in the live columns and the sentinel in the padding."""
    mode = word & 7
    prove = {1: proved(on_128(M), "mode 1"), 2: proved(on_256(M), "mode 2"), 4: lambda p: None}[mode]
    op_gemm(lib, exact_layout(M, N, K, epi, inplace=True), word, prove, {1: R_128, 2: R_256, 4: R_CO}[mode])


# ---------------------------------------------------------------------------------------------------------
# cost-model dispatch (mode 0): one shape per feature of run_gemm, the smallest a search over aigv_plan_gemm found
# ---------------------------------------------------------------------------------------------------------
def planned_route(p):
    """The launches run_gemm makes for plan ``p`` (aigv_plan_gemm), as AIGV_ROUTE_* bits."""
    r = (R_COLUMN_BAND | R_128) if p[6] else 0
    if p[0] != 0:
        r |= R_256
    if p[1] > 0:
        r |= R_SPLITK_256
    if p[4] == 1:
        r |= R_SKINNY
    if p[4] == 2:
        r |= R_SPLITK_128 if p[5] > 1 else R_128
    return r


@pytest.mark.parametrize("feature", sorted(COST_MODEL))
@pytest.mark.parametrize("inplace", [False, True])
def test_cost_model_dispatch(lib, feature, inplace):
    """Each feature is ASSERTED on the plan first: a change of the cost model that loses a route must fail here, not pass silently."""
    M, N, K, epi, shows = COST_MODEL[feature]
    if inplace and epi not in (2, 3):
        epi = 3
    op_gemm(lib, exact_layout(M, N, K, epi, inplace), DEFAULT_WORD, proved(shows, f"{feature} at M={M} N={N} K={K}"), planned_route)


# ---------------------------------------------------------------------------------------------------------
# split-K called directly
# ---------------------------------------------------------------------------------------------------------
def op_splitk(lib, L, S, tile256):
    c = L.case
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    L.accepted(lib)
    n_ws = S * M * N
    ws_whole, ws = fenced(sentinel_like((n_ws,), torch.float32))
    op = lib.aigv_op_gemm_splitk256 if tile256 else lib.aigv_op_gemm_splitk
    sync(op(*L.operands(), M, N, K, epi, S, ws.data_ptr(), None), lib)
    got = ws_whole.cpu().view(torch.int32)
    fence = torch.full((FENCE,), SENTINEL[torch.float32], dtype=torch.int32)
    assert torch.equal(got[:FENCE], fence), "written in front of the split-K workspace"
    assert torch.equal(got[FENCE + n_ws:], fence), "written past the split-K workspace"
    L.check()


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("M", [4, 130, 300])
def test_splitk_128(lib, M, S, epi):
    op_splitk(lib, exact_layout(M, 384, 384, epi), S, False)


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("M", [256, 513])
def test_splitk_256(lib, M, S, epi):
    op_splitk(lib, exact_layout(M, 256, 384, epi), S, True)


@pytest.mark.parametrize("tile256,M,N,epi", [(False, 300, 384, 3), (False, 130, 384, 2), (True, 513, 256, 3), (True, 256, 256, 2)])
def test_splitk_in_place_residual(lib, tile256, M, N, epi):
    op_splitk(lib, exact_layout(M, N, 384, epi, inplace=True), 2, tile256)


# ---------------------------------------------------------------------------------------------------------
# per-sequence row plans
# ---------------------------------------------------------------------------------------------------------
# knob settings beyond the defaults (aigv_tune_gemm word for the body tile, AIGV_TUNE_TAIL_SLICES, _FUSE_TAILS, _LONE_BODY, co-resident K
# threshold) with the list each runs on
ROW_KNOBS = {
    # name: (word, tail slices, fuse tails, lone body, co-resident K threshold, list, the launches run_gemm_rows must report)
    "body_tile_128": (DEFAULT_WORD + (2 << 14), 0, 0, 1, 0, "tails_up_to_and_above_128", R_TAB_128 | R_TAB_256),
    "body_tile_128_tails_apart": (DEFAULT_WORD + (2 << 14), 2, 0, 1, 0, "short_next_to_long", R_TAB_128 | R_TAB_SPLITK),
    "tail_slices_1": (DEFAULT_WORD, 1, 0, 1, 0, "tiny_tails", R_TAB_256 | R_TINY),
    "tail_slices_2": (DEFAULT_WORD, 2, 0, 1, 0, "tails_up_to_and_above_128", R_TAB_FUSED),        # two body tiles leave the round open: fused by fill
    "tail_slices_2_never_fused": (DEFAULT_WORD, 2, 1, 1, 0, "tails_up_to_and_above_128", R_TAB_256 | R_TAB_SPLITK),
    "tail_slices_2_always_fused": (DEFAULT_WORD, 2, 2, 1, 0, "short_next_to_long", R_TAB_FUSED),
    "lone_body": (DEFAULT_WORD, 0, 0, 2, 0, "short_next_to_long", R_TAB_LONE),
    "lone_body_tails_apart": (DEFAULT_WORD, 2, 0, 2, 0, "tails_up_to_and_above_128", R_TAB_LONE | R_TAB_SPLITK),
    "co_resident_uniform": (DEFAULT_WORD, 0, 0, 1, K_ROWS, "uniform_tiny_tails_1", R_TAB_CO | R_TINY_STRIDED),
    "co_resident": (DEFAULT_WORD, 0, 0, 1, K_ROWS, "tiny_tails", R_TAB_CO | R_TINY),
}
# at the defaults (K = 512 is too short for tail slices of their own, the co-resident kernel is off): every half tile in one launch of the 256
# kernel, the tiny tails on the skinny kernel
DEFAULT_ROUTES = {
    "whole_tiles": R_TAB_256, "tails_up_to_and_above_128": R_TAB_256, "tiny_tails": R_TAB_256 | R_TINY,
    "uniform_tiny_tails_1": R_TAB_256 | R_TINY_STRIDED, "uniform_tiny_tails_4": R_TAB_256 | R_TINY_STRIDED, "short_next_to_long": R_TAB_256,
}


def op_gemm_rows(lib, L, lens, route, knobs=None):
    from aigv_assessor_amd import native
    c = L.case
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    assert cu[-1] == c["M"]
    L.accepted(lib)
    try:
        if knobs is not None:
            word, tail_slices, fuse, lone, co_kmax = knobs
            native.check(lib.aigv_tune_gemm(word, 0.0))
            native.check(lib.aigv_tune_default(TUNE_TAIL_SLICES, tail_slices))
            native.check(lib.aigv_tune_default(TUNE_FUSE_TAILS, fuse))
            native.check(lib.aigv_tune_default(TUNE_LONE_BODY, lone))
            native.check(lib.aigv_tune_co_gemm(co_kmax))
            if tail_slices > 1:                                    # a forced factor that does not divide is silently ignored (tail_slices())
                assert (c["K"] // 64) % tail_slices == 0 and c["K"] // 64 // tail_slices >= 4
            assert co_kmax == 0 or c["K"] <= co_kmax
        lib.aigv_gemm_route(1)
        sync(lib.aigv_op_gemm_rows(*L.operands(), (ctypes.c_int32 * len(cu))(*cu), len(lens), c["N"], c["K"], c["epi"], None), lib)
        ran(lib, route, f"lengths {lens}, knobs {knobs}")
    finally:
        restore(lib)
    L.check()


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("name", sorted(ROW_LISTS))
def test_row_plans_at_the_defaults(lib, name, N, epi):
    lens = ROW_LISTS[name]
    op_gemm_rows(lib, exact_layout(sum(lens), N, K_ROWS, epi), lens, DEFAULT_ROUTES[name])


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("knob", sorted(ROW_KNOBS))
def test_row_plans_under_every_knob(lib, knob, N, epi):
    """With exact data every knob must give the SAME image - asserted against the CPU image, not against another kernel run."""
    *knobs, name, route = ROW_KNOBS[knob]
    lens = ROW_LISTS[name]
    op_gemm_rows(lib, exact_layout(sum(lens), N, K_ROWS, epi), lens, route, knobs)


@pytest.mark.parametrize("epi", [2, 3])
@pytest.mark.parametrize("knob", [None, "tail_slices_2_always_fused", "co_resident_uniform", "lone_body"])
def test_row_plans_in_place_residual(lib, knob, epi):
    knobs, name, route = (None, "tiny_tails", DEFAULT_ROUTES["tiny_tails"]) if knob is None else (ROW_KNOBS[knob][:5], *ROW_KNOBS[knob][5:])
    lens = ROW_LISTS[name]
    op_gemm_rows(lib, exact_layout(sum(lens), 256, K_ROWS, epi, inplace=True), lens, route, knobs)


# ---------------------------------------------------------------------------------------------------------
# the weight-streaming skinny kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,R,p,epi", SKINNY_CASES)
def test_skinny_kernel(lib, N, R, p, epi):
    """ldx = K + 8, ldw = K + 16, ldo = n_out + 12 (a multiple of 4 that is none of 8: the kernel moves 8 bytes), ldr = n_out + 24."""
    from aigv_assessor_amd import native
    K = K_SKINNY
    L = exact_layout(R, N, K, epi, ldo_pad=12)
    rc = lib.aigv_op_skinny_gemm_check(L.dA.data_ptr(), L.lda, R, L.dW.data_ptr(), L.ldw, N, K, L.resid_ptr, L.ldr if L.resid_ptr else 0, L.C_ptr, L.ldc, SK_OF[epi])
    assert rc == 0, lib.aigv_last_error(None)
    try:
        native.check(lib.aigv_tune_skinny(p))
        sync(lib.aigv_op_skinny_gemm(L.dA.data_ptr(), L.lda, R, L.dW.data_ptr(), L.ldw, N, K, L.bias_ptr, L.resid_ptr, L.ldr if L.resid_ptr else 0,
                                     L.C_ptr, L.ldc, SK_OF[epi], None), lib)
    finally:
        restore(lib)
    L.check()


@pytest.mark.parametrize("R,p", [(64, 1), (5, 2), (1, 4)])
def test_skinny_kernel_in_place_residual(lib, R, p):
    from aigv_assessor_amd import native
    N, K = 288, K_SKINNY
    L = exact_layout(R, N, K, 3, inplace=True, ldo_pad=12)
    try:
        native.check(lib.aigv_tune_skinny(p))
        sync(lib.aigv_op_skinny_gemm(L.dA.data_ptr(), L.lda, R, L.dW.data_ptr(), L.ldw, N, K, None, L.resid_ptr, L.ldr, L.C_ptr, L.ldc, 1, None), lib)
    finally:
        restore(lib)
    L.check()


# ---------------------------------------------------------------------------------------------------------
# GELU and SwiGLU: one case each over every route, bit for bit
# ---------------------------------------------------------------------------------------------------------
def live_bits(L):
    """The live elements of layout ``L``'s output, as int16 bit patterns."""
    n = L.image.numel()
    got = L.whole.cpu()[FENCE:FENCE + n].view(L.image.shape)
    return got[FENCE_ROWS + L.rows, :L.no].contiguous().view(torch.int16)


@pytest.mark.parametrize("M,N,K,epi", GX.CROSS_ROUTE)
def test_gelu_and_swiglu_bits_agree_on_every_route(lib, M, N, K, epi):
    """The accumulator of every element of an exact case is the same number in any summation order, so the GELU / SwiGLU output of one case is
    ONE bit pattern whichever kernel ran - the same epilogue arithmetic (csrc/epilogue.h) on the same argument - not merely within an ulp
    of torch, which is all Layout.check asks of these two epilogues.  The plain 128-tile route is the reference; every op below also checks
    fences, padding and the tolerance as the tests above do."""
    from aigv_assessor_amd import native
    lens = GX.CROSS_ROUTE_LENS
    assert sum(lens) == M

    def fresh():
        return exact_layout(M, N, K, epi)

    L = fresh()
    op_gemm(lib, L, 1, proved(on_128(M), "mode 1"), R_128)
    ref = live_bits(L)
    routes = {}
    for variant in VARIANT_WORDS:
        L = fresh()
        op_gemm(lib, L, 2 + variant, proved(on_256(M), "mode 2"), R_256)
        routes[f"256 kernel, schedule word {variant}"] = live_bits(L)
    for variant in VARIANT_WORDS[:2]:                                  # both shipped schedules (mode 4 makes no plan: the record proves the launch)
        L = fresh()
        op_gemm(lib, L, 4 + variant, lambda p: None, R_CO)
        routes[f"co-resident kernel, schedule word {variant}"] = live_bits(L)
    for tile256 in (False, True):
        for S in (2, 4):
            L = fresh()
            op_splitk(lib, L, S, tile256)
            routes[f"split-K, {'256' if tile256 else '128'} tile, {S} slices"] = live_bits(L)
    L = fresh()
    op_gemm_rows(lib, L, lens, DEFAULT_ROUTES["tiny_tails"])
    routes["row plan at the defaults"] = live_bits(L)
    for knob in ("tail_slices_1", "co_resident"):
        *knobs, name, route = ROW_KNOBS[knob]
        assert ROW_LISTS[name] == lens
        L = fresh()
        op_gemm_rows(lib, L, lens, route, knobs)
        routes[f"row plan, {knob}"] = live_bits(L)
    # the fused body + tail-slice launch and the lone body need a tile tail: the same rows as another list of sequences (a row's bits do not
    # depend on the sequence it sits in)
    for what, knobs, route in (("fused tails", (DEFAULT_WORD, 2, 2, 1, 0), R_TAB_FUSED), ("lone body", (DEFAULT_WORD, 0, 0, 2, 0), R_TAB_LONE)):
        L = fresh()
        op_gemm_rows(lib, L, GX.CROSS_ROUTE_TAIL_LENS, route, knobs)
        routes[f"row plan, {what}"] = live_bits(L)
    for what, got in routes.items():
        differ = int((got != ref).sum())
        assert differ == 0, f"{what}: {differ} of {ref.numel()} elements differ from the 128-tile route's bits"
    # the weight-streaming kernel on the first rows of the same A
    R = GX.CROSS_ROUTE_SKINNY_ROWS
    sub = GX.first_rows(L.case, R)
    assert GX.is_exact(sub), "the case is not exact: the test itself is wrong"
    S = Layout(sub, False, 12)
    rc = lib.aigv_op_skinny_gemm_check(S.dA.data_ptr(), S.lda, R, S.dW.data_ptr(), S.ldw, N, K, None, 0, S.C_ptr, S.ldc, SK_OF[epi])
    assert rc == 0, lib.aigv_last_error(None)
    try:
        native.check(lib.aigv_tune_skinny(1))
        sync(lib.aigv_op_skinny_gemm(S.dA.data_ptr(), S.lda, R, S.dW.data_ptr(), S.ldw, N, K, S.bias_ptr, None, 0, S.C_ptr, S.ldc, SK_OF[epi], None), lib)
    finally:
        restore(lib)
    S.check()
    differ = int((live_bits(S) != ref[:R]).sum())
    assert differ == 0, f"skinny kernel: {differ} of {ref[:R].numel()} elements differ from the 128-tile route's bits"


# ---------------------------------------------------------------------------------------------------------
# the fp8 form: row quantisation, the e4m3 tile kernel and its split-K form, the e4m3 decode GEMV
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(M, K) for M in (1, 257) for K in (128, 256)])
def test_fp8_row_quantisation_layout(lib, M, K):
    """ldx = K + 8 elements with NaN padding, ldq = K + 16 bytes with sentinel padding, two sentinel rows around the bytes, fences around
    the scales.  A dyadic row with a power-of-two amax quantises exactly (x * 448 / amax is 112, 224 or 448 times a power of two: e4m3
    numbers), so the bytes and scales are those of test_fp8_row_quantisation_is_bit_exact's restatement, bit for bit."""
    case = GX.exact_case(M, 256, K, 0)
    x = case["A"].clone() + 0.0                                    # -0 -> +0: one byte pattern for zero
    if M > 3:
        x[3] = 0                                                   # an all-zero row: scale 1, bytes 0
    q_ref, s_ref = _quant_ref(x)
    amax = x.float().abs().amax(1, keepdim=True)
    assert torch.equal(q_ref.float() * amax, x.float() * 448.0) and bool((amax.log2() % 1 == 0)[amax > 0].all()), \
        "the case is not exact: the test itself is wrong"               # x * 448 / amax is an e4m3 number: the quantisation rounds nothing
    ldx, ldq = K + 8, K + 16
    before = sentinel_like((FENCE_ROWS + M + FENCE_ROWS, ldq), torch.uint8)
    q_whole, q_view = fenced(before)
    s_whole, s_view = fenced(sentinel_like((M,), torch.float32))
    dx = dev(padded_rows(x, ldx, 2))
    sync(lib.aigv_op_quant_fp8_rows(dx.data_ptr(), ldx, M, K, q_view.data_ptr() + FENCE_ROWS * ldq, ldq, s_view.data_ptr(), None), lib)
    image = before.clone()
    image[FENCE_ROWS:FENCE_ROWS + M, :K] = q_ref.view(torch.uint8)
    same_bits(q_whole, image)
    same_bits(s_whole, s_ref)


class Fp8Layout(Layout):
    """The same case behind power-of-two scales (GX.fp8_operands): e4m3 A with lda = K + 16 BYTES, W with ldw = K + 32, NaN bytes (0x7f) in
    the padding and in two rows behind A's last one; the scale vectors inside NaN-filled vectors."""

    def put_operands(self, ldo_pad):
        """The e4m3 operands take the place of the bf16 ones: lda8 / ldw8 are in BYTES."""
        case = self.case
        if "fp8" in case:                                          # a case that brings its own e4m3 operands (tests/gemm_rounding_reference.py,
            ops = case["fp8"]                                      # whose tests assert its bound themselves)
        else:
            ops = GX.fp8_operands(case)
            assert GX.fp8_is_exact(case, ops), "the case is not exact: the test itself is wrong"
        K = case["K"]
        self.lda8, self.ldw8 = K + 16, K + 32
        assert len({self.lda8, self.ldw8, self.ldc}) == 3 and self.ldr not in (self.lda8, self.ldw8)

        def rows8(t, ld, extra):
            out = torch.full((t.shape[0] + extra, ld), 0x7f, dtype=torch.uint8)
            out[:t.shape[0], :K] = t.view(torch.uint8)
            return dev(out)
        self.dA8, self.dW8 = rows8(ops["A8"], self.lda8, 2), rows8(ops["W8"], self.ldw8, 0)
        (self.drs, self.rs_ptr), (self.dcs, self.cs_ptr) = padded_vec(ops["row_scale"]), padded_vec(ops["col_scale"])

    def operands(self):
        raise NotImplementedError("aigv_op_gemm_fp8 takes other arguments: see run()")

    def run(self, lib, k_slices=0, ws_ptr=None):
        c = self.case
        sync(lib.aigv_op_gemm_fp8(self.dA8.data_ptr(), self.lda8, self.dW8.data_ptr(), self.ldw8, self.C_ptr, self.ldc, self.rs_ptr, self.cs_ptr,
                                  self.bias_ptr, self.ls_ptr, self.resid_ptr, self.ldr if self.resid_ptr else 0, c["M"], c["N"], c["K"], c["epi"],
                                  k_slices, ws_ptr, None), lib)
        self.check()


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K", GX.SHAPES_FP8)
def test_fp8_gemm(lib, M, N, K, epi):
    Fp8Layout(GX.exact_case(M, N, K, epi)).run(lib)


@pytest.mark.parametrize("M,K,epi", [(257, 256, 3), (1, 128, 2)])
def test_fp8_gemm_in_place_residual(lib, M, K, epi):
    Fp8Layout(GX.exact_case(M, 256, K, epi), inplace=True).run(lib)


@pytest.mark.parametrize("epi,inplace", [(2, False), (3, True)])
def test_fp8_gemm_splitk(lib, epi, inplace):
    """Two K slices of 128: scaled fp32 slabs in a fenced workspace (only its fences are looked at), then the bf16 path's finalize."""
    M, N, K, S = 257, 256, 256, 2
    L = Fp8Layout(GX.exact_case(M, N, K, epi), inplace)
    n_ws = S * M * N
    ws_whole, ws = fenced(sentinel_like((n_ws,), torch.float32))
    L.run(lib, S, ws.data_ptr())
    got = ws_whole.cpu().view(torch.int32)
    fence = torch.full((FENCE,), SENTINEL[torch.float32], dtype=torch.int32)
    assert torch.equal(got[:FENCE], fence), "written in front of the split-K workspace"
    assert torch.equal(got[FENCE + n_ws:], fence), "written past the split-K workspace"


@pytest.mark.parametrize("R,N,K,epi,norm,p", [(1, 512, 4096, 1, False, 1), (3, 256, 4096, 1, False, 4), (4, 256, 4096, 2, True, 2), (2, 384, 6144, 2, True, 1)])
def test_fp8_decode_gemv_layout(lib, R, N, K, epi, norm, p):
    """aigv_op_skinny_gemm_fp8 on ldx = K + 8, ldw = K + 16 bytes, ldo = n_out + 12, ldr = n_out + 24: padding and fences bit for bit, the live
    values by test_fp8_decode_gemv's rule (its data, its restatement, its ulp_check)."""
    import math
    g = torch.Generator().manual_seed(R + N + K + p)
    x = (torch.randn(R, K, generator=g) * 0.7).to(BF)
    x[:, 5] *= 6.0
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    gw = (torch.rand(K, generator=g) + 0.5).to(BF) if norm else None
    eps = 1e-5
    nout = N // 2 if epi == 2 else N
    resid = torch.randn(R, nout, generator=g).to(BF) if epi == 1 else None
    xin = x
    if norm:
        xf = x.float()
        xin = (gw.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(BF).float()).to(BF)
    qa, sa = _quant_ref(xin)
    qw, sw = _quant_ref(w)
    acc = ((qa.float().double() @ qw.float().double().t()).float() * sa[:, None]) * sw[None, :]
    want = _epilogue_ref(acc, 4 if epi == 2 else 3, None, None, resid)
    ldx, ldw, ldo, ldr = K + 8, K + 16, nout + 12, nout + 24
    dx = dev(padded_rows(x, ldx, 2))
    w8 = torch.full((N, ldw), 0x7f, dtype=torch.uint8)
    w8[:, :K] = qw.view(torch.uint8)
    dw8 = dev(w8)
    dsw_whole, sw_ptr = padded_vec(sw)
    dgw, gw_ptr = padded_vec(gw)
    dr = dev(padded_rows(resid, ldr, 2)) if resid is not None else None
    before = sentinel_like((FENCE_ROWS + R + FENCE_ROWS, ldo), BF)
    whole, view = fenced(before)
    sync(lib.aigv_op_skinny_gemm_fp8(dx.data_ptr(), ldx, R, dw8.data_ptr(), ldw, ctypes.cast(sw_ptr, ctypes.POINTER(ctypes.c_float)), N, K,
                                     dr.data_ptr() if dr is not None else None, ldr if dr is not None else 0, view.data_ptr() + FENCE_ROWS * ldo * 2, ldo,
                                     epi, gw_ptr, eps, p, None), lib)
    got = whole.cpu()[FENCE:FENCE + before.numel()].view(before.shape)
    image = before.clone()
    image[FENCE_ROWS:FENCE_ROWS + R, :nout] = got[FENCE_ROWS:FENCE_ROWS + R, :nout]
    same_bits(whole, image)
    ulp_check(got[FENCE_ROWS:FENCE_ROWS + R, :nout], want, frac=0.03, max_ulps=4 if epi == 2 else 2, atol_rel=2.0 ** -7 if epi == 1 else 2e-5)
