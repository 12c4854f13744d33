"""CPU side of the GEMM layout tests (tests/test_gpu_gemm_layouts.py, tests/test_gemm_layouts_cpu.py): GEMM cases whose arithmetic is exact.

A and W are sparse with entries from {0, +-0.5, +-1, +-2}: every product is a multiple of the quantum Q = 2^-2.  As long as, for every
output element, sum_k |a||w| + |bias| (+ |pos|) stays below 2^8 Q, every partial sum - of any K slice, any MFMA chain, any split-K slab
and its finalize pass, in any order - is a multiple of Q below 2^8 Q: exact in fp32 and a bf16 number.  Bias, residual and position rows are
multiples of Q, layer-scale entries powers of two, and the same bound holds at the later rounding points (``is_exact`` states it).  For the
epilogues 0 (store), 2 (layer-scale + residual), 3 (residual) and 5 (patch) ``want`` is then the ONLY correct bit pattern, whatever kernel,
tile, slice or row plan computed it.  GELU (1) and SwiGLU (4) get an exact argument; their own rounding is judged by the rules of the
tests in tests/test_gpu_ops.py.

Plain torch on the CPU; no GPU call."""
import functools

import torch

BF = torch.bfloat16
Q = 0.25
LIMIT = 2.0 ** 8 * Q
EXACT_EPILOGUES = (0, 2, 3, 5)


def n_out(N, epi):
    return N // 2 if epi == 4 else N


def patch_np(M):
    """Patches per frame of a patch-epilogue case with M rows: M over its smallest prime factor (several frames wherever M is composite)."""
    for d in range(2, M + 1):
        if M % d == 0:
            return M // d
    return 1


def _draw(M, N, K, epi, seed):
    g = torch.Generator().manual_seed(90001 * seed + 7 * M + 3 * N + K + 1000003 * epi)
    # GELU: its argument must stay in |x| <= 4 (the range test_gelu_epilogue_over_all_bf16_inputs bounds to one ulp): three products of
    # at most 1 and a bias of at most 1
    a_vals = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    w_vals = torch.tensor([0.5, -0.5]) if epi == 1 else a_vals
    nnz = min(3 if epi == 1 else 6, K)
    A = a_vals[torch.randint(0, len(a_vals), (M, K), generator=g)] * (torch.rand(M, K, generator=g) < 0.5)
    cols = torch.rand(N, K, generator=g).argsort(1)[:, :nnz]
    W = torch.zeros(N, K).scatter_(1, cols, w_vals[torch.randint(0, len(w_vals), (N, nnz), generator=g)])
    case = {"M": M, "N": N, "K": K, "epi": epi, "A": A.to(BF), "W": W.to(BF), "bias": None, "ls": None, "resid": None, "pos": None, "np": 0}
    no = n_out(N, epi)
    if epi in (0, 1, 2, 5):
        case["bias"] = (torch.randint(-4, 5, (N,), generator=g) * Q).to(BF)
    if epi == 2:
        case["ls"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)].to(BF)
    if epi in (2, 3):
        case["resid"] = (torch.randint(-16, 17, (M, no), generator=g) * Q).to(BF)
    if epi == 5:
        case["np"] = patch_np(M)
        case["pos"] = (torch.randint(-16, 17, (case["np"] + 1, N), generator=g) * Q).to(BF)
    return case


def _a_wt(A, W):
    """float64 A W^T.  W has a handful of non-zeros per row, so the product is taken through its sparse form: the same float64 sums as the
    dense product (zeros add nothing) at a cost that does not grow with K - the largest cost-model case stays well under a second."""
    return torch.sparse.mm(W.double().to_sparse(), A.double().t()).t().contiguous()


def linear(case):
    """float64 A W^T + bias: the accumulator every epilogue starts from."""
    acc = _a_wt(case["A"], case["W"])
    return acc if case["bias"] is None else acc + case["bias"].double()


def _multiple(x, q):
    return bool(((x / q) == (x / q).round()).all())


def is_exact(case):
    """The bound of the module docstring, in float64, at every rounding point of the case's epilogue."""
    epi = case["epi"]
    mag = _a_wt(case["A"].abs(), case["W"].abs())
    if case["bias"] is not None:
        mag = mag + case["bias"].double().abs()
    y = linear(case)
    if not (bool((mag < LIMIT).all()) and _multiple(y, Q)):
        return False
    if epi == 1:
        return bool((y.abs() <= 4.0).all())
    if epi == 2:                                   # bf16(resid + bf16(y * ls)): ls = 2^e scales the grid, the sum lives on the finer of the two
        ls, r = case["ls"].double(), case["resid"].double()
        q2 = Q * ls.clamp(max=1.0)
        return bool((mag * ls + r.abs() < 2.0 ** 8 * q2).all()) and _multiple(r, Q)
    if epi == 3:
        return bool((mag + case["resid"].double().abs() < LIMIT).all()) and _multiple(case["resid"].double(), Q)
    if epi == 5:
        m = torch.arange(case["M"])
        p = case["pos"].double()[(m % case["np"]) + 1]
        return bool((mag + p.abs() < LIMIT).all()) and _multiple(p, Q)
    return True


def want(case):
    """The result rows [M, n_out] as bf16: float64 arithmetic cast to bf16 once per rounding point of the kernels (for an exact case none of
    them rounds).  Epilogue 5: the M patch rows, in input order (``patch_rows`` maps them to their output rows).  GELU: torch's bf16 GELU of
    the exact argument.  SwiGLU: the rounding points of the kernels on the exact gate and up values."""
    epi, y = case["epi"], linear(case)
    if epi == 4:
        blk = y.view(y.shape[0], case["N"] // 32, 2, 16)
        gt, up = blk[:, :, 0, :].reshape(y.shape[0], -1).to(BF), blk[:, :, 1, :].reshape(y.shape[0], -1).to(BF)
        return (torch.nn.functional.silu(gt.float()).to(BF).float() * up.float()).to(BF)
    y = y.to(BF)
    if epi == 1:
        return torch.nn.functional.gelu(y)
    if epi == 2:
        y = (y.double() * case["ls"].double()).to(BF)
    if epi in (2, 3):
        y = (case["resid"].double() + y.double()).to(BF)
    if epi == 5:
        m = torch.arange(case["M"])
        y = (y.double() + case["pos"].double()[(m % case["np"]) + 1]).to(BF)
    return y


def patch_rows(M, np_):
    """Output row of input row m under the patch epilogue: one class row is skipped in front of every frame."""
    m = torch.arange(M)
    return m + m // np_ + 1


def distinguishes_positions(case, w):
    """A shifted, swapped or skipped row, tile or segment cannot give ``w`` by accident.  What is guaranteed, exactly: every row differs
    from the next one and from the rows 128 and 256 below it; no row equals its residual row; every 4- and 8-column segment differs from
    its right-hand neighbour in the first row, in the last row (the row that sits alone in a ragged last tile at M = 129, 257, 513) AND in
    at least one row of every band of 128 rows (every half tile of every kernel).  Not guaranteed: that two neighbouring segments differ
    in EVERY row - the sums take a few dozen values, so among the 10^5 to 10^7 segment pairs of a case some coincide, whatever the draw."""
    b = w.view(torch.int16)
    for d in (1, 128, 256):
        if b.shape[0] > d and not bool((b[d:] != b[:-d]).any(1).all()):
            return False
    for s in (4, 8):
        seg = b.view(b.shape[0], b.shape[1] // s, s)
        differs = (seg[:, 1:] != seg[:, :-1]).any(2)                 # [row, segment pair]
        if not bool(differs[0].all() and differs[-1].all()):
            return False
        for r0 in range(0, b.shape[0], 128):
            if not bool(differs[r0:r0 + 128].any(0).all()):
                return False
    if case["resid"] is not None and not bool((b != case["resid"].view(torch.int16)).any(1).all()):
        return False
    return True


@functools.lru_cache(maxsize=None)
def exact_case(M, N, K, epi, seed=0):
    """A, W and whatever the epilogue needs (dict; see ``_draw``), with ``want`` under key "want".  The draw is repeated with another seed
    until ``want`` distinguishes positions (a one-row case can draw two equal neighbouring segments); key "draw" says which draw it was.
    Whether the case is exact is NOT assumed here: the tests assert ``is_exact`` first.  Cached: the tests share one case, and must leave
    it unchanged."""
    for attempt in range(16):
        case = _draw(M, N, K, epi, seed + 1000 * attempt)
        case["want"] = want(case)
        case["draw"] = attempt
        if distinguishes_positions(case, case["want"]):
            return case
    raise AssertionError(f"no draw of M={M} N={N} K={K} epi={epi} distinguishes positions")


# ---------------------------------------------------------------------------------------------------------
# the fp8 form: the same case behind power-of-two row and column scales
# ---------------------------------------------------------------------------------------------------------
def fp8_operands(case):
    """aigv_op_gemm_fp8 computes bf16((sum_k A8 W8) * row_scale[m] * col_scale[n] + bias).  A8 = A / row_scale and W8 = W / col_scale with
    scales from {0.5, 1, 2} that change from row to row and column to column: entries of magnitude 0.25 .. 4, all e4m3 numbers, and every
    partial sum is the bf16 case's times one power of two - as exact as that one, so ``want`` is unchanged.  A wrong scale index, or a scale
    left out, moves the result by a factor of 2 or 4."""
    M, N = case["M"], case["N"]
    rs = torch.tensor([0.5, 1.0, 2.0])[(torch.arange(M) * 5 + 1) % 3]
    cs = torch.tensor([2.0, 0.5, 1.0])[(torch.arange(N) // 3 + torch.arange(N)) % 3]
    A8 = (case["A"].float() / rs[:, None]).to(torch.float8_e4m3fn)
    W8 = (case["W"].float() / cs[:, None]).to(torch.float8_e4m3fn)
    return {"A8": A8, "W8": W8, "row_scale": rs, "col_scale": cs}


def fp8_is_exact(case, ops):
    """The bf16 case is exact, the scales are powers of two, and the e4m3 operands times their scales ARE the bf16 operands."""
    def pow2(t):
        return bool((t > 0).all() and (t.double().log2() == t.double().log2().round()).all())
    return (is_exact(case) and pow2(ops["row_scale"]) and pow2(ops["col_scale"])
            and torch.equal(ops["A8"].float() * ops["row_scale"][:, None], case["A"].float())
            and torch.equal(ops["W8"].float() * ops["col_scale"][:, None], case["W"].float()))


# ---------------------------------------------------------------------------------------------------------
# the layouts and shapes of tests/test_gpu_gemm_layouts.py (its CPU companion tests/test_gemm_layouts_cpu.py reads them here too)
# ---------------------------------------------------------------------------------------------------------
def strides(no, K, ldo_pad=8):
    """lda = K + 8, ldw = K + 16, ldc = n_out + 8, ldr = n_out + 24: pairwise different, and different from N and K.  (n_out == K would make
    lda == ldc: lda = K + 32 there.)"""
    lda, ldw, ldc, ldr = K + 8, K + 16, no + ldo_pad, no + 24
    if lda == ldc:
        lda = K + 32
    assert len({lda, ldw, ldc, ldr}) == 4 and not {lda, ldw, ldc, ldr} & {no, 2 * no, K}
    return lda, ldw, ldc, ldr


SHAPES_128 = [(M, N, K) for M in (1, 127, 129, 300) for N in (128, 384) for K in (64, 192)]
SHAPES_256 = [(M, N, K) for M in (1, 255, 257, 514) for N in (256, 512) for K in (64, 128)]
SHAPES_SPLITK_128 = [(M, 384, 384) for M in (4, 130, 300)]
SHAPES_SPLITK_256 = [(M, 256, 384) for M in (256, 513)]
SHAPES_FP8 = [(M, 256, K) for M in (1, 257) for K in (128, 256)]

# Cost-model dispatch (mode 0): one shape per feature of run_gemm, the smallest a search over aigv_plan_gemm found.  Searched: M*N*K minimal
# over N in 256..4096 step 128, K in 64..4096 step 64, M = 256 j + r (r in steps of 16, and 1) up to 800 rows for the first two features
# and up to 15000 for the others.  The bands of the 256 kernel only pay once a problem fills more than one round of the chip: below ~1e9
# multiply-adds the model runs everything in one launch of the 256 kernel or on the 128 / skinny kernels.
COST_MODEL = {
    # feature: (M, N, K, epi, what the plan must show)
    "skinny_remainder": (1, 256, 128, 0, lambda p: p[4] == 1 and p[3] == 1),                          # the smallest
    "skinny_remainder_ls_resid": (33, 256, 128, 2, lambda p: p[4] == 1 and p[3] == 33),                # three row tiles of the skinny kernel
    "skinny_remainder_ls_resid_2_tiles": (17, 256, 128, 2, lambda p: p[4] == 1 and p[3] == 17),
    "skinny_remainder_ls_resid_4_tiles": (64, 256, 128, 2, lambda p: p[4] == 1 and p[3] == 64),
    "splitk_last_band_128": (1, 256, 960, 3, lambda p: p[4] == 2 and p[5] > 1),                       # the smallest
    "splitk_last_band_128_ragged": (130, 256, 960, 2, lambda p: p[4] == 2 and p[5] > 1),
    "splitk_mid_band_256": (1280, 3328, 3840, 2, lambda p: p[1] > 0 and p[2] > 1),
    "top_band_then_last_band": (7169, 2304, 64, 2, lambda p: p[0] > 0 and p[3] > 0 and p[4] == 2),
    "right_hand_column_band": (6792, 2432, 64, 2, lambda p: p[6] == 128),                             # N = 256 * 9 + 128; bias, ls and residual
}

ROW_LISTS = {
    "whole_tiles": [512, 256],
    "tails_up_to_and_above_128": [300, 77, 449],
    "tiny_tails": [257, 3, 260],
    "uniform_tiny_tails_1": [257, 257, 257],           # the tiny rows share one skinny launch whose row stride is the sequence length
    "uniform_tiny_tails_4": [260, 260],
    "short_next_to_long": [40, 600],
}
K_ROWS = 512

# One case of each inexact epilogue (GELU, SwiGLU) run over EVERY route: the accumulators are exact in any order, so all routes must give the
# same bits (test_gelu_and_swiglu_bits_agree_on_every_route).  M = 520 as the row list 257 + 3 + 260: a ragged 256 tile, a tiny tail, a tail
# above 128; the skinny kernel takes the first CROSS_ROUTE_SKINNY_ROWS rows of the same A.
CROSS_ROUTE = [(520, 256, K_ROWS, 1), (520, 256, K_ROWS, 4)]
CROSS_ROUTE_LENS = ROW_LISTS["tiny_tails"]
CROSS_ROUTE_TAIL_LENS = [40, 480]              # the same 520 rows with a ragged tile tail (224 rows) for the fused and the lone row plans
CROSS_ROUTE_SKINNY_ROWS = 64


def first_rows(case, R):
    """The case of the first R rows of ``case``'s A (GELU / SwiGLU cases: no residual, no position rows): a sub-case of an exact case."""
    assert case["resid"] is None and case["pos"] is None
    return dict(case, M=R, A=case["A"][:R].contiguous(), want=case["want"][:R].contiguous())


SK_OF = {0: 0, 3: 1, 4: 2, 1: 3}                 # GEMM epilogue -> aigv_op_skinny_gemm epilogue (store, residual, swiglu, gelu)
K_SKINNY = 512
# the sub-slab forms p = 2 / 4 take at most 16 / p rows and have no GELU epilogue: only the legal combinations are cases
SKINNY_CASES = [(N, R, p, epi) for N in (128, 288) for R in (1, 5, 64) for p in (1, 2, 4) for epi in (0, 1, 3, 4) if p == 1 or (R <= 16 // p and epi != 1)]


def tile_cases():
    """(M, N, K, epi) of every aigv_op_gemm* and aigv_op_gemm_fp8 case of tests/test_gpu_gemm_layouts.py."""
    out = [(M, N, K, e) for M, N, K in SHAPES_128 + SHAPES_256 for e in range(6)]
    out += [(M, N, K, e) for M, N, K, e, _ in COST_MODEL.values()] + [(M, N, K, 3) for M, N, K, e, _ in COST_MODEL.values()]
    out += [(M, N, K, e) for M, N, K in SHAPES_SPLITK_128 + SHAPES_SPLITK_256 + SHAPES_FP8 for e in range(5)]
    out += [(sum(lens), N, K_ROWS, e) for lens in ROW_LISTS.values() for N in (256, 512) for e in range(5)]
    out += CROSS_ROUTE
    return sorted(set(out))


def skinny_cases():
    return sorted({(R, N, K_SKINNY, e) for N, R, p, e in SKINNY_CASES})
