"""CPU side of the GEMM rounding tests (tests/test_gpu_gemm_rounding.py, tests/test_gemm_rounding_cpu.py): GEMM cases whose fp32 accumulator
is exact in ANY summation order and is NOT a bf16 number - it sits at a chosen distance from a rounding boundary, so every rounding point
of csrc/epilogue.h has one correct result, whichever kernel, K slice, split-K slab or row plan computed it.

tests/gemm_exact_reference.py pins addressing with sums that never round; this module pins the rounding decisions themselves.

Construction.  K is cut into eight classes of columns, k % 8 = slot.  W carries ONE value per (output column n, slot) in every column of
the slot's class; every row of A carries its factor of a slot in exactly ONE column of the class, in a K tile of 64 that rotates with the
row.  An accumulator is therefore a sum of at most three products (plus the bias),

    y[m, n] = a_base[m] w_base[n] + a_tail[m] w_tail[n] + a_sticky[m] w_sticky[n]     (+ bias[n])          "normal" columns
    y[m, n] = a_u1[m] w_u1[n] + a_u2[m] w_u2[n]                                                           "underflow" columns
    y[m, n] = a_o1[m] w_o1[n] + a_o2[m] w_o2[n]                                                           "overflow" columns

whose terms land in different K tiles and different split-K slices; zeros add nothing, so every partial sum, in any order and on any
slab, is a subset sum of these few terms.  Both factors are bf16 numbers of few significant bits: the column factor carries the binade
(1, 2^9, 2^-11), a base such as 1, 1 + 2^-7 or 2 - 2^-7, half an ulp of it and a sticky term of 2^-12 .. 2^-15 of either sign; the row
factor carries a sign, a power-of-two scale, a tail multiplier (1 or 3: the tie moves to the neighbour of the other parity) and a sticky
multiplier (1, -1, 2).  The class of a column therefore changes from row to row, and EVERY non-zero row carries every class (the first and
the last row included: the last one sits alone in a ragged tile at M = 129, 257, 513).

Exactness is asserted, not assumed (``exactness``): for every element, with q the largest power of two dividing every term that feeds one
fp32 add and S the sum of their magnitudes, S < 2^16 q - every subset sum fits 17 significant bits, far inside fp32's 24 - at the
accumulator and again at every later fp32 add of the chain (bf16 x bf16 products are exact in fp32 without any bound).  The float64 sum then
IS the fp32 accumulator, and ``want`` is float64 arithmetic cast to bf16 once per rounding point.  24-bit-wide sums are out of scope: they
would measure the MFMA's internal adder, not this project's code.

Classes are not claimed by the generator: ``classify`` reads them off the exact accumulator, and the census, the placement conditions
(``placement_holes``) and the mutant conditions (``mutant_counts``: truncation, round-half-up, round-half-away, a skipped Linear or
layer-scale rounding, flushed subnormals, saturation, a dropped sign of zero must each change ``want`` in every band of 128 rows and in the
last row) are asserted on the CPU.

Plain torch / numpy on the CPU; no GPU call."""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

from gemm_exact_reference import (BF, n_out, patch_np, patch_rows, strides, distinguishes_positions, first_rows, SK_OF, K_SKINNY,  # noqa: F401
                                  SKINNY_CASES, CROSS_ROUTE_LENS, CROSS_ROUTE_TAIL_LENS)

BASE, TAIL, STICKY, U1, U2, O1, O2, FINE = range(8)          # slot = k % 8 (FINE: the fp8 form only)
SLOT_START = {BASE: 0.0, TAIL: 3 / 8, STICKY: 6 / 8, U1: 1 / 8, U2: 5 / 8, O1: 1 / 8, O2: 5 / 8, FINE: 1 / 2}      # first K tile of a slot, as a fraction of K
BOUND = 2.0 ** 16
BF_MAX = 2.0 ** 128 - 2.0 ** 120
CLASSES = ("exact", "tie_even_down", "tie_even_up", "above_tie", "below_tie", "other", "underflow", "overflow", "zero")
ROUNDING_CLASSES = ("tie_even_down", "tie_even_up", "above_tie", "below_tie", "carry")
NEAR = 2.0 ** -4                 # "a tie +- a sticky term": within 1/16 ulp of the halfway point (2^-12 relative is 2^-5 ulp)

# the seven designs of a normal column: (base, sign of the sticky term); the tail is half an ulp of [1, 2), 2^-8.  With the row's tail
# multiplier (1 | 3) and sticky multiplier (> 0 | < 0) they give: tie to even below | above; the reverse; above | below a tie; the reverse;
# a carry into the exponent | a quarter ulp; a tie to even below | a carry; below | above a tie - every class in every row.
NORMAL = ((1.0, 0), (1 + 2.0 ** -7, 0), (1 + 2.0 ** -6, 1), (1.5 + 2.0 ** -7, -1), (2 - 2.0 ** -7, 0), (2 - 2.0 ** -6, 0), (1.75 + 2.0 ** -7, -1))
# by epilogue.  GELU keeps |x| <= 4: its upper binade is [2, 4].  SwiGLU: silu(gate) of a large negative gate is a zero, whatever was rounded
BINADES = {0: (1.0, 2.0 ** 9, 2.0 ** -11), 1: (1.0, 2.0, 2.0 ** -11), 4: (1.0, 8.0, 2.0 ** -11)}
ROW_SCALES = {0: (1.0, 2.0, 0.5, 4.0), 1: (1.0, 0.5, 0.25, 0.125)}
# underflow columns: a_u1 w_u1 + a_u2 w_u2 = j 2^-14 alpha beta with a_u1 = alpha 129/128, a_u2 = alpha, w_u1 = beta x/128, w_u2 = -beta v/128,
# x = 128 + j, v = (129 x - j) / 128: two NORMAL products of normal operands that cancel down to an fp32 subnormal.  (j, log2 beta); alpha = 2^-60
UNDERFLOW = ((1, -60), (3, -60), (65, -66), (-1, -66))       # 2^-134 (tie -> 0), 3 2^-134 (-> 2^-132), 2^-134 + 2^-140 (-> 2^-133), -2^-140 (-> -0)
# overflow columns: 2^60 (255 2^60) + 2^60 w_o2.  2^128 - 2^119 is the tie between the largest bf16 and 2^128 (-> Inf); 2^128 - 2^119 - 2^112 -> 0x7f7f
# (a sticky term of 2^112, not 2^111: 2^128 - 2^119 - 2^111 has S = 2^17 q, one bit past the bound every other element keeps)
OVERFLOW = ((1, 2.0 ** 59), (1, 127 * 2.0 ** 52), (-1, 2.0 ** 59), (-1, 127 * 2.0 ** 52))
LS_MENU = (1.5, 1.0, 0.5, 1.25, -1.5, 2.0, 0.75)
# The fp8 form (aigv_op_gemm_fp8: bf16((sum_k A8 W8) * row_scale[m] * col_scale[n] + bias) and on).  e4m3 has four significant bits and no
# normal number below 2^-6, and the scales come from {0.5, 1, 2}: the same sums are made of operands that stay normal e4m3 numbers under
# every pair of scales.  The base is split into an e4m3 number and a FINE term in a slot of its own ((base, fine, tail in half ulps)
# below give tests NORMAL's bases: 2 - 2^-7 = 1.75 + 7 2^-5 + 6 2^-8, 2 - 2^-6 = 1.75 + 15 2^-6); the small terms are split between the
# two operands (tail 2^-8 = 2^-4 2^-4, sticky 2^-12 = 2^-5 2^-7) and the binades are 2^2, 2^4, 2^6 - a binade of 2^2 has room for a sticky
# term of 2^-12 only, 2^4 down to 2^-14.  No underflow or overflow class: e4m3 has not the range.
NORMAL_FP8 = ((1.0, 0.0, 1), (1.0, 2.0 ** -7, 1), (1.0, 2.0 ** -6, 1), (1.5, 2.0 ** -7, 1), (1.75, 7 * 2.0 ** -5, 7), (1.75, 15 * 2.0 ** -6, 1),
              (1.75, 2.0 ** -7, 1))
BINADES_FP8 = (16.0, 64.0, 4.0)
ROW_SCALES_FP8 = (1.0, 2.0, 1.0, 4.0)
A_TAIL_FP8, A_STICKY_FP8 = 2.0 ** -4, 2.0 ** -5                # the part of the small terms that A carries


# ---------------------------------------------------------------------------------------------------------
# rounding to bf16, stated on float64 values (all of them fp32 numbers: float64 holds them exactly)
# ---------------------------------------------------------------------------------------------------------
def _grid(x):
    """|x| in ulps of its bf16 binade: (whole ulps below, fraction of an ulp, ulp).  Exact: x has at most 24 significant bits."""
    ax = np.abs(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, ex = np.frexp(np.where(np.isfinite(ax), ax, 1.0))
    ulp = np.ldexp(1.0, np.maximum(ex - 1, -126) - 7)
    f = np.where(np.isfinite(ax), ax, 0.0) / ulp
    lo = np.floor(f)
    return lo, f - lo, ulp


def round_bf16(x, mode="rne", flush=False, saturate=False, drop_zero_sign=False):
    """x (float64) rounded to a bf16 number, as float64.  ``mode``: rne (the contract), trunc, half_up (ties towards +Inf), half_away.  The
    flags are the other wrong chains: subnormal results flushed to zero, overflow saturated to the largest finite value, -0 stored as +0."""
    x = np.asarray(x, dtype=np.float64)
    lo, frac, ulp = _grid(x)
    odd = np.mod(lo, 2.0) == 1.0
    up = {"rne": (frac > 0.5) | ((frac == 0.5) & odd), "trunc": np.zeros_like(odd), "half_up": (frac > 0.5) | ((frac == 0.5) & (x > 0)),
          "half_away": frac >= 0.5}[mode]
    mag = (lo + up) * ulp
    mag = np.where(mag >= 2.0 ** 128, BF_MAX if saturate else np.inf, mag)
    mag = np.where(np.isinf(x), BF_MAX if saturate else np.inf, mag)
    if flush:
        mag = np.where(mag < 2.0 ** -126, 0.0, mag)
    out = np.copysign(mag, x)
    if drop_zero_sign:
        out = np.where(out == 0, 0.0, out)
    return out


def rne_fraction(v):
    """Round-to-nearest-even to bf16 of ONE float, in exact rational arithmetic: the independent restatement ``want`` is checked against.
    Returns a float (a bf16 number, +-Inf, or a signed zero)."""
    if v == 0 or v != v or v in (float("inf"), float("-inf")):
        return v
    x = abs(Fraction(v))
    e = max(math.frexp(v)[1] - 1, -126)                             # 2^e <= |v| < 2^(e + 1); the subnormals share the last binade's grid
    ulp = Fraction(2) ** (e - 7)
    n, rest = divmod(x, ulp)
    if rest * 2 > ulp or (rest * 2 == ulp and n % 2 == 1):
        n += 1
    r = n * ulp
    r = float("inf") if r >= Fraction(2) ** 128 else float(r)
    return -r if v < 0 else r


def _low_bit(x):
    """The largest power of two dividing each element (Inf for zero)."""
    m, e = np.frexp(np.abs(x))
    mant = np.ldexp(m, 53).astype(np.int64)
    low = (mant & -mant).astype(np.float64)
    return np.where(mant == 0, np.inf, np.ldexp(low, e - 53))


def _bf(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(BF)     # x holds bf16 numbers: the cast is exact (signed zeros and Inf included)


# ---------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------
def slot_column(m, slot, K):
    """The ONE column of A's row m that carries its factor of ``slot``: a K tile that rotates with the row, and inside the tile one of the eight
    columns of the slot's class."""
    T = K // 64
    tile = (int(SLOT_START[slot] * T) + m) % T
    return tile * 64 + slot + 8 * ((m // T + 3 * slot) % 8)


def row_factors(m, M, epi, fp8=False):
    """(sign, scale, tail multiplier, sticky multiplier) of row m, or None for an all-zero row (one in every 64 rows, never the first or
    the last).  48 combinations in steps of 5: every 64 consecutive rows hold all of them, and rows 1, 128 and 256 apart differ."""
    if m % 64 == (37 + 5 * (m // 64)) % 64 and 0 < m < M - 1:        # (never 1, 128 or 256 rows apart)
        return None
    i = (5 * m + m // 64) % 48
    return (1.0, -1.0)[i % 2], (ROW_SCALES_FP8 if fp8 else ROW_SCALES.get(epi, ROW_SCALES[0]))[(i // 12) % 4], (1.0, 3.0)[(i // 2) % 2], (1.0, -1.0, 2.0)[(i // 4) % 3]


def column_factors(n, epi, special, fp8=False):
    """Column n: its W value per slot and its bias.  With ``special`` every fifth column is an underflow, an overflow or an all-zero column."""
    w, bias = [0.0] * 8, (-0.0 if n % 2 else 0.0)
    if special and n % 5 == 4:
        k = n // 5
        sub = (k // 3) % 4
        if k % 3 == 0:
            j, lb = UNDERFLOW[sub]
            x = 128 + abs(j)
            v = (129 * x - abs(j)) // 128
            assert 129 * x - 128 * v == abs(j)
            s = 1.0 if j > 0 else -1.0
            w[U1], w[U2] = s * 2.0 ** lb * x / 128, -s * 2.0 ** lb * v / 128
        elif k % 3 == 1:
            s, w2 = OVERFLOW[sub]
            w[O1], w[O2] = s * 255 * 2.0 ** 60, s * w2
        return w, bias
    q, r = divmod(n, 8)
    kind = (q + r) % 7                  # columns n and n + 56 share a design and a residue mod 8, and at most one of the two is special
    sg = -1.0 if q % 2 else 1.0
    if fp8:
        B = BINADES_FP8[q % 3]
        (c, fine, halves), s = NORMAL_FP8[kind], NORMAL[kind][1]
        sticky = 2.0 ** -min(12 + (q // 7) % 4, 11 + int(np.log2(B)) // 2)
        B *= sg
        w[BASE], w[FINE], w[TAIL], w[STICKY] = B * c, B * fine, B * halves * 2.0 ** -8 / A_TAIL_FP8, B * s * sticky / A_STICKY_FP8
        assert c + fine + (halves - 1) * 2.0 ** -8 == NORMAL[kind][0]
    else:
        B = sg * BINADES.get(epi, BINADES[0])[q % 3]
        c, s = NORMAL[kind]
        w[BASE], w[TAIL], w[STICKY] = B * c, B * 2.0 ** -8, B * s * 2.0 ** -(12 + (q // 7) % 4)
    if kind == 6 and epi in (0, 1, 2, 5):
        if q % 2:
            w[TAIL], bias = 0.0, B * 2.0 ** -8                       # the half ulp arrives with the bias, after the last product
        else:
            bias = -B * 2.0 ** -7                                    # a whole ulp
    return w, bias


def _operands(M, N, K, epi, special, fp8=False):
    A, W = np.zeros((M, K)), np.zeros((N, K))
    bias = np.zeros(N)
    for n in range(N):
        w, bias[n] = column_factors(n, epi, special, fp8)
        for slot in range(8):
            W[n, slot::8] = w[slot]
    for m in range(M):
        f = row_factors(m, M, epi, fp8)
        if f is None:
            continue
        sg, rho, tau, mu = f
        a = {BASE: sg * rho, TAIL: sg * rho * tau, STICKY: sg * rho * mu}
        if fp8:
            a = {BASE: sg * rho, FINE: sg * rho, TAIL: sg * rho * tau * A_TAIL_FP8, STICKY: sg * rho * mu * A_STICKY_FP8}
        if special:
            a.update({U1: sg * 2.0 ** -60 * 129 / 128, U2: sg * 2.0 ** -60, O1: sg * 2.0 ** 60, O2: sg * 2.0 ** 60})
        for slot, v in a.items():
            A[m, slot_column(m, slot, K)] = v
    return A, W, bias


def _second_term(t, m_idx, n_idx):
    """The residual / position element added to the bf16 value ``t`` of the chain, chosen so that the SECOND rounding decides: half an ulp of t
    (a tie the fused chain does not see), three halves, a tie +- a sticky eighth, the exact cancellation (-> +0), a signed zero.  Around
    zero and the subnormals: a signed zero.  Next to the largest finite value: half an ulp of it, same sign (the second rounding overflows).
    An Inf meets a signed zero or a finite value of its own sign."""
    sel = (3 * m_idx + n_idx + n_idx // 8) % 8                     # (changes along a row within one column residue mod 8 too)
    at = np.abs(t)
    zero = np.where((m_idx + n_idx) % 2 == 1, -0.0, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, ex = np.frexp(np.where(np.isfinite(at) & (at > 0), at, 1.0))
    h = np.ldexp(1.0, ex - 1 - 8)                                   # half an ulp of t
    sg = np.copysign(1.0, t)
    r = np.select([sel == 0, sel == 1, sel == 2, sel == 3, sel == 4, sel == 5, sel == 6],
                  [sg * h, -sg * h, zero, sg * 3 * h, -t, sg * 512 * h, sg * h * 1.125], sg * h * 0.875)
    r = np.where(at < 2.0 ** -100, zero, r)
    r = np.where(np.isfinite(at) & (at >= 2.0 ** 127), np.where(sel % 2 == 0, sg * 2.0 ** 119, zero), r)
    return np.where(np.isinf(t), np.where(sel % 3 == 0, sg * 2.0 ** 120, zero), r)


def pilot_column(m, K):
    """The column of A's row m that carries the row's pilot element (class k % 8 = 3: W is zero there in a case without special columns)."""
    return U1 + 8 * ((5 * m + 1) % (K // 8))


def fp8_scales(M, N):
    """Row and column scales from {0.5, 1, 2} that change from row to row and column to column (as tests/gemm_exact_reference.py's)."""
    return (torch.tensor([0.5, 1.0, 2.0])[(torch.arange(M) * 5 + 1) % 3], torch.tensor([2.0, 0.5, 1.0])[(torch.arange(N) // 3 + torch.arange(N)) % 3])


@functools.lru_cache(maxsize=None)
def rounding_case(M, N, K, epi, special=None, fp8=False, pilot=False):
    """A, W and whatever the epilogue needs, as tests/gemm_exact_reference.py's cases carry them, with ``want`` under key "want".
    ``special`` (underflow, overflow and all-zero columns) defaults to the epilogues 0, 2, 3, 5.  Whether the case is exact, holds every
    class where it must and tells every mutant apart is NOT assumed here: tests/test_gemm_rounding_cpu.py asserts it.  Cached: the tests
    share one case and must leave it unchanged."""
    special = epi in (0, 2, 3, 5) if special is None else special
    assert not (fp8 and special)
    A, W, bias = _operands(M, N, K, epi, special, fp8)
    if pilot:
        # aigv_op_skinny_gemm_fp8 quantises its bf16 rows itself, by 448 / amax (true IEEE divisions).  One element of +-448 row_scale[m] in
        # a column where every W is zero adds nothing to any sum and makes amax = 448 row_scale: 448 / amax IS 1 / row_scale and amax / 448 IS
        # row_scale, so the kernel's own quantisation yields exactly A8 = A / row_scale below, and its pilot byte the largest e4m3 number.
        assert fp8 and not special
        for m in range(M):
            A[m, pilot_column(m, K)] = (-448.0 if m % 2 else 448.0) * float(fp8_scales(M, N)[0][m])
    case = {"M": M, "N": N, "K": K, "epi": epi, "A": _bf(A), "W": _bf(W), "bias": _bf(bias) if epi in (0, 1, 2, 5) else None, "ls": None,
            "resid": None, "pos": None, "np": 0, "special": special, "pilot": pilot}
    assert np.array_equal(case["A"].double().numpy(), A) and np.array_equal(case["W"].double().numpy(), W), "an operand is not a bf16 number"
    mi, ni = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    if epi in (2, 3, 5):
        t = round_bf16(linear(case))
        if epi == 2:
            ls = np.array([LS_MENU[n % 7] if not (special and n % 5 == 4) else (1.0, 1.5, 0.5)[(n // 15) % 3] for n in range(N)])     # (n // 15: not in step with the kind of special column)
            case["ls"] = _bf(ls)
            with np.errstate(over="ignore"):
                t = round_bf16(t * ls)
        if epi == 5:
            case["np"] = np_ = patch_np(M)
            zero_row = np.array([row_factors(m, M, epi, fp8) is None for m in range(np_)])
            r = _second_term(np.where(zero_row[:, None], 0.0, t[:np_]), mi[:np_], ni[:np_])
            case["pos"] = _bf(np.concatenate([np.full((1, N), 7.0), r]))
        else:
            case["resid"] = _bf(_second_term(t, mi, ni))
    case["want"] = chain(case)
    if fp8:
        # A8 = A / row_scale, W8 = W / col_scale with scales from {0.5, 1, 2} that change from row to row and column to column (as
        # tests/gemm_exact_reference.py's fp8_operands): every partial sum is the bf16 case's times one power of two, ``want`` is unchanged
        rs, cs = fp8_scales(M, N)
        case["fp8"] = {"A8": (case["A"].float() / rs[:, None]).to(torch.float8_e4m3fn), "W8": (case["W"].float() / cs[:, None]).to(torch.float8_e4m3fn),
                       "row_scale": rs, "col_scale": cs}
    return case


def fp8_case(M, N, K, epi, pilot=False):
    """The fp8 form of a case: ``fp8_holes`` says whether the e4m3 operands times their scales ARE its A and W.  ``pilot``: the form for the
    kernel that quantises its rows itself."""
    return rounding_case(M, N, K, epi, False, True, pilot)


def fp8_holes(case):
    """What keeps the fp8 form from reproducing the bf16 case exactly (empty for a good case): operands that are no normal e4m3 numbers,
    scales outside {0.5, 1, 2}, operands times scales that are not A and W; with a pilot, a row whose amax is not 448 row_scale or whose
    pilot meets a non-zero W."""
    ops, holes = case["fp8"], []
    for k in ("A8", "W8"):
        v = ops[k].float()
        if ops[k].dtype != torch.float8_e4m3fn or not bool(((v == 0) | (v.abs() >= 2.0 ** -6)).all()) or not bool((v.abs() <= 448).all()):
            holes.append(f"{k}: a subnormal or non-finite e4m3 operand")
    for k in ("row_scale", "col_scale"):
        if not set(ops[k].tolist()) <= {0.5, 1.0, 2.0} or len(set(ops[k].tolist())) != min(3, ops[k].numel()):
            holes.append(f"{k}: {sorted(set(ops[k].tolist()))}")
    if not torch.equal(ops["A8"].float() * ops["row_scale"][:, None], case["A"].float()):
        holes.append("A8 * row_scale is not A")
    if not torch.equal(ops["W8"].float() * ops["col_scale"][:, None], case["W"].float()):
        holes.append("W8 * col_scale is not W")
    if case["pilot"]:
        A = case["A"].float()
        cols = torch.tensor([pilot_column(m, case["K"]) for m in range(case["M"])])
        if not torch.equal(A.abs().amax(1), 448.0 * ops["row_scale"]) or not torch.equal(A[torch.arange(case["M"]), cols].abs(), 448.0 * ops["row_scale"]):
            holes.append("a row's amax is not its pilot, 448 row_scale")
        if bool((case["W"].float()[:, cols] != 0).any()):
            holes.append("a pilot meets a non-zero W")
        inv, sx = torch.tensor(448.0) / A.abs().amax(1), A.abs().amax(1) / torch.tensor(448.0)        # fp32 divisions, as the kernel's
        if not torch.equal(inv, 1.0 / ops["row_scale"]) or not torch.equal(sx, ops["row_scale"]):
            holes.append("448 / amax or amax / 448 is not the row scale")
    return holes


# ---------------------------------------------------------------------------------------------------------
# the accumulator, its exactness, the chain and its wrong variants
# ---------------------------------------------------------------------------------------------------------
def terms(case):
    """[slots, M, N] float64: the products that make up every accumulator, read off A and W (not off the generator): A must hold at most one
    non-zero per row and column class k % 8."""
    A, W = case["A"].double().numpy(), case["W"].double().numpy()
    out = np.zeros((8, case["M"], case["N"]))
    for slot in range(8):
        cols = np.arange(slot, case["K"], 8)
        sub = A[:, cols]
        assert int((sub != 0).sum(1).max(initial=0)) <= 1, "a row of A carries two factors in one class of columns"
        k = cols[np.abs(sub).argmax(1)]
        out[slot] = A[np.arange(case["M"]), k][:, None] * W[:, k].T          # bf16 x bf16: exact in fp32, let alone float64
    return out


def linear(case):
    """float64 A W^T + bias: the accumulator every epilogue starts from (exact: see ``exactness``)."""
    y = terms(case).sum(0)
    return y if case["bias"] is None else y + case["bias"].double().numpy()[None, :]


def _bounded(parts):
    """S < 2^16 q for one fp32 add (or chain of adds) of ``parts``; adds with a non-finite part are exact by IEEE's rules."""
    parts = [np.broadcast_to(p, parts[0].shape) for p in parts]
    fin = np.all([np.isfinite(p) for p in parts], axis=0)
    safe = [np.where(fin, p, 0.0) for p in parts]
    q = np.min([_low_bit(p) for p in safe], axis=0)
    S = np.sum([np.abs(p) for p in safe], axis=0)
    return (S < BOUND * q) | ~fin | (S == 0)


def exactness(case):
    """The bound of the module docstring at every fp32 add of the case's chain: a dict stage -> number of elements that break it (all zero
    for an exact case).  Also: no subnormal operand, no subnormal single product, every partial sum finite, GELU arguments within |x| <= 4."""
    epi, t = case["epi"], terms(case)
    parts = list(t) + ([case["bias"].double().numpy()[None, :]] if case["bias"] is not None else [])
    bad = {"accumulator": int((~_bounded(parts)).sum())}
    ops = np.concatenate([case["A"].double().numpy().ravel(), case["W"].double().numpy().ravel()])
    bad["subnormal operand"] = int(((ops != 0) & (np.abs(ops) < 2.0 ** -126)).sum())
    bad["subnormal product"] = int(((t != 0) & (np.abs(t) < 2.0 ** -126)).sum())
    bad["partial sum overflows"] = int((np.abs(t).sum(0) >= 2.0 ** 128).sum())
    y1 = round_bf16(linear(case))
    if epi == 1:
        bad["gelu argument"] = int((np.abs(y1) > 4.0).sum())
    if epi in (1, 4):
        bad["non-finite"] = int((~np.isfinite(y1)).sum())
    if epi == 2:
        with np.errstate(over="ignore"):
            y1 = round_bf16(y1 * case["ls"].double().numpy())         # bf16 x bf16: exact
    if epi in (2, 3):
        r = case["resid"].double().numpy()
        bad["residual add"] = int((~_bounded([r, y1])).sum())
        with np.errstate(invalid="ignore"):
            bad["nan"] = int(np.isnan(r + y1).sum())
    if epi == 5:
        p = case["pos"].double().numpy()[(np.arange(case["M"]) % case["np"]) + 1]
        bad["position add"] = int((~_bounded([y1, p])).sum())
        with np.errstate(invalid="ignore"):
            bad["nan"] = int(np.isnan(y1 + p).sum())
    return bad


def is_exact(case):
    return not any(exactness(case).values())


def _act(name, x):
    """GELU / SiLU of bf16-valued float64 ``x`` as the reference computes them: in fp32 (the caller rounds)."""
    f = torch.nn.functional.gelu if name == "gelu" else torch.nn.functional.silu
    return f(torch.from_numpy(np.ascontiguousarray(x)).float()).double().numpy()


def chain(case, mode="rne", skip_linear=False, skip_ls=False, **flags):
    """The rounding chain of csrc/epilogue.h in float64 with one ``round_bf16`` per rounding point; the result rows [M, n_out] as bf16
    (epilogue 5: the M patch rows in input order).  The defaults are the contract (``want``); the arguments select the wrong chains of
    MUTANTS."""
    def rnd(x):
        return round_bf16(x, mode, **flags)
    epi, y = case["epi"], linear(case)
    with np.errstate(over="ignore", invalid="ignore"):
        if epi == 4:
            blk = y.reshape(y.shape[0], case["N"] // 32, 2, 16)
            g, u = blk[:, :, 0, :].reshape(y.shape[0], -1), blk[:, :, 1, :].reshape(y.shape[0], -1)
            if not skip_linear:
                g, u = rnd(g), rnd(u)
            return _bf(rnd(rnd(_act("silu", g)) * u))
        y = y if skip_linear and epi != 0 else rnd(y)
        if epi == 1:
            y = rnd(_act("gelu", y))
        if epi == 2:
            y = y * case["ls"].double().numpy()
            y = y if skip_ls else rnd(y)
        if epi in (2, 3):
            y = rnd(case["resid"].double().numpy() + y)
        if epi == 5:
            y = rnd(y + case["pos"].double().numpy()[(np.arange(case["M"]) % case["np"]) + 1])
    return _bf(y)


# name -> (arguments of ``chain``, the epilogues it applies to, whether it needs the special columns)
MUTANTS = {
    "truncate": ({"mode": "trunc"}, (0, 1, 2, 3, 4, 5), False),
    "round_half_up": ({"mode": "half_up"}, (0, 1, 2, 3, 4, 5), False),
    "round_half_away": ({"mode": "half_away"}, (0, 1, 2, 3, 4, 5), False),
    "skip_linear_rounding": ({"skip_linear": True}, (1, 2, 3, 4, 5), False),
    "skip_ls_rounding": ({"skip_ls": True}, (2,), False),
    "flush_subnormals": ({"flush": True}, (0, 2, 3, 5), True),
    "saturate": ({"saturate": True}, (0, 2, 3, 5), True),
    "drop_zero_sign": ({"drop_zero_sign": True}, (0, 2, 3, 5), True),
}


def mutants_of(case):
    return [name for name, (_, epis, needs_special) in MUTANTS.items() if case["epi"] in epis and (case["special"] or not needs_special)]


def bands(M):
    """The bands of 128 rows, and the last row on its own."""
    return [(r0, min(r0 + 128, M)) for r0 in range(0, M, 128)] + [(M - 1, M)]


def mutant_counts(case):
    """name -> [elements of ``want`` the mutant changes, per band of ``bands``].  NaN-free: bit patterns are compared."""
    w = case["want"].view(torch.int16)
    out = {}
    for name in mutants_of(case):
        got = chain(case, **MUTANTS[name][0]).view(torch.int16)
        diff = got != w
        out[name] = [int(diff[a:b].sum()) for a, b in bands(case["M"])]
    return out


# ---------------------------------------------------------------------------------------------------------
# classes, read off the exact numbers
# ---------------------------------------------------------------------------------------------------------
def classify(x):
    """The class of the rounding of every element of ``x`` (float64, fp32-exact) as an index into CLASSES, and whether it carries into the
    exponent (a mantissa of all ones that rounds up)."""
    x = np.asarray(x, dtype=np.float64)
    lo, frac, _ = _grid(x)
    ax = np.abs(x)
    odd = np.mod(lo, 2.0) == 1.0
    c = np.full(x.shape, CLASSES.index("other"))
    c[(frac > 0.5) & (frac <= 0.5 + NEAR)] = CLASSES.index("above_tie")
    c[(frac < 0.5) & (frac >= 0.5 - NEAR)] = CLASSES.index("below_tie")
    c[(frac == 0.5) & ~odd] = CLASSES.index("tie_even_down")
    c[(frac == 0.5) & odd] = CLASSES.index("tie_even_up")
    c[frac == 0] = CLASSES.index("exact")
    c[(ax < 2.0 ** -126) & (frac != 0)] = CLASSES.index("underflow")
    c[(ax > BF_MAX) & np.isfinite(ax)] = CLASSES.index("overflow")
    c[ax == 0] = CLASSES.index("zero")
    carry = (lo == 255) & (frac >= 0.5) & (ax <= BF_MAX)              # a normal number's mantissa is lo - 128: all ones, and RNE rounds up
    return c, carry


def tags(case):
    """name -> bool [M, N] (accumulator columns; SwiGLU: gate and up columns): the class of the Linear's rounding, ``carry``, and
    ``second_point`` - where a LATER rounding decides: the elements a chain without the Linear's rounding gets wrong (SwiGLU: the output
    columns, padded to N) - with ``second_point_opposed``, where the two roundings of the correct chain go opposite ways."""
    y = linear(case)
    c, carry = classify(y)
    out = {name: c == i for i, name in enumerate(CLASSES)}
    out["carry"] = carry
    if case["epi"] != 0:
        fused = chain(case, skip_linear=True).view(torch.int16) != case["want"].view(torch.int16)
        sp = np.zeros(y.shape, dtype=bool)
        sp[:, :fused.shape[1]] = fused.numpy()
        out["second_point"] = sp
    if case["epi"] in (3, 5):
        y1 = round_bf16(y)
        r = case["resid"].double().numpy() if case["epi"] == 3 else case["pos"].double().numpy()[(np.arange(case["M"]) % case["np"]) + 1]
        with np.errstate(invalid="ignore"):
            z = r + y1
            d1, d2 = np.sign(np.abs(y1) - np.abs(y)), np.sign(np.abs(round_bf16(z)) - np.abs(z))
        out["second_point_opposed"] = np.isfinite(z) & (d1 * d2 < 0)
    return out


def required_classes(case):
    need = list(ROUNDING_CLASSES) + (["second_point"] if case["epi"] != 0 else [])
    if case["epi"] in (3, 5):
        need.append("second_point_opposed")
    return need + (["underflow", "overflow", "zero"] if case["special"] else [])


def placement_holes(case):
    """The placement conditions, as a list of what is missing (empty for a good case).  Every required class occurs: in the first and in
    the last row; for M >= 128, in both 64-row halves of every band of 128 rows, at every column residue mod 8 (the scalar four-element
    form, both halves of every packed pair and the 8- and 16-byte store segments all meet it).  Each rounding class occurs with both signs,
    in [1, 2), in a binade above and in one below (the fp8 form: in three binades)."""
    M, N = case["M"], case["N"]
    t, holes = tags(case), []
    y = linear(case)
    for name in required_classes(case):
        for row in (0, M - 1):
            if not t[name][row].any():
                holes.append(f"{name}: not in row {row}")
        if M >= 128:
            for r0 in range(0, M, 64):
                for res in range(8):
                    if not t[name][r0:r0 + 64, res::8].any():
                        holes.append(f"{name}: not in rows {r0}..{min(r0 + 64, M) - 1} at column residue {res}")
    for name in ROUNDING_CLASSES:
        v = y[t[name]]
        ex = np.floor(np.log2(np.abs(v)))
        if not ((v > 0).any() and (v < 0).any()):
            holes.append(f"{name}: one sign only")
        if "fp8" in case:                                             # (e4m3 operands under scales of 0.5 .. 2 do not reach down to [1, 2))
            if len(set(ex.tolist())) < 3:
                holes.append(f"{name}: binades {sorted(set(ex.tolist()))}")
        elif not ((ex == 0).any() and (ex > 0).any() and (ex < 0).any()):
            holes.append(f"{name}: binades {sorted(set(ex.tolist()))}")
    return holes


def census(case):
    t = tags(case)
    return {name: int(v.sum()) for name, v in t.items()}


# ---------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gemm_rounding.py
# ---------------------------------------------------------------------------------------------------------
EVERY_ROUTE = [(520, 256, 512, epi) for epi in range(6)]      # tests/gemm_exact_reference.py's CROSS_ROUTE shape: 257 + 3 + 260 and 40 + 480 rows
RAGGED = [(M, N, K, epi) for M, N, K in ((1, 128, 64), (129, 128, 192), (257, 256, 128), (513, 256, 384)) for epi in (0, 2, 3)]
SKINNY = [(R, p, epi) for R, p in ((1, 1), (5, 1), (64, 1), (1, 2), (5, 2), (1, 4), (4, 4)) for epi in (0, 3, 1, 4) if p == 1 or epi != 1]
N_SKINNY = 288


def tile_cases():
    return sorted(set(EVERY_ROUTE + RAGGED))


def skinny_cases():
    return sorted({(R, N_SKINNY, K_SKINNY, epi) for R, p, epi in SKINNY})


FP8 = [(257, 256, 256, epi) for epi in (0, 2, 3, 4)]            # one shape of tests/gemm_exact_reference.py's SHAPES_FP8; two K slices of 128


def fp8_cases():
    return list(FP8)


# aigv_op_skinny_gemm_fp8 without a norm (its residual epilogue; the SwiGLU and rope forms only exist with the fused RMSNorm): the shapes
# of tests/test_gpu_gemm_layouts.py's test_fp8_decode_gemv_layout.  (R, N, K, p); R <= 4 and <= 16 / p
SKINNY_FP8 = [(1, 512, 4096, 1), (4, 256, 4096, 1), (4, 256, 4096, 2), (3, 256, 4096, 4)]


def skinny_fp8_cases():
    return sorted({(R, N, K, 3) for R, N, K, p in SKINNY_FP8})
