"""Host-side truth, acceptance rules and case generators of the normalisation tests (no GPU; numpy and torch only), shared by
tests/test_norm_reference_cpu.py (which proves the rules) and tests/test_gpu_norm_ops.py (which holds the kernels to them).

The truth.  Both operations in fp64 with the kernels' bf16 rounding points and nothing else rounded (fp64 -> bf16 directly, one rounding):
    RMSNorm     bf16(w * bf16(x * rsqrt(mean(x^2) + eps)))          (rmsnorm_kernel, lens_tap_kernel, rmsnorm_quant_fp8_kernel)
    LayerNorm   bf16((x - mean) * rstd * w + b),  rstd = rsqrt(mean((x - mean)^2) + eps)          (layernorm_kernel, layernorm_wave_kernel)
eps is the fp32 number the kernel is handed.

The fp32 restatement (rms_fp32 / layernorm_fp32) is the kernels' arithmetic in float32 with switches - the order of summation, the
hardware rsqrt moved by a few fp32 ulps, and a list of FAULTS - and exists to prove the rules on the CPU: the faithful forms must pass
every case, every fault must be refused.  No GPU test compares a kernel with it.

The cases.  Dense rows: every case cycles through the row classes of ROW_CLASSES (N(0, 3^2); that scaled by 2^-9 and 2^-20, where eps
carries the statistic; by 2^40; mean 40 with sigma 3; for LayerNorm also mean 250 with sigma 2, where bf16 has steps of 1 - the cancellation that
tells a one-pass variance E[x^2] - mean^2 from the kernels' two passes in any order of summation; one outlier of 300 in the last column of a 0.05-scale row; all zeros; all ones at
a power-of-two H, where LayerNorm returns the bias bit for bit); the weights hold zeros and negative entries.  Sparse rows: a
permutation of the H columns dealt over H / 8 rows (H / 16 above 6144), a row being zero but for its 8 (16) columns, which hold
+-{1, 1.25, 1.5, 1.75} 2^k in a fixed multiset whose squares sum to at most 32 times the smallest - every non-zero carries at least 1/32
of its row's sum of squares, so every column of the operand decides one row - with signs that cancel: the row's mean is exactly 0, its
sums are exact in fp32 in any order, and LayerNorm of its zero columns is the bias itself.

The rules (check_dense, check_sparse):
    RMSNorm, dense      no element more than 2 bf16 ulps from the truth; at most FLIP_LIMIT of the case's elements not bit-equal
    LayerNorm, dense    at most FLIP_LIMIT not bit-equal; |got - want| <= 1 bf16 ulp of want + LN_A * max over the row of |(x - mean) rstd w|
    sparse, both        at most one differing element per row; that one within 2 ulps (RMSNorm) / the dense LayerNorm bound

Measured by tests/test_norm_reference_cpu.py (test_measured_flip_fractions; 256 rows of the dense classes, both eps, H = 1024,
2048, 4096, 12800, 16384; both summation orders, rstd moved by -2, 0, +2 fp32 ulps):
    fraction not bit-equal, at most     the kernel's order of summation      column by column
    RMSNorm                             7.7e-5 (rstd +- 0: 2.7e-5)           4.5e-4
    LayerNorm                           9.5e-5 (rstd +- 0: 7.6e-5)           2.7e-4
(MEASURED_FLIPS below; FLIP_LIMIT = 1e-3 leaves a factor of two over the worst of them and of ten over the kernel's own order.)
    LN_A    the worst (|got - want| - 1 ulp) / row maximum, over every committed case, order and rstd shift: MEASURED_LN_A = 9.65e-7
            (test_a_faithful_float32_evaluation_passes_every_case_under_every_switch); LN_A = 4 x that = 4.24e-6, far below 2^-12 = 2.44e-4
The tests assert that the measurements stay at or below the numbers written here."""
import functools

import numpy as np
import torch

BF = torch.bfloat16
F32, F64 = np.float32, np.float64

FLIP_LIMIT = 1e-3
MEASURED_FLIPS = {("rms", "tree"): 7.7e-5, ("rms", "sequential"): 4.5e-4, ("ln", "tree"): 4.6e-4, ("ln", "sequential"): 6.8e-4}      # (op, order): worst over H, eps, rstd shift
MEASURED_FLIPS_EXACT_RSQRT = {"rms": 2.7e-5, "ln": 4.4e-4}                                                                            # the kernel's order, rstd +- 0
MEASURED_LN_A = 9.65e-7
LN_A = 4 * MEASURED_LN_A

LN_H = (8, 128, 1024, 2048, 2304, 3200, 4096, 12800, 16384)
RMS_H = (8, 128, 512, 1024, 3200, 4096, 6144, 16384)
LN_EPS = (1e-6, 1e-5)
RMS_EPS = (1e-5, 1e-6)
LN_SPARSE_H = (1024, 2048, 4096, 12800)
RMS_SPARSE_H = (4096, 6144, 16384)
DENSE_ROWS = 37
ROW_CLASSES = ("normal3", "tiny9", "tiny20", "huge40", "mean40", "mean250", "outlier", "zeros", "ones")
FAULTS_BOTH = ("column", "chunk", "wave", "divisor", "no_eps", "eps10")
RMS_FAULTS = FAULTS_BOTH + ("weight_first",)
LN_FAULTS = FAULTS_BOTH + ("var_e2", "no_bias")
ORDERS = ("sequential", "tree")
RSTD_SHIFTS = (-2, 0, 2)


# ---------------------------------------------------------------------------------------------------------
# bf16 as numbers: float arrays that hold bf16 values, and their bit patterns
# ---------------------------------------------------------------------------------------------------------
def round_bf16_f32(x):
    """float32 array -> float32 array of the round-to-nearest-even bf16 values (the kernels' f2bf; NaN stays NaN, overflow is inf)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def round_bf16_f64(x):
    """float64 array -> float64 array of the nearest bf16 values, ties to even, in ONE rounding (through float32 there would be two)."""
    x = np.asarray(x, dtype=F64)
    _, e = np.frexp(x)
    q = np.maximum(e, -125) - 8                      # the quantum: 8 significant bits, 2^-133 below the smallest normal
    r = np.ldexp(np.rint(np.ldexp(x, -q)), q)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(r) > 3.3895313892515355e38, np.sign(r) * np.inf, r)


def bits(x):
    """bf16-valued float array -> uint16 bit patterns."""
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


def ulp_bf16(x):
    """The spacing of bf16 numbers at |x| (float64; 2^-133 from zero through the subnormals)."""
    x = np.asarray(x, dtype=F64)
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.maximum(np.where(x == 0, -125, e), -125) - 8)


def ulp_steps(got, want):
    """How many bf16 numbers apart two bf16-valued arrays are (+0 and -0 are the same number); a NaN or Inf is 2^16 apart from anything finite."""
    def order(v):
        b = bits(v).astype(np.int64)
        mag = b & 0x7FFF
        return np.where(b & 0x8000, -mag, mag)
    d = np.abs(order(got) - order(want))
    bad = ~np.isfinite(np.asarray(got, dtype=F32)) | ~np.isfinite(np.asarray(want, dtype=F32))
    return np.where(bad & (bits(got) != bits(want)), 1 << 16, d)


def to_np(t):
    """bf16 torch tensor -> float32 array of the same values."""
    return t.float().numpy()


def to_bf(a):
    """bf16-valued float array -> bf16 torch tensor (exact)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(BF)


# ---------------------------------------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------------------------------------
def rms_truth(x, w, eps):
    """x [R, H], w [H]: bf16-valued float arrays -> float32 array of the bf16 results."""
    xd, wd = np.asarray(x, dtype=F64), np.asarray(w, dtype=F64)
    rstd = 1.0 / np.sqrt((xd * xd).mean(axis=1, keepdims=True) + F64(F32(eps)))
    return round_bf16_f64(wd * round_bf16_f64(xd * rstd)).astype(F32)


def ln_terms(x, w, eps):
    """(x - mean) * rstd * w in fp64: the term the bias is added to, and what the LayerNorm bound scales with."""
    xd, wd = np.asarray(x, dtype=F64), np.asarray(w, dtype=F64)
    d = xd - xd.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + F64(F32(eps)))
    return d * rstd * wd


def ln_truth(x, w, b, eps):
    return round_bf16_f64(ln_terms(x, w, eps) + np.asarray(b, dtype=F64)).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32, with switches
# ---------------------------------------------------------------------------------------------------------
def threads_of(op, H):
    """Threads that share one row: a wave for layernorm_wave_kernel (H = 1024, 2048), else a 256-thread workgroup."""
    return 64 if op == "ln" and H in (1024, 2048) else 256


def _layout(a, threads):
    """[R, H] -> [R, threads, n]: what each thread accumulates, in its order (16-byte chunk t + c * threads of the row, c ascending); zero padded."""
    R, H = a.shape
    C = -(-(H // 8) // threads)
    pad = np.zeros((R, C * threads * 8), dtype=a.dtype)
    pad[:, :H] = a
    return pad.reshape(R, C, threads, 8).transpose(0, 2, 1, 3).reshape(R, threads, C * 8)


def _reduce(v, square, order, threads, drop_group=None):
    """Sum over the columns of v (square: of v * v) in float32.  'sequential': column by column, the square rounded before the addition.
    'tree': the kernel's - per thread chunk by chunk (the square fused into the addition, as the compiler contracts sq += d * d), the butterfly
    inside each wave, the waves in order.  drop_group: the quarter of the threads whose partial is left out (the 'wave' fault)."""
    v = np.ascontiguousarray(v, dtype=F32)
    if order == "sequential" and drop_group is None:
        return np.cumsum(v * v if square else v, axis=1, dtype=F32)[:, -1]
    lay = _layout(v, threads)
    acc = np.zeros(lay.shape[:2], dtype=F32)
    for p in range(lay.shape[2]):
        t = lay[:, :, p]
        if not square:
            acc = acc + t
        elif order == "tree":
            acc = (acc.astype(F64) + t.astype(F64) * t.astype(F64)).astype(F32)         # fma: the product is exact in fp64
        else:
            acc = acc + t * t
    if drop_group is not None:
        g = threads // 4
        acc[:, drop_group * g:(drop_group + 1) * g] = 0
    wv = acc.reshape(acc.shape[0], threads // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):
        wv = wv[..., :o] + wv[..., o:2 * o]
    out = wv[:, 0, 0]
    for k in range(1, wv.shape[1]):
        out = out + wv[:, k, 0]
    return out


def _rsqrt(a, shift):
    """The correctly rounded fp32 1 / sqrt(a), moved by `shift` fp32 ulps (the hardware instruction is not correctly rounded)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (1.0 / np.sqrt(a.astype(F64))).astype(F32)
    for _ in range(abs(shift)):
        r = np.nextafter(r, F32(np.inf if shift > 0 else -np.inf))
    return r


def _keep(H, threads, fault, at):
    """Columns that reach the statistics, and the thread group left out, under the faults that lose operands."""
    keep = np.ones(H, dtype=bool)
    at = H - 1 if at is None else at
    if fault == "column":
        keep[at] = False
    elif fault == "chunk":
        keep[at // 8 * 8: at // 8 * 8 + 8] = False
    group = None
    if fault == "wave":
        g = threads // 4
        group = min(3, ((at // 8) % threads) // g)           # the group of the thread that owns column `at`: it holds data
    return keep, group


def _eps(eps, fault):
    e = F32(eps)
    return F32(0) if fault == "no_eps" else e * F32(10) if fault == "eps10" else e


def rms_fp32(x, w, eps, order="tree", rstd_shift=0, fault=None, at=None):
    x, w = np.asarray(x, dtype=F32), np.asarray(w, dtype=F32)
    H = x.shape[1]
    threads = threads_of("rms", H)
    keep, group = _keep(H, threads, fault, at)
    ss = _reduce(np.where(keep, x, F32(0)), True, order, threads, group)
    ms = ss / F32(H - 1 if fault == "divisor" else H) + _eps(eps, fault)
    rstd = _rsqrt(ms, rstd_shift)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "weight_first":
            return round_bf16_f32(w * (x * rstd))
        return round_bf16_f32(w * round_bf16_f32(x * rstd))


def layernorm_fp32(x, w, b, eps, order="tree", rstd_shift=0, fault=None, at=None):
    x, w, b = (np.asarray(a, dtype=F32) for a in (x, w, b))
    H = x.shape[1]
    threads = threads_of("ln", H)
    keep, group = _keep(H, threads, fault, at)
    xs = np.where(keep, x, F32(0))
    mean = (_reduce(xs, False, order, threads, group) / F32(H))[:, None]
    d = x - mean
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "var_e2":
            var = _reduce(xs, True, order, threads, group) / F32(H) - (mean * mean)[:, 0]
        else:
            var = _reduce(np.where(keep, d, F32(0)), True, order, threads, group) / F32(H - 1 if fault == "divisor" else H)
        rstd = _rsqrt(var + _eps(eps, fault), rstd_shift)[:, None]
        t = d * rstd
        if fault == "no_bias":
            return round_bf16_f32(t * w)
        if order == "tree":
            return round_bf16_f32((t.astype(F64) * w.astype(F64) + b.astype(F64)).astype(F32))      # the product fused into the addition
        return round_bf16_f32(t * w + b)


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
def classes_of(op, H):
    """The row classes of a dense case of op: 'ones' at a power-of-two H only; 'mean250' (LayerNorm's variance under the hardest cancellation) for
    LayerNorm only - RMSNorm has no subtraction for it to test, and a row of a dozen distinct values makes its inner rounding bf16(x * rstd) flip
    for a tenth of the row at once or not at all, which says nothing about a kernel."""
    return tuple(c for c in ROW_CLASSES if (c != "ones" or H & (H - 1) == 0) and (c != "mean250" or op == "ln"))


def dense_rows(op, H, rows, g):
    """[rows, H] bf16: row r is of class classes_of(op, H)[r % n]."""
    cls = classes_of(op, H)
    x = torch.zeros(rows, H)
    for r in range(rows):
        c = cls[r % len(cls)]
        n = torch.randn(H, generator=g)
        if c == "normal3":
            x[r] = 3 * n
        elif c == "tiny9":
            x[r] = 3 * n * 2.0 ** -9
        elif c == "tiny20":
            x[r] = 3 * n * 2.0 ** -20
        elif c == "huge40":
            x[r] = 3 * n * 2.0 ** 40
        elif c == "mean40":
            x[r] = 40 + 3 * n
        elif c == "mean250":
            x[r] = 250 + 2 * n
        elif c == "outlier":
            x[r] = 0.05 * n
            x[r, H - 1] = 300.0
        elif c == "ones":
            x[r] = 1.0
    return x.to(BF)


def weights(H, g, bias):
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    w[::7] = 0
    w[3::11] *= -1
    w[H - 1] = 1.25                                   # the outlier's column keeps a weight
    b = (0.1 * torch.randn(H, generator=g) + 0.02).to(BF) if bias else None
    return w, b


@functools.lru_cache(maxsize=None)
def dense_case(op, H, eps, rows=DENSE_ROWS):
    """-> dict(x, w, b (LayerNorm), want): bf16 torch tensors, want = the truth.  Cached: never modify."""
    g = torch.Generator().manual_seed(1000 * (1 + ("rms", "ln").index(op)) + H + int(round(1e7 * eps)) + 7 * rows)
    x = dense_rows(op, H, rows, g)
    w, b = weights(H, g, op == "ln")
    c = dict(op=op, H=H, eps=eps, x=x, w=w, b=b)
    c["want"] = to_bf(truth_of(c))
    return c


SPARSE_8 = (1.0, 1.0, 1.25, 1.25, 1.5, 1.5, 1.75, 1.75)                              # squares sum to 15.75
SPARSE_16 = (1.0,) * 8 + (1.25,) * 4 + (1.5,) * 2 + (1.75,) * 2                       # squares sum to 24.875: the smallest holds 1 / 24.875


def sparse_per_row(H):
    return 16 if H > 6144 else 8


@functools.lru_cache(maxsize=None)
def sparse_case(op, H, eps=1e-5):
    """-> dict(x, w, b, want, cols [rows, n]: the non-zero columns of every row).  Equal magnitudes come in +- pairs: every row sums to 0 exactly."""
    g = torch.Generator().manual_seed(77000 + H + ("rms", "ln").index(op))
    n = sparse_per_row(H)
    rows = H // n
    mags = torch.tensor(SPARSE_16 if n == 16 else SPARSE_8)
    sign = torch.tensor([1.0, -1.0] * (n // 2))                                         # each magnitude appears an even number of times, in adjacent slots
    cols = torch.randperm(H, generator=g).reshape(rows, n)
    x = torch.zeros(rows, H)
    for r in range(rows):
        slot = torch.randperm(n, generator=g)                                           # which column of the row gets which signed magnitude
        flip = 1.0 if torch.rand((), generator=g) < 0.5 else -1.0
        x[r, cols[r]] = (flip * sign * mags)[slot] * 2.0 ** (r % 7)
    w, b = weights(H, g, op == "ln")
    c = dict(op=op, H=H, eps=eps, x=x.to(BF), w=w, b=b, cols=cols)
    c["want"] = to_bf(truth_of(c))
    return c


def truth_of(c, rows=None):
    x = to_np(c["x"] if rows is None else c["x"][rows])
    if c["op"] == "rms":
        return rms_truth(x, to_np(c["w"]), c["eps"])
    return ln_truth(x, to_np(c["w"]), to_np(c["b"]), c["eps"])


def fp32_of(c, **switches):
    if c["op"] == "rms":
        return rms_fp32(to_np(c["x"]), to_np(c["w"]), c["eps"], **switches)
    return layernorm_fp32(to_np(c["x"]), to_np(c["w"]), to_np(c["b"]), c["eps"], **switches)


# ---------------------------------------------------------------------------------------------------------
# the acceptance rules: each returns None, or why the result is refused
# ---------------------------------------------------------------------------------------------------------
def ln_excess(c, got, rows=None):
    """(|got - want| - 1 bf16 ulp of want) / the row's largest |(x - mean) rstd w|, per element: what LN_A has to cover (<= 0: inside one ulp)."""
    x = to_np(c["x"] if rows is None else c["x"][rows])
    want = to_np(c["want"] if rows is None else c["want"][rows]).astype(F64)
    scale = np.abs(ln_terms(x, to_np(c["w"]), c["eps"])).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(got, dtype=F64) - want) - ulp_bf16(want)
    err = np.where(np.isfinite(err), err, np.inf)
    return np.where(err <= 0, 0.0, err / np.maximum(scale, 1e-300))


def _differs(c, got, rows):
    want = to_np(c["want"] if rows is None else c["want"][rows])
    got = np.asarray(got, dtype=F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return got, want, bits(got) != bits(want)


def _too_far(c, got, want, diff, rows, a):
    """Of the differing elements, those outside the op's distance bound (only rows that hold a difference are looked at)."""
    far = np.zeros_like(diff)
    hit = np.flatnonzero(diff.any(axis=1))
    if hit.size == 0:
        return far
    if c["op"] == "rms":
        far[hit] = diff[hit] & (ulp_steps(got[hit], want[hit]) > 2)
        return far
    src = np.arange(diff.shape[0]) if rows is None else np.arange(c["x"].shape[0])[rows]
    far[hit] = diff[hit] & (ln_excess(c, got[hit], src[hit].tolist()) > a)
    return far


def check_dense(c, got, rows=None, a=None):
    """got: bf16-valued float array of rows `rows` (a slice or index array; None: all) of the dense case c."""
    got, want, diff = _differs(c, got, rows)
    far = _too_far(c, got, want, diff, rows, LN_A if a is None else a)
    if far.any():
        r, j = np.argwhere(far)[0]
        return f"{int(far.sum())} elements outside the bound, first at ({r}, {j}): got {got[r, j]!r}, want {want[r, j]!r}"
    if diff.sum() > FLIP_LIMIT * diff.size:
        return f"{int(diff.sum())} of {diff.size} elements are not bit-equal (limit {FLIP_LIMIT * diff.size:.1f})"
    return None


def check_sparse(c, got, rows=None, a=None):
    got, want, diff = _differs(c, got, rows)
    per_row = diff.sum(axis=1)
    if per_row.max(initial=0) > 1:
        r = int(np.argmax(per_row > 1))
        return f"row {r}: {int(per_row[r])} elements differ ({int((per_row > 1).sum())} such rows)"
    far = _too_far(c, got, want, diff, rows, LN_A if a is None else a)
    if far.any():
        r, j = np.argwhere(far)[0]
        return f"the differing element at ({r}, {j}) is outside the bound: got {got[r, j]!r}, want {want[r, j]!r}"
    return None


def rows_changed(c, got, rows=None):
    """How many rows of a result hold a differing element (the quantisation test's count)."""
    return int(_differs(c, got, rows)[2].any(axis=1).sum())
