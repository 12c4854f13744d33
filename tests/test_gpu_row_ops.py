"""Op-level parity tests (MI355X only) of the kernels that used to run only inside the whole-model tests: the score head (NaN guard, the
ReLU GEMM layers, the tail kernel), the fused RMSNorm + fp8 row quantisation, RoPE on a slot range (the K-only form of the prefill and
extend passes), the embedding gather, the position / sequence-id kernel and the row movers.  Each is called through its aigv_op_* entry.

Every output buffer sits between two fences (and keeps padding columns where ld > H), all filled with a sentinel: the WHOLE allocation
is compared bit for bit with a CPU image built from the same sentinel, so a write outside the documented region shows like a wrong
value does.  Every index handed to a kernel lies inside its table."""
import ctypes

import numpy as np
import pytest
import torch

import score_head_reference as SH
from test_gpu_ops import BF, dev, lib, rb, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu

FENCE = 64                       # elements in front of and behind every output (keeps 16-byte alignment for every dtype used here)
INT_OF = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32}


SENTINEL = {torch.bfloat16: 0x4ABC, torch.float32: 0x4ABCDEF0, torch.uint8: 0xA5, torch.int32: -77777}      # bit patterns


def fenced(image):
    """A device copy of the CPU tensor ``image`` between two fences of FENCE sentinel elements: returns (the whole allocation, the view a
    kernel gets).  ``image`` itself holds the sentinel (or its input data) wherever the kernel must not write."""
    flat = image.reshape(-1)
    whole = torch.empty(flat.numel() + 2 * FENCE, dtype=image.dtype)
    whole.view(INT_OF[image.dtype]).fill_(SENTINEL[image.dtype])
    whole[FENCE:FENCE + flat.numel()] = flat
    d = dev(whole)
    return d, d[FENCE:FENCE + flat.numel()].view(image.shape)


def sentinel_like(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    t.view(INT_OF[dtype]).fill_(SENTINEL[dtype])
    return t


def same_bits(whole_dev, want_image):
    """The whole allocation (fences included) against the CPU image of the region between the fences."""
    dt = INT_OF[want_image.dtype]
    got = whole_dev.cpu().view(dt)
    n = want_image.numel()
    fence = torch.full((FENCE,), SENTINEL[want_image.dtype], dtype=dt)
    assert torch.equal(got[:FENCE], fence), "written in front of the buffer"
    assert torch.equal(got[FENCE + n:], fence), "written past the buffer"
    want = want_image.reshape(-1).view(dt)
    bad = (got[FENCE:FENCE + n] != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {n} elements differ, first at flat index {int(bad[0])}"


def ptr(t):
    from aigv_assessor_amd.native import ptr as p
    return p(t)


def i32(values):
    from aigv_assessor_amd.native import i32_array
    return i32_array(values)


# ---------------------------------------------------------------------------------------------------------
# score head
# ---------------------------------------------------------------------------------------------------------
PRODUCTION = (4096, 1024, 256, 64, 16, 1)
CHAINS = [PRODUCTION,
          (6144, 1024, 256, 64, 16, 1),
          (64, 16, 1),                   # everything in the tail kernel
          (256, 30, 1),                  # a fan-out that is no multiple of 4 sends a 256-wide layer to the tail
          (1024, 1024, 1)]               # the tail at its 1024 limit


def run_score_head(lib, x, dims, Ws, bs, ldx=None):
    """x: CPU bf16 [B, H].  ldx > H: the rows are laid out with NaN padding columns (a kernel that read them would trip its own guard).
    Returns the fp32 scores; the fences of the score and of the scratch buffer are checked."""
    B, H = x.shape
    ldx = H if ldx is None else ldx
    xp = torch.full((B, ldx), float("nan"), dtype=BF)
    xp[:, :H] = x
    n = len(Ws)
    wd, bd = [dev(w) for w in Ws], [dev(b) for b in bs]
    wp, bp = (ctypes.c_void_p * n)(*[ptr(w) for w in wd]), (ctypes.c_void_p * n)(*[ptr(b) for b in bd])
    n_scratch = 3 * B * max(dims)
    scratch_whole, scratch = fenced(sentinel_like((n_scratch,), BF))
    score_whole, score = fenced(sentinel_like((B,), torch.float32))
    sync(lib.aigv_op_score_head(ptr(dev(xp)), ldx, B, n, i32(dims), wp, bp, ptr(scratch), n_scratch * 2, ptr(score), None), lib)
    got = score_whole.cpu()
    fence = torch.full((FENCE,), SENTINEL[torch.float32], dtype=torch.int32)
    assert torch.equal(got[:FENCE].view(torch.int32), fence) and torch.equal(got[FENCE + B:].view(torch.int32), fence), "score fences"
    sw = scratch_whole.cpu().view(torch.int16)
    fence16 = torch.full((FENCE,), SENTINEL[BF], dtype=torch.int16)
    assert torch.equal(sw[:FENCE], fence16) and torch.equal(sw[FENCE + n_scratch:], fence16), "scratch fences"
    return got[FENCE:FENCE + B].clone()


@pytest.mark.parametrize("B", [1, 3, 17, 40, 64])         # one to four row tiles of the GEMM layers
@pytest.mark.parametrize("dims", CHAINS, ids=lambda d: "-".join(map(str, d)))
def test_score_head_exact_arithmetic(lib, dims, B):
    """Sparse dyadic weights, biases and inputs: every sum is a bf16 number (asserted on the CPU first), so the score must EQUAL the
    reference whatever the order of summation - any wrong row, bias, leading dimension or ping-pong buffer shows."""
    Ws, bs = SH.exact_weights(dims)
    for W in Ws:
        assert int((W != 0).sum(1).max()) <= 8 and set(W.float().unique().tolist()) <= {0.0, 1.0, -1.0, 0.5, -0.5}
    x = SH.exact_inputs(B, dims[0])
    assert SH.is_exact(x, Ws, bs), "the case is not exact: the test itself is wrong"
    want = SH.chain(x, Ws, bs).float()
    assert B < 3 or len(set(want.tolist())) >= 2, "the rows must not all score the same"
    got = run_score_head(lib, x, dims, Ws, bs)
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def test_score_head_exact_arithmetic_with_padded_rows(lib):
    Ws, bs = SH.exact_weights(PRODUCTION)
    x = SH.exact_inputs(17, 4096)
    assert SH.is_exact(x, Ws, bs)
    got = run_score_head(lib, x, PRODUCTION, Ws, bs, ldx=4096 + 40)
    assert torch.equal(got, SH.chain(x, Ws, bs).float())


@pytest.mark.parametrize("B", [17, 64])
def test_score_head_random_numerics(lib, B):
    """Dense random weights on the production chain.  Truth: fp64 sums with the chain's five bf16 rounding points.  The yardstick is the
    oracle's own error against that truth on the same inputs (oracle.score_head: bf16 F.linear on the CPU): the kernel's worst error
    may be at most twice that plus one bf16 ulp of the score - rounding flips at five rounding points compound, and neither order of
    summation is privileged.
    Measured (max |error| over the batch; scores 1.09 .. 3.86 for B = 17, 1.20 .. 7.97 for B = 64): the oracle equals the truth on both
    batches (error 0: its fp32 sums round to the same bf16 numbers at all five points), so the kernel has one bf16 ulp of the score.
    The test prints both errors."""
    from oracle import oracle as O
    g = torch.Generator().manual_seed(4000 + B)
    Ws = [(torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5).to(BF) for i, o in zip(PRODUCTION[:-1], PRODUCTION[1:])]
    Ws[-1] = Ws[-1].abs()                                        # one output unit: its weights' sign decides every row at once
    bs = [(0.1 * torch.randn(o, generator=g) + 0.05).to(BF) for o in PRODUCTION[1:]]
    x = torch.randn(B, 4096, generator=g).to(BF)
    truth = SH.chain(x, Ws, bs)
    assert (truth > 0).float().mean() >= 0.5, "the test would compare zeros"
    sd = {}
    for n, (W, b) in enumerate(zip(Ws, bs), 1):
        sd[f"mlpscore.fc{n}.weight"], sd[f"mlpscore.fc{n}.bias"] = W, b
    oracle = O.score_head(sd, None, x).squeeze(1).double()
    got = run_score_head(lib, x, PRODUCTION, Ws, bs).double()
    assert torch.isfinite(got).all()
    ulp = truth.abs().clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -7
    err_oracle = (oracle - truth).abs().max().item()
    err_kernel = (got - truth).abs().max().item()
    print(f"score head B={B}: oracle-vs-truth {err_oracle:.6g}, kernel-vs-truth {err_kernel:.6g}, max score {truth.max().item():.4g}")
    assert ((got - truth).abs() - ulp).max().item() <= 2 * err_oracle, (err_kernel, err_oracle)


INF_COL, NINF_COL, NAN_COL = 2, 33, 18      # columns whose unit reaches the score through the sparse exact weights (asserted below)


def _guard_inputs(B, nan_at):
    x = SH.exact_inputs(B, 4096)
    x[0, INF_COL] = float("inf")
    x[5, NINF_COL] = float("-inf")
    if nan_at is not None:
        x[nan_at] = float("nan")
    return x


@pytest.mark.parametrize("B,nan_at", [(8, (2, NAN_COL)), (64, (63, 4095))], ids=["nan-in-row-2", "nan-last-element-B64"])
def test_score_head_nan_guard_fires_for_the_whole_slice(lib, B, nan_at):
    """One NaN anywhere: every row goes through nan_to_num(nan = 0, posinf = 1e9, neginf = -1e9), 1e9 being torch's own bf16 value.  The
    exact weights keep the result independent of the summation order next to the +-1e9 terms too (single_big_term), so it must EQUAL
    the reference chain on the guarded input."""
    Ws, bs = SH.exact_weights(PRODUCTION)
    x = _guard_inputs(B, nan_at)
    xg = torch.nan_to_num(x, nan=0.0, posinf=1e9, neginf=-1e9)
    assert xg.dtype == BF and torch.equal(SH.guard(x), xg)
    assert SH.single_big_term(xg, Ws, bs), "the case depends on the summation order: the test itself is wrong"
    want = SH.chain(xg, Ws, bs).float()
    assert torch.isfinite(want).all()
    assert want[0] > 1e6 and want[5] > 1e6, "the replaced infinities must reach the score"
    got = run_score_head(lib, x, PRODUCTION, Ws, bs)
    assert torch.isfinite(got).all(), got.tolist()
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def test_score_head_guard_stays_off_without_a_nan(lib):
    """+-Inf but no NaN: the reference leaves x alone (CHAT:469-473 tests isnan only), the infinite rows turn into NaN in the first Linear
    (Inf * 0) and stay NaN through every ReLU (F.relu keeps a NaN); the other rows are untouched.  Compared with NaN positions included."""
    Ws, bs = SH.exact_weights(PRODUCTION)
    x = _guard_inputs(8, None)
    assert torch.equal(SH.guard(x).view(torch.int16), x.view(torch.int16))
    want = SH.chain(x, Ws, bs).float()
    finite = torch.tensor([False, True, True, True, True, False, True, True])
    assert torch.equal(torch.isfinite(want), finite) and torch.isnan(want[~finite]).all()
    got = run_score_head(lib, x, PRODUCTION, Ws, bs)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want)), (got.tolist(), want.tolist())
    assert torch.allclose(got, want, rtol=0, atol=0, equal_nan=True), (got.tolist(), want.tolist())


@pytest.mark.parametrize("dirty", [False, True], ids=["finite", "nan-and-inf"])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("dims", CHAINS, ids=lambda d: "-".join(map(str, d)))
def test_score_head_is_the_one_group_case_of_the_grouped_op(lib, dims, B, dirty):
    """aigv_op_score_head(x, B) and aigv_op_score_head_groups(x, G = 1, stride 0, B): the same bits, with a NaN in one row and an Inf in
    another (the guard fires for the slice) and without."""
    g = torch.Generator().manual_seed(7000 + B + len(dims))
    Ws = [(torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5).to(BF) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * torch.randn(o, generator=g) + 0.05).to(BF) for o in dims[1:]]
    x = torch.randn(B, dims[0], generator=g).to(BF)
    if dirty:
        x[B // 2, 3] = float("nan")
        x[B - 1, 7] = float("inf")
    single = run_score_head(lib, x, dims, Ws, bs)
    n = len(Ws)
    xd, wd, bd = dev(x), [dev(w) for w in Ws], [dev(b) for b in bs]
    wp, bp = (ctypes.c_void_p * n)(*[ptr(w) for w in wd]), (ctypes.c_void_p * n)(*[ptr(b) for b in bd])
    n_scratch = 3 * B * max(dims)
    scratch_whole, scratch = fenced(sentinel_like((n_scratch,), BF))
    score_whole, score = fenced(sentinel_like((B,), torch.float32))
    sync(lib.aigv_op_score_head_groups(ptr(xd), dims[0], 1, 0, B, n, i32(dims), wp, bp, ptr(scratch), n_scratch * 2, ptr(score), None), lib)
    grouped = score_whole.cpu()[FENCE:FENCE + B]
    assert torch.equal(grouped.view(torch.int32), single.view(torch.int32)), (grouped.tolist(), single.tolist())
    sw = scratch_whole.cpu().view(torch.int16)
    fence16 = torch.full((FENCE,), SENTINEL[BF], dtype=torch.int16)
    assert torch.equal(sw[:FENCE], fence16) and torch.equal(sw[FENCE + n_scratch:], fence16), "scratch fences"
    assert dirty or torch.isfinite(single).all()


# ---------------------------------------------------------------------------------------------------------
# RMSNorm fused with the fp8 row quantisation
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("H", [128, 1032, 4096, 6144, 16384])
def test_rmsnorm_quant_fp8_is_the_two_step_path_bit_for_bit(lib, H, rows):
    """The fused kernel promises the bytes and scales of rmsnorm_kernel followed by quant_fp8_rows_kernel (rmsnorm_kernel is held to the fp64
    truth by tests/test_gpu_norm_ops.py, which also holds this kernel to it directly; the row quantisation is tied to torch by
    tests/test_gpu_ops.py): compared bit for bit, so no +-0 difference either - both convert with the same instruction."""
    g = torch.Generator().manual_seed(H + rows)
    ldx, ldq = H + 24, H + 16
    x = torch.full((rows, ldx), float("nan"), dtype=BF)          # NaN padding columns: reading them would poison the row's statistics
    x[:, :H] = (torch.randn(rows, H, generator=g) * 3).to(BF)
    zero_row = outlier_row = tiny_row = None
    if rows > 1:
        zero_row, outlier_row, tiny_row = 0, 7, rows - 1
        x[zero_row, :H] = 0
        x[outlier_row, :H] = (torch.randn(H, generator=g) * 0.05).to(BF)
        x[outlier_row, H // 2 + 3] = 300.0
        x[tiny_row, :H] = 2.0 ** -20
    else:
        x[0, H - 1] = 300.0                                        # the outlier in the last chunk of the last thread that has one
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    w[::7] = 0
    w[3::11] *= -1
    w[H // 2 + 3] = w[H - 1] = 1.25                                 # the outliers keep a weight
    dx, dw = dev(x), dev(w)
    eps = 1e-5
    # two steps: bf16 y [rows, H], then the row quantisation
    y = torch.empty(rows, H, dtype=BF, device="cuda")
    q2_whole, q2 = fenced(sentinel_like((rows, ldq), torch.uint8))
    s2_whole, s2 = fenced(sentinel_like((rows,), torch.float32))
    sync(lib.aigv_op_rmsnorm(ptr(dx), ldx, ptr(dw), ptr(y), H, rows, H, eps, None, None), lib)
    sync(lib.aigv_op_quant_fp8_rows(ptr(y), H, rows, H, ptr(q2), ldq, ptr(s2), None), lib)
    # fused
    q1_whole, q1 = fenced(sentinel_like((rows, ldq), torch.uint8))
    s1_whole, s1 = fenced(sentinel_like((rows,), torch.float32))
    sync(lib.aigv_op_rmsnorm_quant_fp8(ptr(dx), ldx, ptr(dw), ptr(q1), ldq, ptr(s1), rows, H, eps, None), lib)
    want_q, want_s = q2.cpu(), s2.cpu()
    assert (want_q[:, H:] == SENTINEL[torch.uint8]).all(), "the two-step path wrote its padding columns"
    assert torch.isfinite(want_s).all() and (want_s > 0).all()
    same_bits(q1_whole, want_q)
    same_bits(s1_whole, want_s)
    got_q, got_s = q1.cpu(), s1.cpu()
    if rows > 1:
        # an all-zero row: scale 1, every byte a zero.  0 * w keeps the sign of w (IEEE, and so does torch), hence 0x80 under a negative weight
        zero_bytes = torch.signbit(w).to(torch.uint8) * 0x80
        assert got_s[zero_row] == 1.0 and torch.equal(got_q[zero_row, :H], zero_bytes)
        assert ((got_q[outlier_row, :H] & 0x7F) == 0x7E).sum() == 1                                  # the outlier alone reaches +-448 (0x7E)
        live = (w != 0)
        assert ((got_q[tiny_row, :H] & 0x7F) != 0)[live].all()                                       # tiny inputs are normalised, not flushed
    assert ((got_q[:, :H][:, w == 0] & 0x7F) == 0).all()                                             # zero norm weights give (signed) zero bytes


# ---------------------------------------------------------------------------------------------------------
# RoPE on a slot range
# ---------------------------------------------------------------------------------------------------------
MAX_POS = 300


def rope_case(T, n_kv, g_, D, seed, pad=8):
    from aigv_assessor_amd.modeling import rope_tables
    g = torch.Generator().manual_seed(seed)
    slots = g_ + 2
    row = n_kv * slots * D
    qkv = torch.randn(T, row + pad, generator=g).to(BF)             # the last ``pad`` columns of every row are padding (ld > the row)
    pos = torch.randint(0, MAX_POS, (T,), generator=g, dtype=torch.int32)
    pos[0], pos[-1], pos[T // 2] = 0, MAX_POS - 1, MAX_POS - 1        # the first and the last row of the tables
    cos, sin = rope_tables(D, 1e6, MAX_POS)
    return qkv, pos, cos, sin, slots, row


def rope_reference(qkv, pos, cos, sin, n_kv, slots, D, first, n_rot, row):
    """bf16 tensor ops = the reference's three rounding points (as test_rope_matches_reference_rounding builds it); everything outside
    slots [first, first + n_rot) of every group, and the padding columns, are the input."""
    T = qkv.shape[0]
    want = qkv.clone()
    v = want[:, :row].reshape(T, n_kv, slots, D)
    c = torch.cat([cos, cos], -1)[pos.long()][:, None, None, :]
    s = torch.cat([sin, sin], -1)[pos.long()][:, None, None, :]
    x = v[:, :, first:first + n_rot, :]
    rot = torch.cat((-x[..., D // 2:], x[..., : D // 2]), dim=-1)
    v[:, :, first:first + n_rot, :] = (x * c) + (rot * s)
    want[:, :row] = v.reshape(T, row)
    return want


@pytest.mark.parametrize("g_,n_kv,D", [(1, 1, 128), (4, 2, 128), (6, 8, 128), (2, 2, 64)])
def test_rope_k_only_form(lib, g_, n_kv, D):
    """first_rot = g, n_rot = 1: what every prefill and extend layer launches.  The K slots carry the reference's rotation bit for bit;
    every query slot, every V slot and the padding columns are the input, as are the fences."""
    T = 50
    qkv, pos, cos, sin, slots, row = rope_case(T, n_kv, g_, D, seed=g_ * 100 + n_kv * 10 + D)
    want = rope_reference(qkv, pos, cos, sin, n_kv, slots, D, g_, 1, row)
    w4, q4 = want[:, :row].reshape(T, n_kv, slots, D), qkv[:, :row].reshape(T, n_kv, slots, D)
    assert torch.equal(w4[:, :, :g_], q4[:, :, :g_]) and torch.equal(w4[:, :, g_ + 1], q4[:, :, g_ + 1]) and not torch.equal(w4[:, :, g_], q4[:, :, g_])
    whole, d = fenced(qkv)
    sync(lib.aigv_op_rope_slots(ptr(d), row + 8, ptr(dev(pos)), ptr(dev(cos)), ptr(dev(sin)), T, g_, 1, slots, n_kv, D, None), lib)
    same_bits(whole, want)


def test_rope_slots_from_zero_is_aigv_op_rope(lib):
    T, n_kv, g_, D = 50, 2, 4, 128
    qkv, pos, cos, sin, slots, row = rope_case(T, n_kv, g_, D, seed=5)
    dp, dc, ds = dev(pos), dev(cos), dev(sin)
    whole_a, a = fenced(qkv)
    whole_b, b = fenced(qkv)
    sync(lib.aigv_op_rope(ptr(a), row + 8, ptr(dp), ptr(dc), ptr(ds), T, g_ + 1, slots, n_kv, D, None), lib)
    sync(lib.aigv_op_rope_slots(ptr(b), row + 8, ptr(dp), ptr(dc), ptr(ds), T, 0, g_ + 1, slots, n_kv, D, None), lib)
    same_bits(whole_b, a.cpu())
    same_bits(whole_b, rope_reference(qkv, pos, cos, sin, n_kv, slots, D, 0, g_ + 1, row))


def test_rope_grid_stride_loop_wraps(lib):
    """2500 tokens x 8 groups x 7 slots x 8 chunks = 1.12 M chunks against 4096 blocks x 256 threads = 1.05 M: some threads take two."""
    T, n_kv, g_, D = 2500, 8, 6, 128
    assert T * n_kv * (g_ + 1) * (D // 16) > 4096 * 256
    qkv, pos, cos, sin, slots, row = rope_case(T, n_kv, g_, D, seed=6)
    whole, d = fenced(qkv)
    sync(lib.aigv_op_rope_slots(ptr(d), row + 8, ptr(dev(pos)), ptr(dev(cos)), ptr(dev(sin)), T, 0, g_ + 1, slots, n_kv, D, None), lib)
    same_bits(whole, rope_reference(qkv, pos, cos, sin, n_kv, slots, D, 0, g_ + 1, row))


# ---------------------------------------------------------------------------------------------------------
# embedding gather
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 4096, 6144])
@pytest.mark.parametrize("n_vis,n_mot", [(40, 9), (0, 9), (0, 0)], ids=["visual+motion", "motion-only", "tokens-only"])
def test_embed_selects_token_visual_and_motion_rows(lib, n_vis, n_mot, H):
    T, V = 300, 50
    g = torch.Generator().manual_seed(H + n_vis + n_mot)
    emb = torch.randn(V, H, generator=g).to(BF)
    vis = torch.randn(n_vis, H, generator=g).to(BF) if n_vis else None
    mot = torch.randn(n_mot, H, generator=g).to(BF) if n_mot else None
    ids = torch.randint(0, V, (T,), generator=g, dtype=torch.int64)      # valid everywhere: visual / motion positions carry an id of their own
    slot = torch.full((T,), -1, dtype=torch.int32)
    if n_vis + n_mot:
        where = torch.randperm(T, generator=g)[:200]
        slot[where] = torch.randint(0, n_vis + n_mot, (200,), generator=g, dtype=torch.int32)
        slot[where[0]], slot[where[1]] = 0, n_vis + n_mot - 1                # the first and the last row of the tables ...
        if n_vis and n_mot:
            slot[where[2]], slot[where[3]] = n_vis - 1, n_vis              # ... and both sides of the visual / motion boundary
    want = emb[ids].clone()
    s = slot.long()
    if n_vis:
        want[(s >= 0) & (s < n_vis)] = vis[s[(s >= 0) & (s < n_vis)]]
    if n_mot:
        want[s >= n_vis] = mot[s[s >= n_vis] - n_vis]
    assert (slot >= 0).sum() == (200 if n_vis + n_mot else 0) and (n_vis + n_mot == 0 or not torch.equal(want, emb[ids]))
    whole, out = fenced(sentinel_like((T, H), BF))
    sync(lib.aigv_op_embed(ptr(dev(ids)), ptr(dev(slot)), ptr(dev(emb)), ptr(dev(vis)) if n_vis else None, ptr(dev(mot)) if n_mot else None,
                           n_vis, ptr(out), T, H, None), lib)
    same_bits(whole, want)


# ---------------------------------------------------------------------------------------------------------
# positions, sequence ids and cu_seqlens as kernel arguments
# ---------------------------------------------------------------------------------------------------------
def _mixed_lengths():
    g = torch.Generator().manual_seed(127)
    return torch.randint(1, 8, (127,), generator=g).tolist()


@pytest.mark.parametrize("with_offsets", [False, True])
@pytest.mark.parametrize("lens", [[1, 255, 256, 257, 3], _mixed_lengths(), [1000]], ids=["block-boundaries", "127-sequences", "one-sequence"])
def test_seqpos_positions_sequence_ids_and_cu(lib, lens, with_offsets):
    n_seq = len(lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    tokens = int(cu[-1])
    off = (np.arange(n_seq, dtype=np.int32) * 37 + 5) % 5000 if with_offsets else np.zeros(n_seq, np.int32)
    seq = np.repeat(np.arange(n_seq, dtype=np.int32), lens)
    pos = (np.arange(tokens, dtype=np.int32) - cu[seq] + off[seq]).astype(np.int32)
    pos_whole, dpos = fenced(sentinel_like((tokens,), torch.int32))
    seq_whole, dseq = fenced(sentinel_like((tokens,), torch.int32))
    cu_whole, dcu = fenced(sentinel_like((n_seq + 1,), torch.int32))
    sync(lib.aigv_op_seqpos(i32(cu), n_seq, i32(off) if with_offsets else None, ptr(dpos), ptr(dseq), ptr(dcu), tokens, None), lib)
    same_bits(pos_whole, torch.from_numpy(pos))
    same_bits(seq_whole, torch.from_numpy(seq))
    same_bits(cu_whole, torch.from_numpy(cu))


# ---------------------------------------------------------------------------------------------------------
# row movers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 1024, 4096, 6144])
def test_gather_rows(lib, H):
    g = torch.Generator().manual_seed(H)
    R, ld = 40, H + 8
    src = torch.randn(R, ld, generator=g).to(BF)
    idx = torch.tensor([39, 0, 17, 17, 3, 39, 21, 1, 0, 38, 20], dtype=torch.int32)     # unsorted, with duplicates, first and last row
    whole, dst = fenced(sentinel_like((len(idx), H), BF))
    sync(lib.aigv_op_gather_rows(ptr(dev(src)), ld, ptr(dev(idx)), len(idx), ptr(dst), H, None), lib)
    same_bits(whole, src[idx.long(), :H].contiguous())


@pytest.mark.parametrize("H", [8, 1024, 4096, 6144])
def test_scatter_rows(lib, H):
    g = torch.Generator().manual_seed(H + 1)
    R, ld = 40, H + 8
    idx = torch.tensor([39, 0, 17, 3, 21, 17, 1, 38], dtype=torch.int32)                 # distinct but for the pair of 17s ...
    src = torch.randn(len(idx), H, generator=g).to(BF)
    src[5] = src[2]                                                                      # ... which carries identical rows
    before = torch.randn(R, ld, generator=g).to(BF)
    want = before.clone()
    want[idx.long(), :H] = src
    whole, dst = fenced(before)
    sync(lib.aigv_op_scatter_rows(ptr(dev(src)), ptr(dev(idx)), len(idx), ptr(dst), ld, H, None), lib)
    same_bits(whole, want)                                                                # unlisted rows and the padding columns: as before


@pytest.mark.parametrize("H", [1024, 3200])
def test_cls_rows(lib, H):
    g = torch.Generator().manual_seed(H + 2)
    F_, tpf = 3, 5
    before = torch.randn(F_ * tpf, H, generator=g).to(BF)
    cls = torch.randn(H, generator=g).to(BF)
    want = before.clone()
    want[::tpf] = cls
    whole, x = fenced(before)
    sync(lib.aigv_op_cls_rows(ptr(dev(cls)), ptr(x), F_, tpf, H, None), lib)
    same_bits(whole, want)


@pytest.mark.parametrize("n", [1, 256, 257, 600])
def test_write_ints(lib, n):
    vals = (np.arange(n, dtype=np.int64) * 2654435761 % (2 ** 31) - 2 ** 30).astype(np.int32)
    whole, dst = fenced(sentinel_like((n,), torch.int32))
    sync(lib.aigv_op_write_ints(i32(vals), n, ptr(dst), None), lib)
    same_bits(whole, torch.from_numpy(vals))
