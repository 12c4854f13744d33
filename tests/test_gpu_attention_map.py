"""Attention flow map on the MI355X: the all-rows MFMA kernel and its fold through aigv_op_attention_map (no model) on the op-level case of
tests/score_attention_reference.py - lengths 1, 258 and 513 packed, so that sequences start at the unaligned rows 1 and 259 - with ALL 772
rows checked: key census and one-hot selector (bit-exact), random data against float64 with the derived bound, a sequence alone against the
same sequence packed, the score-row probe on the same buffers, the fold, output fencing and refusals - and the armed scoring pass through the
model (``forward(return_segment_attention=True, return_row_attention=(lo, hi))``).  tests/test_attention_map_cpu.py holds, without a GPU,
the references' own consistency."""
import ctypes
import functools

import pytest
import torch

import aigv_assessor_amd as pkg
import attention_map_reference as M
import score_attention_reference as R
from aigv_assessor_amd import eval_utils, native, prompts, synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D, S, HK = R.D, R.S, R.N_KV
SENTINEL = 0x7FA5A5A5      # a NaN bit pattern the kernels cannot produce
PAD = 64                   # floats in front of and behind every output
T_ALL = sum(R.LENS)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


def bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def tables():
    cos, sin = R.rope_table(D, R.N_POS)
    return cos.cuda(), sin.cuda()


def fenced(n):
    whole = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, ctypes.c_void_p(whole.data_ptr() + 4 * PAD)


def unfenced(whole, n, what, written=True):
    w = whole.cpu()
    assert (w[:PAD] == SENTINEL).all() and (w[PAD + n:] == SENTINEL).all(), f"the map wrote outside {what}"
    if written:
        assert (w[PAD:PAD + n] != SENTINEL).all(), f"the map left part of {what} unwritten"
    else:
        assert (w[PAD:PAD + n] == SENTINEL).all(), f"a refused call wrote to {what}"
    return w[PAD:PAD + n].view(torch.float32).clone()


def amap(lib, fused_d, g, seg_d, lens=R.LENS, n_seg=S, fold=True, refused=None, **over):
    """aigv_op_attention_map on fused rows [T, HK (g + 2) D].  rows and seg_out each sit between two sentinel pads inside an allocation that
    starts as the sentinel: returns (fp32 [T, heads, n_seg], fp32 [B, heads, n_seg, n_seg] or None) after checking that the pads kept their
    bits and that every element was written.  refused: the call must fail with that word in its message and write nothing; over: arguments
    replaced for such a call."""
    h, ld, T, B = HK * g, HK * (g + 2) * D, sum(lens), len(lens)
    n_rows, n_fold = T * h * max(n_seg, 1), B * h * max(n_seg, 1) ** 2
    rows_w, rows_p = fenced(n_rows)
    fold_w, fold_p = fenced(n_fold)
    cos, sin = tables()
    a = dict(q=fused_d.data_ptr(), ldq=ld, k=fused_d.data_ptr() + 2 * g * D, ldk=ld, cu=native.i32_array(R.cu_of(lens)), n_seq=B, n_heads=h, n_kv=HK,
             qgs=(g + 2) * D, khs=(g + 2) * D, d=D, cos=cos.data_ptr(), sin=sin.data_ptr(), max_pos=cos.shape[0], seg=seg_d.data_ptr(), n_seg=n_seg,
             rows=rows_p, fold=fold_p if fold else None)
    a.update(over)
    rc = lib.aigv_op_attention_map(a["q"], a["ldq"], a["k"], a["ldk"], a["cu"], a["n_seq"], a["n_heads"], a["n_kv"], a["qgs"], a["khs"], a["d"], a["cos"], a["sin"],
                                   a["max_pos"], a["seg"], a["n_seg"], a["rows"], a["fold"], native.stream_ptr())
    torch.cuda.synchronize()
    if refused is not None:
        msg = lib.aigv_last_error(None).decode()
        assert rc == -1 and refused in msg and "aigv_op_attention_map" in msg, (rc, msg)
        unfenced(rows_w, n_rows, "rows", written=False)
        unfenced(fold_w, n_fold, "seg_out", written=False)
        return None
    native.check(rc)
    rows = unfenced(rows_w, n_rows, "rows").view(T, h, n_seg)
    return rows, (unfenced(fold_w, n_fold, "seg_out").view(B, h, n_seg, n_seg) if fold else None)


# ---- 1. key census ----------------------------------------------------------------------------------------------------------------
def census_data(g, n_seg):
    gen = torch.Generator().manual_seed(5 + g)
    q = torch.zeros(T_ALL, HK, g, D, dtype=BF)
    k = torch.randn(T_ALL, HK, D, generator=gen).to(BF)
    seg = R.seg_table(R.LENS, n_seg)
    k[(seg < 0) | (seg >= n_seg)] = 3.0e38                                  # dropped segments: huge, finite (0 * huge = 0)
    return q, k, seg


@pytest.mark.parametrize("n_seg", [S, 33, 64])
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_key_census_counts_exactly_for_every_row(lib, g, n_seg):
    """Q = 0: rows == count_in_segment / n_visible, the fp32 division, bit for bit, for all 772 rows - one accumulator pass (5, and 33 needs
    the second), both passes full (64) - and again with NaN in every key behind the rows 0, 1, 254 .. 257, 512 of each sequence and in the
    neighbouring sequences: the rows up to there keep their bits."""
    q, k, seg = census_data(g, n_seg)
    want = M.census(seg, R.LENS, n_seg)
    fused, seg_d = R.fused(q, k).cuda(), seg.cuda()
    got, _ = amap(lib, fused, g, seg_d, n_seg=n_seg, fold=False)
    assert torch.equal(bits(got), bits(want[:, None, :].expand(T_ALL, HK * g, n_seg)))
    cu = R.cu_of(R.LENS)
    for b, r, t in R.probe_rows():
        f = fused.clone()
        kv = f.view(T_ALL, HK, g + 2, D)[:, :, g]
        kv[:cu[b]] = float("nan")
        kv[t + 1:] = float("nan")
        cut, _ = amap(lib, f, g, seg_d, n_seg=n_seg, fold=False)
        assert torch.equal(bits(cut[cu[b]:t + 1]), bits(got[cu[b]:t + 1])), (b, r)


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_key_census_with_poison_behind_every_single_row(lib, g):
    """The census once per row, all 772: NaN in every key the row must not read - directly behind it, inside its own key tile, and in the
    other sequences.  The row keeps the exact count."""
    q, k, seg = census_data(g, S)
    want = bits(M.census(seg, R.LENS, S)[:, None, :].expand(T_ALL, HK * g, S))
    fused, seg_d = R.fused(q, k).cuda(), seg.cuda()
    cu = R.cu_of(R.LENS)
    nan_k = torch.full((T_ALL, HK, D), float("nan"), dtype=BF, device="cuda")
    h, ld = HK * g, HK * (g + 2) * D
    rows = torch.empty(T_ALL, h, S, dtype=torch.float32, device="cuda")
    kept = torch.empty(T_ALL, h, S, dtype=torch.float32, device="cuda")
    cos, sin = tables()
    cu_arr = native.i32_array(cu)
    for b in range(len(R.LENS)):
        for t in range(cu[b], cu[b + 1]):
            f = fused.clone()
            kv = f.view(T_ALL, HK, g + 2, D)[:, :, g]
            kv[:cu[b]] = nan_k[:cu[b]]
            kv[t + 1:] = nan_k[t + 1:]
            native.check(lib.aigv_op_attention_map(f.data_ptr(), ld, f.data_ptr() + 2 * g * D, ld, cu_arr, len(R.LENS), h, HK, (g + 2) * D, (g + 2) * D, D, cos.data_ptr(),
                                                   sin.data_ptr(), cos.shape[0], seg_d.data_ptr(), S, rows.data_ptr(), None, native.stream_ptr()))
            kept[t] = rows[t]
    torch.cuda.synchronize()
    assert torch.equal(bits(kept), want)


# ---- 2. one-hot selector ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_one_hot_selector_is_exactly_one_hot(lib, g):
    """The selected key leads by a margin at which exp underflows to 0: exactly 1.0 in its bin (0.0 if its segment is dropped), 0.0 elsewhere.
    Every key the row must not see - behind it, in the other sequences - is the selected key times two and would win if read."""
    for b, r, sel in R.selector_cases():
        c = R.SelectorCase(g, b, r, sel)
        got, _ = amap(lib, R.fused(c.q, c.k).cuda(), g, c.seg.cuda(), fold=False)
        assert torch.equal(bits(got[c.row]), bits(c.expect())), (b, r, sel, got[c.row].tolist())


# ---- 3. random data against float64 -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(g):
    return R.RandomCase(g)


@functools.lru_cache(maxsize=None)
def device_rotated_q(g):
    """The bf16 bits the kernel's rotation must produce: aigv_op_rope on a copy of the fused rows (the g query slots of every group)."""
    c, lib = random_case(g), native.load()
    f = R.fused(c.q, c.k).cuda()
    cos, sin = tables()
    pos_d = c.pos.cuda()
    native.check(lib.aigv_op_rope(f.data_ptr(), f.shape[1], pos_d.data_ptr(), cos.data_ptr(), sin.data_ptr(), c.T, g, g + 2, HK, D, native.stream_ptr()))
    torch.cuda.synchronize()
    return f.cpu().view(c.T, HK, g + 2, D)[:, :, :g].contiguous()


@functools.lru_cache(maxsize=None)
def random_truth(g):
    """(mass, dropped, eps) in float64 for all rows, computed once and shared."""
    c = random_case(g)
    return M.rows_truth(device_rotated_q(g), c.k, c.seg, R.LENS, S)


@functools.lru_cache(maxsize=None)
def random_map(g):
    c = random_case(g)
    return amap(native.load(), R.fused(c.q, c.k).cuda(), g, c.seg.cuda())


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_random_data_against_float64_within_the_derived_bound(lib, g):
    """Truth from the bf16 bits the kernel sees (q rotated by aigv_op_rope itself), all 772 rows; |d mass| <= mass_bound at eps = 2 x
    score_bound (attention_map_reference.rows_bound: a step of the MFMA accumulation is allowed one ulp, not half)."""
    c = random_case(g)
    assert torch.equal(device_rotated_q(g).view(torch.int16), R.rotate_q(c.q, c.pos, c.cos, c.sin).view(torch.int16))
    got, _ = random_map(g)
    mass, dropped, eps = random_truth(g)
    bound = M.rows_bound(mass, eps, R.LENS, S)
    ratio = ((got.double() - mass).abs() / bound).max().item()
    total = ((got.double().sum(-1) + dropped - 1).abs()).max().item()
    print(f"g={g}: worst |mass - fp64| / bound = {ratio:.4f}; worst |sum of bins + dropped - 1| = {total:.3e}")
    assert ratio <= 1.0


# ---- 3b. head_dim 64: the other half of the instantiations -------------------------------------------------------------------------------
D64 = 64


def amap64(lib, q, k, seg, g, n_seg):
    """aigv_op_attention_map at head_dim 64 on the packed 1 / 258 / 513 case, rows inside a sentinel fence: fp32 [T, heads, n_seg]."""
    fused = R.fused(q, k).cuda()
    h, ld = HK * g, HK * (g + 2) * D64
    n = T_ALL * h * n_seg
    whole, ptr = fenced(n)
    cos, sin = (t.cuda() for t in R.rope_table(D64, R.N_POS))
    seg_d = seg.cuda()
    native.check(lib.aigv_op_attention_map(fused.data_ptr(), ld, fused.data_ptr() + 2 * g * D64, ld, native.i32_array(R.cu_of(R.LENS)), len(R.LENS), h, HK, (g + 2) * D64,
                                           (g + 2) * D64, D64, cos.data_ptr(), sin.data_ptr(), cos.shape[0], seg_d.data_ptr(), n_seg, ptr, None, native.stream_ptr()))
    torch.cuda.synchronize()
    return unfenced(whole, n, "rows").view(T_ALL, h, n_seg)


@pytest.mark.parametrize("n_seg", [S, 64])
@pytest.mark.parametrize("g", [1, 3])
def test_op_head_dim_64_census_and_random_data(lib, g, n_seg):
    """attn_map_kernel<64, 1> (5 segments) and <64, 2> (64): the exact key census for all 772 rows (huge finite K rows in the dropped
    segments), and random data against float64 within ``rows_bound`` - the latter is what sees the rotary pairing
    (k-step s with s + 2) and the [pos][32] table index at this width."""
    gen = torch.Generator().manual_seed(640 + 7 * g + n_seg)
    seg = R.seg_table(R.LENS, n_seg)
    k = torch.randn(T_ALL, HK, D64, generator=gen).to(BF)
    kc = k.clone()
    kc[(seg < 0) | (seg >= n_seg)] = 3.0e38
    got = amap64(lib, torch.zeros(T_ALL, HK, g, D64, dtype=BF), kc, seg, g, n_seg)
    assert torch.equal(bits(got), bits(M.census(seg, R.LENS, n_seg)[:, None, :].expand(T_ALL, HK * g, n_seg)))
    q = torch.randn(T_ALL, HK, g, D64, generator=gen).to(BF)
    cos, sin = R.rope_table(D64, R.N_POS)
    q_rot = R.rotate_q(q, R.positions(), cos, sin)
    mass, dropped, eps = M.rows_truth(q_rot, k, seg, R.LENS, n_seg)
    rnd = amap64(lib, q, k, seg, g, n_seg)
    ratio = ((rnd.double() - mass).abs() / M.rows_bound(mass, eps, R.LENS, n_seg)).max().item()
    print(f"D=64 g={g} S={n_seg}: worst |mass - fp64| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    unrot = M.rows_truth(q, k, seg, R.LENS, n_seg)[0]                      # (the bound does tell a rotated query from an unrotated one)
    assert ((unrot - mass).abs() / M.rows_bound(mass, eps, R.LENS, n_seg)).max().item() > 1.0


# ---- 4. a sequence alone is the sequence packed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_sequence_alone_is_sequence_packed(lib, g):
    c = random_case(g)
    base, base_fold = random_map(g)
    fused = R.fused(c.q, c.k).cuda()
    for b, n in enumerate(R.LENS):
        alone, alone_fold = amap(lib, fused[c.cu[b]:c.cu[b + 1]].contiguous(), g, c.seg[c.cu[b]:c.cu[b + 1]].cuda(), lens=[n])
        assert torch.equal(alone, base[c.cu[b]:c.cu[b + 1]]), b
        assert torch.equal(bits(alone_fold[0]), bits(base_fold[b])), b
    # ... and in another order: the longest sequence first, at packed row 0
    order = [2, 0, 1]
    rows_of = torch.cat([torch.arange(c.cu[b], c.cu[b + 1]) for b in order])
    moved, _ = amap(lib, fused[rows_of.cuda()].contiguous(), g, c.seg[rows_of].cuda(), lens=[R.LENS[b] for b in order], fold=False)
    assert torch.equal(moved, base[rows_of])


# ---- 5. the score-row probe on the same buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_rows_against_the_score_row_probe(lib, g):
    """aigv_op_attention_probe on the same fused rows and table, at probe_rows(): the two kernels sum in different orders, so they agree
    within the sum of their bounds - the probe's (eps = score_bound: explicit fmaf) and the map's (2 x score_bound)."""
    c = random_case(g)
    got, _ = random_map(g)
    fused, seg_d = R.fused(c.q, c.k).cuda(), c.seg.cuda()
    rows = [t for _, _, t in R.probe_rows()]
    h, ld = HK * g, HK * (g + 2) * D
    out = torch.empty(len(rows), h, S, dtype=torch.float32, device="cuda")
    cos, sin = tables()
    native.check(lib.aigv_op_attention_probe(fused.data_ptr(), ld, fused.data_ptr() + 2 * g * D, ld, native.i32_array(c.cu), len(R.LENS), h, HK, (g + 2) * D, (g + 2) * D, 0,
                                             None, D, cos.data_ptr(), sin.data_ptr(), cos.shape[0], native.i32_array(rows), len(rows), seg_d.data_ptr(), None, 0, S,
                                             out.data_ptr(), native.stream_ptr()))
    torch.cuda.synchronize()
    mass, _, eps = random_truth(g)
    n_keys = M.key_counts(R.LENS)
    worst = 0.0
    for i, t in enumerate(rows):
        tol = R.mass_bound(mass[t], eps[t], int(n_keys[t]), S) + R.mass_bound(mass[t], 2 * eps[t], int(n_keys[t]), S)
        worst = max(worst, ((got[t].double() - out[i].cpu().double()).abs() / tol).max().item())
    print(f"g={g}: worst |map - probe| / (sum of the two bounds) = {worst:.4f}")
    assert worst <= 1.0


# ---- 6. the fold ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_fold_is_the_documented_chain(lib, g):
    """seg_out against the host's fp32 chain over the DEVICE's own rows (bit for bit, NaN where a segment has no row in the sequence - the
    one-token sequence, whose id lies outside the bins, leaves all five empty, the third sequence four) and against the float64 mean of those rows, within n 2^-24 RELATIVE, n the rows of the segment: the chain rounds n times -
    n - 1 additions (0 + x is exact), each half an ulp of a running sum that never exceeds the final one (the rows are non-negative), and one division."""
    c = random_case(g)
    rows, fold = random_map(g)
    chain = M.fold_chain(rows, c.seg, R.LENS, S)
    assert torch.equal(bits(fold), bits(chain))
    counts = M.segment_rows(c.seg, R.LENS, S)
    assert (counts[0] > 0).sum() == 0 and (counts[1] > 0).all() and (counts[2] > 0).sum() == 1      # (the one-token sequence's id is -1; sequence 2 holds one id)
    empty = (counts == 0)[:, None, :, None].expand_as(fold)
    assert torch.isnan(fold[empty]).all() and torch.isfinite(fold[~empty]).all()
    truth = M.fold_truth(rows, c.seg, R.LENS, S)
    tol = counts.double()[:, None, :, None] * 2.0 ** -24 * truth
    err = (fold.double() - truth).abs()
    print(f"g={g}: worst fold |d| / bound = {(err[~empty] / tol[~empty].clamp_min(1e-300)).max().item():.4f}")
    assert (err[~empty] <= tol[~empty]).all()
    # the fold of the exact census rows: every row of a segment holds exact small-integer ratios; n_seg = 64 exercises the 16-block grid
    q, k, seg = census_data(g, 64)
    rows64, fold64 = amap(lib, R.fused(q, k).cuda(), g, seg.cuda(), n_seg=64)
    assert torch.equal(bits(fold64), bits(M.fold_chain(rows64, seg, R.LENS, 64)))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_op_refusals_leave_every_buffer_untouched(lib):
    g = 3
    c = random_case(g)
    fused, seg_d = R.fused(c.q, c.k).cuda(), c.seg.cuda()
    ld = HK * (g + 2) * D
    for over, word in ((dict(n_seg=0), "segments"), (dict(n_seg=65), "segments"), (dict(d=96), "head_dim"), (dict(k=fused.data_ptr() + 2 * g * D + 2), "16-byte aligned"),
                       (dict(q=fused.data_ptr() + 2), "16-byte aligned"), (dict(ldk=ld + 4), "multiples of 8"), (dict(ldq=D), "q strides too small"),
                       (dict(khs=D - 8), "K strides too small"), (dict(cu=native.i32_array([0, 1, 1, 772])), "empty sequence"),
                       (dict(cu=native.i32_array([1, 2, 259, 772])), "cu[0]"), (dict(max_pos=512), "longer than the RoPE table"), (dict(n_kv=4), "multiple of n_kv_heads"),
                       (dict(seg=None), "null operand"), (dict(cos=None), "null operand"), (dict(n_seq=0), "sequences"), (dict(n_seq=128), "sequences")):
        assert amap(lib, fused, g, seg_d, refused=word, **over) is None
    h = HK * g
    rc = lib.aigv_op_attention_map(fused.data_ptr(), ld, fused.data_ptr() + 2 * g * D, ld, native.i32_array(c.cu), 3, h, HK, (g + 2) * D, (g + 2) * D, D, tables()[0].data_ptr(),
                                   tables()[1].data_ptr(), R.N_POS, seg_d.data_ptr(), S, None, None, native.stream_ptr())
    assert rc == -1 and "null operand" in lib.aigv_last_error(None).decode()
    got, _ = amap(lib, fused, g, seg_d)                                    # and the next good call is the good call
    assert torch.equal(got, random_map(g)[0])


# =================================================================================================================================
# model level: the tiny rig of tests/test_gpu_score_attention.py (two clips of 2 and 1 frames, two LLM layers)
# =================================================================================================================================
from test_gpu_score_attention import clip_alone, rig      # noqa: E402  (the rig is cached: both files share one model per stage)

OPTS = dict(return_score_attention=True, return_logprobs=True, top_logprobs=3)       # what rig()'s own pass carried


def same_bits(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a.detach().cpu().reshape(-1).view(torch.uint8), b.detach().cpu().reshape(-1).view(torch.uint8))


@functools.lru_cache(maxsize=None)
def mapped(stage):
    """The rig's pass once more with the map armed over every layer, default table (shared by the tests below)."""
    model, cfg, sd, kw, on = rig(stage)
    L = cfg.llm_config.num_hidden_layers
    out = model(**kw, **OPTS, return_segment_attention=True, return_row_attention=(0, L))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("stage", [2, 1])
def test_model_armed_pass_changes_no_other_bit(stage):
    model, cfg, sd, kw, on = rig(stage)
    llm = cfg.llm_config
    L, nh, B, N = llm.num_hidden_layers, llm.num_attention_heads, 2, kw["input_ids"].shape[1]
    out = mapped(stage)
    assert set(out) == set(on) | {"segment_attention", "segment_rows", "row_attention"}
    for key, v in on.items():
        assert (v is None and out[key] is None) or same_bits(out[key], v), key
    Sg = 2 + prompts.N_TEXT_SEGMENTS
    seg_att, seg_rows, rows = out["segment_attention"].cpu(), out["segment_rows"].cpu(), out["row_attention"].cpu()
    assert seg_att.dtype == rows.dtype == torch.float32 and seg_rows.dtype == torch.long
    assert tuple(seg_att.shape) == (B, L, nh, Sg, Sg) and tuple(seg_rows.shape) == (B, Sg) and tuple(rows.shape) == (B, L, nh, N, Sg)
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    assert seg_rows.sum(1).tolist() == plan["lens"] and seg_rows[1, 1] == 0 and (seg_rows[0, :2] > 0).all()      # clip 1 has one frame: its frame bin 1 is empty
    empty = (seg_rows == 0)[:, None, None, :, None].expand_as(seg_att)
    assert torch.isnan(seg_att[empty]).all() and torch.isfinite(seg_att[~empty]).all() and (seg_att[~empty] >= 0).all()
    sums = seg_att.double().sum(-1)[~empty[..., 0]]
    assert (sums - 1).abs().max().item() <= (Sg + 2) * 2.0 ** -23                    # nothing dropped by the default table: every row of the matrix sums to 1
    for b in range(B):
        n = plan["lens"][b]
        assert torch.isnan(rows[b, :, :, n:]).all() and torch.isfinite(rows[b, :, :, :n]).all()
        assert (rows[b, :, :, :n].double().sum(-1) - 1).abs().max().item() <= 4 * 2.0 ** -23
        assert (rows[b, :, :, 0] == torch.nn.functional.one_hot(torch.tensor(Sg - 3), Sg).float()).all()       # the first token reads itself: bin "first token"
    # the fold is the documented chain over the rows the same pass returned
    seg, _ = model._default_segments(plan)
    packed = torch.cat([rows[b, :, :, :plan["lens"][b]] for b in range(B)], 2).permute(0, 2, 1, 3).contiguous()      # [L, T, nh, S]
    for l in range(L):
        assert torch.equal(bits(seg_att[:, l]), bits(M.fold_chain(packed[l], seg, plan["lens"], Sg))), l
    # the context disarmed itself
    again = model(**kw, **OPTS)
    assert set(again) == set(on) and all(v is None or same_bits(again[k], v) for k, v in on.items())


def layer_scores_bound(model, cfg, sd, kw, plan, rows_of):
    """[L][clip] score_bound (float64 [n_heads]) of the packed rows ``rows_of`` in every layer: q and k restated in float64 from the residual
    stream the pass itself consumed (``return_stream`` of every token at every depth) through RMSNorm, wqkv and RoPE.  The restated operands
    differ from the kernel's bf16 ones by 2^-8 relative each at most, so sum |q||k| is inflated by (1 + 2^-8)^2 < 1.01."""
    llm = cfg.llm_config
    H, nh, nkv, L = llm.hidden_size, llm.num_attention_heads, llm.num_key_value_heads, llm.num_hidden_layers
    d, g = H // nh, nh // nkv
    cap = model(**kw, return_stream=kw["attention_mask"])
    stream, index = cap["stream"].cpu().double(), cap["stream_index"].cpu()
    assert stream.shape[0] == plan["cu"][-1] and index[:, 0].tolist() == sorted(index[:, 0].tolist())      # every packed row, clip-major
    from aigv_assessor_amd.modeling import rope_tables
    cos, sin = rope_tables(d, llm.rope_theta, max(plan["lens"]), llm.max_position_embeddings, getattr(llm, "rope_scaling", None))
    cos, sin = torch.cat([cos, cos], -1).double(), torch.cat([sin, sin], -1).double()

    def rot(v, pos):
        r = torch.cat((-v[..., d // 2:], v[..., : d // 2]), -1)
        shape = (len(pos),) + (1,) * (v.dim() - 2) + (d,)
        return v * cos[pos].view(shape) + r * sin[pos].view(shape)

    out = []
    for l in range(L):
        x = stream[:, l]
        xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + llm.rms_norm_eps) * sd[f"language_model.model.layers.{l}.attention_norm.weight"].double()
        qkv = (xn @ sd[f"language_model.model.layers.{l}.attention.wqkv.weight"].double().T).view(-1, nkv, g + 2, d)
        per = []
        for b, t in enumerate(rows_of):
            lo = plan["cu"][b]
            pos = torch.arange(t - lo + 1)
            q = rot(qkv[t:t + 1, :, :g], pos[-1:])[0].reshape(nh, d)
            k = rot(qkv[lo:t + 1, :, g], pos)
            per.append(1.01 * R.score_bound(q, k))
        out.append(per)
    return out


@pytest.mark.parametrize("stage", [2, 1])
def test_model_row_attention_at_the_score_row_is_score_attention(stage):
    """Two kernels, the same Q and K bits, different summation orders: they agree within the SUM of their bounds - the probe's mass_bound at
    eps = score_bound (explicit fmaf) and the map's at 2 x score_bound - taken at the reported mass, in every layer."""
    model, cfg, sd, kw, on = rig(stage)
    out = mapped(stage)
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    probe_rows = model._probe_rows(plan)
    eps = layer_scores_bound(model, cfg, sd, kw, plan, probe_rows)
    att, rows = on["score_attention"].cpu().double(), out["row_attention"].cpu().double()
    Sg, worst = att.shape[-1], 0.0
    for b, t in enumerate(probe_rows):
        p = t - plan["cu"][b]
        for l in range(att.shape[1]):
            mass = att[b, l]
            tol = R.mass_bound(mass, eps[l][b], p + 1, Sg) + R.mass_bound(mass, 2 * eps[l][b], p + 1, Sg)
            worst = max(worst, ((rows[b, l, :, p] - mass).abs() / tol).max().item())
    print(f"stage {stage}: worst |row_attention - score_attention| / (sum of the two bounds) = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("stage", [2, 1])
def test_model_clip_alone_is_clip_in_batch(stage):
    """With one table for both calls (flow_segments of the batch - S = F + 5 = 7; stage 1 has no score row and stops at F + 4 - sliced per clip) a clip alone gives the bits it gives in the
    batch: the matrix, the counts and every row."""
    model, cfg, sd, kw, on = rig(stage)
    L = cfg.llm_config.num_hidden_layers
    table = eval_utils.flow_segments(model, kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    both = model(**kw, attention_segments=table, return_segment_attention=True, return_row_attention=(0, L))
    assert both["segment_attention"].shape[-1] == 2 + prompts.N_TEXT_SEGMENTS + (stage == 2)
    assert stage == 1 or both["segment_rows"][:, -1].tolist() == [1, 1]             # the score row is a bin of its own, one row per clip
    for b in range(2):
        one = clip_alone(kw, b)
        n = one["input_ids"].shape[1]
        alone = model(**one, attention_segments=table[b:b + 1, :n], return_segment_attention=True, return_row_attention=(0, L))
        assert same_bits(alone["segment_attention"][0], both["segment_attention"][b]), b
        assert same_bits(alone["segment_rows"][0], both["segment_rows"][b]), b
        assert same_bits(alone["row_attention"][0], both["row_attention"][b, :, :, :n]), b


def test_model_last_layer_under_row_trimming_is_filled_for_every_row():
    """The row-trimmed last layer finishes only the consumed rows, but Q and K exist for all of them: the window (L - 1, L) alone is filled
    for every token, with the bits of the pass that trims nothing (which also runs the dead tail behind the last consumed row: one more
    column) - and an empty window arms nothing."""
    model, cfg, sd, kw, on = rig(2)
    L = cfg.llm_config.num_hidden_layers
    full = mapped(2)["row_attention"]
    last = model(**kw, return_row_attention=(L - 1, L))
    assert set(last) - set(model(**kw)) == {"row_attention"} and same_bits(last["row_attention"], full[:, L - 1:])
    lens = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)["lens"]
    for b in range(2):
        assert torch.isfinite(last["row_attention"][b, 0, :, :lens[b]]).all()
    try:
        model.set_row_trimming(False)
        untrimmed = model(**kw, return_row_attention=(L - 1, L))
    finally:
        model.set_row_trimming(True)
    for b in range(2):
        assert same_bits(untrimmed["row_attention"][b, :, :, :lens[b]], last["row_attention"][b, :, :, :lens[b]]), b
    empty = model(**kw, return_row_attention=(1, 1))
    assert tuple(empty["row_attention"].shape) == (2, 0) + tuple(full.shape[2:])


def test_model_graph_replay_runs_the_armed_call_eagerly():
    model, cfg, sd, kw, on = rig(2)
    L = cfg.llm_config.num_hidden_layers
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    opts = dict(return_segment_attention=True, return_row_attention=(0, L), return_score_attention=True)
    eager = model(**dev_kw, **opts)
    torch.cuda.synchronize()
    model.enable_graph_replay(True)
    try:
        before = dict(model._graphs)
        for _ in range(3):
            got = model(**dev_kw, **opts)
            for key in ("segment_attention", "segment_rows", "row_attention", "score_attention", "score1"):
                assert same_bits(got[key], eager[key]), key
        assert dict(model._graphs) == before, "a call with the attention map captured a graph"
        plain = [model(**dev_kw)["score1"].clone() for _ in range(3)]                   # unarmed calls still capture and replay
        assert any(isinstance(v, tuple) for v in model._graphs.values()) and all(same_bits(p, eager["score1"]) for p in plain)
    finally:
        model.enable_graph_replay(False)


def test_model_refusals_come_with_a_message_and_write_nothing(lib):
    model, cfg, sd, kw, on = rig(2)
    llm = cfg.llm_config
    L, nh = llm.num_hidden_layers, llm.num_attention_heads
    drop = torch.zeros_like(kw["input_ids"], dtype=torch.bool)
    drop[:, 20] = True
    for opts, word in ((dict(return_segment_attention=True, key_drop=drop), "does not know the mask"), (dict(return_row_attention=(0, L + 1)), "outside 0 <= lo <= hi"),
                       (dict(return_row_attention=(1, 0)), "outside 0 <= lo <= hi"), (dict(return_segment_attention=True, attention_segments=torch.full_like(kw["input_ids"], 64)), "65 segments")):
        with pytest.raises(ValueError, match=word):
            model(**kw, **opts)
    # the C ABI's own refusals: armed by hand in front of the pass
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    T, S3 = plan["cu"][-1], 3
    seg = torch.zeros(T, dtype=torch.int32, device="cuda")
    bufs = [torch.zeros(n, dtype=torch.float32, device="cuda") for n in (T * nh * 65, 2 * L * nh * 65 * 65, (L + 1) * T * nh * 65)]
    scratch, fold, rows = bufs
    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)

    def armed_prefill(n_seg=S3, scratch=scratch, fold=fold, rows=None, lo=0, hi=0, **prefill):
        # (the context is sized for the pass FIRST: a larger KV capacity rebuilds it, and the map is armed on the context the pass runs on)
        _, ctx = model._native(n_tokens=T, n_clips=2, out_rows=len(plan["logit_rows"]), kv_cap=prefill.get("kv_cap", 0))
        native.check(lib.aigv_attention_map_arm(ctx, seg.data_ptr(), n_seg, native.ptr(scratch), native.ptr(fold), native.ptr(rows), lo, hi), ctx)
        return model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"], **prefill)

    words = torch.zeros(2, (max(plan["lens"]) + 63) // 64, dtype=torch.int64)
    for how, word in ((dict(n_seg=65), "65 segments"), (dict(n_seg=0), "0 segments"), (dict(rows=rows, lo=0, hi=L + 1), "outside 0 <= lo <= hi"), (dict(rows=rows, lo=2, hi=1), "outside 0 <= lo <= hi"),
                      (dict(lo=0, hi=1), "rows_out NULL"), (dict(scratch=None), "scratch"), (dict(keep_kv=True, kv_cap=max(plan["lens"]) + 8), "keep_kv"),
                      (dict(drop_words=words), "does not know the mask")):
        with pytest.raises(native.NativeError, match=word):
            armed_prefill(**how)
        torch.cuda.synchronize()
        assert "segment_attention" not in model(**kw)                                # the refused pass disarmed: a plain pass runs
    ctx = model._ctx
    assert lib.aigv_attention_map_arm(ctx, seg.data_ptr(), S3, scratch.data_ptr(), None, None, 0, 0) == -1       # nothing to report: refused when arming
    assert lib.aigv_attention_map_arm(ctx, None, S3, scratch.data_ptr(), fold.data_ptr(), None, 0, 0) == -1
    # aigv_llm_extend refuses an armed map before it looks at anything else
    native.check(lib.aigv_attention_map_arm(ctx, seg.data_ptr(), S3, scratch.data_ptr(), fold.data_ptr(), None, 0, 0), ctx)
    ids = torch.zeros(1, dtype=torch.long, device="cuda")
    assert lib.aigv_llm_extend(ctx, ids.data_ptr(), native.i32_array([0, 1]), 1, None, None, None, 0, None, 0, native.stream_ptr()) != 0
    assert "attention map is armed" in lib.aigv_last_error(ctx).decode()
    torch.cuda.synchronize()
    assert all(float(b.abs().sum()) == 0.0 for b in bufs)                            # no refused pass wrote to any of the caller's buffers
    ok = model(**kw, **OPTS, return_segment_attention=True, return_row_attention=(0, L))
    assert same_bits(ok["segment_attention"], mapped(2)["segment_attention"]) and same_bits(ok["row_attention"], mapped(2)["row_attention"])
