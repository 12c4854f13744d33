"""Score-row attention per token on the MI355X: the dense form of the probe kernel through aigv_op_attention_probe_tokens (no model) on the
constructions of tests/score_attention_reference.py - census and one-hot selector bit-exact PER KEY, random data against float64 within the
derived per-key bound, dense against bins (bit-identical where a bin holds one key), bins unchanged, a row's bits its own, host-side
refusals - every call inside a sentinel fence around both outputs; then ``forward(return_token_attention=True)`` and
``forward_shared_prefix`` through the model, the frame heat maps against frame_saliency, and graph replay.
tests/test_score_attention_tokens_cpu.py holds, without a GPU, what these expectations rest on."""
import ctypes
import functools
import math

import pytest
import torch

import score_attention_reference as R
import score_attention_tokens_reference as TR
import test_gpu_score_attention as G          # the tiny model rig of the score-attention tests (cached: one model for both files)
from aigv_assessor_amd import eval_utils, native, prompts, synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D, S, HK = R.D, R.S, R.N_KV
SENTINEL, PAD = G.SENTINEL, G.PAD
bits = G.bits
ROWS = [t for _, _, t in R.probe_rows()]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


@functools.lru_cache(maxsize=None)
def tables(d=D):
    cos, sin = R.rope_table(d, R.N_POS)
    return cos.cuda(), sin.cuda()


def need_of(rows, lens, kv_off=None):
    """The largest position + 1 over the probe rows: the least ld_tok the call takes."""
    cu = R.cu_of(lens)
    need = 0
    for t in rows:
        b = max(i for i in range(len(lens)) if cu[i] <= t)
        need = max(need, (kv_off[b] if kv_off else 0) + t - cu[b] + 1)
    return need


def probe_tokens(lib, fused_d, g, rows, seg_new_d, lens=R.LENS, cache=None, n_seg=S, extra=0, d=D, ld_tok=None, null_tok=False, refused=None):
    """aigv_op_attention_probe_tokens on fused rows [T, HK (g + 2) d]; cache = (kc, cap, kv_off list, seg_cached_d, ld_cached) for the cache
    form.  `out` and `tok_out` each sit between two sentinel pads inside an allocation that starts as the sentinel.  Returns (out [rows,
    heads, n_seg], tok [rows, heads, ld_tok]) after checking that all four pads kept their bits and that every element of both was written.
    refused = a word of the expected message: the call must return AIGV_ERR_ARG and leave BOTH allocations untouched."""
    h, ld = HK * g, HK * (g + 2) * d
    kv_off = cache[2] if cache is not None else None
    if ld_tok is None:
        ld_tok = need_of(rows, lens, kv_off) + extra
    n, nt = min(len(rows), 64) * h * n_seg, min(len(rows), 64) * h * max(ld_tok, 1)
    whole = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    whole_t = torch.full((PAD + nt + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    out_ptr, tok_ptr = whole.data_ptr() + 4 * PAD, whole_t.data_ptr() + 4 * PAD
    cos, sin = tables(d)
    cu = native.i32_array(R.cu_of(lens))
    if cache is None:
        k_ptr, ldk, hs, ss, off, segc, ldc = fused_d.data_ptr() + 2 * g * d, ld, (g + 2) * d, 0, None, None, 0
    else:
        kc, cap, _, segc_d, ldc = cache
        k_ptr, ldk, hs, ss, off, segc = kc.data_ptr(), d, cap * d, HK * cap * d, native.i32_array(kv_off), segc_d.data_ptr()
    rc = lib.aigv_op_attention_probe_tokens(fused_d.data_ptr(), ld, k_ptr, ldk, cu, len(lens), h, HK, (g + 2) * d, hs, ss, off, d, cos.data_ptr(), sin.data_ptr(),
                                            cos.shape[0], native.i32_array(rows), len(rows), seg_new_d.data_ptr(), segc, ldc, n_seg, ctypes.c_void_p(out_ptr),
                                            None if null_tok else ctypes.c_void_p(tok_ptr), ld_tok, native.stream_ptr())
    torch.cuda.synchronize()
    w, wt = whole.cpu(), whole_t.cpu()
    if refused is not None:
        msg = lib.aigv_last_error(None).decode()
        assert rc == -1 and refused in msg and "aigv_op_attention_probe_tokens" in msg, (rc, msg)
        assert (w == SENTINEL).all() and (wt == SENTINEL).all(), "a refused call wrote something"
        return None, None
    assert rc == 0, lib.aigv_last_error(None).decode()
    assert (w[:PAD] == SENTINEL).all() and (w[PAD + n:] == SENTINEL).all(), "the probe wrote outside its bin output"
    assert (wt[:PAD] == SENTINEL).all() and (wt[PAD + nt:] == SENTINEL).all(), "the probe wrote outside its dense output"
    assert (w[PAD:PAD + n] != SENTINEL).all(), "the probe left part of its bin output unwritten"
    assert (wt[PAD:PAD + nt] != SENTINEL).all(), "the probe left part of its ld_tok columns unwritten"
    return (w[PAD:PAD + n].view(torch.float32).view(len(rows), h, n_seg).clone(),
            wt[PAD:PAD + nt].view(torch.float32).view(len(rows), h, ld_tok).clone())


def cache_form(lib, fused, seg, g, extra=0, d=D, n_seg=S):
    """The op-level case in CACHE form (test_gpu_score_attention.cache_form_probe, with the dense output): K of every token stored at its
    position by aigv_op_kv_store, the rest of the cache NaN; the pass = the rows behind CACHE_OFF[b].  Returns ([(index into probe_rows(), packed
    row of the shortened pass)], out, tok): a pick's dense row is indexed by CACHE position, so it must equal the packed form's."""
    cu, off, cap, T = R.cu_of(R.LENS), R.CACHE_OFF, R.CACHE_CAP, sum(R.LENS)
    kc = torch.full((len(R.LENS), HK, cap, d), float("nan"), dtype=BF, device="cuda")
    vc = torch.zeros_like(kc)
    seq = torch.repeat_interleave(torch.arange(len(R.LENS)), torch.tensor(R.LENS)).to(torch.int32).cuda()
    pos_d = R.positions().cuda()
    native.check(lib.aigv_op_kv_store(fused.data_ptr(), fused.shape[1], seq.data_ptr(), pos_d.data_ptr(), kc.data_ptr(), vc.data_ptr(), T, HK, g, d, cap,
                                      native.stream_ptr()))
    new_lens = [n - o for n, o in zip(R.LENS, off)]
    keep = torch.cat([torch.arange(cu[b] + off[b], cu[b + 1]) for b in range(len(R.LENS))])
    cu_new = R.cu_of(new_lens)
    ldc = max(off) + 3
    segc = torch.full((len(R.LENS), ldc), -1, dtype=torch.int32)
    for b in range(len(R.LENS)):
        segc[b, :off[b]] = seg[cu[b]:cu[b] + off[b]]
    picks = [(i, cu_new[b] + r - off[b]) for i, (b, r, t) in enumerate(R.probe_rows()) if r >= off[b]]
    assert {R.probe_rows()[i][0] for i, _ in picks} == {0, 1, 2} and len(picks) >= 10
    out, tok = probe_tokens(lib, fused[keep.cuda()].contiguous(), g, [t for _, t in picks], seg[keep].cuda(), lens=new_lens,
                            cache=(kc, cap, off, segc.cuda(), ldc), n_seg=n_seg, extra=extra, d=d)
    return picks, out, tok


def extra_of(g):
    return TR.EXTRA_LD if g == 3 else 0          # the cases that are not parametrised over ld_tok take turns


# ---- 1. census ----------------------------------------------------------------------------------------------------------------------
def census_check(lib, g, extra, d=D):
    gen = torch.Generator().manual_seed(5 + g)
    T, cu = sum(R.LENS), R.cu_of(R.LENS)
    q = torch.zeros(T, HK, g, d, dtype=BF)
    k = torch.randn(T, HK, d, generator=gen).to(BF)
    seg = R.seg_table()
    seg_d = seg.cuda()
    out, tok = probe_tokens(lib, R.fused(q, k).cuda(), g, ROWS, seg_d, extra=extra, d=d)
    ld = tok.shape[-1]
    assert ld == max(R.LENS) + extra
    for i, (b, r, t) in enumerate(R.probe_rows()):
        want = TR.census_dense(r + 1, ld)
        assert torch.equal(bits(tok[i]), bits(want.expand(HK * g, ld))), (b, r, tok[i, 0, :r + 2].tolist(), want[0].item())
    picks, _, cached = cache_form(lib, R.fused(q, k).cuda(), seg, g, extra=extra, d=d)
    for j, (i, _) in enumerate(picks):
        assert torch.equal(bits(cached[j]), bits(tok[i])), ("cache form", R.probe_rows()[i])
    # every row alone, NaN in every key it must not read: behind it, and the other sequences'
    for i, (b, r, t) in enumerate(R.probe_rows()):
        kp = k.clone()
        kp[:cu[b]] = float("nan")
        kp[t + 1:] = float("nan")
        _, one = probe_tokens(lib, R.fused(q, kp).cuda(), g, [t], seg_d, extra=extra if i % 2 else TR.EXTRA_LD - extra, d=d)
        assert torch.equal(bits(one[0]), bits(TR.census_dense(r + 1, one.shape[-1]).expand(HK * g, one.shape[-1]))), (b, r)


@pytest.mark.parametrize("extra", [0, TR.EXTRA_LD])
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_census_every_visible_key_holds_one_over_n_and_the_rest_plus_zero(lib, g, extra):
    """Q = 0: tok[j] is the fp32 division 1 / n bit for bit for j <= pos and +0.0 for pos < j < ld_tok, packed and cache form, at ld_tok =
    the need and 40 more; the pads keep the sentinel (probe_tokens); NaN in every key a row must not read changes nothing."""
    census_check(lib, g, extra)


# ---- 2. one-hot selector ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, TR.EXTRA_LD])
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_one_hot_selector_is_exactly_one_hot_per_key(lib, g, extra):
    """The selected key holds exactly 1.0, every other visible key exactly +0.0 (and the columns behind the row +0.0) - packed form, and cache
    form wherever the row lies behind its sequence's CACHE_OFF (there the keys the row must never read sit in the cache behind it)."""
    n_cache = 0
    for b, r, sel in R.selector_cases():
        c = R.SelectorCase(g, b, r, sel)
        fused = R.fused(c.q, c.k).cuda()
        out, tok = probe_tokens(lib, fused, g, [c.row], c.seg.cuda(), extra=extra)
        want = torch.zeros(HK * g, tok.shape[-1])
        want[:, sel] = 1.0
        assert torch.equal(bits(tok[0]), bits(want)), (b, r, sel, tok[0, 0].nonzero().flatten().tolist())
        assert torch.equal(bits(out[0]), bits(c.expect()))
        if r >= R.CACHE_OFF[b]:
            picks, outc, tokc = cache_form(lib, fused, c.seg, g, extra=extra)
            j = [j for j, (i, _) in enumerate(picks) if R.probe_rows()[i][2] == c.row][0]
            wantc = torch.zeros(HK * g, tokc.shape[-1])
            wantc[:, sel] = 1.0
            assert torch.equal(bits(tokc[j]), bits(wantc)), ("cache form", b, r, sel, tokc[j, 0].nonzero().flatten().tolist())
            assert torch.equal(bits(outc[j]), bits(c.expect()))
            n_cache += 1
    assert n_cache >= 9                                                  # (0, 0) and the four selections of each long row


# ---- 3. random data against float64 -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(g):
    return R.RandomCase(g)


@functools.lru_cache(maxsize=None)
def random_run(g):
    """(bins, dense rows) of the random case in packed form, all probe rows in one launch: computed once, shared, never modified."""
    c = random_case(g)
    return probe_tokens(native.load(), R.fused(c.q, c.k).cuda(), g, ROWS, c.seg.cuda(), extra=extra_of(g))


def float64_check(tok, q_rot, k, lens, rows3, g, d):
    worst = worst_sum = 0.0
    cu = R.cu_of(lens)
    for i, (b, r, t) in enumerate(rows3):
        keys = k[cu[b]:cu[b] + r + 1]
        qr = q_rot[t].reshape(HK * g, d)
        p = TR.row_truth(qr, keys)
        bound = TR.key_bound(p, R.score_bound(qr, keys), r + 1)
        worst = max(worst, ((tok[i, :, :r + 1].double() - p).abs() / bound).max().item())
        worst_sum = max(worst_sum, (tok[i].double().sum(-1) - 1).abs().max().item() / TR.row_sum_bound(r + 1))
        assert (tok[i, :, r + 1:].view(torch.int32) == 0).all()
    return worst, worst_sum


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_random_data_per_key_against_float64_within_the_derived_bound(lib, g):
    """|p - p64| <= p64 (e^(2 eps) (1 + gamma_c) - 1) + 2^-126 per key (score_attention_tokens_reference.key_bound: derived, not chosen), and
    every row sums to 1 within (n + 2) 2^-24 in float64."""
    c = random_case(g)
    _, tok = random_run(g)
    worst, worst_sum = float64_check(tok, R.rotate_q(c.q, c.pos, c.cos, c.sin), c.k, R.LENS, R.probe_rows(), g, D)
    print(f"g={g}: worst |p - fp64| / bound = {worst:.4f}; worst |row sum - 1| / bound = {worst_sum:.4f}")
    assert worst <= 1.0 and worst_sum <= 1.0


def test_op_head_dim_64_census_and_random_data(lib):
    """The D = 64 instantiation: the census bit-exact, random data within the same derived bound."""
    g, d = 2, 64
    census_check(lib, g, TR.EXTRA_LD, d=d)
    gen = torch.Generator().manual_seed(6400)
    T = sum(R.LENS)
    q = torch.randn(T, HK, g, d, generator=gen).to(BF)
    k = torch.randn(T, HK, d, generator=gen).to(BF)
    cos, sin = R.rope_table(d, R.N_POS)
    out, tok = probe_tokens(lib, R.fused(q, k).cuda(), g, ROWS, R.seg_table().cuda(), d=d)
    worst, worst_sum = float64_check(tok, R.rotate_q(q, R.positions(), cos, sin), k, R.LENS, R.probe_rows(), g, d)
    print(f"D=64: worst |p - fp64| / bound = {worst:.4f}; worst |row sum - 1| / bound = {worst_sum:.4f}")
    assert worst <= 1.0 and worst_sum <= 1.0


# ---- 4. dense == bins where they must be --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_a_bin_of_one_key_is_that_keys_dense_value_bit_for_bit(lib, g):
    """63 chosen keys of every sequence get a bin each, the rest is dropped: out[..., s] and tok[..., key_s] of the SAME call hold the same bits
    (a key the row cannot see: +0.0 in both)."""
    c = random_case(g)
    seg, keys = TR.one_key_bins()
    out, tok = probe_tokens(lib, R.fused(c.q, c.k).cuda(), g, ROWS, seg.cuda(), n_seg=63, extra=extra_of(g))
    seen = 0
    for i, (b, r, t) in enumerate(R.probe_rows()):
        ks = keys[b]
        assert torch.equal(bits(out[i][:, :len(ks)]), bits(tok[i][:, ks])), (b, r)
        assert (out[i][:, len(ks):].view(torch.int32) == 0).all()
        seen += sum(1 for j in ks if j <= r)
    assert seen > 200 and (out > 0).sum() >= seen                        # (the comparison was not one of zeros)


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_dense_values_of_a_bin_sum_to_the_bin(lib, g):
    """Default-style table: the float64 sum of the dense values of a bin's keys lies within (ceil(n / 256) + 11) 2^-24 bin of the bin."""
    c = random_case(g)
    out, tok = random_run(g)
    worst = 0.0
    for i, (b, r, t) in enumerate(R.probe_rows()):
        seg = c.seg[c.cu[b]:c.cu[b] + r + 1]
        for s in range(S):
            dense = tok[i][:, :r + 1][:, seg == s].double().sum(-1)
            bound = TR.bin_bound(out[i][:, s].double(), r + 1)
            if (bound > 0).any():
                worst = max(worst, ((dense - out[i][:, s].double()).abs()[bound > 0] / bound[bound > 0]).max().item())
            assert (dense[bound == 0] == 0).all()
    print(f"g={g}: worst |sum of dense - bin| / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- 5. bins unchanged ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_bins_of_the_tokens_call_are_the_plain_calls(lib, g):
    c = random_case(g)
    out, _ = random_run(g)
    plain = G.probe(lib, R.fused(c.q, c.k).cuda(), g, ROWS, c.seg.cuda())
    assert torch.equal(bits(out), bits(plain))
    seg, _ = TR.one_key_bins()
    out63, _ = probe_tokens(lib, R.fused(c.q, c.k).cuda(), g, ROWS, seg.cuda(), n_seg=63)
    assert torch.equal(bits(out63), bits(G.probe(lib, R.fused(c.q, c.k).cuda(), g, ROWS, seg.cuda(), n_seg=63)))


# ---- 6. a row's bits are its own ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_cache_form_row_count_and_batch_mates_change_no_bit(lib, g):
    c = random_case(g)
    cu = c.cu
    fused = R.fused(c.q, c.k).cuda()
    seg_d = c.seg.cuda()
    _, base = random_run(g)
    extra = extra_of(g)
    # (a) the same K bits in a KV cache: the dense row is indexed by cache position - the same columns
    picks, _, got = cache_form(lib, fused, c.seg, g, extra=extra)
    for j, (i, _) in enumerate(picks):
        assert torch.equal(bits(got[j]), bits(base[i])), ("cache form", R.probe_rows()[i])
    # (b) a row alone against the same row among 64 probe rows
    many = [ROWS[i % len(ROWS)] for i in range(64)]
    _, crowd = probe_tokens(lib, fused, g, many, seg_d, extra=extra)
    for i, (b, r, t) in enumerate(R.probe_rows()):
        _, alone = probe_tokens(lib, fused, g, [t], seg_d)
        assert alone.shape[-1] == r + 1
        for at in range(i, 64, len(ROWS)):
            assert torch.equal(bits(alone[0]), bits(crowd[at][:, :r + 1])) and (crowd[at][:, r + 1:].view(torch.int32) == 0).all(), ("row alone", t, at)
        assert torch.equal(bits(crowd[i]), bits(base[i]))
    # (c) a sequence alone (its rows re-packed from row 0) against the sequences side by side
    for b, n in enumerate(R.LENS):
        mine = [(i, r) for i, (bb, r, _) in enumerate(R.probe_rows()) if bb == b]
        _, alone = probe_tokens(lib, fused[cu[b]:cu[b + 1]].contiguous(), g, [r for _, r in mine], c.seg[cu[b]:cu[b + 1]].cuda(), lens=[n])
        w = alone.shape[-1]
        for j, (i, _) in enumerate(mine):
            assert torch.equal(bits(alone[j]), bits(base[i][:, :w])) and (base[i][:, w:].view(torch.int32) == 0).all(), ("sequence alone", b)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_op_refusals_are_host_side_and_write_nothing(lib):
    """ld_tok one below the need, a null tok_out, 65 rows: AIGV_ERR_ARG with a message and both fenced allocations still hold the sentinel.
    No case hands the kernel an index out of range: nothing is launched."""
    c = random_case(1)
    fused, seg_d = R.fused(c.q, c.k).cuda(), c.seg.cuda()
    need = need_of(ROWS, R.LENS)
    assert need == 513
    probe_tokens(lib, fused, 1, ROWS, seg_d, ld_tok=need - 1, refused="ld_tok is below")
    probe_tokens(lib, fused, 1, [ROWS[1]], seg_d, ld_tok=0, refused="ld_tok is below")          # a buffer given, no columns
    probe_tokens(lib, fused, 1, ROWS, seg_d, ld_tok=need, null_tok=True, refused="null tok_out")
    probe_tokens(lib, fused, 1, [ROWS[i % len(ROWS)] for i in range(65)], seg_d, ld_tok=need, refused="probe rows")
    out, tok = probe_tokens(lib, fused, 1, ROWS, seg_d, ld_tok=need)                             # and the accepted call next to them
    assert torch.equal(bits(tok), bits(random_run(1)[1][..., :need]))


# =================================================================================================================================
# model level: the tiny configuration of the score-attention tests, two clips of (2, 1) frames
# =================================================================================================================================
OPTS = dict(return_logprobs=True, top_logprobs=3)


@functools.lru_cache(maxsize=None)
def flagged(stage):
    """(model, cfg, sd, kw, the rig's pass WITHOUT the flag, the same pass WITH it, key count of every clip's probe row)."""
    model, cfg, sd, kw, base = G.rig(stage)
    on = model(**kw, return_token_attention=True, **OPTS)
    torch.cuda.synchronize()
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    n_keys = [r - plan["cu"][b] + 1 for b, r in enumerate(model._probe_rows(plan))]
    return model, cfg, sd, kw, base, on, n_keys


@pytest.mark.parametrize("stage", [2, 1])
def test_model_the_flag_changes_nothing_else_and_rows_sum_to_one(stage):
    model, cfg, sd, kw, base, on, n_keys = flagged(stage)
    assert set(on) == set(base) | {"score_attention_tokens"}
    for key in base:                                                     # score_attention included: the bins keep their bits beside the dense rows
        if torch.is_tensor(base[key]):
            assert torch.equal(on[key], base[key]) or torch.equal(bits(on[key]), bits(base[key])), key
    tok = on["score_attention_tokens"]
    llm = cfg.llm_config
    B, N = kw["input_ids"].shape
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (B, llm.num_hidden_layers, llm.num_attention_heads, N)
    t = tok.cpu()
    for b in range(B):
        assert n_keys[b] <= int(kw["attention_mask"][b].sum())
        assert torch.isfinite(t[b]).all() and (t[b] >= 0).all()
        assert (t[b].double().sum(-1) - 1).abs().max().item() <= TR.row_sum_bound(n_keys[b])
        assert (t[b][..., n_keys[b]:].view(torch.int32) == 0).all()         # behind the score row and in the padding columns: +0.0
        assert (t[b][..., :n_keys[b]] > 0).any(-1).all()
    # only the flag: it implies the bin probe
    only = model(**kw, return_token_attention=True)
    assert torch.equal(bits(only["score_attention"]), bits(base["score_attention"])) and torch.equal(bits(only["score_attention_tokens"]), bits(tok))
    # the context disarmed itself: a plain pass writes no stale tensor
    snap = tok.clone()
    again = model(**kw)
    torch.cuda.synchronize()
    assert "score_attention_tokens" not in again and "score_attention" not in again and torch.equal(tok, snap)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_clip_alone_is_clip_in_batch(stage):
    model, cfg, sd, kw, base, on, n_keys = flagged(stage)
    for b in range(2):
        alone = model(**G.clip_alone(kw, b), return_token_attention=True)["score_attention_tokens"]
        n = alone.shape[-1]
        assert n == int(kw["attention_mask"][b].sum())
        assert torch.equal(bits(alone[0]), bits(on["score_attention_tokens"][b][..., :n])), b


def heat_tolerance(n_keys):
    """heat.sum((2, 3)) against frame_saliency: per (layer, head) the dense values of a frame's keys sum to the frame's bin within c u bin, c =
    ceil(n / 256) + 11 (bin_bound), and so do their head- and layer-means; both sides renormalise - a ratio of two such sums, (1 + c u) /
    (1 - c u) - and both hand back fp32 (one rounding each; the float64 arithmetic between is worth 2^-40)."""
    cu = TR.bin_bound(1.0, n_keys)
    return (1 + cu) / (1 - cu) * (1 + TR.U) / (1 - TR.U) * (1 + 2.0 ** -40) - 1


@pytest.mark.parametrize("stage", [2, 1])
def test_model_frame_heatmaps_sum_to_frame_saliency(stage):
    model, cfg, sd, kw, base, on, n_keys = flagged(stage)
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    ntok = model.num_image_token
    pos = prompts.visual_token_positions(plan["slot"], plan["cu"], [2, 1], ntok)
    g = math.isqrt(ntok)
    assert torch.equal(model.visual_token_positions(kw["input_ids"], kw["attention_mask"], kw["image_flags"]), pos)      # the public way to the same table
    assert tuple(pos.shape) == (2, 2, ntok) and (pos[1, 1] == -1).all() and all(int(pos[b].max()) < n_keys[b] for b in range(2))      # every visual token lies in front of its clip's score row
    for layers in (None, [1], [0, 1]):
        heat = eval_utils.frame_heatmaps(on["score_attention_tokens"], pos, layers=layers).cpu()
        sal = eval_utils.frame_saliency(on["score_attention"], layers=layers).cpu().double()
        assert tuple(heat.shape) == (2, 2, g, g) and (heat[1, 1] == 0).all() and (heat >= 0).all()
        got = heat.double().sum((2, 3))
        for b in range(2):
            err = (got[b] - sal[b]).abs()
            print(f"stage {stage} layers {layers} clip {b}: |heat sum - saliency| / tolerance = {(err / (sal[b] * heat_tolerance(n_keys[b]) + 1e-300)).max().item():.4f}")
            assert (err <= sal[b] * heat_tolerance(n_keys[b])).all(), (b, layers)


def test_model_graph_replay_is_eager():
    model, cfg, sd, kw, base, on, n_keys = flagged(2)
    dev_kw = lambda seed, k=kw, f=3: dict(k, pixel_values=synth.synthetic_frames(f, 224, seed=seed).cuda().to(BF), motion_feature=k["motion_feature"].cuda().to(BF))
    keys = ("score_attention_tokens", "score_attention", "score1")
    grab = lambda o: {k: o[k].clone() for k in keys}
    seeds = [421, 422, 423, 424]
    short = G.clip_alone(kw, 1)                                          # another N: one clip, one frame
    assert short["input_ids"].shape[1] != kw["input_ids"].shape[1]
    eager = [grab(model(**dev_kw(s), return_token_attention=True)) for s in seeds]
    eager_short = [grab(model(**dev_kw(s, short, 1), return_token_attention=True)) for s in seeds[:3]]
    torch.cuda.synchronize()
    assert not torch.equal(eager[0]["score_attention_tokens"], eager[1]["score_attention_tokens"])
    model.enable_graph_replay(True)
    try:
        replayed = [grab(model(**dev_kw(s), return_token_attention=True)) for s in seeds]        # eager, capture, then replays: the third call is one
        torch.cuda.synchronize()
        assert any(isinstance(v, tuple) for v in model._graphs.values()), "the armed pass did not capture"
        for e, r in zip(eager, replayed):
            for k in keys:
                assert torch.equal(bits(e[k]), bits(r[k])), k
        # the copies handed back are not the graph's own tensors: a later replay has not overwritten an earlier result
        assert not torch.equal(replayed[2]["score_attention_tokens"], replayed[3]["score_attention_tokens"])
        bins_only = model(**dev_kw(seeds[0]), return_score_attention=True)                      # the flag is part of the key
        assert "score_attention_tokens" not in bins_only and torch.equal(bits(bins_only["score_attention"]), bits(eager[0]["score_attention"]))
        replayed_short = [grab(model(**dev_kw(s, short, 1), return_token_attention=True)) for s in seeds[:3]]      # another N: its own entry, the same bits
        torch.cuda.synchronize()
        for e, r in zip(eager_short, replayed_short):
            for k in keys:
                assert torch.equal(bits(e[k]), bits(r[k])), ("another N", k)
        assert replayed_short[0]["score_attention_tokens"].shape[-1] == short["input_ids"].shape[1]
        again = grab(model(**dev_kw(seeds[1]), return_token_attention=True))                   # and the first shape still replays its own graph
        assert torch.equal(bits(again["score_attention_tokens"]), bits(eager[1]["score_attention_tokens"]))
    finally:
        model.enable_graph_replay(False)


def layer0_truth(lib, model, cfg, sd, common, p):
    """Layer 0 of one prompt restated in float64 from the weights and the embedded rows (as test_gpu_score_attention's first-principles test):
    {clip: (p64 [n_heads, n], bound [n_heads, n])} of the clip's probe row, the per-key bound widened by the bf16 rounding of q and k - 2^-8
    relative per operand, a further score error of 2 * 2^-8 sum |q||k| / sqrt(D)."""
    llm = cfg.llm_config
    H, nh, nkv = llm.hidden_size, llm.num_attention_heads, llm.num_key_value_heads
    d, g = H // nh, nh // nkv
    n_frames = common["pixel_values"].shape[0]
    plan = model._plan(p["input_ids"], p["attention_mask"], p["labels"], common["image_flags"], n_frames)
    vis, motion = model._visual_inputs(common["pixel_values"].cuda().to(BF), None, common["motion_feature"].cuda().to(BF), plan)
    T = plan["cu"][-1]
    x = torch.empty(T, H, dtype=BF, device="cuda")
    emb = sd["language_model.model.tok_embeddings.weight"].to(BF).cuda()
    ids_d, slot_d = plan["ids_packed"].to(torch.long).cuda(), plan["slot"].to(torch.int32).cuda()
    native.check(lib.aigv_op_embed(ids_d.data_ptr(), slot_d.data_ptr(), emb.data_ptr(), vis.data_ptr(), motion.data_ptr(), plan["n_vis"], x.data_ptr(), T, H,
                                   native.stream_ptr()))
    torch.cuda.synchronize()
    x = x.cpu().double()
    w_n = sd["language_model.model.layers.0.attention_norm.weight"].double()
    w = sd["language_model.model.layers.0.attention.wqkv.weight"].double()
    xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + llm.rms_norm_eps) * w_n
    qkv = (xn @ w.T).view(T, nkv, g + 2, d)
    from aigv_assessor_amd.modeling import rope_tables
    cos, sin = rope_tables(d, llm.rope_theta, max(plan["lens"]), llm.max_position_embeddings, getattr(llm, "rope_scaling", None))
    cos, sin = torch.cat([cos, cos], -1).double(), torch.cat([sin, sin], -1).double()

    def rot(v, pos):
        r = torch.cat((-v[..., d // 2:], v[..., : d // 2]), -1)
        shape = (len(pos),) + (1,) * (v.dim() - 2) + (d,)
        return v * cos[pos].view(shape) + r * sin[pos].view(shape)

    out = {}
    for b, t in enumerate(model._probe_rows(plan)):
        lo = plan["cu"][b]
        pos = torch.arange(t - lo + 1)
        q = rot(qkv[t:t + 1, :, :g], pos[-1:])[0].reshape(nh, d)
        k = rot(qkv[lo:t + 1, :, g], pos)
        eps = R.score_bound(q, k)
        p64 = TR.row_truth(q, k)
        out[b] = (p64, TR.key_bound(p64, eps, t - lo + 1, extra_rel=eps / ((d + 2) * TR.U) * 2 * 2.0 ** -8))
    return out


@pytest.mark.parametrize("stage", [2, 1])
def test_model_shared_prefix_against_separate_passes(lib, stage):
    """Each prompt's dense rows from forward_shared_prefix against a separate full pass of that prompt, per key, in EVERY layer:
    |shared - separate| <= key_bound(separate, eps = 0, n) - test 3's bound with its score term dropped.  The score bound eps needs the layer's
    q and k, which no pass hands out above layer 0; eps >= 0 only widens the bound, so the one asserted here is never wider than test 3's
    (at the test shape the two paths agree bit for bit, as their bins do).  argmax over the keys is equal per (layer, head) wherever the top
    two values of the separate pass (taken in float64) lie further apart than twice that bound.  Layer 0 is also restated in float64 from the
    weights: both paths within key_bound with the layer's own eps and the bf16 rounding of q and k (as test_gpu_score_attention's
    first-principles test), the argmax that of the float64 row wherever ITS margin exceeds twice the bound.  In every layer the columns cover
    prefix + continuation in order (the row's keys, then +0.0), a row sums to 1, and the bins beside the dense rows keep their bits."""
    model, cfg, sd, kw, base = G.rig(stage)
    B, T = 2, 2
    toks = synth.canonical_tokens(cfg, B, T, seed=500 + stage)
    pp = synth.perspective_prompts(toks, 2, seed=500 + stage)
    common = dict(pixel_values=synth.synthetic_frames(B * T, 224, seed=500), image_flags=torch.ones(B * T, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(B, cfg.motion_dim, seed=500))
    separate = [model(**common, input_ids=p["input_ids"], attention_mask=p["attention_mask"], labels=p["labels"], return_token_attention=True) for p in pp]
    shared = model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_token_attention=True)
    plain = model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_score_attention=True)
    torch.cuda.synchronize()
    plans = [model._plan(p["input_ids"], p["attention_mask"], p["labels"], common["image_flags"], B * T) for p in pp]
    N = max(max(pl["lens"]) for pl in plans)
    n_argmax = n_argmax0 = 0
    worst = worst0 = 0.0
    for i, (p, pl) in enumerate(zip(pp, plans)):
        sh, se = shared[i]["score_attention_tokens"].cpu(), separate[i]["score_attention_tokens"].cpu()
        assert sh.shape[-1] == N and se.shape[-1] == p["input_ids"].shape[1] and tuple(sh.shape[:3]) == tuple(se.shape[:3])
        assert torch.equal(bits(shared[i]["score_attention"]), bits(plain[i]["score_attention"]))            # the bins keep their bits beside the dense rows
        for key in ("logit",) + (("score1",) if stage == 2 else ()):
            assert torch.equal(shared[i][key], plain[i][key]), key
        truth = layer0_truth(lib, model, cfg, sd, common, p)
        L, H = sh.shape[1], sh.shape[2]
        for b, t in enumerate(model._probe_rows(pl)):
            n = t - pl["cu"][b] + 1
            for name, got in (("shared", sh), ("separate", se)):
                assert (got[b][..., n:].view(torch.int32) == 0).all(), name
                assert (got[b].double().sum(-1) - 1).abs().max().item() <= TR.row_sum_bound(n), name
            # every layer, per key: shared against separate
            a64, b64 = sh[b][..., :n].double().reshape(L * H, n), se[b][..., :n].double().reshape(L * H, n)
            bound = TR.key_bound(b64, torch.zeros(L * H, dtype=torch.float64), n)
            ratio = ((a64 - b64).abs() / bound).view(L, H, n).amax((1, 2))
            print(f"stage {stage} prompt {i} clip {b}: worst |shared - separate| / bound per layer = {[round(v, 4) for v in ratio.tolist()]}")
            worst = max(worst, ratio.max().item())
            assert (ratio <= 1.0).all(), (i, b, ratio.tolist())
            top2 = b64.topk(2, -1)
            clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * bound.gather(1, top2.indices).max(-1).values
            assert torch.equal(a64.argmax(-1)[clear], top2.indices[:, 0][clear]), (i, b)
            n_argmax += int(clear.sum())
            # layer 0 against its float64 restatement
            p64, bound0 = truth[b]
            for name, got in (("shared", sh), ("separate", se)):
                r0 = ((got[b, 0, :, :n].double() - p64).abs() / bound0).max().item()
                worst0 = max(worst0, r0)
                assert r0 <= 1.0, (name, i, b, r0)
            t2 = p64.topk(2, -1)
            clear0 = (t2.values[:, 0] - t2.values[:, 1]) > 2 * bound0.gather(1, t2.indices).max(-1).values
            assert torch.equal(sh[b, 0, :, :n].argmax(-1)[clear0], t2.indices[:, 0][clear0]) and torch.equal(se[b, 0, :, :n].argmax(-1)[clear0], t2.indices[:, 0][clear0])
            n_argmax0 += int(clear0.sum())
    print(f"stage {stage}: shared against separate, all layers: worst |d| / bound = {worst:.4f}, argmax compared on {n_argmax} (prompt, clip, layer, head) rows; "
          f"layer 0 against float64: worst {worst0:.4f}, argmax on {n_argmax0} rows")
    assert n_argmax > 0


def test_model_more_than_64_rows_and_a_short_ld_tok_are_refused_through_the_new_entry_points(lib):
    """65 clips under ``return_token_attention``: the same ValueError as under ``return_score_attention``.  Through the C ABI: an armed pass with
    65 rows, or with ld_tok below the score row's key count, returns AIGV_ERR_ARG with a message, disarms, and writes nothing."""
    model, cfg, sd, kw, base = G.rig(2)
    many, _ = G.two_clips(cfg, 900, frames=(1,) * 65)
    with pytest.raises(ValueError, match="at most 64"):
        model(**many, return_token_attention=True)
    ctx, llm = model._ctx, cfg.llm_config
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    T, N = plan["cu"][-1], kw["input_ids"].shape[1]
    seg = torch.zeros(T, dtype=torch.int32, device="cuda")
    out = torch.zeros(65 * llm.num_hidden_layers * llm.num_attention_heads * 3, dtype=torch.float32, device="cuda")
    tok = torch.zeros(65 * llm.num_hidden_layers * llm.num_attention_heads * N, dtype=torch.float32, device="cuda")
    for rows, ld_tok, word in (([0] * 65, N, "65 rows"), ([plan["score_rows"][0]], plan["score_rows"][0], "ld_tok"), ([0], 262145, "ld_tok")):
        native.check(lib.aigv_score_attention_arm_tokens(ctx, native.i32_array(rows), len(rows), seg.data_ptr(), None, 0, 3, out.data_ptr(), tok.data_ptr(), ld_tok), ctx)
        vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
        with pytest.raises(native.NativeError, match=word):
            model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"])
        torch.cuda.synchronize()
        assert "score_attention_tokens" not in model(**kw)               # the failed pass disarmed
    assert lib.aigv_score_attention_arm_tokens(ctx, native.i32_array([0]), 1, seg.data_ptr(), None, 0, 3, out.data_ptr(), None, N) == -1      # null tok_out_dev: refused when arming
    assert float(out.abs().sum()) == 0.0 and float(tok.abs().sum()) == 0.0
    again = model(**kw, return_token_attention=True, **OPTS)
    assert torch.equal(bits(again["score_attention_tokens"]), bits(flagged(2)[5]["score_attention_tokens"]))


# ---- 9. every read-out in one call ------------------------------------------------------------------------------------------------------
def int_bits(t):
    """A tensor's bit pattern as integers (NaNs compare)."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape and torch.equal(int_bits(got[k]), int_bits(want[k])), (what, k)


def test_model_all_read_outs_at_once_are_each_read_out_alone():
    """``forward``'s docstring: the read-outs combine freely and none changes another's bits.  One call with all six options on - a ragged pair
    of clips (one right-padded), two and three answer rows, four candidates of which one lies outside the vocabulary, k = 3, a user segment
    table - against the calls with one option at a time, bit for bit; the same call replayed from its graph; and ``forward_shared_prefix``
    over two prompts with every option it takes against its own one-at-a-time calls."""
    model, cfg, sd, kw0, _ = G.rig(2)
    V, T = cfg.llm_config.vocab_size, 2
    t0, t1 = synth.canonical_tokens(cfg, 1, T, seed=910, answer_len=2), synth.canonical_tokens(cfg, 1, T, seed=911, answer_len=1)
    n, pad = t0["input_ids"].shape[1], t0["input_ids"].shape[1] - t1["input_ids"].shape[1]
    assert pad > 0
    ids = torch.cat([t0["input_ids"], torch.cat([t1["input_ids"], torch.zeros(1, pad, dtype=torch.long)], 1)])
    labels = torch.cat([t0["labels"], torch.cat([t1["labels"], torch.full((1, pad), -100)], 1)])
    am = torch.ones(2, n, dtype=torch.bool)
    am[1, n - pad:] = False
    assert sorted((labels[:, 1:] != -100).sum(1).tolist()) == [2, 3]
    kw = dict(pixel_values=synth.synthetic_frames(2 * T, 224, seed=910).cuda().to(BF), input_ids=ids, attention_mask=am,
              image_flags=torch.ones(2 * T, 1, dtype=torch.long), labels=labels, motion_feature=synth.synthetic_motion(2, cfg.motion_dim, seed=910).cuda().to(BF))
    cand = [5, V + 3, 7, 11]
    table = (torch.arange(2 * n) % 5).view(2, n)
    singles = [(dict(return_logprobs=True), ("logprob", "ce_loss")), (dict(candidate_ids=cand), ("cand_logprob",)),
               (dict(top_logprobs=3), ("top_ids", "top_logprob")), (dict(return_score_attention=True, attention_segments=table), ("score_attention",)),
               (dict(return_token_attention=True), ("score_attention_tokens",))]
    everything = {k: v for opts, _ in singles for k, v in opts.items()}
    assert len(everything) == 6
    # (a) each output alone
    off = model(**kw)
    both = model(**kw, **everything)
    torch.cuda.synchronize()
    same_bits(both, off, ("score1", "logit"), "all on against all off")
    for opts, keys in singles:
        alone = model(**kw, **opts)
        same_bits(both, alone, keys + ("score1", "logit"), sorted(opts))
    assert both["cand_logprob"].shape == (2 * (n - 1), 4) and both["top_ids"].shape == (2 * (n - 1), 3) and both["score_attention"].shape[-1] == 5
    assert both["score_attention_tokens"].shape[-1] == n
    answer = labels[:, 1:].reshape(-1) != -100
    assert torch.equal(~torch.isnan(both["logprob"]).cpu(), answer) and torch.equal((both["top_ids"] >= 0).all(-1).cpu(), answer)
    assert torch.isnan(both["cand_logprob"][:, 1]).all() and torch.equal(~torch.isnan(both["cand_logprob"][:, 0]).cpu(), answer)
    # (b) the same call through graph replay: eager, capture, replay
    all_keys = tuple(k for _, keys in singles for k in keys) + ("score1", "logit")
    model.enable_graph_replay(True)
    try:
        for i in range(3):
            again = model(**kw, **everything)
            torch.cuda.synchronize()
            same_bits(again, both, all_keys, f"graph replay, call {i}")
        assert sum(isinstance(v, tuple) for v in model._graphs.values()) == 1 and len(model._graphs) == 1
    finally:
        model.enable_graph_replay(False)
    # (c) the shared-prefix pass: every prompt's dict, all options against one at a time
    toks = synth.canonical_tokens(cfg, 2, T, seed=912)
    pp = [(p["input_ids"], p["attention_mask"], p["labels"]) for p in synth.perspective_prompts(toks, 2, seed=912)]
    common = dict(pixel_values=kw["pixel_values"], image_flags=kw["image_flags"], motion_feature=kw["motion_feature"])
    shared_singles = [(opts, keys) if "attention_segments" not in opts else (dict(return_score_attention=True), keys) for opts, keys in singles]
    shared_all = model.forward_shared_prefix(pp, **common, **{k: v for opts, _ in shared_singles for k, v in opts.items()})
    assert len(shared_all) == 2
    for opts, keys in shared_singles:
        alone = model.forward_shared_prefix(pp, **common, **opts)
        for p in range(2):
            same_bits(shared_all[p], alone[p], keys + ("score1", "logit"), ("shared prefix", p, sorted(opts)))
