"""Score-row attention by segment on the MI355X: the probe kernel through aigv_op_attention_probe (no model) on the constructions of
tests/score_attention_reference.py - key census and one-hot selector (bit-exact), random data against float64 with a DERIVED tolerance,
packed against cache addressing, batch invariance, output fencing - and the armed scoring passes through the model
(``forward(return_score_attention=True)``, ``forward_shared_prefix``), stage 2 and stage 1, two clips of different frame counts.
tests/test_score_attention_cpu.py holds, without a GPU, the conditions the exact constructions rest on."""
import ctypes
import functools
import math

import pytest
import torch

import aigv_assessor_amd as pkg
import score_attention_reference as R
from aigv_assessor_amd import eval_utils, native, prompts, synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D, S, HK = R.D, R.S, R.N_KV
SENTINEL = 0x7FA5A5A5      # a NaN bit pattern the kernel cannot produce
PAD = 64                   # floats in front of and behind `out`


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


def probe(lib, fused_d, g, rows, seg_new_d, lens=R.LENS, cache=None, n_seg=S, cos_sin=None, d=D):
    """aigv_op_attention_probe on fused rows [T, HK (g + 2) d]; cache = (kc, cap, kv_off list, seg_cached_d, ld_cached) for the cache form.
    `out` sits between two sentinel pads inside one allocation that starts as the sentinel: returns fp32 [rows, heads, n_seg] after checking
    that the pads kept their bits and that every element of `out` was written."""
    h, ld = HK * g, HK * (g + 2) * d
    n = len(rows) * h * n_seg
    whole = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    out_ptr = whole.data_ptr() + 4 * PAD
    cos, sin = cos_sin or tables()
    cu = native.i32_array(R.cu_of(lens))
    if cache is None:
        k_ptr, ldk, hs, ss, off, segc, ldc = fused_d.data_ptr() + 2 * g * d, ld, (g + 2) * d, 0, None, None, 0
    else:
        kc, cap, kv_off, segc_d, ldc = cache
        k_ptr, ldk, hs, ss, off, segc = kc.data_ptr(), d, cap * d, HK * cap * d, native.i32_array(kv_off), segc_d.data_ptr()
    native.check(lib.aigv_op_attention_probe(fused_d.data_ptr(), ld, k_ptr, ldk, cu, len(lens), h, HK, (g + 2) * d, hs, ss, off, d, cos.data_ptr(),
                                             sin.data_ptr(), cos.shape[0], native.i32_array(rows), len(rows), seg_new_d.data_ptr(), segc, ldc, n_seg,
                                             ctypes.c_void_p(out_ptr), native.stream_ptr()))
    torch.cuda.synchronize()
    w = whole.cpu()
    assert (w[:PAD] == SENTINEL).all() and (w[PAD + n:] == SENTINEL).all(), "the probe wrote outside its output"
    assert (w[PAD:PAD + n] != SENTINEL).all(), "the probe left part of its output unwritten"
    return w[PAD:PAD + n].view(torch.float32).view(len(rows), h, n_seg).clone()


ROWS = [t for _, _, t in R.probe_rows()]


def cache_form_probe(lib, fused, seg, pos, g):
    """The op-level case in CACHE form: K of every token stored at its position by aigv_op_kv_store (the rest of the cache is NaN), the pass =
    the rows behind CACHE_OFF[b] of every sequence (different, non-zero offsets), seg_cached = the table of the cached keys.  Returns
    ([(index into probe_rows(), packed row of the shortened pass)], fp32 [picks, heads, S])."""
    cu, off, cap, T = R.cu_of(R.LENS), R.CACHE_OFF, R.CACHE_CAP, sum(R.LENS)
    kc = torch.full((len(R.LENS), HK, cap, D), float("nan"), dtype=BF, device="cuda")
    vc = torch.zeros_like(kc)
    seq = torch.repeat_interleave(torch.arange(len(R.LENS)), torch.tensor(R.LENS)).to(torch.int32).cuda()
    pos_d = pos.cuda()
    native.check(lib.aigv_op_kv_store(fused.data_ptr(), fused.shape[1], seq.data_ptr(), pos_d.data_ptr(), kc.data_ptr(), vc.data_ptr(), T, HK, g, D, cap,
                                      native.stream_ptr()))
    new_lens = [n - o for n, o in zip(R.LENS, off)]
    keep = torch.cat([torch.arange(cu[b] + off[b], cu[b + 1]) for b in range(len(R.LENS))])
    cu_new = R.cu_of(new_lens)
    ldc = max(off) + 3
    segc = torch.zeros(len(R.LENS), ldc, dtype=torch.int32)
    for b in range(len(R.LENS)):
        segc[b, :off[b]] = seg[cu[b]:cu[b] + off[b]]
    picks = [(i, cu_new[b] + r - off[b]) for i, (b, r, t) in enumerate(R.probe_rows()) if r >= off[b]]
    assert {R.probe_rows()[i][0] for i, _ in picks} == {0, 1, 2} and len(picks) >= 10
    got = probe(lib, fused[keep.cuda()].contiguous(), g, [t for _, t in picks], seg[keep].cuda(), lens=new_lens, cache=(kc, cap, off, segc.cuda(), ldc))
    return picks, got


# ---- 1. key census --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_key_census_counts_exactly_and_ignores_poison(lib, g):
    """Q = 0: out == count_in_segment / n_visible, the fp32 division, bit for bit - for all rows in one launch, and for every row alone with
    NaN in every key it must not read (behind it, the neighbouring sequences) and huge finite K rows in the keys of dropped segments."""
    gen = torch.Generator().manual_seed(5 + g)
    T, cu = sum(R.LENS), R.cu_of(R.LENS)
    q = torch.zeros(T, HK, g, D, dtype=BF)
    k = torch.randn(T, HK, D, generator=gen).to(BF)
    seg = R.seg_table()
    k[(seg < 0) | (seg >= S)] = 3.0e38                                     # dropped segments: huge, finite (0 * huge = 0)
    want = R.census_expect()
    seg_d = seg.cuda()
    got = probe(lib, R.fused(q, k).cuda(), g, ROWS, seg_d)
    for i, t in enumerate(ROWS):
        assert torch.equal(bits(got[i]), bits(want[t].expand(HK * g, S))), (t, got[i, 0].tolist(), want[t].tolist())
    # the census in cache form (per-sequence key offsets 0 / 100 / 254): the same counts over cached + new keys
    picks, cached = cache_form_probe(lib, R.fused(q, k).cuda(), seg, R.positions(), g)
    for j, (i, _) in enumerate(picks):
        assert torch.equal(bits(cached[j]), bits(got[i])), ("cache form", R.probe_rows()[i])
    for i, (b, r, t) in enumerate(R.probe_rows()):
        kp = k.clone()
        kp[:cu[b]] = float("nan")
        kp[t + 1:] = float("nan")
        one = probe(lib, R.fused(q, kp).cuda(), g, [t], seg_d)
        assert torch.equal(bits(one[0]), bits(got[i])), (b, r)


# ---- 2. one-hot selector --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_one_hot_selector_is_exactly_one_hot(lib, g):
    """The selected key leads by a margin at which exp underflows to 0: exactly 1.0 in its bin (0.0 if its segment is dropped), 0.0
    elsewhere - with the real rotary tables: a query left unrotated would select the competitor instead."""
    for b, r, sel in R.selector_cases():
        c = R.SelectorCase(g, b, r, sel)
        got = probe(lib, R.fused(c.q, c.k).cuda(), g, [c.row], c.seg.cuda())
        assert torch.equal(bits(got[0]), bits(c.expect())), (b, r, sel, got[0].tolist())


# ---- 3. random data against float64 ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(g):
    return R.RandomCase(g)


def device_rotated_q(lib, c):
    """The bf16 bits the kernel's rotation must produce: aigv_op_rope on a copy of the fused rows (the g query slots of every group)."""
    g = c.g
    f = R.fused(c.q, c.k).cuda()
    cos, sin = tables()
    pos_d = c.pos.cuda()
    native.check(lib.aigv_op_rope(f.data_ptr(), f.shape[1], pos_d.data_ptr(), cos.data_ptr(), sin.data_ptr(), c.T, g, g + 2, HK, D, native.stream_ptr()))
    torch.cuda.synchronize()
    return f.cpu().view(c.T, HK, g + 2, D)[:, :, :g].contiguous()


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_random_data_against_float64_within_the_derived_bound(lib, g):
    """Truth from the bf16 bits the kernel sees (q rotated by aigv_op_rope itself); |d mass| <= mass (e^(2 eps) - 1 + c 2^-24 (n + S)) + 2^-24
    with eps = (D + 2) 2^-24 max sum |q||k| / sqrt(D) (score_attention_reference.mass_bound: derived, not chosen)."""
    c = random_case(g)
    q_rot = device_rotated_q(lib, c)
    assert torch.equal(q_rot.view(torch.int16), R.rotate_q(c.q, c.pos, c.cos, c.sin).view(torch.int16))      # (the host restatement holds the same bits)
    got = probe(lib, R.fused(c.q, c.k).cuda(), g, ROWS, c.seg.cuda())
    truth = c.truth(q_rot)
    worst = 0.0
    for i, t in enumerate(ROWS):
        mass, bound = truth[t]
        ratio = ((got[i].double() - mass).abs() / bound).max().item()
        worst = max(worst, ratio)
    print(f"g={g}: worst |mass - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- 4. packed against cache addressing, 5. batch invariance ------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_cache_form_and_batch_mates_change_no_bit(lib, g):
    c = random_case(g)
    cu, off, cap = c.cu, R.CACHE_OFF, R.CACHE_CAP
    fused = R.fused(c.q, c.k).cuda()
    seg_d = c.seg.cuda()
    base = probe(lib, fused, g, ROWS, seg_d)
    # (a) the same K bits in a KV cache (aigv_op_kv_store, every token at its position), the pass = the rows behind kv_off of every sequence
    picks, got = cache_form_probe(lib, fused, c.seg, c.pos, g)
    for j, (i, _) in enumerate(picks):
        assert torch.equal(bits(got[j]), bits(base[i])), ("cache form", R.probe_rows()[i])
    # (b) every row alone against all rows in one launch
    for i, t in enumerate(ROWS):
        assert torch.equal(bits(probe(lib, fused, g, [t], seg_d)[0]), bits(base[i])), ("row alone", t)
    # (c) every sequence alone (its rows re-packed from row 0) against the sequences side by side
    for b, n in enumerate(R.LENS):
        mine = [(i, r) for i, (bb, r, _) in enumerate(R.probe_rows()) if bb == b]
        alone = probe(lib, fused[cu[b]:cu[b + 1]].contiguous(), g, [r for _, r in mine], c.seg[cu[b]:cu[b + 1]].cuda(), lens=[n])
        for j, (i, _) in enumerate(mine):
            assert torch.equal(bits(alone[j]), bits(base[i])), ("sequence alone", b)


# ---- 6. fencing: every launch above runs inside `probe`'s sentinel fence; here the largest output the limits allow ------------------
def test_op_output_fence_at_the_limits(lib):
    g, n_seg = 1, 64
    c = random_case(1)
    seg = (torch.arange(c.T) % 64).to(torch.int32)
    rows = [ROWS[i % len(ROWS)] for i in range(64)]
    got = probe(lib, R.fused(c.q, c.k).cuda(), g, rows, seg.cuda(), n_seg=n_seg)
    assert torch.equal(bits(got[0]), bits(got[len(ROWS)]))                 # the same row twice: the same bits
    s = got.double().sum(-1)
    assert (s - 1).abs().max().item() <= 4 * 2.0 ** -23                   # nothing dropped: a row's bins sum to 1


# =================================================================================================================================
# model level
# =================================================================================================================================
def make_model(cfg, sd, stage):
    from aigv_assessor_amd.modeling import InternVLChatModel
    m = InternVLChatModel(cfg, stage=stage)
    m.load_state_dict(sd)
    return m.eval().cuda()


def two_clips(cfg, seed, frames=(2, 1)):
    """Two clips of DIFFERENT frame counts, right-padded to one N."""
    ts = [synth.canonical_tokens(cfg, 1, f, seed=seed + i) for i, f in enumerate(frames)]
    n = max(t["input_ids"].shape[1] for t in ts)
    ids = torch.zeros(len(ts), n, dtype=torch.long)
    labels = torch.full((len(ts), n), -100)
    am = torch.zeros(len(ts), n, dtype=torch.bool)
    for i, t in enumerate(ts):
        k = t["input_ids"].shape[1]
        ids[i, :k], labels[i, :k], am[i, :k] = t["input_ids"][0], t["labels"][0], True
    F = sum(frames)
    return dict(pixel_values=synth.synthetic_frames(F, 224, seed=seed), input_ids=ids, attention_mask=am, image_flags=torch.ones(F, 1, dtype=torch.long),
                labels=labels, motion_feature=synth.synthetic_motion(len(ts), cfg.motion_dim, seed=seed)), ts[0]["img_context_token_id"]


@functools.lru_cache(maxsize=None)
def rig(stage):
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    model = make_model(cfg, sd, stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    on = model(**kw, return_score_attention=True, return_logprobs=True, top_logprobs=3)
    torch.cuda.synchronize()
    return model, cfg, sd, kw, on


def clip_alone(kw, b, frames=(2, 1)):
    f0 = sum(frames[:b])
    n = int(kw["attention_mask"][b].sum())
    return dict(pixel_values=kw["pixel_values"][f0:f0 + frames[b]], input_ids=kw["input_ids"][b:b + 1, :n], attention_mask=kw["attention_mask"][b:b + 1, :n],
                image_flags=kw["image_flags"][f0:f0 + frames[b]], labels=kw["labels"][b:b + 1, :n], motion_feature=kw["motion_feature"][b:b + 1])


@pytest.mark.parametrize("stage", [2, 1])
def test_model_armed_pass_changes_nothing_else_and_sums_to_one(stage):
    model, cfg, sd, kw, on = rig(stage)
    off = model(**kw, return_logprobs=True, top_logprobs=3)
    torch.cuda.synchronize()
    assert set(on) == set(off) | {"score_attention"}
    for key in (["score1"] if stage == 2 else []) + ["logit", "logprob", "top_ids"]:
        assert torch.equal(on[key], off[key]) or torch.equal(bits(on[key]), bits(off[key])), key
    att = on["score_attention"]
    llm = cfg.llm_config
    assert att.dtype == torch.float32 and tuple(att.shape) == (2, llm.num_hidden_layers, llm.num_attention_heads, 2 + prompts.N_TEXT_SEGMENTS)
    a = att.cpu()
    assert torch.isfinite(a).all() and (a >= 0).all()
    assert (a.double().sum(-1) - 1).abs().max().item() <= 4 * 2.0 ** -23            # bins + nothing dropped: 1 within 4 ulp per (clip, layer, head)
    assert (a[1, :, :, 1] == 0).all() and (a[0, :, :, 1] > 0).all()                   # clip 1 has one frame: its frame bin 1 stays empty
    sal = eval_utils.frame_saliency(att)
    assert tuple(sal.shape) == (2, 2) and torch.allclose(sal.sum(-1).cpu(), torch.ones(2), atol=1e-6)
    # the context disarmed itself: the next plain pass gives the plain outputs again and no stale tensor is written
    snap = att.clone()
    again = model(**kw)
    torch.cuda.synchronize()
    assert "score_attention" not in again and torch.equal(att, snap)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_clip_alone_is_clip_in_batch(stage):
    model, cfg, sd, kw, on = rig(stage)
    for b in range(2):
        alone = model(**clip_alone(kw, b), return_score_attention=True)["score_attention"]
        S_b = alone.shape[-1]                                    # clip 1 alone has F = 1: one frame bin fewer, the same bits behind it
        batch = on["score_attention"][b]
        if S_b != batch.shape[-1]:
            batch = torch.cat([batch[..., :1], batch[..., 2:]], -1)
        assert torch.equal(bits(alone[0]), bits(batch)), b


@pytest.mark.parametrize("stage", [2, 1])
def test_model_layer0_from_first_principles(lib, stage):
    """RMSNorm -> wqkv -> RoPE of layer 0 restated in float64 from the weights and the embedded rows (aigv_op_embed on the model's own visual
    and motion tokens); the probe's layer-0 masses lie within the op-level bound widened by the bf16 rounding of q and k - 2^-8 relative
    per operand, i.e. a further score error of 2 * 2^-8 * sum |q||k| / sqrt(D), propagated through the exponent the same way."""
    model, cfg, sd, kw, on = rig(stage)
    llm = cfg.llm_config
    H, nh, nkv = llm.hidden_size, llm.num_attention_heads, llm.num_key_value_heads
    d, g = H // nh, nh // nkv
    n_frames = kw["pixel_values"].shape[0]
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], n_frames)
    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    T = plan["cu"][-1]
    x = torch.empty(T, H, dtype=BF, device="cuda")
    emb = sd["language_model.model.tok_embeddings.weight"].to(BF).cuda()
    ids_d, slot_d = plan["ids_packed"].to(torch.long).cuda(), plan["slot"].to(torch.int32).cuda()     # (held until the synchronise: the op takes raw pointers)
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

    seg, n_seg = model._default_segments(plan)
    rows = model._probe_rows(plan)
    got = on["score_attention"].cpu()
    worst = 0.0
    for b, t in enumerate(rows):
        lo = plan["cu"][b]
        pos = torch.arange(t - lo + 1)
        q = rot(qkv[t:t + 1, :, :g], pos[-1:])[0].reshape(nh, d)
        k = rot(qkv[lo:t + 1, :, g], pos)
        mass, dropped = R.row_truth(q, k, seg[lo:t + 1], n_seg)
        assert dropped.abs().max() == 0
        eps = R.score_bound(q, k)
        bound = R.mass_bound(mass, eps, t - lo + 1, n_seg, extra_rel=eps / ((d + 2) * 2.0 ** -24) * 2 * 2.0 ** -8)
        worst = max(worst, ((got[b, 0].double() - mass).abs() / bound).max().item())
    print(f"stage {stage}: layer 0 worst |mass - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0


def test_model_graph_replay_is_eager():
    model, cfg, sd, kw, on = rig(2)
    dev_kw = lambda seed: dict(kw, pixel_values=synth.synthetic_frames(3, 224, seed=seed).cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    seeds = [411, 412, 413, 414, 415]
    eager = [model(**dev_kw(s), return_score_attention=True)["score_attention"].clone() for s in seeds]
    torch.cuda.synchronize()
    assert not torch.equal(eager[0], eager[1])
    model.enable_graph_replay(True)
    try:
        replayed = [model(**dev_kw(s), return_score_attention=True)["score_attention"].clone() for s in seeds]     # eager, capture, then three replays
        torch.cuda.synchronize()
        assert any(isinstance(v, tuple) for v in model._graphs.values()), "the armed pass did not capture"
        for e, r in zip(eager, replayed):
            assert torch.equal(bits(e), bits(r))
        plain = model(**dev_kw(seeds[0]))                     # the flag is part of the key: a pass without it is another graph entry
        assert "score_attention" not in plain
        # a user's table is a graph INPUT (its bin count is key): other values replay the same graph
        half = lambda cut: (torch.arange(kw["input_ids"].shape[1])[None, :] >= cut).long().expand_as(kw["input_ids"]).contiguous().cuda()
        got = [model(**dev_kw(seeds[0]), return_score_attention=True, attention_segments=half(cut))["score_attention"].clone() for cut in (40, 40, 90, 150)]
        n_graphs = sum(isinstance(v, tuple) for v in model._graphs.values())
        model.enable_graph_replay(False)
        for cut, a in zip((40, 40, 90, 150), got):
            assert torch.equal(bits(a), bits(model(**dev_kw(seeds[0]), return_score_attention=True, attention_segments=half(cut))["score_attention"])), cut
        assert n_graphs == 2                                  # the armed pass with the default table, and ONE graph for the three user tables
    finally:
        model.enable_graph_replay(False)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_shared_prefix_against_separate_passes(stage):
    """Each prompt's tensor from forward_shared_prefix lies within 1.3 x the project's yardstick for 'the same up to summation order' of the
    separate forward of that prompt: the distance between two forward calls that differ only in GEMM mode (1 against 2), measured here."""
    model, cfg, sd, kw, on = rig(stage)
    B, T = 2, 2
    base = synth.canonical_tokens(cfg, B, T, seed=500 + stage)
    pp = synth.perspective_prompts(base, 3, seed=500 + stage)
    common = dict(pixel_values=synth.synthetic_frames(B * T, 224, seed=500), image_flags=torch.ones(B * T, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(B, cfg.motion_dim, seed=500))
    sep = lambda p: model(**common, input_ids=p["input_ids"], attention_mask=p["attention_mask"], labels=p["labels"], return_score_attention=True)["score_attention"]
    try:
        model.set_gemm_mode(1)
        m1 = [sep(p).clone() for p in pp]
        model.set_gemm_mode(2)
        m2 = [sep(p).clone() for p in pp]
    finally:
        model.set_gemm_mode(-1)
    yard = max((a.double() - b.double()).abs().max().item() for a, b in zip(m1, m2))
    separate = [sep(p).clone() for p in pp]
    shared = model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_score_attention=True)
    torch.cuda.synchronize()
    dist = max((s["score_attention"].double() - f.double()).abs().max().item() for s, f in zip(shared, separate))
    print(f"stage {stage}: shared-prefix distance {dist:.3e}, GEMM-mode yardstick {yard:.3e}")
    for s in shared:
        a = s["score_attention"]
        assert tuple(a.shape) == tuple(separate[0].shape) and (a.double().sum(-1) - 1).abs().max().item() <= 4 * 2.0 ** -23
    assert dist <= 1.3 * yard


def test_model_refusals_come_with_a_message_and_no_fault(lib):
    model, cfg, sd, kw, on = rig(2)
    ctx = model._ctx
    llm = cfg.llm_config
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    T = plan["cu"][-1]
    seg = torch.zeros(T, dtype=torch.int32, device="cuda")
    out = torch.zeros(65 * llm.num_hidden_layers * llm.num_attention_heads * 65, dtype=torch.float32, device="cuda")

    def armed_prefill(rows, n_seg):
        native.check(lib.aigv_score_attention_arm(ctx, native.i32_array(rows), len(rows), seg.data_ptr(), None, 0, n_seg, out.data_ptr()), ctx)
        vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
        return model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"])

    for rows, n_seg, word in (([0], 65, "65 segments"), ([0] * 65, 3, "65 rows"), ([T], 3, "outside the pass"), ([-1], 3, "outside the pass")):
        with pytest.raises(native.NativeError, match=word):
            armed_prefill(rows, n_seg)
        torch.cuda.synchronize()
        armed_prefill_ok = model(**kw)                                    # the failed pass disarmed: a plain pass runs, nothing is written to `out`
        assert "score_attention" not in armed_prefill_ok
    assert float(out.abs().sum()) == 0.0
    # aigv_llm_extend armed without seg_cached
    base = synth.canonical_tokens(cfg, 2, 2, seed=77)
    pp = synth.perspective_prompts(base, 2, seed=77)
    common = dict(pixel_values=synth.synthetic_frames(4, 224, seed=77), image_flags=torch.ones(4, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(2, cfg.motion_dim, seed=77))
    keep = model._arm_score_attention

    def arm_without_cached(probe):
        rows, seg_new, _seg_cached, _ld, n = probe
        return keep((rows, seg_new, None, 0, n))

    model._arm_score_attention = arm_without_cached
    try:
        with pytest.raises(native.NativeError, match="seg_cached"):
            model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_score_attention=True)
    finally:
        model._arm_score_attention = keep
    torch.cuda.synchronize()
    ok = model(**kw, return_score_attention=True)
    assert torch.equal(bits(ok["score_attention"]), bits(on["score_attention"]))
    for bad in (dict(attention_segments=torch.zeros(2, 3, dtype=torch.long)), dict(attention_segments=torch.full_like(kw["input_ids"], 64))):
        with pytest.raises(ValueError):
            model(**kw, return_score_attention=True, **bad)


def test_model_user_segment_table(lib):
    """A user's own table (laid out like input_ids): two bins - the clip's first half, its second half - and -1 on the padding."""
    model, cfg, sd, kw, on = rig(2)
    ids = kw["input_ids"]
    table = torch.full_like(ids, -1)
    for b in range(2):
        n = int(kw["attention_mask"][b].sum())
        table[b, :n // 2], table[b, n // 2:n] = 0, 1
    att = model(**kw, return_score_attention=True, attention_segments=table)["score_attention"]
    assert tuple(att.shape)[-1] == 2 and (att.double().sum(-1) - 1).abs().max().item() <= 4 * 2.0 ** -23
    assert torch.equal(bits(att), bits(model(**kw, return_score_attention=True, attention_segments=table.cuda())["score_attention"]))
