"""The depth lens on the GPU: (a) the tap kernel against the gather and the RMSNorm op, bit for bit; (b) the grouped score head against the
single-slice op, group by group; (c) the identities of forward(return_depth_lens=True) on the tiny rig - depth L is the pass's own score,
argmax and log-probabilities, nothing else changes a bit, a clip alone is the clip in its batch, graph replay is eager; (d) under a
knock-out window the depths in front of the window keep their bits; (e) every depth against the composed oracle of
tests/depth_lens_reference.py; (f) the refusals of the C ABI, each by its message."""
import ctypes
import functools

import pytest
import torch

import depth_lens_reference as DL
from test_gpu_key_drop import assert_levels, bits, clip_alone, make_model, same, score_ok, two_clips
from test_gpu_ops import BF, dev, lib, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import FENCE, SENTINEL, fenced, i32, ptr, same_bits, sentinel_like

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth

pytestmark = pytest.mark.gpu

LAYERS = 4
EPS = 1e-6


# =================================================================================================================================
# (a) the tap
# =================================================================================================================================
@pytest.mark.parametrize("pad", [0, 64], ids=["ld=H", "ld=H+64"])
@pytest.mark.parametrize("n", [1, 5, 64, 130])
@pytest.mark.parametrize("H", [128, 4096])
def test_tap_is_gather_and_rmsnorm_bit_for_bit(lib, H, n, pad):
    g = torch.Generator().manual_seed(H + n + pad)
    R, ld = 150, H + pad
    src = (torch.randn(R, ld, generator=g) * 3).to(BF)
    src[7, 5], src[7, H - 1], src[7, 64] = float("nan"), float("inf"), float("-inf")         # travels as through the two ops
    src[9, 0] = float("inf")
    idx = torch.randint(0, R, (n,), generator=g, dtype=torch.int32)
    idx[0] = 7
    if n >= 5:
        idx[1], idx[2], idx[3], idx[4] = R - 1, 0, 7, 9                                      # first and last row, a repeated index
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    src_d, idx_d, w_d = dev(src), dev(idx), dev(w)
    raw_whole, raw = fenced(sentinel_like((n, H), BF))
    nrm_whole, nrm = fenced(sentinel_like((n, H), BF))
    sync(lib.aigv_op_lens_tap(ptr(src_d), ld, ptr(idx_d), n, ptr(w_d), ptr(raw), ptr(nrm), H, EPS, None), lib)
    gathered = dev(torch.zeros(n, H, dtype=BF))
    sync(lib.aigv_op_gather_rows(ptr(src_d), ld, ptr(idx_d), n, ptr(gathered), H, None), lib)
    normed = dev(torch.zeros(n, H, dtype=BF))
    sync(lib.aigv_op_rmsnorm(ptr(gathered), H, ptr(w_d), ptr(normed), H, n, H, EPS, None, None), lib)
    assert torch.equal(gathered.cpu().view(torch.int16), src[idx.long(), :H].contiguous().view(torch.int16))
    same_bits(raw_whole, gathered.cpu())
    same_bits(nrm_whole, normed.cpu())
    assert normed.cpu()[0].isnan().all()                                                    # the NaN row is NaN throughout, as through rmsnorm


# =================================================================================================================================
# (b) the grouped score head
# =================================================================================================================================
PRODUCTION = (4096, 1024, 256, 64, 16, 1)
TINY = (512, 128, 64, 32, 16, 1)


@functools.lru_cache(maxsize=None)
def head_weights(dims):
    g = torch.Generator().manual_seed(sum(dims))
    Ws = tuple((torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5).to(BF) for i, o in zip(dims[:-1], dims[1:]))
    bs = tuple((torch.rand(o, generator=g) * 0.1).to(BF) for o in dims[1:])
    Ws = Ws[:-1] + (Ws[-1].abs(),)                                                          # (a positive last layer: the closing ReLU leaves the scores apart)
    return Ws, bs


def head_single(lib, x_rows_dev, ldx, B, dims, wp, bp):
    n_scratch = 3 * B * max(dims)
    scratch = dev(torch.zeros(n_scratch, dtype=BF))
    score = dev(torch.zeros(B, dtype=torch.float32))
    sync(lib.aigv_op_score_head(ptr(x_rows_dev), ldx, B, len(dims) - 1, i32(dims), wp, bp, ptr(scratch), n_scratch * 2, ptr(score), None), lib)
    return score.cpu()


def head_groups(lib, x, G, B, dims, gap=2):
    """x: CPU bf16 [G, B, H] -> (grouped scores [G, B], per-group single-slice scores [G, B]).  The groups lie `gap` NaN rows apart (the pass's
    layout has the token rows there: a kernel that read them would trip its guard)."""
    H = dims[0]
    lay = torch.full((G, B + gap, H), float("nan"), dtype=BF)
    lay[:, :B] = x
    lay_d = dev(lay)
    n = len(dims) - 1
    Ws, bs = head_weights(dims)
    wd, bd = [dev(w) for w in Ws], [dev(b) for b in bs]
    wp, bp = (ctypes.c_void_p * n)(*[ptr(w) for w in wd]), (ctypes.c_void_p * n)(*[ptr(b) for b in bd])
    n_scratch = 3 * G * B * max(dims)
    scratch_whole, scratch = fenced(sentinel_like((n_scratch,), BF))
    score_whole, score = fenced(sentinel_like((G * B,), torch.float32))
    sync(lib.aigv_op_score_head_groups(ptr(lay_d), H, G, (B + gap) * H, B, n, i32(dims), wp, bp, ptr(scratch), n_scratch * 2, ptr(score), None), lib)
    got = score_whole.cpu()
    fence = torch.full((FENCE,), SENTINEL[torch.float32], dtype=torch.int32)
    assert torch.equal(got[:FENCE].view(torch.int32), fence) and torch.equal(got[FENCE + G * B:].view(torch.int32), fence), "score fences"
    sw = scratch_whole.cpu().view(torch.int16)
    fence16 = torch.full((FENCE,), SENTINEL[BF], dtype=torch.int16)
    assert torch.equal(sw[:FENCE], fence16) and torch.equal(sw[FENCE + n_scratch:], fence16), "scratch fences"
    single = torch.stack([head_single(lib, lay_d[g], H, B, dims, wp, bp) for g in range(G)])
    return got[FENCE:FENCE + G * B].view(G, B).clone(), single, (lay_d, wp, bp, wd, bd)


@pytest.mark.parametrize("G,B", [(1, 4), (5, 1), (33, 3), (33, 4), (3, 64)])
@pytest.mark.parametrize("dims", [PRODUCTION, TINY], ids=["production", "tiny"])
def test_grouped_score_head_is_the_single_slice_op_group_by_group(lib, dims, G, B):
    """With B = 3 a group straddles the 64-row chunk border of the GEMM layers (rows 63, 64, 65 are group 21)."""
    g = torch.Generator().manual_seed(G * 100 + B)
    x = torch.randn(G, B, dims[0], generator=g).to(BF)
    got, single, _ = head_groups(lib, x, G, B, dims)
    assert torch.isfinite(got).all() and (G * B == 1 or got.unique().numel() > 1)
    assert torch.equal(got.view(torch.int32), single.view(torch.int32))


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("dims", [PRODUCTION, TINY], ids=["production", "tiny"])
def test_grouped_score_head_guards_every_group_on_its_own(lib, dims, B):
    """One NaN in group 7 only: every row of group 7 takes the nan_to_num form, no other group does - an Inf in group 9 stays an Inf."""
    G = 33
    g = torch.Generator().manual_seed(B)
    x = torch.randn(G, B, dims[0], generator=g).to(BF)
    x[7, 1, 17] = float("nan")
    x[7, 0, 3] = float("inf")                                                               # group 7's guard turns it into 1e9
    x[9, B - 1, 5] = float("inf")                                                           # group 9 has no NaN: it stays
    got, single, (lay_d, wp, bp, *_keep) = head_groups(lib, x, G, B, dims)
    assert torch.equal(got.view(torch.int32), single.view(torch.int32))
    fixed7 = head_single(lib, dev(torch.nan_to_num(x[7], nan=0.0, posinf=1e9, neginf=-1e9)), dims[0], B, dims, wp, bp)
    assert torch.isfinite(fixed7).all() and torch.equal(got[7].view(torch.int32), fixed7.view(torch.int32))
    assert not torch.isfinite(got[9, B - 1]) and torch.isfinite(got[9, :B - 1]).all()
    others = [i for i in range(G) if i not in (7, 9)]
    assert torch.isfinite(got[others]).all()


# =================================================================================================================================
# model level
# =================================================================================================================================
CAND = [3, 141, 59, 265, 358]
READS = dict(return_logprobs=True, candidate_ids=CAND, top_logprobs=1)
LENS_KEYS = ("lens_score", "lens_score_hidden", "lens_token", "lens_token_logprob", "lens_token_hidden", "lens_cand_logprob")


@functools.lru_cache(maxsize=None)
def rig(stage):
    """The tiny rig with four LLM layers (weights seed 61 + stage, tokens seed 300 + stage: 63 / 302 in stage 2): two clips of 2 and 1 frames,
    N = 215.  -> model, cfg, sd, kw, the segment masks, the unarmed pass, the armed pass."""
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=LAYERS)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    model = make_model(cfg, sd, stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    plain = model(**kw, **READS)
    lens = model(**kw, **READS, return_depth_lens=True)
    torch.cuda.synchronize()
    return model, cfg, sd, kw, seg, plain, lens


def token_positions(kw):
    return [DL.token_row(kw["labels"][b]) for b in range(kw["labels"].shape[0])]


def assert_depth_L_is_the_pass(out, kw, stage):
    """Identities 1 to 4 of one armed call's result dict."""
    B, N = kw["input_ids"].shape
    pos = token_positions(kw)
    if stage == 2:
        assert out["lens_score"].dtype == torch.float32 and tuple(out["lens_score"].shape) == (B, LAYERS + 1)
        assert torch.equal(out["lens_score"], out["lens_score"].to(BF).float())              # the head computes in bf16: exact in fp32
        assert same(out["lens_score"][:, LAYERS].to(BF), out["score1"])                      # 1
    else:
        assert "lens_score" not in out and "lens_score_hidden" not in out
    at = torch.tensor([b * (N - 1) + p for b, p in enumerate(pos)], device=out["logit"].device)
    assert out["lens_token"].dtype == torch.long and same(out["lens_token"][:, LAYERS], out["logit"][at])                    # 2
    assert same(out["lens_token_logprob"][:, LAYERS], out["top_logprob"][at, 0])             # 3
    assert same(out["lens_cand_logprob"][:, LAYERS], out["cand_logprob"][at])                # 4
    assert same(out["lens_token"][:, LAYERS], out["top_ids"][at, 0])


@pytest.mark.parametrize("stage", [2, 1])
def test_depth_L_is_the_pass_and_nothing_else_changes(stage):
    """1 - 5 and 8: depth L of every read-out is the pass's own output, bit for bit; every other output of the armed pass is the unarmed
    pass's; a stage-1 model has the token outputs and no score outputs."""
    model, cfg, sd, kw, seg, plain, lens = rig(stage)
    H = cfg.llm_config.hidden_size
    assert_depth_L_is_the_pass(lens, kw, stage)
    assert set(lens) - set(plain) == set(LENS_KEYS[0 if stage == 2 else 2:])
    for key in plain:                                                                        # 5
        assert plain[key] is None and lens[key] is None or same(plain[key], lens[key]), key
    assert tuple(lens["lens_token_hidden"].shape) == (2, LAYERS + 1, H) and lens["lens_token_hidden"].dtype == BF
    assert tuple(lens["lens_cand_logprob"].shape) == (2, LAYERS + 1, len(CAND)) and torch.isfinite(lens["lens_token_logprob"]).all()
    if stage == 2:
        assert eval_utils.settling_depth(lens["lens_score"], 10.0).tolist() == [0, 0]
        assert eval_utils.settling_depth(lens["lens_score"], 0.0).min() >= 0
    # the flag alone: no labels -> no token outputs (stage 2); other options off -> the lens outputs keep their bits
    bare = model(**kw, return_depth_lens=True)
    for key in LENS_KEYS[0 if stage == 2 else 2:-1]:
        assert same(bare[key], lens[key]), key
    assert "lens_cand_logprob" not in bare and "top_logprob" not in bare
    if stage == 2:
        unl = model(**dict(kw, labels=None), return_depth_lens=True)
        assert not [k for k in unl if k.startswith("lens_token") or k == "lens_cand_logprob"]
        assert same(unl["lens_score"], lens["lens_score"]) and same(unl["lens_score_hidden"], lens["lens_score_hidden"])
    # a clip without an answer token: -1 / NaN there, the other clip untouched
    lab = kw["labels"].clone(); lab[1] = -100
    part = model(**dict(kw, labels=lab), candidate_ids=CAND, return_depth_lens=True)
    assert part["lens_token"][1].eq(-1).all() and part["lens_token_logprob"][1].isnan().all() and part["lens_cand_logprob"][1].isnan().all()
    for key in LENS_KEYS[2:]:
        assert same(part[key][0], lens[key][0]), key


@pytest.mark.parametrize("stage", [2, 1])
def test_clip_alone_is_clip_in_batch(stage):
    """6.  (The data is free of NaN, so the guard slices do not differ.)"""
    model, cfg, sd, kw, seg, plain, lens = rig(stage)
    for b in range(2):
        one, n = clip_alone(kw, b)
        alone = model(**one, **READS, return_depth_lens=True)
        for key in LENS_KEYS[0 if stage == 2 else 2:]:
            assert same(alone[key], lens[key][b:b + 1]), (b, key)


def test_graph_replay_is_eager_and_the_unarmed_graph_stays():
    """7.  The flag is part of the graph key: the armed pass captures a graph of its own, its replay has the eager bits, and a call without the
    flag still replays its old graph."""
    model, cfg, sd, kw, seg, plain, lens = rig(2)
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    model.enable_graph_replay(True)
    try:
        graphs = lambda: sum(isinstance(v, tuple) for v in model._graphs.values())
        outs = [model(**dev_kw, **READS) for _ in range(3)]                                  # eager, capture, replay
        assert graphs() == 1 and len(model._graphs) == 1
        armed = [model(**dev_kw, **READS, return_depth_lens=True) for _ in range(3)]         # eager, capture, replay
        assert graphs() == 2 and len(model._graphs) == 2
        again = model(**dev_kw, **READS)                                                     # the old graph; the armed passes disarmed
        assert graphs() == 2 and len(model._graphs) == 2
        torch.cuda.synchronize()
        for o in outs + [again]:
            assert set(o) == set(plain)
            for key in plain:
                assert plain[key] is None and o[key] is None or same(plain[key], o[key]), key
        for o in armed:
            assert set(o) == set(lens)
            for key in lens:
                assert lens[key] is None and o[key] is None or same(lens[key], o[key]), key
    finally:
        model.enable_graph_replay(False)
    eager = model(**kw, **READS, return_depth_lens=True)
    for key in LENS_KEYS:
        assert same(eager[key], lens[key]), key


def test_fp8_mode_row_trimming_off_and_a_mixed_batch():
    """9, 10: identity 1 (and 2 - 4) in the fp8 mode, with row trimming off (depth L read from the full residual stream) and in a mixed batch
    - clip 0 with more than 16 answer rows finishes on the tile kernels, clip 1's rows are scattered back."""
    model, cfg, sd, kw, seg, plain, lens = rig(2)
    model.set_precision("fp8")
    try:
        out8 = model(**kw, **READS, return_depth_lens=True)
        assert_depth_L_is_the_pass(out8, kw, 2)
        assert not same(out8["lens_score_hidden"], lens["lens_score_hidden"])                # another arithmetic from layer 0 on
        assert same(out8["lens_score_hidden"][:, 0], lens["lens_score_hidden"][:, 0])        # the embedding is the embedding
    finally:
        model.set_precision("bf16")
    model.set_row_trimming(False)
    try:
        untrimmed = model(**kw, **READS, return_depth_lens=True)
        assert_depth_L_is_the_pass(untrimmed, kw, 2)
        for key in LENS_KEYS:                                                                # the depths below L never met the trimmed path
            assert same(untrimmed[key][:, :LAYERS], lens[key][:, :LAYERS]), key
    finally:
        model.set_row_trimming(True)
    n0 = int(kw["attention_mask"][0].sum())
    lab = kw["labels"].clone()
    lab[0, n0 - 24:n0 - 1] = kw["input_ids"][0, n0 - 24:n0 - 1]                              # 20+ answer rows in clip 0
    mixed_kw = dict(kw, labels=lab)
    assert int((lab[0] != -100).sum()) > 16 and int((lab[1] != -100).sum()) <= 16
    mixed = model(**mixed_kw, **READS, return_depth_lens=True)
    assert_depth_L_is_the_pass(mixed, mixed_kw, 2)
    assert same(mixed["lens_score_hidden"][:, :LAYERS], lens["lens_score_hidden"][:, :LAYERS])
    unarmed = model(**mixed_kw, **READS)
    for key in unarmed:
        assert unarmed[key] is None and mixed[key] is None or same(unarmed[key], mixed[key]), key


# ---- (d) under a knock-out ---------------------------------------------------------------------------------------------------------------
def test_under_a_knockout_window_the_depths_in_front_of_it_keep_their_bits():
    model, cfg, sd, kw, seg, plain, lens = rig(2)
    out = model(**kw, **READS, return_depth_lens=True, key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(2, 4))
    for key in ("lens_score_hidden", "lens_token_hidden", "lens_score"):
        assert same(out[key][:, :3], lens[key][:, :3]), key                                  # layers 0 and 1 ran the launches they always ran
    assert_depth_L_is_the_pass(out, kw, 2)                                                   # ... of that masked pass
    masked = model(**kw, **READS, key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(2, 4))
    assert same(out["lens_score"][:, LAYERS].to(BF), masked["score1"]) and not same(masked["logprob"], plain["logprob"])
    assert not same(out["lens_score_hidden"][:, 3:], lens["lens_score_hidden"][:, 3:])
    assert not same(out["lens_token_hidden"][:, 3:], lens["lens_token_hidden"][:, 3:])


def test_flow_knockout_carries_the_lens():
    """The flag travels through eval_utils.flow_knockout's read-out keywords: every pass of the sweep carries its own lens, the depths in front
    of a window keep the base pass's bits, and depth L is that pass's score."""
    model, cfg, sd, kw, seg, plain, lens = rig(2)
    res = eval_utils.flow_knockout(model, **kw, width=2, return_depth_lens=True)
    assert res["windows"] == [(0, 2), (2, 4)] and len(res["outs"]) == 1 + 3 * 2
    base = res["outs"][0]
    for key in LENS_KEYS[:5]:
        assert same(base[key], lens[key]), key
    for p in range(3):
        for w, (lo, hi) in enumerate(res["windows"]):
            out = res["outs"][1 + p * 2 + w]
            assert same(out["lens_score"][:, :lo + 1], base["lens_score"][:, :lo + 1]), (p, w)
            assert same(out["lens_score_hidden"][:, :lo + 1], base["lens_score_hidden"][:, :lo + 1]), (p, w)
            assert same(out["lens_score"][:, LAYERS].to(BF), out["score1"]), (p, w)
    assert any(not same(o["lens_score_hidden"], base["lens_score_hidden"]) for o in res["outs"][1:])


# ---- (e) against the oracle -----------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def oracle_lens(stage, b):
    """The composed reference of clip b alone (its score row is then hidden[:, -4]) in bf16, and the residual rows of the same pass in fp32."""
    model, cfg, sd, kw, seg, plain, lens = rig(stage)
    one, n = clip_alone(kw, b)
    inputs = {k: v for k, v in one.items() if k != "labels"}
    states = DL.composed_states(sd, cfg, **inputs, img_context_token_id=model.img_context_token_id)
    ref = DL.lens(sd, cfg, states, one["attention_mask"], one["labels"], stage, candidate_ids=CAND)
    sd32 = {k: v.float() for k, v in sd.items()}
    in32 = dict(inputs, pixel_values=inputs["pixel_values"].float(), motion_feature=inputs["motion_feature"].float())
    states32 = DL.composed_states(sd32, cfg, **in32, img_context_token_id=model.img_context_token_id)
    ref32 = DL.lens(sd32, cfg, states32, one["attention_mask"], one["labels"], stage)
    return ref, ref32


@pytest.mark.parametrize("stage", [2, 1])
def test_every_depth_against_the_composed_oracle(stage):
    """lens_score within the tiny rig's score bar (1e-3 or 1 bf16 ulp; clip 0's adjacent depths are at least 2 ulps apart: a shifted tap
    fails), lens_token identical up to rows the oracle itself decides within 2 bf16 ulps, and the raw rows by relative L2 distance to the
    oracle's fp32 states, per depth at most 1.3 x the oracle's own bf16-versus-fp32 distance there (DESIGN section 5's factor)."""
    model, cfg, sd, kw, seg, plain, lens = rig(stage)
    for b in range(2):
        ref, ref32 = oracle_lens(stage, b)
        if stage == 2:
            for d in range(LAYERS + 1):
                score_ok(lens["lens_score"][b:b + 1, d], ref["score"][:, d])
        ties = assert_levels(lens["lens_token"][b].cpu(), ref["token"][0], ref["token_logits"][0])
        assert ties <= 1                                                                     # (the existing rule: max(1, rows // 10) of a clip's rows)
        for key, rkey in (("lens_score_hidden", "score_hidden"), ("lens_token_hidden", "token_hidden"))[0 if stage == 2 else 1:]:
            own = rel_l2(ref[rkey][0], ref32[rkey][0])
            got = rel_l2(lens[key][b].cpu(), ref32[rkey][0])
            for d in range(LAYERS + 1):
                print(f"stage {stage} clip {b} {key} depth {d}: hip vs fp32 {got[d].item():.5f}, oracle bf16 vs fp32 {own[d].item():.5f}, bar {1.3 * own[d].item():.5f}")
            assert bool((got <= 1.3 * own).all()), (b, key, got.tolist(), own.tolist())


# ---- (f) refusals through the C ABI --------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message_and_no_fault(lib):
    model, cfg, sd, kw, seg, plain, lens = rig(2)
    ctx = model._ctx
    H, D = cfg.llm_config.hidden_size, LAYERS + 1
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    srows, clips, trows = model._depth_lens_rows(plan, True)
    hidden = torch.zeros(D, 4, H, dtype=BF, device="cuda")
    normed = torch.zeros_like(hidden)
    score = torch.zeros(D, 2, dtype=torch.float32, device="cuda")
    err = lambda: lib.aigv_last_error(ctx).decode()

    def arm(s=srows, t=trows, h=hidden.data_ptr(), n=normed.data_ptr(), sc=score.data_ptr(), ns=None, nt=None):
        return lib.aigv_depth_lens_arm(ctx, i32(s) if s else None, len(s) if ns is None else ns, i32(t) if t else None, len(t) if nt is None else nt, h, n, sc)

    def plain_again():
        torch.cuda.synchronize()
        out = model(**kw, **READS)
        assert same(out["score1"], plain["score1"]) and same(out["logprob"], plain["logprob"])

    # refused by the arm call: nothing armed
    long = list(range(65))
    for kwargs, word in ((dict(s=long), "each list holds 0..64 rows"), (dict(t=long), "each list holds 0..64 rows"), (dict(s=[], t=[]), "no row to read"),
                         (dict(ns=2, s=[]), "null row list"), (dict(h=None), "hidden_out_bf16 is null"), (dict(h=hidden.data_ptr() + 2), "hidden_out_bf16 is null or not 16-byte aligned"),
                         (dict(n=None), "normed_out_bf16 is null"), (dict(n=normed.data_ptr() + 8), "normed_out_bf16 is null or not 16-byte aligned"),
                         (dict(sc=None), "score_out is null"), (dict(sc=score.data_ptr() + 2), "score_out is null or not 4-byte aligned")):
        assert arm(**kwargs) == -1 and word in err() and err().startswith("aigv_depth_lens_arm:"), (kwargs, err())
    plain_again()                                                                           # nothing was armed

    # refused by the pass, before any launch; the context disarms
    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    prefill = lambda score_rows, logit_rows: model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, score_rows, logit_rows)
    not_consumed = [r for r in range(plan["cu"][-1]) if r not in plan["logit_rows"] and r not in plan["score_rows"]][5]
    assert arm(t=[trows[0], not_consumed]) == 0
    with pytest.raises(native.NativeError, match="is not among the pass's consumed rows"):
        prefill(plan["score_rows"], plan["logit_rows"])
    plain_again()
    assert arm() == 0
    with pytest.raises(native.NativeError, match="score == NULL"):
        prefill(None, plan["logit_rows"])
    plain_again()
    assert arm() == 0
    with pytest.raises(native.NativeError, match="no output rows"):
        prefill(None, [])
    plain_again()

    # aigv_llm_extend under an armed lens (the shared-prefix path arms nothing itself: arm by hand behind its prefill)
    base = synth.canonical_tokens(cfg, 2, 2, seed=77)
    pp = synth.perspective_prompts(base, 2, seed=77)
    common = dict(pixel_values=synth.synthetic_frames(4, 224, seed=77), image_flags=torch.ones(4, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(2, cfg.motion_dim, seed=77))
    keep = model._prefill

    def prefill_then_arm(*a, **k):
        out = keep(*a, **k)
        assert arm() == 0
        return out

    model._prefill = prefill_then_arm
    try:
        with pytest.raises(native.NativeError, match="aigv_llm_extend: the depth lens is armed"):
            model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common)
    finally:
        del model._prefill
    plain_again()                                                                           # the refused continuation disarmed too
    again = model(**kw, **READS, return_depth_lens=True)
    for key in LENS_KEYS:
        assert same(again[key], lens[key]), key
    with pytest.raises(TypeError):
        model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_depth_lens=True)
