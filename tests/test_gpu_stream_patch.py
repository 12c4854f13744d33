"""Activation patching on the GPU: (a) the row-copy kernel in both directions against torch indexing, bit for bit, between fences; (b) the capture
of forward(return_stream=...) against what the pass itself produces; (c) the identities of forward(stream_patch=...) on the tiny rig - a
self-patch changes nothing, a transplant of every row turns the recipient into the donor from that depth on, a depth-0 patch of text rows is
the pass on the donor's ids, a capture reads the patched stream, causality; (d) the patched pass against the composed oracle of
tests/stream_patch_reference.py; (e) with a knock-out, in fp8 mode, under graph replay; (f) eval_utils.causal_trace; (g) the refusals of the C
ABI at the pass, each by its message."""
import functools

import pytest
import torch

import stream_patch_reference as SP
from test_gpu_key_drop import assert_levels, clip_alone, make_model, same, score_ok, two_clips
from test_gpu_ops import BF, dev, lib, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import fenced, i32, ptr, same_bits, sentinel_like

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth
from aigv_assessor_amd.readouts import StreamPatch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LAYERS = 4
FRAMES = (2, 2)


# =================================================================================================================================
# (a) the kernel
# =================================================================================================================================
def special_rows(t, H):
    """A NaN, a +Inf and a -Inf payload in the first row of t [rows, >= H] (and a NaN with another payload in its last column)."""
    t[0, 5], t[0, H // 2], t[0, H // 4] = float("nan"), float("inf"), float("-inf")
    t.view(torch.int16)[0, H - 1] = 0x7FA5                                                  # a NaN with a payload of its own: the copy moves bits
    return t


@pytest.mark.parametrize("pad", [0, 64], ids=["ld=H", "ld=H+64"])
@pytest.mark.parametrize("n_depths", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 130])
@pytest.mark.parametrize("H", [128, 4096])
def test_row_copy_both_directions_against_torch_indexing(lib, H, n, n_depths, pad):
    g = torch.Generator().manual_seed(H + 7 * n + n_depths + pad)
    R, ld, depth = 150, H + pad, n_depths // 2                                               # (a middle depth of three)
    if n == 1:
        rows = [R - 1] if n_depths == 1 else [0]
    else:
        inner = (torch.randperm(R - 2, generator=g)[:n - 2] + 1).sort().values.tolist()
        rows = [0] + inner + [R - 1]                                                        # the first and the last row, strictly ascending
    at = torch.tensor(rows)

    # capture: side(i, depth) = stream[rows[i]]; the other depths, the stream and the fences keep their bits
    stream = (torch.randn(R, ld, generator=g) * 3).to(BF)
    stream[rows[0]] = special_rows(stream[rows[0]:rows[0] + 1].clone(), H)[0]
    stream_whole, stream_d = fenced(stream)
    side_whole, side_d = fenced(sentinel_like((n, n_depths, H), BF))
    idx_whole, idx_d = fenced(sentinel_like((n,), torch.int32))
    sync(lib.aigv_op_stream_rows(ptr(stream_d), ld, R, i32(rows), n, ptr(idx_d), ptr(side_d), n_depths, depth, H, 0, None), lib)
    want = sentinel_like((n, n_depths, H), BF)
    want[:, depth] = stream[at, :H]
    same_bits(side_whole, want)
    same_bits(stream_whole, stream)
    same_bits(idx_whole, at.to(torch.int32))
    assert side_d[0, depth].isnan().any() and side_d[0, depth].isinf().sum() == 2

    # patch: stream[rows[i]] = side(i, depth); rows not selected, the padding columns, the side buffer and the fences keep their bits
    values = (torch.randn(n, n_depths, H, generator=g) * 3).to(BF)
    values[0, depth] = special_rows(values[0, depth][None].clone(), H)[0]
    stream_whole, stream_d = fenced(stream)
    side_whole, side_d = fenced(values)
    sync(lib.aigv_op_stream_rows(ptr(stream_d), ld, R, i32(rows), n, ptr(idx_d), ptr(side_d), n_depths, depth, H, 1, None), lib)
    want = stream.clone()
    want[at, :H] = values[:, depth]
    same_bits(stream_whole, want)
    same_bits(side_whole, values)
    assert n == R or not torch.equal(want.view(torch.int16), stream.view(torch.int16))


# =================================================================================================================================
# model level
# =================================================================================================================================
CAND = [3, 141, 59, 265, 358]
READS = dict(return_logprobs=True, candidate_ids=CAND, top_logprobs=1, return_depth_lens=True)
LENS_HIDDEN = ("lens_score_hidden", "lens_token_hidden")


def assert_same_outputs(got, want, skip=()):
    assert set(got) - set(skip) == set(want) - set(skip), (sorted(got), sorted(want))
    for key in want:
        if key not in skip:
            assert want[key] is None and got[key] is None or same(got[key], want[key]), key


@functools.lru_cache(maxsize=None)
def rig():
    """The tiny stage-2 rig with four LLM layers (weights seed 63, tokens seed 302): two clips of two frames each, both of 215 tokens with equal
    <IMG_CONTEXT> positions.  -> model, cfg, sd, kw, the segment masks, the plain pass (with every read-out and the lens), the pass that captures
    every row at every depth."""
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=LAYERS)
    sd = synth.make_state_dict(cfg, seed=63, rich=True)
    model = make_model(cfg, sd, 2)
    kw, ctx_id = two_clips(cfg, 302, frames=FRAMES)
    model.img_context_token_id = ctx_id
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    plain = model(**kw, **READS)
    whole = model(**kw, **READS, return_stream=torch.ones_like(kw["attention_mask"]))
    torch.cuda.synchronize()
    return model, cfg, sd, kw, seg, plain, whole


def rows_of(whole, mask):
    """The rows of the all-rows capture that a mask [B, N] selects: (stream rows [n, L, H], their index [n, 2] on the host)."""
    index = whole["stream_index"].cpu()
    own = mask[index[:, 0], index[:, 1]]
    return whole["stream"][own.to(whole["stream"].device)], index[own]


def only_clip(mask, b):
    out = torch.zeros_like(mask)
    out[b] = mask[b]
    return out


# ---- (b) the capture ----------------------------------------------------------------------------------------------------------------
def test_capture_reads_what_the_pass_produces_and_changes_nothing_else():
    model, cfg, sd, kw, seg, plain, whole = rig()
    H = cfg.llm_config.hidden_size
    assert_same_outputs(whole, plain, skip=("stream", "stream_index"))
    n = int(whole["stream_index"].shape[0])
    assert whole["stream"].dtype == BF and tuple(whole["stream"].shape) == (n, LAYERS, H) and whole["stream_index"].dtype == torch.long
    index = whole["stream_index"].cpu()
    # padding and the dead tail are skipped: both clips run positions 0 .. 213 of their 215 tokens (the closing token follows the last consumed row)
    assert n == 2 * 214 and torch.equal(index, torch.stack([torch.arange(2).repeat_interleave(214), torch.arange(214).repeat(2)], 1))
    # depth 0 of the visual rows: the projector's output, in frame order
    vis, vis_index = rows_of(whole, seg["frames"])
    feature = model.extract_feature(kw["pixel_values"].cuda().to(BF))
    assert same(vis[:, 0], feature.reshape(-1, H)) and vis.shape[0] == sum(FRAMES) * model.num_image_token
    # the score row at depths 0 .. L - 1: the lens' rows; through a capture of its own, with a window
    srow = model(**kw, return_stream=seg["score_row"].long().cuda())
    assert same(srow["stream"], plain["lens_score_hidden"][:, :LAYERS]) and srow["stream_index"].tolist() == [[0, 211], [1, 211]]
    part = model(**kw, return_stream=seg["text_after"], stream_depths=(1, 3))
    assert same(part["stream"], rows_of(whole, seg["text_after"])[0][:, 1:3]) and same(part["score1"], plain["score1"])
    # empty selections and windows
    none = model(**kw, return_stream=torch.zeros_like(seg["frames"]))
    assert tuple(none["stream"].shape) == (0, LAYERS, H) and tuple(none["stream_index"].shape) == (0, 2)
    flat = model(**kw, return_stream=seg["score_row"], stream_depths=(2, 2))
    assert tuple(flat["stream"].shape) == (2, 0, H) and flat["stream_index"].tolist() == [[0, 211], [1, 211]]
    dead = torch.zeros_like(seg["frames"]); dead[:, 214] = True
    assert model(**kw, return_stream=dead)["stream"].shape[0] == 0


def test_capture_of_a_clip_alone_is_the_clip_in_its_batch_and_padding_is_skipped():
    model, cfg, sd, kw, seg, plain, whole = rig()
    index = whole["stream_index"].cpu()
    for b in range(2):
        one, n = clip_alone(kw, b, frames=FRAMES)
        alone = model(**one, return_stream=torch.ones_like(one["attention_mask"]))
        own = index[:, 0] == b
        assert same(alone["stream"], whole["stream"][own.cuda()]), b
        assert torch.equal(alone["stream_index"].cpu()[:, 1], index[own][:, 1]) and not alone["stream_index"][:, 0].any()
    # a ragged batch (two frames and one frame): the shorter clip's padding is not captured, nor either clip's dead tail
    ragged, _ = two_clips(cfg, 302, frames=(2, 1))
    lens = ragged["attention_mask"].sum(1).tolist()
    assert lens[1] < lens[0] == 215
    out = model(**ragged, return_stream=torch.ones_like(ragged["attention_mask"]), stream_depths=(0, 1))
    got = out["stream_index"].cpu()
    want = torch.cat([torch.stack([torch.full((n - 1,), b), torch.arange(n - 1)], 1) for b, n in enumerate(lens)])
    assert torch.equal(got, want) and out["stream"].shape[0] == sum(lens) - 2


# ---- (c) the patch identities -------------------------------------------------------------------------------------------------------------
def test_self_patch_changes_no_output():
    model, cfg, sd, kw, seg, plain, whole = rig()
    every = torch.ones_like(kw["attention_mask"])
    for mask, depths in ((every, (0, LAYERS)), (seg["frames"], (1, 3)), (seg["score_row"], (3, 4)), (seg["text_after"] | seg["motion"], (0, 1))):
        cap = model(**kw, return_stream=mask, stream_depths=depths)
        for values, idx in ((cap["stream"], cap["stream_index"]), (cap["stream"].cpu(), None)):      # on the device with the index, on the host without
            out = model(**kw, **READS, stream_patch=StreamPatch(mask, values, depths, idx))
            assert_same_outputs(out, plain)
    # an empty window and an empty selection: the plain pass
    H = cfg.llm_config.hidden_size
    for patch in (StreamPatch(every, torch.zeros(428, 0, H, dtype=BF), (2, 2)), StreamPatch(torch.zeros_like(every), torch.zeros(0, 2, H, dtype=BF), (1, 3))):
        assert_same_outputs(model(**kw, **READS, stream_patch=patch), plain)


def test_transplant_of_every_row_turns_the_recipient_into_the_donor_from_that_depth_on():
    model, cfg, sd, kw, seg, plain, whole = rig()
    N = kw["input_ids"].shape[1]
    every = torch.ones_like(kw["attention_mask"])
    donor_rows, donor_index = rows_of(whole, only_clip(every, 0))
    recipient = only_clip(every, 1)
    want = (kw["labels"][:, 1:] != -100)
    assert torch.equal(want[0], want[1])                                                      # the answer rows sit at the same positions
    per_clip = lambda t: t.view(2, N - 1, *t.shape[1:])
    assert not same(plain["score1"][0:1], plain["score1"][1:2])
    for d in range(LAYERS):
        out = model(**kw, **READS, stream_patch=StreamPatch(recipient, donor_rows[:, d:d + 1].contiguous(), (d, d + 1)))
        for key in LENS_HIDDEN:
            assert same(out[key][1, :d], plain[key][1, :d]), (d, key)                          # below d: its own
            assert same(out[key][1, d:], plain[key][0, d:]), (d, key)                          # from d on: the donor's
            assert same(out[key][0], plain[key][0]), (d, key)
        assert same(out["lens_score"][1, d:], plain["lens_score"][0, d:]) and same(out["lens_token"][1, d:], plain["lens_token"][0, d:])
        assert same(out["score1"][1:], plain["score1"][:1]) and same(out["score1"][:1], plain["score1"][:1]), d
        for key in ("logit", "cand_logprob"):
            assert same(per_clip(out[key])[1], per_clip(plain[key])[0]) and same(per_clip(out[key])[0], per_clip(plain[key])[0]), (d, key)
        assert same(per_clip(out["logprob"])[0], per_clip(plain["logprob"])[0])                # clip 0 is unchanged


def test_depth_0_patch_of_text_rows_is_the_pass_on_the_donors_ids():
    model, cfg, sd, kw, seg, plain, whole = rig()
    ids = kw["input_ids"]
    differ = (ids[0] != ids[1]) & kw["attention_mask"][0]
    assert differ.any() and not (differ & (ids[0] == model.img_context_token_id)).any()       # text positions only
    mask0, mask1 = torch.zeros_like(kw["attention_mask"]), torch.zeros_like(kw["attention_mask"])
    mask0[0], mask1[1] = differ, differ
    donor_rows, _ = rows_of(whole, mask0)
    assert donor_rows.shape[0] > 0
    out = model(**kw, **READS, stream_patch=StreamPatch(mask1, donor_rows[:, :1].contiguous(), (0, 1)))
    swapped = ids.clone()
    swapped[1, differ] = ids[0, differ]
    assert_same_outputs(out, model(**dict(kw, input_ids=swapped), **READS))
    assert not same(out["lens_score_hidden"][1], plain["lens_score_hidden"][1])


def test_capture_in_a_patched_pass_reads_the_patch_and_the_past_is_untouched():
    model, cfg, sd, kw, seg, plain, whole = rig()
    H = cfg.llm_config.hidden_size
    g = torch.Generator().manual_seed(11)
    # the score rows of both clips replaced by random rows in front of layers 1 and 2; the capture of the same pass returns them at those depths
    values = torch.randn(2, 2, H, generator=g).to(BF)
    out = model(**kw, **READS, return_stream=seg["score_row"], stream_patch=StreamPatch(seg["score_row"], values, (1, 3)))
    assert same(out["stream"][:, 1:3], values.cuda()) and same(out["stream"][:, 0], plain["lens_score_hidden"][:, 0])
    assert same(out["lens_score_hidden"][:, 1:3], values.cuda()) and not same(out["score1"], plain["score1"])
    # causality: patching the tokens at positions >= p leaves the stream of the tokens in front of p as it was, at every depth
    p = 120
    behind = kw["attention_mask"] & (torch.arange(kw["input_ids"].shape[1]) >= p)
    front = kw["attention_mask"] & ~behind
    n = int(model(**kw, return_stream=behind, stream_depths=(0, 0))["stream_index"].shape[0])
    noise = torch.randn(n, LAYERS, H, generator=g).to(BF)
    out = model(**kw, return_stream=front, stream_patch=StreamPatch(behind, noise, (0, LAYERS)))
    assert same(out["stream"], rows_of(whole, front)[0]) and not same(out["score1"], plain["score1"])


# ---- (d) against the composed oracle ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_clips():
    """Every clip alone in bf16: (the clip's inputs, the oracle's keyword inputs, its plain composed states, the clip's own segment masks)."""
    model, cfg, sd, kw, seg, plain, whole = rig()
    clips = []
    for b in range(2):
        one, n = clip_alone(kw, b, frames=FRAMES)
        inputs = dict({k: v for k, v in one.items() if k != "labels"}, img_context_token_id=model.img_context_token_id)
        clips.append((one, inputs, SP.composed_states(sd, cfg, **inputs), {k: v[b:b + 1, :n] for k, v in seg.items()}))
    return clips


ORACLE_CASES = (("score_row", (1, 2)), ("score_row", (2, 3)), ("score_row", (3, 4)), ("text_after", (1, 3)))


@pytest.mark.parametrize("group,depths", ORACLE_CASES, ids=[f"{g}-{lo}-{hi}" for g, (lo, hi) in ORACLE_CASES])
def test_patched_pass_against_the_composed_oracle(group, depths):
    """Clip 0 the donor, clip 1 the recipient, each alone.  The oracle patches its own donor rows into its own recipient pass; the GPU pass does
    the same with the rows it captured itself (end to end), and once more with the oracle's donor rows handed to it from the host (the same
    assignment on both sides).  score1 within the tiny rig's bar (1e-3 or 1 bf16 ulp of the oracle's value - tests/test_stream_patch_cpu.py shows
    that the three score-row cases move the oracle's score by at least 2 ulps), the answer tokens identical up to rows the oracle itself decides
    within 2 bf16 ulps."""
    model, cfg, sd, kw, seg, plain, whole = rig()
    (d_one, _, donor, _), (one, inputs, own, one_seg) = oracle_clips()
    am, mask, (lo, hi) = one["attention_mask"], one_seg[group].clone(), depths
    mask[:, am.shape[1] - 1:] = False                                                         # (the closing token is not run: the dead tail)
    values, index = SP.capture(donor, mask, am, depths)
    states = SP.composed_states(sd, cfg, **inputs, patches=[(mask, values, depths)])
    ref = SP.lens(sd, cfg, states, am, one["labels"], 2)
    w, eps = sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps
    logits = O.lm_logits(sd, O.rms_norm_cast_then_scale(states[LAYERS], w, eps))[0, :-1]
    want = one["labels"][0, 1:] != -100
    cap = model(**d_one, return_stream=mask, stream_depths=depths)
    assert torch.equal(cap["stream_index"].cpu(), index)
    for what, patch in (("end to end", StreamPatch(mask, cap["stream"], depths, cap["stream_index"])), ("the oracle's rows", StreamPatch(mask, values, depths, index))):
        out = model(**one, stream_patch=patch)
        print(f"{group} over [{lo}, {hi}), {what}: plain recipient {plain['score1'][1].item():.5f}, donor {plain['score1'][0].item():.5f}")
        score_ok(out["score1"], ref["score"][:, LAYERS])
        ties = assert_levels(out["logit"].cpu()[want], logits[want].argmax(-1), logits[want])
        assert ties <= max(1, int(want.sum()) // 10)
    if group == "score_row":
        assert not same(out["score1"], plain["score1"][1:2])                                  # the patch moved the score


# ---- (e) combinations ----------------------------------------------------------------------------------------------------------------
def test_with_a_knockout_the_lens_in_front_of_both_windows_keeps_the_plain_bits():
    model, cfg, sd, kw, seg, plain, whole = rig()
    donor_rows, _ = rows_of(whole, only_clip(seg["score_row"], 0))
    patch = StreamPatch(only_clip(seg["score_row"], 1), donor_rows[:, 3:4].contiguous(), (3, 4))
    knock = dict(key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(2, 4))
    out = model(**kw, **READS, **knock, stream_patch=patch)
    knocked = model(**kw, **READS, **knock)
    for key in LENS_HIDDEN + ("lens_score",):
        assert same(out[key][:, :3], plain[key][:, :3]), key                                  # layers 0 and 1 ran as they always do; depth 2 feeds the first armed layer
        assert same(out[key][0], knocked[key][0]), key                                        # clip 0 carries the knock-out only
    assert same(out["lens_score_hidden"][1, 3], plain["lens_score_hidden"][0, 3])             # the patched row, as layer 3 consumes it
    assert not same(out["lens_score_hidden"][1, 3], knocked["lens_score_hidden"][1, 3]) and not same(knocked["lens_score_hidden"][:, 3], plain["lens_score_hidden"][:, 3])
    assert same(out["lens_score"][:, LAYERS].to(BF), out["score1"])


def test_fp8_mode_self_patch_is_bit_neutral():
    model, cfg, sd, kw, seg, plain, whole = rig()
    model.set_precision("fp8")
    try:
        plain8 = model(**kw, **READS)
        cap = model(**kw, return_stream=seg["frames"] | seg["score_row"], stream_depths=(1, 4))
        out = model(**kw, **READS, stream_patch=StreamPatch(seg["frames"] | seg["score_row"], cap["stream"], (1, 4), cap["stream_index"]))
        assert_same_outputs(out, plain8)
        assert not same(plain8["lens_score_hidden"], plain["lens_score_hidden"])              # another arithmetic from layer 0 on
    finally:
        model.set_precision("bf16")
    assert_same_outputs(model(**kw, **READS), plain)


def test_graph_replay_runs_armed_calls_eagerly():
    model, cfg, sd, kw, seg, plain, whole = rig()
    donor_rows, _ = rows_of(whole, only_clip(seg["score_row"], 0))
    armed_kw = dict(return_stream=seg["text_after"], stream_depths=(1, 3),
                    stream_patch=StreamPatch(only_clip(seg["score_row"], 1), donor_rows[:, 2:3].contiguous(), (2, 3)))
    eager = model(**kw, **READS, **armed_kw)
    assert not same(eager["score1"], plain["score1"])
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    model.enable_graph_replay(True)
    try:
        graphs = lambda: sum(isinstance(v, tuple) for v in model._graphs.values())
        outs = [model(**dev_kw, **READS) for _ in range(3)]                                   # eager, capture, replay
        assert graphs() == 1 and len(model._graphs) == 1
        armed = [model(**dev_kw, **READS, **armed_kw) for _ in range(2)]
        only_capture = model(**dev_kw, **READS, return_stream=seg["text_after"], stream_depths=(1, 3))
        assert graphs() == 1 and len(model._graphs) == 1                                       # nothing captured, nothing even remembered
        again = model(**dev_kw, **READS)                                                      # replays; the armed passes before it disarmed
        assert graphs() == 1 and len(model._graphs) == 1
        torch.cuda.synchronize()
        for o in outs + [again]:
            assert_same_outputs(o, plain)
        for o in armed:
            assert_same_outputs(o, eager)
        assert_same_outputs(only_capture, plain, skip=("stream", "stream_index"))
        assert same(only_capture["stream"], rows_of(whole, seg["text_after"])[0][:, 1:3])
    finally:
        model.enable_graph_replay(False)
    assert_same_outputs(model(**kw, **READS), plain)


# ---- (f) causal_trace ---------------------------------------------------------------------------------------------------------------------
def test_causal_trace_on_the_rig():
    model, cfg, sd, kw, seg, plain, whole = rig()
    swap = torch.tensor([1, 0])
    frames = torch.tensor([2, 3, 0, 1])
    corrupt = dict(kw, input_ids=kw["input_ids"][swap], labels=kw["labels"][swap], pixel_values=kw["pixel_values"][frames], motion_feature=kw["motion_feature"][swap])
    every = kw["attention_mask"].clone()
    groups = [("all", every), ("none", torch.zeros_like(every)), ("score_row", seg["score_row"])]
    calls = []
    keep = model.vit_tokens
    model.vit_tokens = lambda pv: (calls.append(int(pv.shape[0])), keep(pv))[1]
    try:
        res = eval_utils.causal_trace(model, clean=kw, corrupt=corrupt, groups=groups, width=2, stride=2, candidate_ids=CAND)
        assert calls == [4, 4]                                                                # InternViT ran as often as in two passes
        default = eval_utils.causal_trace(model, clean=kw, corrupt=corrupt, width=LAYERS, stride=LAYERS)
    finally:
        del model.vit_tokens
    assert res["windows"] == [(0, 2), (2, 4)] and res["names"] == ["all", "none", "score_row"] and len(res["outs"]) == 2 + 3 * 2
    assert same(res["clean_score"], plain["score1"].float()) and same(res["corrupt_score"], plain["score1"].float()[swap.cuda()])
    assert tuple(res["score"].shape) == (2, 3, 2) and tuple(res["restored"].shape) == (2, 3, 2)
    assert (res["restored"][:, 0] == 1).all() and (res["restored"][:, 1] == 0).all()          # exactly
    assert torch.isfinite(res["restored"][:, 2]).all() and (res["restored"][:, 2] != 0).any()
    assert same(res["outs"][2]["cand_logprob"], res["outs"][0]["cand_logprob"])               # every row patched: every read-out is the donor's
    assert same(res["restored"], eval_utils.restored_fraction(res["score"], res["clean_score"], res["corrupt_score"]))
    assert default["names"] == ["frame0", "frame1", "motion", "text_before", "text_after", "score_row"] and default["windows"] == [(0, LAYERS)]
    assert tuple(default["score"].shape) == (2, 6, 1) and len(default["outs"]) == 2 + 6
    parts = torch.stack([m for _, m in default["groups"]]).long().sum(0)
    first = torch.zeros_like(parts); first[:, 0] = 1
    assert torch.equal(parts + first, kw["attention_mask"].long())                            # with the first token, the groups partition every clip


# ---- (g) refusals through the C ABI --------------------------------------------------------------------------------------------------------
def test_refusals_at_the_pass_come_with_a_message_and_no_fault(lib):
    model, cfg, sd, kw, seg, plain, whole = rig()
    ctx = model._ctx
    H = cfg.llm_config.hidden_size
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 4)
    T = plan["cu"][-1]
    buf = torch.zeros(4, 1, H, dtype=BF, device="cuda")
    err = lambda: lib.aigv_last_error(ctx).decode()

    def plain_again():
        torch.cuda.synchronize()
        assert_same_outputs(model(**kw, **READS), plain)

    # refused by the arm calls: nothing armed
    for arm, name in ((lib.aigv_stream_capture_arm, "aigv_stream_capture_arm"), (lib.aigv_stream_patch_arm, "aigv_stream_patch_arm")):
        for args, word in (((i32([0, 1]), -1, 0, 1, buf.data_ptr()), "-1 rows outside 0..max_tokens"), ((None, 2, 0, 1, buf.data_ptr()), "null row list"),
                           ((i32([0, 1]), 2, 0, 1, None), "null or not 16-byte aligned"), ((i32([0, 1]), 2, 0, 1, buf.data_ptr() + 8), "null or not 16-byte aligned")):
            assert arm(ctx, *args) == -1 and word in err() and err().startswith(name + ":"), (name, args, err())
    plain_again()

    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    prefill = lambda **k: model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"], **k)
    # refused by the pass, before any launch; the context disarms
    for arm, what in ((lib.aigv_stream_patch_arm, "stream patch"), (lib.aigv_stream_capture_arm, "stream capture")):
        for rows, lo, hi, word in (([0, 5, T], 0, 1, f"row 2 \\(packed row {T}\\) outside \\[0, {T}\\)"), ([0, 9, 5], 0, 1, "rows 1 and 2 \\(packed rows 9, 5\\) are not strictly ascending"),
                                   ([0, 5, 5], 0, 1, "not strictly ascending"), ([0, 5, 9], 4, 5, f"depths \\[4, 5\\) outside 0 <= lo <= hi <= {LAYERS}"),
                                   ([0, 5, 9], 2, 1, "depths \\[2, 1\\) outside")):
            assert arm(ctx, i32(rows), 3, lo, hi, buf.data_ptr()) == 0
            with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: the {what} .*" + word):
                prefill()
            plain_again()
        assert arm(ctx, i32([0, 5, 9]), 3, 0, 1, buf.data_ptr()) == 0
        with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: keep_kv while a {what} is armed"):
            prefill(keep_kv=True, kv_cap=256)
        plain_again()

    # aigv_llm_extend while armed (the shared-prefix path arms nothing itself: arm by hand behind its prefill)
    base = synth.canonical_tokens(cfg, 2, 2, seed=77)
    pp = synth.perspective_prompts(base, 2, seed=77)
    common = dict(pixel_values=synth.synthetic_frames(4, 224, seed=77), image_flags=torch.ones(4, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(2, cfg.motion_dim, seed=77))
    keep = model._prefill
    for arm, what in ((lib.aigv_stream_patch_arm, "patch"), (lib.aigv_stream_capture_arm, "capture")):
        def prefill_then_arm(*a, **k):
            out = keep(*a, **k)
            assert arm(model._ctx, i32([0, 5, 9]), 3, 0, 1, buf.data_ptr()) == 0
            return out

        model._prefill = prefill_then_arm
        try:
            with pytest.raises(native.NativeError, match=f"aigv_llm_extend: a stream {what} is armed"):
                model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common)
        finally:
            del model._prefill
        plain_again()                                                                         # the refused continuation disarmed too
    with pytest.raises(TypeError):
        model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_stream=seg["frames"])
