"""Key-drop by query row and layer window without a GPU: the ABI entries, the row patterns and their words, model.segment_masks, every
host-side refusal of forward(key_drop_rows=..., key_drop_layers=...), generate* and forward_shared_prefix, the op's host refusals, and the
model-level reference of tests/test_gpu_key_drop_rows.py pinned to the existing oracle - composed layer by layer from the oracle's own
functions, it equals oracle.forward_eval bit for bit wherever the two describe the same computation, and on the rig the two knock-outs the
GPU file compares move the oracle's own result by more than that file's bar."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import key_drop_reference as R
import key_drop_rows_reference as RR
from test_key_drop_cpu import bf16_ulps, naive_words, two_clips

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, prompts, readouts, synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = 4


# ---- the ABI entries ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_two_entries():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I = ctypes.c_void_p, ctypes.c_int
    drop = native.PROTOTYPES["aigv_op_attention_drop"]
    for name, proto in (("aigv_key_drop_arm_ex", (I, [P, P, P, I, I, I])), ("aigv_op_attention_drop_rows", (drop[0], drop[1][:-2] + [P, I, P]))):
        assert name in note and re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == proto, name
    src = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert "const uint64_t* drop_rows;" in src and "struct AttnArgsKeyDrop : AttnArgsUnmasked" in src and "struct AttnArgs : AttnArgsKeyDrop" in src


def test_op_refusals_without_a_gpu():
    """The refusals of the row selector come before any HIP call: AIGV_ERR_ARG and a message naming the op (fake, aligned, non-null
    addresses: nothing is dereferenced)."""
    lib = native.load()
    D, h, n = 128, 2, 215
    ld = 4 * D
    P = 0x10000

    def call(head_dim=D, causal=1, key_drop=P, row_words=P, ld_drop=4, kv_seq_stride=0, kv_off=None):
        rc = lib.aigv_op_attention_drop_rows(P, ld, P, ld, P, ld, P, h * D, P, 1, n, h, h, 2 * D, 2 * D, kv_seq_stride, kv_off, head_dim, causal, 11.3, 1.0, None,
                                             None, None, 0, 0, key_drop, row_words, ld_drop, None)
        return rc, (lib.aigv_last_error(None) or b"").decode()

    for kw, word in ((dict(causal=0), "causal head_dim 128"), (dict(head_dim=64), "causal head_dim 128"), (dict(ld_drop=3), "ld_drop"),
                     (dict(key_drop=None), "row_words qualify a key_drop mask"), (dict(row_words=P + 4), "drop_rows must be 8-byte aligned"),
                     (dict(key_drop=P + 4), "key_drop must be 8-byte aligned"), (dict(kv_seq_stride=4096), "packed prefill only"),
                     (dict(kv_seq_stride=4096, kv_off=P), "packed prefill only")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and msg.startswith("aigv_op_attention_drop_rows:"), (kw, rc, msg)
    assert lib.aigv_key_drop_arm_ex(None, P, P, 4, 0, 1) == -1 and "null context" in lib.aigv_last_error(None).decode()


# ---- the row patterns and their words --------------------------------------------------------------------------------------------------
def test_the_row_patterns_are_the_ones_the_issue_names():
    case = R.packed_case(1)
    assert case.cnts == [215, 144, 64, 1] and RR.ROW_PATTERNS == ("none", "all", "one", "wave", "group", "odd", "last") and RR.KEY_PATTERNS == "abcdf"
    nz = lambda p, s=0: np.nonzero(RR.row_sets(case, p)[s])[0].tolist()
    assert not any(m.any() for m in RR.row_sets(case, "none")) and all(m.all() for m in RR.row_sets(case, "all"))
    assert nz("one") == [211] and nz("one", 1) == [140] and nz("one", 2) == [60] and nz("one", 3) == []
    assert nz("wave") == list(range(20, 41)) and nz("group") == list(range(120, 137)) and nz("group", 2) == []
    assert nz("odd") == list(range(1, 215, 2))
    assert nz("last") == list(range(192, 215)) and nz("last", 1) == list(range(128, 144)) and nz("last", 2) == list(range(32, 64)) and nz("last", 3) == [0]


def test_row_words_against_a_naive_loop():
    case = R.packed_case(1)
    lens, W = case.cnts, R.words_needed(case)
    cu = [0] + list(np.cumsum(lens))
    for pat in RR.ROW_PATTERNS:
        rows = RR.row_sets(case, pat)
        sel = torch.zeros(len(lens), max(lens), dtype=torch.bool)
        for b, m in enumerate(rows):
            sel[b, :len(m)] = torch.from_numpy(m)
        want = naive_words(sel, lens, W)
        assert torch.equal(R.drop_words(rows, W), want), pat                         # what the op-level tests upload
        assert torch.equal(prompts.key_drop_words(sel, cu), want), pat               # what forward(key_drop_rows=...) uploads


def test_census_visibility():
    """The (rows, keys) census: all rows = key_drop_reference.census; no rows, or no keys = the unmasked census; a row that is not selected
    counts the dropped keys it may see."""
    case = R.packed_case(3)
    drops = R.drop_sets(case, "b")
    every, none = RR.row_sets(case, "all"), RR.row_sets(case, "none")
    assert torch.equal(RR.census(case, drops, every).expect, R.census(case, drops).expect)
    assert torch.equal(RR.census(case, drops, none).expect, case.census().expect)
    assert torch.equal(RR.census(case, R.drop_sets(case, "f"), every).expect, case.census().expect)
    odd = RR.row_sets(case, "odd")
    vis = RR.visible_sets(case, 0, drops[0], odd[0])
    assert vis[100].sum() == 101 and vis[101].sum() == 102 - (101 - 45 + 1) and vis[214].sum() == 215 and vis[213].sum() == 214 - 64
    mixed = RR.census(case, drops, odd).expect.view(-1, case.h, case.D)
    full, plain = R.census(case, drops).expect.view(-1, case.h, case.D), case.census().expect.view(-1, case.h, case.D)
    assert torch.equal(mixed[1:215:2], full[1:215:2]) and torch.equal(mixed[0:215:2], plain[0:215:2])


# ---- segment masks and the host refusals (a model object on the host: no GPU work) -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_rig(stage=2):
    from aigv_assessor_amd.modeling import InternVLChatModel
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=LAYERS)
    model = InternVLChatModel(cfg, stage=stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    return model, cfg, kw


@pytest.mark.parametrize("stage", [2, 1])
def test_segment_masks_partition_every_clip_and_agree_with_unit_masks(stage):
    model, cfg, kw = host_rig(stage)
    ids, am, flags = kw["input_ids"], kw["attention_mask"], kw["image_flags"]
    seg = model.segment_masks(ids, am, flags)
    assert sorted(seg) == ["first", "frames", "motion", "score_row", "text_after", "text_before"]
    assert all(v.dtype == torch.bool and v.shape == ids.shape for v in seg.values())
    parts = torch.stack([seg[k] for k in ("frames", "motion", "first", "text_before", "text_after")]).long().sum(0)
    assert torch.equal(parts, am.long())                                                      # every run token in exactly one group, padding in none
    units = model.unit_masks(ids, am, flags)
    F = units.shape[1] - 1
    assert torch.equal(seg["frames"], units[:, :F].any(1)) and torch.equal(seg["motion"], units[:, F])
    assert seg["first"][:, 0].all() and seg["first"].sum() == 2
    lens = am.sum(1)
    for b in range(2):
        last_vis = int(seg["frames"][b].nonzero().max())
        assert not seg["text_after"][b, :last_vis].any() and not seg["text_before"][b, last_vis:].any()
        if stage == 2:
            assert seg["score_row"][b].nonzero().flatten().tolist() == [int(lens[b]) - 4] and seg["text_after"][b, int(lens[b]) - 4]
    if stage == 1:
        assert not seg["score_row"].any()
    assert all(torch.equal(v, seg[k]) for k, v in model.segment_masks(ids, am, None, n_frames=3).items())
    with pytest.raises(ValueError, match="segment_masks"):
        model.segment_masks(ids, am)


def test_host_refusals_come_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError.  Every message names its option."""
    model, cfg, kw = host_rig()
    ids, am = kw["input_ids"], kw["attention_mask"]
    seg = model.segment_masks(ids, am, kw["image_flags"])
    keys, rows = seg["frames"], seg["text_after"]

    def bad(word, **opts):
        with pytest.raises(ValueError, match=word):
            model(**kw, **opts)

    bad("key_drop_rows: qualifies key_drop", key_drop_rows=rows)
    bad("key_drop_layers: qualifies key_drop", key_drop_layers=(0, 2))
    bad("key_drop_rows: shape", key_drop=keys, key_drop_rows=rows[:, :100])
    bad("key_drop_rows: expected a bool or integer tensor", key_drop=keys, key_drop_rows=rows.float())
    bad("key_drop_rows: expected a bool or integer tensor", key_drop=keys, key_drop_rows=rows[0])
    for window in ((2, 1), (-1, 2), (0, LAYERS + 1), (0,), (0, 1, 2), 2, (0.0, 2), (False, True)):
        bad("key_drop_layers", key_drop=keys, key_drop_layers=window)
    itself = rows.clone(); itself[1, 50] = True                                               # a frame token of clip 1 as a row and a key
    assert keys[1, 50]
    bad("key_drop_rows: clip 1: a token is both", key_drop=keys, key_drop_rows=itself)
    first = keys.clone(); first[0, 0] = True
    bad("key_drop: clip 0: the first token", key_drop=first, key_drop_rows=rows)
    bad("return_score_attention", key_drop=keys, key_drop_rows=rows, return_score_attention=True)
    # without key_drop_rows today's rules hold under a window: a consumed row is no key
    bad("consumed row", key_drop=seg["score_row"], key_drop_layers=(0, 2))
    # with it, consumed rows may be keys: the words come back, padded positions are ignored, integer masks are taken
    plan = model._plan(ids, am, kw["labels"], kw["image_flags"], 3)
    answer_keys = seg["text_after"] & ~seg["score_row"]
    w_keys, w_rows = model._key_drop_words(plan, answer_keys, seg["score_row"])
    assert torch.equal(w_keys, prompts.key_drop_words(answer_keys, plan["cu"], plan["row_of"]))
    assert torch.equal(w_rows, prompts.key_drop_words(seg["score_row"], plan["cu"], plan["row_of"])) and w_rows.shape == w_keys.shape == (2, 4)
    padded = rows.long(); padded[1, 200] = 1
    got_rows, got_window = readouts.key_drop_qualifiers(keys, padded, [1, 3], ids.shape, LAYERS)
    assert got_window == (1, 3) and torch.equal(model._key_drop_words(plan, keys, got_rows)[1], prompts.key_drop_words(rows, plan["cu"], plan["row_of"]))
    assert readouts.key_drop_qualifiers(keys, None, (2, 2), ids.shape, LAYERS) == (None, (2, 2))
    # the options travel through the record as key_drop does
    ro = readouts.ReadOuts.parse(cfg.llm_config.vocab_size, kw["labels"], key_drop=keys, ids_shape=ids.shape, key_drop_rows=rows, key_drop_layers=(0, 2),
                                 n_layers=LAYERS)
    fk = readouts.forward_kwargs(ro)
    assert torch.equal(fk["key_drop_rows"], rows) and fk["key_drop_layers"] == (0, 2) and torch.equal(fk["key_drop"], keys)
    assert not {"key_drop", "key_drop_rows", "key_drop_layers"} & set(readouts.forward_kwargs(readouts.ReadOuts(logprobs=True)))


def test_generate_and_shared_prefix_refuse_the_qualifiers():
    model, cfg, kw = host_rig()
    ids, am, flags = kw["input_ids"], kw["attention_mask"], kw["image_flags"]
    seg = model.segment_masks(ids, am, flags)
    for opts, word in ((dict(key_drop_rows=seg["text_after"]), "key_drop_rows"), (dict(key_drop_layers=(0, 2)), "key_drop_layers")):
        with pytest.raises(ValueError, match=word + ": generate"):
            model.generate_stage2(kw["pixel_values"], ids, am, flags, kw["motion_feature"], key_drop=seg["frames"], max_new_tokens=2, **opts)
        with pytest.raises(ValueError, match=word + ": generate"):
            model.generate(kw["pixel_values"], ids, am, key_drop=seg["frames"], max_new_tokens=2, **opts)
        with pytest.raises(ValueError, match=word + ": forward_shared_prefix"):
            model.forward_shared_prefix([(ids, am, kw["labels"])], pixel_values=kw["pixel_values"], image_flags=flags, motion_feature=kw["motion_feature"], **opts)
    with pytest.raises(ValueError, match="flow_knockout: width"):
        eval_utils.flow_knockout(model, **{k: v for k, v in kw.items() if k != "motion_feature"}, width=LAYERS + 1)


# ---- the composed reference, pinned to the existing oracle --------------------------------------------------------------------------------
def one_clip(kw, b, frames=(2, 1)):
    f0 = sum(frames[:b])
    n = int(kw["attention_mask"][b].sum())
    return dict(pixel_values=kw["pixel_values"][f0:f0 + frames[b]], input_ids=kw["input_ids"][b:b + 1, :n], attention_mask=kw["attention_mask"][b:b + 1, :n],
                image_flags=kw["image_flags"][f0:f0 + frames[b]], labels=kw["labels"][b:b + 1, :n], motion_feature=kw["motion_feature"][b:b + 1]), n


def knockouts(seg, b=None, n=None):
    """The two knock-outs the GPU file compares against the composed oracle: (name, keys, rows, window) - the masks of clip b alone, cut to its
    n tokens, or (b None) of the whole batch."""
    cut = (lambda m: m) if b is None else (lambda m: m[b:b + 1, :n])
    ctx = cut(seg["frames"] | seg["motion"])
    return (("text after <- IMG_CONTEXT, layers [0, 2)", ctx, cut(seg["text_after"]), (0, 2)), ("all rows <- IMG_CONTEXT, layer [0, 1)", ctx, None, (0, 1)))


@pytest.mark.parametrize("stage", [2, 1])
def test_composed_reference_is_the_oracle_where_the_two_coincide(stage):
    """All rows, all layers = oracle.forward_eval(attention_mask & ~drop), bit for bit; empty keys, empty rows or an empty window = the plain
    forward_eval, bit for bit."""
    model, cfg, kw = host_rig(stage)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    for b in range(2):
        one, n = one_clip(kw, b)
        common = dict(img_context_token_id=model.img_context_token_id, stage=stage)
        drop = seg["frames"][b:b + 1, :n]
        am = one["attention_mask"]

        def same(got, ref):
            assert torch.equal(got["logit"], ref["logit"]) and torch.equal(got["logits"], ref["logits"]) and torch.equal(got["label"], ref["label"])
            if stage == 2:
                assert torch.equal(got["score1"].view(torch.int16), ref["score1"].view(torch.int16))

        masked = O.forward_eval(sd, cfg, **dict(one, attention_mask=am & ~drop), **common, return_intermediates=True)
        plain = O.forward_eval(sd, cfg, **one, **common, return_intermediates=True)
        assert not torch.equal(masked["logits"], plain["logits"])
        same(RR.composed_forward(sd, cfg, **one, **common, drop=drop, rows=None, window=None), masked)
        same(RR.composed_forward(sd, cfg, **one, **common, drop=drop, rows=torch.ones_like(drop), window=(0, LAYERS)), masked)
        same(RR.composed_forward(sd, cfg, **one, **common), plain)
        same(RR.composed_forward(sd, cfg, **one, **common, drop=torch.zeros_like(drop), rows=seg["text_after"][b:b + 1, :n], window=(0, LAYERS)), plain)
        same(RR.composed_forward(sd, cfg, **one, **common, drop=drop, rows=torch.zeros_like(drop), window=(0, LAYERS)), plain)
        same(RR.composed_forward(sd, cfg, **one, **common, drop=drop, rows=None, window=(2, 2)), plain)


@pytest.mark.parametrize("stage", [2, 1])
def test_oracle_condition_the_two_knockouts_move_the_oracle(stage):
    """Per stage and knock-out, over the two clips: the score moves by >= 3 bf16 ulps or >= 2 answer-row argmaxes move - more than the GPU
    file's bar, so a device pass that ignored the rows or the window could not pass its comparison.  Measured (stage 2, clip 0, 215 tokens):
    0.48047 -> 0.48828 = 4 ulps with 3 of 10 rows (text after <- IMG_CONTEXT, [0, 2)) and 7 of 10 rows (all rows, [0, 1))."""
    model, cfg, kw = host_rig(stage)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    ulps, moved = {}, {}
    for b in range(2):
        one, n = one_clip(kw, b)
        common = dict(img_context_token_id=model.img_context_token_id, stage=stage)
        base = RR.composed_forward(sd, cfg, **one, **common)
        want = base["label"] != -100
        for name, keys, rows, window in knockouts(seg, b, n):
            o = RR.composed_forward(sd, cfg, **one, **common, drop=keys, rows=rows, window=window)
            moved[name] = moved.get(name, 0) + int((o["logit"][want] != base["logit"][want]).sum())
            if stage == 2:
                assert torch.isfinite(o["score1"].float()).all()
                ulps[name] = max(ulps.get(name, 0.0), bf16_ulps(float(o["score1"][0]), float(base["score1"][0])))
            print(f"stage {stage} clip {b} {name}: answer rows moved so far {moved[name]}, score ulps so far {ulps.get(name)}")
    for name in moved:
        assert ulps.get(name, 0.0) >= 3 or moved[name] >= 2, (name, ulps.get(name), moved[name])
    if stage == 2:
        assert int(seg["frames"][0].sum() + seg["motion"][0].sum()) == 129 and int(kw["attention_mask"][0].sum()) == 215
        assert min(ulps.values()) >= 3
