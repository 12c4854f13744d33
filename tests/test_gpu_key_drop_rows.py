"""Key-drop by query row and layer window on the MI355X: the row-selective form of the prefill flash kernel (AttnArgs::drop_rows) at op level
through aigv_op_attention_drop_rows - bit-exact on the (rows, keys) key census of tests/key_drop_rows_reference.py over every row pattern x
key pattern, both score numerics, both wave counts, with row trimming; the identities with aigv_op_attention_drop and the unmasked op; random
data against float64 under the project's own bar; fencing; the refusals - and at model level on the tiny rig with four layers:
forward(key_drop=, key_drop_rows=, key_drop_layers=) against the oracle composed layer by layer, the bit identities, a window alone, a clip
alone, graph replay, eval_utils.flow_knockout and the refusals of generate* / forward_shared_prefix.

The bars are those of tests/test_gpu_key_drop.py (score: 1e-3 or 1 bf16 ulp; level tokens identical up to the oracle's own 2-ulp ties).
tests/test_key_drop_rows_cpu.py holds, without a GPU, the conditions the comparison rests on."""
import functools

import numpy as np
import pytest
import torch

import key_drop_reference as R
import key_drop_rows_reference as RR
from attention_exact_reference import BF
from attention_reference import check_sequence, rope_table
from test_gpu_key_drop import (AIGV_ERR_ARG, D, N_POS, PAD, SENTINEL, Staged, _KEEP, _release_device_tensors, assert_bits, assert_levels, bits, clip_alone,  # noqa: F401
                               dev, expect_whole, lib, make_model, pattern, same, score_ok, sync, tables, tuned, two_clips)     # (the fixtures are used by name)
from test_key_drop_rows_cpu import LAYERS, knockouts

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth

pytestmark = pytest.mark.gpu


def attend_rows(lib, st, key_words, row_words, round_scores, q_tail=0):
    """-> the WHOLE output allocation [PAD + T + PAD, h * D]; both word buffers hold exactly n_seq * ld_drop words (row_words None: NULL)."""
    out = pattern((st.T + 2 * PAD, st.case.h * D), SENTINEL)
    a = st.args(out, round_scores, q_tail)
    kw = dev(key_words)
    rw = None if row_words is None else dev(row_words)
    assert kw.numel() == len(st.case.cnts) * key_words.shape[1] and (rw is None or rw.shape == kw.shape)
    sync(lib.aigv_op_attention_drop_rows(*a, kw.data_ptr(), native.ptr(rw), key_words.shape[1], None))
    return out


# =================================================================================================================================
# op level
# =================================================================================================================================
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_row_and_key_census_is_exact(lib, g):
    """1.  Every row pattern (none, all, one row, across a wave border, across a workgroup border, every other row, the ragged last wave) x the
    key patterns a, b, c, d, f: every visible key counted once, and a dropped key counted by exactly the rows that are not selected.  One wrong
    visibility bit changes a count and the divisor.  Both score numerics, 4 and 8 waves, q_tail 0 and 4."""
    case = R.packed_case(g)
    ld = R.words_needed(case)
    rope = tables("census")
    try:
        for kp in RR.KEY_PATTERNS:
            drops = R.drop_sets(case, kp)
            key_words = R.drop_words(drops, ld)
            st = None
            for rp in RR.ROW_PATTERNS:
                rows = RR.row_sets(case, rp)
                data = RR.census(case, drops, rows)
                if st is None:                                               # (the inputs depend on the keys only: staged once per key pattern)
                    st = Staged(case, data, rope)
                    staged = len(_KEEP)
                row_words = R.drop_words(rows, ld)
                for knob in (0, 8):
                    tuned(lib, knob)
                    for rs in (True, False):
                        for q_tail in R.Q_TAILS:
                            want = expect_whole(data.expect, R.waves_written(case.cnts, q_tail))
                            assert_bits(attend_rows(lib, st, key_words, row_words, rs, q_tail), want, case,
                                        f"rows {rp} keys {kp} knob {knob} round_scores {rs} q_tail {q_tail}")
                del _KEEP[staged:]                                           # (keep the staged case, drop the outputs and words)
            _KEEP.clear()
    finally:
        tuned(lib, 0)


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_identities_with_the_key_drop_and_the_unmasked_op(lib, g):
    """2.  All-ones row words (every bit, also those past a sequence's end) = aigv_op_attention_drop; a NULL selector likewise; all-zero row
    words or all-zero key words = aigv_op_attention_ex: bit for bit, whole allocation, random data."""
    case = R.packed_case(g)
    data = R.random_case(case)
    st = Staged(case, data, rope_table(D, N_POS))
    ld = R.words_needed(case)
    ones, zeros = torch.full((len(case.cnts), ld), -1, dtype=torch.int64), torch.zeros(len(case.cnts), ld, dtype=torch.int64)
    odd = R.drop_words(RR.row_sets(case, "odd"), ld)
    staged = len(_KEEP)
    try:
        for knob in (0, 8):
            tuned(lib, knob)
            for rs in (True, False):
                for q_tail in R.Q_TAILS:
                    plain = st.attend(lib, None, rs, q_tail, plain=True).view(torch.int16)
                    for kp in "bc":
                        words = R.drop_words(R.drop_sets(case, kp), ld)
                        masked = st.attend(lib, words, rs, q_tail).view(torch.int16)
                        assert not torch.equal(masked, plain)
                        assert torch.equal(attend_rows(lib, st, words, ones, rs, q_tail).view(torch.int16), masked), (knob, rs, q_tail, kp, "all-ones rows")
                        assert torch.equal(attend_rows(lib, st, words, None, rs, q_tail).view(torch.int16), masked), (knob, rs, q_tail, kp, "NULL rows")
                        assert torch.equal(attend_rows(lib, st, words, zeros, rs, q_tail).view(torch.int16), plain), (knob, rs, q_tail, kp, "all-zero rows")
                    assert torch.equal(attend_rows(lib, st, zeros, odd, rs, q_tail).view(torch.int16), plain), (knob, rs, q_tail, "all-zero keys")
                    assert torch.equal(attend_rows(lib, st, zeros, ones, rs, q_tail).view(torch.int16), plain), (knob, rs, q_tail, "all-zero keys, all rows")
                del _KEEP[staged:]
    finally:
        tuned(lib, 0)


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_random_data_against_float64_under_the_projects_bar(lib, g):
    """3.  attention_reference.check_sequence per sequence for three row x key combinations: at least as accurate against the float64 softmax
    under the (rows, keys) visibility as the eager bf16 restatement of the reference's additive mask."""
    case = R.packed_case(g)
    data = R.random_case(case)
    st = Staged(case, data, None)                                             # (no rotation: q and k are used as stored on both sides)
    ld = R.words_needed(case)
    try:
        for rp, kp in (("wave", "b"), ("odd", "c"), ("last", "a")):
            drops, rows = R.drop_sets(case, kp), RR.row_sets(case, rp)
            refs = [(RR.masked_attention(data.q[s], data.k[s], data.v[s], drops[s], rows[s], R.POST, torch.float64),
                     RR.masked_attention(data.q[s], data.k[s], data.v[s], drops[s], rows[s], R.POST, BF).double()) for s in range(len(case.cnts))]
            for knob in (0, 8):
                tuned(lib, knob)
                for rs in (True, False):
                    out = attend_rows(lib, st, R.drop_words(drops, ld), R.drop_words(rows, ld), rs)
                    whole = out.cpu().view(torch.int16)
                    assert (whole[:PAD] == SENTINEL).all() and (whole[PAD + st.T:] == SENTINEL).all()
                    got = out[PAD:PAD + st.T].cpu().double().view(st.T, case.h, D)
                    row = 0
                    for s, n in enumerate(case.cnts):
                        check_sequence(got[row:row + n], *refs[s])
                        row += n
    finally:
        tuned(lib, 0)


def test_op_fences(lib):
    """4.  Both word buffers are exactly n_seq * ld_drop words at the SMALLEST ld_drop the check admits, K / V beyond every sequence is NaN and
    nothing of it shows; the output sits between sentinel pads and the rows of whole waves in front of q_tail stay unwritten."""
    case = R.packed_case(3)
    drops, rows = R.drop_sets(case, "d"), RR.row_sets(case, "last")
    data = RR.census(case, drops, rows)
    st = Staged(case, data, rope_table(D, N_POS))
    ld = R.words_needed(case)
    assert ld == -(-max(case.cnts) // 64)
    for q_tail in (0, 4):
        written = R.waves_written(case.cnts, q_tail)
        out = attend_rows(lib, st, R.drop_words(drops, ld), R.drop_words(rows, ld), False, q_tail)
        assert_bits(out, expect_whole(data.expect, written), case, f"fence q_tail {q_tail}")
        assert torch.isfinite(out[PAD:PAD + st.T][written.cuda()].float()).all()
        assert q_tail == 0 or (out.view(torch.int16)[PAD:PAD + st.T][~written.cuda()] == SENTINEL).all() and int((~written).sum()) == 192 + 128 + 32


def test_op_refusals_come_with_a_message_and_no_fault(lib):
    """5.  Every refusal of the row selector: AIGV_ERR_ARG and a message, nothing launched (sentinel intact); then a clean launch."""
    case = R.packed_case(1)
    drops, rows = R.drop_sets(case, "a"), RR.row_sets(case, "wave")
    data = RR.census(case, drops, rows)
    st = Staged(case, data, None)
    ld = R.words_needed(case)
    kw, rw = dev(R.drop_words(drops, ld + 1)), dev(R.drop_words(rows, ld + 1))
    out = pattern((st.T + 2 * PAD, case.h * D), SENTINEL)
    a = list(st.args(out, False, 0))
    I_KV_SEQ_STRIDE, I_KV_OFF, I_HEAD_DIM, I_CAUSAL = 15, 16, 17, 18
    off = dev(torch.zeros(len(case.cnts), dtype=torch.int32))

    def refused(args, key_drop, row_words, ld_drop, word):
        rc = lib.aigv_op_attention_drop_rows(*args, key_drop, row_words, ld_drop, None)
        msg = (lib.aigv_last_error(None) or b"").decode()
        assert rc == AIGV_ERR_ARG and word in msg and "aigv_op_attention_drop_rows" in msg, (rc, msg)

    non_causal = list(a); non_causal[I_CAUSAL] = 0
    refused(non_causal, kw.data_ptr(), rw.data_ptr(), ld + 1, "causal head_dim 128")
    d64 = list(a); d64[I_HEAD_DIM] = 64
    refused(d64, kw.data_ptr(), rw.data_ptr(), ld + 1, "causal head_dim 128")
    refused(a, kw.data_ptr(), rw.data_ptr(), ld - 1, "ld_drop")
    refused(a, kw.data_ptr(), rw.data_ptr() + 4, ld, "drop_rows must be 8-byte aligned")
    refused(a, kw.data_ptr() + 4, rw.data_ptr(), ld, "key_drop must be 8-byte aligned")
    refused(a, None, rw.data_ptr(), ld, "need one")
    cache = list(a); cache[I_KV_SEQ_STRIDE] = 4096
    refused(cache, kw.data_ptr(), rw.data_ptr(), ld + 1, "packed prefill only")
    cache[I_KV_OFF] = off.data_ptr()
    refused(cache, kw.data_ptr(), rw.data_ptr(), ld + 1, "packed prefill only")
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == SENTINEL).all()                                           # nothing was launched
    assert_bits(attend_rows(lib, st, R.drop_words(drops, ld), R.drop_words(rows, ld), False), expect_whole(data.expect), case, "after the refusals")


# =================================================================================================================================
# model level
# =================================================================================================================================
KEYS = ("score1", "logit", "logprob")


@functools.lru_cache(maxsize=None)
def rig(stage):
    """The tiny rig with four LLM layers (weights seed 61 + stage, tokens seed 300 + stage: 63 / 302 in stage 2): two clips of 2 and 1 frames,
    N = 215.  -> model, cfg, sd, kw, the segment masks, the plain pass, the pass with every frame hidden from every row in every layer."""
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=LAYERS)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    model = make_model(cfg, sd, stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    plain = model(**kw, return_logprobs=True)
    masked = model(**kw, return_logprobs=True, key_drop=seg["frames"])
    torch.cuda.synchronize()
    return model, cfg, sd, kw, seg, plain, masked


def outputs_equal(a, b, stage, what):
    for key in KEYS[0 if stage == 2 else 1:]:
        assert same(a[key], b[key]), (what, key)


def differs(a, b):
    return not same(a["logprob"], b["logprob"])


@functools.lru_cache(maxsize=None)
def oracle_ref(stage, b, which):
    """The composed oracle of clip b alone (hidden[:, -4] is then its score row): which = 'plain', 0 / 1 (the two knock-outs of
    test_key_drop_rows_cpu.knockouts) or 'window' (all rows <- the frames, layers [1, 3))."""
    model, cfg, sd, kw, seg, plain, masked = rig(stage)
    one, n = clip_alone(kw, b)
    common = dict(img_context_token_id=model.img_context_token_id, stage=stage)
    if which == "plain":
        return RR.composed_forward(sd, cfg, **one, **common)
    if which == "window":
        return RR.composed_forward(sd, cfg, **one, **common, drop=seg["frames"][b:b + 1, :n], rows=None, window=(1, 3))
    name, keys, rows, window = knockouts(seg, b, n)[which]
    return RR.composed_forward(sd, cfg, **one, **common, drop=keys, rows=rows, window=window)


def against_the_oracle(stage, out, which):
    """The batched device pass `out` against the composed oracle of every clip; -> (largest score movement of the ORACLE against its own plain
    pass in bf16 ulps, answer rows the oracle moved)."""
    model, cfg, sd, kw, seg, plain, masked = rig(stage)
    N = kw["input_ids"].shape[1]
    got_logit = out["logit"].cpu().view(2, N - 1)
    ulps, moved = 0.0, 0
    for b in range(2):
        n = int(kw["attention_mask"][b].sum())
        ref, base = oracle_ref(stage, b, which), oracle_ref(stage, b, "plain")
        want = ref["label"] != -100
        ties = assert_levels(got_logit[b, :n - 1][want], ref["logit"][want], ref["logits"][0, :-1][want])
        assert ties <= max(1, int(want.sum()) // 10)
        moved += int((ref["logit"][want] != base["logit"][want]).sum())
        if stage == 2:
            score_ok(out["score1"][b:b + 1], ref["score1"])
            a, c = float(ref["score1"][0]), float(base["score1"][0])
            ulps = max(ulps, abs(a - c) / 2.0 ** (np.floor(np.log2(abs(c))) - 7))
    return ulps, moved


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("stage", [2, 1])
def test_model_knockout_against_the_composed_oracle(stage, which):
    """6.  Rows after the last visual token <- the IMG_CONTEXT keys in layers [0, 2), and all rows <- those keys in layer [0, 1): first the
    oracle's own movement (>= 3 bf16 ulps of score or >= 2 answer rows: a pass that ignored the mask, the rows or the window could not pass),
    then the device against it, clip by clip."""
    model, cfg, sd, kw, seg, plain, masked = rig(stage)
    name, keys, rows, window = knockouts(seg)[which]
    out = model(**kw, return_logprobs=True, key_drop=keys, key_drop_rows=rows, key_drop_layers=window)
    ulps, moved = against_the_oracle(stage, out, which)
    print(f"stage {stage} {name}: the oracle moves its score by {ulps:.1f} bf16 ulps and {moved} answer rows")
    assert ulps >= 3 or moved >= 2
    assert differs(out, plain)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_bit_identities(stage):
    """7.  No qualifier, or all rows in all layers = today's key_drop call; empty rows, empty keys or an empty window = the plain pass, with
    the same set of keys in the result dict."""
    model, cfg, sd, kw, seg, plain, masked = rig(stage)
    keys = seg["frames"]
    assert differs(masked, plain)
    for what, opts in (("None, None", dict(key_drop_rows=None, key_drop_layers=None)), ("all rows, (0, L)", dict(key_drop_rows=kw["attention_mask"] & ~keys, key_drop_layers=(0, LAYERS))),
                       ("(0, L)", dict(key_drop_layers=(0, LAYERS)))):
        out = model(**kw, return_logprobs=True, key_drop=keys, **opts)
        assert set(out) == set(masked), what
        if what.startswith("all rows"):
            # (every row that is no dropped key: a frame token is cut from the frame tokens in front of it in `masked` only - the consumed rows agree)
            outputs_equal(out, masked, stage, what)
        else:
            for key in out:
                assert out[key] is None and masked[key] is None or same(out[key], masked[key]), (what, key)
    for what, opts in (("empty rows", dict(key_drop=keys, key_drop_rows=torch.zeros_like(keys))), ("empty keys", dict(key_drop=torch.zeros_like(keys), key_drop_rows=seg["text_after"])),
                       ("empty keys, window", dict(key_drop=torch.zeros_like(keys), key_drop_layers=(1, 3))), ("(2, 2)", dict(key_drop=keys, key_drop_layers=(2, 2))),
                       ("(0, 0), rows", dict(key_drop=keys, key_drop_rows=seg["text_after"], key_drop_layers=(0, 0)))):
        out = model(**kw, return_logprobs=True, **opts)
        assert set(out) == set(plain), what
        for key in out:
            assert out[key] is None and plain[key] is None or same(out[key], plain[key]), (what, key)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_a_window_alone(stage):
    """8.  key_drop_layers alone is key_drop applied in those layers only: (1, 3) with all rows agrees with the composed oracle and differs in
    bits from the plain and from the fully masked pass; two windows that tile the layers are not the full mask either way round."""
    model, cfg, sd, kw, seg, plain, masked = rig(stage)
    out = model(**kw, return_logprobs=True, key_drop=seg["frames"], key_drop_layers=(1, 3))
    against_the_oracle(stage, out, "window")
    assert differs(out, plain) and differs(out, masked)
    early = model(**kw, return_logprobs=True, key_drop=seg["frames"], key_drop_layers=(0, 1))
    assert differs(early, out) and differs(early, plain) and differs(early, masked)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_clip_alone_is_clip_in_batch_under_rows_and_window(stage):
    """9."""
    model, cfg, sd, kw, seg, plain, masked = rig(stage)
    N = kw["input_ids"].shape[1]
    opts = lambda b, n: dict(key_drop=seg["frames"][b, :n][None], key_drop_rows=seg["text_after"][b, :n][None], key_drop_layers=(1, 3))
    batch = model(**kw, return_logprobs=True, key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(1, 3))
    assert differs(batch, plain)
    for b in range(2):
        one, n = clip_alone(kw, b)
        alone = model(**one, return_logprobs=True, **opts(b, n))
        if stage == 2:
            assert torch.equal(bits(alone["score1"]), bits(batch["score1"][b:b + 1])), b
        for key in ("logit", "logprob"):
            assert torch.equal(bits(alone[key]), bits(batch[key].view(2, N - 1)[b, :n - 1])), (b, key)


def test_model_graph_replay_runs_knockout_calls_eagerly():
    """10.  With replay enabled a call with rows and a window has the eager bits and captures nothing; the plain calls around it keep
    replaying with their old bits."""
    model, cfg, sd, kw, seg, plain, masked = rig(2)
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    opts = dict(key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(0, 2))
    eager = model(**kw, return_logprobs=True, **opts)
    assert differs(eager, plain)
    model.enable_graph_replay(True)
    try:
        outs = [model(**dev_kw, return_logprobs=True) for _ in range(3)]                       # eager, capture, replay
        graphs = lambda: sum(isinstance(v, tuple) for v in model._graphs.values())
        assert graphs() == 1 and len(model._graphs) == 1
        m1 = model(**dev_kw, return_logprobs=True, **opts)
        m2 = model(**dev_kw, return_logprobs=True, **opts)
        assert graphs() == 1 and len(model._graphs) == 1                                       # nothing captured, nothing even remembered
        again = model(**dev_kw, return_logprobs=True)                                          # replays; the pass before it disarmed
        assert graphs() == 1
        torch.cuda.synchronize()
        for o in outs + [again]:
            outputs_equal(o, plain, 2, "replayed plain pass")
        for m in (m1, m2):
            outputs_equal(m, eager, 2, "knock-out under replay")
    finally:
        model.enable_graph_replay(False)
    outputs_equal(model(**kw, return_logprobs=True), plain, 2, "eager plain pass afterwards")


def test_model_flow_knockout(lib):
    """11.  Shapes; every entry is bit for bit the manual forward; window (0, L) of frames -> all rows is frame_ablation's result where the two
    coincide (clip 1 has one frame: its unit 0 is all its frames); a clip without the keys is NaN, frame_ablation's convention; the ViT ran once."""
    model, cfg, sd, kw, seg, plain, masked = rig(2)
    calls = []
    keep = model.vit_tokens

    def counted(pv):
        calls.append(tuple(pv.shape))
        return keep(pv)

    model.vit_tokens = counted
    try:
        res = eval_utils.flow_knockout(model, **kw, width=2, return_logprobs=True)
        assert len(calls) == 1 and calls[0][0] == 3
        units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
        whole = eval_utils.flow_knockout(model, **kw, paths=[("frames->all", seg["frames"], None), ("frame 1->all", units[:, 1], None)], width=LAYERS)
        assert len(calls) == 2
    finally:
        del model.vit_tokens
    torch.cuda.synchronize()
    assert [p[0] for p in res["paths"]] == ["frames->score_row", "frames->text_after", "text_after->score_row"] and res["windows"] == [(0, 2), (2, 4)]
    assert len(res["outs"]) == 1 + 3 * 2 and tuple(res["knocked"].shape) == tuple(res["delta"].shape) == (2, 3, 2) and tuple(res["score1"].shape) == (2,)
    outputs_equal(res["outs"][0], plain, 2, "base")
    assert same(res["score1"].cpu(), plain["score1"].float().cpu())
    i = 1
    for p, (name, keys, rows) in enumerate(res["paths"]):
        for w, window in enumerate(res["windows"]):
            manual = model(**kw, return_logprobs=True, key_drop=keys, key_drop_rows=rows, key_drop_layers=window)
            outputs_equal(res["outs"][i], manual, 2, (name, window))
            assert torch.equal(res["knocked"][:, p, w].cpu(), manual["score1"].float().cpu())
            i += 1
    assert torch.isfinite(res["knocked"]).all() and torch.equal(res["delta"].cpu(), plain["score1"].float().cpu()[:, None, None] - res["knocked"].cpu())
    assert torch.equal(res["paths"][2][1], seg["text_after"] & ~seg["score_row"]) and torch.equal(res["paths"][2][2], seg["score_row"])
    # (0, L) of frames -> every row against frame_ablation
    abl = eval_utils.frame_ablation(model, **kw)
    assert whole["windows"] == [(0, LAYERS)] and tuple(whole["knocked"].shape) == (2, 2, 1)
    assert same(whole["knocked"][1, 0, 0].cpu(), abl["ablated"][1, 0].cpu()) and same(whole["delta"][1, 0, 0].cpu(), abl["delta"][1, 0].cpu())
    assert same(whole["knocked"][:, 0, 0].cpu(), masked["score1"].float().cpu())
    assert same(whole["knocked"][0, 1, 0].cpu(), abl["ablated"][0, 1].cpu())                    # clip 0's frame 1: the same unit, the same pass
    k, d = whole["knocked"].cpu(), whole["delta"].cpu()
    assert torch.isnan(k[1, 1, 0]) and torch.isnan(d[1, 1, 0]) and torch.isnan(abl["ablated"][1, 1]) and torch.isfinite(k[0]).all() and torch.isfinite(k[1, 0]).all()


def test_model_generate_and_shared_prefix_refuse_and_leave_the_model_usable(lib):
    """12."""
    model, cfg, sd, kw, seg, plain, masked = rig(2)
    ids, am, flags = kw["input_ids"], kw["attention_mask"], kw["image_flags"]
    for opts, word in ((dict(key_drop_rows=seg["text_after"]), "key_drop_rows"), (dict(key_drop_layers=(0, 2)), "key_drop_layers")):
        with pytest.raises(ValueError, match=word + ": generate"):
            model.generate_stage2(kw["pixel_values"], ids, am, flags, kw["motion_feature"], key_drop=seg["frames"], max_new_tokens=2, **opts)
        with pytest.raises(ValueError, match=word + ": forward_shared_prefix"):
            model.forward_shared_prefix([(ids, am, kw["labels"])], pixel_values=kw["pixel_values"], image_flags=flags, motion_feature=kw["motion_feature"], **opts)
        outputs_equal(model(**kw, return_logprobs=True), plain, 2, "plain pass after the refusal")
    # the C ABI's own refusals: a window outside the layers arms nothing; keep_kv under rows or a partial window is refused by the pass, which disarms
    plan = model._plan(ids, am, kw["labels"], flags, 3)
    lib_, ctx = model._native(n_tokens=plan["cu"][-1], n_clips=2, out_rows=len(plan["logit_rows"]), kv_cap=256)      # (sized for the keep_kv passes below before anything is armed)
    w_keys, w_rows = (w.cuda() for w in model._key_drop_words(plan, seg["frames"], seg["text_after"]))
    for window in ((-1, 2), (3, 2), (0, LAYERS + 1)):
        assert lib.aigv_key_drop_arm_ex(ctx, w_keys.data_ptr(), w_rows.data_ptr(), 4, *window) == AIGV_ERR_ARG and "layers" in lib.aigv_last_error(ctx).decode()
    assert lib.aigv_key_drop_arm_ex(ctx, w_keys.data_ptr(), w_rows.data_ptr() + 4, 4, 0, 2) == AIGV_ERR_ARG and "row_words_dev" in lib.aigv_last_error(ctx).decode()
    outputs_equal(model(**kw, return_logprobs=True), plain, 2, "plain pass: nothing was armed")
    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    for rows_ptr, window in ((w_rows.data_ptr(), (0, LAYERS)), (None, (0, 2))):
        native.check(lib.aigv_key_drop_arm_ex(ctx, w_keys.data_ptr(), rows_ptr, 4, *window), ctx)
        with pytest.raises(native.NativeError, match="keep_kv under a key-drop mask"):
            model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"], keep_kv=True, kv_cap=256)
        outputs_equal(model(**kw, return_logprobs=True), plain, 2, "plain pass after the refused keep_kv pass")
    out = model(**kw, return_logprobs=True, key_drop=seg["frames"])
    outputs_equal(out, masked, 2, "masked pass afterwards")
