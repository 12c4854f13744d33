"""The depth lens without a GPU: the ABI entries, the refusals that come before any launch, the graph key, eval_utils.settling_depth on hand-made
inputs, and the reference of tests/test_gpu_depth_lens.py pinned to the existing oracle - composed layer by layer from the oracle's own
functions it equals oracle.forward_eval at depth L and oracle.llm_forward(all_hidden=True)'s states below it, bit for bit, and on the rig the
depths are far enough apart that a tap reading the wrong depth could not pass the GPU file's comparison."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import depth_lens_reference as DL
from test_key_drop_cpu import bf16_ulps
from test_key_drop_rows_cpu import LAYERS, host_rig, one_clip

from aigv_assessor_amd import dist_utils, eval_utils, native, readouts, synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the ABI entries ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_entries():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I, I32P, F = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_float
    head = native.PROTOTYPES["aigv_op_score_head"]
    want = {"aigv_depth_lens_arm": (I, [P, I32P, I, I32P, I, P, P, P]),
            "aigv_depth_lens_token_readout": (I, [P, P, I, I, P, I, P, P, P, P]),
            "aigv_op_lens_tap": (I, [P, I, P, I, P, P, P, I, F, P]),
            "aigv_op_score_head_groups": (head[0], head[1][:2] + [I, ctypes.c_int64] + head[1][2:])}
    for name, proto in want.items():
        assert name in note and re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == proto, name
    assert re.search(r"#define AIGV_MAX_LENS_ROWS 64\b", header) and readouts.MAX_LENS_ROWS == 64
    kernels = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert "aigv_launch_lens_tap(" in kernels and "aigv_launch_score_head_groups(" in kernels


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_native_refusals_without_a_gpu():
    """Every check of the two ops comes before any HIP call: AIGV_ERR_ARG and a message that starts with the op's name (fake, aligned,
    non-null addresses: nothing is dereferenced).  The context entry points refuse a null handle."""
    lib = native.load()
    P = 0x10000
    last = lambda: (lib.aigv_last_error(None) or b"").decode()

    def tap(src=P, ld=128, idx=P, n=4, w=P, raw=P, normed=P, H=128):
        return lib.aigv_op_lens_tap(src, ld, idx, n, w, raw, normed, H, 1e-6, None), last()

    for kw, word in ((dict(src=None), "null operand"), (dict(idx=None), "null operand"), (dict(w=None), "null operand"), (dict(normed=None), "null operand"),
                     (dict(n=-1), "must not be negative"), (dict(H=100), "multiple of 8"), (dict(ld=120), "leading dimension"), (dict(ld=132), "leading dimension"),
                     (dict(src=P + 8), "16-byte aligned"), (dict(raw=P + 8), "16-byte aligned"), (dict(normed=P + 8), "16-byte aligned"), (dict(w=P + 2), "16-byte aligned"),
                     (dict(H=16392, ld=16392), "above 16384")):
        rc, msg = tap(**kw)
        assert rc == -1 and word in msg and msg.startswith("aigv_op_lens_tap:"), (kw, rc, msg)

    dims = native.i32_array([256, 64, 16, 1])
    ptrs = (ctypes.c_void_p * 3)(P, P, P)

    def groups(G=3, B=4, stride=4 * 256, scratch_bytes=3 * 12 * 256 * 2, x=P, n_layers=3, d=dims):
        return lib.aigv_op_score_head_groups(x, 256, G, stride, B, n_layers, d, ptrs, ptrs, P, scratch_bytes, P, None), last()

    for kw, word in ((dict(G=0), "G = 0"), (dict(G=65, B=64), "G * B <= 4096"), (dict(stride=-1), "group_stride"), (dict(B=65, G=1), "B = 65 outside 1..64"),
                     (dict(B=0), "B = 0 outside 1..64"), (dict(scratch_bytes=3 * 12 * 256 * 2 - 2), "scratch of"), (dict(x=None), "null operand"),
                     (dict(n_layers=9), "n_layers"), (dict(n_layers=1, d=native.i32_array([256, 4])), "no tail layer")):
        rc, msg = groups(**kw)
        assert rc == -1 and word in msg and msg.startswith("aigv_op_score_head_groups:"), (kw, rc, msg)
    assert lib.aigv_depth_lens_arm(None, None, 0, None, 0, P, P, P) == -1 and "aigv_depth_lens_arm: null context" in last()
    assert lib.aigv_depth_lens_token_readout(None, P, 128, 1, None, 0, P, P, None, None) == -1 and "aigv_depth_lens_token_readout: null argument" in last()


def test_host_refusals_come_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError."""
    model, cfg, kw = host_rig(1)
    with pytest.raises(ValueError, match="return_depth_lens: nothing to read"):
        model(**dict(kw, labels=None), return_depth_lens=True)                       # stage 1 without labels: neither a score row nor a token row
    with pytest.raises(ValueError, match="return_depth_lens: nothing to read"):
        model(**dict(kw, labels=torch.full_like(kw["labels"], -100)), return_depth_lens=True)
    with pytest.raises(ValueError, match="return_depth_lens: at most 64 clips"):
        readouts.ReadOuts.parse(cfg.llm_config.vocab_size, "given", ids_shape=(65, 10), return_depth_lens=True)
    # the entry points the issue leaves alone keep their signatures
    model2 = host_rig(2)[0]
    for fn in (model2.forward_shared_prefix, model2.generate, model2.generate_stage2, eval_utils.batched, dist_utils.score_clips_dp):
        assert "return_depth_lens" not in inspect.signature(fn).parameters, fn
    assert "return_depth_lens" in inspect.signature(model2.forward).parameters


def test_depth_lens_rows_follow_the_probes_stage_1_rule():
    for stage in (2, 1):
        model, cfg, kw = host_rig(stage)
        plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
        score_rows, clips, token_rows = model._depth_lens_rows(plan, True)
        assert clips == [0, 1] and token_rows == model._probe_rows(dict(plan, score_rows=None))
        assert score_rows == ([int(r) for r in plan["score_rows"]] if stage == 2 else [])
        assert set(token_rows) <= set(plan["logit_rows"])                                # consumed rows: the last layer finishes them
        lab = kw["labels"].clone(); lab[1] = -100                                        # clip 1 without an answer token
        plan1 = model._plan(kw["input_ids"], kw["attention_mask"], lab, kw["image_flags"], 3)
        if stage == 2:
            s1, c1, t1 = model._depth_lens_rows(plan1, True)
            assert c1 == [0] and len(t1) == 1 and len(s1) == 2
            assert model._depth_lens_rows(plan, False)[1:] == ([], [])                   # without labels the token outputs are absent


# ---- the graph key ------------------------------------------------------------------------------------------------------------------
def test_key_tail_without_the_flag_is_the_tuple_it_was():
    V, shape = 1000, (2, 215)
    cases = (dict(), dict(return_logprobs=True), dict(candidate_ids=[1, 2, 3], top_logprobs=4), dict(return_score_attention=True),
             dict(return_token_attention=True, return_logprobs=True))
    was = ((), ("logprobs",), ("candidates", ("top_logprobs", 4)), (("score_attention", 0),), ("logprobs", ("score_attention", 0), ("score_attention_tokens", 215)))
    for kw, tail in zip(cases, was):
        assert readouts.ReadOuts.parse(V, "given", ids_shape=shape, **kw).key_tail(shape) == tail, kw
        ro = readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_depth_lens=True, **kw)
        assert ro.depth_lens and ro.key_tail(shape) == tail + ("depth_lens",), kw
        assert readouts.forward_kwargs(ro)["return_depth_lens"] is True
    assert "return_depth_lens" not in readouts.forward_kwargs(readouts.ReadOuts(logprobs=True))
    assert "lens_score" not in [f[0] for f in readouts.ROW_FIELDS]                       # per clip, like score_attention: no row field


# ---- settling_depth ------------------------------------------------------------------------------------------------------------------
def test_settling_depth_on_hand_made_inputs():
    nan = float("nan")
    s = torch.tensor([[0.10, 0.50, 0.49, 0.50],      # settles at 1
                      [0.50, 0.50, 0.50, 0.50],      # all equal: 0
                      [0.10, 0.20, 0.30, 0.50],      # only the last depth qualifies: L
                      [0.50, nan, 0.50, 0.50],       # a NaN never qualifies: 2
                      [0.50, 0.10, 0.50, 0.50],      # a late excursion resets: 2
                      [0.50, 0.50, 0.50, nan]])      # a NaN final score: L
    got = eval_utils.settling_depth(s, 0.02)
    assert got.dtype == torch.long and got.tolist() == [1, 0, 3, 2, 2, 3]
    assert eval_utils.settling_depth(s, 0.0).tolist() == [3, 0, 3, 2, 2, 3]              # |0.49 - 0.5| > 0; exact equality qualifies
    assert eval_utils.settling_depth(s[:3], 1.0).tolist() == [0, 0, 0]
    assert eval_utils.settling_depth(s[:, 3:], 0.0).tolist() == [0] * 6                  # L = 0
    assert eval_utils.settling_depth(s.to(torch.bfloat16), 0.02).tolist() == [1, 0, 3, 2, 2, 3]
    for bad in (lambda: eval_utils.settling_depth(s[0], 0.1), lambda: eval_utils.settling_depth(s, -1.0), lambda: eval_utils.settling_depth(s, nan)):
        with pytest.raises(ValueError, match="settling_depth"):
            bad()


# ---- the composed reference, pinned to the existing oracle ----------------------------------------------------------------------------
def rig_lens(stage, b):
    model, cfg, kw = host_rig(stage)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    one, n = one_clip(kw, b)
    common = dict(img_context_token_id=model.img_context_token_id)
    inputs = {k: v for k, v in one.items() if k != "labels"}
    states = DL.composed_states(sd, cfg, **inputs, **common)
    return model, cfg, sd, one, common, inputs, states


@pytest.mark.parametrize("stage", [2, 1])
def test_composed_reference_is_the_oracle_at_depth_L_and_its_own_states_below(stage):
    for b in range(2):
        model, cfg, sd, one, common, inputs, states = rig_lens(stage, b)
        assert len(states) == LAYERS + 1
        ref = O.forward_eval(sd, cfg, **one, **common, stage=stage, return_intermediates=True)
        _, _, own = O.llm_forward(sd, cfg, ref["inputs_embeds"], one["attention_mask"], all_hidden=True)
        assert len(own) == LAYERS + 1
        for d in range(LAYERS):
            assert torch.equal(states[d], own[d]), d                                     # the layer inputs: depths 0 .. L - 1
        normed = O.rms_norm_cast_then_scale(states[LAYERS], sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps)
        assert torch.equal(normed, own[LAYERS]) and torch.equal(normed, ref["hidden"])
        got = DL.lens(sd, cfg, states, one["attention_mask"], one["labels"], stage, candidate_ids=[5, 7, 11])
        t = DL.token_row(one["labels"][0])
        assert int(got["token"][0, LAYERS]) == int(ref["logit"][t]) and torch.equal(got["token_logits"][0, LAYERS], ref["logits"][0, t])
        logp = torch.log_softmax(ref["logits"][0, t], -1)
        assert torch.equal(got["token_logprob"][0, LAYERS], logp[ref["logit"][t]]) and torch.equal(got["cand_logprob"][0, LAYERS], logp[[5, 7, 11]])
        if stage == 2:
            assert torch.equal(got["score"][:, LAYERS].view(torch.int16), ref["score1"].view(torch.int16))
            assert torch.equal(got["score_hidden"][0, 0], ref["inputs_embeds"][0, -4])
        else:
            assert "score" not in got
    # a clip without an answer token: -1 / NaN / zeros
    lab = torch.full_like(one["labels"], -100)
    none = DL.lens(sd, cfg, states, one["attention_mask"], lab, stage)
    assert none["token"].eq(-1).all() and none["token_logprob"].isnan().all() and not none["token_hidden"].any()


def test_oracle_condition_every_depth_is_told_apart():
    """Weights seed 63, tokens seed 302 (the stage-2 rig of the GPU file), every clip alone in bf16.  Measured: clip 0 (215 tokens) scores at
    depths 0..4 0.49609, 0.48242, 0.48633, 0.47070, 0.48047 - adjacent depths at least 2 bf16 ulps apart, depth 4 the documented base score - and
    token-row argmaxes 576, 849, 752, 245, 499; clip 1: depths 2 and 4 share a score, the tokens 368, 720, 683, 41, 490 tell every depth
    apart.  A tap that read another depth could not pass the GPU file's comparison.  (The table is printed, not asserted: the oracle's bf16
    matmuls sum in an order that follows the host's thread count, and clip 0's depth-3 row is decided within 1 bf16 ulp - 245 against 779.)"""
    scores, tokens = [], []
    for b in range(2):
        model, cfg, sd, one, common, inputs, states = rig_lens(2, b)
        got = DL.lens(sd, cfg, states, one["attention_mask"], one["labels"], 2)
        scores.append([float(v) for v in got["score"][0]])
        tokens.append(got["token"][0].tolist())
        print(f"clip {b}: lens scores {['%.5f' % v for v in scores[-1]]}, token-row argmax {tokens[-1]}")
    assert int(host_rig(2)[2]["attention_mask"][0].sum()) == 215
    # adjacent depths - what a tap shifted by one layer would read - are at least 2 bf16 ulps apart, twice the GPU file's bar; so is every other
    # pair but one: depths 1 and 4 (0.48242 and 0.48047 of the table above) are exactly 1 ulp apart, so "pairwise at least 2" cannot be asserted of
    # these five numbers - every pair is asserted at what the table gives it
    for i in range(LAYERS + 1):
        for j in range(i):
            assert bf16_ulps(scores[0][i], scores[0][j]) >= (1 if (i, j) == (4, 1) else 2), (i, j)
    assert all(len(set(t)) == LAYERS + 1 for t in tokens)
