"""Key-drop through the KV cache, the conditions that need no GPU: the rig of tests/test_gpu_key_drop_cache.py is not vacuous (hiding the
chosen unit changes what the oracle generates), the word rows the cache mask is filled from, the new C-ABI symbol in the header and the
binding, the host refusals of generate*(key_drop=...) before any launch, and the signatures that stay as they are."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import key_drop_reference as R
from test_key_drop_cpu import host_rig

import aigv_assessor_amd as pkg
from aigv_assessor_amd import dist_utils, eval_utils, native, prompts, synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_TOKENS = 6
UNIT = 0                      # frame 0 of every clip: the unit the GPU file hides
# Weight seeds of the GPU file's rig, by stage, picked here among seeds 100..139 for the widest gap between the two largest logits over the six
# steps of the UNMASKED oracle reply of both clips (the GPU file lets no unmasked row differ between generate and the one-piece pass): stage 2
# seed 111 - smallest gap 0.086, about 11 bf16 ulps of these logits -, stage 1 seed 108 - 0.078 (seed 127, 0.094, generates the <IMG_CONTEXT> id,
# which a teacher-forced prompt cannot carry).  The rig's own seeds (63 / 62) leave 0.008 / 0.0.
WEIGHT_SEED = {2: 111, 1: 108}
MIN_UNMASKED_GAP = 0.07


# ---- the rig is not vacuous --------------------------------------------------------------------------------------------------------------
def oracle_reply(sd, cfg, one, ctx_id, drop, steps=NEW_TOKENS):
    """Greedy decode of ONE clip with the keys `drop` [1, n] hidden, as the reference hides them: oracle.llm_forward with explicit
    position_ids = arange (oracle.greedy_generate derives the positions from the mask and would shift them) and attention_mask & ~drop, the
    new tokens visible.  -> (tokens [steps], gap between the two largest logits of every step)."""
    vit = O.extract_feature(sd, cfg, one["pixel_values"])[one["image_flags"].squeeze(-1) == 1]
    motion = O.projector(sd, "motion_mlp", one["motion_feature"].view(1, -1))
    emb = O.scatter_embeds(sd, one["input_ids"], ctx_id, vit, motion)
    n = one["input_ids"].shape[1]
    mask = ~drop.clone()
    hidden, past, _ = O.llm_forward(sd, cfg, emb, mask, torch.arange(n)[None])
    toks, gaps = [], []
    for _ in range(steps):
        logits = O.lm_logits(sd, hidden[:, -1:, :])[0, -1]
        top = logits.topk(2).values
        toks.append(int(logits.argmax()))
        gaps.append(float(top[0] - top[1]))
        mask = torch.cat([mask, torch.ones(1, 1, dtype=torch.bool)], 1)
        pos = torch.tensor([[mask.shape[1] - 1]])
        hidden, past, _ = O.llm_forward(sd, cfg, F.embedding(torch.tensor([[toks[-1]]]), O.embed_weight(sd)), mask, pos, past)
    return toks, gaps


@pytest.mark.parametrize("stage", [2, 1])
def test_hiding_frame_0_changes_what_the_oracle_generates(stage):
    """The rig of the GPU file: weights seed WEIGHT_SEED[stage], tokens seed 300 + stage, two clips of 2 and 1 frames, unit 0 (frame 0 of each
    clip) hidden, 6 new tokens.  Measured: stage 2 - clip 0 changes 6 of its 6 tokens, clip 1 changes 5; stage 1 - clip 0 changes 4, clip 1 all 6.
    The unmasked replies' top-2 logit gaps stay above MIN_UNMASKED_GAP (see WEIGHT_SEED), and no reply holds the <IMG_CONTEXT> id: the GPU file
    feeds the replies back as prompt tokens."""
    model, cfg, kw = host_rig(stage)
    sd = synth.make_state_dict(cfg, seed=WEIGHT_SEED[stage], rich=True)
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    changed, f0 = [], 0
    for b, frames in enumerate((2, 1)):
        n = int(kw["attention_mask"][b].sum())
        one = dict(pixel_values=kw["pixel_values"][f0:f0 + frames], input_ids=kw["input_ids"][b:b + 1, :n], image_flags=kw["image_flags"][f0:f0 + frames],
                   motion_feature=kw["motion_feature"][b:b + 1])
        f0 += frames
        base, gaps = oracle_reply(sd, cfg, one, model.img_context_token_id, torch.zeros(1, n, dtype=torch.bool))
        hid, hgaps = oracle_reply(sd, cfg, one, model.img_context_token_id, units[b:b + 1, UNIT, :n])
        changed.append(sum(x != y for x, y in zip(base, hid)))
        assert min(gaps) >= MIN_UNMASKED_GAP, (b, gaps)
        assert model.img_context_token_id not in base + hid
        print(f"stage {stage} clip {b}: base {base} (top-2 logit gaps {[round(g, 3) for g in gaps]}) hidden {hid} (gaps {[round(g, 3) for g in hgaps]}): "
              f"{changed[-1]} of {NEW_TOKENS} tokens changed")
    assert all(c >= 1 for c in changed), changed


# ---- the rows of the cache mask ----------------------------------------------------------------------------------------------------------
def test_cache_mask_rows_are_the_kernel_words_with_a_zero_tail():
    """What a masked keep_kv prefill is armed with (Generation._gen_drop_words) against the word layout restated one bit at a time
    (key_drop_reference.drop_words): bit j & 63 of word j >> 6 = prompt token j of the clip; nothing at or past a clip's length, so that - cut to
    the length and zero-filled to ceil(kv_capacity / 64) words, as the pass stores it - every key a decode step appends starts out visible."""
    model, cfg, kw = host_rig(2)
    ids, am = kw["input_ids"], kw["attention_mask"]
    units = model.unit_masks(ids, am, kw["image_flags"])
    plan = model._plan(ids, am, None, kw["image_flags"], 3, drop_dead_tail=False)
    lens = plan["lens"]
    assert lens == [215, 144]
    drop = units[:, UNIT].clone()
    drop[1, 200] = True                                                        # a padded position of clip 1: ignored
    words = model._gen_drop_words(drop, ids.shape, plan["cu"], plan["row_of"])
    naive = R.drop_words([units[b, UNIT, :lens[b]].numpy() for b in range(2)], 4)
    assert words.dtype == torch.int64 and tuple(words.shape) == (2, 4) and torch.equal(words, naive)
    cap = 215 + NEW_TOKENS + 1                                                 # generate()'s capacity for this prompt
    ld = -(-cap // 64)
    wide = prompts.key_drop_words(drop, plan["cu"], plan["row_of"], n_words=ld)
    assert tuple(wide.shape) == (2, ld) and torch.equal(wide[:, :4], words)
    for b in range(2):
        bits = np.unpackbits(wide[b].numpy().view(np.uint8), bitorder="little")     # bit j of the row = key j
        assert bits.shape[0] == 64 * ld and not bits[lens[b]:].any()                # the zero tail: the new tokens' keys
        assert np.array_equal(bits[:lens[b]].astype(bool), units[b, UNIT, :lens[b]].numpy())
    assert model._gen_drop_words(None, ids.shape, plan["cu"], plan["row_of"]) is None


# ---- the binding -------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    m = re.search(r"int aigv_op_attention_decode_drop\(([^;]*)\);", header)
    assert m, "aigv_op_attention_decode_drop is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    plain = re.search(r"int aigv_op_attention_decode\(([^;]*)\);", header)
    plain_args = [a.strip() for a in plain.group(1).replace("\n", " ").split(",")]
    assert args == plain_args[:-1] + ["const uint64_t* key_drop", "int ld_drop", "void* stream"]           # the op's arguments plus the two new ones
    res, argtypes = native.PROTOTYPES["aigv_op_attention_decode_drop"]
    _, plain_types = native.PROTOTYPES["aigv_op_attention_decode"]
    assert res is native._I and argtypes == plain_types[:-1] + [native._P, native._I, native._P]
    assert "aigv_op_attention_decode_drop" in header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    arm = header[header.index("/* Key-drop mask:"):header.index("int aigv_key_drop_arm(")]
    assert "keep_kv != 0 under a" not in arm and "part of the KV state" in arm                             # the comment no longer says keep_kv is refused


# ---- host refusals and signatures --------------------------------------------------------------------------------------------------------
def test_generate_refuses_on_the_host_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError (or fail to find a GPU), not ValueError."""
    model, cfg, kw = host_rig(2)
    ids, am, flags = kw["input_ids"], kw["attention_mask"], kw["image_flags"]
    ok = model.unit_masks(ids, am, flags)[:, UNIT]

    def bad(mask, word):
        with pytest.raises(ValueError, match=word):
            model.generate_stage2(kw["pixel_values"], ids, am, flags, kw["motion_feature"], key_drop=mask, max_new_tokens=NEW_TOKENS)
        with pytest.raises(ValueError, match=word):
            model.generate(pixel_values=kw["pixel_values"], input_ids=ids, attention_mask=am, key_drop=mask, max_new_tokens=NEW_TOKENS)
        with pytest.raises(ValueError, match=word):
            model.generate2(torch.zeros(2, ids.shape[1], 8), attention_mask=am, key_drop=mask, max_new_tokens=NEW_TOKENS)
        with pytest.raises(ValueError, match=word):
            model.chat2(_Tok(model.img_context_token_id), kw["pixel_values"], ids, dict(max_new_tokens=NEW_TOKENS), am, image_flags=flags,
                        motion_feature=kw["motion_feature"], key_drop=mask)

    bad(ok[:, :100], "shape")
    bad(ok[0], "expected a bool or integer tensor")
    bad(ok.float(), "expected a bool or integer tensor")
    first = ok.clone(); first[1, 0] = True
    bad(first, "clip 1: the first token")
    last = ok.clone(); last[1, 143] = True                                    # clip 1 has 144 prompt tokens: its last row predicts the first new token
    bad(last, "clip 1: the last prompt token")
    last0 = ok.long(); last0[0, 214] = 1
    bad(last0, "clip 0: the last prompt token")


class _Tok:
    """The two tokenizer calls chat2 makes in front of generate_stage2."""

    def __init__(self, ctx_id):
        self.ctx_id = ctx_id

    def convert_tokens_to_ids(self, tok):
        return self.ctx_id if tok == "<IMG_CONTEXT>" else 2


def test_signatures():
    model, cfg, kw = host_rig(2)
    for fn in (model.generate, model.generate2, model.generate_stage2, model.chat2):
        p = inspect.signature(fn).parameters
        assert "key_drop" in p and p["key_drop"].default is None, fn.__name__
    p = inspect.signature(model.generate_stage2).parameters
    assert p["visual_tokens"].default is None and "motion_feature" in p
    sig = inspect.signature(eval_utils.frame_ablation_generate)
    assert list(sig.parameters) == ["model", "pixel_values", "input_ids", "attention_mask", "image_flags", "max_new_tokens", "candidate_ids", "gen"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.parameters.items() if k not in ("model", "gen"))
    assert sig.parameters["candidate_ids"].default is None and sig.parameters["gen"].kind is inspect.Parameter.VAR_KEYWORD
    # left exactly as they are
    assert "key_drop" not in inspect.signature(model.forward_shared_prefix).parameters
    assert "key_drop" not in inspect.signature(eval_utils.batched).parameters and "key_drop" not in inspect.signature(dist_utils.score_clips_dp).parameters
    with pytest.raises(ValueError, match="return_score_attention"):
        model(**kw, key_drop=model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])[:, UNIT], return_score_attention=True)
