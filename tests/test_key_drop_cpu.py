"""Key-drop attention without a GPU: the conditions tests/test_gpu_key_drop.py rests on, the host helpers (prompts.key_drop_words,
model.unit_masks), every host-side refusal of forward(key_drop=...), the header / binding of the two ABI entries, and the oracle condition -
on the tiny rig the GPU file uses, hiding frame 0 from the oracle moves a score by at least 8 bf16 ulps and changes answer tokens, so a
masked pass that ignored its mask could not pass the GPU file's comparison."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import key_drop_reference as R
from attention_exact_reference import BF, bf16_bits, census_bits

import aigv_assessor_amd as pkg
from aigv_assessor_amd import native, prompts, readouts, synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("packed", g) for g in R.GROUPS] + [("cache", g) for g in R.GROUPS]


def make_case(form, g):
    return R.packed_case(g) if form == "packed" else R.cache_case(g)


def patterns_of(form):
    return [p for p in R.PATTERNS if p != "g" or form == "cache"]


# ---- the ABI entries ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_two_entries():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("#define AIGV_MAX_CANDIDATES")]
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ex = native.PROTOTYPES["aigv_op_attention_ex"]
    for name, proto in (("aigv_key_drop_arm", (I, [P, P, I])), ("aigv_op_attention_drop", (ex[0], ex[1][:-1] + [P, I, P]))):
        assert name in note and re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == proto, name
    src = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert "const uint64_t* key_drop;" in src and "int ld_drop;" in src


def test_op_refusals_without_a_gpu():
    """aigv_attn_check's refusals of the two new fields come before any HIP call: AIGV_ERR_ARG and a message naming the op (fake, aligned,
    non-null addresses: nothing is dereferenced)."""
    lib = native.load()
    D, h, n = 128, 2, 215
    ld = 4 * D
    P = 0x10000

    def call(head_dim=D, causal=1, key_drop=P, ld_drop=4, max_len=n):
        rc = lib.aigv_op_attention_drop(P, ld, P, ld, P, ld, P, h * D, P, 1, max_len, h, h, 2 * D, 2 * D, 0, None, head_dim, causal, 11.3, 1.0, None, None, None, 0, 0,
                                        key_drop, ld_drop, None)
        return rc, (lib.aigv_last_error(None) or b"").decode()

    for kw, word in ((dict(causal=0), "causal head_dim 128"), (dict(head_dim=64), "causal head_dim 128"), (dict(ld_drop=3), "ld_drop"), (dict(ld_drop=0), "ld_drop"),
                     (dict(ld_drop=-1), "ld_drop"), (dict(key_drop=P + 4), "8-byte aligned"), (dict(max_len=257, ld_drop=4), "ld_drop")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and msg.startswith("aigv_op_attention_drop:"), (kw, rc, msg)
    assert lib.aigv_key_drop_arm(None, P, 4) == -1 and "null context" in lib.aigv_last_error(None).decode()


# ---- the patterns and the word layout ---------------------------------------------------------------------------------------------------
def test_the_cases_and_patterns_are_the_ones_the_issue_names():
    assert R.PACKED_LENS == [215, 144, 64, 1] and R.CACHE_OFF == [0, 100, 254] and R.Q_TAILS == (0, 4) and R.GROUPS == [1, 3, 4]
    case = R.packed_case(1)
    a = R.drop_sets(case, "a")[0]
    assert a[31] and a[32] and a[63] and not a[0]
    assert np.array_equal(np.nonzero(R.drop_sets(case, "b")[0])[0], np.arange(45, 109))
    c = R.drop_sets(case, "c")[0]
    assert np.array_equal(np.nonzero(c)[0], np.arange(64, 192))
    w = R.drop_words([c], 4)[0].tolist()
    assert w == [0, -1, -1, 0]                                            # whole tiles: all-ones words, the skip path
    d = np.nonzero(R.drop_sets(case, "d")[0])[0]
    assert d.min() >= 192 and d.max() < 215 and len(d) > 3               # the ragged last tile (keys 192..214)
    e = R.drop_sets(case, "e")
    assert all(m[0] for m in e)
    assert not any(m.any() for m in R.drop_sets(case, "f"))
    g = R.drop_sets(R.cache_case(1), "g")
    assert not g[0].any() and g[1][:100].any() and not g[1][100:].any() and g[2][:254].any() and not g[2][254:].any()
    assert R.words_needed(R.cache_case(1)) == 8 and R.words_needed(case) == 4


def naive_words(kd, lens, W):
    out = torch.zeros(len(lens), W, dtype=torch.int64)
    for b, n in enumerate(lens):
        for j in range(n):
            if bool(kd[b, j]):
                bit = 1 << (j & 63)
                out[b, j >> 6] |= bit - (1 << 64) if bit >= 1 << 63 else bit
    return out


def test_key_drop_words_against_a_naive_loop():
    lens = [64, 65, 215, 1, 128]                                           # exactly one tile, one key more, ragged, one token, two tiles
    N = 215
    gen = torch.Generator().manual_seed(5)
    kd = torch.rand(len(lens), N, generator=gen) < 0.3
    kd[0, 63] = kd[1, 63] = kd[1, 64] = kd[2, 214] = True
    cu = [0] + list(np.cumsum(lens))
    got = prompts.key_drop_words(kd, cu)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, 4)
    assert torch.equal(got, naive_words(kd, lens, 4))                      # bits past a clip's length are clear: the naive loop stops there
    assert got[0, 0] < 0 and got[0, 1:].eq(0).all() and got[1, 1] == 1 and got[3, 0] in (0, 1)
    assert torch.equal(prompts.key_drop_words(kd.long(), cu, n_words=6)[:, :4], got) and prompts.key_drop_words(kd, cu, n_words=6)[:, 4:].eq(0).all()
    # the same through row_of (left-padded rows: the packed position is not the column)
    row_of = torch.full((len(lens), N), -1, dtype=torch.long)
    shifted = torch.zeros_like(kd)
    for b, n in enumerate(lens):
        row_of[b, N - n:] = torch.arange(cu[b], cu[b + 1])
        shifted[b, N - n:] = kd[b, :n]
        shifted[b, :N - n] = True                                          # padding: ignored
    assert torch.equal(prompts.key_drop_words(shifted, cu, row_of), got)
    # and the reference module's own loop agrees with it
    assert torch.equal(R.drop_words([kd[b, :n].numpy() for b, n in enumerate(lens)], 4), got)
    for bad in (lambda: prompts.key_drop_words(kd.float(), cu), lambda: prompts.key_drop_words(kd, cu[:-1]), lambda: prompts.key_drop_words(kd, cu, n_words=3),
                lambda: prompts.key_drop_words(kd[:, :100], cu)):
        with pytest.raises(ValueError):
            bad()


# ---- the two constructions under a mask -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(form, g, pattern, construction):
    case = make_case(form, g)
    drops = R.drop_sets(case, pattern)
    return case, drops, (R.census if construction == "census" else R.selector)(case, drops)


def fp64_bits(case, data, drops, ignore_mask, construction):
    """The float64 masked softmax of the generated tensors -> the kernel's output bits.  Census: the un-normalised sums of the fp64 softmax
    (integers) under the prefill kernel's own normalisation (fp32 count x reciprocal); selector: the fp64 output rounded to bf16."""
    out = []
    for s in range(len(case.cnts)):
        q, k, v, off, drop = data.q[s], data.k[s], data.v[s], case.offs[s], drops[s]
        if construction == "census":
            assert (q == 0).all() and torch.isfinite(k.float()).all() and (k[torch.from_numpy(drop)].float() == float(torch.tensor(R.BIG_K).to(BF))).all()
            vis = (np.arange(case.tot[s])[None, :] <= (off + np.arange(case.cnts[s]))[:, None]) & (ignore_mask | ~drop[None, :])
            p = torch.from_numpy(vis).double()                               # exp(0 - 0) = 1 on every visible key (Q = 0: K cannot matter)
            num = torch.einsum("nt,tkd->nkd", p, v.double()).numpy()
            e = np.stack([census_bits(num[:, kh], vis.sum(1), "prefill") for kh in range(case.hk)], 1)
            want = num / np.maximum(vis.sum(1), 1)[:, None, None]
            got = torch.from_numpy(e).view(BF).double().numpy()
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(want, 1e-30))) - 7)
            assert (np.abs(got - want) <= ulp).all()                         # ... which is the fp64 quotient to one bf16 ulp
            out.append(torch.from_numpy(np.repeat(e, case.g, axis=1)))
        else:
            o = R.masked_attention(q, k, v, off, drop, case.post, torch.float64, ignore_mask)
            out.append(torch.from_numpy(bf16_bits(o.float().numpy())))
    return torch.cat(out)


@pytest.mark.parametrize("construction", ["census", "selector"])
@pytest.mark.parametrize("form,g", CASES)
def test_fp64_masked_softmax_rounds_to_the_expected_bits_and_the_mask_matters(form, g, construction):
    for pattern in patterns_of(form):
        case, drops, data = built(form, g, pattern, construction)
        assert torch.equal(fp64_bits(case, data, drops, False, construction), data.expect), (pattern, "the expectation is not the masked softmax")
        ignored = fp64_bits(case, data, drops, True, construction)
        if pattern == "f":
            assert torch.equal(ignored, data.expect)
        else:
            assert not torch.equal(ignored, data.expect), (pattern, "ignoring the mask changes nothing: the GPU test would prove nothing")
            # ... and on EVERY row that sees a dropped key
            row = 0
            for s, n in enumerate(case.cnts):
                sees = ((np.arange(case.tot[s])[None, :] <= (case.offs[s] + np.arange(n))[:, None]) & drops[s][None, :]).any(1)
                diff = (ignored[row:row + n] != data.expect[row:row + n]).any(-1).any(-1).numpy()
                # (census: a row whose visible keys number a multiple of D with AND without the mask has the same count in every column
                # either way - one row in these cases; the selector has no such blind row)
                blind = 0 if construction == "selector" else 1
                assert not (diff & ~sees).any() and (sees & ~diff).sum() <= blind, (pattern, s, np.nonzero(diff != sees)[0][:8])
                row += n


@pytest.mark.parametrize("form,g", CASES)
def test_selector_decoys_tie_the_chosen_key_and_everything_else_underflows(form, g):
    for pattern in patterns_of(form):
        case, drops, data = built(form, g, pattern, "selector")
        for s in range(len(case.cnts)):
            pi, drop, off = data.pi[s], drops[s], case.offs[s]
            sc = torch.einsum("nhd,thd->nht", data.q[s].double(), data.k[s].double().repeat_interleave(case.g, 1)) / case.post
            for r in range(case.cnts[s]):
                seen = np.arange(case.tot[s]) <= off + r
                if pi[r, 0] < 0:
                    assert not (seen & ~drop).any()                           # no visible key: the zero row
                    assert (data.expect[sum(case.cnts[:s]) + r] == 0).all()
                    continue
                assert not drop[pi[r, 0]] and seen[pi[r, 0]]
                top = sc[r, :, pi[r, 0]]
                decoy = torch.from_numpy(seen & drop)
                assert (sc[r][:, decoy] == top[:, None]).all()               # every visible dropped key ties the chosen one exactly
                other = torch.from_numpy(seen & ~drop)
                other[pi[r, 0]] = False
                if other.any():
                    assert ((top[:, None] - sc[r][:, other]).min() * 1.4426950408889634) >= 160      # > 149 octaves: P underflows to 0 in fp32


def test_q_tail_rows():
    w = R.waves_written([215, 144, 64, 1], 4)
    assert w.sum() == (215 - 192) + (144 - 128) + 32 + 1 and R.waves_written([215], 0).all()


# ---- unit masks and the host refusals (a model object on the host: no GPU work) -----------------------------------------------------------
def two_clips(cfg, seed, frames=(2, 1)):
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
def host_rig(stage=2):
    from aigv_assessor_amd.modeling import InternVLChatModel
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    model = InternVLChatModel(cfg, stage=stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    return model, cfg, kw


def test_the_rig_has_the_shape_the_issue_states():
    model, cfg, kw = host_rig()
    assert kw["input_ids"].shape == (2, 215) and model.num_image_token == 64
    pos = model.visual_token_positions(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    assert int(pos[0, 0, 0]) == 45 and kw["attention_mask"].sum(1).tolist() == [215, 144]


def test_unit_masks_against_visual_token_positions():
    model, cfg, kw = host_rig()
    ids, am, flags = kw["input_ids"], kw["attention_mask"], kw["image_flags"]
    units = model.unit_masks(ids, am, flags)
    pos = model.visual_token_positions(ids, am, flags)                       # [B, F, 64] in-clip positions = columns (right-padded)
    B, F, ntok = pos.shape
    assert units.dtype == torch.bool and tuple(units.shape) == (B, F + 1, ids.shape[1]) and F == 2
    for b in range(B):
        for f in range(F):
            want = torch.zeros(ids.shape[1], dtype=torch.bool)
            if int(pos[b, f, 0]) >= 0:
                want[pos[b, f]] = True
            assert torch.equal(units[b, f], want), (b, f)
        assert units[b, F].sum() == 1                                         # the motion token: the clip's last <IMG_CONTEXT>
        ctx = (ids[b] == model.img_context_token_id) & am[b]
        assert int(units[b, F].nonzero()) == int(ctx.nonzero().max())
        assert torch.equal(units[b].any(0), ctx)                              # the units cover exactly the clip's visual + motion tokens
    assert not units[1, 1].any() and units[0, 1].sum() == ntok                # clip 1 has one frame: its frame-1 row is all False
    assert torch.equal(model.unit_masks(ids, am, None, n_frames=3), units)


def test_host_refusals_come_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError."""
    model, cfg, kw = host_rig()
    ids, am = kw["input_ids"], kw["attention_mask"]
    units = model.unit_masks(ids, am, kw["image_flags"])
    ok = units[:, 0]
    plan = model._plan(ids, am, kw["labels"], kw["image_flags"], 3)

    def bad(mask, word, **extra):
        with pytest.raises(ValueError, match=word):
            model(**kw, key_drop=mask, **extra)

    bad(ok[:, :100], "shape")
    bad(ok[0], "expected a bool or integer tensor")
    bad(ok.float(), "expected a bool or integer tensor")
    first = ok.clone(); first[1, 0] = True
    bad(first, "clip 1: the first token")
    score = ok.clone(); score[0, 215 - 4] = True
    bad(score, "consumed row")
    answer = ok.clone()
    b, p = [int(x) for x in (kw["labels"][:, 1:] != -100).nonzero()[0]]
    answer[b, p] = True                                                       # the row that predicts the first answer token
    bad(answer, "consumed row")
    bad(ok, "return_score_attention", return_score_attention=True)
    bad(ok, "return_score_attention", return_token_attention=True)
    # padded positions are ignored; integer masks are taken
    padded = ok.long(); padded[1, 200] = 1
    w = model._key_drop_words(plan, readouts.key_drop_mask(padded, ids.shape))
    assert torch.equal(w, model._key_drop_words(plan, ok)) and torch.equal(w, prompts.key_drop_words(ok, plan["cu"], plan["row_of"]))
    assert tuple(w.shape) == (2, 4) and bin(int(w[0, 0]) & (2 ** 64 - 1)).count("1") == 64 - 45
    # forward_shared_prefix, batched and score_clips_dp do not take the argument
    import inspect
    from aigv_assessor_amd import dist_utils, eval_utils
    assert "key_drop" not in inspect.signature(model.forward_shared_prefix).parameters
    assert "key_drop" not in inspect.signature(eval_utils.batched).parameters and "key_drop" not in inspect.signature(dist_utils.score_clips_dp).parameters
    assert "key_drop" not in readouts.forward_kwargs(readouts.ReadOuts(logprobs=True))


# ---- the oracle condition --------------------------------------------------------------------------------------------------------------
def bf16_ulps(a, b):
    ulp = 2.0 ** (np.floor(np.log2(abs(b))) - 7)
    return abs(a - b) / ulp


def test_oracle_condition_hiding_frame_0_moves_the_score_and_the_answer_tokens():
    """Weights seed 63, tokens seed 302 (the stage-2 rig of the GPU file), every clip on its own so that hidden[:, -4] is its score row.
    Measured: clip 1 (one frame) 0.4765625 -> 0.5 = 12 bf16 ulps with 10 of 10 answer tokens changed; clip 0 (two frames) by 2 ulps with 6 of
    10 tokens changed; hiding the motion token moves neither score."""
    model, cfg, kw = host_rig(2)
    sd = synth.make_state_dict(cfg, seed=63, rich=True)
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    moved, flipped = [], []
    f0 = 0
    for b, frames in enumerate((2, 1)):
        n = int(kw["attention_mask"][b].sum())
        one = dict(pixel_values=kw["pixel_values"][f0:f0 + frames], input_ids=kw["input_ids"][b:b + 1, :n], image_flags=kw["image_flags"][f0:f0 + frames],
                   labels=kw["labels"][b:b + 1, :n], motion_feature=kw["motion_feature"][b:b + 1], img_context_token_id=model.img_context_token_id, stage=2)
        f0 += frames
        am = kw["attention_mask"][b:b + 1, :n]
        base = O.forward_eval(sd, cfg, attention_mask=am, **one)
        drop = O.forward_eval(sd, cfg, attention_mask=am & ~units[b:b + 1, 0, :n], **one)
        assert torch.isfinite(drop["score1"].float()).all()
        want = base["label"] != -100
        moved.append(bf16_ulps(float(drop["score1"][0]), float(base["score1"][0])))
        flipped.append(int((drop["logit"][want] != base["logit"][want]).sum()))
        print(f"clip {b}: score {float(base['score1'][0])} -> {float(drop['score1'][0])} = {moved[-1]:.1f} bf16 ulps, {flipped[-1]} of {int(want.sum())} answer tokens changed")
    assert max(moved) >= 8 and min(flipped) > 0
