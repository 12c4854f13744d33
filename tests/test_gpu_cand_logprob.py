"""Candidate-token log-probabilities (``candidate_ids``; MI355X only): the distribution over the quality-level words from ONE pass.

Op level: ``aigv_op_cand_logprob`` against an fp64 log-softmax (the 1e-5 bar tests/test_gpu_logprob.py applies to ``aigv_op_label_logprob``
- the same arithmetic) and against ``aigv_op_label_logprob`` itself, bit for bit; ``aigv_op_lm_head_argmax_cand_logprob`` (the decode
step's lm-head) against ``aigv_op_lm_head_argmax_logprob`` and the store form of the same GEMV, bit for bit.

Model level: ``forward`` / ``forward_shared_prefix`` / ``eval_utils.batched`` / ``score_clips_dp`` / ``generate`` with ``candidate_ids``
against the label log-probabilities of the same passes (bit for bit), the CPU oracle's logits (the bar of
``test_logprob_and_ce_loss_against_the_oracle``: |lp_hip - lp_oracle| <= 2 max_v |l_hip - l_oracle| + 1e-5 per row) and the README's
five-candidate recipe."""
import os
import subprocess
import sys

import pytest
import torch

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, generation, native, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def make_model(cfg, sd, stage=2):
    from aigv_assessor_amd.modeling import InternVLChatModel
    m = InternVLChatModel(cfg, stage=stage)
    m.load_state_dict(sd)
    return m.eval().cuda()


# ---- 1. the scoring pass's operator --------------------------------------------------------------------------------------------------

def _cand_op(lib, x, rows, V, ldo, cand):
    cd = torch.tensor(cand, dtype=torch.long, device="cuda")
    out = torch.full((rows, len(cand)), 7.0, dtype=torch.float32, device="cuda")
    native.check(lib.aigv_op_cand_logprob(x.data_ptr(), rows, V, ldo, cd.data_ptr(), len(cand), out.data_ptr(), native.stream_ptr()))
    return out


@pytest.mark.parametrize("V", [1, 515, 2053, 92553])
def test_op_cand_logprob_against_fp64_label_logprob_and_invariances(V):
    lib = native.load()
    R = 64
    for ldo in sorted({V, (V + 3) // 4 * 4, (V + 3) // 4 * 4 + 8}):      # unaligned rows (scalar loads), aligned, padded
        g = torch.Generator().manual_seed(V + ldo)
        x = (torch.randn(R, ldo, generator=g) * 3).to(BF)
        x[:, V:] = 100.0                                                   # padding columns must not count
        cand = [0, V - 1, V // 2, V // 3, V // 2]                          # first, last, a duplicate
        xd = x.cuda()
        out = _cand_op(lib, xd, R, V, ldo, cand)
        torch.cuda.synchronize()
        want = torch.log_softmax(x[:, :V].double(), -1)[:, cand]
        err = (out.cpu().double() - want).abs().max().item()
        print(f"V={V} ldo={ldo}: max |cand lp - fp64| = {err:.3g}")
        assert err <= 1e-5
        # column c = aigv_op_label_logprob with labels = cand[c], bit for bit
        for c, tok in enumerate(cand):
            lab = torch.full((R,), tok, dtype=torch.long, device="cuda")
            one = torch.empty(R, dtype=torch.float32, device="cuda")
            native.check(lib.aigv_op_label_logprob(xd.data_ptr(), R, V, ldo, lab.data_ptr(), one.data_ptr(), native.stream_ptr()))
            assert torch.equal(bits(one), bits(out[:, c])), (c, tok)
        # bits do not depend on the number of rows, on C or on the candidates' order
        for r in (0, 17, 63):
            assert torch.equal(bits(_cand_op(lib, xd[r], 1, V, ldo, cand)), bits(out[r:r + 1]))
        assert torch.equal(bits(_cand_op(lib, xd, 33, V, ldo, cand)), bits(out[:33]))
        assert torch.equal(bits(_cand_op(lib, xd, R, V, ldo, cand[:1])), bits(out[:, :1]))
        perm = [3, 0, 4, 2, 1]
        assert torch.equal(bits(_cand_op(lib, xd, R, V, ldo, [cand[i] for i in perm])), bits(out[:, perm]))
        many = [(7 * i) % V for i in range(64)]
        assert torch.equal(bits(_cand_op(lib, xd, R, V, ldo, many)[:, 5]), bits(_cand_op(lib, xd, R, V, ldo, [many[5]])[:, 0]))
        # an out-of-range candidate: a NaN column, the others untouched
        bad = _cand_op(lib, xd, R, V, ldo, [cand[0], V, cand[1], -100, -1, cand[2]]).cpu()
        assert torch.isnan(bad[:, [1, 3, 4]]).all()
        assert torch.equal(bits(bad[:, [0, 2, 5]]), bits(out[:, [0, 1, 2]]))


# ---- 2. the decode step's lm-head ---------------------------------------------------------------------------------------------------

def _argmax_logprob(lib, h, W, V):
    R, H = h.shape
    nbytes = lib.aigv_op_lm_head_argmax_logprob_scratch_bytes(R, V)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    idx = torch.full((R,), -7, dtype=torch.long, device="cuda")
    val = torch.full((R,), float("nan"), device="cuda")
    lp = torch.full((R,), float("nan"), device="cuda")
    native.check(lib.aigv_op_lm_head_argmax_logprob(h.data_ptr(), R, H, W.data_ptr(), V, scratch.data_ptr(), nbytes, idx.data_ptr(), val.data_ptr(),
                                                    lp.data_ptr(), native.stream_ptr()))
    return idx, val, lp


def _argmax_cand_logprob(lib, h, W, V, cand):
    R, H = h.shape
    nbytes = lib.aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(R, V)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bits everywhere
    cd = torch.tensor(cand, dtype=torch.long, device="cuda")
    idx = torch.full((R,), -7, dtype=torch.long, device="cuda")
    val = torch.full((R,), float("nan"), device="cuda")
    lp = torch.full((R,), float("nan"), device="cuda")
    clp = torch.full((R, len(cand)), 7.0, device="cuda")
    native.check(lib.aigv_op_lm_head_argmax_cand_logprob(h.data_ptr(), R, H, W.data_ptr(), V, cd.data_ptr(), len(cand), scratch.data_ptr(), nbytes,
                                                         idx.data_ptr(), val.data_ptr(), lp.data_ptr(), clp.data_ptr(), native.stream_ptr()))
    return idx, val, lp, clp


def _store_logits(lib, h, W, V):
    """bf16 logits [R, V] from the skinny GEMM's store form (W padded to a multiple of 4 rows: every column is computed on its own)."""
    R, H = h.shape
    Np = (V + 3) // 4 * 4
    Wp = torch.zeros((Np, H), dtype=BF, device="cuda")
    Wp[:V] = W
    out = torch.full((R, Np), float("nan"), dtype=BF, device="cuda")
    native.check(lib.aigv_op_skinny_gemm(h.data_ptr(), H, R, Wp.data_ptr(), H, Np, H, None, None, 0, out.data_ptr(), Np, 0, native.stream_ptr()))
    return out[:, :V]


@pytest.mark.parametrize("V,H", [(1, 384), (17, 384), (2053, 640), (92553, 512)])
def test_op_lm_head_cand_logprob_holds_the_lm_heads_own_bits(V, H):
    lib = native.load()
    R = 64
    g = torch.Generator(device="cuda").manual_seed(V)
    h = torch.randn((R, H), generator=g, device="cuda").to(BF)
    W = (torch.randn((V, H), generator=g, device="cuda") * 0.05).to(BF)
    idx0, val0, lp0 = _argmax_logprob(lib, h, W, V)
    torch.cuda.synchronize()
    a = min(V - 1, 37)
    # column 0, column V - 1, two columns of one 16-column slab, a duplicate, the argmax of rows 0 and 5, and enough to fill 2 workgroups
    cand = [0, V - 1, a, min(V - 1, a + 1), a, int(idx0[0]), int(idx0[5])] + [(11 * i + 3) % V for i in range(13)]
    idx, val, lp, clp = _argmax_cand_logprob(lib, h, W, V, cand)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx0) and torch.equal(bits(val), bits(val0)) and torch.equal(bits(lp), bits(lp0))
    logits = _store_logits(lib, h, W, V)                              # (R = 64: four row tiles, the 4-slice kernel the argmax forms run)
    lse = val - lp                                                    # exact: val is a bf16 value of the log-sum-exp's magnitude or below
    want = logits[:, cand].float() - lse.view(-1, 1)
    assert torch.equal(bits(clp), bits(want))
    for r in range(R):                                                # the argmax among the candidates: its column IS logprob
        for c, tok in enumerate(cand):
            if tok == int(idx[r]):
                assert torch.equal(bits(clp[r, c:c + 1]), bits(lp[r:r + 1])), (r, c)
    assert torch.equal(bits(clp[0, 5:6]), bits(lp[0:1])) and torch.equal(bits(clp[5, 6:7]), bits(lp[5:6]))
    err = (clp.double() - torch.log_softmax(logits.double(), -1)[:, cand]).abs().max().item()
    print(f"V={V}: max |cand lp - fp64| = {err:.3g}")
    assert err <= 1e-5
    # bits do not depend on the rows in the launch (1, 5, 16, 33 rows: one to three row tiles), on C, or on the order
    for rows in (1, 5, 16, 33):
        i2, v2, l2, c2 = _argmax_cand_logprob(lib, h[:rows].contiguous(), W, V, cand)
        assert torch.equal(i2, idx[:rows]) and torch.equal(bits(l2), bits(lp[:rows])) and torch.equal(bits(c2), bits(clp[:rows])), rows
    _, _, l3, c3 = _argmax_cand_logprob(lib, h, W, V, cand[:3][::-1])
    assert torch.equal(bits(c3), bits(clp[:, [2, 1, 0]])) and torch.equal(bits(l3), bits(lp))
    many = [(5 * i) % V for i in range(64)]
    _, _, _, c4 = _argmax_cand_logprob(lib, h, W, V, many)
    assert torch.equal(bits(c4), bits(logits[:, many].float() - lse.view(-1, 1)))
    # out of range: NaN columns only
    _, _, l5, c5 = _argmax_cand_logprob(lib, h, W, V, [0, V, -1, V - 1])
    assert torch.isnan(c5[:, 1:3]).all() and torch.equal(bits(c5[:, [0, 3]]), bits(clp[:, [0, 1]])) and torch.equal(bits(l5), bits(lp))


# ---- 3. the scoring pass -------------------------------------------------------------------------------------------------------------

CAND = [11, 5, 400, 77, 3]


def _ragged_batch(cfg, seed, T=2):
    """Two clips with different answer lengths, right-padded to one N (labels -100 on the padding), as the training collator does."""
    t0 = synth.canonical_tokens(cfg, 1, T, seed=seed, answer_len=9)
    t1 = synth.canonical_tokens(cfg, 1, T, seed=seed + 1, answer_len=5)
    n = t0["input_ids"].shape[1]
    pad = n - t1["input_ids"].shape[1]
    ids = torch.cat([t0["input_ids"], torch.cat([t1["input_ids"], torch.zeros(1, pad, dtype=torch.long)], 1)])
    labels = torch.cat([t0["labels"], torch.cat([t1["labels"], torch.full((1, pad), -100)], 1)])
    am = torch.ones(2, n, dtype=torch.bool)
    am[1, n - pad:] = False
    return (t0, t1), ids, am, labels, synth.synthetic_frames(2 * T, 224, seed=seed), synth.synthetic_motion(2, cfg.motion_dim, seed=seed)


@pytest.mark.parametrize("stage", [1, 2])
def test_forward_candidates_equal_label_logprobs_and_the_oracle(stage):
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    seed = 17 + stage
    sd = synth.make_state_dict(cfg, seed=seed, rich=True)
    model = make_model(cfg, sd, stage=stage)
    T = 2
    clips, ids, am, labels, pv, motion = _ragged_batch(cfg, seed, T)
    model.img_context_token_id = clips[0]["img_context_token_id"]
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=torch.ones(2 * T, 1, dtype=torch.long), labels=labels, motion_feature=motion)
    off = model(**kw)
    lp_only = model(**kw, return_logprobs=True)
    on = model(**kw, candidate_ids=CAND)
    both = model(**kw, candidate_ids=torch.tensor(CAND), return_logprobs=True)
    torch.cuda.synchronize()
    assert set(on) == set(off) | {"cand_logprob"} and set(both) == set(lp_only) | {"cand_logprob"}
    for k in ("logit", "label") + (("score1",) if stage == 2 else ()):
        assert torch.equal(on[k], off[k]) and torch.equal(both[k], off[k]), k
    assert torch.equal(bits(both["logprob"]), bits(lp_only["logprob"])) and torch.equal(bits(both["ce_loss"].view(1)), bits(lp_only["ce_loss"].view(1)))
    n = ids.shape[1]
    x = on["cand_logprob"]
    assert x.dtype == torch.float32 and x.shape == (2 * (n - 1), len(CAND)) and torch.equal(bits(x), bits(both["cand_logprob"]))
    lab = on["label"].cpu()
    assert torch.equal(torch.isnan(x.cpu()), (lab == -100).view(-1, 1).expand(-1, len(CAND)))
    # column c = the label log-probabilities of the same pass with every answer label replaced by cand[c]
    for c, tok in enumerate(CAND):
        swapped = torch.where(labels != -100, torch.full_like(labels, tok), labels)
        ref = model(**dict(kw, labels=swapped), return_logprobs=True)
        assert torch.equal(bits(ref["logprob"]), bits(x[:, c])), c
    # out of range: a NaN column, the rest as it was
    oor = model(**kw, candidate_ids=[CAND[0], cfg.llm_config.vocab_size, CAND[1]])["cand_logprob"]
    assert torch.isnan(oor[:, 1]).all() and torch.equal(bits(oor[:, [0, 2]]), bits(x[:, [0, 1]]))
    # label rules as return_logprobs, and labels are needed
    bad = labels.clone()
    bad[0, -1] = cfg.llm_config.vocab_size
    with pytest.raises(ValueError, match="outside"):
        model(**dict(kw, labels=bad), candidate_ids=CAND)
    with pytest.raises(ValueError, match="needs labels"):
        model(**dict(kw, labels=None), candidate_ids=CAND)
    # the oracle: log_softmax of its logits at the candidates, bar per row from the two sides' logits
    want = (lab != -100).view(2, n - 1)
    R = int(want.sum())
    nS = 2 if stage == 2 else 0
    model(**kw, candidate_ids=CAND)
    l_hip = model._row_logits(nS + R)[nS:].cpu()
    r = 0
    for b, t in enumerate(clips):
        ref = O.forward_eval(sd, cfg, pv[T * b:T * (b + 1)], t["input_ids"], t["attention_mask"], torch.ones(T, 1, dtype=torch.long),
                             t["labels"], motion[b:b + 1], t["img_context_token_id"], stage=stage, return_intermediates=True)
        nb = t["input_ids"].shape[1]
        sel = ref["label"] != -100
        lo = ref["logits"][0, :-1][sel]
        k = int(sel.sum())
        bar = 2 * (l_hip[r:r + k] - lo).abs().amax(1).double() + 1e-5
        r += k
        lp_o = torch.log_softmax(lo.double(), -1)[:, CAND]
        got = x.cpu().view(2, n - 1, -1)[b, : nb - 1][sel].double()
        d = (got - lp_o).abs()
        print(f"stage {stage} clip {b}: max |cand lp_hip - lp_oracle| = {d.max().item():.3g} ({(d / bar.view(-1, 1)).max().item():.2f} of the bar)")
        assert bool((d <= bar.view(-1, 1)).all())


def test_candidates_are_batch_graph_and_loop_invariant():
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    sd = synth.make_state_dict(cfg, seed=23, rich=True)
    model = make_model(cfg, sd)
    T = 2
    toks = synth.canonical_tokens(cfg, 3, T, seed=23)
    model.img_context_token_id = toks["img_context_token_id"]
    pv = synth.synthetic_frames(3 * T, 224, seed=23).cuda()
    motion = synth.synthetic_motion(3, cfg.motion_dim, seed=23).cuda()
    flags = torch.ones(3 * T, 1, dtype=torch.long)

    def run(b0, b1, frames=pv, cand=CAND, **kw):
        o = model(pixel_values=frames[T * b0:T * b1], input_ids=toks["input_ids"][b0:b1], attention_mask=toks["attention_mask"][b0:b1],
                  image_flags=flags[T * b0:T * b1], labels=toks["labels"][b0:b1], motion_feature=motion[b0:b1], candidate_ids=cand, **kw)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in o.items() if torch.is_tensor(v)}

    n = toks["input_ids"].shape[1]
    alone = run(0, 1)
    batch = run(0, 3)
    assert torch.equal(bits(alone["cand_logprob"]), bits(batch["cand_logprob"][: n - 1]))
    # graph replay: call 1 eager, call 2 captures, calls 3.. replay - other frames AND other candidate values each time, one graph
    frames = [synth.synthetic_frames(3 * T, 224, seed=40 + i).cuda() for i in range(4)]
    cands = [CAND, [9, 8, 7, 6, 5], [300, 2, 41, 41, 0], torch.tensor([1, 2, 3, 4, 499])]
    eager = [run(0, 3, f, c, return_logprobs=True) for f, c in zip(frames, cands)]
    model.enable_graph_replay(True)
    try:
        got = [run(0, 3, f, c, return_logprobs=True) for f, c in zip(frames, cands)]
        held = [k for k, v in model._graphs.items() if isinstance(v, tuple)]
        assert len(held) == 1 and held[0][0][-1] == "candidates" and held[0][1][-1] == ((5,), torch.int64)
        run(0, 3, frames[0], CAND[:3], return_logprobs=True)          # another C: another key
        assert len(model._graphs) == 2
    finally:
        model.enable_graph_replay(False)
    for g, e in zip(got, eager):
        for k in ("cand_logprob", "logprob", "logit", "score1"):
            assert torch.equal(bits(g[k]), bits(e[k])), k
    assert not torch.equal(bits(got[2]["cand_logprob"]), bits(got[3]["cand_logprob"]))
    # the batched loop (k = 3, ragged prompts) against the plain loop
    items = []
    for i, alen in enumerate((9, 4, 12, 6)):
        t = synth.canonical_tokens(cfg, 1, T, seed=50 + i, answer_len=alen)
        items.append({"input_ids": t["input_ids"], "attention_mask": t["attention_mask"], "labels": t["labels"],
                      "image_flags": torch.ones(1, T, 1, dtype=torch.long), "pixel_values": synth.synthetic_frames(T, 224, seed=50 + i).unsqueeze(0),
                      "motion_feature": synth.synthetic_motion(1, cfg.motion_dim, seed=50 + i)})
    looped = list(eval_utils.batched(items, model, k=3, candidate_ids=CAND))
    assert len(looped) == len(items)
    for it, o in looped:
        ref = model(pixel_values=it["pixel_values"][0].cuda(), input_ids=it["input_ids"], attention_mask=it["attention_mask"],
                    image_flags=it["image_flags"][0], labels=it["labels"], motion_feature=it["motion_feature"].cuda(), candidate_ids=CAND)
        assert o["cand_logprob"].shape == ref["cand_logprob"].shape and torch.equal(bits(o["cand_logprob"]), bits(ref["cand_logprob"]))
        assert "logprob" not in o


def test_score_clips_dp_candidates_over_rccl_single_rank():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cand_rccl_single_rank_child.py")], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CAND_DP_OK" in r.stdout


def _level_rig(seed=29):
    """The rig of test_shared_prefix_candidate_answers_rank_like_the_oracle with single-token level words: five candidate answers
    [word, <|im_end|>] behind one prompt."""
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    sd = synth.make_state_dict(cfg, seed=seed, rich=True)
    model = make_model(cfg, sd)
    B, T = 2, 2
    base = synth.canonical_tokens(cfg, B, T, seed=seed, answer_len=1)
    model.img_context_token_id = base["img_context_token_id"]
    n_prompt = int((base["labels"][0] == -100).sum())
    words = torch.randint(3, 500, (16,), generator=torch.Generator().manual_seed(seed)).unique()[:5].tolist()
    assert len(words) == 5
    prompts = []
    for w in words:
        ans = [int(w), int(base["im_end_id"])]
        ids = torch.cat([base["input_ids"][:, :n_prompt], torch.tensor([ans] * B)], 1)
        lab = torch.cat([torch.full((B, n_prompt), -100), torch.tensor([ans] * B)], 1)
        prompts.append((ids, torch.ones_like(ids, dtype=torch.bool), lab))
    kw = dict(pixel_values=synth.synthetic_frames(B * T, 224, seed=seed), image_flags=torch.ones(B * T, 1, dtype=torch.long),
              motion_feature=synth.synthetic_motion(B, cfg.motion_dim, seed=seed))
    return model, cfg, B, n_prompt, words, prompts, kw


def test_shared_prefix_candidates_equal_its_label_logprobs():
    model, cfg, B, n_prompt, words, prompts, kw = _level_rig()
    outs = model.forward_shared_prefix(prompts, **kw, candidate_ids=words, return_logprobs=True)
    plain = model.forward_shared_prefix(prompts, **kw, return_logprobs=True)
    only = model.forward_shared_prefix(prompts, **kw, candidate_ids=words)
    for o, p, q in zip(outs, plain, only):
        assert set(o) == set(p) | {"cand_logprob"} and set(q) == set(o) - {"logprob", "ce_loss"}
        for k in ("logit", "score1", "logprob"):
            assert torch.equal(bits(o[k]), bits(p[k])), k
        assert torch.equal(bits(o["cand_logprob"]), bits(q["cand_logprob"]))
    # separate passes of the same shape with the answer labels replaced by candidate c: its column, bit for bit
    for c, w in enumerate(words):
        swapped = [(ids, am, torch.where(lab != -100, torch.full_like(lab, int(w)), lab)) for ids, am, lab in prompts]
        sep = model.forward_shared_prefix(swapped, **kw, return_logprobs=True)
        for o, s in zip(outs, sep):
            assert torch.equal(bits(s["logprob"]), bits(o["cand_logprob"][:, c])), c


def test_expected_level_in_one_pass_agrees_with_the_five_candidate_recipe():
    """README's graded level.  Recipe: five candidate answers behind one prefix, the level distribution = softmax over the candidates'
    first-answer-token log-probabilities.  One pass: the candidates' columns of ONE answer row.

    (a) Inside the five-candidate pass every prompt's first answer row sees the same tokens; prompt p's row holds the recipe's number for
    candidate p in column p bit for bit (test_shared_prefix_candidates_equal_its_label_logprobs), and the rows of the five prompts are
    required to be the same bits here.  ``expected_level`` then gets identical inputs on both sides: the bound is 0 up to the order of
    the last softmax's operations - asserted as 5 x 2^-22 (five products <= 5, each within two fp32 roundings).
    (b) The README's one pass is a plain ``forward`` - a prefill instead of a continuation over cached keys: other kernels, so other
    logits within their summation order.  A log-softmax moves by at most twice the largest change of its logits, and the expected level
    by at most max |w - E| <= 2 ... 4 times the largest change of a log-probability (dE/dx_c = p_c (w_c - E), sum_c p_c |w_c - E| <= 4):
    bar = 4 (2 max_v |l_forward - l_shared| + 1e-5) + 5 x 2^-22, from the logits the two passes actually produced."""
    model, cfg, B, n_prompt, words, prompts, kw = _level_rig()
    P = len(prompts)
    outs = model.forward_shared_prefix(prompts, **kw, candidate_ids=words, return_logprobs=True)
    R_all = sum(int((lab[:, 1:] != -100).sum()) for _, _, lab in prompts)
    l_shared = model._row_logits(B * P + R_all)[B * P:].cpu()                       # rows: prompt 0 (clip 0: word, end; clip 1: ...), prompt 1, ...
    n1 = prompts[0][0].shape[1] - 1
    row = n_prompt - 1                                                            # the shifted row that predicts the level word
    first = [o["cand_logprob"].view(B, n1, P)[:, row] for o in outs]              # per prompt: [B, 5]
    for p in range(1, P):
        assert torch.equal(bits(first[p]), bits(first[0])), p
    recipe = torch.stack([o["logprob"].view(B, n1)[:, row] for o in outs], -1)    # [B, 5]: candidate p's log-probability from ITS prompt
    assert torch.equal(bits(recipe), bits(first[0]))
    e5 = eval_utils.expected_level(recipe)
    e1 = eval_utils.expected_level(first[0])
    print(f"expected level: recipe {e5.tolist()} one row of the same pass {e1.tolist()}")
    assert (e1.double() - e5.double()).abs().max().item() <= 5 * 2 ** -22
    ids, am, lab = prompts[0]
    fwd = model(input_ids=ids, attention_mask=am, labels=lab, **kw, candidate_ids=words)
    l_fwd = model._row_logits(B + 2 * B)[B:].cpu()                                 # clip b's word row: 2 b
    d_logit = torch.stack([(l_fwd[2 * b] - l_shared[2 * b]).abs().max() for b in range(B)]).double()
    e_fwd = eval_utils.expected_level(fwd["cand_logprob"].view(B, n1, P)[:, row]).cpu().double()
    bar = 4 * (2 * d_logit + 1e-5) + 5 * 2 ** -22
    print(f"expected level: plain forward {e_fwd.tolist()}, |d| {(e_fwd - e5.cpu().double()).abs().tolist()}, bar {bar.tolist()}")
    assert bool(((e_fwd - e5.cpu().double()).abs() <= bar).all())
    assert bool(((e_fwd >= 1) & (e_fwd <= 5)).all())


# ---- 4. generate ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    return make_model(cfg, synth.make_state_dict(cfg, seed=71, rich=True)), cfg


def _prompts(model, cfg, B, seed, ragged=False):
    T = 2
    toks = synth.canonical_tokens(cfg, B, T, seed=seed)
    n_prompt = int((toks["labels"][0] == -100).sum())
    ids = toks["input_ids"][:, :n_prompt].clone()
    ctx = toks["img_context_token_id"]
    for b in range(B):
        ids[b, (ids[b] == ctx).nonzero()[-1]] = 7          # generate() prompts carry no motion slot
    am = torch.ones_like(ids)
    if ragged:                                             # left padding, as batch_chat builds it
        for b in range(1, B):
            am[b, : 2 * b] = 0
    model.img_context_token_id = ctx
    return synth.synthetic_frames(B * T, 224, seed=seed), ids, am


def _ended_mask(seq, eos):
    ended = torch.zeros_like(seq, dtype=torch.bool)
    for b in range(seq.shape[0]):
        hit = [t for t in range(seq.shape[1]) if int(seq[b, t]) in eos]
        if hit:
            ended[b, hit[0] + 1:] = True
    return ended


def _check_greedy(model, pv, ids, am, n_new, cand, eos=None):
    """Greedy generate with candidate_ids: sequences / logprobs as without them (bit for bit); the fused path against an fp64 log-softmax
    of the materialised raw logits (<= 1e-5, the bar of the fused ``logprobs``), the materialised path equal to generation.token_logprobs."""
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=n_new, do_sample=False)
    if eos is not None:
        kw.update(eos_token_id=eos, pad_token_id=2)
    base = model.generate(**kw, return_logprobs=True)
    fused = model.generate(**kw, return_dict_in_generate=True, return_logprobs=True, candidate_ids=cand)
    alone = model.generate(**kw, return_dict_in_generate=True, candidate_ids=torch.tensor(cand))
    mat = model.generate(**kw, return_dict_in_generate=True, output_logits=True, return_logprobs=True, candidate_ids=cand)
    for o in (fused, alone, mat):
        assert isinstance(o, generation.GenerateOutput) and torch.equal(o.sequences, base.sequences)
        assert o.cand_logprobs.shape == base.sequences.shape + (len(cand),) and o.cand_logprobs.dtype == torch.float32
    assert torch.equal(bits(fused.logprobs), bits(base.logprobs)) and alone.logprobs is None and base.cand_logprobs is None
    assert torch.equal(bits(alone.cand_logprobs), bits(fused.cand_logprobs))
    ended = _ended_mask(base.sequences.cpu(), [eos] if isinstance(eos, int) else (eos or []))
    for o in (fused, mat):
        assert torch.equal(torch.isnan(o.cand_logprobs.cpu()), ended.unsqueeze(-1).expand(-1, -1, len(cand)))
    for t, raw in enumerate(mat.logits):
        live = ~ended[:, t]
        for c, tok in enumerate(cand):
            want = generation.token_logprobs(raw, torch.full((raw.shape[0],), tok, device=raw.device))
            assert torch.equal(bits(mat.cand_logprobs[:, t, c])[live], bits(want)[live]), (t, c)
            ref = torch.log_softmax(raw.double(), -1)[:, tok].cpu()
            assert (fused.cand_logprobs[:, t, c].cpu().double() - ref)[live].abs().max().item() <= 1e-5, (t, c)
        # a candidate that is the emitted token carries logprobs, bit for bit
        for b in range(raw.shape[0]):
            for c, tok in enumerate(cand):
                if live[b] and tok == int(base.sequences[b, t]):
                    assert torch.equal(bits(fused.cand_logprobs[b, t, c:c + 1]), bits(fused.logprobs[b, t:t + 1]))
    return base, fused


def test_generate_candidates_fused_ragged_eos_and_batch_invariant(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 3, seed=72, ragged=True)
    plain = model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=9, do_sample=False)
    cand = [11, 5, int(plain[0, 2]), int(plain[1, 0]), 400]             # two of them get emitted
    base, fused = _check_greedy(model, pv, ids, am, 9, cand)
    assert torch.equal(base.sequences, plain)
    eos = int(plain[0, 3])                                              # the first sequence ends mid-run
    _, ragged = _check_greedy(model, pv, ids, am, 9, cand, eos=eos)
    assert bool(torch.isnan(ragged.cand_logprobs[0, 4:]).all()) and not bool(torch.isnan(ragged.cand_logprobs[0, :4]).any())
    for b in (0, 2):                                                    # a sequence's bits do not depend on its batch mates
        keep = am[b].bool()
        one = model.generate(pixel_values=pv[2 * b:2 * b + 2], input_ids=ids[b:b + 1, keep], attention_mask=am[b:b + 1, keep], max_new_tokens=9,
                             do_sample=False, return_dict_in_generate=True, candidate_ids=cand)
        assert torch.equal(one.sequences[0], plain[b]) and torch.equal(bits(one.cand_logprobs[0]), bits(fused.cand_logprobs[b]))
    lvl = eval_utils.expected_level(fused.cand_logprobs)
    assert lvl.shape == plain.shape and bool(((lvl >= 1) & (lvl <= 5)).all())


def test_generate_candidates_in_fp8_mode(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=73)
    model.set_precision("fp8")
    try:
        _check_greedy(model, pv, ids, am, 6, CAND)
    finally:
        model.set_precision("bf16")


def test_generate_candidates_with_processors_sampling_and_beams(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=74)
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=7)
    flags = dict(return_dict_in_generate=True, output_logits=True)
    # repetition penalty: tokens as without candidates; the candidates' distribution is that of the RAW logits
    base = model.generate(**kw, do_sample=False, repetition_penalty=1.3)
    o = model.generate(**kw, do_sample=False, repetition_penalty=1.3, **flags, candidate_ids=CAND)
    assert torch.equal(o.sequences, base)
    for t in range(base.shape[1]):
        assert torch.equal(bits(o.cand_logprobs[:, t]), bits(generation.candidate_logprobs(o.logits[t], torch.tensor(CAND))))
    samp = dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.8)
    base = model.generate(**kw, **samp, generator=torch.Generator(device=model.device).manual_seed(11))
    o = model.generate(**kw, **samp, generator=torch.Generator(device=model.device).manual_seed(11), **flags, candidate_ids=CAND)
    assert torch.equal(o.sequences, base)
    for t in range(base.shape[1]):
        for c, tok in enumerate(CAND):
            assert torch.equal(o.cand_logprobs[:, t, c], generation.token_logprobs(o.logits[t], torch.full((2,), tok, device=model.device)))
    with pytest.raises(NotImplementedError, match="candidate_ids"):
        model.generate(**kw, do_sample=False, num_beams=3, return_dict_in_generate=True, candidate_ids=CAND)
    beams = model.generate(**kw, do_sample=False, num_beams=3)          # without them: as before
    assert torch.is_tensor(beams)


def test_generate2_and_generate_stage2_carry_the_candidates(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=76)
    emb = model.language_model.get_input_embeddings().weight[ids.cuda()]
    base = model.generate2(emb, max_new_tokens=5, do_sample=False)
    o = model.generate2(emb, max_new_tokens=5, do_sample=False, return_dict_in_generate=True, output_logits=True, candidate_ids=CAND)
    f = model.generate2(emb, max_new_tokens=5, do_sample=False, return_dict_in_generate=True, candidate_ids=CAND)
    ref = torch.stack([torch.log_softmax(l.double(), -1)[:, CAND] for l in o.logits], 1)
    assert torch.equal(o.sequences, base) and torch.equal(f.sequences, base)
    assert (f.cand_logprobs.double() - ref).abs().max().item() <= 1e-5 and (o.cand_logprobs.double() - ref).abs().max().item() <= 1e-5
    toks = synth.canonical_tokens(cfg, 2, 2, seed=77)
    n_prompt = int((toks["labels"][0] == -100).sum())
    sids, sam = toks["input_ids"][:, :n_prompt], toks["attention_mask"][:, :n_prompt]
    spv = synth.synthetic_frames(4, 224, seed=77)
    motion = synth.synthetic_motion(2, cfg.motion_dim, seed=77)
    model.img_context_token_id = toks["img_context_token_id"]
    flags_ = torch.ones(4, 1, dtype=torch.long)
    base = model.generate_stage2(spv, sids, sam, flags_, motion, max_new_tokens=5, do_sample=False)
    o = model.generate_stage2(spv, sids, sam, flags_, motion, max_new_tokens=5, do_sample=False, generation_config=dict(
        return_dict_in_generate=True, output_logits=True))
    f = model.generate_stage2(spv, sids, sam, flags_, motion, max_new_tokens=5, do_sample=False, return_dict_in_generate=True, candidate_ids=CAND)
    ref = torch.stack([torch.log_softmax(l.double(), -1)[:, CAND] for l in o.logits], 1)
    assert torch.equal(f.sequences, base) and (f.cand_logprobs.double() - ref).abs().max().item() <= 1e-5
