"""Label log-probabilities and the cross-entropy loss of the scoring pass (``return_logprobs=True``; MI355X only): the
``aigv_op_label_logprob`` kernel against an fp64 log-softmax, the whole pass against the CPU oracle's logits (the reference's
``CrossEntropyLoss()(shift_logits, shift_labels)``, internvl_chat_eval2/modeling_internvl_chat.py:452-463), and the invariances the
scorer promises: batch mates, graph replay, the batched loop and the shared-prefix path.

Oracle bar, per consumed row: |lp_hip - lp_oracle| <= 2 max_v |l_hip - l_oracle| + 1e-5 - a log-softmax moves by at most twice the
largest change of its logits, so the bar follows from the logits the two sides actually produced."""
import math

import pytest
import torch

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def make_model(cfg, sd, stage=2):
    from aigv_assessor_amd.modeling import InternVLChatModel
    m = InternVLChatModel(cfg, stage=stage)
    m.load_state_dict(sd)
    return m.eval().cuda()


def bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def lp_fp64(logits, labels):
    """fp64 log_softmax(logits)[label] per row, NaN where the label is outside [0, V)."""
    V = logits.shape[-1]
    ok = (labels >= 0) & (labels < V)
    lp = torch.log_softmax(logits.double(), -1).gather(1, labels.clamp(0, V - 1).view(-1, 1)).view(-1)
    return torch.where(ok, lp, torch.full_like(lp, float("nan")))


@pytest.mark.parametrize("V", [1, 515, 2053, 92553])
def test_op_label_logprob_against_fp64_and_batch_invariant(V):
    lib = native.load()
    R = 64
    for ldo in sorted({V, (V + 3) // 4 * 4, (V + 3) // 4 * 4 + 8}):      # unaligned rows (scalar loads), aligned, padded
        g = torch.Generator().manual_seed(V + ldo)
        x = (torch.randn(R, ldo, generator=g) * 3).to(BF)
        x[:, V:] = 100.0                                                   # padding columns must not count
        labels = torch.randint(0, V, (R,), generator=g)
        labels[0], labels[1], labels[2], labels[3], labels[4] = 0, V - 1, -100, V, -1
        xd, ld = x.cuda(), labels.cuda()
        out = torch.empty(R, dtype=torch.float32, device="cuda")
        native.check(lib.aigv_op_label_logprob(xd.data_ptr(), R, V, ldo, ld.data_ptr(), out.data_ptr(), native.stream_ptr()))
        one = torch.empty(R, dtype=torch.float32, device="cuda")
        for r in range(R):                                                 # each row alone, same bits as inside the 64-row batch
            native.check(lib.aigv_op_label_logprob(xd[r].data_ptr(), 1, V, ldo, ld[r:r + 1].data_ptr(), one[r:r + 1].data_ptr(),
                                                   native.stream_ptr()))
        torch.cuda.synchronize()
        got = out.cpu()
        want = lp_fp64(x[:, :V].float(), labels)
        valid = (labels >= 0) & (labels < V)
        assert torch.equal(torch.isnan(got), ~valid)
        err = (got[valid].double() - want[valid]).abs().max().item()
        print(f"V={V} ldo={ldo}: max |lp - fp64| = {err:.3g}")
        assert err <= 1e-5
        assert torch.equal(bits(one), bits(out))
        if V == 1:
            assert float(got[0]) == 0.0


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
    pv = synth.synthetic_frames(2 * T, 224, seed=seed)
    motion = synth.synthetic_motion(2, cfg.motion_dim, seed=seed)
    return (t0, t1), ids, am, labels, pv, motion


@pytest.mark.parametrize("stage", [1, 2])
def test_logprob_and_ce_loss_against_the_oracle(stage):
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    seed = 17 + stage
    sd = synth.make_state_dict(cfg, seed=seed, rich=True)
    model = make_model(cfg, sd, stage=stage)
    T = 2
    clips, ids, am, labels, pv, motion = _ragged_batch(cfg, seed, T)
    model.img_context_token_id = clips[0]["img_context_token_id"]
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=torch.ones(2 * T, 1, dtype=torch.long), labels=labels,
              motion_feature=motion)
    off = model(**kw)
    on = model(**kw, return_logprobs=True)
    torch.cuda.synchronize()
    # the flag changes nothing that was there and adds exactly two keys
    assert set(on) == set(off) | {"logprob", "ce_loss"} and "logprob" not in off and "ce_loss" not in off
    for k in ("logit", "label") + (("score1",) if stage == 2 else ()):
        assert torch.equal(on[k], off[k]), k
    n = ids.shape[1]
    lab = on["label"].cpu()
    lp = on["logprob"].cpu()
    assert lp.dtype == torch.float32 and lp.shape == (2 * (n - 1),) and on["ce_loss"].dim() == 0
    assert torch.equal(torch.isnan(lp), lab == -100)
    want = (lab != -100).view(2, n - 1)
    R = int(want.sum())
    nS = 2 if stage == 2 else 0
    l_hip = model._row_logits(nS + R)[nS:].cpu()                           # [R, V] in the order of the consumed rows
    r = 0
    lp_or, bound = [], []
    for b, t in enumerate(clips):
        ref = O.forward_eval(sd, cfg, pv[T * b:T * (b + 1)], t["input_ids"], t["attention_mask"], torch.ones(T, 1, dtype=torch.long),
                             t["labels"], motion[b:b + 1], t["img_context_token_id"], stage=stage, return_intermediates=True)
        nb = t["input_ids"].shape[1]
        sel = ref["label"] != -100
        lo = ref["logits"][0, :-1][sel]                                     # the reference's fp32-upcast bf16 logits of the answer rows
        k = int(sel.sum())
        assert torch.equal(want[b, : nb - 1], sel)
        lh = l_hip[r:r + k]
        r += k
        d_logit = (lh - lo).abs().amax(1).double()
        lp_o = lp_fp64(lo, ref["label"][sel])
        got = lp.view(2, n - 1)[b, : nb - 1][sel].double()
        worst = ((got - lp_o).abs() / (2 * d_logit + 1e-5)).max().item()
        print(f"stage {stage} clip {b}: max |lp_hip - lp_oracle| = {(got - lp_o).abs().max().item():.3g} ({worst:.2f} of the bar)")
        assert bool(((got - lp_o).abs() <= 2 * d_logit + 1e-5).all())
        lp_or.append(lp_o)
        bound.append(2 * d_logit + 1e-5)
    lp_or, bound = torch.cat(lp_or), torch.cat(bound)
    ce_or = -lp_or.mean()
    ce = float(on["ce_loss"])
    print(f"ce_loss hip {ce:.6f} oracle {ce_or.item():.6f}")
    assert abs(ce - ce_or.item()) <= bound.mean().item() + 1e-6
    assert abs(ce - (-lp[lab != -100]).double().mean().float().item()) <= math.ulp(ce)


def test_no_label_rows_give_a_nan_loss_and_bad_labels_raise():
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=1)
    sd = synth.make_state_dict(cfg, seed=5, rich=True)
    model = make_model(cfg, sd)
    toks = synth.canonical_tokens(cfg, 1, 2, seed=5)
    model.img_context_token_id = toks["img_context_token_id"]
    kw = dict(pixel_values=synth.synthetic_frames(2, 224, seed=5), input_ids=toks["input_ids"], attention_mask=toks["attention_mask"],
              image_flags=torch.ones(2, 1, dtype=torch.long), motion_feature=synth.synthetic_motion(1, cfg.motion_dim, seed=5))
    out = model(**kw, labels=torch.full_like(toks["labels"], -100), return_logprobs=True)
    assert torch.isnan(out["ce_loss"]).item() and torch.isnan(out["logprob"]).all()
    bad = toks["labels"].clone()
    bad[0, -1] = cfg.llm_config.vocab_size
    with pytest.raises(ValueError, match="outside"):
        model(**kw, labels=bad, return_logprobs=True)
    model(**kw, labels=bad)                                                 # without the flag: as before (the label is never read)


def test_logprob_is_batch_graph_and_loop_invariant():
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    sd = synth.make_state_dict(cfg, seed=23, rich=True)
    model = make_model(cfg, sd)
    T = 2
    toks = synth.canonical_tokens(cfg, 3, T, seed=23)
    model.img_context_token_id = toks["img_context_token_id"]
    pv = synth.synthetic_frames(3 * T, 224, seed=23).cuda()
    motion = synth.synthetic_motion(3, cfg.motion_dim, seed=23).cuda()
    flags = torch.ones(3 * T, 1, dtype=torch.long)

    def run(b0, b1, frames=pv):
        o = model(pixel_values=frames[T * b0:T * b1], input_ids=toks["input_ids"][b0:b1], attention_mask=toks["attention_mask"][b0:b1],
                  image_flags=flags[T * b0:T * b1], labels=toks["labels"][b0:b1], motion_feature=motion[b0:b1], return_logprobs=True)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in o.items() if torch.is_tensor(v)}

    n = toks["input_ids"].shape[1]
    alone = run(0, 1)
    batch = run(0, 3)
    assert torch.equal(bits(alone["logprob"]), bits(batch["logprob"][: n - 1]))
    # graph replay: call 1 eager, call 2 captures, call 3 replays - every call the eager bits; different frames each time
    frames = [synth.synthetic_frames(3 * T, 224, seed=40 + i).cuda() for i in range(3)]
    eager = [run(0, 3, f) for f in frames]
    model.enable_graph_replay(True)
    try:
        got = [run(0, 3, f) for f in frames]
        assert any(isinstance(v, tuple) for v in model._graphs.values())
        assert any(k[0][-1] == "logprobs" for k in model._graphs)
    finally:
        model.enable_graph_replay(False)
    for g, e in zip(got, eager):
        for k in ("logprob", "ce_loss", "logit", "score1"):
            assert torch.equal(bits(g[k]), bits(e[k])), k
    # the batched loop (k = 3, ragged prompts) against the plain loop
    items = []
    for i, alen in enumerate((9, 4, 12, 6)):
        t = synth.canonical_tokens(cfg, 1, T, seed=50 + i, answer_len=alen)
        items.append({"input_ids": t["input_ids"], "attention_mask": t["attention_mask"], "labels": t["labels"],
                      "image_flags": torch.ones(1, T, 1, dtype=torch.long),
                      "pixel_values": synth.synthetic_frames(T, 224, seed=50 + i).unsqueeze(0),
                      "motion_feature": synth.synthetic_motion(1, cfg.motion_dim, seed=50 + i)})
    looped = list(eval_utils.batched(items, model, k=3, return_logprobs=True))
    assert len(looped) == len(items)
    for it, o in looped:
        ref = model(pixel_values=it["pixel_values"][0].cuda(), input_ids=it["input_ids"], attention_mask=it["attention_mask"],
                    image_flags=it["image_flags"][0], labels=it["labels"], motion_feature=it["motion_feature"].cuda(), return_logprobs=True)
        assert o["logprob"].shape == ref["logprob"].shape
        assert torch.equal(bits(o["logprob"]), bits(ref["logprob"]))
        a, b = float(o["ce_loss"]), float(ref["ce_loss"])
        assert abs(a - b) <= math.ulp(b), (a, b)


def test_shared_prefix_candidate_answers_rank_like_the_oracle():
    """Five candidate answers behind ONE video prefix (forward_shared_prefix): each prompt's logprob is that of its separate full pass
    within the oracle bar (with the two passes' logits in place of hip / oracle), and the candidates' summed answer log-likelihoods rank
    like the oracle's wherever the oracle's margin exceeds that bar."""
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    seed = 29
    sd = synth.make_state_dict(cfg, seed=seed, rich=True)
    model = make_model(cfg, sd)
    B, T = 2, 2
    base = synth.canonical_tokens(cfg, B, T, seed=seed, answer_len=1)
    model.img_context_token_id = base["img_context_token_id"]
    n_prompt = int((base["labels"][0] == -100).sum())
    g = torch.Generator().manual_seed(seed)
    prompts = []
    for c in range(5):                                                    # candidate answers of 1-3 tokens + <|im_end|>
        ans = torch.randint(3, 500, (1 + c % 3,), generator=g).tolist() + [int(base["im_end_id"])]
        ids = torch.cat([base["input_ids"][:, :n_prompt], torch.tensor([ans] * B)], 1)
        lab = torch.cat([torch.full((B, n_prompt), -100), torch.tensor([ans] * B)], 1)
        prompts.append((ids, torch.ones_like(ids, dtype=torch.bool), lab))
    pv = synth.synthetic_frames(B * T, 224, seed=seed)
    motion = synth.synthetic_motion(B, cfg.motion_dim, seed=seed)
    flags = torch.ones(B * T, 1, dtype=torch.long)
    outs = model.forward_shared_prefix(prompts, pixel_values=pv, image_flags=flags, motion_feature=motion, return_logprobs=True)
    R_all = sum(int((lab[:, 1:] != -100).sum()) for _, _, lab in prompts)
    l_shared = model._row_logits(B * len(prompts) + R_all)[B * len(prompts):].cpu()
    off = 0
    hip_sum, or_sum, or_bar = torch.zeros(5, B, dtype=torch.float64), torch.zeros(5, B, dtype=torch.float64), torch.zeros(5, B, dtype=torch.float64)
    for c, ((ids, am, lab), got) in enumerate(zip(prompts, outs)):
        assert set(got) >= {"logprob", "ce_loss"}
        sep = model(pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=flags, labels=lab, motion_feature=motion, return_logprobs=True)
        want = lab[:, 1:] != -100
        R = int(want.sum())
        l_sep = model._row_logits(B + R)[B:].cpu()
        bar = 2 * (l_shared[off:off + R] - l_sep).abs().amax(1).double() + 1e-5
        off += R
        a, s = got["logprob"].cpu()[want.reshape(-1)].double(), sep["logprob"].cpu()[want.reshape(-1)].double()
        assert torch.equal(torch.isnan(got["logprob"].cpu()), ~want.reshape(-1))
        assert bool(((a - s).abs() <= bar).all()), ((a - s).abs().max(), bar.min())
        ref = O.forward_eval(sd, cfg, pv, ids, am, flags, lab, motion, base["img_context_token_id"], stage=2, return_intermediates=True)
        sel = ref["label"] != -100
        lo = ref["logits"][:, :-1].reshape(-1, ref["logits"].shape[-1])[sel]
        lp_o = lp_fp64(lo, ref["label"][sel])
        bar_o = 2 * (l_sep - lo).abs().amax(1).double() + 1e-5
        per_clip = want.sum(1).tolist()
        for b, (x, y, z) in enumerate(zip(a.split(per_clip), lp_o.split(per_clip), bar_o.split(per_clip))):
            hip_sum[c, b] = torch.nansum(got["logprob"].cpu().view(B, -1)[b].double())
            assert abs(hip_sum[c, b] - x.sum()) < 1e-9
            or_sum[c, b] = y.sum()
        # bar of the shared-prefix sum against the oracle's: shared vs separate pass + separate pass vs oracle, summed over the answer rows
        or_bar[c] = torch.stack([(u + v).sum() for u, v in zip(bar.split(per_clip), bar_o.split(per_clip))])
    checked = 0
    for b in range(B):
        for i in range(5):
            for j in range(i + 1, 5):
                margin = abs(or_sum[i, b] - or_sum[j, b])
                if margin > or_bar[i, b] + or_bar[j, b]:
                    checked += 1
                    assert (hip_sum[i, b] > hip_sum[j, b]) == (or_sum[i, b] > or_sum[j, b]), (b, i, j)
    print(f"candidate pairs ranked against the oracle: {checked} of {B * 10}")
    # the README's expected level: softmax over the candidates' log-likelihoods
    p = torch.softmax(hip_sum.t(), -1)
    assert torch.allclose(p.sum(-1), torch.ones(B, dtype=torch.float64))
