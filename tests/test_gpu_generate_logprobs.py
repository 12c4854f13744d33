"""Per-token log-probabilities and HF's ``return_dict_in_generate`` outputs of generate() (MI355X only).

Op level: ``aigv_op_lm_head_argmax_logprob`` (the decode step's lm-head with the log-sum-exp fused into its argmax) against
``aigv_op_lm_head_argmax`` (idx / val bit for bit, planted ties included) and an fp64 log-softmax of the logits that the store form of
the same GEMV (``aigv_op_skinny_gemm``, epilogue 0, no bias) writes - first checked to hold ``val`` at ``idx`` bit for bit, so the two
forms round every column alike and the bar is the plain 1e-5 of ``aigv_op_label_logprob``.  The hidden widths are chosen so that the
store form runs the 4-slice kernel the argmax forms run (K % 256 != 0 or more than 256 workgroups).

Model level: greedy / processed / sampled / beam generate() with the flags against the flagless call and against the logits the loop
materialises, generate2 / generate_stage2, fp8 mode, and ``score_clips_dp(return_logprobs=True)`` against ``forward``."""
import math

import pytest
import torch

import aigv_assessor_amd as pkg
from aigv_assessor_amd import dist_utils, generation, native, synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _argmax_logprob(lib, h, W, V, rows=None):
    R = h.shape[0] if rows is None else rows
    H = h.shape[1]
    nbytes = lib.aigv_op_lm_head_argmax_logprob_scratch_bytes(R, V)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bits everywhere
    idx = torch.full((R,), -7, dtype=torch.long, device="cuda")
    val = torch.full((R,), float("nan"), device="cuda")
    lp = torch.full((R,), float("nan"), device="cuda")
    native.check(lib.aigv_op_lm_head_argmax_logprob(h.data_ptr(), R, H, W.data_ptr(), V, scratch.data_ptr(), nbytes, idx.data_ptr(),
                                                    val.data_ptr(), lp.data_ptr(), native.stream_ptr()))
    return idx, val, lp


def _argmax(lib, h, W, V):
    R, H = h.shape
    packed = torch.zeros(64, dtype=torch.long, device="cuda")
    idx = torch.full((R,), -7, dtype=torch.long, device="cuda")
    val = torch.full((R,), float("nan"), device="cuda")
    native.check(lib.aigv_op_lm_head_argmax(h.data_ptr(), R, H, W.data_ptr(), V, packed.data_ptr(), idx.data_ptr(), val.data_ptr(),
                                            native.stream_ptr()))
    return idx, val


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
def test_op_argmax_logprob_against_argmax_and_fp64(V, H):
    lib = native.load()
    R = 64
    g = torch.Generator(device="cuda").manual_seed(V)
    h = torch.randn((R, H), generator=g, device="cuda").to(BF)
    W = (torch.randn((V, H), generator=g, device="cuda") * 0.05).to(BF)
    if V >= 17:                                    # planted ties: two identical dominant columns for rows 0 and 1, the first must win
        a, b = (3, 11) if V == 17 else (100, V - 5)
        W[a] = W[b] = (h[0].float() * 0.02).to(BF)
        c, d = (1, 16) if V == 17 else (16, 31)    # (another pair, in the same / next 16-column slab)
        W[c] = W[d] = (h[1].float() * 0.02).to(BF)
    idx, val, lp = _argmax_logprob(lib, h, W, V)
    ai, av = _argmax(lib, h, W, V)
    torch.cuda.synchronize()
    assert torch.equal(idx, ai) and torch.equal(bits(val), bits(av))
    if V >= 17:
        assert int(idx[0]) == a and int(idx[1]) == c
    logits = _store_logits(lib, h, W, V)
    got_val = logits.gather(1, idx.view(-1, 1)).view(-1)
    assert torch.equal(bits(got_val), bits(val))                   # the store form rounds the chosen column alike
    want = torch.log_softmax(logits.double(), -1).gather(1, idx.view(-1, 1)).view(-1)
    err = (lp.double() - want).abs().max().item()
    print(f"V={V}: max |lp - fp64| = {err:.3g}")
    assert err <= 1e-5
    if V == 1:
        assert torch.equal(lp.cpu(), torch.zeros(R))
    # a row alone gives the bits it gets among 64, and a repeated call the same bits
    for r in (0, 1, 2, 17, 63):
        i1, v1, l1 = _argmax_logprob(lib, h[r:r + 1].contiguous(), W, V)
        assert int(i1) == int(idx[r]) and torch.equal(bits(v1), bits(val[r:r + 1])) and torch.equal(bits(l1), bits(lp[r:r + 1]))
    for rows in (5, 16, 33):
        i2, v2, l2 = _argmax_logprob(lib, h[:rows].contiguous(), W, V)
        assert torch.equal(i2, idx[:rows]) and torch.equal(bits(l2), bits(lp[:rows]))
    i3, v3, l3 = _argmax_logprob(lib, h, W, V)
    assert torch.equal(i3, idx) and torch.equal(bits(l3), bits(lp))


@pytest.mark.parametrize("V", [1, 17, 2053, 92553])
def test_op_argmax_logprob_edge_values(V):
    lib = native.load()
    H, R = 256, 8
    g = torch.Generator(device="cuda").manual_seed(3 + V)
    h = torch.randn((R, H), generator=g, device="cuda").to(BF)
    same = torch.randn((1, H), generator=g, device="cuda").to(BF).expand(V, H).contiguous()   # identical rows: -log V
    idx, val, lp = _argmax_logprob(lib, h, same, V)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), torch.zeros(R, dtype=torch.long))
    assert (lp.double().cpu() + math.log(V)).abs().max().item() <= 1e-5
    if V == 1:
        assert torch.equal(lp.cpu(), torch.zeros(R))
    W = (torch.randn((V, H), generator=g, device="cuda") * 0.05).to(BF)
    col = V // 2
    W[col] = (h[2].float() * 0.5).to(BF)           # a dominant column for row 2
    idx, val, lp = _argmax_logprob(lib, h, W, V)
    torch.cuda.synchronize()
    assert int(idx[2]) == col and -1e-5 <= float(lp[2]) <= 0.0


# ---- model level ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    from aigv_assessor_amd.modeling import InternVLChatModel
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    sd = synth.make_state_dict(cfg, seed=71, rich=True)
    model = InternVLChatModel(cfg)
    model.load_state_dict(sd)
    model.eval().cuda()
    return model, cfg


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


def _ref_logprobs(out):
    """fp64 log_softmax of the materialised raw logits at the emitted tokens, NaN after each sequence's end (from the lp NaN mask)."""
    cols = [torch.log_softmax(l.double(), -1).gather(1, out.sequences[:, t].view(-1, 1)).view(-1) for t, l in enumerate(out.logits)]
    return torch.stack(cols, 1)


def _ended_mask(seq, eos):
    ended = torch.zeros_like(seq, dtype=torch.bool)
    for b in range(seq.shape[0]):
        hit = [t for t in range(seq.shape[1]) if int(seq[b, t]) in eos]
        if hit:
            ended[b, hit[0] + 1:] = True
    return ended


def _check_greedy(model, pv, ids, am, n_new, eos=None):
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=n_new, do_sample=False)
    if eos is not None:
        kw.update(eos_token_id=eos, pad_token_id=2)
    base = model.generate(**kw)
    assert torch.is_tensor(base)
    fused = model.generate(**kw, return_logprobs=True)
    mat = model.generate(**kw, return_dict_in_generate=True, output_logits=True, return_logprobs=True)
    assert isinstance(fused, generation.GenerateOutput) and torch.equal(fused.sequences, base) and torch.equal(mat.sequences, base)
    assert fused.logprobs.shape == base.shape and fused.logprobs.dtype == torch.float32 and len(mat.logits) == base.shape[1]
    ref = _ref_logprobs(mat)
    ended = _ended_mask(base.cpu(), [eos] if isinstance(eos, int) else (eos or []))
    for lp in (fused.logprobs, mat.logprobs):
        lp = lp.cpu()
        assert torch.equal(torch.isnan(lp), ended)
        err = (lp[~ended].double() - ref.cpu()[~ended]).abs().max().item()
        assert err <= 1e-5, err
    return base, fused


def test_greedy_logprobs_fused_ragged_eos_and_batch_invariant(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 3, seed=72, ragged=True)
    base, fused = _check_greedy(model, pv, ids, am, 9)
    eos = int(base[0, 3])                                   # the first sequence ends mid-run
    seq, _ = _check_greedy(model, pv, ids, am, 9, eos=eos)
    assert bool(torch.isnan(model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=9, do_sample=False,
                                           eos_token_id=eos, pad_token_id=2, return_logprobs=True).logprobs[0, 4:]).all())
    # a sequence's bits do not depend on its batch mates
    for b in (0, 2):
        keep = am[b].bool()
        one = model.generate(pixel_values=pv[2 * b:2 * b + 2], input_ids=ids[b:b + 1, keep], attention_mask=am[b:b + 1, keep],
                             max_new_tokens=9, do_sample=False, return_logprobs=True)
        assert torch.equal(one.sequences[0], base[b]) and torch.equal(bits(one.logprobs[0]), bits(fused.logprobs[b]))


def test_greedy_logprobs_in_fp8_mode(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=73)
    model.set_precision("fp8")
    try:
        _check_greedy(model, pv, ids, am, 6)
    finally:
        model.set_precision("bf16")


def test_scores_and_logits_with_processors_and_sampling(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=74)
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=7)
    flags = dict(return_dict_in_generate=True, output_scores=True, output_logits=True, return_logprobs=True)
    # repetition penalty: the processed scores the loop chose from
    base = model.generate(**kw, do_sample=False, repetition_penalty=1.3)
    o = model.generate(**kw, do_sample=False, repetition_penalty=1.3, **flags)
    assert torch.equal(o.sequences, base) and len(o.scores) == len(o.logits) == base.shape[1]
    pen = model._repetition_penalty(1.3)
    for t in range(base.shape[1]):
        assert torch.equal(o.scores[t], pen(base[:, :t], o.logits[t]))
        assert torch.equal(o.scores[t].argmax(-1), base[:, t])
        assert torch.equal(o.logprobs[:, t], generation.token_logprobs(o.scores[t], base[:, t]))
    raw = model.generate(**kw, do_sample=False, return_dict_in_generate=True, output_logits=True)
    assert torch.equal(raw.logits[0], o.logits[0])          # the first step's logits do not depend on the processors
    # sampling under a fixed generator: same draws with and without the flags; scores = the warped logits
    samp = dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.8)
    g = torch.Generator(device=model.device).manual_seed(11)
    base = model.generate(**kw, **samp, generator=g)
    g = torch.Generator(device=model.device).manual_seed(11)
    o = model.generate(**kw, **samp, generator=g, **flags)
    assert torch.equal(o.sequences, base)
    for t in range(base.shape[1]):
        assert torch.equal(o.scores[t], model._warp(o.logits[t], 0.8, 5, 0.9))
        assert torch.isfinite(o.logprobs[:, t]).all()
        assert torch.equal(o.logprobs[:, t], generation.token_logprobs(o.scores[t], base[:, t]))


def test_beam_search_sequences_scores_and_refusals(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=75)
    n_new, lp_pen = 6, 0.7
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=n_new, do_sample=False, num_beams=3, length_penalty=lp_pen)
    base = model.generate(**kw)
    o = model.generate(**kw, return_dict_in_generate=True)
    assert torch.equal(o.sequences, base) and set(o) == {"sequences", "sequences_scores"} and o.sequences_scores.shape == (2,)
    # HF's formula over the returned tokens: sum of log_softmax(logits) along the hypothesis / length ** length_penalty (no end token
    # here: every hypothesis runs to max_new_tokens); the logits along it from a greedy run forced onto those tokens
    seq = base

    def force(hist, logits):
        out = torch.full_like(logits, float("-inf"))
        out[torch.arange(logits.shape[0]), seq[:, hist.shape[1]].to(logits.device)] = 0
        return out

    from aigv_assessor_amd.modeling import InternVLChatModel
    orig = InternVLChatModel.__dict__["_gen_args"]
    try:
        InternVLChatModel._gen_args = staticmethod(lambda c, k: orig.__func__(c, k)[:4] + ([force], None))
        forced = model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=n_new, do_sample=False,
                                return_dict_in_generate=True, output_logits=True)
    finally:
        InternVLChatModel._gen_args = orig
    assert torch.equal(forced.sequences, seq)
    total = sum(torch.log_softmax(l.float(), -1).gather(1, seq[:, t].view(-1, 1)).view(-1) for t, l in enumerate(forced.logits))
    want = total / float(seq.shape[1] ** lp_pen)
    assert torch.allclose(o.sequences_scores, want, atol=1e-4, rtol=0), (o.sequences_scores, want)
    for k in ("output_scores", "output_logits", "return_logprobs"):
        with pytest.raises(NotImplementedError, match=k):
            model.generate(**kw, return_dict_in_generate=True, **{k: True})


def test_generate2_and_generate_stage2_carry_the_outputs(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=76)
    emb = model.language_model.get_input_embeddings().weight[ids.cuda()]
    base = model.generate2(emb, max_new_tokens=5, do_sample=False)
    o = model.generate2(emb, max_new_tokens=5, do_sample=False, return_dict_in_generate=True, output_logits=True, return_logprobs=True)
    assert torch.equal(o.sequences, base)
    assert (o.logprobs.double() - _ref_logprobs(o)).abs().max().item() <= 1e-5
    f = model.generate2(emb, max_new_tokens=5, do_sample=False, return_logprobs=True)
    assert torch.equal(f.sequences, base) and (f.logprobs.double() - _ref_logprobs(o)).abs().max().item() <= 1e-5
    # stage 2: the motion slot stays in the prompt
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
    f = model.generate_stage2(spv, sids, sam, flags_, motion, max_new_tokens=5, do_sample=False, return_logprobs=True)
    assert torch.equal(o.sequences, base) and torch.equal(f.sequences, base)
    assert (f.logprobs.double() - _ref_logprobs(o)).abs().max().item() <= 1e-5


def test_score_clips_dp_logprobs_equal_forward(rig):
    model, cfg = rig
    B, T = 2, 2
    toks = synth.canonical_tokens(cfg, B, T, seed=78)
    pv = synth.synthetic_frames(B * T, 224, seed=78)
    motion = synth.synthetic_motion(B, cfg.motion_dim, seed=78)
    flags_ = torch.ones(B * T, 1, dtype=torch.long)
    model.img_context_token_id = toks["img_context_token_id"]
    args = (pv, toks["input_ids"], toks["attention_mask"], flags_, toks["labels"], motion)
    want = model(pixel_values=pv, input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags_,
                 labels=toks["labels"], motion_feature=motion, return_logprobs=True)
    plain = dist_utils.score_clips_dp(model, *args)
    assert "logprob" not in plain and "ce_loss" not in plain
    runs = [dist_utils.score_clips_dp(model, *args, return_logprobs=True)]
    model.enable_graph_replay(True)                 # eager, captured on the second call, replayed from the third
    try:
        runs += [dist_utils.score_clips_dp(model, *args, return_logprobs=True) for _ in range(3)]
    finally:
        model.enable_graph_replay(False)
    for got in runs:
        assert torch.equal(bits(got["logprob"]), bits(want["logprob"]))
        assert torch.equal(bits(got["ce_loss"].view(1)), bits(want["ce_loss"].view(1)))
        assert torch.equal(got["logit"], want["logit"])
