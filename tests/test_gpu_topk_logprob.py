"""Top-k log-probabilities (``top_logprobs=k``; MI355X only): what the model preferred at a row, selected on the device.

The rule, everywhere: entry j is the j-th largest bf16 lm-head logit, equal logits by ascending token id - the order of the lm-head's
packed argmax key - so ``torch.sort(logits.float(), descending=True, stable=True)`` on the same bf16 logits states it exactly, and
``top_logprob[j] = float(logit) - lse(row)`` with the log-sum-exp the label / candidate kernels use: every column is compared bit for bit
with ``aigv_op_cand_logprob`` / ``aigv_op_label_logprob`` (scoring form) and ``aigv_op_lm_head_argmax_cand_logprob`` (decode form) fed the
selected ids, and within 1e-5 of an fp64 log-softmax (the bar tests/test_gpu_logprob.py applies to this arithmetic)."""
import os
import subprocess
import sys

import pytest
import torch

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, generation, native, synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")


def bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def stable_topk(logits, k):
    return torch.sort(logits.float(), dim=-1, descending=True, stable=True).indices[..., :k]


def make_model(cfg, sd, stage=2):
    from aigv_assessor_amd.modeling import InternVLChatModel
    m = InternVLChatModel(cfg, stage=stage)
    m.load_state_dict(sd)
    return m.eval().cuda()


# ---- 1. the scoring pass's operator --------------------------------------------------------------------------------------------------

def _topk_op(lib, x, rows, V, ldo, k):
    ids = torch.full((rows, k), -7, dtype=torch.long, device="cuda")
    lp = torch.full((rows, k), 7.0, dtype=torch.float32, device="cuda")
    native.check(lib.aigv_op_topk_logprob(x.data_ptr(), rows, V, ldo, k, ids.data_ptr(), lp.data_ptr(), native.stream_ptr()))
    return ids, lp


def _planted(V, k, R=64):
    """bf16 logits [R, V], randn * 3 with rows 0..4 overwritten: all-equal; a run of equal values across the k-th place; ties across the
    thread-chunk (4t+3 | 4t+4), slab (15 | 16) and stride (1023 | 1024) edges; the top value at V - 1; -inf everywhere but k - 1 columns."""
    g = torch.Generator().manual_seed(1000 * V + k)
    x = (torch.randn(R, V, generator=g) * 3).to(BF)
    x[0] = 1.5
    for i in range(max(k - 2, 0)):
        x[1, (5 + 3 * i) % V] = 40.0 + i
    run = sorted({V - 1, 2 % V, V // 2, 7 % V, 11 % V})
    x[1, run] = 30.0
    edges = [c for c in (3, 4, 15, 16, 1023, 1024, 4 * 97 + 3, 4 * 97 + 4) if c < V]
    x[2, edges] = 35.0
    x[3, V - 1] = 60.0
    x[3, 0] = 59.0
    x[4] = NEG
    if k > 1:
        x[4, V - k + 1:] = (torch.randn(k - 1, generator=g) * 3).to(BF)
    return x


@pytest.mark.parametrize("V", [16, 515, 2053, 92553])
def test_op_topk_logprob_is_the_stable_sort_and_the_candidate_kernels_bits(V):
    lib = native.load()
    R = 64
    forms = sorted({V, (V + 3) // 4 * 4, (V + 3) // 4 * 4 + 8})          # unaligned rows (scalar loads), aligned, padded
    for k in (1, 5, 16):
        x = _planted(V, k)
        want_ids = stable_topk(x, k)
        ref = torch.log_softmax(x.double(), -1).gather(-1, want_ids)
        assert want_ids[0].tolist() == list(range(k)) and int(want_ids[3, 0]) == V - 1 and int(want_ids[4, k - 1]) == 0
        first = None
        for ldo in forms:
            xp = torch.full((R, ldo), 100.0, dtype=BF)                    # padding columns must not count
            xp[:, :V] = x
            xd = xp.cuda()
            ids, lp = _topk_op(lib, xd, R, V, ldo, k)
            torch.cuda.synchronize()
            assert torch.equal(ids.cpu(), want_ids), (V, ldo, k)
            got = lp.cpu().double()
            fin = torch.isfinite(ref)
            err = (got - ref)[fin].abs().max().item() if bool(fin.any()) else 0.0
            print(f"V={V} ldo={ldo} k={k}: max |top lp - fp64| = {err:.3g}")
            assert err <= 1e-5
            assert not bool(torch.isfinite(got[~fin]).any())              # -inf logits: -inf (NaN in the row that holds nothing else)
            # column j = the candidate kernel fed this row's ids, and the label kernel fed column j, bit for bit
            for r in range(R):
                c = torch.empty((1, k), dtype=torch.float32, device="cuda")
                native.check(lib.aigv_op_cand_logprob(xd[r].data_ptr(), 1, V, ldo, ids[r].data_ptr(), k, c.data_ptr(), native.stream_ptr()))
                assert torch.equal(bits(c[0]), bits(lp[r])), (r, ldo, k)
            for j in range(k):
                one = torch.empty(R, dtype=torch.float32, device="cuda")
                lab = ids[:, j].contiguous()
                native.check(lib.aigv_op_label_logprob(xd.data_ptr(), R, V, ldo, lab.data_ptr(), one.data_ptr(), native.stream_ptr()))
                assert torch.equal(bits(one), bits(lp[:, j])), (j, ldo, k)
            # a row's results depend neither on the rows in the launch ...
            for r in (0, 1, 2, 3, 4, 63):
                i1, l1 = _topk_op(lib, xd[r], 1, V, ldo, k)
                assert torch.equal(i1, ids[r:r + 1]) and torch.equal(bits(l1), bits(lp[r:r + 1])), r
            i33, l33 = _topk_op(lib, xd, 33, V, ldo, k)
            assert torch.equal(i33, ids[:33]) and torch.equal(bits(l33), bits(lp[:33]))
            # ... nor on k: the first columns of k = 16 (where the vocabulary has 16) are this k's
            kk = min(16, V)
            ibig, lbig = _topk_op(lib, xd, R, V, ldo, kk)
            assert torch.equal(ibig[:, :k], ids) and torch.equal(bits(lbig[:, :k]), bits(lp))
            # ... nor on how the row is loaded (8-byte vector loads | scalar loads)
            if first is None:
                first = lp
            assert torch.equal(bits(lp), bits(first)), ldo
    # refused before anything runs
    xd = _planted(V, 1).cuda()
    ids = torch.zeros((R, 17), dtype=torch.long, device="cuda")
    lp = torch.zeros((R, 17), dtype=torch.float32, device="cuda")
    assert lib.aigv_op_topk_logprob(xd.data_ptr(), R, V, V, 17, ids.data_ptr(), lp.data_ptr(), native.stream_ptr()) == -1      # AIGV_ERR_ARG
    assert lib.aigv_op_topk_logprob(xd.data_ptr(), R, 3, V, 5, ids.data_ptr(), lp.data_ptr(), native.stream_ptr()) == -1       # k > vocab


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


def _argmax_cand_logprob(lib, h, W, V, cand_d):
    R, H = h.shape
    nbytes = lib.aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(R, V)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    idx = torch.full((R,), -7, dtype=torch.long, device="cuda")
    lp = torch.full((R,), float("nan"), device="cuda")
    clp = torch.full((R, cand_d.numel()), 7.0, device="cuda")
    native.check(lib.aigv_op_lm_head_argmax_cand_logprob(h.data_ptr(), R, H, W.data_ptr(), V, cand_d.data_ptr(), cand_d.numel(), scratch.data_ptr(), nbytes,
                                                         idx.data_ptr(), None, lp.data_ptr(), clp.data_ptr(), native.stream_ptr()))
    return idx, lp, clp


def _argmax_topk_logprob(lib, h, W, V, k, cand=None):
    R, H = h.shape
    nbytes = lib.aigv_op_lm_head_argmax_topk_logprob_scratch_bytes(R, V)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bits everywhere
    idx = torch.full((R,), -7, dtype=torch.long, device="cuda")
    val = torch.full((R,), float("nan"), device="cuda")
    lp = torch.full((R,), float("nan"), device="cuda")
    tid = torch.full((R, k), -7, dtype=torch.long, device="cuda")
    tlp = torch.full((R, k), 7.0, device="cuda")
    cd = None if cand is None else torch.tensor(cand, dtype=torch.long, device="cuda")
    clp = None if cand is None else torch.full((R, len(cand)), 7.0, device="cuda")
    native.check(lib.aigv_op_lm_head_argmax_topk_logprob(h.data_ptr(), R, H, W.data_ptr(), V, k, native.ptr(cd), 0 if cand is None else len(cand),
                                                         scratch.data_ptr(), nbytes, idx.data_ptr(), val.data_ptr(), lp.data_ptr(), tid.data_ptr(),
                                                         tlp.data_ptr(), native.ptr(clp), native.stream_ptr()))
    return idx, val, lp, tid, tlp, clp


def _store_logits(lib, h, W, V):
    """bf16 logits [R, V] from the skinny GEMM's store form (W padded to a multiple of 4 rows: every column is computed on its own)."""
    R, H = h.shape
    Np = (V + 3) // 4 * 4
    Wp = torch.zeros((Np, H), dtype=BF, device="cuda")
    Wp[:V] = W
    out = torch.full((R, Np), float("nan"), dtype=BF, device="cuda")
    native.check(lib.aigv_op_skinny_gemm(h.data_ptr(), H, R, Wp.data_ptr(), H, Np, H, None, None, 0, out.data_ptr(), Np, 0, native.stream_ptr()))
    return out[:, :V]


@pytest.mark.parametrize("V,H", [(17, 384), (2053, 640), (92553, 512)])
def test_op_lm_head_topk_holds_the_lm_heads_own_bits(V, H):
    lib = native.load()
    g = torch.Generator(device="cuda").manual_seed(V)
    h_all = torch.randn((33, H), generator=g, device="cuda").to(BF)
    W = (torch.randn((V, H), generator=g, device="cuda") * 0.05).to(BF)
    W[V // 2] = W[3]                                                   # two columns with the same logit in every row: ties by id
    W[V - 1] = W[3]
    cand = [0, V - 1, 5, V // 3]
    for R in (1, 5, 17, 33):                                           # one to three row tiles: both slab-per-workgroup forms
        h = h_all[:R].contiguous()
        idx0, val0, lp0 = _argmax_logprob(lib, h, W, V)
        logits = _store_logits(lib, h, W, V).cpu()
        for k in (1, 5, 16):
            idx, val, lp, tid, tlp, _ = _argmax_topk_logprob(lib, h, W, V, k)
            torch.cuda.synchronize()
            assert torch.equal(idx, idx0) and torch.equal(bits(val), bits(val0)) and torch.equal(bits(lp), bits(lp0)), (R, k)
            assert torch.equal(tid.cpu(), stable_topk(logits, k)), (R, k)
            assert torch.equal(tid[:, 0], idx) and torch.equal(bits(tlp[:, 0]), bits(lp)), (R, k)
            for r in range(R):                                         # every column: the candidate GEMV fed those ids
                _, l1, c1 = _argmax_cand_logprob(lib, h[r:r + 1].contiguous(), W, V, tid[r].contiguous())
                assert torch.equal(bits(c1[0]), bits(tlp[r])) and torch.equal(bits(l1), bits(lp[r:r + 1])), (R, k, r)
            err = (tlp.cpu().double() - torch.log_softmax(logits.double(), -1).gather(-1, tid.cpu())).abs().max().item()
            assert err <= 1e-5, err
            # candidates present or absent: nothing else moves, and they are the candidate op's bits
            i2, v2, l2, t2, tl2, c2 = _argmax_topk_logprob(lib, h, W, V, k, cand)
            _, _, cref = _argmax_cand_logprob(lib, h, W, V, torch.tensor(cand, device="cuda"))
            assert torch.equal(i2, idx) and torch.equal(bits(v2), bits(val)) and torch.equal(bits(l2), bits(lp))
            assert torch.equal(t2, tid) and torch.equal(bits(tl2), bits(tlp)) and torch.equal(bits(c2), bits(cref))
        # rows alone == rows in the batch: compared against the 33-row launch
        if R == 33:
            full = (tid, tlp)
        print(f"V={V} R={R}: max |top lp - fp64| = {err:.3g}")
    for R in (1, 5, 17):
        _, _, _, t, tl, _ = _argmax_topk_logprob(lib, h_all[:R].contiguous(), W, V, 16)
        assert torch.equal(t, full[0][:R]) and torch.equal(bits(tl), bits(full[1][:R])), R


def test_op_lm_head_topk_at_four_row_tiles():
    """R = 64: the four-row-tile form of the storing lm-head (the test above stops at three) - the stored logits' top-k in the key's order, and
    the argmax / log-prob bits of the form that stores nothing."""
    lib = native.load()
    V, H, R, k = 2053, 128, 64, 5
    g = torch.Generator(device="cuda").manual_seed(V + R)
    h = torch.randn((R, H), generator=g, device="cuda").to(BF)
    W = (torch.randn((V, H), generator=g, device="cuda") * 0.05).to(BF)
    W[V - 1] = W[3]
    idx0, val0, lp0 = _argmax_logprob(lib, h, W, V)
    logits = _store_logits(lib, h, W, V).cpu()
    idx, val, lp, tid, tlp, _ = _argmax_topk_logprob(lib, h, W, V, k)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx0) and torch.equal(bits(val), bits(val0)) and torch.equal(bits(lp), bits(lp0))
    assert torch.equal(tid.cpu(), stable_topk(logits, k))
    assert torch.equal(tid[:, 0], idx) and torch.equal(bits(tlp[:, 0]), bits(lp))
    err = (tlp.cpu().double() - torch.log_softmax(logits.double(), -1).gather(-1, tid.cpu())).abs().max().item()
    assert err <= 1e-5, err


# ---- 3. the scoring pass -------------------------------------------------------------------------------------------------------------

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
def test_forward_top_logprobs_are_the_sorted_logits_and_the_candidate_bits(stage):
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    seed = 117 + stage
    model = make_model(cfg, synth.make_state_dict(cfg, seed=seed, rich=True), stage=stage)
    T, K = 2, 5
    clips, ids, am, labels, pv, motion = _ragged_batch(cfg, seed, T)
    model.img_context_token_id = clips[0]["img_context_token_id"]
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=torch.ones(2 * T, 1, dtype=torch.long), labels=labels, motion_feature=motion)
    off = model(**kw)
    lp_only = model(**kw, return_logprobs=True)
    on = model(**kw, top_logprobs=K)
    allthree = model(**kw, top_logprobs=K, return_logprobs=True, candidate_ids=[11, 5, 400])
    cand_only = model(**kw, candidate_ids=[11, 5, 400])
    torch.cuda.synchronize()
    assert set(on) == set(off) | {"top_ids", "top_logprob"}
    for k_ in ("logit", "label") + (("score1",) if stage == 2 else ()):
        assert torch.equal(on[k_], off[k_]) and torch.equal(allthree[k_], off[k_]), k_
    assert torch.equal(bits(allthree["logprob"]), bits(lp_only["logprob"])) and torch.equal(bits(allthree["cand_logprob"]), bits(cand_only["cand_logprob"]))
    assert torch.equal(allthree["top_ids"], on["top_ids"]) and torch.equal(bits(allthree["top_logprob"]), bits(on["top_logprob"]))
    n = ids.shape[1]
    tid, tlp = on["top_ids"], on["top_logprob"]
    assert tid.dtype == torch.long and tlp.dtype == torch.float32 and tid.shape == tlp.shape == (2 * (n - 1), K)
    lab = on["label"].cpu()
    scored = lab != -100
    assert torch.equal(tid.cpu() == -1, (~scored).view(-1, 1).expand(-1, K)) and torch.equal(torch.isnan(tlp.cpu()), (~scored).view(-1, 1).expand(-1, K))
    assert torch.equal(tid[:, 0], on["logit"])                         # entry 0: the argmax token
    # the same pass's logits at the answer rows (consumed rows: [score rows | answer rows]), sorted
    R = int(scored.sum())
    nS = 2 if stage == 2 else 0
    rows = model._row_logits(nS + R)[nS:].cpu()
    assert torch.equal(tid.cpu()[scored], stable_topk(rows, K))
    # full_logits (an argmax at every row): `logit` as without, the top-k still only where a label is
    full = model(**kw, full_logits=True, top_logprobs=K)
    assert torch.equal(full["logit"], model(**kw, full_logits=True)["logit"])
    # (that pass keeps the clips' dead tails, so its GEMMs see other row counts: its logits are its own, not compared bit for bit)
    assert torch.equal(full["top_ids"].cpu() == -1, (~scored).view(-1, 1).expand(-1, K)) and torch.equal(torch.isnan(full["top_logprob"].cpu()), full["top_ids"].cpu() == -1)
    assert torch.equal(full["top_ids"][:, 0].cpu()[scored], full["logit"].cpu()[scored])
    # candidate_ids = a row's ids: its log-probabilities, bit for bit; the label among them carries logprob
    lp_lab = lp_only["logprob"]
    hit = 0
    for r in scored.nonzero().flatten().tolist()[::3]:
        c = model(**kw, candidate_ids=tid[r])["cand_logprob"]
        assert torch.equal(bits(c[r]), bits(tlp[r])), r
    for r in scored.nonzero().flatten().tolist():
        for j in range(K):
            if int(tid[r, j]) == int(lab[r]):
                assert torch.equal(bits(tlp[r, j:j + 1]), bits(lp_lab[r:r + 1])), (r, j)
                hit += 1
    swapped = torch.where(labels != -100, torch.cat([labels[:, :1], tid[:, 0].cpu().view(2, n - 1)], 1), labels)   # every label = the row's argmax
    assert torch.equal(bits(model(**dict(kw, labels=swapped), return_logprobs=True)["logprob"]), bits(tlp[:, 0]))
    with pytest.raises(ValueError, match="needs labels"):
        model(**dict(kw, labels=None), top_logprobs=K)
    with pytest.raises(ValueError, match="expected an int in 1..16"):
        model(**kw, top_logprobs=17)


def test_top_logprobs_are_batch_graph_prefix_and_loop_invariant():
    cfg = pkg.tiny(image_size=224, vit_layers=1)
    model = make_model(cfg, synth.make_state_dict(cfg, seed=123, rich=True))
    T = 2
    toks = synth.canonical_tokens(cfg, 3, T, seed=123)
    model.img_context_token_id = toks["img_context_token_id"]
    pv = synth.synthetic_frames(3 * T, 224, seed=123).cuda()
    motion = synth.synthetic_motion(3, cfg.motion_dim, seed=123).cuda()
    flags = torch.ones(3 * T, 1, dtype=torch.long)

    def run(b0, b1, frames=pv, k=5, **kw):
        o = model(pixel_values=frames[T * b0:T * b1], input_ids=toks["input_ids"][b0:b1], attention_mask=toks["attention_mask"][b0:b1],
                  image_flags=flags[T * b0:T * b1], labels=toks["labels"][b0:b1], motion_feature=motion[b0:b1], top_logprobs=k, **kw)
        torch.cuda.synchronize()
        return {k_: v.clone() for k_, v in o.items() if torch.is_tensor(v)}

    n = toks["input_ids"].shape[1]
    alone, batch = run(0, 1), run(0, 3)
    assert torch.equal(alone["top_ids"], batch["top_ids"][: n - 1]) and torch.equal(bits(alone["top_logprob"]), bits(batch["top_logprob"][: n - 1]))
    big = run(0, 3, k=16)
    assert torch.equal(big["top_ids"][:, :5], batch["top_ids"]) and torch.equal(bits(big["top_logprob"][:, :5]), bits(batch["top_logprob"]))
    # graph replay: call 1 eager, call 2 captures, calls 3.. replay; another k is another graph, and replaying the first afterwards still holds
    frames = [synth.synthetic_frames(3 * T, 224, seed=140 + i).cuda() for i in range(4)]
    eager = [run(0, 3, f) for f in frames]
    eager16 = run(0, 3, frames[0], k=16)
    model.enable_graph_replay(True)
    try:
        got = [run(0, 3, f) for f in frames]
        held = [k_ for k_, v in model._graphs.items() if isinstance(v, tuple)]
        assert len(held) == 1 and held[0][0][-1] == ("top_logprobs", 5)
        got16 = [run(0, 3, frames[0], k=16) for _ in range(3)]
        assert len(model._graphs) == 2
        again = run(0, 3, frames[1])                                  # a replay after a call with another k
    finally:
        model.enable_graph_replay(False)
    for g_, e in zip(got + [again], eager + [eager[1]]):
        for k_ in ("top_ids", "top_logprob", "logit", "score1"):
            assert torch.equal(bits(g_[k_]) if g_[k_].is_floating_point() else g_[k_], bits(e[k_]) if e[k_].is_floating_point() else e[k_]), k_
    for g_ in got16:
        assert torch.equal(g_["top_ids"], eager16["top_ids"]) and torch.equal(bits(g_["top_logprob"]), bits(eager16["top_logprob"]))
    # the batched loop (k = 3, ragged prompts) against the plain loop
    items = []
    for i, alen in enumerate((9, 4, 12, 6)):
        t = synth.canonical_tokens(cfg, 1, T, seed=150 + i, answer_len=alen)
        items.append({"input_ids": t["input_ids"], "attention_mask": t["attention_mask"], "labels": t["labels"],
                      "image_flags": torch.ones(1, T, 1, dtype=torch.long), "pixel_values": synth.synthetic_frames(T, 224, seed=150 + i).unsqueeze(0),
                      "motion_feature": synth.synthetic_motion(1, cfg.motion_dim, seed=150 + i)})
    looped = list(eval_utils.batched(items, model, k=3, top_logprobs=5))
    assert len(looped) == len(items)
    for it, o in looped:
        ref = model(pixel_values=it["pixel_values"][0].cuda(), input_ids=it["input_ids"], attention_mask=it["attention_mask"],
                    image_flags=it["image_flags"][0], labels=it["labels"], motion_feature=it["motion_feature"].cuda(), top_logprobs=5)
        assert torch.equal(o["top_ids"], ref["top_ids"].cpu()) and torch.equal(bits(o["top_logprob"]), bits(ref["top_logprob"]))
    # the shared-prefix pass: its own candidate bits, its own sorted logits
    B = 2
    base = synth.canonical_tokens(cfg, B, T, seed=129, answer_len=1)
    model.img_context_token_id = base["img_context_token_id"]
    n_prompt = int((base["labels"][0] == -100).sum())
    prompts = []
    for w in (11, 40, 77):
        ans = [w, int(base["im_end_id"])]
        pid = torch.cat([base["input_ids"][:, :n_prompt], torch.tensor([ans] * B)], 1)
        plab = torch.cat([torch.full((B, n_prompt), -100), torch.tensor([ans] * B)], 1)
        prompts.append((pid, torch.ones_like(pid, dtype=torch.bool), plab))
    kw = dict(pixel_values=synth.synthetic_frames(B * T, 224, seed=129), image_flags=torch.ones(B * T, 1, dtype=torch.long),
              motion_feature=synth.synthetic_motion(B, cfg.motion_dim, seed=129))
    outs = model.forward_shared_prefix(prompts, **kw, top_logprobs=5, return_logprobs=True)
    plain = model.forward_shared_prefix(prompts, **kw, return_logprobs=True)
    P_ = len(prompts)
    l_shared = model._row_logits(B * P_ + 2 * B * P_)[B * P_:].cpu()   # rows: prompt 0 (clip 0: word, end; clip 1: ...), prompt 1, ...
    r0 = 0
    for o, p in zip(outs, plain):
        assert set(o) == set(p) | {"top_ids", "top_logprob"}
        for k_ in ("logit", "score1"):
            assert torch.equal(o[k_], p[k_]), k_
        assert torch.equal(bits(o["logprob"]), bits(p["logprob"]))
        scored = (o["label"] != -100).cpu()
        assert torch.equal(o["top_ids"].cpu()[scored], stable_topk(l_shared[r0:r0 + 2 * B], 5))
        assert torch.equal(o["top_ids"][:, 0], o["logit"])
        r0 += 2 * B
    row = scored.nonzero().flatten()[0].item()
    c = model.forward_shared_prefix(prompts, **kw, candidate_ids=outs[0]["top_ids"][row])
    assert torch.equal(bits(c[0]["cand_logprob"][row]), bits(outs[0]["top_logprob"][row]))


def test_score_clips_dp_top_logprobs_over_rccl_single_rank():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "topk_rccl_single_rank_child.py")], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "TOPK_DP_OK" in r.stdout


# ---- 4. generate ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    return make_model(cfg, synth.make_state_dict(cfg, seed=171, rich=True)), cfg


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


def _check_greedy(model, pv, ids, am, n_new, K, eos=None):
    """Greedy generate with top_logprobs: sequences / logprobs as without (bit for bit); entry 0 is the emitted token and its logprob; the
    first token (prompt-pass rows) and the later ones (fused decode step) against generation.top_logprobs of the step's raw logits - ids
    exactly, log-probabilities within 1e-5 (other reduction trees); the materialised path equal to it."""
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=n_new, do_sample=False)
    if eos is not None:
        kw.update(eos_token_id=eos, pad_token_id=2)
    base = model.generate(**kw, return_logprobs=True)
    fused = model.generate(**kw, return_logprobs=True, top_logprobs=K)
    alone = model.generate(**kw, top_logprobs=K)
    mat = model.generate(**kw, return_dict_in_generate=True, output_logits=True, return_logprobs=True, top_logprobs=K)
    for o in (fused, alone, mat):
        assert isinstance(o, generation.GenerateOutput) and torch.equal(o.sequences, base.sequences)
        assert o.top_ids.shape == o.top_logprobs.shape == base.sequences.shape + (K,)
        assert o.top_ids.dtype == torch.long and o.top_logprobs.dtype == torch.float32
    assert torch.equal(bits(fused.logprobs), bits(base.logprobs)) and alone.logprobs is None and base.top_ids is None
    assert torch.equal(alone.top_ids, fused.top_ids) and torch.equal(bits(alone.top_logprobs), bits(fused.top_logprobs))
    ended = _ended_mask(base.sequences.cpu(), [eos] if isinstance(eos, int) else (eos or []))
    live = ~ended
    for o in (fused, mat):
        assert torch.equal(o.top_ids.cpu() == -1, ended.unsqueeze(-1).expand(-1, -1, K))
        assert torch.equal(torch.isnan(o.top_logprobs.cpu()), ended.unsqueeze(-1).expand(-1, -1, K))
    assert torch.equal(fused.top_ids[:, :, 0].cpu()[live], base.sequences.cpu()[live])
    assert torch.equal(bits(fused.top_logprobs[:, :, 0])[live], bits(fused.logprobs)[live])
    for t, raw in enumerate(mat.logits):
        want_ids, want_lp = generation.top_logprobs(raw, K)
        lv = live[:, t]
        assert torch.equal(mat.top_ids[:, t].cpu()[lv], want_ids.cpu()[lv]) and torch.equal(bits(mat.top_logprobs[:, t])[lv], bits(want_lp)[lv]), t
        assert torch.equal(fused.top_ids[:, t].cpu()[lv], want_ids.cpu()[lv]), t
        ref = torch.log_softmax(raw.double(), -1).gather(-1, want_ids).cpu()
        assert (fused.top_logprobs[:, t].cpu().double() - ref)[lv].abs().max().item() <= 1e-5, t
    return base, fused


def test_generate_top_logprobs_fused_ragged_eos_and_batch_invariant(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 3, seed=172, ragged=True)
    plain = model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=9, do_sample=False)
    base, fused = _check_greedy(model, pv, ids, am, 9, 5)
    assert torch.equal(base.sequences, plain)
    eos = int(plain[0, 3])                                              # the first sequence ends mid-run
    stop = [t for t in range(9) if int(plain[0, t]) == eos][0]
    _, ragged = _check_greedy(model, pv, ids, am, 9, 5, eos=eos)
    assert bool((ragged.top_ids[0, stop + 1:] == -1).all()) and bool(torch.isnan(ragged.top_logprobs[0, stop + 1:]).all())
    assert not bool(torch.isnan(ragged.top_logprobs[0, : stop + 1]).any())
    # with candidates in the same fused step: neither moves the other
    both = model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=9, do_sample=False, top_logprobs=5, candidate_ids=[11, 5, 400])
    cand = model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=9, do_sample=False, candidate_ids=[11, 5, 400])
    assert torch.equal(both.top_ids, fused.top_ids) and torch.equal(bits(both.top_logprobs), bits(fused.top_logprobs))
    assert torch.equal(bits(both.cand_logprobs), bits(cand.cand_logprobs))
    big = model.generate(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=9, do_sample=False, top_logprobs=16)
    assert torch.equal(big.top_ids[:, :, :5], fused.top_ids) and torch.equal(bits(big.top_logprobs[:, :, :5]), bits(fused.top_logprobs))
    for b in (0, 2):                                                    # a sequence's bits do not depend on its batch mates
        keep = am[b].bool()
        one = model.generate(pixel_values=pv[2 * b:2 * b + 2], input_ids=ids[b:b + 1, keep], attention_mask=am[b:b + 1, keep], max_new_tokens=9,
                             do_sample=False, top_logprobs=5)
        assert torch.equal(one.sequences[0], plain[b])
        assert torch.equal(one.top_ids[0], fused.top_ids[b]) and torch.equal(bits(one.top_logprobs[0]), bits(fused.top_logprobs[b]))


def test_generate_top_logprobs_in_fp8_mode(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=173)
    model.set_precision("fp8")
    try:
        _check_greedy(model, pv, ids, am, 6, 5)
    finally:
        model.set_precision("bf16")


def test_generate_top_logprobs_with_processors_sampling_and_beams(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=174)
    kw = dict(pixel_values=pv, input_ids=ids, attention_mask=am, max_new_tokens=7)
    flags = dict(return_dict_in_generate=True, output_logits=True)
    base = model.generate(**kw, do_sample=False, repetition_penalty=1.3)
    o = model.generate(**kw, do_sample=False, repetition_penalty=1.3, **flags, top_logprobs=5)
    assert torch.equal(o.sequences, base)
    for t in range(base.shape[1]):
        wi, wl = generation.top_logprobs(o.logits[t], 5)
        assert torch.equal(o.top_ids[:, t], wi) and torch.equal(bits(o.top_logprobs[:, t]), bits(wl))
    samp = dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.8)
    base = model.generate(**kw, **samp, generator=torch.Generator(device=model.device).manual_seed(11))
    o = model.generate(**kw, **samp, generator=torch.Generator(device=model.device).manual_seed(11), **flags, top_logprobs=5)
    assert torch.equal(o.sequences, base)
    for t in range(base.shape[1]):
        wi, wl = generation.top_logprobs(o.logits[t], 5)
        assert torch.equal(o.top_ids[:, t], wi) and torch.equal(bits(o.top_logprobs[:, t]), bits(wl))
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        model.generate(**kw, do_sample=False, num_beams=3, top_logprobs=5)


def test_generate2_and_generate_stage2_carry_the_top_logprobs(rig):
    model, cfg = rig
    pv, ids, am = _prompts(model, cfg, 2, seed=176)
    emb = model.language_model.get_input_embeddings().weight[ids.cuda()]
    base = model.generate2(emb, max_new_tokens=5, do_sample=False)
    o = model.generate2(emb, max_new_tokens=5, do_sample=False, return_dict_in_generate=True, output_logits=True, top_logprobs=5)
    f = model.generate2(emb, max_new_tokens=5, do_sample=False, top_logprobs=5)
    assert torch.equal(o.sequences, base) and torch.equal(f.sequences, base) and torch.equal(f.top_ids, o.top_ids)
    assert (f.top_logprobs.double() - o.top_logprobs.double()).abs().max().item() <= 1e-5
    toks = synth.canonical_tokens(cfg, 2, 2, seed=177)
    n_prompt = int((toks["labels"][0] == -100).sum())
    sids, sam = toks["input_ids"][:, :n_prompt], toks["attention_mask"][:, :n_prompt]
    spv = synth.synthetic_frames(4, 224, seed=177)
    motion = synth.synthetic_motion(2, cfg.motion_dim, seed=177)
    model.img_context_token_id = toks["img_context_token_id"]
    flags_ = torch.ones(4, 1, dtype=torch.long)
    base = model.generate_stage2(spv, sids, sam, flags_, motion, max_new_tokens=5, do_sample=False)
    f = model.generate_stage2(spv, sids, sam, flags_, motion, max_new_tokens=5, do_sample=False, top_logprobs=5)
    assert torch.equal(f.sequences, base) and torch.equal(f.top_ids[:, :, 0], base)
