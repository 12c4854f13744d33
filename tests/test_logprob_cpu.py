"""The label log-probability feature without a GPU: the C ABI it adds (header, library exports, ctypes prototypes; ABI version 2, now 3),
the clear error a stale library gives, the host-side label checks of ``return_logprobs`` and the per-item results of
``eval_utils.batched``."""
import ctypes
import os
import re

import pytest
import torch

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aigv_out_row_logprob", "aigv_op_label_logprob")


def test_abi_3_declares_and_exports_the_logprob_entry_points():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header)
    assert native.ABI_VERSION == 3
    lib = ctypes.CDLL(native.LIB_PATH)
    assert lib.aigv_abi_version() == 3
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in native.PROTOTYPES
        getattr(lib, name)
    assert native.PROTOTYPES["aigv_out_row_logprob"][1] == [native._P, native._I, native._I, native._P, native._P, native._P]
    assert native.PROTOTYPES["aigv_op_label_logprob"][1] == [native._P, native._I, native._I, native._I, native._P, native._P, native._P]


def test_a_missing_symbol_is_reported_as_an_abi_mismatch(monkeypatch):
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setitem(native.PROTOTYPES, "aigv_not_exported_anywhere", (native._I, []))
    with pytest.raises(native.NativeError, match=r"ABI mismatch.*missing aigv_not_exported_anywhere"):
        native.load()


def _model_and_tokens(B=2):
    from aigv_assessor_amd.modeling import InternVLChatModel
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=1)
    model = InternVLChatModel(cfg)
    toks = synth.canonical_tokens(cfg, B, 1, seed=3)
    model.img_context_token_id = toks["img_context_token_id"]
    return model, cfg, toks


def test_logprob_labels_are_checked_on_the_host():
    model, cfg, toks = _model_and_tokens()
    V = cfg.llm_config.vocab_size
    plan = model._plan(toks["input_ids"], toks["attention_mask"], toks["labels"], None, 2)
    lab = model._logprob_labels(plan)
    assert torch.equal(lab, toks["labels"][:, 1:][toks["labels"][:, 1:] != -100])
    for bad_value in (V, -1, -101):
        bad = toks["labels"].clone()
        bad[1, -1] = bad_value
        plan = model._plan(toks["input_ids"], toks["attention_mask"], bad, None, 2)
        with pytest.raises(ValueError, match="outside"):
            model._logprob_labels(plan)
    # a scored label behind a padded position: the reference would score the padded row - refused
    am = toks["attention_mask"].clone()
    am[1, -2] = False
    plan = model._plan(toks["input_ids"], am, toks["labels"], None, 2)
    with pytest.raises(ValueError, match="padded"):
        model._logprob_labels(plan)
    # full_logits keeps every row: rows with label -100 are passed on as -100 (NaN from the kernel)
    plan = model._plan(toks["input_ids"], toks["attention_mask"], toks["labels"], None, 2, full_logits=True)
    assert int((model._logprob_labels(plan) == -100).sum()) == int((toks["labels"][:, 1:] == -100).sum())


class _FakeModel:
    """Stands in for the GPU model: logprob[b, p] = -(b + 1) * (p + 1) / 100 at the answer rows, NaN elsewhere; records its kwargs."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def prefetch(self, pixel_values=None, frames_u8=None, n_clips=1):
        return pixel_values

    def __call__(self, **kw):
        self.calls.append(sorted(kw))
        lab = kw["labels"][:, 1:]
        B, n = lab.shape
        lp = -(torch.arange(1, B + 1).view(-1, 1) * torch.arange(1, n + 1).view(1, -1)).float() / 100
        lp = torch.where(lab != -100, lp, torch.full_like(lp, float("nan")))
        out = {"logit": torch.zeros(B * n, dtype=torch.long), "label": lab.reshape(-1), "score1": torch.zeros(B, dtype=torch.bfloat16)}
        if kw.get("return_logprobs"):
            out["logprob"] = lp.reshape(-1)
            out["ce_loss"] = (-lp[lab != -100]).double().mean().float()
        return out


def test_batched_passes_the_flag_and_splits_logprob_per_item():
    items = []
    for i, (n, n_ans) in enumerate(((12, 3), (9, 4), (15, 0))):
        ids = torch.arange(3, 3 + n).view(1, -1)
        lab = torch.full((1, n), -100)
        if n_ans:
            lab[0, -n_ans:] = ids[0, -n_ans:]
        items.append({"input_ids": ids, "attention_mask": torch.ones(1, n, dtype=torch.bool), "labels": lab,
                      "pixel_values": torch.zeros(1, 1, 3, 4, 4)})
    fake = _FakeModel()
    plain = list(eval_utils.batched(items, fake, k=3))
    assert "return_logprobs" not in fake.calls[0] and "logprob" not in plain[0][1]
    fake = _FakeModel()
    got = list(eval_utils.batched(items, fake, k=3, return_logprobs=True))
    assert "return_logprobs" in fake.calls[0]
    for b, ((it, o), (n, n_ans)) in enumerate(zip(got, ((12, 3), (9, 4), (15, 0)))):
        assert o["logprob"].shape == (n - 1,)
        want = torch.full((n - 1,), float("nan"))
        if n_ans:
            p = torch.arange(n - 1 - n_ans, n - 1)
            want[p] = -(b + 1) * (p + 1).float() / 100
        assert torch.equal(torch.isnan(o["logprob"]), torch.isnan(want))
        assert torch.equal(o["logprob"][~torch.isnan(want)], want[~torch.isnan(want)])
        if n_ans:
            assert o["ce_loss"].item() == pytest.approx(-want[~torch.isnan(want)].double().mean().item(), rel=1e-6)
        else:
            assert torch.isnan(o["ce_loss"])


def test_graph_key_tails_of_the_readouts_record():
    """What each read-out appends to a graph's host key, written out: nothing for an option that is off, then - in this order - "logprobs",
    "candidates", ("top_logprobs", k), ("score_attention", S) with S = 0 for the default table and the largest id + 1 for a user table, and
    ("score_attention_tokens", N).  A record with every option off passes no keyword on."""
    from aigv_assessor_amd import readouts
    model, cfg, toks = _model_and_tokens()
    V = cfg.llm_config.vocab_size
    input_ids = torch.zeros(2, 24, dtype=torch.long)
    table = (torch.arange(48) % 5).view(2, 24)
    assert int(table.max()) == 4
    tail = lambda **kw: readouts.ReadOuts.parse(V, toks["labels"], **kw).key_tail(input_ids.shape)
    assert tail() == ()
    assert tail(return_logprobs=True) == ("logprobs",)
    assert tail(candidate_ids=[3, 5]) == ("candidates",)
    assert tail(top_logprobs=3) == (("top_logprobs", 3),)
    assert tail(return_score_attention=True) == (("score_attention", 0),)
    assert tail(return_score_attention=True, attention_segments=table) == (("score_attention", 5),)
    assert tail(return_token_attention=True) == (("score_attention", 0), ("score_attention_tokens", 24))
    assert tail(return_logprobs=True, candidate_ids=[3, 5], top_logprobs=3, return_score_attention=True, attention_segments=table,
                return_token_attention=True) == ("logprobs", "candidates", ("top_logprobs", 3), ("score_attention", 5), ("score_attention_tokens", 24))
    assert readouts.forward_kwargs(readouts.ReadOuts.parse(V, toks["labels"])) == {}
    assert readouts.forward_kwargs(readouts.ReadOuts()) == {}
