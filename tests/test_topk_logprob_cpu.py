"""Top-k log-probabilities without a GPU: the C ABI the feature adds (header, kernels.h, ctypes prototypes, exports; AIGV_MAX_TOPK; the
ABI version stays 3), the host-side argument checks of the new entry points - a refused call returns AIGV_ERR_ARG naming the op before
anything reaches the device -, ``generation.top_logprobs`` against the stable-sort statement of the selection rule on planted ties, the
``top_logprobs`` validation helper, and the plumbing through ``generation.build`` / ``eval_utils.batched`` / beam search."""
import ctypes
import os
import re

import pytest
import torch

from aigv_assessor_amd import eval_utils, generation, native
from aigv_assessor_amd.modeling import InternVLChatModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = native._P, native._I
NEW = {
    "aigv_op_topk_logprob": [P, I, I, I, I, P, P, P],
    "aigv_out_row_topk_logprob": [P, I, I, I, P, P, P],
    "aigv_decode_step_topk_logprob": [P, P, P, P, I, P, P, P, I, P, P],
    "aigv_op_lm_head_argmax_topk_logprob": [P, I, I, P, I, I, P, I, P, ctypes.c_int64, P, P, P, P, P, P, P],
    "aigv_op_lm_head_argmax_topk_logprob_scratch_bytes": [I, I],
}
FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it: a call that reached the device would fault or fail with a HIP error


def test_abi_declares_and_exports_the_topk_entry_points():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    kernels = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"#define AIGV_ABI_VERSION (\d+)\b", header).group(1)) == native.ABI_VERSION == 3
    assert re.search(r"#define AIGV_MAX_TOPK 16\b", header) and re.search(r"#define AIGV_MAX_TOPK 16\b", kernels)
    assert InternVLChatModel.MAX_TOPK == 16
    lib = ctypes.CDLL(native.LIB_PATH)
    assert lib.aigv_abi_version() == 3
    for name, args in NEW.items():
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
        assert native.PROTOTYPES[name][1] == args, name
        getattr(lib, name)
    assert native.PROTOTYPES["aigv_op_lm_head_argmax_topk_logprob_scratch_bytes"][0] is ctypes.c_int64
    assert re.search(r"aigv_launch_topk_logprob\(", kernels)
    for name in NEW:                                                  # the version comment names what joined version 3
        if not name.endswith("_scratch_bytes"):
            assert name in header.split("#define AIGV_ABI_VERSION")[1].split("*/")[0], name


def _refused(lib, rc, op, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG, not AIGV_ERR_HIP
    assert msg.startswith(op + ":") and re.search(what, msg), msg


def test_topk_entry_points_refuse_bad_arguments_on_the_host():
    lib = native.load()
    op = "aigv_op_topk_logprob"
    call = lambda logits=FAKE, rows=2, V=100, ldo=100, k=5, ids=FAKE, out=FAKE: lib.aigv_op_topk_logprob(logits, rows, V, ldo, k, ids, out, None)
    _refused(lib, call(k=0), op, r"k = 0 outside")
    _refused(lib, call(k=17), op, r"k = 17 outside")
    _refused(lib, call(V=3, ldo=4, k=5), op, r"k = 5 outside")
    _refused(lib, call(ldo=99), op, r"bad argument")
    _refused(lib, call(ids=None), op, r"null operand")
    _refused(lib, call(out=None), op, r"null operand")
    assert call(rows=0, logits=None, ids=None, out=None) == 0         # no rows: nothing to do
    op = "aigv_op_lm_head_argmax_topk_logprob"
    sb = lib.aigv_op_lm_head_argmax_topk_logprob_scratch_bytes
    assert sb(0, 100) == -1 and sb(65, 100) == -1 and sb(4, 0) == -1
    assert sb(4, 100) >= lib.aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(4, 100) + 4 * 100 * 2

    def head(k=5, cand=None, C=0, rows=4, V=100, nbytes=None, top_ids=FAKE, top_lp=FAKE, clp=None):
        nbytes = sb(rows, V) if nbytes is None else nbytes
        return lib.aigv_op_lm_head_argmax_topk_logprob(FAKE, rows, 128, FAKE, V, k, cand, C, FAKE, nbytes, FAKE, None, FAKE, top_ids, top_lp, clp, None)
    _refused(lib, head(k=0), op, r"k = 0 outside")
    _refused(lib, head(k=17), op, r"k = 17 outside")
    _refused(lib, head(k=5, V=4), op, r"k = 5 outside")
    _refused(lib, head(C=3), op, r"C = 3 candidates")
    _refused(lib, head(cand=FAKE, C=65, clp=FAKE), op, r"C = 65 candidates")
    _refused(lib, head(cand=FAKE, C=5), op, r"null operand")
    _refused(lib, head(top_ids=None), op, r"null operand")
    _refused(lib, head(nbytes=sb(4, 100) - 1), op, r"scratch of")
    _refused(lib, lib.aigv_out_row_topk_logprob(None, 0, 1, 0, FAKE, FAKE, None), "aigv_out_row_topk_logprob", r"k = 0 outside")
    _refused(lib, lib.aigv_out_row_topk_logprob(None, 0, 1, 17, FAKE, FAKE, None), "aigv_out_row_topk_logprob", r"k = 17 outside")
    _refused(lib, lib.aigv_out_row_topk_logprob(None, 0, 1, 5, FAKE, FAKE, None), "aigv_out_row_topk_logprob", r"null argument")
    step = lambda k=5, cand=None, C=0, clp=None, lp=FAKE: lib.aigv_decode_step_topk_logprob(None, FAKE, FAKE, lp, k, FAKE, FAKE, cand, C, clp, None)
    _refused(lib, step(k=17), "aigv_decode_step_topk_logprob", r"k = 17 outside")
    _refused(lib, step(C=2), "aigv_decode_step_topk_logprob", r"C = 2 candidates")
    _refused(lib, step(cand=FAKE, C=5), "aigv_decode_step_topk_logprob", r"null argument")
    _refused(lib, step(lp=None), "aigv_decode_step_topk_logprob", r"null argument")
    _refused(lib, step(), "aigv_decode_step_topk_logprob", r"null argument")       # (no context)


def _stable(x, k):
    return torch.sort(x.float(), dim=-1, descending=True, stable=True).indices[..., :k]


@pytest.mark.parametrize("k", [1, 5, 16])
def test_generation_top_logprobs_is_the_stable_sort_rule_on_planted_ties(k):
    V = 515
    g = torch.Generator().manual_seed(k)
    x = (torch.randn(6, V, generator=g) * 3).to(torch.bfloat16)
    x[0] = 1.5                                                        # an all-equal row: ids 0 .. k - 1
    run = [V - 1, 2, V // 2, 7, 300]                                  # a run of equal values straddling position k
    for i in range(max(k - 2, 0)):
        x[1, 20 + 3 * i] = 40.0 + i
    x[1, run] = 30.0
    x[2, V - 1] = 60.0                                                # the maximum at the last column
    x[3, [3, 4, 15, 16]] = 35.0
    ids, lp = generation.top_logprobs(x, k)
    assert ids.dtype == torch.long and lp.dtype == torch.float32 and ids.shape == lp.shape == (6, k)
    assert torch.equal(ids, _stable(x, k))
    assert ids[0].tolist() == list(range(k)) and int(ids[2, 0]) == V - 1
    tail = sorted(run)
    n_before = max(k - 2, 0)
    assert ids[1, n_before:].tolist() == tail[: k - n_before]
    assert ids[3, : min(k, 4)].tolist() == [3, 4, 15, 16][: min(k, 4)]
    want = torch.log_softmax(x.double(), -1).gather(-1, ids)
    assert (lp.double() - want).abs().max().item() <= 1e-5
    assert torch.equal(lp, torch.log_softmax(x.float(), -1).gather(-1, ids))
    # the first columns of a larger k are the smaller k's
    if k > 1:
        i1, l1 = generation.top_logprobs(x, 1)
        assert torch.equal(i1, ids[:, :1]) and torch.equal(l1, lp[:, :1])
    with pytest.raises(ValueError, match="outside"):
        generation.top_logprobs(x[:, :3], 4)


def test_top_logprobs_validation_helper():
    chk = InternVLChatModel._top_logprobs_k
    assert chk(None, 100) == 0 and chk(None, 100, None) == 0
    assert chk(1, 100) == 1 and chk(16, 100) == 16 and chk(3, 3) == 3
    for bad in (0, 17, -1, True, False, 5.0, "5", torch.tensor(5)):
        with pytest.raises(ValueError, match="top_logprobs: expected an int in 1..16"):
            chk(bad, 100)
    with pytest.raises(ValueError, match="exceeds the vocabulary"):
        chk(5, 4)
    with pytest.raises(ValueError, match="needs labels"):
        chk(5, 100, None)


def test_generate_output_carries_the_two_fields():
    assert "top_ids" in generation.FIELDS and "top_logprobs" in generation.FIELDS
    flags = {k: False for k in generation.FLAGS}
    seq = torch.tensor([[5, 6], [7, 2]])
    ids = [torch.tensor([[5, 1, 0], [7, 3, 2]]), torch.tensor([[6, 5, 4], [2, 9, 8]]), torch.tensor([[0, 0, 0], [0, 0, 0]])]
    lps = [torch.full((2, 3), -1.0), torch.full((2, 3), -2.0), torch.full((2, 3), -3.0)]
    live = torch.tensor([True, False])
    ids[1] = generation.mask_ids_after_end(ids[1], live)
    lps[1] = generation.mask_after_end(lps[1], live)
    out = generation.build(seq, flags, top_ids=ids, top_logprobs=lps)
    assert out.top_ids.shape == out.top_logprobs.shape == (2, 2, 3) and out.top_ids.dtype == torch.long
    assert out.top_ids[1, 1].tolist() == [-1, -1, -1] and bool(torch.isnan(out.top_logprobs[1, 1]).all())
    assert out.top_ids[0, 1].tolist() == [6, 5, 4] and out["top_logprobs"][0, 1].tolist() == [-2.0] * 3
    plain = generation.build(seq, flags)
    assert "top_ids" not in plain and plain.top_ids is None and plain.top_logprobs is None
    assert generation.mask_ids_after_end(ids[0], None) is ids[0]


def test_beam_search_refuses_top_logprobs():
    with pytest.raises(NotImplementedError, match=r"beam search.*top_logprobs not implemented"):
        InternVLChatModel._gen_flags(None, {}, beams={"num_beams": 3}, topk=5)
    with pytest.raises(NotImplementedError, match=r"candidate_ids, top_logprobs"):
        InternVLChatModel._gen_flags(None, {}, beams={"num_beams": 3}, cand=torch.tensor([1]), topk=5)
    assert InternVLChatModel._gen_flags(None, {}, beams={"num_beams": 3}) == {k: False for k in generation.FLAGS}
    assert InternVLChatModel._gen_flags(None, {}, topk=5) == {k: False for k in generation.FLAGS}


class _FakeModel:
    """Stands in for the GPU model: top_ids[b, p, j] = 10 b + j and top_logprob = -(b + 1) - j / 8 at the answer rows; records its kwargs."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def prefetch(self, pixel_values=None, n_clips=0, **kw):
        return pixel_values

    def __call__(self, **kw):
        self.calls.append(kw)
        lab = kw["labels"][:, 1:]
        B, n = lab.shape
        out = {"logit": torch.zeros(B * n, dtype=torch.long), "label": lab.reshape(-1), "score1": torch.zeros(B, dtype=torch.bfloat16)}
        k = kw.get("top_logprobs")
        if k is not None:
            j = torch.arange(k)
            ids = (10 * torch.arange(B).view(B, 1, 1) + j).expand(B, n, k)
            lp = (-(torch.arange(B).view(B, 1, 1) + 1.0) - j / 8).expand(B, n, k)
            scored = (lab != -100).unsqueeze(-1)
            out["top_ids"] = torch.where(scored, ids, torch.full_like(ids, -1)).reshape(B * n, k)
            out["top_logprob"] = torch.where(scored, lp, torch.full_like(lp, float("nan"))).reshape(B * n, k)
        return out


def test_batched_hands_every_item_its_own_rows():
    items = []
    for n in (6, 4, 7):
        lab = torch.full((1, n), -100)
        lab[0, -2:] = 3
        items.append({"input_ids": torch.ones(1, n, dtype=torch.long), "attention_mask": torch.ones(1, n, dtype=torch.bool), "labels": lab,
                      "pixel_values": torch.zeros(1, 2, 3, 8, 8)})
    fake = _FakeModel()
    plain = list(eval_utils.batched(items, fake, k=3, ahead=False))
    assert "top_logprobs" not in fake.calls[0] and "top_ids" not in plain[0][1]
    fake = _FakeModel()
    got = list(eval_utils.batched(items, fake, k=3, ahead=False, top_logprobs=4))
    assert fake.calls[0]["top_logprobs"] == 4 and len(got) == 3
    for b, (it, o) in enumerate(got):
        n = it["input_ids"].shape[1]
        assert o["top_ids"].shape == o["top_logprob"].shape == (n - 1, 4)
        assert o["top_ids"][-1].tolist() == [10 * b + j for j in range(4)] and o["top_ids"][0].tolist() == [-1] * 4
        assert o["top_logprob"][-1].tolist() == [-(b + 1.0) - j / 8 for j in range(4)] and bool(torch.isnan(o["top_logprob"][0]).all())
