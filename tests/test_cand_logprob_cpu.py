"""Candidate-token log-probabilities without a GPU: ``eval_utils.expected_level``, ``prompts.level_token_ids`` on the stub tokenizer, the
C ABI the feature adds (header, exports, ctypes prototypes; the ABI constants of header, binding and library agree), the host-side argument checks of the new entry points - a
refused call returns AIGV_ERR_ARG with a message naming the op before anything reaches the device - and the host-side plumbing of
``candidate_ids`` (``_candidates``, ``generation.candidate_logprobs`` / ``build``, ``eval_utils.batched``)."""
import ctypes
import os
import re

import pytest
import torch

from aigv_assessor_amd import eval_utils, generation, native, prompts
from stub_tokenizer import StubTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = native._P, native._I
NEW = {
    "aigv_op_cand_logprob": [P, I, I, I, P, I, P, P],
    "aigv_out_row_cand_logprob": [P, I, I, P, I, P, P],
    "aigv_decode_step_cand_logprob": [P, P, P, P, P, I, P, P],
    "aigv_op_lm_head_argmax_cand_logprob": [P, I, I, P, I, P, I, P, ctypes.c_int64, P, P, P, P, P],
    "aigv_op_lm_head_argmax_cand_logprob_scratch_bytes": [I, I],
}
FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it: a call that reached the device would fault or fail with a HIP error


def test_expected_level_against_fp64():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 5, generator=g) * 4 - 9
    x[3] = float("nan")
    got = eval_utils.expected_level(x)
    assert got.shape == (7,) and got.dtype == torch.float32
    p = torch.softmax(x.double(), -1)
    want = (p * torch.tensor([1, 2, 3, 4, 5], dtype=torch.float64)).sum(-1)
    ok = torch.arange(7) != 3
    assert torch.isnan(got[3]) and not torch.isnan(got[ok]).any()
    assert (got[ok].double() - want[ok]).abs().max().item() <= 5 * 2 ** -22          # five terms <= 5, each within an fp32 rounding or two
    assert bool(((got[ok] >= 1) & (got[ok] <= 5)).all())
    # a certain answer gives its own level; other weights, leading dimensions
    sure = torch.full((5,), -80.0)
    sure[3] = 0.0
    assert eval_utils.expected_level(sure).item() == 4.0
    y = torch.randn(2, 3, 4, generator=g)
    w = (0.0, 1.0, 2.5, 10.0)
    want = (torch.softmax(y.double(), -1) * torch.tensor(w, dtype=torch.float64)).sum(-1)
    assert (eval_utils.expected_level(y, weights=w).double() - want).abs().max().item() <= 1e-5


def test_level_token_ids_on_the_stub_tokenizer():
    tok = StubTokenizer()
    ids = prompts.level_token_ids(tok)
    assert ids == [tok.encode(c, add_special_tokens=False)[0] for c in "bpfge"]        # character level: the words' first letters, in context
    # the position is the first that differs between the candidates, not a fixed offset: a shared stem is skipped
    ids = prompts.level_token_ids(tok, words=("very bad", "very good"), template="It is {}.")
    assert ids == [tok.encode("b", add_special_tokens=False)[0], tok.encode("g", add_special_tokens=False)[0]]
    assert prompts.level_token_ids(tok, words=("fair",)) == [tok.encode("f", add_special_tokens=False)[0]]
    with pytest.raises(ValueError, match="'good' and 'great' share"):
        prompts.level_token_ids(tok, words=("bad", "good", "great"))
    with pytest.raises(ValueError, match="do not differ"):
        prompts.level_token_ids(tok, words=("good", "good"))
    with pytest.raises(ValueError, match=r"needs a \{\}"):
        prompts.level_token_ids(tok, template="no slot")


def test_abi_declares_and_exports_the_candidate_entry_points():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    version = int(re.search(r"#define AIGV_ABI_VERSION (\d+)\b", header).group(1))
    assert version == native.ABI_VERSION
    assert re.search(r"#define AIGV_MAX_CANDIDATES 64\b", header)
    lib = ctypes.CDLL(native.LIB_PATH)
    assert lib.aigv_abi_version() == version
    for name, args in NEW.items():
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
        assert native.PROTOTYPES[name][1] == args, name
        getattr(lib, name)
    assert native.PROTOTYPES["aigv_op_lm_head_argmax_cand_logprob_scratch_bytes"][0] is ctypes.c_int64
    # every prototype the binding lists is declared in the header
    for name in native.PROTOTYPES:
        assert re.search(r"\b" + name + r"\(", header), name


def test_a_library_without_the_new_symbols_is_refused_by_name(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name == "aigv_out_row_cand_logprob":
                raise AttributeError(name)
            return lambda *a: 3
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native.C, "CDLL", lambda path: Old())
    with pytest.raises(native.NativeError, match=r"ABI mismatch.*missing aigv_out_row_cand_logprob"):
        native.load()


def _refused(lib, rc, op, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG, not AIGV_ERR_HIP
    assert msg.startswith(op + ":") and re.search(what, msg), msg


def test_candidate_entry_points_refuse_bad_arguments_on_the_host():
    lib = native.load()
    op = "aigv_op_cand_logprob"
    call = lambda logits=FAKE, rows=2, V=100, ldo=100, cand=FAKE, C=5, out=FAKE: lib.aigv_op_cand_logprob(logits, rows, V, ldo, cand, C, out, None)
    _refused(lib, call(C=0), op, r"C = 0 candidates outside 1\.\.64")
    _refused(lib, call(C=65), op, r"C = 65 candidates outside 1\.\.64")
    _refused(lib, call(cand=None), op, r"null operand")
    _refused(lib, call(out=None), op, r"null operand")
    _refused(lib, call(logits=None), op, r"null operand")
    _refused(lib, call(ldo=99), op, r"ldo 99")
    _refused(lib, call(V=0, ldo=0), op, r"vocab 0")
    op = "aigv_op_lm_head_argmax_cand_logprob"
    sb = lib.aigv_op_lm_head_argmax_cand_logprob_scratch_bytes
    assert sb(0, 100) == -1 and sb(65, 100) == -1 and sb(1, 0) == -1
    for rows, V in ((1, 1), (3, 92553), (64, 2053)):
        base = lib.aigv_op_lm_head_argmax_logprob_scratch_bytes(rows, V)
        assert sb(rows, V) == (base + 15) // 16 * 16 + rows * 64 * 2              # + [rows][64] bf16 candidate logits

    def head(h=FAKE, rows=2, H=256, W=FAKE, V=100, cand=FAKE, C=5, scratch=FAKE, nbytes=None, idx=FAKE, val=FAKE, lp=FAKE, clp=FAKE):
        nbytes = max(sb(max(1, min(rows, 64)), max(V, 1)), 0) if nbytes is None else nbytes
        return lib.aigv_op_lm_head_argmax_cand_logprob(h, rows, H, W, V, cand, C, scratch, nbytes, idx, val, lp, clp, None)
    _refused(lib, head(C=0), op, r"C = 0 candidates")
    _refused(lib, head(C=65), op, r"C = 65 candidates")
    for k in ("h", "W", "cand", "scratch", "idx", "lp", "clp"):
        _refused(lib, head(**{k: None}), op, r"null operand")
    _refused(lib, head(rows=0), op, r"rows = 0")
    _refused(lib, head(rows=65), op, r"rows = 65")
    _refused(lib, head(H=200), op, r"hidden = 200")
    _refused(lib, head(V=0), op, r"vocab = 0")
    _refused(lib, head(h=FAKE + 2), op, r"16-byte aligned")
    need = sb(2, 100)
    _refused(lib, head(nbytes=need - 1), op, rf"scratch of {need - 1} bytes, needs {need}")
    # the context entry points check C and their pointers before they look at the context
    _refused(lib, lib.aigv_out_row_cand_logprob(None, 0, 1, FAKE, 0, FAKE, None), "aigv_out_row_cand_logprob", r"C = 0 candidates")
    _refused(lib, lib.aigv_out_row_cand_logprob(None, 0, 1, FAKE, 65, FAKE, None), "aigv_out_row_cand_logprob", r"C = 65 candidates")
    _refused(lib, lib.aigv_out_row_cand_logprob(None, 0, 1, FAKE, 5, FAKE, None), "aigv_out_row_cand_logprob", r"null argument")
    _refused(lib, lib.aigv_decode_step_cand_logprob(None, FAKE, FAKE, FAKE, FAKE, 0, FAKE, None), "aigv_decode_step_cand_logprob", r"C = 0 candidates")
    _refused(lib, lib.aigv_decode_step_cand_logprob(None, FAKE, FAKE, FAKE, None, 5, FAKE, None), "aigv_decode_step_cand_logprob", r"null argument")
    _refused(lib, lib.aigv_decode_step_cand_logprob(None, FAKE, FAKE, FAKE, FAKE, 5, FAKE, None), "aigv_decode_step_cand_logprob", r"null argument")


def test_candidate_ids_are_normalised_and_checked_on_the_host():
    from aigv_assessor_amd.modeling import InternVLChatModel as M
    assert M._candidates(None) is None
    t = M._candidates([5, 7, 9])
    assert t.dtype == torch.long and t.tolist() == [5, 7, 9]
    assert M._candidates(torch.tensor([3], dtype=torch.int32)).dtype == torch.long
    assert M._candidates(list(range(64))).numel() == 64
    for bad in ([], list(range(65)), torch.zeros(2, 2, dtype=torch.long), torch.tensor([1.0, 2.0]), torch.tensor([True])):
        with pytest.raises(ValueError, match="candidate_ids"):
            M._candidates(bad)
    with pytest.raises(ValueError, match="needs labels"):
        M._candidates([1, 2], None)


def test_generation_helpers_carry_the_candidates():
    g = torch.Generator().manual_seed(2)
    raw = torch.randn(3, 50, generator=g) * 3
    cand = torch.tensor([0, 49, 7, 50, -1, 7])
    got = generation.candidate_logprobs(raw, cand)
    assert got.shape == (3, 6) and got.dtype == torch.float32
    assert torch.isnan(got[:, 3]).all() and torch.isnan(got[:, 4]).all()
    for c in (0, 1, 2, 5):
        assert torch.equal(got[:, c], generation.token_logprobs(raw, cand[c].expand(3)))
    live = torch.tensor([True, False, True])
    masked = generation.mask_after_end(got[:, :3], live)
    assert torch.isnan(masked[1]).all() and torch.equal(masked[0], got[0, :3]) and torch.equal(masked[2], got[2, :3])
    assert torch.equal(generation.mask_after_end(got[:, 0], live).isnan(), ~live)          # the [B] form is what it was
    flags = {k: False for k in generation.FLAGS}
    seq = torch.zeros(3, 2, dtype=torch.long)
    out = generation.build(seq, flags, cand_logprobs=[got[:, :3], masked, got[:, :3]])
    assert out.cand_logprobs.shape == (3, 2, 3) and torch.equal(out.cand_logprobs[:, 0], got[:, :3])
    assert "cand_logprobs" not in generation.build(seq, flags) and generation.build(seq, flags).cand_logprobs is None


class _FakeModel:
    """Stands in for the GPU model: cand_logprob[b, p, c] = -(b + 1) (p + 1) - c / 8 at the answer rows, NaN rows elsewhere; records its kwargs."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def prefetch(self, pixel_values=None, frames_u8=None, n_clips=1):
        return pixel_values

    def __call__(self, **kw):
        self.calls.append(kw)
        lab = kw["labels"][:, 1:]
        B, n = lab.shape
        out = {"logit": torch.zeros(B * n, dtype=torch.long), "label": lab.reshape(-1), "score1": torch.zeros(B, dtype=torch.bfloat16)}
        if kw.get("candidate_ids") is not None:
            C = len(kw["candidate_ids"])
            v = -(torch.arange(1, B + 1).view(-1, 1, 1) * torch.arange(1, n + 1).view(1, -1, 1)).float() - torch.arange(C).view(1, 1, -1) / 8
            out["cand_logprob"] = torch.where((lab != -100).unsqueeze(-1), v, torch.full_like(v, float("nan"))).reshape(B * n, C)
        return out


def test_batched_passes_the_candidates_and_splits_them_per_item():
    shapes = ((12, 3), (9, 4), (15, 0))
    items = []
    for n, n_ans in shapes:
        ids = torch.arange(3, 3 + n).view(1, -1)
        lab = torch.full((1, n), -100)
        if n_ans:
            lab[0, -n_ans:] = ids[0, -n_ans:]
        items.append({"input_ids": ids, "attention_mask": torch.ones(1, n, dtype=torch.bool), "labels": lab, "pixel_values": torch.zeros(1, 1, 3, 4, 4)})
    fake = _FakeModel()
    plain = list(eval_utils.batched(items, fake, k=3))
    assert "candidate_ids" not in fake.calls[0] and "cand_logprob" not in plain[0][1]
    fake = _FakeModel()
    got = list(eval_utils.batched(items, fake, k=3, candidate_ids=[4, 5, 6, 7, 8]))
    assert fake.calls[0]["candidate_ids"] == [4, 5, 6, 7, 8] and "return_logprobs" not in fake.calls[0]
    for b, ((it, o), (n, n_ans)) in enumerate(zip(got, shapes)):
        x = o["cand_logprob"]
        assert x.shape == (n - 1, 5)
        rows = torch.zeros(n - 1, dtype=torch.bool)
        if n_ans:
            rows[n - 1 - n_ans:] = True
        assert torch.equal(torch.isnan(x), ~rows.view(-1, 1).expand(-1, 5))
        p = rows.nonzero().flatten()
        want = -((b + 1) * (p + 1)).float().view(-1, 1) - torch.arange(5).view(1, -1) / 8
        assert torch.equal(x[rows], want)
        lvl = eval_utils.expected_level(x)
        assert torch.equal(torch.isnan(lvl), ~rows)
