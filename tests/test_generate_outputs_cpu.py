"""generate()'s HF-style outputs without a GPU: the C entry points of the fused lm-head log-probabilities (header, exports, ctypes
prototypes, host-side argument checks), the output flags and object, the log-probabilities taken from a step's scores and the
NaN-after-end rule - pinned against the installed transformers' ``compute_transition_scores`` - and beam search's ``sequences_scores``
against transformers' own ``generate(num_beams > 1, return_dict_in_generate=True)``."""
import ctypes
import math
import os
import re

import pytest
import torch

from aigv_assessor_amd import beam, generation, native
from aigv_assessor_amd.modeling import InternVLChatModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = native._P, native._I
NEW = {
    "aigv_decode_step_logprob": (I, [P, P, P, P, P]),
    "aigv_op_lm_head_argmax_logprob": (I, [P, I, I, P, I, P, ctypes.c_int64, P, P, P, P]),
    "aigv_op_lm_head_argmax_logprob_scratch_bytes": (ctypes.c_int64, [I, I]),
}
FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it: a call that reached the device would fault or fail with a HIP error


@pytest.fixture(scope="module")
def lib():
    return native.load()


def test_fused_logprob_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, (res, args) in NEW.items():
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == (res, args), name
        getattr(lib, name)


def test_scratch_size_query(lib):
    f = lib.aigv_op_lm_head_argmax_logprob_scratch_bytes
    for rows, vocab in ((1, 1), (64, 92553), (5, 2053), (64, 16), (3, 17)):
        assert f(rows, vocab) == 64 * 8 + rows * math.ceil(vocab / 16) * 8
    for rows, vocab in ((0, 10), (65, 10), (4, 0), (-1, 5)):
        assert f(rows, vocab) == -1


def _refused(lib, rc, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG, not AIGV_ERR_HIP
    assert msg.startswith("aigv_op_lm_head_argmax_logprob:") and re.search(what, msg), msg


def test_op_refuses_bad_arguments_before_any_launch(lib):
    op = lib.aigv_op_lm_head_argmax_logprob
    need = lib.aigv_op_lm_head_argmax_logprob_scratch_bytes(4, 1000)
    good = dict(h=FAKE, rows=4, hidden=256, W=FAKE, vocab=1000, scratch=FAKE, nbytes=need, idx=FAKE, val=FAKE, lp=FAKE)

    def call(**kw):
        a = dict(good, **kw)
        return op(a["h"], a["rows"], a["hidden"], a["W"], a["vocab"], a["scratch"], a["nbytes"], a["idx"], a["val"], a["lp"], None)

    _refused(lib, call(h=None), "null operand")
    _refused(lib, call(W=None), "null operand")
    _refused(lib, call(scratch=None), "null operand")
    _refused(lib, call(idx=None), "null operand")
    _refused(lib, call(lp=None), "null operand")
    _refused(lib, call(rows=0), r"rows = 0 outside 1\.\.64")
    _refused(lib, call(rows=65), r"rows = 65 outside 1\.\.64")
    _refused(lib, call(hidden=100), "hidden = 100")
    _refused(lib, call(hidden=0), "hidden = 0")
    _refused(lib, call(vocab=0), "vocab = 0")
    _refused(lib, call(h=FAKE + 8), "aligned")
    _refused(lib, call(scratch=FAKE + 4), "aligned")
    _refused(lib, call(nbytes=need - 1), f"scratch of {need - 1} bytes, needs {need}")
    _refused(lib, call(rows=5), "needs")                           # the size follows the rows


def test_decode_step_logprob_refuses_without_state(lib):
    rc = lib.aigv_decode_step_logprob(None, FAKE, FAKE, FAKE, None)
    assert rc == -1 and "aigv_decode_step_logprob" in lib.aigv_last_error(None).decode()


# ---- flags and the output object -------------------------------------------------------------------------------------------------

def test_output_flags_from_kwargs_and_config():
    off = {k: False for k in generation.FLAGS}
    assert generation.output_flags(None, {}) == off
    assert generation.output_flags({"max_new_tokens": 3}, {}) == off
    assert generation.output_flags({"output_scores": True}, {"return_dict_in_generate": 1}) == dict(off, output_scores=True, return_dict_in_generate=True)
    assert generation.output_flags({"output_logits": True}, {"output_logits": False}) == off          # kwargs win

    class Cfg:                                                                                         # a GenerationConfig-like object
        return_dict_in_generate = True
        output_scores = False
        return_logprobs = True
    assert generation.output_flags(Cfg(), {}) == dict(off, return_dict_in_generate=True, return_logprobs=True)
    assert not generation.wants_output(dict(off, output_scores=True, output_logits=True))            # as HF: scores only inside the dict
    assert generation.wants_output(dict(off, return_dict_in_generate=True))
    assert generation.wants_output(dict(off, return_logprobs=True))
    # _gen_args ignores the output flags
    assert InternVLChatModel._gen_args(dict(max_new_tokens=4, return_dict_in_generate=True, output_scores=True, return_logprobs=True), {}) == \
        InternVLChatModel._gen_args(dict(max_new_tokens=4), {})


def test_beam_search_refuses_per_step_outputs():
    beams = InternVLChatModel._gen_args(dict(num_beams=3), {})[5]
    assert InternVLChatModel._gen_flags(dict(return_dict_in_generate=True), {}, beams)["return_dict_in_generate"]
    for k in ("output_scores", "output_logits", "return_logprobs"):
        with pytest.raises(NotImplementedError, match=k):
            InternVLChatModel._gen_flags({}, {k: True, "return_dict_in_generate": True}, beams)
    assert InternVLChatModel._gen_flags({}, {"output_scores": True}, None)["output_scores"]


def test_generate_output_object():
    seq = torch.tensor([[5, 2, 0], [7, 8, 2]])
    flags = {k: True for k in generation.FLAGS}
    sc = [torch.randn(2, 11) for _ in range(4)]
    lp = [torch.randn(2) for _ in range(4)]
    out = generation.build(seq, flags, scores=sc, logits=sc, logprobs=lp)
    assert out.sequences is seq and out["sequences"] is seq
    assert isinstance(out.scores, tuple) and len(out.scores) == 3 and out.scores[2] is sc[2]
    assert len(out["logits"]) == 3
    assert out.logprobs.shape == (2, 3) and torch.equal(out.logprobs[:, 1], lp[1])
    assert out.sequences_scores is None and "sequences_scores" not in out
    with pytest.raises(AttributeError):
        out.not_a_field
    plain = generation.build(seq, dict({k: False for k in generation.FLAGS}, return_dict_in_generate=True))
    assert set(plain) == {"sequences"} and plain.scores is None and plain.logprobs is None
    bs = generation.build(seq, dict({k: False for k in generation.FLAGS}, return_dict_in_generate=True), sequences_scores=torch.zeros(2))
    assert set(bs) == {"sequences", "sequences_scores"}


# ---- log-probabilities from scores, against transformers -------------------------------------------------------------------------

def _tiny_hf_lm(vocab: int, seed: int):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=vocab, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    m = LlamaForCausalLM(cfg).double().eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(12.0)
    return m


@pytest.mark.parametrize("kw", [
    dict(do_sample=False),
    dict(do_sample=False, repetition_penalty=1.3),
    dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9),
])
def test_logprobs_from_scores_match_compute_transition_scores(kw):
    """What generate()'s loop does per column (token_logprobs of the step's scores, NaN once the sequence has ended) equals transformers'
    compute_transition_scores(sequences, scores, normalize_logits=True) at every live column."""
    V, P, B = 11, 5, 4
    for seed in range(3):
        lm = _tiny_hf_lm(V, seed)
        g = torch.Generator().manual_seed(7 + seed)
        emb = lm.get_input_embeddings()(torch.randint(3, V, (B, P), generator=g))
        torch.manual_seed(seed)
        with torch.no_grad():
            o = lm.generate(inputs_embeds=emb, attention_mask=torch.ones(B, P, dtype=torch.long), max_new_tokens=8, eos_token_id=2,
                            pad_token_id=0, return_dict_in_generate=True, output_scores=True, **kw)
        seq = o.sequences
        T = seq.shape[1]
        assert len(o.scores) == T
        want = lm.compute_transition_scores(seq, o.scores, normalize_logits=True)
        ended = torch.zeros(B, dtype=torch.bool)
        cols = []
        for t in range(T):
            cols.append(generation.mask_after_end(generation.token_logprobs(o.scores[t], seq[:, t]), ~ended))
            ended |= seq[:, t] == 2
        got = torch.stack(cols, 1)
        live = ~torch.isnan(got)
        assert torch.allclose(got[live], want[live].float(), atol=1e-6, rtol=0), (got, want)
        # NaN exactly after the end token, never at it
        for b in range(B):
            hits = (seq[b] == 2).nonzero().flatten().tolist()
            first = hits[0] if hits else T
            assert live[b, :first + 1].all() and not live[b, first + 1:].any()


def test_mask_after_end():
    lp = torch.tensor([-0.5, -1.0, -2.0])
    assert torch.equal(generation.mask_after_end(lp, None), lp)
    got = generation.mask_after_end(lp, torch.tensor([True, False, True]))
    assert got[0] == -0.5 and math.isnan(got[1]) and got[2] == -2.0


@pytest.mark.parametrize("num_beams,eos,length_penalty,early_stopping,max_new", [
    (2, [2], 1.0, False, 6),
    (3, [2], 2.0, False, 8),
    (4, [2], 0.6, True, 9),
    (3, [], 1.0, False, 5),
])
def test_beam_sequences_scores_follow_transformers(num_beams, eos, length_penalty, early_stopping, max_new):
    """beam.beam_search(return_scores=True) against transformers' generate(num_beams, return_dict_in_generate=True, output_scores=True):
    the same sequences and the same sequences_scores (HF's length-penalised hypothesis score)."""
    V, P, B = 11, 5, 3
    for seed in range(3):
        lm = _tiny_hf_lm(V, seed)
        g = torch.Generator().manual_seed(100 + seed)
        emb = lm.get_input_embeddings()(torch.randint(3, V, (B, P), generator=g))
        with torch.no_grad():
            want = lm.generate(inputs_embeds=emb, attention_mask=torch.ones(B, P, dtype=torch.long), max_new_tokens=max_new,
                               num_beams=num_beams, do_sample=False, length_penalty=length_penalty, early_stopping=early_stopping,
                               eos_token_id=(eos if eos else None), pad_token_id=0, return_dict_in_generate=True, output_scores=True)
        hist = {"tok": torch.zeros((B, num_beams, 0), dtype=torch.long)}

        def logits_of(tok_hist):
            t = tok_hist.shape[2]
            e = emb[:, None].expand(B, num_beams, P, emb.shape[-1]).reshape(B * num_beams, P, -1)
            if t:
                e = torch.cat((e, lm.get_input_embeddings()(tok_hist.reshape(B * num_beams, t))), dim=1)
            with torch.no_grad():
                return lm(inputs_embeds=e).logits[:, -1, :].float().view(B, num_beams, V)

        def reorder(parent):
            hist["tok"] = torch.gather(hist["tok"], 1, parent[:, :, None].expand(-1, -1, hist["tok"].shape[2]))

        def step(tok):
            hist["tok"] = torch.cat((hist["tok"], tok[:, :, None]), dim=2)
            return logits_of(hist["tok"])

        first = logits_of(hist["tok"])[:, 0, :]
        seq, score = beam.beam_search(first, step, reorder, num_beams, max_new, eos_ids=eos, pad_id=0, length_penalty=length_penalty,
                                      early_stopping=early_stopping, return_scores=True)
        assert torch.equal(seq, want.sequences), (seed, seq.tolist(), want.sequences.tolist())
        assert score.dtype == torch.float32 and score.shape == (B,)
        assert torch.allclose(score, want.sequences_scores.float(), atol=1e-6, rtol=1e-6), (score, want.sequences_scores)
