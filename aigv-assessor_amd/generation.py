"""What ``generate`` / ``generate2`` / ``generate_stage2`` return beyond the token tensor: HF's ``return_dict_in_generate`` output.

The reference's generate paths hand ``**generate_kwargs`` to HF's ``language_model.generate`` (modeling_internvl_chat.py:798-809), so a caller
may ask for ``return_dict_in_generate=True`` with ``output_scores`` / ``output_logits`` and read ``out.sequences`` / ``out.scores``.  This
module holds the host-side part of that: which flags were asked for, the output object (attribute and key access, like transformers'
``ModelOutput``, without depending on transformers) and the log-probabilities of emitted tokens under the scores they were drawn from.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

FLAGS = ("return_dict_in_generate", "output_scores", "output_logits", "return_logprobs")
FIELDS = ("sequences", "sequences_scores", "scores", "logits", "logprobs", "cand_logprobs", "top_ids", "top_logprobs")


class GenerateOutput(dict):
    """The ``return_dict_in_generate`` result: ``out.sequences`` and ``out["sequences"]`` alike.

    sequences          long [B, T]: the tensor generate returns without the flags
    scores             (output_scores) tuple of T fp32 [B, V]: the processed scores of each step (after repetition penalty / n-gram
                       blocking; for sampling also after temperature / top-k / top-p) - HF's ``scores``
    logits             (output_logits) tuple of T fp32 [B, V]: the raw lm-head logits of each step
    logprobs           (return_logprobs) fp32 [B, T]: log-probability of each emitted token under the distribution it was chosen from
                       (``compute_transition_scores(sequences, scores, normalize_logits=True)``), NaN after the sequence's end token
    cand_logprobs      (candidate_ids) fp32 [B, T, C]: full-vocabulary log-probability of each candidate token at each step under the RAW
                       lm-head logits (before logits processors / sampling warpers), NaN after the sequence's end token
    top_ids            (top_logprobs=k) long [B, T, k]: the ids of the k largest RAW lm-head logits of each step, equal logits by ascending
                       id (entry 0 is the greedy token), -1 after the sequence's end token
    top_logprobs       (top_logprobs=k) fp32 [B, T, k]: their full-vocabulary log-probabilities, NaN after the sequence's end token
    sequences_scores   (beam search) fp32 [B]: HF's length-penalised score of the returned hypothesis
    A field that was not asked for is absent from the keys and reads as None, as in transformers' output classes."""

    def __getattr__(self, name):
        if name in self:
            return self[name]
        if name in FIELDS:
            return None
        raise AttributeError(name)


def output_flags(generation_config, kw: Dict) -> Dict[str, bool]:
    """The four output flags from a generation config (dict or object) and the call's kwargs (kwargs win), all False by default."""
    if isinstance(generation_config, dict):
        cfg = {k: generation_config.get(k) for k in FLAGS}
    else:
        cfg = {k: getattr(generation_config, k, None) for k in FLAGS}
    cfg.update({k: kw[k] for k in FLAGS if k in kw})
    return {k: bool(cfg.get(k)) for k in FLAGS}


def wants_output(flags: Dict[str, bool]) -> bool:
    """True when generate returns a GenerateOutput: ``return_dict_in_generate``, or ``return_logprobs`` (which only the output object can
    carry).  ``output_scores`` / ``output_logits`` alone change nothing, as in HF (the scores are returned only inside the dict)."""
    return flags["return_dict_in_generate"] or flags["return_logprobs"]


def token_logprobs(scores: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """fp32 [B]: log_softmax(scores)[b, tokens[b]] - one column of ``compute_transition_scores(..., normalize_logits=True)``."""
    return torch.log_softmax(scores.float(), dim=-1).gather(1, tokens.view(-1, 1).long()).view(-1)


def candidate_logprobs(raw_logits: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """fp32 [B, C]: log_softmax(raw_logits.float())[:, cand] over the full vocabulary; a NaN column for an id outside [0, V)."""
    V = raw_logits.shape[-1]
    cand = cand.to(raw_logits.device).long()
    ok = (cand >= 0) & (cand < V)
    lp = torch.log_softmax(raw_logits.float(), dim=-1).index_select(1, cand.clamp(0, V - 1))
    return torch.where(ok.view(1, -1), lp, torch.full_like(lp, float("nan")))


def top_logprobs(raw_logits: torch.Tensor, k: int):
    """(long [B, k], fp32 [B, k]): the ids of the k largest ``raw_logits.float()`` of every row - equal logits by ascending id: the first k
    of a stable descending sort, the order of the lm-head's fused argmax - and ``log_softmax(raw_logits.float())`` at them."""
    x = raw_logits.float()
    if not 1 <= int(k) <= x.shape[-1]:
        raise ValueError(f"top_logprobs: k = {k} outside 1..{x.shape[-1]}")
    ids = torch.sort(x, dim=-1, descending=True, stable=True).indices[..., : int(k)].contiguous()
    return ids, torch.log_softmax(x, dim=-1).gather(-1, ids)


def mask_ids_after_end(ids: torch.Tensor, live: Optional[torch.Tensor]) -> torch.Tensor:
    """mask_after_end for token ids: -1 where the sequence had already ended."""
    if live is None:
        return ids
    return torch.where(live.view(-1, *([1] * (ids.dim() - 1))), ids, torch.full_like(ids, -1))


def mask_after_end(logprob: torch.Tensor, live: Optional[torch.Tensor]) -> torch.Tensor:
    """A column's log-probabilities ([B] or [B, C]) with NaN where the sequence had already ended before it (``live`` False; None = all live)."""
    if live is None:
        return logprob
    return torch.where(live.view(-1, *([1] * (logprob.dim() - 1))), logprob, torch.full_like(logprob, float("nan")))


def build(sequences: torch.Tensor, flags: Dict[str, bool], scores: Sequence[torch.Tensor] = (), logits: Sequence[torch.Tensor] = (),
          logprobs: Sequence[torch.Tensor] = (), sequences_scores: Optional[torch.Tensor] = None,
          cand_logprobs: Optional[Sequence[torch.Tensor]] = None, top_ids: Optional[Sequence[torch.Tensor]] = None,
          top_logprobs: Optional[Sequence[torch.Tensor]] = None) -> GenerateOutput:
    """The output object of one generate call; per-step lists are cut to the returned length."""
    T = sequences.shape[1]
    out = GenerateOutput(sequences=sequences)
    if flags["output_scores"]:
        out["scores"] = tuple(scores[:T])
    if flags["output_logits"]:
        out["logits"] = tuple(logits[:T])
    if flags["return_logprobs"]:
        lp = list(logprobs[:T])
        out["logprobs"] = torch.stack(lp, dim=1) if lp else torch.empty((sequences.shape[0], 0), dtype=torch.float32, device=sequences.device)
    if cand_logprobs is not None:       # candidate_ids: T x [B, C] -> [B, T, C]
        out["cand_logprobs"] = torch.stack(list(cand_logprobs[:T]), dim=1)
    if top_ids is not None:             # top_logprobs=k: T x [B, k] -> [B, T, k]
        out["top_ids"] = torch.stack(list(top_ids[:T]), dim=1)
        out["top_logprobs"] = torch.stack(list(top_logprobs[:T]), dim=1)
    if sequences_scores is not None:
        out["sequences_scores"] = sequences_scores
    return out


def gen_args(generation_config, kw):
    """(max_new_tokens, eos ids, pad id, sampler, processors, beams) from a HF-style generation config / kwargs.  ``sampler`` is None for greedy
    decoding or the warper settings of HF's multinomial sampling (temperature -> top-k -> top-p, transformers' order and
    defaults: top_k 50, top_p 1.0, temperature 1.0); ``processors`` = HF's repetition-penalty / no-repeat-n-gram logits processors
    when asked for; ``beams`` is None or HF's beam-search settings (num_beams > 1: num_beams, length_penalty, early_stopping)."""
    cfg = dict(generation_config) if isinstance(generation_config, dict) else {}
    if generation_config is not None and not isinstance(generation_config, dict):
        cfg = {k: getattr(generation_config, k) for k in ("max_new_tokens", "do_sample", "num_beams", "eos_token_id", "pad_token_id",
                                                          "temperature", "top_k", "top_p", "repetition_penalty", "no_repeat_ngram_size",
                                                          "length_penalty", "early_stopping", "num_return_sequences", "num_beam_groups")
               if hasattr(generation_config, k)}
    cfg.update(kw)
    beams = None
    if (cfg.get("num_beams") or 1) > 1:
        if cfg.get("do_sample"):
            raise NotImplementedError("beam-search multinomial sampling is not implemented on the gfx950 path (beam search, greedy and sampling are)")
        if (cfg.get("num_return_sequences") or 1) != 1 or (cfg.get("num_beam_groups") or 1) != 1:
            raise NotImplementedError("beam search returns the best hypothesis only (num_return_sequences = 1, no beam groups)")
        beams = dict(num_beams=int(cfg["num_beams"]), length_penalty=float(cfg["length_penalty"]) if cfg.get("length_penalty") is not None else 1.0,
                     early_stopping=cfg.get("early_stopping") if cfg.get("early_stopping") is not None else False)
    processors = []       # HF's order (GenerationMixin._get_logits_processor): repetition penalty, then n-gram blocking
    if cfg.get("repetition_penalty") not in (None, 1, 1.0):
        processors.append(repetition_penalty(float(cfg["repetition_penalty"])))
    if cfg.get("no_repeat_ngram_size") not in (None, 0):
        processors.append(no_repeat_ngram(int(cfg["no_repeat_ngram_size"])))
    sampler = None
    if cfg.get("do_sample"):
        sampler = dict(temperature=float(cfg["temperature"]) if cfg.get("temperature") is not None else 1.0,
                       top_k=int(cfg["top_k"]) if cfg.get("top_k") is not None else 50,
                       top_p=float(cfg["top_p"]) if cfg.get("top_p") is not None else 1.0, generator=cfg.get("generator"))
        if sampler["temperature"] <= 0 or not (0 < sampler["top_p"] <= 1.0) or sampler["top_k"] < 0:
            raise ValueError(f"bad sampling settings {sampler}")
    eos = cfg.get("eos_token_id")
    eos = [] if eos is None else ([int(eos)] if not isinstance(eos, (list, tuple)) else [int(e) for e in eos])
    return int(cfg.get("max_new_tokens") or 20), eos, cfg.get("pad_token_id"), sampler, processors, beams


def gen_flags(generation_config, kw, beams=None, cand=None, topk=0):
    """HF's output flags (return_dict_in_generate, output_scores, output_logits) and return_logprobs from a generation config / kwargs
    (generation.output_flags).  Beam search returns ``sequences_scores`` only: per-step scores, logits and log-probabilities of its
    hypotheses are not implemented and raise."""
    flags = output_flags(generation_config, kw)
    if beams:
        asked = [k for k in ("output_scores", "output_logits", "return_logprobs") if flags[k]] + (["candidate_ids"] if cand is not None else []) + \
            (["top_logprobs"] if topk else [])
        if asked:
            raise NotImplementedError(f"beam search (num_beams > 1) returns sequences and sequences_scores only: {', '.join(asked)} "
                                      "not implemented")
    return flags


def repetition_penalty(penalty: float):
    """HF RepetitionPenaltyLogitsProcessor over the GENERATED tokens (the reference's generate() passes inputs_embeds, so HF's
    input_ids start empty): the logit of every token already emitted is divided by ``penalty`` if positive, multiplied if negative."""
    if penalty <= 0:
        raise ValueError("repetition_penalty must be a strictly positive float")

    def proc(hist: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
        if hist.shape[1] == 0:
            return logits
        sc = logits.gather(1, hist)
        sc = torch.where(sc < 0, sc * penalty, sc / penalty)
        return logits.scatter(1, hist, sc)
    return proc


def no_repeat_ngram(n: int):
    """HF NoRepeatNGramLogitsProcessor: a token that would complete an n-gram already present in the generated tokens gets -inf."""
    if n <= 0:
        raise ValueError("no_repeat_ngram_size must be a strictly positive integer")

    def proc(hist: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
        cur = hist.shape[1]
        if cur + 1 < n:
            return logits
        rows = hist.tolist()          # host glue of generate(): a few dozen tokens per sequence
        logits = logits.clone()
        for b, seq in enumerate(rows):
            prefix = tuple(seq[cur + 1 - n:cur])
            banned = [seq[i + n - 1] for i in range(cur - n + 1) if tuple(seq[i:i + n - 1]) == prefix]
            if banned:
                logits[b, banned] = float("-inf")
        return logits
    return proc


def sample(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, generator=None) -> torch.Tensor:
    """One multinomial draw per row after HF's logits warpers in HF's order (TemperatureLogitsWarper, TopKLogitsWarper,
    TopPLogitsWarper with min_tokens_to_keep = 1; transformers/generation/logits_process.py).  Host-side glue of generate():
    a handful of torch ops on [B, vocab], not part of the scoring hot path."""
    return torch.multinomial(warp(logits, temperature, top_k, top_p).softmax(-1), 1, generator=generator).squeeze(1)


def warp(logits: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """HF's three logits warpers in HF's order (pinned against transformers' own classes in tests/test_host.py)."""
    x = logits / temperature if temperature != 1.0 else logits
    if top_k > 0:
        kth = torch.topk(x, min(top_k, x.shape[-1]))[0][..., -1, None]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        srt, idx = torch.sort(x, descending=False)
        remove = srt.softmax(-1).cumsum(-1) <= (1.0 - top_p)
        remove[..., -1:] = False
        x = x.masked_fill(remove.scatter(1, idx, remove), float("-inf"))
    return x
