"""Host-side input building of the eval drivers: frame sampling and prompt -> ids -> label mask.

Deterministic integer / string code, restated from the reference and pinned to fixtures recorded from the reference's own
functions (tests/golden/make_host_golden.py -> tests/golden/host_inputs.pt):

* ``get_index``        stage2_eval.py:429-441   segment-centre frame indices of ``load_video``
* ``video_prompt``     stage2_eval.py:465-481   "<video>\\n" -> "Frame1: <image>\\n...FrameT: <image>\\nMotion Feature: <image>"
* ``build_inputs``     stage2_eval.py:488-498 + internvl/train/dataset.py:595-682 (``preprocess_internlm``): template join,
                       <image> expansion with ``num_image_tokens = [256] * T + [1]``, tokenisation, labels = the assistant's
                       answer tokens + the closing <|im_end|>, everything else -100.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .conversation import get_conv_template

IGNORE_TOKEN_ID = -100          # transformers LabelSmoother.ignore_index (dataset.py:3,34)
IMG_START_TOKEN, IMG_END_TOKEN, IMG_CONTEXT_TOKEN = "<img>", "</img>", "<IMG_CONTEXT>"     # internvl/train/constants.py:1-3


def get_index(bound: Optional[Tuple[float, float]], fps: float, max_frame: int, first_idx: int = 0, num_segments: int = 8) -> List[int]:
    """stage2_eval.py:429-441: centres of ``num_segments`` equal segments of [start, end] (numpy's round = half to even,
    which Python's ``round`` shares; ``int()`` truncates)."""
    start, end = (bound[0], bound[1]) if bound else (-100000, 100000)
    start_idx = max(first_idx, round(start * fps))
    end_idx = min(round(end * fps), max_frame)
    seg = float(end_idx - start_idx) / num_segments
    return [int(start_idx + (seg / 2) + round(seg * i)) for i in range(num_segments)]


def video_prompt(question: str, n_frames: int) -> str:
    """stage2_eval.py:465-481: the user turn of a video sample."""
    if "<video>" not in question:
        question = "<video>\n" + question
    tokens = "\n".join(f"Frame{i + 1}: <image>" for i in range(n_frames)) + "\nMotion Feature: <image>"
    return question.replace("<video>\n", tokens)


def build_inputs(tokenizer, question: str, answer: str, n_frames: int, num_image_token: int = 256,
                 template: str = "internlm2-chat", system_message: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """One stage-2 eval sample: ``input_ids`` / ``labels`` / ``attention_mask`` [N] exactly as ``video_get_item`` +
    ``preprocess_internlm`` build them (un-padded: the eval scripts run with group_by_length, dataset.py:636)."""
    conv = get_conv_template(template)
    if system_message is not None:
        conv.system_message = system_message
    conv.append_message(conv.roles[0], video_prompt(question, n_frames).strip())
    conv.append_message(conv.roles[1], answer.strip())
    text = conv.get_prompt()
    counts = [num_image_token] * n_frames + [1]                     # the 9th placeholder is the motion token (stage2_eval.py:493-494)
    for n in counts:
        text = text.replace("<image>", f"{IMG_START_TOKEN}{IMG_CONTEXT_TOKEN * n}{IMG_END_TOKEN}", 1)
    ids = tokenizer(text, return_tensors="pt", padding=False, max_length=tokenizer.model_max_length, truncation=True).input_ids[0]
    labels = ids.clone()
    # dataset.py:643-666: <s> and everything up to and including the assistant role string are ignored; the answer and its
    # <|im_end|> are kept; lengths are measured by re-tokenising the pieces (minus the <s> each call prepends)
    parts = text.split(conv.roles[1])
    cur = 1
    labels[:cur] = IGNORE_TOKEN_ID
    n0 = len(tokenizer(parts[0] + conv.roles[1]).input_ids) - 1
    labels[cur:cur + n0] = IGNORE_TOKEN_ID
    cur += n0
    for mid in parts[1:-1]:                                            # earlier assistant turns of a multi-turn sample
        p1, p2 = mid.split(conv.roles[0])
        cur += len(tokenizer(p1).input_ids) - 1
        n = len(tokenizer(conv.roles[0] + p2 + conv.roles[1]).input_ids) - 1
        labels[cur:cur + n] = IGNORE_TOKEN_ID
        cur += n
    cur += len(tokenizer(parts[-1]).input_ids) - 1
    labels[cur:] = IGNORE_TOKEN_ID
    if cur < tokenizer.model_max_length and cur != int(ids.ne(tokenizer.pad_token_id).sum()):
        labels[:] = IGNORE_TOKEN_ID                                    # the reference's "tokenization mismatch" fallback (:671-675)
    return {"input_ids": ids, "labels": labels, "attention_mask": ids.ne(tokenizer.pad_token_id)}


def batch_inputs(samples: Sequence[Dict[str, torch.Tensor]], pad_token_id: int = 2) -> Dict[str, torch.Tensor]:
    """Right-pad several samples to one [B, N] batch the way the reference's collator does (internvl/patch/pad_data_collator.py:
    ids with the pad id, labels with -100); the scorer strips the padding again (packed layout)."""
    n = max(int(s["input_ids"].numel()) for s in samples)
    ids = torch.full((len(samples), n), pad_token_id, dtype=torch.long)
    labels = torch.full((len(samples), n), IGNORE_TOKEN_ID, dtype=torch.long)
    mask = torch.zeros((len(samples), n), dtype=torch.bool)
    for i, s in enumerate(samples):
        k = int(s["input_ids"].numel())
        ids[i, :k], labels[i, :k], mask[i, :k] = s["input_ids"], s["labels"], True
    return {"input_ids": ids, "labels": labels, "attention_mask": mask}


def level_token_ids(tokenizer, words: Sequence[str] = ("bad", "poor", "fair", "good", "excellent"),
                    template: str = "The quality of the video is {}.") -> List[int]:
    """The candidate token ids of the quality levels for ``forward(candidate_ids=...)`` / ``generate(candidate_ids=...)``: every word is put
    into the answer ``template`` and tokenised IN CONTEXT (a SentencePiece vocabulary tokenises a word differently behind a space); the id
    returned for a word is its token at the first position where the candidates' tokenisations differ - the token whose distribution
    tells the levels apart.  Raises ValueError when two words share that token (multi-token words with a common first piece: score the
    candidate answers with ``forward_shared_prefix`` instead, README) or when the template has no ``{}``."""
    if "{}" not in template:
        raise ValueError("level_token_ids: the template needs a {} for the level word")
    if len(words) < 1:
        raise ValueError("level_token_ids: no level words")
    rows = [list(tokenizer(template.format(w)).input_ids) for w in words]
    n = min(len(r) for r in rows)
    pos = next((i for i in range(n) if any(r[i] != rows[0][i] for r in rows)), None)
    if pos is None:
        if len(words) > 1:
            raise ValueError(f"level_token_ids: the tokenisations of {list(words)} do not differ within their first {n} tokens")
        bare = list(tokenizer(template.format("")).input_ids)      # one word: the first token the word itself brings in
        pos = next((i for i in range(min(n, len(bare))) if rows[0][i] != bare[i]), None)
        if pos is None:
            raise ValueError(f"level_token_ids: {words[0]!r} adds no token of its own to the template")
    ids = [int(r[pos]) for r in rows]
    for i, a in enumerate(ids):
        for j in range(i):
            if ids[j] == a:
                raise ValueError(f"level_token_ids: {words[j]!r} and {words[i]!r} share their first distinguishing token {a}; score the whole "
                                 "candidate answers instead (forward_shared_prefix)")
    return ids


N_TEXT_SEGMENTS = 4             # bins behind the F frame bins: motion token | first token (the sink) | text up to the last visual token | text after it


def _visual_layout(name: str, slot, cu: Sequence[int], n_frames, tokens_per_frame: int):
    """What ``attention_segments`` and ``visual_token_positions`` share: the validated slot map -> (F, [(lo, hi, mask of the clip's visual
    tokens, mask of its motion token, their number)] per clip).  ``name`` heads the messages."""
    slot = torch.as_tensor(slot).to(torch.long).flatten()
    cu = [int(v) for v in cu]
    B = len(cu) - 1
    if B < 1 or cu[0] != 0 or cu[-1] != slot.numel() or any(cu[b + 1] <= cu[b] for b in range(B)):
        raise ValueError(f"{name}: cu {cu} does not divide the {slot.numel()} packed tokens into non-empty clips")
    if tokens_per_frame < 1:
        raise ValueError(f"{name}: tokens_per_frame must be positive")
    per_clip = [int(n_frames)] * B if isinstance(n_frames, int) else [int(v) for v in n_frames]
    if len(per_clip) != B or min(per_clip) < 0:
        raise ValueError(f"{name}: n_frames {n_frames!r} is neither an int nor one count per clip ({B} clips)")
    exact = not isinstance(n_frames, int)
    F = max(per_clip)
    n_vis = int((slot >= 0).sum()) - B                  # every clip carries exactly one motion token: the B largest slots
    if n_vis < 0 or sorted(slot[slot >= 0].tolist()) != list(range(n_vis + B)):
        raise ValueError(f"{name}: the slots must be 0 .. n_vis - 1 (visual tokens) and n_vis + b (the motion token of clip b), each once")
    is_motion = slot >= n_vis
    clips = []
    for b in range(B):
        lo, hi = cu[b], cu[b + 1]
        vis = ((slot[lo:hi] >= 0) & ~is_motion[lo:hi])
        n_v = int(vis.sum())
        if n_v % tokens_per_frame or n_v > per_clip[b] * tokens_per_frame or (exact and n_v != per_clip[b] * tokens_per_frame):
            raise ValueError(f"{name}: clip {b} holds {n_v} visual tokens, expected {'' if exact else 'up to '}{per_clip[b]} frames of {tokens_per_frame}")
        clips.append((lo, hi, vis, is_motion[lo:hi], n_v))
    return F, clips


def attention_segments(slot, cu: Sequence[int], n_frames, tokens_per_frame: int) -> torch.Tensor:
    """The key-segment table of ``forward(return_score_attention=True)``: one int32 id per PACKED token (host, no GPU), so that the
    score row's attention mass can be read per frame.  ``slot`` is the pass's slot map (int per packed token: -1 a text token, 0 ..
    n_vis - 1 a visual token in frame order, n_vis + b the motion token of clip b), ``cu`` the clips' row offsets [B + 1].  With F frame
    bins the ids are

    * ``f``      the visual tokens of the clip's frame f (its visual tokens in order, ``tokens_per_frame`` each),
    * ``F``      the motion token,
    * ``F + 1``  the first token of the clip - the BOS sink gets a bin of its own, because it usually takes most of the mass,
    * ``F + 2``  every other text token in front of the clip's last visual token (system prompt, "Frame i:" separators),
    * ``F + 3``  the text behind it (question and answer).

    ``n_frames``: an int F - every clip may hold up to F frames - or one count per clip (ragged clips in one packed batch: F is the
    largest, a shorter clip leaves its later frame bins empty).  Users may build another table and pass it as ``attention_segments=``."""
    F, clips = _visual_layout("attention_segments", slot, cu, n_frames, tokens_per_frame)
    seg = torch.empty(clips[-1][1], dtype=torch.int32)
    for lo, hi, vis, motion, n_v in clips:
        last_vis = int(vis.nonzero().max()) if n_v else -1
        part = torch.full((hi - lo,), F + 3, dtype=torch.int32)
        part[:max(last_vis, 0)] = F + 2
        part[0] = F + 1
        part[vis] = (torch.arange(n_v) // tokens_per_frame).to(torch.int32)
        part[motion] = F
        seg[lo:hi] = part
    return seg


def patch_drop_words(patch_drop) -> torch.Tensor:
    """The patch mask of ``vit_tokens(patch_drop=...)`` in the attention kernel's layout (host only): bool [F, G, G] -> int64 [F, ceil((G * G + 1) /
    64)] in ``key_drop_words``' word layout, one row per frame.  Key 0 of a frame is its cls token, which the mask cannot address: bit 0 of word 0
    is always clear, so no row is ever without a visible key.  Key ``1 + G * y + x`` is patch (y, x)."""
    pd = torch.as_tensor(patch_drop)
    if pd.dim() != 3 or pd.shape[1] != pd.shape[2] or pd.dtype != torch.bool or pd.shape[0] < 1 or pd.shape[1] < 1:
        raise ValueError(f"patch_drop_words: patch_drop must be a bool tensor [F, G, G] with F, G >= 1, got {pd.dtype} {tuple(pd.shape)}")
    n_f, G, _ = pd.shape
    S = G * G + 1
    keys = torch.cat([torch.zeros(n_f, 1, dtype=torch.bool), pd.to("cpu").reshape(n_f, G * G)], 1)      # [F, S]: cls in front, never dropped
    return key_drop_words(keys, [f * S for f in range(n_f + 1)])


def key_drop_words(key_drop, cu: Sequence[int], row_of=None, n_words: Optional[int] = None) -> torch.Tensor:
    """The key-drop mask of ``forward(key_drop=...)`` in the attention kernel's layout (host only): int64 [B, W], bit ``j & 63`` of word
    ``[b, j >> 6]`` set = token j of clip b (its position inside the PACKED clip, 0 = its first token) is dropped; bits at and past a clip's
    length are clear.  One word is one 64-key tile.  ``key_drop``: bool / integer [B, N] laid out like ``input_ids``; ``cu``: the clips' packed
    row offsets [B + 1]; ``row_of`` [B, N]: the packed row of every [b, p], negative where the pass does not run the token (padding: ignored) -
    default: clip b's tokens are its first ``cu[b + 1] - cu[b]`` columns (right-padded inputs).  W = ``n_words`` or ceil(longest clip / 64).
    (int64 because torch has no uint64 arithmetic: bit 63 is the sign bit, the device reads the same 64 bits.)"""
    import numpy as np
    kd = torch.as_tensor(key_drop)
    if kd.dim() != 2 or kd.is_floating_point():
        raise ValueError("key_drop_words: key_drop must be a bool or integer tensor [B, N]")
    kd = kd.to("cpu").bool()
    cu = [int(v) for v in cu]
    B, N = kd.shape
    if len(cu) != B + 1 or cu[0] != 0 or any(cu[b + 1] <= cu[b] for b in range(B)):
        raise ValueError(f"key_drop_words: cu {cu} does not describe {B} non-empty clips")
    lens = [cu[b + 1] - cu[b] for b in range(B)]
    W = -(-max(lens) // 64)
    if n_words is not None:
        if int(n_words) < W:
            raise ValueError(f"key_drop_words: n_words = {n_words} is below the {W} words of the longest clip ({max(lens)} tokens)")
        W = int(n_words)
    if row_of is None:
        if max(lens) > N:
            raise ValueError(f"key_drop_words: a clip of {max(lens)} tokens does not fit the {N} columns of key_drop")
        j = torch.arange(N).expand(B, N).clone()
        j[j >= torch.tensor(lens)[:, None]] = -1
    else:
        row_of = torch.as_tensor(row_of).to("cpu").long()
        if tuple(row_of.shape) != (B, N):
            raise ValueError(f"key_drop_words: row_of {tuple(row_of.shape)} is not laid out like key_drop {(B, N)}")
        j = torch.where(row_of >= 0, row_of - torch.tensor(cu[:-1])[:, None], torch.full_like(row_of, -1))
        if bool((j >= torch.tensor(lens)[:, None]).any()) or bool(((row_of >= 0) & (j < 0)).any()):
            raise ValueError("key_drop_words: row_of points outside its clip")
    words = np.zeros((B, W), dtype=np.uint64)
    b_idx, p_idx = (kd & (j >= 0)).nonzero(as_tuple=True)
    jj = j[b_idx, p_idx].numpy().astype(np.uint64)
    np.bitwise_or.at(words, (b_idx.numpy(), (jj >> np.uint64(6)).astype(np.int64)), np.uint64(1) << (jj & np.uint64(63)))
    return torch.from_numpy(words.view(np.int64))


def visual_token_positions(slot, cu: Sequence[int], n_frames, tokens_per_frame: int) -> torch.Tensor:
    """Where every visual token of every frame sits INSIDE its own clip: long [B, F, tokens_per_frame], entry [b, f, t] = the position (0 =
    the clip's first token) of token t of clip b's frame f - the column of ``forward(return_token_attention=True)``'s
    ``score_attention_tokens[b]`` that holds its mass - or -1 where a ragged clip has no frame f.  Built from the slot map
    ``attention_segments`` reads, with its arguments and its validation: position [b, f, t] carries segment id f there.
    ``eval_utils.frame_heatmaps`` folds the dense attention with it."""
    F, clips = _visual_layout("visual_token_positions", slot, cu, n_frames, tokens_per_frame)
    pos = torch.full((len(clips), F * tokens_per_frame), -1, dtype=torch.long)
    for b, (lo, hi, vis, motion, n_v) in enumerate(clips):
        pos[b, :n_v] = vis.nonzero().flatten()
    return pos.view(len(clips), F, tokens_per_frame)
