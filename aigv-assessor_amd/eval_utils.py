"""Host-side result handling of the eval drivers: answer-token slice, quality-level parse, CSV and
correlation metrics — deterministic string/array code, restated from internvl/train/internvl/eval/stage2_eval.py."""
from __future__ import annotations

import csv
from typing import Optional, Sequence

LEVELS = (("bad", 1), ("poor", 2), ("fair", 3), ("good", 4), ("excellent", 5))
CSV_COLUMNS = ("video_name", "answer", "output", "mos", "pred_score", "level")   # stage2_eval.py:654


def answer_ids(labels_row, logit_row, im_end_id: int = 92542):
    """stage2_eval.py:940-941: answer tokens = labels not in {-100, <|im_end|>}; predictions = logit[-len-1:-1]."""
    n = sum(1 for x in labels_row.tolist() if x != -100 and x != im_end_id)
    return logit_row[-n - 1:-1]


def parse_level(text: str) -> int:
    """stage2_eval.py:956-967: substring tests in the order bad, poor, fair, good, excellent -> 1..5, else 0."""
    for word, level in LEVELS:
        if word in text:
            return level
    return 0


def save_and_evaluate(rows: Sequence[Sequence], output_file: Optional[str] = None) -> dict:
    """stage2_eval.py:652-688: CSV dump, substring accuracy (output in answer), SRCC/PLCC/KRCC of level and of
    pred_score against mos."""
    from scipy.stats import kendalltau, pearsonr, spearmanr
    if output_file:
        with open(output_file, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(CSV_COLUMNS)
            w.writerows(rows)
    total = len(rows)
    acc = sum(1 for r in rows if r[2] in r[1]) / total if total else 0.0
    mos = [float(r[3]) for r in rows]
    out = {"acc": acc}
    for name, col in (("level", 5), ("pred_score", 4)):
        vals = [float(r[col]) for r in rows]
        out[f"{name}_srcc"] = spearmanr(mos, vals)[0]
        out[f"{name}_plcc"] = pearsonr(mos, vals)[0]
        out[f"{name}_krcc"] = kendalltau(mos, vals)[0]
    return out


def lookahead(items, model, frames, n_clips: int = 1):
    """Iterate an eval loop one item ahead: yields ``(item, ahead)`` where ``ahead`` is ``model.prefetch(...)`` of THAT item's frames, started
    while the previous item was still being scored - the next clip's frame ingest, InternViT pass and SlowFast branch run beside the
    current clip's InternLM2 pass.  ``frames(item)`` returns the item's frames: uint8 [F, H, W, 3] (ingested on the GPU) or normalised
    [F, 3, S, S] ``pixel_values``.  The reference's loop (stage2_eval.py:908-941) changes by two lines:

        for item, ahead in eval_utils.lookahead(dataloader, model, frames=lambda it: it["pixel_values"][0]):
            output = model(pixel_values=ahead, input_ids=..., ...)            # instead of pixel_values=item["pixel_values"][0].to(...).cuda()

    Scores and level tokens are those of the plain loop, bit for bit."""
    import torch

    def start(item):
        f = frames(item)
        return model.prefetch(frames_u8=f, n_clips=n_clips) if f.dtype == torch.uint8 else model.prefetch(pixel_values=f, n_clips=n_clips)
    it = iter(items)
    try:
        cur = next(it)
    except StopIteration:
        return
    ahead = start(cur)
    for nxt in it:
        nxt_ahead = start(nxt)          # enqueued BEFORE the caller scores `cur`: the two then run side by side
        yield cur, ahead
        cur, ahead = nxt, nxt_ahead
    yield cur, ahead


# ---- the reference's eval loop at batch k, on N ranks (stage2_eval.py:908-941) -------------------------------------------------------
def shard(items, rank: int, world: int):
    """This rank's share of an eval set: items rank, rank + world, rank + 2 world, ...  The reference launches ``torchrun
    --nproc_per_node=${GPUS}`` (shell/eval/stage2_eval.sh:20-25) with a plain ``DataLoader(train_dataset, batch_size=1)`` and no sampler
    (stage2_eval.py:908-911): with GPUS > 1 every rank scores the WHOLE set.  A map-style dataset (``__len__`` + ``__getitem__``) comes
    back as a ``torch.utils.data.Subset`` - so the other ranks' videos are never decoded here -, any other iterable as a strided
    iterator.  ``gather_rows`` puts the per-rank result rows back into the set's order."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside 0..{world - 1}")
    if world == 1:
        return items
    if hasattr(items, "__len__") and hasattr(items, "__getitem__"):
        from torch.utils.data import Subset
        return Subset(items, range(rank, len(items), world))
    import itertools
    return itertools.islice(items, rank, None, world)


def gather_rows(rows: Sequence, group=None) -> list:
    """The result rows of every rank (each the rows of its ``shard``, in its own order) -> the rows of the whole set in the set's order, on
    every rank.  One ``all_gather_object`` of small host tuples at the END of the loop: nothing crosses ranks while clips are scored."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return list(rows)
    world = dist.get_world_size(group)
    parts = [None] * world
    dist.all_gather_object(parts, list(rows), group=group)
    return _interleave(parts)


def _interleave(parts: Sequence[Sequence]) -> list:
    """The inverse of ``shard``: rank r holds items r, r + world, r + 2 world, ... of the set as its 0th, 1st, 2nd, ... row."""
    out = []
    for i in range(max((len(p) for p in parts), default=0)):
        for p in parts:                                   # item j of the set went to rank j % world as its (j // world)-th
            if i < len(p):
                out.append(p[i])
    return out


def _frames_of(item):
    pv = item["pixel_values"]
    return pv[0] if pv.dim() == 5 else pv                  # DataLoader(batch_size=1) adds the leading 1 (stage2_eval.py:932 takes [0])


def expected_level(cand_logprob, weights=(1, 2, 3, 4, 5)):
    """The mean quality level of the closed-set distribution over the level words: ``(softmax(cand_logprob, -1) * weights).sum(-1)`` for
    ``cand_logprob`` [..., C] (``forward(candidate_ids=...)``'s ``cand_logprob`` / ``generate``'s ``cand_logprobs``, the candidates ordered worst to
    best) - in [weights[0], weights[-1]], NaN where the row is NaN (no answer token there)."""
    import torch
    w = torch.as_tensor(weights, dtype=cand_logprob.dtype, device=cand_logprob.device)
    return (torch.softmax(cand_logprob, -1) * w).sum(-1)


def frame_saliency(att, layers=None):
    """Which frames the score row reads: ``att`` is ``forward(return_score_attention=True)``'s ``score_attention`` [B, L, n_heads, F + 4]
    (bins: F frames, then motion | first token | text before | text after: ``prompts.attention_segments``); returns [B, F] - the mass on
    the frame bins, averaged over the heads and over ``layers`` (an index list; None: all layers), renormalised over the frames so that a
    clip's row sums to 1 (NaN where the row puts no mass on any frame)."""
    import torch
    from .prompts import N_TEXT_SEGMENTS
    if att.dim() != 4 or att.shape[-1] <= N_TEXT_SEGMENTS:
        raise ValueError(f"frame_saliency: expected [B, L, n_heads, F + {N_TEXT_SEGMENTS}] with F >= 1, got {tuple(att.shape)}")
    if layers is not None:
        att = att.index_select(1, torch.as_tensor(list(layers), dtype=torch.long, device=att.device))
    mass = att[..., :att.shape[-1] - N_TEXT_SEGMENTS].double().mean(dim=(1, 2))
    return (mass / mass.sum(-1, keepdim=True)).to(att.dtype)


def frame_heatmaps(tok_att, positions, layers=None):
    """Where INSIDE each frame the score row reads: ``tok_att`` is ``forward(return_token_attention=True)``'s ``score_attention_tokens``
    [B, L, n_heads, N] (one softmax value per key), ``positions`` is ``prompts.visual_token_positions`` [B, F, tokens_per_frame] (-1: a
    ragged clip has no such frame); returns [B, F, g, g] with g * g = tokens_per_frame (ValueError if that is no perfect square) - the
    mass on every visual token, averaged over the heads and over ``layers`` (an index list; None: all layers) in float64 and renormalised
    over ALL of the clip's visual tokens: ``heat.sum((2, 3))`` is ``frame_saliency(score_attention, layers)``, a clip's maps sum to 1 (a
    frame the clip does not have stays 0; NaN where the row puts no mass on any frame).

    Geometry: token t of a frame is cell ``divmod(t, g)`` = (r, c), row-major - pixel-shuffle v2's order (modeling_internvl_chat.py:492-506):
    cell (r, c) is the concatenation of the ViT patches of patch rows 2r, 2r + 1 x patch columns 2c, 2c + 1.  For a 448 x 448 frame (14-pixel
    patches, a 32 x 32 patch grid, g = 16) that is the pixel rectangle rows 28r .. 28r + 27 x columns 28c .. 28c + 27: ``heat[b, f]`` lies
    over the frame as an image does, first axis down, second axis right."""
    import math
    import torch
    if tok_att.dim() != 4 or positions.dim() != 3 or positions.shape[0] != tok_att.shape[0]:
        raise ValueError(f"frame_heatmaps: expected [B, L, n_heads, N] and [B, F, tokens_per_frame], got {tuple(tok_att.shape)} and {tuple(positions.shape)}")
    B, F, T = positions.shape
    g = math.isqrt(T)
    if g * g != T:
        raise ValueError(f"frame_heatmaps: tokens_per_frame = {T} is not a perfect square")
    if int(positions.max()) >= tok_att.shape[-1] or int(positions.min()) < -1:
        raise ValueError(f"frame_heatmaps: positions outside -1 .. {tok_att.shape[-1] - 1}")
    if layers is not None:
        tok_att = tok_att.index_select(1, torch.as_tensor(list(layers), dtype=torch.long, device=tok_att.device))
    per_key = tok_att.double().mean(dim=(1, 2))                               # [B, N]
    idx = positions.to(per_key.device).view(B, F * T)
    mass = per_key.gather(1, idx.clamp_min(0)) * (idx >= 0)
    return (mass / mass.sum(-1, keepdim=True)).view(B, F, g, g).to(tok_att.dtype)


def flow_segments(model, input_ids, attention_mask=None, image_flags=None):
    """The table to pass as ``forward(attention_segments=..., return_segment_attention=True)`` for the question WHO READS WHOM (host only, no
    GPU work): long [B, N] laid out like ``input_ids`` - the default bins (``prompts.attention_segments``: frame 0 .. F - 1 | motion token F |
    first token F + 1 | text up to the last visual token F + 2 | text after it F + 3) with the SCORE ROW as a bin of its own, F + 4; S = F + 5.
    -1 on the padding.  Built from ``model.unit_masks`` and ``model.segment_masks``; a stage-1 model has no score row and leaves bin F + 4 empty
    (its rows of ``segment_attention`` are NaN)."""
    import torch
    units = model.unit_masks(input_ids, attention_mask, image_flags)          # [B, F + 1, N]: the frames, the motion token
    groups = model.segment_masks(input_ids, attention_mask, image_flags)
    F = units.shape[1] - 1
    table = torch.full(tuple(units.shape[::2]), -1, dtype=torch.long)
    for name, s in (("first", F + 1), ("text_before", F + 2), ("text_after", F + 3)):
        table[groups[name]] = s
    for u in range(F + 1):
        table[units[:, u]] = u
    table[groups["score_row"]] = F + 4
    return table


def _pick(t, dim, index, what):
    import torch
    if index is None:
        return t
    idx = torch.as_tensor(list(index), dtype=torch.long, device=t.device)
    if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= t.shape[dim]:
        raise ValueError(f"{what}: an index list inside 0..{t.shape[dim] - 1} with at least one entry, got {list(index)}")
    return t.index_select(dim, idx)


def segment_flow(seg_att, layers=None, heads=None):
    """Who reads whom, in one matrix per clip: ``seg_att`` is ``forward(return_segment_attention=True)``'s ``segment_attention`` [B, L, n_heads,
    S, S]; returns [B, S, S] - entry [a, c], the mass the rows of segment a put on the keys of segment c, averaged in float64 over ``layers`` and
    ``heads`` (index lists; None: all).  The row of a segment the clip does not have stays NaN."""
    if seg_att.dim() != 5 or seg_att.shape[-1] != seg_att.shape[-2]:
        raise ValueError(f"segment_flow: expected [B, L, n_heads, S, S], got {tuple(seg_att.shape)}")
    t = _pick(_pick(seg_att, 1, layers, "segment_flow: layers"), 2, heads, "segment_flow: heads")
    return t.double().mean(dim=(1, 2)).to(seg_att.dtype)


def attention_rollout(seg_att, alpha: float = 0.5, layers=None):
    """Attention rollout over the segments (Abnar & Zuidema 2020): ``seg_att`` [B, L, n_heads, S, S] as above; returns [B, S, S] - the product
    over depth, the deepest layer leftmost, of ``alpha I + (1 - alpha) A_l`` with A_l the head mean of layer l (``alpha``: the residual
    connection's share, 0 <= alpha <= 1); entry [a, c] is how much of segment c's INPUT reaches the rows of segment a at the top through
    attention and residual paths.  The row of a segment the clip does not have (NaN in ``seg_att``) is the identity's in every layer, so it stays
    out of every other row.  ``layers``: an index list (multiplied in the order given, the last one leftmost); None: all layers.  float64
    inside; alpha = 1 gives I exactly, alpha = 0 with permutation matrices gives their product exactly."""
    import torch
    if seg_att.dim() != 5 or seg_att.shape[-1] != seg_att.shape[-2]:
        raise ValueError(f"attention_rollout: expected [B, L, n_heads, S, S], got {tuple(seg_att.shape)}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"attention_rollout: alpha = {alpha!r} outside 0..1")
    a = _pick(seg_att, 1, layers, "attention_rollout: layers").double().mean(2)              # [B, L', S, S]
    eye = torch.eye(a.shape[-1], dtype=torch.float64, device=a.device)
    empty = torch.isnan(a).any(-1, keepdim=True)
    step = torch.where(empty, eye, float(alpha) * eye + (1.0 - float(alpha)) * torch.nan_to_num(a))
    out = eye.expand(a.shape[0], -1, -1)
    for l in range(a.shape[1]):
        out = step[:, l] @ out
    return out.to(seg_att.dtype)


def vit_rollout(att, alpha: float = 0.5, layers=None):
    """Attention rollout INSIDE the vision tower (Abnar & Zuidema 2020), per frame: ``att`` is ``model.vit_attention(pixel_values)``'s head-mean
    ``vit_attention`` [F, L', S, S] (S = patches + 1, row / column 0 the cls token); returns [F, S, S] - the product over depth, the deepest layer
    leftmost, of ``alpha I + (1 - alpha) A_l`` (``alpha``: the residual connection's share, 0 <= alpha <= 1); entry [i, j] is how much of patch
    row j's INPUT reaches row i at the top of the tower through attention and residual paths.  ``layers``: an index list (multiplied in the
    order given, the last one leftmost); None: all layers of ``att``.  float64 inside, one frame at a time (a frame's product is S x S doubles:
    8.4 MB at S = 1025); alpha = 1 gives I exactly, alpha = 0 with permutation matrices gives their product exactly."""
    import torch
    if att.dim() != 4 or att.shape[-1] != att.shape[-2]:
        raise ValueError(f"vit_rollout: expected the head-mean maps [F, L, S, S], got {tuple(att.shape)}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"vit_rollout: alpha = {alpha!r} outside 0..1")
    att = _pick(att, 1, layers, "vit_rollout: layers")
    eye = torch.eye(att.shape[-1], dtype=torch.float64, device=att.device)
    out = torch.empty(att.shape[0], att.shape[-1], att.shape[-1], dtype=att.dtype, device=att.device)
    for f in range(att.shape[0]):
        roll = eye
        for l in range(att.shape[1]):
            roll = (float(alpha) * eye + (1.0 - float(alpha)) * att[f, l].double()) @ roll
        out[f] = roll.to(att.dtype)
    return out


def _cells_to_patches(t):
    """The ONE statement of which ViT patches a visual token's cell holds (``frame_heatmaps``' geometry paragraph): [..., g, g] over cells ->
    [..., 2g, 2g] over patches, cell (r, c)'s value on its patches (y, x) in {2r, 2r + 1} x {2c, 2c + 1}.  ``pixel_heatmaps`` spreads heat with
    it, ``cell_patches`` marks patches with it."""
    return t.repeat_interleave(2, -2).repeat_interleave(2, -1)


def cell_patches(cells):
    """Bool [..., g, g] over visual tokens (cells, ``frame_heatmaps``' layout) -> bool [..., 2g, 2g] over ViT patches: the four patches of every
    marked cell, by the index ``pixel_heatmaps`` spreads a cell's heat with - what ``vit_tokens(patch_drop=...)`` takes for a region picked on a
    token heat map."""
    import torch
    cells = torch.as_tensor(cells)
    if cells.dtype != torch.bool or cells.dim() < 2 or cells.shape[-1] != cells.shape[-2]:
        raise ValueError(f"cell_patches: expected a bool tensor [..., g, g], got {cells.dtype} {tuple(cells.shape)}")
    return _cells_to_patches(cells)


def pixel_heatmaps(heat, rollout):
    """From visual tokens back to the pixels: ``heat`` is ``frame_heatmaps``' [B, F, g, g] (the score row's mass per visual token), ``rollout``
    is ``vit_rollout``'s [B * F, S, S] in clip-major frame order (frame f of clip b at index b * F + f), S = (2 g)^2 + 1; returns
    ``(pix [B, F, 2g, 2g], cls [B, F])`` in float64 - one cell per ViT patch (14 x 14 pixels of a 448 x 448 frame: ``pix[b, f]`` lies over the
    frame as an image does), and what lands on the cls token's input.

    A visual token is the CONCATENATION of the four ViT patches of its cell (``frame_heatmaps``' geometry paragraph), so nothing says how its
    heat divides among them.  The convention here is the EQUAL SPLIT: a quarter of cell (r, c)'s heat goes to each of the rollout rows
    1 + 2g * y + x of its patches (y, x) in {2r, 2r + 1} x {2c, 2c + 1}; a row passes its share on along its rollout row - ``pix`` collects
    the columns 1 .., patch (y, x) at column 1 + 2g * y + x, ``cls`` column 0.  Wherever the rollout's rows sum to 1,
    ``pix.sum((2, 3)) + cls == heat.sum((2, 3))`` up to float64 rounding.  An identity rollout gives each cell's heat / 4 on its four patches
    exactly; a permutation rollout moves those quarters exactly."""
    import torch
    if heat.dim() != 4 or heat.shape[-1] != heat.shape[-2] or rollout.dim() != 3 or rollout.shape[-1] != rollout.shape[-2]:
        raise ValueError(f"pixel_heatmaps: expected [B, F, g, g] and [B * F, S, S], got {tuple(heat.shape)} and {tuple(rollout.shape)}")
    B, F, g, _ = heat.shape
    n = 2 * g
    if rollout.shape[0] != B * F or rollout.shape[-1] != n * n + 1:
        raise ValueError(f"pixel_heatmaps: heat [B = {B}, F = {F}, g = {g}] needs rollout [{B * F}, {n * n + 1}, {n * n + 1}], got {tuple(rollout.shape)}")
    rows = _cells_to_patches(heat.double() / 4.0).reshape(B * F, 1, n * n)      # the weight of rollout row 1 + 2g y + x
    out = torch.empty(B * F, n * n + 1, dtype=torch.float64, device=heat.device)
    for i in range(B * F):                                                  # (a frame at a time: the float64 copy of one rollout matrix)
        out[i] = (rows[i] @ rollout[i, 1:].to(heat.device).double())[0]
    return out[:, 1:].reshape(B, F, n, n), out[:, 0].reshape(B, F)


def source_writes(model, out, direction=None, layers=None):
    """WHAT the score row takes from each source: ``out`` is the result dict of ``forward(return_score_values=True)`` (or one of
    ``forward_shared_prefix``'s), whose ``score_values`` [B, L, n_heads, S, D] holds, per layer and head, the value-weighted sum the row read from
    each of the S key segments.  Put through the layer's own ``language_model.model.layers.{l}.attention.wo.weight`` [H, n_heads D] that is the
    vector each (head, source) WRITES into the score row's residual stream.  ``layers``: an index list (None: all layers; L' of them).
    With ``direction`` ([H], or [B, H]: one per clip - a steering or good-minus-bad direction from ``lens_score_hidden`` / ``return_stream``):
    returns fp32 [B, L', n_heads, S], the scalar ``<direction, wo_l[:, hD:(h+1)D] @ score_values[b, l, h, s]>`` - computed as ``direction @ wo_l``
    viewed [n_heads, D] and dotted with the values; the [.., S, H] tensor is never formed.  Summed over heads and sources (plus the same form of
    ``score_values_rest``) it is the attention block's write along the direction, bias-free as ``wo`` is.
    Without ``direction``: returns fp32 [B, L', S], the L2 norm of ``sum_h wo_l[:, hD:(h+1)D] @ score_values[b, l, h, s]`` - the size of what each
    source writes at that layer (norm-based attention analysis: mass on a key whose value is tiny writes nothing).
    fp32 arithmetic on the values' device."""
    import torch
    val = out["score_values"] if isinstance(out, dict) else out
    if val.dim() != 5:
        raise ValueError(f"source_writes: expected score_values [B, L, n_heads, S, D], got {tuple(val.shape)}")
    B, L, nh, S, D = val.shape
    idx = list(range(L)) if layers is None else [int(l) for l in layers]
    if any(not 0 <= l < L for l in idx):
        raise ValueError(f"source_writes: layers outside 0..{L - 1}")
    params = dict(model.named_parameters())
    d = None
    if direction is not None:
        d = torch.as_tensor(direction).to(device=val.device, dtype=torch.float32)
        if d.dim() not in (1, 2) or (d.dim() == 2 and d.shape[0] != B):
            raise ValueError(f"source_writes: direction must be [H] or [B = {B}, H], got {tuple(d.shape)}")
        d = d.expand(B, -1) if d.dim() == 2 else d[None].expand(B, -1)
    res = []
    for l in idx:
        wo = params[f"language_model.model.layers.{l}.attention.wo.weight"].detach().to(device=val.device, dtype=torch.float32)      # [H, n_heads D]
        if tuple(wo.shape[1:]) != (nh * D,) or (d is not None and d.shape[1] != wo.shape[0]):
            raise ValueError(f"source_writes: wo of layer {l} is {tuple(wo.shape)}, the values have {nh} heads x {D}"
                             + ("" if d is None else f", the direction {d.shape[1]} elements"))
        v = val[:, l].to(torch.float32)                                          # [B, n_heads, S, D]
        if d is not None:
            res.append(torch.einsum("bhd,bhsd->bhs", (d @ wo).view(B, nh, D), v))
        else:
            res.append(torch.linalg.vector_norm(torch.einsum("bhsd,ohd->bso", v, wo.view(-1, nh, D)), dim=-1))
    return torch.stack(res, 1)


def frame_write_saliency(norms, layers=None):
    """Which frames the score row is WRITTEN from: ``norms`` is ``source_writes(model, out)`` [B, L, F + 4] (the norm form, default segments);
    returns [B, F] - the frame columns, averaged over ``layers`` (an index list; None: all layers) and renormalised over the frames so that a
    clip's row sums to 1 (NaN where no frame writes anything).  ``frame_saliency``'s counterpart: that one weighs frames by attention mass, this
    one by the size of what the mass carries."""
    import torch
    from .prompts import N_TEXT_SEGMENTS
    if norms.dim() != 3 or norms.shape[-1] <= N_TEXT_SEGMENTS:
        raise ValueError(f"frame_write_saliency: expected [B, L, F + {N_TEXT_SEGMENTS}] with F >= 1, got {tuple(norms.shape)}")
    if layers is not None:
        norms = norms.index_select(1, torch.as_tensor(list(layers), dtype=torch.long, device=norms.device))
    size = norms[..., :norms.shape[-1] - N_TEXT_SEGMENTS].double().mean(dim=1)
    return (size / size.sum(-1, keepdim=True)).to(norms.dtype)


def settling_depth(lens_score, tol: float):
    """AT WHICH DEPTH the score exists: ``lens_score`` is ``forward(return_depth_lens=True)``'s [B, L + 1] (the score head on the score row after
    d layers, column L the pass's own score); returns int64 [B] - the smallest depth d such that EVERY depth d' >= d has ``|lens_score[:, d'] -
    lens_score[:, L]| <= tol``, L where only the last depth qualifies.  A NaN never qualifies (a NaN final score: L).  Host-side arithmetic on
    whatever device the tensor lives on; ``tol`` >= 0."""
    import torch
    if lens_score.dim() != 2 or lens_score.shape[1] < 1:
        raise ValueError(f"settling_depth: expected [B, L + 1], got {tuple(lens_score.shape)}")
    if not tol >= 0:
        raise ValueError(f"settling_depth: tol = {tol!r} must be >= 0")
    s = lens_score.double()
    L = s.shape[1] - 1
    ok = (s - s[:, L:]).abs() <= tol                                   # (NaN compares False)
    ok[:, L] = True                                                    # the last depth stands for itself
    # the length of the run of qualifying depths that ends at L: every d' >= d qualifies iff no failure at or behind d
    settled = torch.flip(torch.cumprod(torch.flip(ok.long(), (1,)), 1), (1,))
    return (L + 1 - settled.sum(1)).to(torch.long)


# ---- what the sweeps below share -----------------------------------------------------------------------------------------------------
def _once_per_batch(model, pixel_values, readout_kwargs, **inputs):
    """InternViT and the SlowFast branch run ONCE for a sweep -> the keyword arguments every pass of it shares: ``inputs`` (``input_ids`` among
    them), ``visual_tokens``, ``motion_feature`` (the one in ``readout_kwargs``, else computed here) and the other ``readout_kwargs``."""
    readout_kwargs = dict(readout_kwargs)
    motion_feature = readout_kwargs.pop("motion_feature", None)
    if motion_feature is None:
        motion_feature = model.motion_feature(pixel_values, int(inputs["input_ids"].shape[0]))
    return dict(inputs, visual_tokens=model.vit_tokens(pixel_values), motion_feature=motion_feature, **readout_kwargs)


def _recipient(model, corrupt, B, readout_kwargs):
    """The ``corrupt`` dict of a donor / recipient sweep as the keyword arguments every pass of the recipient shares: its SlowFast feature and its
    InternViT tokens computed ONCE, no ``pixel_values``, ``readout_kwargs`` on top."""
    common = {k: v for k, v in corrupt.items() if k != "pixel_values"}
    if common.get("motion_feature") is None:
        common["motion_feature"] = model.motion_feature(corrupt["pixel_values"], B)
    common.update(visual_tokens=model.vit_tokens(corrupt["pixel_values"]), **readout_kwargs)
    return common


def _windows(where, L, width, stride):
    """The layer windows of a sweep: ``(lo, min(lo + width, L))`` for lo = 0, stride, 2 stride, ... < L; ``stride`` None: ``width``."""
    width = int(width)
    stride = width if stride is None else int(stride)
    if not 1 <= width <= L or stride < 1:
        raise ValueError(f"{where}: width = {width} outside 1..{L} or stride = {stride} below 1")
    return [(lo, min(lo + width, L)) for lo in range(0, L, stride)]


def _knocked(res, outs, B, shape, absent):
    """``score1`` / ``knocked`` [B, *shape] / ``delta`` of a knock-out sweep whose passes behind the base one are ``outs[1:]``.  ``absent``: None, or
    bool [B] or [B, shape[0]] - where the clip has nothing to knock out (no selected row; in ``flow_knockout``, per path, no key or no row): NaN."""
    import torch
    if "score1" in outs[0]:
        base = outs[0]["score1"].float()
        knocked = torch.stack([o["score1"].float() for o in outs[1:]], 1).view(B, *shape) if len(outs) > 1 else base.new_zeros(B, *shape)
        if absent is not None:
            knocked = knocked.masked_fill(absent.view(*absent.shape, *([1] * (1 + len(shape) - absent.dim()))).to(knocked.device), float("nan"))
        res.update(score1=base, knocked=knocked, delta=base.view(B, *([1] * len(shape))) - knocked)
    return res


def _restored(res, outs, B, shape):
    """``clean_score`` / ``corrupt_score`` / ``score`` [B, *shape] / ``restored`` of a donor / recipient sweep whose patched passes are ``outs[2:]``."""
    import torch
    if "score1" in outs[0]:
        clean_score, corrupt_score = outs[0]["score1"].float(), outs[1]["score1"].float()
        score = torch.stack([o["score1"].float() for o in outs[2:]], 1).view(B, *shape) if len(outs) > 2 else clean_score.new_zeros(B, *shape)
        res.update(score=score, clean_score=clean_score, corrupt_score=corrupt_score, restored=restored_fraction(score, clean_score, corrupt_score))
    return res


def frame_ablation(model, *, pixel_values, input_ids, attention_mask, image_flags, labels=None, motion_feature=None, **readout_kwargs):
    """WHAT IF a frame were not there: the batch scored once as it is and once per unit with that unit's tokens hidden from the LLM
    (``forward(key_drop=model.unit_masks(...)[:, u])``) - unit u < F is frame u's visual tokens, unit F the motion token.  Positions, the
    "FrameK:" text and every other token stay as they are, so a delta isolates the unit's content.  InternViT and the SlowFast branch run
    ONCE; their outputs are handed to every pass (``visual_tokens=``, ``motion_feature=``).  ``readout_kwargs`` go to every ``forward`` call.

    Returns a dict: ``outs`` - the F + 2 result dicts of ``forward``, base first, then unit 0 .. F; ``units`` - the masks, bool [B, F + 1, N];
    and for a stage-2 model ``score1`` [B] (the base scores, fp32), ``ablated`` [B, F + 1] (the score with the unit hidden; NaN where the
    clip lacks the frame) and ``delta`` = ``score1[:, None] - ablated``: positive where the unit raised the score."""
    import torch
    units = model.unit_masks(input_ids, attention_mask, image_flags, n_frames=int(pixel_values.shape[0]))      # host bool [B, F + 1, N]
    common = _once_per_batch(model, pixel_values, dict(readout_kwargs, motion_feature=motion_feature), input_ids=input_ids, attention_mask=attention_mask,
                             image_flags=image_flags, labels=labels)
    outs = [model.forward(**common)] + [model.forward(key_drop=units[:, u], **common) for u in range(units.shape[1])]
    res = {"outs": outs, "units": units}
    if "score1" in outs[0]:
        base = outs[0]["score1"].float()
        ablated = torch.stack([o["score1"].float() for o in outs[1:]], 1)
        absent = ~units.any(-1)                                             # [B, F + 1]: the clip has no such frame
        ablated = ablated.masked_fill(absent.to(ablated.device), float("nan"))
        res.update(score1=base, ablated=ablated, delta=base[:, None] - ablated)
    return res


def patch_occlusion(model, *, pixel_values, input_ids, attention_mask, image_flags, labels=None, cell=4, frames=None, hide_tokens=True, **readout_kwargs):
    """WHAT IF a region of a frame could not be read INSIDE the vision tower: occlusion sensitivity (Zeiler & Fergus 2014) without grey pixels.  Per
    clip, per frame and per block of ``cell`` x ``cell`` visual tokens the batch is scored with the block's ViT patches (``cell_patches``) hidden, as
    keys, from every row of their frame in every layer of the tower (``vit_tokens(patch_drop=...)``): pixels, positions, cls and every other patch
    stay.  The hidden patches' own rows still carry their content into the block's own tokens; with ``hide_tokens`` those tokens are hidden from the
    LLM as well (``forward(key_drop=...)``) and the delta is the region's whole contribution; without it the delta is what THE REST of the frame loses
    when it cannot read the region.  ``cell`` must divide the token grid T (T * T = tokens per frame); ``frames``: the frame indices to sweep
    (default: all F).  ``readout_kwargs`` (``motion_feature`` among them) go to every ``forward`` call.

    The sweep shares ``frame_ablation``'s structure: InternViT (unmasked) and the SlowFast branch run ONCE; per frame index one masked ViT batch
    holds, for every clip that has the frame, the frame repeated (T / cell)^2 + 1 times - an EMPTY mask first, the control, then one mask per
    block; a variant's tokens are spliced into the base tokens (``forward(visual_tokens=...)``); one LLM pass per (frame index, block) over all B
    clips, plus the control's.  ``delta`` is measured against the control, which went through the same ViT batch as the variants (InternViT is
    batch-invariant: tests/test_gpu_vit_attention.py, a frame alone across a chunk boundary), so a block whose mask is empty gives 0 exactly.
    ``control`` has ``score1``'s bits unless the lead-key tune knob is on (the masked attention kernel runs without it).

    Returns a dict: ``outs`` - the base result dict, then per swept frame index the control's and the blocks', row-major; ``blocks`` - bool
    [T / cell, T / cell, T, T], the cells of every block; and for a stage-2 model ``score1`` [B] (the base scores, fp32), ``control`` [B, F],
    ``occluded`` [B, F, T / cell, T / cell] (NaN where the clip lacks the frame or the frame was not swept) and ``delta`` = ``control[:, :, None,
    None] - occluded``: positive where the region raised the score."""
    import math
    import torch
    B, NF = int(input_ids.shape[0]), int(pixel_values.shape[0])
    T = math.isqrt(int(model.num_image_token))
    v = model.config.vision_config
    if T * T != model.num_image_token or 2 * T != model.config.image_size // v.patch_size:
        raise ValueError(f"patch_occlusion: {model.num_image_token} tokens per frame are no T x T grid of 2 x 2 patch cells")
    cell = int(cell)
    if cell < 1 or T % cell:
        raise ValueError(f"patch_occlusion: cell = {cell} does not divide the token grid {T}")
    nb = T // cell
    blocks = torch.zeros(nb, nb, T, T, dtype=torch.bool)
    for r in range(nb):
        for c in range(nb):
            blocks[r, c, r * cell:(r + 1) * cell, c * cell:(c + 1) * cell] = True
    units = model.unit_masks(input_ids, attention_mask, image_flags, n_frames=NF)[:, :-1]                      # host bool [B, F, N]: frame f's tokens
    F = int(units.shape[1])
    has = units.any(-1)                                                                                        # [B, F]
    sweep = list(range(F)) if frames is None else [int(f) for f in frames]
    if any(not 0 <= f < F for f in sweep) or len(set(sweep)) != len(sweep):
        raise ValueError(f"patch_occlusion: frames = {frames!r} are not distinct indices in 0..{F - 1}")
    flags = None if image_flags is None else image_flags.detach().to("cpu").reshape(-1)
    keep = torch.arange(NF) if flags is None else (flags == 1).nonzero().flatten()                             # the frames the clips' visual tokens come from, in order
    first = [0] + torch.cumsum(has.sum(1), 0).tolist()                                                         # clip b's frame f is keep[first[b] + f]
    common = _once_per_batch(model, pixel_values, readout_kwargs, input_ids=input_ids, attention_mask=attention_mask, image_flags=image_flags, labels=labels)
    base_tokens = common.pop("visual_tokens")
    outs = [model.forward(visual_tokens=base_tokens, **common)]
    patch_masks = torch.cat([torch.zeros(1, 2 * T, 2 * T, dtype=torch.bool), cell_patches(blocks).view(nb * nb, 2 * T, 2 * T)])      # [1 + blocks, G, G], the control first
    nv = patch_masks.shape[0]
    for f in sweep:
        clips = [b for b in range(B) if bool(has[b, f])]                                                       # (never empty: the longest clip has every f < F)
        src = [int(keep[first[b] + f]) for b in clips]
        pv = pixel_values[src].repeat_interleave(nv, 0)                                                        # clip-major, variant-minor
        variants = model.vit_tokens(pv, patch_drop=patch_masks.repeat(len(clips), 1, 1)).view(len(clips), nv, *base_tokens.shape[1:])
        for i in range(nv):
            tokens = base_tokens.clone()
            tokens[src] = variants[:, i]
            kw = {}
            if hide_tokens and i > 0:
                keys = torch.zeros(units.shape[0], units.shape[2], dtype=torch.bool)
                for b in clips:
                    keys[b, units[b, f].nonzero().flatten()[blocks.view(nb * nb, T * T)[i - 1]]] = True      # the block's tokens among frame f's, in order
                kw["key_drop"] = keys
            outs.append(model.forward(visual_tokens=tokens, **kw, **common))
    res = {"outs": outs, "blocks": blocks}
    if "score1" in outs[0]:
        base = outs[0]["score1"].float()
        control = torch.full((B, F), float("nan"), dtype=torch.float32, device=base.device)
        occluded = torch.full((B, F, nb * nb), float("nan"), dtype=torch.float32, device=base.device)
        for n, f in enumerate(sweep):
            got = outs[1 + n * nv:1 + (n + 1) * nv]
            there = has[:, f].to(base.device)
            control[:, f] = torch.where(there, got[0]["score1"].float(), control[:, f])
            occluded[:, f] = torch.where(there[:, None], torch.stack([o["score1"].float() for o in got[1:]], 1), occluded[:, f])
        occluded = occluded.view(B, F, nb, nb)
        res.update(score1=base, control=control, occluded=occluded, delta=control[:, :, None, None] - occluded)
    return res


def flow_knockout(model, *, pixel_values, input_ids, attention_mask, image_flags, labels=None, paths=None, width=4, stride=None, **readout_kwargs):
    """WHICH WAY, AT WHICH DEPTH a group of tokens reaches the score: the attention knock-out.  The batch is scored once as it is and once per
    (path, layer window) with the edges of that path cut inside that window (``forward(key_drop=keys, key_drop_rows=rows,
    key_drop_layers=(lo, hi))``); every other edge and layer stays.  ``paths``: a list of ``(name, keys, rows)`` with bool [B, N] masks laid out
    like ``input_ids`` (``rows`` None: every row) - default, from ``model.segment_masks``: ``frames->score_row``, ``frames->text_after`` and
    ``text_after->score_row`` (the text behind the frames minus the score row itself, read by the score row).  Windows: ``(lo, min(lo + width,
    L))`` for lo = 0, stride, 2 stride, ... < L; ``stride`` defaults to ``width``.  InternViT and the SlowFast branch run ONCE; their outputs
    are handed to every pass.  ``readout_kwargs`` (``motion_feature`` among them) go to every ``forward`` call.

    Returns a dict: ``outs`` - the base result dict, then one per path and window, path-major; ``paths`` - the list of (name, keys, rows);
    ``windows`` - the list of (lo, hi); and for a stage-2 model ``score1`` [B] (the base scores, fp32), ``knocked`` [B, P, W] (the score under
    the knock-out; NaN where the clip has no such key or no such row, ``frame_ablation``'s convention for a frame a clip lacks) and ``delta`` =
    ``score1[:, None, None] - knocked``: positive where the path, in that window, raised the score."""
    import torch
    B = int(input_ids.shape[0])
    windows = _windows("flow_knockout", int(model.config.llm_config.num_hidden_layers), width, stride)
    if paths is None:
        seg = model.segment_masks(input_ids, attention_mask, image_flags, n_frames=int(pixel_values.shape[0]))
        paths = [("frames->score_row", seg["frames"], seg["score_row"]), ("frames->text_after", seg["frames"], seg["text_after"]),
                 ("text_after->score_row", seg["text_after"] & ~seg["score_row"], seg["score_row"])]
    paths = [(str(name), keys.detach().to("cpu").bool(), None if rows is None else rows.detach().to("cpu").bool()) for name, keys, rows in paths]
    common = _once_per_batch(model, pixel_values, readout_kwargs, input_ids=input_ids, attention_mask=attention_mask, image_flags=image_flags, labels=labels)
    outs = [model.forward(**common)]
    for name, keys, rows in paths:
        for w in windows:
            outs.append(model.forward(key_drop=keys, key_drop_rows=rows, key_drop_layers=w, **common))
    absent = [~keys.any(-1) | (torch.zeros(B, dtype=torch.bool) if rows is None else ~rows.any(-1)) for _, keys, rows in paths]      # per path: keys or rows missing
    return _knocked({"outs": outs, "paths": paths, "windows": windows}, outs, B, (len(paths), len(windows)), torch.stack(absent, 1) if paths else None)


def restored_fraction(score, clean_score, corrupt_score):
    """How far a patched score moved from the corrupt pass's towards the clean pass's: ``(score - corrupt) / (clean - corrupt)``, 0 = the patch did
    nothing, 1 = the clean score restored.  ``score`` [B, ...], ``clean_score`` / ``corrupt_score`` [B]; fp32; NaN where the denominator is 0."""
    import torch
    score, clean, corrupt = score.float(), clean_score.float(), corrupt_score.float()
    if clean.shape != corrupt.shape or clean.dim() != 1 or score.dim() < 1 or score.shape[0] != clean.shape[0]:
        raise ValueError(f"restored_fraction: expected score [B, ...] and clean / corrupt [B], got {tuple(score.shape)}, {tuple(clean.shape)}, {tuple(corrupt.shape)}")
    shape = (-1,) + (1,) * (score.dim() - 1)
    den = (clean - corrupt).view(shape).expand_as(score)
    out = (score - corrupt.view(shape)) / den
    return torch.where(den == 0, torch.full_like(out, float("nan")), out)


def _same_layout(where, model, clean, corrupt):
    """The input checks of a donor / recipient sweep (``causal_trace``, ``head_trace``): equal shapes, equal ``attention_mask``, equal
    ``<IMG_CONTEXT>`` positions, equal ``image_flags`` - else a ValueError that starts with ``where``.  -> (B, N)."""
    import torch
    ids, ids_c = clean["input_ids"], corrupt["input_ids"]
    if tuple(ids.shape) != tuple(ids_c.shape):
        raise ValueError(f"{where}: input_ids of shape {tuple(ids.shape)} (clean) and {tuple(ids_c.shape)} (corrupt): the two need one token layout")
    B, N = (int(v) for v in ids.shape)
    for key in ("pixel_values", "image_flags"):
        if tuple(clean[key].shape) != tuple(corrupt[key].shape):
            raise ValueError(f"{where}: {key} of shape {tuple(clean[key].shape)} (clean) and {tuple(corrupt[key].shape)} (corrupt)")
    am, am_c = clean.get("attention_mask"), corrupt.get("attention_mask")
    if (am is None) != (am_c is None) or (am is not None and not torch.equal(am.detach().cpu().bool(), am_c.detach().cpu().bool())):
        raise ValueError(f"{where}: the clean and the corrupt attention_mask differ")
    ctx_id = model.img_context_token_id
    if not torch.equal(ids.detach().cpu() == ctx_id, ids_c.detach().cpu() == ctx_id):
        raise ValueError(f"{where}: the clean and the corrupt input_ids have their <IMG_CONTEXT> tokens at different positions")
    if not torch.equal(clean["image_flags"].detach().cpu(), corrupt["image_flags"].detach().cpu()):
        raise ValueError(f"{where}: the clean and the corrupt image_flags differ")
    return B, N


def causal_trace(model, *, clean, corrupt, groups=None, width=1, stride=1, **readout_kwargs):
    """WHERE THE QUALITY LIVES: activation patching (causal tracing, Meng et al. 2022) between two clips that share a token layout.  ``clean`` (the
    donor) and ``corrupt`` (the recipient) are dicts of ``forward``'s inputs (``pixel_values``, ``input_ids``, ``attention_mask``, ``image_flags``,
    optionally ``labels``, ``motion_feature``, ``mos``) with equal shapes, equal ``attention_mask`` and equal ``<IMG_CONTEXT>`` positions - anything
    else is a ValueError.  The clean batch runs once, capturing the residual stream of the union of the groups at every depth
    (``forward(return_stream=...)``); the corrupt batch runs once as it is and once per (group, depth window) with the clean rows of that group
    patched in at the depths of the window (``forward(stream_patch=...)``).  ``groups``: a list of ``(name, mask)`` with bool [B, N] masks laid out
    like ``input_ids`` - default: ``frame0`` .. (``model.unit_masks``), ``motion``, ``text_before``, ``text_after`` (minus the score row) and
    ``score_row`` (``model.segment_masks``).  Windows: ``(lo, min(lo + width, L))`` for lo = 0, stride, 2 stride, ... < L.  The corrupt clip's
    InternViT and SlowFast branch run ONCE; their outputs are handed to every pass.  ``readout_kwargs`` go to every ``forward`` call.

    Returns a dict: ``outs`` - the clean result dict, the corrupt one, then one per group and window, group-major; ``names``; ``groups`` - the list
    of (name, mask); ``windows`` - the list of (lo, hi); and for a stage-2 model ``clean_score`` / ``corrupt_score`` [B] (fp32), ``score`` [B, G, W]
    (the corrupt clip's score under the patch) and ``restored`` = ``restored_fraction(score, clean_score, corrupt_score)``."""
    import torch
    from .readouts import StreamPatch
    B, N = _same_layout("causal_trace", model, clean, corrupt)
    ids, am = clean["input_ids"], clean.get("attention_mask")
    windows = _windows("causal_trace", int(model.config.llm_config.num_hidden_layers), width, stride)
    n_frames = int(clean["pixel_values"].shape[0])
    if groups is None:
        units = model.unit_masks(ids, am, clean["image_flags"], n_frames=n_frames)
        seg = model.segment_masks(ids, am, clean["image_flags"], n_frames=n_frames)
        F = units.shape[1] - 1
        groups = [(f"frame{u}", units[:, u]) for u in range(F)] + [("motion", units[:, F]), ("text_before", seg["text_before"]),
                                                                     ("text_after", seg["text_after"] & ~seg["score_row"]), ("score_row", seg["score_row"])]
    groups = [(str(name), mask.detach().to("cpu").bool()) for name, mask in groups]
    for name, mask in groups:
        if tuple(mask.shape) != (B, N):
            raise ValueError(f"causal_trace: group {name!r} has shape {tuple(mask.shape)}, input_ids {(B, N)}")
    union = torch.zeros(B, N, dtype=torch.bool)
    for _, mask in groups:
        union |= mask
    donor = model.forward(**clean, return_stream=union, **readout_kwargs)                      # all depths: [n, L, H]
    index = donor["stream_index"].cpu()
    common = _recipient(model, corrupt, B, readout_kwargs)
    outs = [donor, model.forward(**common)]
    for name, mask in groups:
        own = mask[index[:, 0], index[:, 1]]                                                   # the union's rows that belong to this group
        at = own.nonzero().flatten().to(donor["stream"].device)
        rows = donor["stream"].index_select(0, at)
        for lo, hi in windows:
            outs.append(model.forward(stream_patch=StreamPatch(mask, rows[:, lo:hi].contiguous(), (lo, hi), index[own]), **common))
    return _restored({"outs": outs, "names": [name for name, _ in groups], "groups": groups, "windows": windows}, outs, B, (len(groups), len(windows)))


def _head_grid(where, model, layers, heads):
    L, nh = int(model.config.llm_config.num_hidden_layers), int(model.config.llm_config.num_attention_heads)
    layers = list(range(L)) if layers is None else [int(l) for l in layers]
    heads = list(range(nh)) if heads is None else [int(h) for h in heads]
    if any(not 0 <= l < L for l in layers) or any(not 0 <= h < nh for h in heads):
        raise ValueError(f"{where}: layers {layers} outside 0..{L - 1} or heads {heads} outside 0..{nh - 1}")
    return L, nh, layers, heads


def head_knockout(model, *, pixel_values, input_ids, attention_mask, image_flags, labels=None, layers=None, heads=None, rows=None, **readout_kwargs):
    """WHICH HEADS matter: the head knock-out (Michel et al. 2019).  The batch is scored once as it is and once per (layer, head) with that head's
    attention output multiplied by 0 in front of that layer's ``wo`` (``forward(head_scale=HeadScale(scale, rows))``, ``scale`` all ones but that
    entry); every other head and layer stays.  ``layers`` / ``heads``: the layer and head numbers swept (default: all); ``rows``: an optional bool
    [B, N] mask laid out like ``input_ids`` that restricts the knock-out to those query rows, e.g. ``model.segment_masks(...)["score_row"]``
    (None: every row).  InternViT and the SlowFast branch run ONCE; their outputs are handed to every pass.  ``readout_kwargs``
    (``motion_feature`` among them) go to every ``forward`` call.

    Returns a dict: ``outs`` - the base result dict, then one per layer and head, layer-major; ``layers``; ``heads``; and for a stage-2 model
    ``score1`` [B] (the base scores, fp32), ``knocked`` [B, L', n'] (the score with that head knocked out; NaN where ``rows`` selects no row of
    the clip, ``flow_knockout``'s convention) and ``delta`` = ``score1[:, None, None] - knocked``: positive where the head raised the score."""
    import torch
    from .readouts import HeadScale
    B = int(input_ids.shape[0])
    L, nh, layers, heads = _head_grid("head_knockout", model, layers, heads)
    rows = None if rows is None else rows.detach().to("cpu").bool()
    common = _once_per_batch(model, pixel_values, readout_kwargs, input_ids=input_ids, attention_mask=attention_mask, image_flags=image_flags, labels=labels)
    outs = [model.forward(**common)]
    for l in layers:
        for h in heads:
            scale = torch.ones(L, nh)
            scale[l, h] = 0.0
            outs.append(model.forward(head_scale=HeadScale(scale, rows), **common))
    return _knocked({"outs": outs, "layers": layers, "heads": heads}, outs, B, (len(layers), len(heads)), None if rows is None else ~rows.any(-1))


def head_trace(model, *, clean, corrupt, layers=None, heads=None, rows=None, **readout_kwargs):
    """WHICH HEADS carry the quality from one clip to another: head-level activation patching (path patching, Wang et al. 2022) between two clips
    that share a token layout.  ``clean`` (the donor) and ``corrupt`` (the recipient) are dicts of ``forward``'s inputs under ``causal_trace``'s
    conditions - anything else is a ValueError.  The clean batch runs once, capturing the head outputs of the tokens ``rows`` selects (bool [B, N];
    default: every token the pass runs) at every layer (``forward(return_heads=...)``); the corrupt batch runs once as it is and once per (layer,
    head) with that clean head patched in over those rows (``forward(head_patch=HeadPatch(rows, values, (l, l + 1), index, heads={h}))``).  The
    corrupt clip's InternViT and SlowFast branch run ONCE.  ``readout_kwargs`` go to every ``forward`` call.

    Returns a dict: ``outs`` - the clean result dict, the corrupt one, then one per layer and head, layer-major; ``layers``; ``heads``; and for a
    stage-2 model ``clean_score`` / ``corrupt_score`` [B] (fp32), ``score`` [B, L', n'] (the corrupt clip's score under the patch) and
    ``restored`` = ``restored_fraction(score, clean_score, corrupt_score)``."""
    import torch
    from .readouts import HeadPatch
    B, N = _same_layout("head_trace", model, clean, corrupt)
    L, nh, layers, heads = _head_grid("head_trace", model, layers, heads)
    rows = torch.ones(B, N, dtype=torch.bool) if rows is None else rows.detach().to("cpu").bool()
    if tuple(rows.shape) != (B, N):
        raise ValueError(f"head_trace: rows has shape {tuple(rows.shape)}, input_ids {(B, N)}")
    donor = model.forward(**clean, return_heads=rows, **readout_kwargs)                        # all layers: [n, L, n_heads, D]
    index = donor["heads_index"].cpu()
    common = _recipient(model, corrupt, B, readout_kwargs)
    outs = [donor, model.forward(**common)]
    for l in layers:
        values = donor["heads"][:, l:l + 1].contiguous()
        for h in heads:
            only = torch.zeros(nh, dtype=torch.bool)
            only[h] = True
            outs.append(model.forward(head_patch=HeadPatch(rows, values, (l, l + 1), index, only), **common))
    return _restored({"outs": outs, "layers": layers, "heads": heads}, outs, B, (len(layers), len(heads)))


def mlp_knockout(model, *, pixel_values, input_ids, attention_mask, image_flags, labels=None, layers=None, rows=None, **readout_kwargs):
    """WHICH MLP matters: the whole-block knock-out.  The batch is scored once as it is and once per layer with every neuron of that layer's MLP
    multiplied by 0 in front of its ``w2`` (``forward(neuron_scale=NeuronScale(scale, rows=rows))``, ``scale`` [L] all ones but that entry) - the
    MLP then adds nothing to the stream there.  ``layers``: the layers swept (default: all); ``rows``: an optional bool [B, N] mask that restricts
    the knock-out to those rows (None: every row).  In a row-trimmed last layer only the consumed rows have an MLP to knock out.  InternViT and
    the SlowFast branch run ONCE.  Beside ``head_knockout`` (all heads of a layer) this answers, per layer, whether attention or the MLP carries
    the score.

    Returns a dict: ``outs`` - the base result dict, then one per layer; ``layers``; and for a stage-2 model ``score1`` [B], ``knocked`` [B, L']
    (NaN where ``rows`` selects no row of the clip) and ``delta`` = ``score1[:, None] - knocked``."""
    import torch
    from .readouts import NeuronScale
    B = int(input_ids.shape[0])
    L = int(model.config.llm_config.num_hidden_layers)
    layers = list(range(L)) if layers is None else [int(l) for l in layers]
    if any(not 0 <= l < L for l in layers):
        raise ValueError(f"mlp_knockout: layers {layers} outside 0..{L - 1}")
    rows = None if rows is None else rows.detach().to("cpu").bool()
    common = _once_per_batch(model, pixel_values, readout_kwargs, input_ids=input_ids, attention_mask=attention_mask, image_flags=image_flags, labels=labels)
    outs = [model.forward(**common)]
    for l in layers:
        scale = torch.ones(L)
        scale[l] = 0.0
        outs.append(model.forward(neuron_scale=NeuronScale(scale, None, rows), **common))
    return _knocked({"outs": outs, "layers": layers}, outs, B, (len(layers),), None if rows is None else ~rows.any(-1))


def neuron_knockout(model, neurons, *, pixel_values, input_ids, attention_mask, image_flags, labels=None, rows=None, **readout_kwargs):
    """WHICH NEURONS matter: the single-neuron ablation.  ``neurons``: integer tensor (or list of pairs) [m, 2] of (layer, neuron).  The batch is
    scored once as it is and once per listed pair with that neuron multiplied by 0 (``forward(neuron_scale=NeuronScale([0.], [[l, j]], rows))``).
    ``rows`` and the once-per-batch front end as in ``mlp_knockout``.

    Returns a dict: ``outs`` - the base result dict, then one per pair; ``neurons`` (host int64 [m, 2]); and for a stage-2 model ``score1`` [B],
    ``knocked`` [B, m] and ``delta`` = ``score1[:, None] - knocked``."""
    import torch
    from .readouts import NeuronScale
    B = int(input_ids.shape[0])
    l = model.config.llm_config
    neurons = torch.as_tensor(neurons).detach().to("cpu")
    if neurons.is_floating_point() or neurons.dtype == torch.bool or neurons.dim() != 2 or int(neurons.shape[1]) != 2:
        raise ValueError("neuron_knockout: neurons must be an integer tensor [m, 2] of (layer, neuron) pairs")
    neurons = neurons.to(torch.long)
    if neurons.numel() and (int(neurons.min()) < 0 or int(neurons[:, 0].max()) >= l.num_hidden_layers or int(neurons[:, 1].max()) >= l.intermediate_size):
        raise ValueError(f"neuron_knockout: a (layer, neuron) pair outside layers 0..{l.num_hidden_layers - 1}, neurons 0..{l.intermediate_size - 1}")
    rows = None if rows is None else rows.detach().to("cpu").bool()
    common = _once_per_batch(model, pixel_values, readout_kwargs, input_ids=input_ids, attention_mask=attention_mask, image_flags=image_flags, labels=labels)
    outs = [model.forward(**common)]
    for pair in neurons:
        outs.append(model.forward(neuron_scale=NeuronScale(torch.zeros(1), pair[None], rows), **common))
    return _knocked({"outs": outs, "neurons": neurons}, outs, B, (int(neurons.shape[0]),), None if rows is None else ~rows.any(-1))


def rank_neurons(clean, corrupt, top: int):
    """The ranking ``neuron_trace`` patches by: ``clean`` / ``corrupt`` - two captures [n, W, I] of the same rows - -> int64 [W, top]: per layer the
    neurons with the largest |clean - corrupt|, taken in fp32 and summed over the n rows (all clips together), largest first; among equals the
    lower neuron number first.  A NaN difference (a row the trimmed last layer does not consume) counts as 0."""
    import torch
    diff = torch.nan_to_num((clean.float() - corrupt.float()).abs(), nan=0.0, posinf=float("inf")).sum(0)      # [W, I]
    return torch.sort(diff, dim=-1, descending=True, stable=True).indices[:, :int(top)].cpu()


def neuron_trace(model, *, clean, corrupt, layers=None, top: int = 16, rows=None, **readout_kwargs):
    """WHICH NEURONS carry the quality from one clip to another: neuron-level activation patching between two clips that share a token layout
    (``causal_trace``'s conditions - anything else is a ValueError).  Both batches run once, capturing the MLP neurons of the tokens ``rows``
    selects (bool [B, N]; default: the score row) over the window ``layers`` = (lo, hi) (default: every layer).  Per layer the neurons are ranked by
    |clean - corrupt| (``rank_neurons``), and for each of the ``top`` first the clean neuron is patched into the corrupt batch over those rows in
    one sparse patch pass (``forward(neuron_patch=NeuronPatch(rows, values, (l, l + 1), index, neurons=[j]))``).  The corrupt clip's InternViT and
    SlowFast branch run ONCE.

    Returns a dict: ``outs`` - the clean result dict, the corrupt one, then one per layer and rank, layer-major; ``layers`` (the window);
    ``neurons`` (int64 [hi - lo, top]); and for a stage-2 model ``clean_score`` / ``corrupt_score`` [B], ``score`` [B, hi - lo, top] and
    ``restored`` = ``restored_fraction(score, clean_score, corrupt_score)``."""
    import torch
    from .readouts import NeuronPatch
    B, N = _same_layout("neuron_trace", model, clean, corrupt)
    L, I = int(model.config.llm_config.num_hidden_layers), int(model.config.llm_config.intermediate_size)
    lo, hi = (0, L) if layers is None else (int(layers[0]), int(layers[1]))
    top = int(top)
    if not 0 <= lo <= hi <= L or not 1 <= top <= I:
        raise ValueError(f"neuron_trace: layers ({lo}, {hi}) outside 0 <= lo <= hi <= {L} or top = {top} outside 1..{I}")
    if rows is None:
        rows = model.segment_masks(clean["input_ids"], clean.get("attention_mask"), clean["image_flags"])["score_row"]
    rows = rows.detach().to("cpu").bool()
    if tuple(rows.shape) != (B, N):
        raise ValueError(f"neuron_trace: rows has shape {tuple(rows.shape)}, input_ids {(B, N)}")
    donor = model.forward(**clean, return_neurons=rows, neuron_layers=(lo, hi), **readout_kwargs)         # [n, hi - lo, I]
    index = donor["neurons_index"].cpu()
    common = _recipient(model, corrupt, B, readout_kwargs)
    base = model.forward(**common, return_neurons=rows, neuron_layers=(lo, hi))
    ranked = rank_neurons(donor["neurons"], base["neurons"], top)
    outs = [donor, base]
    for w in range(hi - lo):
        for j in ranked[w].tolist():
            values = donor["neurons"][:, w:w + 1, j:j + 1].contiguous()
            outs.append(model.forward(neuron_patch=NeuronPatch(rows, values, (lo + w, lo + w + 1), index, torch.tensor([j])), **common))
    return _restored({"outs": outs, "layers": (lo, hi), "neurons": ranked}, outs, B, (hi - lo, top))


def frame_ablation_generate(
model, *, pixel_values, input_ids, attention_mask, image_flags, max_new_tokens, candidate_ids=None, **gen):
    """WHAT IF a frame were not there, in WORDS: the reply to the stage-2 prompt as it is and once per unit with that unit's tokens hidden from
    the LLM (``generate_stage2(key_drop=model.unit_masks(...)[:, u])``) - unit u < F is frame u's visual tokens, unit F the motion token.
    InternViT and the SlowFast branch run ONCE; their outputs are handed to every call (``visual_tokens=``, ``motion_feature=``).  ``gen`` goes to
    every ``generate_stage2`` call (``eos_token_id``, ``pad_token_id``, ``motion_feature``, sampling settings, ...).

    Returns a dict: ``sequences`` long [B, F + 2, T], T = ``max_new_tokens`` - row 0 the base reply, row u + 1 the reply with unit u hidden, the pad
    id (``pad_token_id`` of ``gen``, else the model's) after a reply's end token and in the rows of units a clip does not have; ``units`` - the
    masks, bool [B, F + 1, N]; with ``candidate_ids`` also ``cand_logprobs`` fp32 [B, F + 2, T, C] - the candidates' log-probabilities at every
    step of every reply, NaN after the end token and for the units a clip does not have."""
    import torch
    B, T = int(input_ids.shape[0]), int(max_new_tokens)
    n_frames = int(pixel_values.shape[0])
    units = model.unit_masks(input_ids, attention_mask, image_flags, n_frames=n_frames)                        # host bool [B, F + 1, N]
    gen = dict(gen)
    motion_feature = gen.pop("motion_feature", None)
    if motion_feature is None:
        motion_feature = model.motion_feature(pixel_values, B)
    tokens = model.vit_tokens(pixel_values)
    pad = gen.get("pad_token_id")
    pad = model.config.llm_config.pad_token_id if pad is None else pad
    common = dict(input_ids=input_ids, attention_mask=attention_mask, image_flags=image_flags, motion_feature=motion_feature, visual_tokens=tokens,
                  max_new_tokens=T, **gen)
    if candidate_ids is not None:
        common["candidate_ids"] = candidate_ids
    outs = [model.generate_stage2(None, **common)] + [model.generate_stage2(None, key_drop=units[:, u], **common) for u in range(units.shape[1])]
    seqs = [o if torch.is_tensor(o) else o["sequences"] for o in outs]
    dev = seqs[0].device
    absent = torch.cat([torch.zeros(B, 1, dtype=torch.bool), ~units.any(-1)], 1).to(dev)                      # [B, F + 2]: the clip has no such unit
    sequences = torch.full((B, len(outs), T), int(pad), dtype=torch.long, device=dev)
    for i, sq in enumerate(seqs):
        sequences[:, i, : sq.shape[1]] = sq
    sequences = sequences.masked_fill(absent[:, :, None], int(pad))
    res = {"sequences": sequences, "units": units}
    if candidate_ids is not None:
        C = outs[0]["cand_logprobs"].shape[-1]
        clp = torch.full((B, len(outs), T, C), float("nan"), dtype=torch.float32, device=dev)
        for i, o in enumerate(outs):
            clp[:, i, : o["cand_logprobs"].shape[1]] = o["cand_logprobs"]
        res["cand_logprobs"] = clp.masked_fill(absent[:, :, None, None], float("nan"))
    return res


def batched(items, model, k: int = 4, frames=None, ahead: bool = True, pad_id: int = 2, return_logprobs: bool = False, candidate_ids=None,
            top_logprobs=None):
    """The reference's eval loop at batch ``k`` instead of batch 1: yields ``(item, output)`` for EVERY item of ``items`` (the loop's
    ``DataLoader(batch_size=1)`` items: ``input_ids`` / ``attention_mask`` / ``labels`` [1, N_i] with N_i ragged, ``image_flags``
    [1, T, 1], ``pixel_values`` [1, T, 3, S, S] or what ``frames(item)`` returns - uint8 [T, H, W, 3] decoded frames are ingested on the
    GPU), where ``output`` is what ``model(...)`` on that item alone returns - ``score1`` [1], ``logit`` [N_i - 1], ``label`` [N_i - 1], and
    ``loss`` when the item carries ``mos`` - as HOST tensors, bit for bit: a clip's score and level tokens do not depend on its batch
    mates (per-clip row plans; tests/test_gpu_e2e.py proves ``torch.equal``), so grouping changes the speed and nothing else.

    Up to ``k`` consecutive items of the same frame geometry form a group: ids / labels right-padded to the group's longest prompt as
    the reference's collator does (internvl/patch/pad_data_collator.py:60-67: pad id, IGNORE_INDEX, mask = ids != pad - here the items'
    own masks are kept), frames and flags concatenated (:93-99), ONE ``forward`` and ONE device-to-host copy of its results per group.
    With ``ahead`` the NEXT group's visual front (H2D copy, resize + normalise, InternViT, SlowFast) runs on its own stream beside this
    group's InternLM2 pass (``InternVLChatModel.prefetch``), and a group's results are fetched only after the next group's pass has been
    enqueued (the GPU never waits for the host's loop body; results arrive one group late, in order).  The loop changes by two lines:

        for item2, output in eval_utils.batched(eval_utils.shard(train_dataloader, rank, world), model, k=4):
            score1 = output['score1'].item()          # `output = model(...)` and the `.to(model.device)` copies above it go away

    ``items`` may be sharded first (``shard``) so that N ranks score N disjoint shares.

    ``return_logprobs``: ``model(..., return_logprobs=True)`` per group; each item's output adds ``logprob`` [N_i - 1] (bit for bit the
    item's own pass) and its own ``ce_loss``, ``-(logprob[label != -100]).double().mean().float()`` (NaN without answer labels).

    ``candidate_ids``: ``model(..., candidate_ids=...)`` per group; each item's output adds ``cand_logprob`` [N_i - 1, C], bit for bit the
    item's own pass.

    ``top_logprobs``: ``model(..., top_logprobs=k)`` per group; each item's output adds ``top_ids`` / ``top_logprob`` [N_i - 1, k], bit for
    bit the item's own pass."""
    import torch
    import torch.nn.functional as F
    from . import readouts
    if k < 1:
        raise ValueError("k must be >= 1")
    ro = readouts.ReadOuts(bool(return_logprobs), candidate_ids, top_logprobs)
    get = frames or _frames_of

    def groups():
        cur, geom = [], None
        for item in items:
            f = get(item)
            g = (tuple(f.shape), f.dtype)
            if cur and (g != geom or len(cur) == k):
                yield cur
                cur = []
            geom = g
            cur.append((item, f))
        if cur:
            yield cur

    def start(group):
        fr = [f for _, f in group]
        if fr[0].dtype == torch.uint8:                     # decoded frames: copied up clip by clip and joined on the device (ingest_frames)
            return model.prefetch(frames_u8=fr, n_clips=len(group)) if ahead else model.ingest_frames(fr)
        pv = torch.cat([f.to(device=model.device, dtype=torch.bfloat16, non_blocking=True) for f in fr]) if len(fr) > 1 else \
            fr[0].to(device=model.device, dtype=torch.bfloat16, non_blocking=True)
        return model.prefetch(pixel_values=pv, n_clips=len(group)) if ahead else pv

    def row(t):
        return t.reshape(-1) if t.dim() <= 1 or t.shape[0] != 1 else t[0].reshape(-1)

    def enqueue(group, front):
        """ONE forward for the group: everything is enqueued, nothing is waited for."""
        ids = [row(it["input_ids"]) for it, _ in group]
        labels = [row(it["labels"]) for it, _ in group]
        masks = [row(it["attention_mask"]).bool() if it.get("attention_mask") is not None else torch.ones_like(i, dtype=torch.bool) for (it, _), i in zip(group, ids)]
        n = [int(i.numel()) for i in ids]
        nmax = max(n)
        pad = lambda t, v: F.pad(t.cpu(), (0, nmax - t.numel()), value=v)
        flags = None
        if all(it.get("image_flags") is not None for it, _ in group):
            flags = torch.cat([(it["image_flags"][0] if it["image_flags"].dim() == 3 else it["image_flags"]).reshape(-1, 1) for it, _ in group])
        motion = None                                      # (optional: items that carry a precomputed SlowFast feature [1, motion_dim])
        if all(it.get("motion_feature") is not None for it, _ in group):
            motion = torch.cat([it["motion_feature"].reshape(1, -1) for it, _ in group])
        out = model(mos=None, pixel_values=front, input_ids=torch.stack([pad(i, pad_id) for i in ids]),
                    attention_mask=torch.stack([pad(m, False) for m in masks]), image_flags=flags,
                    labels=torch.stack([pad(l, -100) for l in labels]), **({} if motion is None else {"motion_feature": motion}),
                    **readouts.forward_kwargs(ro))
        return group, n, nmax, out

    def collect(run):
        """The group's results to the host - ONE synchronisation per group (the plain loop has one per clip: score1.item(), stage2_eval.py:938) - and
        out per item."""
        group, n, nmax, out = run
        rows = {name: out[name].view((len(group), nmax - 1) + width).cpu() for name, width in [("label", ())] + [f[:2] for f in ro.row_fields()]}
        score1 = out["score1"].cpu() if "score1" in out else None
        for b, (it, _) in enumerate(group):
            o = {name: t[b, : n[b] - 1].clone() for name, t in rows.items()}
            if return_logprobs:
                o["ce_loss"] = (-o["logprob"][o["label"] != -100]).double().mean().float()
            if score1 is not None:
                o["score1"] = score1[b: b + 1].clone()
                mos = it.get("mos")
                o["loss"] = F.l1_loss(o["score1"], row(mos)[:1].to(o["score1"].dtype)) if mos is not None else None
            yield it, o

    it = groups()
    try:
        cur = next(it)
    except StopIteration:
        return
    front = start(cur)
    # Software pipeline, two deep: group g's forward is ENQUEUED before group g - 1's results are fetched, so the GPU already holds its next pass
    # while the host copies results back and the caller's loop body (token decoding, CSV rows) runs; the results of a group therefore come
    # out one group late - every item still comes out, in order.
    pending = None
    for nxt in it:
        nxt_front = start(nxt) if ahead else None          # enqueued BEFORE this group's InternLM2 pass: the two run side by side
        run = enqueue(cur, front)
        if pending is not None:
            yield from collect(pending)
        pending = run
        cur, front = nxt, nxt_front if ahead else start(nxt)
    run = enqueue(cur, front)
    if pending is not None:
        yield from collect(pending)
    yield from collect(run)


def score_dataset(items, model, tokenizer, k: int = 4, frames=None, group=None, output_file: Optional[str] = None, im_end_id: int = 92542):
    """The body of the reference's eval loop as ONE call (stage2_eval.py:908-972; stage1_eval.py:905-960 is the same body without the score):
    every item of ``items`` (this rank's share: pass ``shard(dataset, rank, world)`` wrapped in the driver's ``DataLoader(batch_size=1)``) scored
    through ``batched`` in groups of ``k``; per item the answer-token slice (:940-941) is decoded with ``tokenizer``, parsed into a level
    (:956-967) and appended as the driver's row ``[video_name, answer, output, mos, score1, level]`` (:970); the rows of all ranks of ``group``
    are put back into the set's order (``gather_rows``) and, on the caller's side, go through ``save_and_evaluate`` (:973) when ``output_file``
    is given or metrics are wanted.  Returns ``(rows, metrics)``; ``metrics`` is None when the set is empty.  A stage-1 model returns no ``score1``: its
    rows carry 0.0 in that column."""
    rows = []
    for item, out in batched(items, model, k=k, frames=frames):
        labels_row = item["labels"][0] if item["labels"].dim() == 2 else item["labels"]
        pred = answer_ids(labels_row, out["logit"], im_end_id=im_end_id)
        text = tokenizer.decode(pred)
        name = item["video_name"][0] if isinstance(item.get("video_name"), (list, tuple)) else item.get("video_name")
        answer = item["answer"][0] if isinstance(item.get("answer"), (list, tuple)) else item.get("answer", "")
        mos = float(item["mos"].reshape(-1)[0]) if item.get("mos") is not None else 0.0
        score1 = float(out["score1"].float().item()) if "score1" in out else 0.0
        rows.append([name, answer, text, mos, score1, parse_level(text)])
    rows = gather_rows(rows, group)
    return rows, (save_and_evaluate(rows, output_file) if rows else None)
