"""Which read-outs a scoring pass carries: label log-probs, candidate log-probs, top-k log-probs, score attention by segment and per token, the
score row's value vectors per segment (``return_score_values``), the depth lens, a capture of residual-stream rows (``return_stream`` /
``stream_depths``) or of per-head attention outputs (``return_heads`` /
``head_layers``) - and whether it runs under a key-drop mask (``key_drop`` with its qualifiers ``key_drop_rows`` / ``key_drop_layers``), a patch of the
stream (``stream_patch``), a patch of head outputs (``head_patch``) or a per-head scale (``head_scale``): not read-outs, but per-call options that
travel the same way.  The MLP's side of a layer has the same three: a capture of the neurons ``w2`` consumes (``return_neurons`` / ``neuron_layers`` /
``neuron_ids``), a patch (``neuron_patch``) and a scale (``neuron_scale``).  The attention flow map of every query row (``return_segment_attention`` /
``return_row_attention``) travels as ``ReadOuts.attention_map``, a plain attribute beside the fields.

This module is the one place that knows that decision.  A new read-out adds, HERE: a member to ``ReadOuts`` and its check to
``ReadOuts.parse``; the element it appends to a graph's host key to ``ReadOuts.key_tail``; its keyword to ``forward_kwargs``; and - when it
is laid out per label position like ``logit`` - a row of ``ROW_FIELDS``.  Elsewhere it adds only what computes it: the native call in
``ScoringPass._read_rows`` (or the probe) and, for generate(), in ``Generation._decode_step``.  ``forward``, the graph key, the shared-prefix
slices, ``dist_utils.score_clips_dp`` and ``eval_utils.batched`` follow from the record and the table.

The stream, head and neuron options are three lines of ONE table, ``FAMILIES``: a line names the family's keywords, records, messages' words and
``ReadOuts`` fields, and ``_capture`` / ``_patch`` / ``_scale`` check what the families share.  A new option of a family adds its slot to the line
and its check to the function of its kind; a new family adds a line, its records, the hooks for what only it has (a patch's extra field, a
scale's shape rules), a thin ``*_options`` front, its ``ReadOuts`` fields with their call in ``parse``, and ``forward()``'s keywords with their
paragraph.  ``touches_stream``, ``forward_kwargs``, ``ScoringPass.forward``'s eager half and its patch planner walk the table.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, NamedTuple, Optional

import torch

MAX_CANDIDATES = 64      # = AIGV_MAX_CANDIDATES
MAX_TOPK = 16            # = AIGV_MAX_TOPK
MAX_LENS_ROWS = 64       # = AIGV_MAX_LENS_ROWS
MAX_PROBE_ROWS = 64      # = AIGV_MAX_PROBE_ROWS
MAX_ATTN_SEGMENTS = 64   # = AIGV_MAX_ATTN_SEGMENTS
MAX_MAP_CLIPS = 127      # the attention map's sequence table: what one prefill call takes


def top_logprobs_k(top_logprobs, vocab: int, labels="given") -> int:
    """``top_logprobs`` (None or an int k, 1 <= k <= min(16, vocab)) -> k, 0 for None."""
    if top_logprobs is None:
        return 0
    if labels is None:
        raise ValueError("top_logprobs: needs labels (they mark the answer rows whose distribution is read)")
    k = top_logprobs
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_TOPK:
        raise ValueError(f"top_logprobs: expected an int in 1..{MAX_TOPK}, got {k!r}")
    if k > vocab:
        raise ValueError(f"top_logprobs: k = {k} exceeds the vocabulary ({vocab} tokens)")
    return k


def candidates(candidate_ids, labels="given") -> Optional[torch.Tensor]:
    """``candidate_ids`` (None, a list of ints or an integer tensor [C], on any device) -> None or a contiguous int64 tensor [C], 1 <= C <= 64.
    The VALUES are not looked at (they may live on the device): an id outside the vocabulary gives a NaN column."""
    if candidate_ids is None:
        return None
    if labels is None:
        raise ValueError("candidate_ids: needs labels (they mark the answer rows whose distribution is read)")
    t = candidate_ids if torch.is_tensor(candidate_ids) else torch.tensor([int(v) for v in candidate_ids], dtype=torch.long)
    if t.dim() != 1 or t.is_floating_point() or t.dtype == torch.bool or not 1 <= t.numel() <= MAX_CANDIDATES:
        raise ValueError(f"candidate_ids: expected 1..{MAX_CANDIDATES} integer token ids in one dimension, got "
                         f"{tuple(t.shape)} {t.dtype}")
    return t.to(torch.long).contiguous()


def _got(t) -> str:
    """How a message names what it got: a tensor's shape and dtype, anything else's type."""
    return f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__


def _token_mask(name: str, t, ids_shape=None) -> torch.Tensor:
    if not torch.is_tensor(t) or t.is_floating_point() or t.is_complex() or t.dim() != 2:
        raise ValueError(f"{name}: expected a bool or integer tensor [B, N] laid out like input_ids")
    if ids_shape is not None and tuple(t.shape) != tuple(ids_shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} differs from input_ids {tuple(ids_shape)}")
    return t.detach().to("cpu").bool().contiguous()


def _depth_window(name: str, depths, n_layers: Optional[int] = None) -> tuple:
    w = tuple(depths) if isinstance(depths, (tuple, list)) else None
    if w is None or len(w) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in w):
        raise ValueError(f"{name}: expected a pair of ints (lo, hi), got {depths!r}")
    lo, hi = w
    if not 0 <= lo <= hi or (n_layers is not None and hi > n_layers):
        raise ValueError(f"{name}: ({lo}, {hi}) outside 0 <= lo <= hi <= {n_layers if n_layers is not None else 'L'}")
    return lo, hi


def key_drop_mask(key_drop, ids_shape=None, probing: bool = False) -> Optional[torch.Tensor]:
    """``key_drop`` (None, or a bool / integer tensor [B, N] laid out like ``input_ids``, on any device) -> None or a HOST bool tensor [B, N].
    The shape is checked where ``ids_shape`` is known; the clip-dependent rules (first token, consumed rows) where the plan is
    (``ScoringPass._key_drop_words``)."""
    if key_drop is None:
        return None
    if probing:
        raise ValueError("key_drop: cannot be combined with return_score_attention / return_token_attention / return_score_values (the probe does not know "
                         "the mask)")
    return _token_mask("key_drop", key_drop, ids_shape)


def key_drop_qualifiers(key_drop, key_drop_rows=None, key_drop_layers=None, ids_shape=None, n_layers: Optional[int] = None):
    """The two qualifiers of ``key_drop`` -> (None or a HOST bool tensor [B, N], None or a pair of ints (lo, hi)).  ``key_drop_rows`` (bool or
    integer tensor [B, N] laid out like ``input_ids``, on any device): the query rows that are cut from the dropped keys - None: every row.
    ``key_drop_layers`` = (lo, hi): the layers lo <= l < hi run under the mask - None: all of them; 0 <= lo <= hi <= ``n_layers`` where that
    is known.  Either one without ``key_drop`` is a ValueError.  The clip-dependent rule (no row is cut from itself) is checked where the
    plan is (``ScoringPass._key_drop_words``)."""
    rows, window = None, None
    if key_drop_rows is not None:
        if key_drop is None:
            raise ValueError("key_drop_rows: qualifies key_drop and needs one")
        rows = _token_mask("key_drop_rows", key_drop_rows, ids_shape)
    if key_drop_layers is not None:
        if key_drop is None:
            raise ValueError("key_drop_layers: qualifies key_drop and needs one")
        window = _depth_window("key_drop_layers", key_drop_layers, n_layers)
    return rows, window


def refuse_key_drop_qualifiers(where: str, key_drop_rows=None, key_drop_layers=None) -> None:
    """The entry points that run through the KV cache take ``key_drop`` whole or not at all: the mask kept beside the cache has neither rows
    nor a layer window."""
    for name, v in (("key_drop_rows", key_drop_rows), ("key_drop_layers", key_drop_layers)):
        if v is not None:
            raise ValueError(f"{name}: {where} does not take it (the key-drop mask kept beside the KV cache has neither query rows nor a layer "
                             "window); forward() does")


class AttentionMap(NamedTuple):
    """``forward(return_segment_attention=..., return_row_attention=...)``, checked: the attention flow map of EVERY query row.  ``segments``: the
    segment-to-segment matrix per layer and head is returned; ``rows``: None, or the layer window (lo, hi) whose per-row bins are returned."""
    segments: bool
    rows: Optional[tuple]


def attention_map(return_segment_attention=False, return_row_attention=None, key_drop=None, n_layers: Optional[int] = None, ids_shape=None) -> Optional[AttentionMap]:
    """``return_segment_attention`` / ``return_row_attention`` -> None (both off) or the checked ``AttentionMap``.  ValueError for a window
    outside 0 <= lo <= hi <= L and for a call that also carries ``key_drop`` (the map recomputes the unmasked softmax: it does not know the
    mask) - and, where ``ids_shape`` is known, for more than 127 clips (the kernels' sequence table).  The bin count (at most 64) is checked
    where the table is counted (``ReadOuts.map_segments``)."""
    if not return_segment_attention and return_row_attention is None:
        return None
    if key_drop is not None:
        raise ValueError("key_drop: cannot be combined with return_segment_attention / return_row_attention (the map does not know the mask)")
    window = None if return_row_attention is None else _depth_window("return_row_attention", return_row_attention, n_layers)
    if ids_shape is not None and int(ids_shape[0]) > MAX_MAP_CLIPS:
        raise ValueError(f"return_segment_attention / return_row_attention: at most {MAX_MAP_CLIPS} clips per pass, got {int(ids_shape[0])}")
    return AttentionMap(bool(return_segment_attention), window)


# ---- the row options: a capture, a patch and a scale of the rows a layer consumes, per family (FAMILIES below) -----------------------------------
@dataclass(frozen=True, eq=False)
class StreamPatch:
    """``forward(stream_patch=...)``: overwrite rows of the residual stream.  ``rows``: bool or integer tensor [B, N] laid out like ``input_ids``
    (on any device) - the tokens patched; ``depths`` = (lo, hi), 0 <= lo <= hi <= L: immediately before each layer d, lo <= d < hi, runs;
    ``values``: bf16 [n, hi - lo, H] on the device or the host, laid out exactly like the ``stream`` that ``forward(return_stream=rows,
    stream_depths=depths)`` returns - n the selected tokens the pass runs, clip-major, position-ascending; ``index``: optionally the donor's
    ``stream_index`` (int64 [n, 2]), then checked pair by pair against the recipient's."""
    rows: torch.Tensor
    values: torch.Tensor
    depths: tuple
    index: Optional[torch.Tensor] = None


MAX_HEADS = 64     # a head mask travels as one uint64 per layer


@dataclass(frozen=True, eq=False)
class HeadPatch:
    """``forward(head_patch=...)``: overwrite per-head attention outputs - the row ``wo`` of a layer consumes.  ``rows``: bool or integer tensor [B, N]
    laid out like ``input_ids`` - the tokens patched; ``layers`` = (lo, hi), 0 <= lo <= hi <= L; ``values``: bf16 [n, hi - lo, n_heads, D] on the
    device or the host, laid out exactly like the ``heads`` that ``forward(return_heads=rows, head_layers=layers)`` returns; ``index``: optionally
    the donor's ``heads_index`` (int64 [n, 2]), checked pair by pair against the recipient's; ``heads``: bool [n_heads] or [hi - lo, n_heads] - the
    heads whose columns are overwritten (None: every head); an unselected head's values are not read."""
    rows: torch.Tensor
    values: torch.Tensor
    layers: tuple
    index: Optional[torch.Tensor] = None
    heads: Optional[torch.Tensor] = None


@dataclass(frozen=True, eq=False)
class HeadScale:
    """``forward(head_scale=...)``: multiply per-head attention outputs by a factor.  ``scale``: float tensor [L, n_heads] (taken to fp32 on the
    host; no NaN) - head h of layer l becomes ``bf16(fp32(x) * scale[l, h])``, an entry that is exactly 1 leaves its head untouched, 0 knocks it
    out; ``rows``: optional bool or integer tensor [B, N] - the query rows scaled (None: every row the pass runs)."""
    scale: torch.Tensor
    rows: Optional[torch.Tensor] = None


MAX_NEURON_SEL = 4096     # a sparse neuron list: at most this many entries per option (the context's device tables)


@dataclass(frozen=True, eq=False)
class NeuronPatch:
    """``forward(neuron_patch=...)``: overwrite MLP neurons - the row ``w2`` of a layer consumes.  ``rows``: bool or integer tensor [B, N] laid out
    like ``input_ids`` - the tokens patched; ``layers`` = (lo, hi), 0 <= lo <= hi <= L; ``values``: bf16 [n, hi - lo, I] - or [n, hi - lo, m] with
    ``neurons`` - on the device or the host, laid out exactly like the ``neurons`` that ``forward(return_neurons=rows, neuron_layers=layers,
    neuron_ids=neurons)`` returns; ``index``: optionally the donor's ``neurons_index`` (int64 [n, 2]), checked pair by pair against the
    recipient's; ``neurons``: integer tensor [m], strictly ascending inside [0, I) - the neurons overwritten (None: all of them); an unselected
    neuron is neither read nor written."""
    rows: torch.Tensor
    values: torch.Tensor
    layers: tuple
    index: Optional[torch.Tensor] = None
    neurons: Optional[torch.Tensor] = None


@dataclass(frozen=True, eq=False)
class NeuronScale:
    """``forward(neuron_scale=...)``: multiply MLP neurons by a factor.  With ``neurons=None``, ``scale`` is a float tensor [L]: every neuron of
    layer l becomes ``bf16(fp32(x) * scale[l])`` - 0 knocks the MLP block out.  Otherwise ``neurons`` is an integer tensor [m, 2] of unique
    (layer, neuron) pairs and ``scale`` a float tensor [m].  A factor that is exactly 1 leaves its neurons untouched; no NaN.  ``rows``: optional
    bool or integer tensor [B, N] - the rows scaled (None: every row the pass runs)."""
    scale: torch.Tensor
    neurons: Optional[torch.Tensor] = None
    rows: Optional[torch.Tensor] = None


def head_bits(heads: torch.Tensor) -> list:
    """A HOST bool [n_layers, n_heads] -> one int per layer with bit h set where head h is selected (the C ABI's uint64 words)."""
    return [sum(1 << h for h, on in enumerate(row) if on) for row in heads.tolist()]


def _neuron_ids(name: str, t, n_inter: Optional[int] = None) -> torch.Tensor:
    if not torch.is_tensor(t) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or t.dim() != 1:
        raise ValueError(f"{name}: expected an integer tensor [m] of neuron numbers")
    t = t.detach().to("cpu").to(torch.long).contiguous()
    m = int(t.numel())
    if m > MAX_NEURON_SEL:
        raise ValueError(f"{name}: {m} neurons, at most {MAX_NEURON_SEL} per option")
    if m and (int(t.min()) < 0 or (n_inter is not None and int(t.max()) >= n_inter)):
        raise ValueError(f"{name}: neuron numbers outside 0..{'I - 1' if n_inter is None else n_inter - 1}")
    if m > 1 and not bool((t[1:] > t[:-1]).all()):
        raise ValueError(f"{name}: neuron numbers must be strictly ascending")
    return t


# the families' own hooks.  ``sizes``: what is known of the model - n_layers, n_heads, head_dim, n_inter, hidden; a missing or None entry is not checked
def _patch_heads(p, values, lo, hi, sizes):
    """``HeadPatch.heads`` (checked behind the values, whose head count it goes by) -> None or a HOST bool [hi - lo, n_heads]."""
    hm, nh = p.heads, int(values.shape[2])
    if hm is None:
        return None
    if not torch.is_tensor(hm) or hm.dtype != torch.bool or tuple(hm.shape) not in ((nh,), (hi - lo, nh)):
        raise ValueError(f"head_patch: heads must be a bool tensor [n_heads = {nh}] or [hi - lo = {hi - lo}, n_heads = {nh}], got {_got(hm)}")
    return hm.detach().to("cpu").expand(hi - lo, nh).contiguous()


def _patch_neurons(p, values, lo, hi, sizes):
    """``NeuronPatch.neurons`` (checked in front of the values, whose width it sets) -> None or a HOST int64 [m]."""
    return None if p.neurons is None else _neuron_ids("neuron_patch: neurons", p.neurons, sizes.get("n_inter"))


def _head_scale_rules(q, sizes):
    t, L, nh = q.scale, sizes.get("n_layers"), sizes.get("n_heads")
    if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != 2 or (L is not None and int(t.shape[0]) != L) or (nh is not None and int(t.shape[1]) != nh):
        raise ValueError(f"head_scale: scale must be a float tensor [L{'' if L is None else f' = {L}'}, n_heads{'' if nh is None else f' = {nh}'}], got {_got(t)}")
    return HeadScale


def _neuron_scale_rules(q, sizes):
    """[L] factors, or [m] beside [m, 2] unique (layer, neuron) pairs - which then travel in the C ABI's order: by layer, then by neuron."""
    t, sel, L, I = q.scale, q.neurons, sizes.get("n_layers"), sizes.get("n_inter")
    if sel is None:
        if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != 1 or (L is not None and int(t.shape[0]) != L):
            raise ValueError(f"neuron_scale: scale must be a float tensor [L{'' if L is None else f' = {L}'}] when neurons is None, got {_got(t)}")
        return lambda t, rows: NeuronScale(t, None, rows)
    if not torch.is_tensor(sel) or sel.is_floating_point() or sel.dtype == torch.bool or sel.dim() != 2 or int(sel.shape[1]) != 2:
        raise ValueError("neuron_scale: neurons must be an integer tensor [m, 2] of (layer, neuron) pairs")
    sel = sel.detach().to("cpu").to(torch.long).contiguous()
    m = int(sel.shape[0])
    if m > MAX_NEURON_SEL:
        raise ValueError(f"neuron_scale: {m} neurons, at most {MAX_NEURON_SEL} per option")
    if not torch.is_tensor(t) or not t.is_floating_point() or tuple(t.shape) != (m,):
        raise ValueError(f"neuron_scale: scale must be a float tensor [m = {m}] beside neurons [m, 2], got {_got(t)}")
    if m and (int(sel.min()) < 0 or (L is not None and int(sel[:, 0].max()) >= L) or (I is not None and int(sel[:, 1].max()) >= I)):
        raise ValueError(f"neuron_scale: a (layer, neuron) pair outside layers 0..{'L - 1' if L is None else L - 1}, neurons 0..{'I - 1' if I is None else I - 1}")
    if int(torch.unique(sel, dim=0).shape[0]) != m:
        raise ValueError("neuron_scale: the (layer, neuron) pairs must be unique")
    order = torch.argsort(sel[:, 0] * (int(sel[:, 1].max()) + 1) + sel[:, 1]) if m else torch.arange(0)
    return lambda t, rows: NeuronScale(t[order].contiguous(), sel[order].contiguous(), rows)


class Family(NamedTuple):
    """One line of ``FAMILIES``: what differs between the families of row options.  ``_capture``, ``_patch`` and ``_scale`` below check what they
    share; ``ScoringPass.forward`` and its patch planner walk the same lines."""
    name: str                   # ``_prefill``'s keywords are <name>_capture, <name>_patch, <name>_scale
    capture: str                # forward()'s keywords: the capture's mask, ...
    window: str                 # ... its window, also the ``ReadOuts`` field, ...
    ids: Optional[str]          # ... a further qualifier of the capture, ...
    patch: str                  # ... the patch, ...
    scale: Optional[str]        # ... and the scale, where the family has them
    rows: str                   # the ``ReadOuts`` field of the capture's mask (every other field carries its keyword's name)
    word: str                   # the window's name in a patch record and in messages
    Patch: type
    Scale: Optional[type]
    dims: Callable              # (sizes, the patch's extra) -> ((message word, size or None), ...): the trailing dims of a captured row
    like: str                   # what a patch's values are laid out like
    result: str                 # the result dict's entry (beside <result>_index)
    extra: Optional[str] = None             # a patch record's own field ...
    patch_extra: Optional[Callable] = None  # ... its check (p, values, lo, hi, sizes) -> the checked field ...
    extra_first: bool = False               # ... run in front of the values' check (it sets their width) or behind it (it goes by their shape)
    scale_rules: Optional[Callable] = None  # (q, sizes): the scale's shape rules -> what builds the checked record from (fp32 factors, rows)
    # ---- what ``ScoringPass`` reads -----
    misfit: Optional[Callable] = None       # (got dims, the model's) -> the planner's message for values of another width
    pack: Optional[Callable] = None         # the extra as the C ABI takes it -> (packed or None: everything, whether it selects anything)
    scale_args: Optional[Callable] = None   # the checked scale record -> what ``_prefill`` arms behind the packed rows
    trimmed_last: bool = False              # a capture's slice of the row-trimmed last layer is NaN where no launch writes it

    @property
    def keywords(self) -> tuple:
        return tuple(k for k in (self.capture, self.window, self.ids, self.patch, self.scale) if k)

    @property
    def fields(self) -> tuple:
        """The ``ReadOuts`` fields, in the order of ``keywords`` - and of the tuple the family's ``*_options`` returns."""
        return (self.rows,) + self.keywords[1:]


FAMILIES = (
    Family("stream", "return_stream", "stream_depths", None, "stream_patch", None, "stream_rows", "depths", StreamPatch, None,
           lambda sizes, _: (("H", sizes.get("hidden")),), "a captured stream", "stream",
           misfit=lambda got, want: f"values of width {got[0]}, the residual stream has H = {want[0]}"),
    Family("head", "return_heads", "head_layers", None, "head_patch", "head_scale", "head_rows", "layers", HeadPatch, HeadScale,
           lambda sizes, _: (("n_heads", sizes.get("n_heads")), ("D", sizes.get("head_dim"))), "captured heads", "heads",
           extra="heads", patch_extra=_patch_heads, scale_rules=_head_scale_rules,
           misfit=lambda got, want: f"values of {got[0]} heads x {got[1]}, the model has {want[0]} x {want[1]}",
           pack=lambda heads: (None, True) if heads is None else (head_bits(heads), bool(heads.any())), scale_args=lambda q: (q.scale,)),
    Family("neuron", "return_neurons", "neuron_layers", "neuron_ids", "neuron_patch", "neuron_scale", "neuron_rows", "layers", NeuronPatch, NeuronScale,
           lambda sizes, cols: (("I", sizes.get("n_inter")),) if cols is None else (("m", int(cols.numel())),), "captured neurons", "neurons",
           extra="neurons", patch_extra=_patch_neurons, extra_first=True, scale_rules=_neuron_scale_rules,
           pack=lambda cols: (None, True) if cols is None else (cols.to(torch.int32).contiguous(), bool(cols.numel())),
           scale_args=lambda q: (q.scale, None, None, None) if q.neurons is None else
           (None, q.neurons[:, 0].to(torch.int32).contiguous(), q.neurons[:, 1].to(torch.int32).contiguous(), q.scale), trimmed_last=True),
)
STREAM, HEAD, NEURON = FAMILIES


def _capture(fam: Family, mask, window, ids=None, ids_shape=None, n_layers: Optional[int] = None):
    """A capture with its qualifiers -> (None or a HOST bool mask [B, N], None or (lo, hi) - by default (0, L) where L is known).  A qualifier
    without the capture is refused."""
    if mask is None:
        for name, v in ((fam.window, window), (fam.ids, ids)):
            if v is not None:
                raise ValueError(f"{name}: qualifies {fam.capture} and needs one")
        return None, None
    return (_token_mask(fam.capture, mask, ids_shape),
            _depth_window(fam.window, window, n_layers) if window is not None else (0, n_layers) if n_layers is not None else None)


def _patch(fam: Family, p, ids_shape=None, **sizes):
    """A patch record, checked without the plan: its type, window, values' layout, donor index and row mask, the family's extra where the line
    says -> None or the record with HOST masks and index, a checked window and the values as given."""
    if p is None:
        return None
    if not isinstance(p, fam.Patch):
        raise ValueError(f"{fam.patch}: expected a readouts.{fam.Patch.__name__}, got {type(p).__name__}")
    lo, hi = _depth_window(f"{fam.patch}: {fam.word}", getattr(p, fam.word), sizes.get("n_layers"))
    v, extra = p.values, ()
    if fam.extra_first:
        extra = (fam.patch_extra(p, v, lo, hi, sizes),)
    dims = fam.dims(sizes, *extra or (None,))
    if (not torch.is_tensor(v) or v.dtype != torch.bfloat16 or v.dim() != 2 + len(dims) or int(v.shape[1]) != hi - lo
            or any(size is not None and int(n) != size for n, (_, size) in zip(v.shape[2:], dims))):
        layout = ", ".join(word + ("" if size is None else f" = {size}") for word, size in dims)
        raise ValueError(f"{fam.patch}: values must be a bf16 tensor [n, hi - lo = {hi - lo}, {layout}] laid out like {fam.like}, got {_got(v)}")
    idx = p.index
    if idx is not None:
        if not torch.is_tensor(idx) or idx.is_floating_point() or idx.dtype == torch.bool or idx.dim() != 2 or int(idx.shape[1]) != 2:
            raise ValueError(f"{fam.patch}: index must be an integer tensor [n, 2] of (clip, position) pairs (a donor's {fam.result}_index)")
        idx = idx.detach().to("cpu").to(torch.long).contiguous()
    if fam.patch_extra is not None and not fam.extra_first:
        extra = (fam.patch_extra(p, v, lo, hi, sizes),)
    return fam.Patch(_token_mask(f"{fam.patch}: rows", p.rows, ids_shape), v, (lo, hi), idx, *extra)


def _scale(fam: Family, q, ids_shape=None, **sizes):
    """A scale record, checked: its type, the family's shape rules, the factors as HOST fp32 without a NaN, the optional row mask."""
    if q is None:
        return None
    if not isinstance(q, fam.Scale):
        raise ValueError(f"{fam.scale}: expected a readouts.{fam.Scale.__name__}, got {type(q).__name__}")
    build = fam.scale_rules(q, sizes)
    t = q.scale.detach().to("cpu").to(torch.float32).contiguous()
    if torch.isnan(t).any():
        raise ValueError(f"{fam.scale}: scale[{', '.join(str(i) for i in torch.isnan(t).nonzero()[0].tolist())}] is NaN")
    return build(t, None if q.rows is None else _token_mask(f"{fam.scale}: rows", q.rows, ids_shape))


def stream_options(return_stream=None, stream_depths=None, stream_patch=None, ids_shape=None, n_layers: Optional[int] = None):
    """``return_stream`` / ``stream_depths`` / ``stream_patch`` -> (None or a HOST bool mask [B, N], None or (lo, hi), None or a ``StreamPatch``
    whose ``rows`` is such a mask, whose ``depths`` is a checked pair and whose ``index`` is a HOST int64 [n, 2]).  Depth d, 0 <= d < L, is the
    stream layer d consumes; ``stream_depths`` defaults to (0, L) and needs ``return_stream``.  The values' dtype and the shapes that do not need
    the plan are checked here; the counts and the (clip, position) pairs where the plan is (``ScoringPass._stream_rows``)."""
    return (*_capture(STREAM, return_stream, stream_depths, None, ids_shape, n_layers), _patch(STREAM, stream_patch, ids_shape, n_layers=n_layers))


def head_options(return_heads=None, head_layers=None, head_patch=None, head_scale=None, ids_shape=None, n_layers: Optional[int] = None,
                 n_heads: Optional[int] = None, head_dim: Optional[int] = None):
    """``return_heads`` / ``head_layers`` / ``head_patch`` / ``head_scale`` -> (None or a HOST bool mask [B, N], None or (lo, hi), None or a
    ``HeadPatch`` whose ``rows`` is such a mask, whose ``layers`` is a checked pair, whose ``index`` is a HOST int64 [n, 2] and whose ``heads`` is a
    HOST bool [hi - lo, n_heads] or None, None or a ``HeadScale`` whose ``scale`` is a HOST fp32 [L, n_heads] and whose ``rows`` is such a mask or
    None).  Layer l, 0 <= l < L, names the input of that layer's ``wo``; ``head_layers`` defaults to (0, L) and needs ``return_heads``.  Shapes,
    dtypes and windows are checked here (those that need the model's sizes only when they are given); counts and (clip, position) pairs where the
    plan is (``ScoringPass._head_patch_plan``)."""
    if (return_heads is not None or head_patch is not None or head_scale is not None) and n_heads is not None and n_heads > MAX_HEADS:
        raise ValueError(f"return_heads / head_patch / head_scale: the model has {n_heads} query heads, a head mask holds at most {MAX_HEADS}")
    sizes = dict(n_layers=n_layers, n_heads=n_heads, head_dim=head_dim)
    return (*_capture(HEAD, return_heads, head_layers, None, ids_shape, n_layers), _patch(HEAD, head_patch, ids_shape, **sizes), _scale(HEAD, head_scale, ids_shape, **sizes))


def neuron_options(return_neurons=None, neuron_layers=None, neuron_ids=None, neuron_patch=None, neuron_scale=None, ids_shape=None,
                   n_layers: Optional[int] = None, n_inter: Optional[int] = None):
    """``return_neurons`` / ``neuron_layers`` / ``neuron_ids`` / ``neuron_patch`` / ``neuron_scale`` -> (None or a HOST bool mask [B, N], None or
    (lo, hi), None or a HOST int64 [m], None or a ``NeuronPatch`` whose ``rows`` is such a mask, whose ``layers`` is a checked pair, whose ``index``
    is a HOST int64 [n, 2] and whose ``neurons`` is a HOST int64 [m] or None, None or a ``NeuronScale`` whose ``scale`` is a HOST fp32 [L] (or
    [m], beside ``neurons``: a HOST int64 [m, 2] sorted by (layer, neuron)) and whose ``rows`` is such a mask or None).  Layer l, 0 <= l < L, names
    the input of that layer's ``w2``; ``neuron_layers`` defaults to (0, L); it and ``neuron_ids`` need ``return_neurons``.  Shapes, dtypes, windows
    and lists are checked here (those that need the model's sizes only when they are given); counts and (clip, position) pairs where the plan is
    (``ScoringPass._neuron_patch_plan``)."""
    rows, window = _capture(NEURON, return_neurons, neuron_layers, neuron_ids, ids_shape, n_layers)
    ids = None if rows is None or neuron_ids is None else _neuron_ids("neuron_ids", neuron_ids, n_inter)
    sizes = dict(n_layers=n_layers, n_inter=n_inter)
    return rows, window, ids, _patch(NEURON, neuron_patch, ids_shape, **sizes), _scale(NEURON, neuron_scale, ids_shape, **sizes)


_NAN = float("nan")
# every result laid out per label position, [B (N - 1)] + width: name in the result dict, the ``ReadOuts`` member that switches it on and gives
# its trailing width (None: always there), dtype, fill wherever the row is not an answer row
ROW_FIELDS = (("logit", None, torch.long, -1),
              ("logprob", "logprobs", torch.float32, _NAN),
              ("cand_logprob", "cand", torch.float32, _NAN),
              ("top_ids", "topk", torch.long, -1),
              ("top_logprob", "topk", torch.float32, _NAN))


@dataclass(frozen=True, eq=False)
class ReadOuts:
    """What one call asked for.  ``parse`` gives the checked form the model works with (``cand`` an int64 tensor, ``topk`` an int or None);
    the loops that only pass the options on (``score_clips_dp``, ``batched``) fill ``logprobs`` / ``cand`` / ``topk`` in as they got them."""
    logprobs: bool = False
    cand: Optional[torch.Tensor] = None         # candidate_ids
    topk: Optional[int] = None                  # top_logprobs=k
    score_attention: bool = False               # (return_token_attention implies it)
    segments: Optional[torch.Tensor] = None     # the user's attention_segments table; None: prompts.attention_segments
    token_attention: bool = False
    score_values: bool = False                  # return_score_values: what the score row takes from every segment, per head (implies score_attention; forward and
                                                # forward_shared_prefix only)
    key_drop: Optional[torch.Tensor] = None     # host bool [B, N]: tokens hidden, as keys, from every row of their clip (forward; generate* check theirs with key_drop_mask)
    key_drop_rows: Optional[torch.Tensor] = None    # host bool [B, N]: ... from these query rows only (None: every row)
    key_drop_layers: Optional[tuple] = None         # (lo, hi): ... in the layers lo <= l < hi only (None: every layer)
    depth_lens: bool = False                    # return_depth_lens: the score row and the token row after every layer (forward only)
    # (the neuron options stand in front of the stream and head ones: tests/test_head_patch_cpu.py pins that no field follows head_scale)
    neuron_rows: Optional[torch.Tensor] = None      # return_neurons: host bool [B, N], the tokens whose MLP neurons - the row w2 consumes - are captured (forward only)
    neuron_layers: Optional[tuple] = None           # (lo, hi): ... at the layers lo <= l < hi (None with neuron_rows None)
    neuron_ids: Optional[torch.Tensor] = None       # host int64 [m]: ... those neurons only (None: all I of them)
    neuron_patch: Optional[NeuronPatch] = None      # neurons overwritten between the SwiGLU and w2 of the layers of its window (forward only)
    neuron_scale: Optional[NeuronScale] = None      # neurons multiplied by a factor per layer or per (layer, neuron) (forward only)
    stream_rows: Optional[torch.Tensor] = None      # return_stream: host bool [B, N], the tokens whose residual-stream rows are captured (forward only)
    stream_depths: Optional[tuple] = None           # (lo, hi): ... at the depths lo <= d < hi (None with stream_rows None)
    stream_patch: Optional[StreamPatch] = None      # rows of the stream overwritten in front of the layers of its window (forward only)
    head_rows: Optional[torch.Tensor] = None        # return_heads: host bool [B, N], the tokens whose per-head attention outputs are captured (forward only)
    head_layers: Optional[tuple] = None             # (lo, hi): ... at the layers lo <= l < hi (None with head_rows None)
    head_patch: Optional[HeadPatch] = None          # head outputs overwritten between the attention and wo of the layers of its window (forward only)
    head_scale: Optional[HeadScale] = None          # head outputs multiplied by a factor per (layer, head) (forward only)
    # The attention flow map (return_segment_attention / return_row_attention; forward only): None or an ``AttentionMap``.  NOT a dataclass field - the
    # field list is pinned from both ends (tests/test_head_patch_cpu.py: nothing follows head_scale; tests/test_option_parse_cpu.py: the families start at
    # field 11) - so it is a plain attribute that ``parse`` sets on the record it returns; the constructor leaves it None.
    attention_map = None

    def with_(self, **changes) -> "ReadOuts":
        """``dataclasses.replace`` that keeps ``attention_map``: ``replace`` rebuilds the record from its FIELDS alone and would drop it."""
        ro = replace(self, **changes)
        object.__setattr__(ro, "attention_map", self.attention_map)
        return ro

    @classmethod
    def parse(cls, vocab: int, labels="given", *, return_logprobs: bool = False, candidate_ids=None, top_logprobs: Optional[int] = None,
              return_score_attention: bool = False, attention_segments=None, return_token_attention: bool = False, key_drop=None,
              ids_shape=None, key_drop_rows=None, key_drop_layers=None, n_layers: Optional[int] = None, return_depth_lens: bool = False,
              return_stream=None, stream_depths=None, stream_patch=None, return_heads=None, head_layers=None, head_patch=None, head_scale=None,
              n_heads: Optional[int] = None, head_dim: Optional[int] = None, return_neurons=None, neuron_layers=None, neuron_ids=None, neuron_patch=None,
              neuron_scale=None, n_inter: Optional[int] = None, return_score_values: bool = False, return_segment_attention: bool = False,
              return_row_attention=None) -> "ReadOuts":
        """The record of a call's public keyword arguments, checked.  ``labels=None`` (``forward`` without labels) refuses candidates and top-k;
        the shared-prefix and generate entry points leave the default.  A user segment table is checked where its bins are counted
        (``n_segments``: it needs the shape of ``input_ids``).  Every check that needs no plan, in the order a call meets them: the clip count of
        ``return_score_values``, the key-drop qualifiers, ``key_drop``, the attention map's window and its refusal of ``key_drop``, the stream, head
        and neuron families, ``candidate_ids``, ``top_logprobs``, the clip count of ``return_depth_lens``."""
        att = bool(return_score_attention or return_token_attention or return_score_values)
        if return_score_values and ids_shape is not None and int(ids_shape[0]) > MAX_PROBE_ROWS:
            raise ValueError(f"return_score_values: at most {MAX_PROBE_ROWS} clips per pass, got {int(ids_shape[0])}")
        rows, window = key_drop_qualifiers(key_drop, key_drop_rows, key_drop_layers, ids_shape, n_layers)
        mask = key_drop_mask(key_drop, ids_shape, att)
        amap = attention_map(return_segment_attention, return_row_attention, key_drop, n_layers, ids_shape)
        stream = stream_options(return_stream, stream_depths, stream_patch, ids_shape, n_layers)
        heads = head_options(return_heads, head_layers, head_patch, head_scale, ids_shape, n_layers, n_heads, head_dim)
        neurons = neuron_options(return_neurons, neuron_layers, neuron_ids, neuron_patch, neuron_scale, ids_shape, n_layers, n_inter)
        cand = candidates(candidate_ids, labels)
        k = top_logprobs_k(top_logprobs, vocab, labels)
        if return_depth_lens and ids_shape is not None and int(ids_shape[0]) > MAX_LENS_ROWS:
            raise ValueError(f"return_depth_lens: at most {MAX_LENS_ROWS} clips per pass, got {int(ids_shape[0])}")
        ro = cls(bool(return_logprobs), cand, k or None, att, attention_segments if att or amap else None, bool(return_token_attention), bool(return_score_values),
                 mask, rows, window, bool(return_depth_lens), *neurons, *stream, *heads)
        object.__setattr__(ro, "attention_map", amap)      # (frozen: the record is not rebound afterwards)
        return ro

    @property
    def touches_stream(self) -> bool:
        """A capture or a patch of the residual stream, or a capture, patch or scale of head outputs or of MLP neurons: such a call runs eagerly
        under graph replay, as a masked call does."""
        return any(getattr(self, f) is not None for fam in FAMILIES for f in (fam.rows, fam.patch, fam.scale) if f)

    @property
    def runs_eagerly(self) -> bool:
        """Under graph replay: a masked call, a call that touches the stream, a call that returns the score row's value vectors and a call that returns
        the attention map run eagerly and capture nothing; every other call keeps the graph key it always had (``key_tail``)."""
        return self.key_drop is not None or self.touches_stream or self.score_values or self.attention_map is not None

    @property
    def wants_labels(self) -> bool:
        """The lm-head read-outs, which need the pass's checked answer labels."""
        return self.logprobs or self.cand is not None or bool(self.topk)

    def n_segments(self, ids_shape) -> int:
        """S of a user segment table (its largest id + 1; the table is checked first), 0 for the default table.  Reads the table's maximum
        back from wherever it lives: never called inside a captured pass."""
        t = self.segments
        if t is None:
            return 0
        if not torch.is_tensor(t) or t.is_floating_point() or t.dtype == torch.bool or tuple(t.shape) != tuple(ids_shape):
            raise ValueError(f"attention_segments: expected an integer tensor shaped like input_ids {tuple(ids_shape)}")
        return int(t.max()) + 1

    def map_segments(self, ids_shape, default: int) -> int:
        """S of the attention map: a user table's bin count, else ``default`` (the default table's, which the caller has from its plan) - checked
        against the most bins a pass takes."""
        S = self.n_segments(ids_shape) if self.segments is not None else int(default)
        if not 1 <= S <= MAX_ATTN_SEGMENTS:
            raise ValueError(f"return_segment_attention / return_row_attention: {S} segments, outside 1..{MAX_ATTN_SEGMENTS}")
        return S

    def key_tail(self, ids_shape, n_seg: Optional[int] = None) -> tuple:
        """What the record appends to a graph's host key (``n_seg``: ``n_segments`` when the caller has it already).  Nothing for an option
        that is off: the keys of passes without it are those they always were.  The candidates' VALUES and a user segment table are graph
        INPUT, not key; the candidates' number is in the key with the device inputs' shapes.  k, a user table's bin count (the default
        table follows from the ids, which are in the key) and ld_tok = N are output shapes: another value is another graph.  ``key_drop`` and
        the stream, head and neuron options add nothing: such calls are never captured - nor is one with ``score_values`` or with the attention map."""
        S = (self.n_segments(ids_shape) if n_seg is None else n_seg) if self.score_attention else 0
        on = ((self.logprobs, "logprobs"), (self.cand is not None, "candidates"), (self.topk is not None, ("top_logprobs", self.topk)),
              (self.score_attention, ("score_attention", S)), (self.token_attention, ("score_attention_tokens", int(ids_shape[1]))),
              (self.depth_lens, "depth_lens"))
        return tuple(element for yes, element in on if yes)

    def row_fields(self):
        """[(name, trailing shape, dtype, fill)] of the ``ROW_FIELDS`` this record switches on."""
        n_cand = 0 if self.cand is None else int(self.cand.numel() if torch.is_tensor(self.cand) else len(self.cand))
        width = {None: (), "logprobs": () if self.logprobs else None, "cand": None if self.cand is None else (n_cand,),
                 "topk": None if self.topk is None else (int(self.topk),)}
        return [(name, width[m], dt, fill) for name, m, dt, fill in ROW_FIELDS if width[m] is not None]


def forward_kwargs(r: ReadOuts) -> dict:
    """The record as keyword arguments of ``forward``.  An option that is off is NOT passed: callers hand these to any object with
    ``forward``'s call form, which need not know the options it is not asked for."""
    kw = dict(return_logprobs=r.logprobs or None, candidate_ids=r.cand, top_logprobs=r.topk, return_score_attention=r.score_attention or None,
              attention_segments=r.segments, return_token_attention=r.token_attention or None, return_score_values=r.score_values or None, key_drop=r.key_drop,
              key_drop_rows=r.key_drop_rows, key_drop_layers=r.key_drop_layers, return_depth_lens=r.depth_lens or None,
              return_segment_attention=(r.attention_map is not None and r.attention_map.segments) or None,
              return_row_attention=None if r.attention_map is None else r.attention_map.rows,
              **{k: getattr(r, f) for fam in FAMILIES for k, f in zip(fam.keywords, fam.fields)})
    return {k: v for k, v in kw.items() if v is not None}


def ce_loss(logprob: torch.Tensor, labels: torch.Tensor, to_device=None) -> torch.Tensor:
    """The reference's ``CrossEntropyLoss()``: the mean of ``-logprob`` over the non-ignored ``labels`` (both [B (N - 1)]; labels on the
    host), in fp64, rounded once; NaN when there are none.  ``to_device``: how the host index list goes up (default ``.to``)."""
    scored = (labels.reshape(-1) != -100).nonzero().flatten()      # (host: no sync)
    if not scored.numel():
        return torch.full((), _NAN, dtype=torch.float32, device=logprob.device)
    scored = to_device(scored) if to_device is not None else scored.to(logprob.device)
    return (-logprob.index_select(0, scored)).double().mean().float()
