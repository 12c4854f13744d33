"""Host-side reference of MLP neuron knock-out and neuron patching (no GPU; torch only): ``depth_lens_reference.composed_states`` run under an
``oracle.LLM_LINEAR_HOOK`` that does to the input of ``w2`` (``down_proj`` for the Llama family) of the armed layers what the product does to the
SwiGLU output - scale, then patch, then capture - which is what a forward pre-hook on ``layers[l].feed_forward.w2`` does in the reference.  The hook
is restored to None afterwards.  The read-outs of the modified pass come from ``depth_lens_reference.lens``.  The oracle runs every layer for every
row: it has no row-trimmed last layer, so its capture of layer L - 1 holds a value for every row."""
import torch
import torch.nn.functional as F

import depth_lens_reference as DL
from stream_patch_reference import selected

from oracle import oracle as O


def composed_states(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, motion_feature, img_context_token_id, layer_scale=None, sel=None,
                    sel_factors=None, scale_rows=None, patches=(), capture=None, drop=None, rows=None, window=None):
    """-> ([L + 1 tensors [B, N, H]] as ``depth_lens_reference.composed_states`` gives them, None or the capture [n, hi - lo, I or m]).
    The scale, over the rows ``scale_rows`` selects (bool [B, N]; None: every row): dense - layer_scale: float [L], every neuron of layer l becomes
    ``(x.float() * s).to(x.dtype)``; sparse - sel: long [m, 2] of (layer, neuron) with sel_factors: float [m]; a factor that is exactly 1 leaves its
    neurons untouched.  patches: an iterable of (mask [B, N], values [n, hi - lo, I or m], (lo, hi), neurons: None | long [m]) - values laid out like
    a capture with that mask, those layers and those neurons (``stream_patch_reference.selected`` gives the order of n).  capture: (mask [B, N],
    (lo, hi), neurons: None | long [m]).  Inside a layer: scale, patch, capture.  With none of the three: ``depth_lens_reference.composed_states``,
    bit for bit.  drop / rows / window: that function's knock-out."""
    l = cfg.llm_config
    L, I = l.num_hidden_layers, l.intermediate_size
    every = torch.arange(I)
    patches = [(selected(mask, attention_mask), values, (int(lo), int(hi)), every if cols is None else cols.long()) for mask, values, (lo, hi), cols in patches]
    for at, values, (lo, hi), cols in patches:
        assert 0 <= lo <= hi <= L and tuple(values.shape) == (at.shape[0], hi - lo, cols.numel()), (tuple(values.shape), at.shape[0], lo, hi)
    cap_at = cap = cap_cols = None
    if capture is not None:
        cap_at, (c_lo, c_hi) = selected(capture[0], attention_mask), capture[1]
        cap_cols = every if capture[2] is None else capture[2].long()
        cap = [None] * (c_hi - c_lo)
    srows = None if scale_rows is None else scale_rows.bool()

    def scaled(x, cols, s, n):
        new = (x[..., cols].float() * s).to(x.dtype)
        x[..., cols] = new if srows is None else torch.where(srows[:, :n, None], new, x[..., cols])

    def hook(x, w, layer, name):
        if name in ("w2", "down_proj"):
            n = x.shape[1]
            x = x.clone()
            if layer_scale is not None and float(layer_scale[layer]) != 1.0:                   # exactly 1: the layer is not touched
                scaled(x, every, float(layer_scale[layer]), n)
            if sel is not None:
                for (sl, j), s in zip(sel.tolist(), sel_factors.tolist()):
                    if sl == layer and s != 1.0:
                        scaled(x, torch.tensor([j]), s, n)
            for at, values, (lo, hi), cols in patches:
                if lo <= layer < hi and at.shape[0] and cols.numel():
                    x[at[:, 0][:, None], at[:, 1][:, None], cols[None]] = values[:, layer - lo].to(x.dtype)      # the pre-hook's assignment: a copy
            if cap is not None and c_lo <= layer < c_hi:
                cap[layer - c_lo] = x[cap_at[:, 0], cap_at[:, 1]][:, cap_cols].clone()
        return F.linear(x, w)

    assert O.LLM_LINEAR_HOOK is None
    O.LLM_LINEAR_HOOK = hook
    try:
        states = DL.composed_states(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, motion_feature, img_context_token_id, drop, rows, window)
    finally:
        O.LLM_LINEAR_HOOK = None
    if cap is not None:
        cap = torch.stack(cap, 1) if cap else states[0].new_zeros(cap_at.shape[0], 0, cap_cols.numel())
    return states, cap


def lens(sd, cfg, states, attention_mask, labels, stage=2, candidate_ids=None):
    """The read-outs of the (modified) pass: ``depth_lens_reference.lens`` on its states - column L is the pass's own score / token / log-probs."""
    return DL.lens(sd, cfg, states, attention_mask, labels, stage, candidate_ids)
