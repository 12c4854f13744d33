"""Host-side reference of head knock-out and head patching (no GPU; torch only): ``depth_lens_reference.composed_states`` run under an
``oracle.LLM_LINEAR_HOOK`` that does to the input of ``wo`` (``o_proj`` for the Llama family) of the armed layers what the product does to its
attention output - scale, then patch, then capture - which is what a forward pre-hook on ``layers[l].attention.wo`` does in the reference.  The
hook is restored to None afterwards.  The read-outs of the modified pass come from ``depth_lens_reference.lens``."""
import torch
import torch.nn.functional as F

import depth_lens_reference as DL
from stream_patch_reference import selected

from oracle import oracle as O


def head_masks(heads, n_layers, n_heads):
    """None | bool [n_heads] | bool [n_layers, n_heads] -> bool [n_layers, n_heads]."""
    if heads is None:
        return torch.ones(n_layers, n_heads, dtype=torch.bool)
    return heads.bool().expand(n_layers, n_heads)


def composed_states(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, motion_feature, img_context_token_id, scale=None, scale_rows=None,
                    patches=(), capture=None, drop=None, rows=None, window=None):
    """-> ([L + 1 tensors [B, N, H]] as ``depth_lens_reference.composed_states`` gives them, None or the capture [n, hi - lo, n_heads, D]).
    scale: float [L, n_heads] - over the rows ``scale_rows`` selects (bool [B, N]; None: every row) head h of layer l becomes ``(x.float() *
    s).to(x.dtype)``; an entry that is exactly 1 leaves its head untouched.  patches: an iterable of (mask [B, N], values [n, hi - lo, n_heads, D],
    (lo, hi), heads: None | bool [n_heads] | bool [hi - lo, n_heads]) - values laid out like a capture with that mask and those layers
    (``stream_patch_reference.selected`` gives the order of n).  capture: (mask [B, N], (lo, hi)).  Inside a layer: scale, patch, capture.  With
    none of the three: ``depth_lens_reference.composed_states``, bit for bit.  drop / rows / window: that function's knock-out."""
    l = cfg.llm_config
    L, nh, d = l.num_hidden_layers, l.num_attention_heads, l.head_dim
    patches = [(selected(mask, attention_mask), values, (int(lo), int(hi)), head_masks(heads, int(hi) - int(lo), nh)) for mask, values, (lo, hi), heads in patches]
    for at, values, (lo, hi), _ in patches:
        assert 0 <= lo <= hi <= L and tuple(values.shape) == (at.shape[0], hi - lo, nh, d), (tuple(values.shape), at.shape[0], lo, hi)
    cap_at = cap = None
    if capture is not None:
        cap_at, (c_lo, c_hi) = selected(capture[0], attention_mask), capture[1]
        cap = [None] * (c_hi - c_lo)
    srows = None if scale_rows is None else scale_rows.bool()

    def hook(x, w, layer, name):
        if name in ("wo", "o_proj"):
            b, n, _ = x.shape
            xh = x.reshape(b, n, nh, d).clone()
            if scale is not None:
                for h in range(nh):
                    s = float(scale[layer, h])
                    if s != 1.0:                                                              # exactly 1: the head is not touched
                        new = (xh[:, :, h].float() * s).to(x.dtype)
                        xh[:, :, h] = new if srows is None else torch.where(srows[:, :n, None], new, xh[:, :, h])
            for at, values, (lo, hi), heads in patches:
                if lo <= layer < hi and at.shape[0]:
                    for h in heads[layer - lo].nonzero().flatten().tolist():
                        xh[at[:, 0], at[:, 1], h] = values[:, layer - lo, h].to(x.dtype)      # the pre-hook's assignment: a copy, no arithmetic
            if cap is not None and c_lo <= layer < c_hi:
                cap[layer - c_lo] = xh[cap_at[:, 0], cap_at[:, 1]].clone()
            x = xh.reshape(b, n, nh * d)
        return F.linear(x, w)

    assert O.LLM_LINEAR_HOOK is None
    O.LLM_LINEAR_HOOK = hook
    try:
        states = DL.composed_states(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, motion_feature, img_context_token_id, drop, rows, window)
    finally:
        O.LLM_LINEAR_HOOK = None
    if cap is not None:
        cap = torch.stack(cap, 1) if cap else states[0].new_zeros(cap_at.shape[0], 0, nh, d)
    return states, cap


def lens(sd, cfg, states, attention_mask, labels, stage=2, candidate_ids=None):
    """The read-outs of the (modified) pass: ``depth_lens_reference.lens`` on its states - column L is the pass's own score / token / log-probs."""
    return DL.lens(sd, cfg, states, attention_mask, labels, stage, candidate_ids)
