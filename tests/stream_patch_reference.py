"""Host-side reference of activation patching (no GPU; torch only): the residual stream of a batch composed from the oracle's own layer function
exactly as ``depth_lens_reference.composed_states`` composes it, with the assignment ``x[b, pos] = value`` in front of layer d for every d of a
patch's window - what a forward pre-hook on ``language_model.model.layers[d]`` does in the reference - optionally under a knock-out's blocked
mask; the capture in the product's layout; and the read-outs of the patched pass through ``depth_lens_reference.lens``."""
import torch

import depth_lens_reference as DL
import key_drop_rows_reference as RR

from oracle import oracle as O


def selected(mask, attention_mask):
    """int64 [n, 2]: the (clip, position) pairs a mask [B, N] selects among the un-padded tokens, clip-major and position-ascending - the order of
    the product's ``stream_index`` (without the dead tail, which the reference runs: cut the mask to the tokens the product runs first)."""
    return (mask.bool() & attention_mask.bool()).nonzero().to(torch.long)


def composed_states(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, motion_feature, img_context_token_id, patches=(), drop=None, rows=None,
                    window=None):
    """-> [L + 1 tensors [B, N, H]]: entry d < L is the stream AS LAYER d CONSUMES IT (after the patches of depth d), entry L what the final norm
    consumes.  patches: an iterable of (mask [B, N], values [n, hi - lo, H], (lo, hi)) - values laid out like a capture with that mask and those
    depths (``selected`` gives the order of n).  Without patches: ``depth_lens_reference.composed_states``, bit for bit.  drop / rows / window:
    that function's knock-out."""
    flags = image_flags.squeeze(-1)
    vit = O.extract_feature(sd, cfg, pixel_values)[flags == 1]
    motion = O.projector(sd, "motion_mlp", motion_feature.view(input_ids.shape[0], -1))
    x = O.scatter_embeds(sd, input_ids, img_context_token_id, vit, motion)
    n = x.shape[1]
    L = cfg.llm_config.num_hidden_layers
    lo_k, hi_k = (0, L) if window is None else window
    pos = torch.arange(n, dtype=torch.long).unsqueeze(0)
    plain = O.additive_mask(attention_mask, n, 0, x.dtype)
    cut = plain if drop is None else RR.blocked_mask(attention_mask, drop, rows, x.dtype)
    patches = [(selected(mask, attention_mask), values, (int(lo), int(hi))) for mask, values, (lo, hi) in patches]
    for at, values, (lo, hi) in patches:
        assert 0 <= lo <= hi <= L and tuple(values.shape) == (at.shape[0], hi - lo, x.shape[-1]), (tuple(values.shape), at.shape[0], lo, hi)
    states = []
    for i in range(L):
        for at, values, (lo, hi) in patches:
            if lo <= i < hi and at.shape[0]:
                x = x.clone()
                x[at[:, 0], at[:, 1]] = values[:, i - lo].to(x.dtype)            # the pre-hook's assignment: a copy, no arithmetic
        states.append(x)
        x, _ = O.llm_layer(sd, cfg, i, x, cut if lo_k <= i < hi_k else plain, pos)
    states.append(x)
    return states


def capture(states, mask, attention_mask, depths):
    """The product's ``stream`` / ``stream_index`` of such states: ([n, hi - lo, H], int64 [n, 2])."""
    lo, hi = depths
    at = selected(mask, attention_mask)
    H = states[0].shape[-1]
    rows = [states[d][at[:, 0], at[:, 1]] for d in range(lo, hi)]
    return (torch.stack(rows, 1) if rows else states[0].new_zeros(at.shape[0], 0, H)), at


def lens(sd, cfg, states, attention_mask, labels, stage=2, candidate_ids=None):
    """The read-outs of the (patched) pass: ``depth_lens_reference.lens`` on its states - column L is the pass's own score / token / log-probs."""
    return DL.lens(sd, cfg, states, attention_mask, labels, stage, candidate_ids)
