"""Host-side generators of the row-selective key-drop tests (no GPU; torch and numpy only): the row patterns over a sequence, the key
census of tests/key_drop_reference.py under a (rows, keys) knock-out, the float64 / eager-bf16 masked attention with the same visibility,
and the model-level reference - the oracle's own functions composed layer by layer under a per-layer additive mask.

Visibility of key j to query row r of a packed sequence (no cached keys): causal & ~(row_sel[r] & drop[j]).  Everything else - Q = 0, the
one-hot V, BIG_K in the dropped keys' K rows, the phases and the weights - is ``key_drop_reference.census``."""
import numpy as np
import torch

import key_drop_reference as R
from attention_exact_reference import BF, ExactData, census_bits, census_weight

from oracle import oracle as O

ROW_PATTERNS = ("none", "all", "one", "wave", "group", "odd", "last")
KEY_PATTERNS = "abcdf"


def row_sets(case, pattern):
    """-> [bool array over the query rows of every sequence] (a packed case: row i is position i).  none; all; the single row len - 4; rows
    20..40, which cross a 32-row wave; rows 120..136, which cross a 128-row workgroup; every other row; the rows of the ragged last wave."""
    assert not any(case.offs), "the row-selective form is the packed prefill's"
    out = []
    for n in case.cnts:
        m = np.zeros(n, dtype=bool)
        if pattern == "none":
            idx = []
        elif pattern == "all":
            idx = range(n)
        elif pattern == "one":
            idx = [n - 4]
        elif pattern == "wave":
            idx = range(20, 41)
        elif pattern == "group":
            idx = range(120, 137)
        elif pattern == "odd":
            idx = range(1, n, 2)
        elif pattern == "last":
            idx = range(32 * ((n - 1) // 32), n)
        else:
            raise ValueError(pattern)
        for i in idx:
            if 0 <= i < n:
                m[i] = True
        out.append(m)
    return out


def visible_sets(case, s, drop, rows):
    """bool [cnt, tot]: key j is visible to row r of sequence s under the knock-out (rows, drop)."""
    n, tot = case.cnts[s], case.tot[s]
    causal = np.arange(tot)[None, :] <= np.arange(n)[:, None]
    return causal & ~(rows[:, None] & drop[None, :])


def census(case, drops, rows):
    """``key_drop_reference.census`` (the same inputs: the seed, Q, K with BIG_K, V do not depend on the rows) with the expectation of the
    (rows, keys) visibility."""
    base = R.census(case, drops)
    exp = []
    for s, (n, t) in enumerate(zip(case.cnts, case.tot)):
        vis = visible_sets(case, s, drops[s], rows[s])
        l = vis.sum(1)
        e = []
        for kh in range(case.hk):
            onehot = np.zeros((t, case.D), dtype=np.int64)
            onehot[np.arange(t), (np.arange(t) + int(case.phase[s, kh])) % case.D] = census_weight(kh)
            e.append(census_bits(vis.astype(np.int64) @ onehot, l, "prefill"))
        exp.append(torch.from_numpy(np.repeat(np.stack(e, 1), case.g, axis=1)))
    return ExactData(case, base.q, base.k, base.v, torch.cat(exp))


def masked_attention(q, k, v, drop, rows, post_div, dtype):
    """ONE packed sequence, q [n, h, D], k / v [n, hk, D]: causal attention with the edges (rows, drop) cut, as the reference cuts them (an
    additive finfo.min).  float64 -> truth; bf16 -> the reference's eager rounding points.  ``key_drop_reference.masked_attention`` with the
    (rows, keys) visibility.  -> [n, h, D] in `dtype`."""
    n, h = q.shape[0], q.shape[1]
    rep = h // k.shape[1]
    qq = q.transpose(0, 1).to(dtype)
    kk = k.transpose(0, 1).repeat_interleave(rep, 0).to(dtype)
    vv = v.transpose(0, 1).repeat_interleave(rep, 0).to(dtype)
    s = (qq @ kk.transpose(1, 2)) / post_div
    hide = torch.arange(k.shape[0])[None, :] > torch.arange(n)[:, None]
    hide = hide | (torch.from_numpy(np.asarray(rows))[:, None] & torch.from_numpy(np.asarray(drop))[None, :])
    s = s.masked_fill(hide[None], torch.finfo(dtype).min)
    p = torch.softmax(s, -1, dtype=torch.float32).to(BF) if dtype == BF else torch.softmax(s, -1)
    o = p @ vv
    o = o.masked_fill(hide.all(1)[None, :, None], 0)
    return o.transpose(0, 1)


def blocked_mask(attention_mask, drop, rows, dtype):
    """The additive mask [B, 1, N, N] of a layer inside the window: ``oracle.additive_mask`` plus finfo.min at every (row r, key j) with
    rows[b, r] and drop[b, j].  rows None: every row."""
    b, n = attention_mask.shape
    rows = torch.ones(b, n, dtype=torch.bool) if rows is None else rows.bool()
    cut = (rows[:, :, None] & drop.bool()[:, None, :])[:, None]
    extra = torch.zeros(b, 1, n, n, dtype=dtype).masked_fill(cut, torch.finfo(dtype).min)
    return extra + O.additive_mask(attention_mask, n, 0, dtype)


def composed_forward(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, labels, motion_feature, img_context_token_id, stage=2, drop=None,
                     rows=None, window=None):
    """``oracle.forward_eval`` with the LLM run layer by layer: ``oracle.llm_layer`` under ``blocked_mask`` in the layers lo <= l < hi and under
    ``oracle.additive_mask`` in the others, then the final norm, the score head on [:, -4] and the lm-head.  drop None: the plain pass.
    window None: every layer.  -> {'label', 'logit', 'logits', 'score1' (stage 2)}."""
    flags = image_flags.squeeze(-1)
    vit = O.extract_feature(sd, cfg, pixel_values)[flags == 1]
    motion = O.projector(sd, "motion_mlp", motion_feature.view(input_ids.shape[0], -1))
    x = O.scatter_embeds(sd, input_ids, img_context_token_id, vit, motion)
    b, n, _ = x.shape
    L = cfg.llm_config.num_hidden_layers
    lo, hi = (0, L) if window is None else window
    pos = torch.arange(n, dtype=torch.long).unsqueeze(0)
    plain = O.additive_mask(attention_mask, n, 0, x.dtype)
    cut = plain if drop is None else blocked_mask(attention_mask, drop, rows, x.dtype)
    for i in range(L):
        x, _ = O.llm_layer(sd, cfg, i, x, cut if lo <= i < hi else plain, pos)
    hidden = O.rms_norm_cast_then_scale(x, sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps)
    logits = O.lm_logits(sd, hidden)
    out = {"label": labels[..., 1:].contiguous().view(-1), "logit": torch.argmax(logits[..., :-1, :].contiguous().view(-1, logits.shape[-1]), dim=1),
           "logits": logits}
    if stage == 2:
        out["score1"] = O.score_head(sd, cfg, hidden[:, -4, :]).squeeze(1)
    return out
