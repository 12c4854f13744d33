"""Host-side reference of the depth lens (no GPU; torch only): the residual stream of a clip after every layer, composed from the oracle's own
layer function the way ``key_drop_rows_reference.composed_forward`` composes its pass - depth L un-normed is not in ``oracle.llm_forward``'s
``states`` - optionally under the blocked mask of a knock-out, and the lens read-outs on two rows of it: the oracle's final norm, its score
head under the reference's NaN guard over the batch's score rows of that depth, its lm-head."""
import torch

import key_drop_rows_reference as RR

from oracle import oracle as O


def token_row(labels_row):
    """The position whose logits predict the clip's first answer token (labels laid out like input_ids), or None."""
    at = (labels_row[1:] != -100).nonzero().flatten()
    return int(at[0]) if at.numel() else None


def composed_states(sd, cfg, pixel_values, input_ids, attention_mask, image_flags, motion_feature, img_context_token_id, drop=None, rows=None,
                    window=None):
    """-> [L + 1 tensors [B, N, H]]: the residual stream after d layers, d = 0 the embedding, d = L what the final norm consumes.
    drop / rows / window: ``composed_forward``'s knock-out (drop None: the plain pass).  The arithmetic runs in the dtype of ``sd``."""
    flags = image_flags.squeeze(-1)
    vit = O.extract_feature(sd, cfg, pixel_values)[flags == 1]
    motion = O.projector(sd, "motion_mlp", motion_feature.view(input_ids.shape[0], -1))
    x = O.scatter_embeds(sd, input_ids, img_context_token_id, vit, motion)
    n = x.shape[1]
    L = cfg.llm_config.num_hidden_layers
    lo, hi = (0, L) if window is None else window
    pos = torch.arange(n, dtype=torch.long).unsqueeze(0)
    plain = O.additive_mask(attention_mask, n, 0, x.dtype)
    cut = plain if drop is None else RR.blocked_mask(attention_mask, drop, rows, x.dtype)
    states = [x]
    for i in range(L):
        x, _ = O.llm_layer(sd, cfg, i, x, cut if lo <= i < hi else plain, pos)
        states.append(x)
    return states


def lens(sd, cfg, states, attention_mask, labels, stage=2, candidate_ids=None):
    """The lens read-outs of a right-padded batch from its ``composed_states``.  Score row of clip b: position len(b) - 4 (stage 2); token row:
    ``token_row``.  -> dict: 'score' [B, L + 1] in the dtype of the pass, 'score_hidden' [B, L + 1, H] (stage 2); 'token' int64 [B, L + 1] (-1:
    no answer token), 'token_logits' [B, L + 1, V] fp32 (the row's logits, for the tie rule), 'token_logprob' fp32 [B, L + 1], 'token_hidden'
    [B, L + 1, H], 'cand_logprob' fp32 [B, L + 1, C] with ``candidate_ids``."""
    B = attention_mask.shape[0]
    lens_ = attention_mask.long().sum(1).tolist()
    w, eps = sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps
    ar = torch.arange(B)
    out = {}
    if stage == 2:
        srow = torch.tensor([n - 4 for n in lens_])
        raw = torch.stack([x[ar, srow] for x in states], 1)                                   # [B, L + 1, H]
        score = []
        for d in range(len(states)):
            h = O.rms_norm_cast_then_scale(raw[:, d], w, eps)                                 # the batch's B score rows of depth d: the guard's slice
            if torch.isnan(h).any():
                h = torch.nan_to_num(h, nan=0.0, posinf=1e9, neginf=-1e9)
            score.append(O.score_head(sd, cfg, h).squeeze(1))
        out.update(score=torch.stack(score, 1), score_hidden=raw)
    if labels is not None:
        trow = [token_row(labels[b]) for b in range(B)]
        have = [b for b in range(B) if trow[b] is not None]
        D, H = len(states), states[0].shape[-1]
        V = O.lm_logits(sd, states[0][:1, :1]).shape[-1]
        tok = torch.full((B, D), -1, dtype=torch.long)
        logits = torch.full((B, D, V), float("nan"))
        lp = torch.full((B, D), float("nan"))
        hid = torch.zeros(B, D, H, dtype=states[0].dtype)
        C = 0 if candidate_ids is None else len(candidate_ids)
        cl = torch.full((B, D, C), float("nan"))
        for b in have:
            raw = torch.stack([x[b, trow[b]] for x in states])                                # [L + 1, H]
            lg = O.lm_logits(sd, O.rms_norm_cast_then_scale(raw, w, eps))                     # [L + 1, V] fp32
            logp = torch.log_softmax(lg, -1)
            tok[b] = torch.argmax(lg, -1)                                                     # (the first maximal index: ties go to the lower id)
            logits[b], hid[b] = lg, raw
            lp[b] = logp.gather(1, tok[b][:, None])[:, 0]
            if C:
                cl[b] = logp[:, torch.as_tensor(list(candidate_ids), dtype=torch.long)]
        out.update(token=tok, token_logits=logits, token_logprob=lp, token_hidden=hid)
        if C:
            out["cand_logprob"] = cl
    return out
