"""Host references of the DENSE form of the score-row attention probe (one softmax value per key: aigv_op_attention_probe_tokens /
aigv_score_attention_arm_tokens / ``forward(return_token_attention=True)``), shared by tests/test_score_attention_tokens_cpu.py and
tests/test_gpu_score_attention_tokens.py.  The shapes, the data and the exact constructions are tests/score_attention_reference.py's own;
this file adds what is per KEY: the float64 row, the derived tolerances, the expectations of the census and the selector, the segment table
that gives chosen keys a bin each, and the Appendix-A clip with its hand-written positions."""
import math

import torch

import score_attention_reference as R

U = 2.0 ** -24                  # unit roundoff of fp32
EXP_ULP = 2 * U                 # the device expf's stated 1 ulp, relative (an ulp is at most 2^-23 of the value)
ABS_FLOOR = 2.0 ** -126         # below the normal range a result may lose bits or be flushed: absolute, and far below any probability read
EXTRA_LD = 40                   # ld_tok is tested at exactly the need and at this many columns more


def total_additions(n_keys):
    """Additions behind the kernel's softmax total: a thread's ceil(n / 256) keys in ascending order, 6 butterfly steps, 3 wave additions (+ 0.0
    start).  All terms are non-negative, so k additions lose at most k roundings RELATIVE to the sum."""
    return -(-n_keys // 256) + 9


def row_truth(q_rot, keys):
    """ONE probe row in float64, per key: q_rot [h, D] (already rotated), keys [n, hk, D] -> p [h, n], the causal softmax of the row."""
    h, hk = q_rot.shape[0], keys.shape[1]
    kk = keys.double().transpose(0, 1).repeat_interleave(h // hk, 0)
    s = torch.einsum("hd,hnd->hn", q_rot.double(), kk) / math.sqrt(q_rot.shape[-1])
    return torch.softmax(s, -1)


def key_bound(p, eps, n_keys, extra_rel=0.0):
    """|p_fp32 - p| <= p (e^(2 eps) (1 + gamma_c) - 1) + 2^-126 for ONE key's probability p = e_j / total, the per-key analogue of
    score_attention_reference.mass_bound.  A score error eps (score_bound: the fp32 dot, its division, the subtraction of the maximum) moves
    every exp by a factor e^(+-eps), so the ratio e_j / total by at most e^(2 eps).  Then c = 2 + 2 + k + 1 roundings of at most 2^-24 each,
    relative: expf's stated ulp (2 * 2^-24) on the numerator and, as every term of the total carries it, on the total; the total's
    k = ceil(n / 256) + 9 additions of non-negative terms; ONE division.  gamma_c = c u / (1 - c u) bounds their product.  eps: [h];
    extra_rel: a further score error (model level: the bf16 rounding of q and k), already in the exponent's units."""
    c = 2 * (EXP_ULP / U) + total_additions(n_keys) + 1
    gamma = c * U / (1 - c * U)
    rel = torch.exp(2 * (eps + extra_rel))[:, None] * (1 + gamma) - 1
    return p * rel + ABS_FLOOR


def row_sum_bound(n_keys):
    """|sum_j p_j - 1| in float64: every p_j = e_j / total rounds once (the division), the total's own error is at most n roundings."""
    return (n_keys + 2) * U


def bin_bound(bin_value, n_keys):
    """|float64 sum of a bin's dense values - the bin|: the bin's chain (thread additions, 6 butterfly steps, 3 wave additions, one division)
    against one division per key; all terms non-negative, so everything is relative to the bin."""
    return (-(-n_keys // 256) + 11) * U * bin_value


def census_dense(n_keys, ld_tok):
    """The census row (Q = 0): fp32 1 / n - ONE correctly rounded division - on the n visible keys, +0.0 behind them."""
    out = torch.zeros(ld_tok, dtype=torch.float32)
    out[:n_keys] = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n_keys), dtype=torch.float32)
    return out


def one_key_bins(lens=R.LENS, n_bins=63):
    """(segment table int32 [T], keys: per sequence the local key position of every bin) - up to n_bins chosen keys of every sequence get a bin
    EACH (both sides of the 256-thread stride, the first and the last key among them), every other key is dropped (-1)."""
    seg, keys = [], []
    for n in lens:
        want = [0, 1, 254, 255, 256, 257, 511, 512, n - 1] + list(range(3, n, 4))
        chosen = []
        for j in want:
            if 0 <= j < n and j not in chosen and len(chosen) < n_bins:
                chosen.append(j)
        part = torch.full((n,), -1, dtype=torch.int32)
        for s, j in enumerate(chosen):
            part[j] = s
        seg.append(part)
        keys.append(chosen)
    return torch.cat(seg), keys


def appendix_a_clip(n_frames, tpf=4, first_slot=0, motion_slot=0):
    """The slot map of ONE clip in the Appendix-A layout: <s> system | 'Frame i: <img>' ctx x tpf '</img>\\n' per frame | 'Motion Feature:
    <img>' ctx '</img>' | question | answer."""
    slot = [-1] * 4                                                    # <s> + system prompt
    for f in range(n_frames):
        slot += [-1, -1] + list(range(first_slot + f * tpf, first_slot + (f + 1) * tpf)) + [-1]
    return slot + [-1, -1, motion_slot, -1] + [-1] * 5


APPENDIX_A_POSITIONS = [[6, 7, 8, 9], [13, 14, 15, 16]]                # two frames of four tokens, written down by hand from the layout above
