"""Host references of the attention flow map (csrc/attnmap.hip; aigv_op_attention_map / aigv_attention_map_arm /
``forward(return_segment_attention=True, return_row_attention=(lo, hi))``), shared by tests/test_attention_map_cpu.py and
tests/test_gpu_attention_map.py.  Built on tests/score_attention_reference.py: the op-level case (three sequences of lengths 1, 258 and 513
packed together, so that sequences start at the unaligned rows 1 and 259), its segment tables, rotation and bounds are that module's; here
are their ALL-ROWS forms - every one of the 772 rows is a query row - and the fold of the rows into the segment-to-segment matrix.

* ``rows_truth``: float64 causal softmax of every row over its own sequence's keys, folded into the bins (``row_truth`` for all rows);
* ``rows_bound``: ``mass_bound`` per row with eps = 2 x ``score_bound`` - the MFMA accumulation's rounding mode is not documented, so a step
  of the score's accumulation is allowed one ulp instead of the half ulp of a correctly rounded fmaf;
* ``census``: the key census (Q = 0: a bin is a COUNT, the result one fp32 division) for every row;
* the selector: ``score_attention_reference.SelectorCase`` as it stands - the map is read at the case's row;
* ``fold_truth`` (float64) and ``fold_chain`` (the documented fp32 chain: rows added in ascending order from +0.0, one division by their
  number, 0 / 0 = NaN for a segment without a row)."""
import math

import torch

import score_attention_reference as R

D, N_KV = R.D, R.N_KV


def key_counts(lens):
    """[T] int: the number of keys row t sees (its position + 1)."""
    return torch.cat([torch.arange(1, n + 1) for n in lens])


def rows_truth(q_rot, k, seg, lens, n_seg):
    """q_rot [T, hk, g, D] bf16 (already rotated), k [T, hk, D] bf16 (rotated), seg [T] -> (mass [T, h, n_seg] float64, dropped [T, h],
    eps [T, h]): every row's causal softmax over the keys 0 .. p of its own sequence, summed per segment; the mass of the keys whose id lies
    outside [0, n_seg); and ``score_bound`` of the row (over the keys it sees)."""
    T, hk, g, d = q_rot.shape
    h = hk * g
    mass = torch.zeros(T, h, n_seg, dtype=torch.float64)
    dropped = torch.zeros(T, h, dtype=torch.float64)
    eps = torch.zeros(T, h, dtype=torch.float64)
    cu = R.cu_of(lens)
    for b, n in enumerate(lens):
        q = q_rot[cu[b]:cu[b + 1]].double().reshape(n, h, d).transpose(0, 1)                       # [h, n, D]
        kk = k[cu[b]:cu[b + 1]].double().transpose(0, 1).repeat_interleave(g, 0)                   # [h, n, D]
        causal = torch.ones(n, n, dtype=torch.bool).tril()
        s = (q @ kk.transpose(1, 2) / math.sqrt(d)).masked_fill(~causal, float("-inf"))
        p = torch.softmax(s, -1)                                                                   # [h, n, n]
        sg = seg[cu[b]:cu[b + 1]].long()
        inside = (sg >= 0) & (sg < n_seg)
        onehot = torch.zeros(n, n_seg, dtype=torch.float64)
        onehot[inside, sg[inside]] = 1.0
        mass[cu[b]:cu[b + 1]] = (p @ onehot).transpose(0, 1)
        dropped[cu[b]:cu[b + 1]] = p[:, :, ~inside].sum(-1).transpose(0, 1)
        mag = (q.abs() @ kk.abs().transpose(1, 2)).masked_fill(~causal, 0.0).max(-1).values     # [h, n]: max over the visible keys of sum |q||k|
        eps[cu[b]:cu[b + 1]] = ((d + 2) * 2.0 ** -24 * mag / math.sqrt(d)).transpose(0, 1)
    return mass, dropped, eps


def rows_bound(mass, eps, lens, n_seg, extra_rel=None):
    """[T, h, n_seg]: ``score_attention_reference.mass_bound`` of every row at eps = 2 x ``score_bound`` (module docstring).  ``extra_rel``
    [T, h]: a further score error (model level), as in ``mass_bound``."""
    n_keys = key_counts(lens)
    out = torch.empty_like(mass)
    for t in range(mass.shape[0]):
        out[t] = R.mass_bound(mass[t], 2 * eps[t], int(n_keys[t]), n_seg, 0.0 if extra_rel is None else extra_rel[t])
    return out


def census(seg, lens, n_seg):
    """fp32 [T, n_seg]: the count of row t's visible keys per segment / their number, ONE fp32 division."""
    out = []
    cu = R.cu_of(lens)
    for b, n in enumerate(lens):
        sg = seg[cu[b]:cu[b + 1]].long()
        onehot = torch.zeros(n, n_seg, dtype=torch.float32)
        inside = (sg >= 0) & (sg < n_seg)
        onehot[inside, sg[inside]] = 1.0
        out.append(onehot.cumsum(0) / torch.arange(1, n + 1, dtype=torch.float32)[:, None])     # (counts <= 513: exact in fp32)
    return torch.cat(out)


def segment_rows(seg, lens, n_seg):
    """int64 [B, n_seg]: the query rows of every sequence per segment."""
    cu = R.cu_of(lens)
    return torch.stack([torch.bincount(seg[cu[b]:cu[b + 1]][(seg[cu[b]:cu[b + 1]] >= 0) & (seg[cu[b]:cu[b + 1]] < n_seg)].long(), minlength=n_seg)
                        for b in range(len(lens))])


def fold_truth(rows, seg, lens, n_seg):
    """rows [T, h, n_seg] -> float64 [B, h, n_seg, n_seg]: out[b][h][a][c] = mean over the rows t of sequence b with seg[t] == a of
    rows[t][h][c]; NaN where there is none."""
    cu = R.cu_of(lens)
    out = torch.full((len(lens), rows.shape[1], n_seg, n_seg), float("nan"), dtype=torch.float64)
    for b in range(len(lens)):
        sg = seg[cu[b]:cu[b + 1]]
        for a in range(n_seg):
            mine = rows[cu[b]:cu[b + 1]][sg == a].double()
            if mine.shape[0]:
                out[b, :, a] = mine.mean(0)
    return out


def fold_chain(rows, seg, lens, n_seg):
    """The fold as the kernel documents it, in fp32 on the host: the rows of segment a added one by one in ascending row order starting from
    +0.0, then ONE division by their number (0 / 0 = NaN).  rows fp32 [T, h, n_seg] -> fp32 [B, h, n_seg, n_seg]."""
    assert rows.dtype == torch.float32
    cu = R.cu_of(lens)
    out = torch.empty(len(lens), rows.shape[1], n_seg, n_seg, dtype=torch.float32)
    for b in range(len(lens)):
        acc = torch.zeros(n_seg, rows.shape[1], n_seg, dtype=torch.float32)                        # [a][h][c]
        cnt = torch.zeros(n_seg, dtype=torch.float32)
        for t in range(cu[b], cu[b + 1]):
            a = int(seg[t])
            if 0 <= a < n_seg:
                acc[a] = acc[a] + rows[t]
                cnt[a] += 1.0
        out[b] = (acc / cnt[:, None, None]).transpose(0, 1)
    return out
