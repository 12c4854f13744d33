"""Host references of the VALUES form of the score-row attention probe (what the row takes from every segment: aigv_op_attention_probe_values /
aigv_score_attention_arm_values / ``forward(return_score_values=True)``), shared by tests/test_score_values_cpu.py and
tests/test_gpu_score_values.py.  The shapes, the data and the exact constructions are tests/score_attention_reference.py's own; this file adds
what is per (segment, column): the float64 row, the derived tolerance, the expectations of the census and the selector, a table of contiguous
runs beside ``seg_table`` (which changes the id at every key), and a CPU restatement of the kernel's stated fp32 chain with a free number of
key lanes - the yardstick's own proof, and the carrier of the planted faults."""
import math

import torch

import score_attention_reference as R
import score_attention_tokens_reference as TR

U, EXP_ULP, ABS_FLOOR = TR.U, TR.EXP_ULP, TR.ABS_FLOOR
MAX_LANES = 4                   # key lanes of the kernel: 256 / D, 2 at D = 128 and 4 at D = 64


def slot_of(seg, n_seg):
    """The output slot of every key: its id inside [0, n_seg), else the rest slot n_seg."""
    seg = seg.long()
    return torch.where((seg >= 0) & (seg < n_seg), seg, torch.full_like(seg, n_seg))


def run_table(lens=R.LENS, n_seg=R.S, run=37):
    """int32 id per packed token: contiguous runs of `run` keys, shifted per sequence (a table of another sequence differs), every id inside
    [0, n_seg) - the shape of the default table (frames are runs), where the kernel's running accumulator is exchanged once per run."""
    return torch.cat([(((torch.arange(n) + 11 * b) // run + b) % n_seg).to(torch.int32) for b, n in enumerate(lens)])


def row_truth(q_rot, keys, vals, seg, n_seg):
    """ONE probe row in float64: q_rot [h, D] (rotated), keys / vals [n, hk, D], seg [n] -> (val [h, n_seg + 1, D] = sum over the keys of every
    slot of p_j v_j, slot n_seg = the keys outside [0, n_seg); weight [h, n_seg + 1, D] = sum of p_j |v_j|: what the bound is relative to)."""
    h, hk = q_rot.shape[0], keys.shape[1]
    p = TR.row_truth(q_rot, keys)                                                     # [h, n]
    vv = vals.double().transpose(0, 1).repeat_interleave(h // hk, 0)                  # [h, n, D]
    onehot = torch.zeros(len(seg), n_seg + 1, dtype=torch.float64)
    onehot[torch.arange(len(seg)), slot_of(seg, n_seg)] = 1.0
    return torch.einsum("hn,ns,hnd->hsd", p, onehot, vv), torch.einsum("hn,ns,hnd->hsd", p, onehot, vv.abs())


def chain_roundings(n_keys, key_lanes=None):
    """c of ``value_bound``: the roundings between exact e_j, v_j and one stored element, as csrc/attnprobe.hip's header states the chain -
    expf's stated ulp (2 units) on the numerator's e_j and, as every term carries it, on the total; the total's ceil(n / 256) + 9 additions
    (score_attention_tokens_reference.total_additions); ONE fma per key of the longest key lane, ceil(n / KL); the KL - 1 lane additions; ONE
    division.  key_lanes None: the count that holds for every KL <= 4 at once, n fmas and 3 lane additions (ceil(n / KL) + KL - 1 <= n + 3)."""
    chain = n_keys + MAX_LANES - 1 if key_lanes is None else -(-n_keys // key_lanes) + key_lanes - 1
    return 2 * (EXP_ULP / U) + TR.total_additions(n_keys) + chain + 1


def value_bound(weight, eps, n_keys, key_lanes=None, extra_rel=0.0):
    """|val_fp32 - val| <= (sum_{j in s} p_j |v_j[c]|) (e^(2 eps) (1 + gamma_c) - 1) + 2^-126, the per-(segment, column) analogue of
    score_attention_tokens_reference.key_bound.  Derivation: val = (sum_j e_j v_j) / total.  A score error eps (score_bound: the fp32 dot, its
    division, the subtraction of the maximum) moves every e_j by a factor e^(+-eps), so every term e_j v_j / total by at most e^(2 eps) - relative
    to |p_j v_j|, whatever the signs of v: the terms of a sum may cancel, the bound is relative to the sum of their magnitudes.  v_j is bf16 and
    exact in fp32.  An fma chain of m steps carries every term through at most m roundings (each relative to a partial sum of magnitude at most
    sum |e_j v_j|), the lane additions KL - 1 more, the numerator's e_j has expf's ulp, the total its own chain, and one division ends it: c =
    chain_roundings roundings of at most 2^-24, gamma_c = c u / (1 - c u) bounds their product.  2^-126 absolute: below the normal range a
    product may lose bits.  Nothing here is measured.  weight: row_truth's second result; eps: [h]; extra_rel as in key_bound."""
    c = chain_roundings(n_keys, key_lanes)
    gamma = c * U / (1 - c * U)
    rel = torch.exp(2 * (eps + extra_rel))[:, None, None] * (1 + gamma) - 1
    return weight * rel + ABS_FLOOR


def census_values(vals, seg, n_keys, n_seg, g):
    """The census row (Q = 0: every e_j is exactly 1) over small-integer V (|v| <= 8: every partial sum stays <= 8 * 513 = 4104, an integer, exact
    in fp32 in any order): fp32(sum_{j in s} v_j[c]) / fp32(n), ONE correctly rounded division.  vals [n, hk, D] -> fp32 [hk g, n_seg + 1, D]."""
    hk, d = vals.shape[1], vals.shape[2]
    sums = torch.zeros(hk, n_seg + 1, d, dtype=torch.float64)
    sums.index_add_(1, slot_of(seg[:n_keys], n_seg), vals[:n_keys].double().transpose(0, 1))
    assert sums.abs().max() <= 2 ** 24
    return (sums.float() / torch.tensor(float(n_keys), dtype=torch.float32)).repeat_interleave(g, 0)


def census_v(T, hk=R.N_KV, d=R.D, seed=0):
    """bf16 V of small integers in -8 .. 8."""
    gen = torch.Generator().manual_seed(8100 + seed)
    return torch.randint(-8, 9, (T, hk, d), generator=gen).to(R.BF)


def random_v(T, hk=R.N_KV, d=R.D, seed=0):
    gen = torch.Generator().manual_seed(8200 + seed)
    return torch.randn(T, hk, d, generator=gen).to(R.BF)


def selector_values(case, vals, n_seg=R.S):
    """SelectorCase: the selected key's slot holds V[sel] exactly (weight exactly 1, total exactly 1), every other slot 0 (compare by value: the
    sign of a zero is not part of the contract).  -> fp32 [hk g, n_seg + 1, D]."""
    t = case.cu[case.b] + case.sel
    e = torch.zeros(R.N_KV * case.g, n_seg + 1, vals.shape[-1], dtype=torch.float32)
    e[:, int(slot_of(case.seg[t:t + 1], n_seg))] = vals[t].float().repeat_interleave(case.g, 0)
    return e


# ---- the kernel's fp32 chain, restated on the CPU ---------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fma emulated: the float64 product of two fp32 numbers is exact, the float64 sum rounds once (at 2^-53), then once to fp32."""
    return (a.double() * b.double() + c.double()).float()


def chain_fp32(q_rot, keys, vals, seg, n_seg, lanes=2, fault=None, off=0):
    """ONE probe row through the chain csrc/attnprobe.hip's header states, in float32 torch ops: q_rot [h, D] bf16 (rotated), keys / vals
    [n, hk, D] bf16, seg [n] -> fp32 [h, n_seg + 1, D].  Scores by fma in element order and one division, e_j = exp(s_j - max), the total as the
    256 thread partials (keys t, t + 256, ..), a butterfly inside each 64-lane wave and the four waves in order; then per key lane kl (keys j = kl
    mod `lanes`, ascending) one fma per key into the slot of the key's id, the lanes added in order, ONE division by the total.
    fault: a planted error, for the test that the yardstick refuses it - 'no_division', 'last_key' (the last visible key left out of the value
    sum), 'boundary' (the cached / new boundary `off` of the id lookup off by one: the keys from off - 1 on take the next key's id)."""
    n, hk, d = keys.shape
    h = q_rot.shape[0]
    kk = keys.float().transpose(0, 1).repeat_interleave(h // hk, 0)                     # [h, n, D]
    vv = vals.float().transpose(0, 1).repeat_interleave(h // hk, 0)
    q = q_rot.float()
    acc = torch.zeros(h, n, dtype=torch.float32)
    for i in range(d):
        acc = fma32(q[:, i:i + 1], kk[:, :, i], acc)
    s = acc / torch.tensor(math.sqrt(d), dtype=torch.float32)
    e = torch.exp(s - s.max(-1, keepdim=True).values)                                  # fp32
    part = torch.zeros(h, 256, dtype=torch.float32)
    for j0 in range(0, n, 256):
        w = min(256, n - j0)
        part[:, :w] = part[:, :w] + e[:, j0:j0 + w]
    lane = torch.arange(64)
    wv = part.view(h, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        wv = wv + wv[:, :, lane ^ o]
    total = ((wv[:, 0, 0] + wv[:, 1, 0]) + wv[:, 2, 0]) + wv[:, 3, 0]                  # [h]
    slot = slot_of(seg, n_seg)
    if fault == "boundary" and off >= 1:
        slot = torch.cat([slot[:off - 1], slot[off:], slot[-1:]])
    last = n - 1 if fault == "last_key" else n
    out = torch.zeros(lanes, h, n_seg + 1, d, dtype=torch.float32)
    for kl in range(lanes):
        for j in range(kl, last, lanes):
            sl = int(slot[j])
            out[kl, :, sl] = fma32(e[:, j:j + 1], vv[:, j], out[kl, :, sl])
    val = out[0]
    for kl in range(1, lanes):
        val = val + out[kl]
    return val if fault == "no_division" else val / total[:, None, None]


class ValuesCase(R.RandomCase):
    """RandomCase with a random bf16 V [T, hk, D] beside q and k; ``seg``: seg_table (every key changes the id; -1 and S: the rest slot)."""

    def __init__(self, g, seed=0, lens=R.LENS):
        super().__init__(g, seed, lens)
        self.v = random_v(self.T, seed=17 * g + seed)
        self.runs = run_table(lens)

    def truth(self, seg=None, q_rot=None, key_lanes=None, n_seg=R.S):
        """{packed row: (val [h, S + 1, D] float64, bound)} over `seg` (default: seg_table)."""
        seg = self.seg if seg is None else seg
        q_rot = R.rotate_q(self.q, self.pos, self.cos, self.sin) if q_rot is None else q_rot
        out = {}
        for b, r, t in R.probe_rows(self.lens):
            lo = self.cu[b]
            qr = q_rot[t].reshape(R.N_KV * self.g, R.D)
            val, weight = row_truth(qr, self.k[lo:lo + r + 1], self.v[lo:lo + r + 1], seg[lo:lo + r + 1], n_seg)
            out[t] = (val, value_bound(weight, R.score_bound(qr, self.k[lo:lo + r + 1]), r + 1, key_lanes))
        return out
