"""Host references of the score-row attention probe (csrc/attnprobe.hip; aigv_op_attention_probe / aigv_score_attention_arm), shared by
tests/test_score_attention_cpu.py and tests/test_gpu_score_attention.py.

* the float64 reference of one probe row: rotate q, causal softmax over the row's keys, fold into segment bins;
* the op-level case: three sequences of lengths 1, 258 and 513 packed together, probe rows at the local indices 0, 1, 254, 255, 256, 257
  and 512 wherever a sequence has them - one key, both sides of the kernel's 256-thread key stride, a second full sweep - as fused wqkv
  rows [g query heads | K | V] per kv head, with a segment table that also holds ids outside [0, S) (dropped keys);
* the two constructions whose result is exact in fp32 whatever a correct kernel's summation order: the key census (Q = 0: every visible key
  weighs exactly 1, a bin is a COUNT) and the one-hot selector (one key leads the others by a margin at which exp underflows to 0)."""
import math

import torch

from attention_reference import rope_ref, rope_table

BF = torch.bfloat16
D = 128
N_KV = 2                      # kv heads: the query-head -> kv-head map is part of what is tested
GROUPS = [1, 3, 4]            # g query heads per kv head
LENS = [1, 258, 513]
LOCALS = [0, 1, 254, 255, 256, 257, 512]
S = 5                         # bins; the table below also carries -1 and S: keys that count for the total only
N_POS = 600                   # rows of the rotary tables
CACHE_OFF = [0, 100, 254]     # cache form: keys of every sequence that were cached before the pass
CACHE_CAP = 520
EXP_UNDERFLOW = 104.0         # exp(-x) is exactly 0 in fp32 for x >= 103.98 (below half the smallest subnormal 2^-149)
SELECT_SCALE = 64.0           # the selector's keys are +-SELECT_SCALE * (a query vector): a power of two, exact in bf16


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def probe_rows(lens=LENS, locals_=LOCALS):
    """[(sequence, local row, packed row)] of every probe row the lengths admit, in packed order."""
    cu = cu_of(lens)
    return [(b, r, cu[b] + r) for b in range(len(lens)) for r in locals_ if r < lens[b]]


def seg_table(lens=LENS, n_seg=S):
    """int32 id per packed token in -1 .. n_seg: a different residue pattern per sequence, so that a key taken from another sequence, or
    shifted by one, lands in another bin; -1 and n_seg are outside [0, n_seg) - dropped from the bins, kept in the total."""
    out = []
    for b, n in enumerate(lens):
        j = torch.arange(n)
        out.append(((j * (3 + 2 * b) + b) % (n_seg + 2) - 1).to(torch.int32))
    return torch.cat(out)


def fused(q, k, v=None):
    """q [T, hk, g, D], k [T, hk, D] bf16 -> the fused wqkv rows [T, hk * (g + 2) * D] ([g query heads | K | V] per kv head)."""
    T, hk, g, d = q.shape
    v = torch.zeros_like(k) if v is None else v
    return torch.cat([q, k[:, :, None], v[:, :, None]], 2).reshape(T, hk * (g + 2) * d).contiguous()


def rotate_q(q, pos, cos, sin):
    """q [T, hk, g, D] bf16 rotated at pos [T]: the bf16 bits aigv_op_rope stores (rope_ref: the same three rounding points)."""
    return rope_ref(q, pos, cos, sin)


def positions(lens=LENS):
    return torch.cat([torch.arange(n) for n in lens]).to(torch.int32)


def row_truth(q_rot, keys, seg, n_seg):
    """ONE probe row in float64: q_rot [h, D] (already rotated), keys [n, hk, D] (the row's visible keys, rotated), seg [n] ->
    (mass [h, n_seg], dropped [h]): the causal softmax of the row over its n keys, summed per segment; mass.sum(-1) + dropped = 1."""
    h, hk = q_rot.shape[0], keys.shape[1]
    kk = keys.double().transpose(0, 1).repeat_interleave(h // hk, 0)            # [h, n, D]
    s = torch.einsum("hd,hnd->hn", q_rot.double(), kk) / math.sqrt(q_rot.shape[-1])
    p = torch.softmax(s, -1)
    mass = torch.zeros(h, n_seg, dtype=torch.float64)
    inside = (seg >= 0) & (seg < n_seg)
    mass.index_add_(1, seg[inside].long(), p[:, inside])
    return mass, p[:, ~inside].sum(-1)


def score_bound(q_rot, keys):
    """The per-score error bound of the kernel's fp32 dot: eps = (D + 2) 2^-24 max_j sum_i |q_i| |k_ji| / sqrt(D), per head [h] - D fused
    multiply-adds, one division and the subtraction of the row maximum, each rounding once relative to at most sum |q||k| / sqrt(D)."""
    h, hk = q_rot.shape[0], keys.shape[1]
    kk = keys.double().abs().transpose(0, 1).repeat_interleave(h // hk, 0)
    d = q_rot.shape[-1]
    return (d + 2) * 2.0 ** -24 * torch.einsum("hd,hnd->hn", q_rot.double().abs(), kk).max(-1).values / math.sqrt(d)


EXP_C = 4.0   # covers the device expf's stated 1 ulp (2 * 2^-24) on both sides of the division + the division's own rounding, next to the n + S additions


def mass_bound(mass, eps, n_keys, n_seg, extra_rel=0.0):
    """|d mass| <= mass (e^(2 eps) - 1 + c 2^-24 (n + S)) + 2^-24: a score error eps moves every exp by a factor e^(+-eps), so a ratio of sums
    of them by at most e^(2 eps); the exps (c), the n additions of the total and of a bin and the final division round relative to the mass;
    2^-24 absolute for masses near the bottom of fp32's range of interest.  extra_rel: a further relative score error (model level: the bf16
    rounding of q and k), already propagated to the exponent by the caller."""
    rel = torch.expm1(2 * (eps + extra_rel))[:, None] + EXP_C * 2.0 ** -24 * (n_keys + n_seg)
    return mass * rel + 2.0 ** -24


def census_expect(lens=LENS, n_seg=S, seg=None, off=None):
    """{packed row: fp32 [n_seg]} of the key census: count of the row's visible keys per segment / their number, ONE fp32 division."""
    seg = seg_table(lens, n_seg) if seg is None else seg
    cu = cu_of(lens)
    out = {}
    for b, r, t in probe_rows(lens):
        vis = seg[cu[b]:cu[b] + r + 1]
        counts = torch.tensor([int((vis == s).sum()) for s in range(n_seg)], dtype=torch.float32)
        out[t] = counts / torch.tensor(float(r + 1), dtype=torch.float32)
    return out


class RandomCase:
    """Seeded bf16 data of the op-level case for g query heads per kv head: q [T, hk, g, D] unrotated, k [T, hk, D] (taken as rotated)."""

    def __init__(self, g, seed=0, lens=LENS, scale=1.0):
        gen = torch.Generator().manual_seed(4100 + 17 * g + seed)
        self.g, self.lens, self.cu, self.T = g, lens, cu_of(lens), sum(lens)
        self.q = (torch.randn(self.T, N_KV, g, D, generator=gen) * scale).to(BF)
        self.k = (torch.randn(self.T, N_KV, D, generator=gen) * scale).to(BF)
        self.seg = seg_table(lens)
        self.pos = positions(lens)
        self.cos, self.sin = rope_table(D, N_POS)

    def truth(self, q_rot=None):
        """{packed row: (mass [h, S] float64, bound [h, S])}; q_rot [T, hk, g, D]: the device's rotation, else the host's."""
        q_rot = rotate_q(self.q, self.pos, self.cos, self.sin) if q_rot is None else q_rot
        out = {}
        for b, r, t in probe_rows(self.lens):
            keys = self.k[self.cu[b]:self.cu[b] + r + 1]
            qr = q_rot[t].reshape(N_KV * self.g, D)
            mass, _ = row_truth(qr, keys, self.seg[self.cu[b]:self.cu[b] + r + 1], S)
            out[t] = (mass, mass_bound(mass, score_bound(qr, keys), r + 1, S))
        return out


class SelectorCase:
    """One-hot selector for the probe row (sequence b, local row r) with the selected key at local position `sel`: q is a +-1 vector per
    head; the selected key is SELECT_SCALE * (q ROTATED at the row's position), a competitor in another bin at position `comp` is
    SELECT_SCALE * (q UNROTATED), every other visible key is zero - and every key the row may NOT see (behind it, other sequences) is the
    selected key times two, which would win.  With q rotated as the RoPE kernel rotates it the selected key leads every other by
    `margin()` >= EXP_UNDERFLOW; with q left unrotated the competitor leads."""

    def __init__(self, g, b, r, sel, lens=LENS):
        gen = torch.Generator().manual_seed(977 + 31 * r + sel)
        self.g, self.b, self.r, self.sel, self.lens, self.cu, self.T = g, b, r, sel, lens, cu_of(lens), sum(lens)
        self.row = self.cu[b] + r
        self.comp = None
        self.cos, self.sin = rope_table(D, N_POS)
        self.pos = positions(lens)
        self.seg = seg_table(lens)
        for step in range(3, r + 1):                        # the competitor: a visible key of ANOTHER bin (inside [0, S): its mass would show)
            j = (sel + step) % (r + 1)
            sg = int(self.seg[self.cu[b] + j])
            if j != sel and 0 <= sg < S and sg != int(self.seg[self.cu[b] + sel]):
                self.comp = j
                break
        # one +-1 vector per KV head, shared by its g query heads: the key of a kv head can then select for all of them
        qv = (torch.randint(0, 2, (N_KV, 1, D), generator=gen) * 2 - 1).to(BF).expand(N_KV, g, D)
        self.q = torch.zeros(self.T, N_KV, g, D, dtype=BF)
        self.q[self.row] = qv
        q_rot = rotate_q(self.q[self.row:self.row + 1], torch.tensor([r]), self.cos, self.sin)[0]        # [hk, g, D]
        k_sel = (q_rot[:, 0].float() * SELECT_SCALE).to(BF)                                             # exact: a power of two
        self.k = torch.zeros(self.T, N_KV, D, dtype=BF)
        self.k[:] = k_sel * 2                                # what the row must never read ...
        self.k[self.cu[b]:self.row + 1] = 0                  # ... its own visible keys: zero,
        self.k[self.cu[b] + sel] = k_sel                     # the selected one,
        if self.comp is not None:
            self.k[self.cu[b] + self.comp] = (qv[:, 0].float() * SELECT_SCALE).to(BF)     # and the competitor
        self.q_rot = q_rot

    def margin(self):
        """The least lead (float64) of the selected key's score over any other visible key's, over the heads."""
        keys = self.k[self.cu[self.b]:self.row + 1].double()                                 # [n, hk, D]
        s = torch.einsum("kgd,nkd->kgn", self.q_rot.double(), keys) / math.sqrt(D)
        lead = s[..., self.sel:self.sel + 1] - s
        lead[..., self.sel] = float("inf")
        return float(lead.min())

    def expect(self):
        e = torch.zeros(N_KV * self.g, S, dtype=torch.float32)
        sg = int(self.seg[self.cu[self.b] + self.sel])
        if 0 <= sg < S:
            e[:, sg] = 1.0
        return e


def selector_cases():
    """(sequence, local probe row, selected key): the key at the first position, the last, and on both sides of the 256-thread stride, for
    the last rows of the two long sequences; for rows 0 and 1 (one key, two keys) every choice."""
    cases = [(0, 0, 0), (1, 1, 0), (1, 1, 1)]
    for b, r in ((1, 257), (2, 512)):
        cases += [(b, r, sel) for sel in (0, 255, 256, r)]
    return cases
