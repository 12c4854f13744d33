"""Host-side references of the attention tests (no GPU needed): fp64 truth and the reference's eager bf16 path of one sequence, the
acceptance rule that holds a kernel result against both, the rotary rotation with its three bf16 roundings, and the continuation cases
(new query rows behind keys that sit in a KV cache) of tests/test_gpu_attention_forms.py with their per-sequence references.

The continuation cases live here so that tests/test_attention_forms_cpu.py can check, without a GPU, that every case's references are
finite and non-degenerate: the acceptance rule is relative to the eager path's own error, which must therefore be a real number."""
import math

import torch

BF = torch.bfloat16


def attn_truth(q, k, v, causal, scale_pre, post_div, dtype, kv_off=0):
    """q [n,h,d], k/v [m,hk,d] for ONE sequence.  dtype=float64 -> truth; bf16 -> the reference's eager path
    (modeling_intern_vit.py:153-157 / modeling_internlm2.py:407-424) with its rounding points.
    kv_off: keys in front of the first query row (m = kv_off + n): causal query row r sees keys 0 .. kv_off + r."""
    h, hk = q.shape[1], k.shape[1]
    rep = h // hk
    qq = q.transpose(0, 1).to(dtype)
    kk = k.transpose(0, 1).repeat_interleave(rep, 0).to(dtype)
    vv = v.transpose(0, 1).repeat_interleave(rep, 0).to(dtype)
    if scale_pre != 1.0:
        qq = qq * scale_pre
    s = qq @ kk.transpose(1, 2)
    if post_div != 1.0:
        s = s / post_div
    if causal:
        n = q.shape[0]
        m = torch.full((n, k.shape[0]), torch.finfo(dtype).min, dtype=dtype).triu(1 + kv_off)
        s = s + m
    if dtype == BF and post_div != 1.0:
        p = torch.softmax(s, -1, dtype=torch.float32).to(BF)      # LLM: fp32 softmax, cast back
    else:
        p = torch.softmax(s, -1)
    return (p @ vv).transpose(0, 1)


def check_sequence(got, truth, eager):
    """The acceptance rule of ONE sequence (got / truth / eager: float64 [n,h,d]): the kernel is at least as accurate against fp64 truth as
    the eager bf16 path.  Returns (sum |hip - eager|, sum |eager - truth|) for the caller's round_scores rule over the whole case."""
    e_hip = (got - truth).abs()
    e_ref = (eager - truth).abs()
    assert torch.isfinite(got).all()
    assert e_hip.mean() <= 1.5 * e_ref.mean() + 1e-4, (e_hip.mean().item(), e_ref.mean().item())
    assert e_hip.max() <= 2.0 * e_ref.max() + 2e-3, (e_hip.max().item(), e_ref.max().item())
    return (got - eager).abs().sum().item(), e_ref.sum().item()


def rope_ref(x, pos, cos, sin):
    """x [T, ..., D] bf16 rotated at pos [T] with the tables cos / sin [max_pos, D/2] bf16: bf16 ops = the reference's three rounding points
    (modeling_internlm2.py:247-261), the arithmetic of aigv_op_rope and of the attention kernel's query load."""
    D = x.shape[-1]
    shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (D,)
    c = torch.cat([cos, cos], -1)[pos.long()].view(shape)
    s = torch.cat([sin, sin], -1)[pos.long()].view(shape)
    rot = torch.cat((-x[..., D // 2:], x[..., : D // 2]), dim=-1)
    return (x * c) + (rot * s)


def rope_table(d, n_pos):
    """cos / sin [n_pos, d/2] bf16 (theta 1e6, InternLM2's), fp32 angles."""
    ang = torch.arange(0, n_pos)[:, None].float() * (1.0 / (1.0e6 ** (torch.arange(0, d // 2).float() / (d // 2))))[None, :]
    return ang.cos().to(BF), ang.sin().to(BF)


D = 128
N_POS = 2600        # rows of the rotary tables: past the longest sequence of any case (2177 + 210)

# Continuation cases: (name, key offsets per sequence, new-row counts per sequence, query heads, kv heads, cache capacity).
# Every offset of {0, 1, 63, 64, 65, 127, 128, 2175, 2176, 2177} meets every count of {1, 31, 32, 33, 127, 128, 129, 210} as one sequence of an
# eight-sequence launch (max_len = 210 = the largest count); the group sizes 1, 3, 4, 6, 8 rotate over the offsets.  Then the ragged batches
# that mix offsets and counts, the group sizes again at the scoring shape (2176 cached tokens, a question behind them), and a capacity that
# is no multiple of the 64-key tile (2441) next to ones that are.
OFFSETS = [0, 1, 63, 64, 65, 127, 128, 2175, 2176, 2177]
COUNTS = [1, 31, 32, 33, 127, 128, 129, 210]
_GROUPS = [(1, 1), (3, 1), (4, 2), (6, 1), (8, 1)]      # (g, kv heads)
CONTINUATION_CASES = []
for _i, _off in enumerate(OFFSETS):
    _g, _hk = _GROUPS[_i % len(_GROUPS)]
    CONTINUATION_CASES.append((f"off{_off}-g{_g}", [_off] * len(COUNTS), COUNTS, _g * _hk, _hk, 2441 if _i % 2 == 0 else 2432))
CONTINUATION_CASES += [
    ("ragged-2176-63-0", [2176, 63, 0], [40, 210, 1], 8, 2, 2441),
    ("ragged-2169-2176", [2169, 2176], [23, 16], 6, 1, 2441),
    ("ragged-g3", [2177, 128, 65, 1], [129, 33, 210, 64], 6, 2, 2441),
    ("scoring-g1", [2176, 2176], [210, 20], 2, 2, 2441),
    ("scoring-g6x8", [2176], [77], 48, 8, 2441),
    ("scoring-g8", [2176, 2175], [20, 210], 8, 1, 2496),
]
CASE_IDS = [c[0] for c in CONTINUATION_CASES]


class ContinuationCase:
    """The tensors of one continuation case.  Token order of ``rows``: sequence after sequence, each with its cached tokens first and its
    new tokens behind them (position = index in the sequence).  ``rows`` [tokens, hk * (g + 2) * D] is the fused wqkv layout, per kv group
    [g q heads | K | V], UNROTATED (the device rotates K with aigv_op_rope and Q inside the attention kernel); ``q_rot_new`` / ``k_rot`` are the
    host's rotation of the same numbers for the references."""

    def __init__(self, name, offs, cnts, h, hk, cap):
        assert len(offs) == len(cnts) and h % hk == 0 and all(o + n <= cap and o + n <= N_POS for o, n in zip(offs, cnts))
        self.name, self.offs, self.cnts, self.h, self.hk, self.cap, self.g = name, list(offs), list(cnts), h, hk, cap, h // hk
        gen = torch.Generator().manual_seed(1000 * sum(offs) + 7 * sum(cnts) + h + len(name))
        tot = [o + n for o, n in zip(offs, cnts)]
        T = sum(tot)
        q = (torch.randn(T, h, D, generator=gen) * 1.5).to(BF)
        k = (torch.randn(T, hk, D, generator=gen) * 1.5).to(BF)
        v = torch.randn(T, hk, D, generator=gen).to(BF)
        self.seq = torch.cat([torch.full((t,), s, dtype=torch.int32) for s, t in enumerate(tot)])
        self.pos = torch.cat([torch.arange(t, dtype=torch.int32) for t in tot])
        start = [0]
        for t in tot:
            start.append(start[-1] + t)
        self.start = start
        # large, late-arriving maxima so that the online-softmax rescale path is exercised, as in _attention_case: one inside the cached
        # part (the rows in front of the second one see only it) and one inside the new rows (a late maximum for the rows behind it)
        # (not for a sequence with ONE new row: no row lies behind a late maximum there, and a key its only query favours would make the
        # whole sequence one-hot - a V row copied out, exact in every evaluation, which measures nothing)
        for s, (o, n) in enumerate(zip(offs, cnts)):
            if n == 1:
                continue
            if o > 0:
                k[start[s] + o // 2] *= 6.0
            k[start[s] + o + n // 2] *= 6.0
        self.cos, self.sin = rope_table(D, N_POS)
        fused = torch.zeros(T, hk, self.g + 2, D, dtype=BF)
        fused[:, :, : self.g] = q.view(T, hk, self.g, D)
        fused[:, :, self.g] = k
        fused[:, :, self.g + 1] = v
        self.rows = fused.view(T, -1)
        # the packed new rows (what a continuation pass holds): indices into ``rows``
        self.new_idx = torch.cat([torch.arange(start[s] + o, start[s] + o + n) for s, (o, n) in enumerate(zip(offs, cnts))])
        self.q_rot_new = rope_ref(q[self.new_idx], self.pos[self.new_idx], self.cos, self.sin)     # (only the new rows query)
        self.k_rot = rope_ref(k, self.pos, self.cos, self.sin)
        self.v = v
        self._refs = None

    def references(self):
        """Per sequence (truth, eager) as float64 [n, h, D]: fp64 truth and the eager bf16 restatement over the concatenated keys, new row r
        seeing keys 0 .. off + r.  Computed once per case."""
        if self._refs is None:
            post = math.sqrt(D)
            self._refs = []
            row = 0
            for s, (o, n) in enumerate(zip(self.offs, self.cnts)):
                a = self.start[s]
                qs, ks, vs = self.q_rot_new[row: row + n], self.k_rot[a: a + o + n], self.v[a: a + o + n]
                row += n
                truth = attn_truth(qs, ks, vs, True, 1.0, post, torch.float64, kv_off=o)
                eager = attn_truth(qs, ks, vs, True, 1.0, post, BF, kv_off=o).double()
                self._refs.append((truth, eager))
        return self._refs


_CASES = {}


def continuation_case(name):
    if name not in _CASES:
        _CASES[name] = ContinuationCase(*CONTINUATION_CASES[CASE_IDS.index(name)])
    return _CASES[name]
