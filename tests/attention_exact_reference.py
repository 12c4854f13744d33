"""Host-side generators of the EXACT attention tests (no GPU, torch and numpy only): two input constructions whose softmax is exact in
every correct evaluation order, so that the expected output of a kernel is one fixed bit pattern and a single wrong key, row or head
flips output bits - where the statistical bar of attention_reference.check_sequence lets a dropped key of a long row pass.

Key census.  Q = 0, so every visible score is exactly 0, every visible P is exp2(0) = 1, the running sum l is the NUMBER of visible keys and
the accumulator an integer count per column: V[s, hk][j, c] = w(hk) where (j + phase(s, hk)) mod D == c (j: the key's position in its
sequence, cached keys included; the phases are pairwise distinct over the (sequence, kv head) pairs of a launch; the weight w is 1 + hk,
so that a row with a multiple of D visible keys - the same count in every column whatever the phase - still tells any two kv heads
apart; cnt below is w times the count, still an integer), K is random and must not matter.
The output restates the kernel's normalisation: bf16(fp32(cnt) * (1.0f / fp32(l))) for the prefill kernel's store epilogue,
bf16(fp32(cnt) / fp32(l)) for the decode merge pass (no fast-math: both correctly rounded; the key-split, lead-key and chunk merges
multiply by exp(0) = 1).  It pins the exact SET of visible keys of every row and, through the phase, the sequence base and KV head it reads.

One-hot selector.  Keys carry a +-16 repetition code of their index (ceil(log2 n) bits, each floor(D / bits) times, spare dimensions
constant; the index is XORed with the kv head so that neighbouring kv heads hold different codes at the same position), query row r of
head h carries the code of one chosen visible key pi_h(r), V is random.  The selected score leads every other visible one by hundreds of
octaves: its P is 1 (within 2^-10: bf16 1.0), every other P underflows to 0, and the output is the row V[pi_h(r)] bit for bit.  It pins K
addressing against V's, the query-head -> KV-head map, the head order of the output, and the rescale with a late maximum (alpha = 0).

Every case is a list of sequences (offset = keys in front of the first query row, count = query rows); a packed prefill has offset 0, a
decode step is offset len - 1, count 1.  tests/test_attention_exact_cpu.py holds the conditions the constructions rest on."""
import math

import numpy as np
import torch

from attention_reference import CONTINUATION_CASES     # (the case LIST of the continuation tests: offsets x counts)

BF = torch.bfloat16
AMP = 16
KT, DC = 64, 128          # keys per tile of the prefill kernel / per chunk of the decode kernel: where the selector aims


def bf16_bits(x):
    """float32 array -> the int16 bit patterns of round-to-nearest-even bf16 (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def census_counts(l, phase, D):
    """cnt[row, c] = number of keys j < l[row] with (j + phase) mod D == c."""
    l = np.asarray(l, dtype=np.int64).reshape(-1, 1)
    j0 = (np.arange(D) - phase) % D
    return np.clip((l - j0 + D - 1) // D, 0, None)


def census_weight(kh):
    """The value of the one-hot of kv head kh: no two kv heads share it (at most 8 kv heads: bf16-exact, and w * count stays far below 2^24)."""
    return 1 + kh


def census_bits(cnt, l, form):
    """The kernel's normalisation of integer counts, restated in float32: 'prefill' multiplies by the reciprocal, 'decode' divides.
    A row without a visible key is written as zeros by both kernels."""
    c = np.asarray(cnt).astype(np.float32)
    lf = np.asarray(l).reshape(-1, 1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = c * (np.float32(1.0) / lf) if form == "prefill" else c / lf
    return bf16_bits(np.where(lf > 0, x, np.float32(0.0)).astype(np.float32))


def code_bits(n):
    return max(1, (n - 1).bit_length())


def codes(idx, n, D):
    """The repetition code of the indices idx (any shape) among n keys -> float32 [..., D] of +-AMP."""
    b = code_bits(n)
    rep = D // b
    d = np.arange(D)
    bit = np.minimum(d // rep, b - 1)
    val = ((np.asarray(idx, dtype=np.int64)[..., None] >> bit) & 1) * 2 - 1
    return np.where(d < b * rep, val, 1).astype(np.float32) * AMP


class ExactData:
    """One construction of one case.  q[s] [cnt, h, D] (the query rows), k[s] / v[s] [off + cnt, hk, D] (all keys of the sequence), bf16;
    expect [sum cnt, h, D] int16 bit patterns; pi[s] [cnt, h] the selected keys (selector only)."""

    def __init__(self, case, q, k, v, expect, pi=None):
        self.case, self.q, self.k, self.v, self.expect, self.pi = case, q, k, v, expect, pi

    def fused(self):
        """All tokens as fused rows [tokens, hk * (g + 2) * D], per kv group [g q heads | K | V], sequence after sequence with the cached
        tokens in front (their query slots are zero: nothing queries them)."""
        c = self.case
        out = []
        for s, (o, n) in enumerate(zip(c.offs, c.cnts)):
            f = torch.zeros(o + n, c.hk, c.g + 2, c.D, dtype=BF)
            f[o:, :, : c.g] = self.q[s].view(n, c.hk, c.g, c.D)
            f[:, :, c.g] = self.k[s]
            f[:, :, c.g + 1] = self.v[s]
            out.append(f.view(o + n, -1))
        return torch.cat(out)


class ExactCase:
    def __init__(self, name, D, causal, h, hk, offs, cnts, cap=0, form="prefill"):
        assert h % hk == 0 and len(offs) == len(cnts) and (causal or not any(offs))
        self.name, self.D, self.causal, self.h, self.hk, self.g = name, D, causal, h, hk, h // hk
        self.offs, self.cnts, self.cap, self.form = list(offs), list(cnts), cap, form
        self.tot = [o + n for o, n in zip(offs, cnts)]
        self.start = [0] + list(np.cumsum(self.tot))
        self.new_idx = torch.cat([torch.arange(self.start[s] + o, self.start[s] + o + n) for s, (o, n) in enumerate(zip(offs, cnts))])
        self.seq = torch.cat([torch.full((t,), s, dtype=torch.int32) for s, t in enumerate(self.tot)])
        self.pos = torch.cat([torch.arange(t, dtype=torch.int32) for t in self.tot])
        n_seq = len(offs)
        assert n_seq * hk <= D, "the phases could not be pairwise distinct"
        self.phase = (37 * np.arange(n_seq * hk) + 1).reshape(n_seq, hk) % D     # 37 is odd, D a power of two: distinct below D pairs
        self.seed = 7919 * sum(self.tot) + 31 * h + hk + D + len(name)
        # query pre-scale and score division as the suite's cases: InternViT scales q by d^-1/2, InternLM2 divides the scores by sqrt(d)
        self.pre = 1.0 if causal else D ** -0.5
        self.post = math.sqrt(D) if causal else 1.0

    def visible(self, s):
        """Number of visible keys per query row of sequence s (the keys 0 .. visible - 1)."""
        o, n = self.offs[s], self.cnts[s]
        return np.arange(n) + o + 1 if self.causal else np.full(n, o + n)

    def census(self):
        gen = torch.Generator().manual_seed(self.seed)
        q, k, v, exp = [], [], [], []
        for s, (n, t) in enumerate(zip(self.cnts, self.tot)):
            q.append(torch.zeros(n, self.h, self.D, dtype=BF))
            k.append((torch.randn(t, self.hk, self.D, generator=gen) * 1.5).to(BF))
            vs = torch.zeros(t, self.hk, self.D, dtype=BF)
            j = torch.arange(t)
            for kh in range(self.hk):
                vs[j, kh, (j + int(self.phase[s, kh])) % self.D] = float(census_weight(kh))
            v.append(vs)
            vis = self.visible(s)
            e = np.stack([census_bits(census_weight(kh) * census_counts(vis, self.phase[s, kh], self.D), vis, self.form) for kh in range(self.hk)], 1)    # [n, hk, D]
            exp.append(torch.from_numpy(np.repeat(e, self.g, axis=1)))
        return ExactData(self, q, k, v, torch.cat(exp))

    def choose(self, s, rng, rnd=0):
        """pi [cnt, h]: the selected key of every (row, query head).  The aims rotate over rows, heads and sequences: the diagonal, key 0,
        the first / last key of a 64-key tile, the first / last key of a 128-key chunk, the last visible key, a uniformly random visible
        key.  A decode step has one row: its heads rotate over keys 0, 127, 128, len - 1, one key of the last chunk and a random key, and
        ``rnd`` turns the rotation on so that six rounds give every head every aim.  Heads of one group then move off each other's keys."""
        n, h = self.cnts[s], self.h
        vis = self.visible(s)[:, None]
        r, hq = np.arange(n)[:, None], np.arange(h)[None, :]
        u = rng.random((n, h))
        if self.form == "decode":
            last0 = DC * ((vis - 1) // DC)
            cand = [0 * vis, 0 * vis + 127, 0 * vis + 128, vis - 1, last0 + (u * (vis - last0)).astype(np.int64), (u * vis).astype(np.int64)]
            mode = (hq + s + rnd) % 6
        else:
            ft, fc = vis // KT, vis // DC          # complete tiles / chunks among the visible keys
            cand = [np.minimum(self.offs[s] + r, vis - 1) + 0 * hq, 0 * vis,
                    KT * (u * -(-vis // KT)).astype(np.int64), np.where(ft > 0, KT * (u * ft).astype(np.int64) + KT - 1, vis - 1),
                    DC * (u * -(-vis // DC)).astype(np.int64), np.where(fc > 0, DC * (u * fc).astype(np.int64) + DC - 1, vis - 1),
                    vis - 1, (u * vis).astype(np.int64)]
            mode = (r + 3 * hq + s) % 8
        pi = np.zeros((n, h), dtype=np.int64)
        for m, c in enumerate(cand):
            pi = np.where(mode == m, np.minimum(np.broadcast_to(c, (n, h)), vis - 1), pi)
        for a in range(h):                       # different heads of one group choose different keys (where enough keys are visible)
            first = a - a % self.g
            for _ in range(self.g):
                clash = np.zeros(n, dtype=bool)
                for b in range(first, a):
                    clash |= pi[:, b] == pi[:, a]
                clash &= vis[:, 0] > a - first
                if not clash.any():
                    break
                pi[clash, a] = (pi[clash, a] + 1) % vis[clash, 0]
        return pi

    def choices(self, rnd=0):
        rng = np.random.default_rng(self.seed + 2)
        return [self.choose(s, rng, rnd) for s in range(len(self.cnts))]

    def selector(self, rnd=0, base=None):
        """base: an earlier round's data of this case, whose K and V are kept (only the queries and the expectation change with rnd)."""
        gen = torch.Generator().manual_seed(self.seed + 1)
        q, k, v, exp, pis = [], [], [], [], []
        for s, (pi, t) in enumerate(zip(self.choices(rnd), self.tot)):
            mask = np.arange(self.hk) & ((1 << code_bits(t)) - 1)
            q.append(torch.from_numpy(codes(pi ^ np.repeat(mask, self.g)[None, :], t, self.D)).to(BF))
            if base is None:
                k.append(torch.from_numpy(codes(np.arange(t)[:, None] ^ mask[None, :], t, self.D)).to(BF))
                vs = torch.randn(t, self.hk, self.D, generator=gen).to(BF)
            else:
                k.append(base.k[s])
                vs = base.v[s]
            v.append(vs)
            kv_of = torch.arange(self.h) // self.g
            exp.append(vs[torch.from_numpy(pi), kv_of[None, :]].contiguous().view(torch.int16))
            pis.append(pi)
        return ExactData(self, q, k, v, torch.cat(exp), pis)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# packed prefill (aigv_op_attention): (name, D, causal, query heads, kv heads, lengths, uniform flag under the default kernel, lead-key forms)
PACKED = [
    ("vit-1025x2", 64, False, 2, 2, [1025, 1025], True, (False, True)),          # the left-over 1025th row: key split
    ("vit-257-65-1", 64, False, 2, 2, [257, 65, 1], False, (False, True)),
    ("vit-512-300-33", 64, False, 2, 2, [512, 300, 33], False, (False,)),
    ("vit-edges", 64, False, 2, 2, [63, 64, 65, 127, 128, 129], False, (False,)),
    ("llm-g2", 128, True, 4, 2, [200, 77], False, (False,)),
    ("llm-g4", 128, True, 8, 2, [513, 64, 1], False, (False,)),
    ("llm-g3", 128, True, 3, 1, [300, 129], False, (False,)),
    ("llm-g5", 128, True, 10, 2, [257, 64], False, (False,)),
    ("llm-g6", 128, True, 6, 1, [513, 64, 1], False, (False,)),
    ("llm-g7", 128, True, 7, 1, [200, 77], False, (False,)),
    ("llm-g8", 128, True, 8, 1, [385], False, (False,)),
    ("llm-g1-edges", 128, True, 2, 2, [63, 64, 65, 127, 128, 129], False, (False,)),
    ("llm-2176", 128, True, 4, 2, [2176], False, (False,)),
    ("llm-48x8", 128, True, 48, 8, [300, 77, 129], False, (False,)),
    ("vit6b-384-129", 128, False, 2, 2, [384, 129], False, (False,)),
]
PACKED_IDS = [c[0] for c in PACKED]
ONCE = "llm-2176"                       # the canonical clip runs once (default kernel, fp32 scores), not over the cross product
ROPE = ("rope-g4", 128, True, 8, 2, [300, 77, 129])          # aigv_op_attention_rope
# aigv_op_attention_ex: the offsets x counts launches of the continuation tests and three ragged ones
EX_NAMES = [c[0] for c in CONTINUATION_CASES if c[0].startswith("off")] + ["ragged-2176-63-0", "ragged-g3", "scoring-g6x8"]
TRIM_CASE, Q_TAILS = "ragged-g3", (1, 20, 33)
# decode (aigv_op_attention_decode): (g, kv heads) of test_decode_attention_matches_fp64_at_ragged_lengths over its lengths, and the 20 000-key launch
DECODE_PAIRS = [(1, 1), (2, 2), (3, 8), (4, 1), (5, 2), (6, 8), (7, 1), (8, 2), (4, 8)]
DECODE_LENS = [1, 127, 128, 129, 2177, 8191, 8192, 8193, 16384]
DECODE_CAP = 16384 + 128
DECODE_LONG = (4, 2, [20000, 1, 16385, 300], 20480)
DECODE_ROUNDS = 6


def packed_case(name):
    n, D, causal, h, hk, lens, _, _ = PACKED[PACKED_IDS.index(name)]
    return ExactCase(n, D, causal, h, hk, [0] * len(lens), lens)


def rope_case():
    n, D, causal, h, hk, lens = ROPE
    return ExactCase(n, D, causal, h, hk, [0] * len(lens), lens)


def ex_case(name):
    n, offs, cnts, h, hk, cap = [c for c in CONTINUATION_CASES if c[0] == name][0]
    return ExactCase("ex-" + n, 128, True, h, hk, offs, cnts, cap)


def decode_case(g, n_kv, lens=None, cap=DECODE_CAP):
    lens = DECODE_LENS if lens is None else lens
    return ExactCase(f"decode-g{g}x{n_kv}", 128, True, g * n_kv, n_kv, [n - 1 for n in lens], [1] * len(lens), cap, form="decode")


def all_cases():
    """(id, factory) of every case the GPU file runs."""
    out = [(n, lambda n=n: packed_case(n)) for n in PACKED_IDS] + [(ROPE[0], rope_case)] + [("ex-" + n, lambda n=n: ex_case(n)) for n in EX_NAMES]
    out += [(f"decode-g{g}x{k}", lambda g=g, k=k: decode_case(g, k)) for g, k in DECODE_PAIRS]
    g, k, lens, cap = DECODE_LONG
    return out + [("decode-long", lambda: decode_case(g, k, lens, cap))]
