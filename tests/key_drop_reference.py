"""Host-side generators of the key-drop attention tests (no GPU; torch and numpy only): the two exact constructions of
tests/attention_exact_reference.py - the key census and the one-hot selector - under a per-key "dropped" mask, the drop patterns, the word
layout of AttnArgs::key_drop restated as a naive loop, and float64 / eager-bf16 references of a masked sequence.

Census under a mask.  Q = 0, so every visible score is exactly 0 and the output of row r restates the prefill kernel's normalisation of
w x #{j <= pos, not dropped, (j + phase) mod D = c} over l = #{j <= pos, not dropped}.  The K rows of dropped keys are 3.0e38: finite, and they
must not matter.  A row without a visible key is all zero bits.

Selector under a mask.  One un-dropped key c* per sequence is the chosen key of every row that sees it (c* = the largest un-dropped key <=
max(offset, 1), so every row but possibly the first sees it; a first row in front of it chooses key 0).  EVERY dropped key carries the code
of c* - a decoy whose score ties the chosen key's exactly: a kernel that ignores even one mask bit of a row returns a blend of V rows
instead of V[c*].  The other keys carry the code of their own index.

Every case is a list of sequences (offset = keys in front of the first query row, count = query rows), as in attention_exact_reference;
the drop mask of a sequence is a bool array over its ABSOLUTE key positions, cached keys first."""
import math

import numpy as np
import torch

from attention_exact_reference import BF, KT, ExactCase, ExactData, bf16_bits, census_bits, census_weight, codes, code_bits
from attention_reference import check_sequence      # noqa: F401  (the project's own bar for random data: re-exported for the GPU file)
from score_attention_reference import CACHE_OFF, GROUPS, N_KV

D = 128
BIG_K = 3.0e38                      # K of a dropped key in the census: finite in bf16 (max 3.39e38)
PACKED_LENS = [215, 144, 64, 1]
CACHE_CNTS = [215, 115, 40]         # behind CACHE_OFF = [0, 100, 254]: 215, 215 and 294 keys
CACHE_CAP = 300                     # no multiple of the 64-key tile; rows past a sequence's keys are poisoned by the GPU file
Q_TAILS = (0, 4)
PATTERNS = "abcdefg"
assert CACHE_OFF == [0, 100, 254] and GROUPS == [1, 3, 4]


def packed_case(g):
    return ExactCase(f"drop-packed-g{g}", D, True, g * N_KV, N_KV, [0] * len(PACKED_LENS), PACKED_LENS)


def cache_case(g):
    return ExactCase(f"drop-cache-g{g}", D, True, g * N_KV, N_KV, CACHE_OFF, CACHE_CNTS, CACHE_CAP)


def drop_sets(case, pattern):
    """-> [bool array over the tot keys of every sequence].  (a) scattered single bits, the lane-boundary keys 31, 32 and 63 among them;
    (b) a range crossing tile borders, 45..108; (c) whole tiles, 64..191: the skip path; (d) keys of the ragged last tile; (e) key 0 (and 33):
    a first row without a visible key; (f) nothing; (g) cached keys (cache form; a packed case drops nothing there)."""
    out = []
    for off, tot in zip(case.offs, case.tot):
        m = np.zeros(tot, dtype=bool)
        if pattern == "a":
            idx = [5, 31, 32, 63, 64, 100, 127, 128, 200]
        elif pattern == "b":
            idx = range(45, 109)
        elif pattern == "c":
            idx = range(64, 192)
        elif pattern == "d":
            first = KT * ((tot - 1) // KT)
            idx = [j for j in range(max(first, 1), tot - 1) if (j - first) % 2 == 0] + [tot - 2]
        elif pattern == "e":
            idx = [0, 33]
        elif pattern == "f":
            idx = []
        elif pattern == "g":
            idx = list(range(10, off - 1, 3)) + [off - 1]
        else:
            raise ValueError(pattern)
        for j in idx:
            if 0 <= j < tot and (j > 0 or pattern == "e"):
                m[j] = True
        out.append(m)
    return out


def drop_words(drops, ld):
    """The kernel's word layout, one bit at a time: bit j & 63 of word [s][j >> 6] set = key j of sequence s is dropped.  int64 [n_seq, ld]
    (the same 64 bits the device reads as uint64)."""
    words = [[0] * ld for _ in drops]
    for s, m in enumerate(drops):
        assert -(-len(m) // KT) <= ld
        for j in np.nonzero(m)[0].tolist():
            words[s][j >> 6] |= 1 << (j & 63)
    return torch.tensor([[w - (1 << 64) if w >= (1 << 63) else w for w in row] for row in words], dtype=torch.int64).view(len(drops), ld)


def words_needed(case):
    """ceil((largest key offset + longest count) / 64): what aigv_attn_check asks of ld_drop."""
    return -(-(max(case.offs) + max(case.cnts)) // KT)


def visible_sets(case, s, drop):
    """bool [cnt, tot]: key j is visible to new row r of sequence s."""
    off, n, tot = case.offs[s], case.cnts[s], case.tot[s]
    return (np.arange(tot)[None, :] <= (off + np.arange(n))[:, None]) & ~drop[None, :]


def census(case, drops):
    """ExactCase.census under the masks: the same Q (zero) and V (one-hot of (j + phase) mod D, value 1 + kv head), K random with the
    dropped keys' rows set to BIG_K."""
    gen = torch.Generator().manual_seed(case.seed)
    q, k, v, exp = [], [], [], []
    for s, (n, t) in enumerate(zip(case.cnts, case.tot)):
        q.append(torch.zeros(n, case.h, case.D, dtype=BF))
        ks = (torch.randn(t, case.hk, case.D, generator=gen) * 1.5).to(BF)
        ks[torch.from_numpy(drops[s])] = BIG_K
        k.append(ks)
        vs = torch.zeros(t, case.hk, case.D, dtype=BF)
        j = torch.arange(t)
        for kh in range(case.hk):
            vs[j, kh, (j + int(case.phase[s, kh])) % case.D] = float(census_weight(kh))
        v.append(vs)
        vis = visible_sets(case, s, drops[s])                                   # [n, t]
        l = vis.sum(1)
        e = []
        for kh in range(case.hk):
            onehot = np.zeros((t, case.D), dtype=np.int64)
            onehot[np.arange(t), (np.arange(t) + int(case.phase[s, kh])) % case.D] = census_weight(kh)
            e.append(census_bits(vis.astype(np.int64) @ onehot, l, "prefill"))
        exp.append(torch.from_numpy(np.repeat(np.stack(e, 1), case.g, axis=1)))      # [n, h, D]
    return ExactData(case, q, k, v, torch.cat(exp))


def chosen_key(case, s, drop):
    """c*: the largest un-dropped key <= max(offset, 1) (and inside the sequence), or None."""
    for j in range(min(max(case.offs[s], 1), case.tot[s] - 1), -1, -1):
        if not drop[j]:
            return j
    return None


def selector(case, drops):
    """-> ExactData with pi [cnt, h] per sequence (-1: the row has no visible key, its output is zero)."""
    gen = torch.Generator().manual_seed(case.seed + 1)
    q, k, v, exp, pis = [], [], [], [], []
    kv_of = torch.arange(case.h) // case.g
    for s, (n, t) in enumerate(zip(case.cnts, case.tot)):
        drop, off = drops[s], case.offs[s]
        cstar = chosen_key(case, s, drop)
        mask = np.arange(case.hk) & ((1 << code_bits(t)) - 1)
        key_code = np.arange(t)
        if cstar is not None:
            key_code = np.where(drop, cstar, key_code)                            # the decoys
        k.append(torch.from_numpy(codes(key_code[:, None] ^ mask[None, :], t, case.D)).to(BF))
        vs = torch.randn(t, case.hk, case.D, generator=gen).to(BF)
        v.append(vs)
        pi = np.full((n, case.h), -1, dtype=np.int64)
        for r in range(n):
            if cstar is not None and cstar <= off + r:
                pi[r] = cstar
            elif not drop[0]:
                pi[r] = 0                                                          # (a first row in front of c*: no dropped key is visible to it)
        q.append(torch.from_numpy(codes(np.maximum(pi, 0) ^ np.repeat(mask, case.g)[None, :], t, case.D)).to(BF))
        e = vs[torch.from_numpy(np.maximum(pi, 0)), kv_of[None, :]].contiguous().view(torch.int16).clone()
        e[torch.from_numpy(pi < 0)] = 0
        exp.append(e)
        pis.append(pi)
    return ExactData(case, q, k, v, torch.cat(exp), pis)


def waves_written(lens, q_tail):
    """AttnArgs::q_tail (kernels.h): whole 32-row waves in front of the consumed rows write nothing; every other row is computed."""
    keep = []
    for n in lens:
        r = torch.arange(n)
        keep.append((r // 32) * 32 + 32 > n - q_tail if q_tail else torch.ones(n, dtype=torch.bool))
    return torch.cat(keep)


def masked_attention(q, k, v, off, drop, post_div, dtype, ignore_mask=False):
    """ONE sequence, q [n, h, D], k / v [tot, hk, D]: causal attention of the n new rows behind `off` cached keys with the keys `drop` hidden,
    as the reference hides them (an additive finfo.min on the masked scores).  float64 -> truth; bf16 -> the reference's eager rounding
    points (scores in bf16, softmax in fp32, P cast back).  -> [n, h, D] in `dtype`."""
    n, h = q.shape[0], q.shape[1]
    rep = h // k.shape[1]
    qq = q.transpose(0, 1).to(dtype)
    kk = k.transpose(0, 1).repeat_interleave(rep, 0).to(dtype)
    vv = v.transpose(0, 1).repeat_interleave(rep, 0).to(dtype)
    s = (qq @ kk.transpose(1, 2)) / post_div
    hide = torch.arange(k.shape[0])[None, :] > (off + torch.arange(n))[:, None]
    if not ignore_mask:
        hide = hide | torch.from_numpy(np.asarray(drop))[None, :]
    s = s.masked_fill(hide[None], torch.finfo(dtype).min)
    p = torch.softmax(s, -1, dtype=torch.float32).to(BF) if dtype == BF else torch.softmax(s, -1)
    o = p @ vv
    o = o.masked_fill(hide.all(1)[None, :, None], 0)            # a row without a visible key: zeros (the kernel's convention)
    return o.transpose(0, 1)


def random_case(case, seed=0):
    """Seeded random bf16 q / k / v of a case's shapes, with a late large key per sequence so that the online-softmax rescale runs."""
    gen = torch.Generator().manual_seed(9000 + case.seed % 1000 + seed)
    q, k, v = [], [], []
    for n, t in zip(case.cnts, case.tot):
        q.append((torch.randn(n, case.h, case.D, generator=gen) * 1.5).to(BF))
        ks = (torch.randn(t, case.hk, case.D, generator=gen) * 1.5).to(BF)
        if t > 8:
            ks[(2 * t) // 3] *= 6.0
        k.append(ks)
        v.append(torch.randn(t, case.hk, case.D, generator=gen).to(BF))
    return ExactData(case, q, k, v, None)


POST = math.sqrt(D)
