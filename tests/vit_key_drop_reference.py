"""Host-side generators of the NON-causal key-drop attention tests (no GPU; torch and numpy only): the two exact constructions of
tests/attention_exact_reference.py - the key census and the one-hot selector - under a per-key "dropped" mask where every query row sees every
un-dropped key of its sequence (InternViT's attention), the drop patterns, float64 / eager-bf16 references of a masked sequence, and a masked
eager InternViT layer stack composed from the oracle's own functions.  The word layout is key_drop_reference.drop_words', unchanged.

Visibility.  Key j is visible to EVERY row of its sequence iff it is not dropped: ``~drop``.  A dropped key is hidden from its own row too; a
sequence whose every key is dropped has all-zero output rows.

Census under a mask.  Q = 0, so every visible score is exactly 0 and the output of every row restates the prefill kernel's normalisation of
w x #{j not dropped, (j + phase) mod D = c} over l = #{j not dropped} (the key-split merge multiplies by exp2(0) = 1; a wave that saw no key is
merged with weight 0).  The K rows of dropped keys are key_drop_reference.BIG_K: finite, and they must not matter.

Selector under a mask.  One un-dropped key c* per sequence is the chosen key of every row and head: the LAST un-dropped key of even sequences (a
late maximum: every state in front of it is rescaled by alpha = 0; in the key split it sits in one wave's walk and the three others merge with
weight 0) and the FIRST un-dropped key of odd ones.  EVERY dropped key carries the code of c* - a decoy whose score ties the chosen key's
exactly: a kernel that ignores one mask bit returns a blend of V rows instead of V[c*]."""
import numpy as np
import torch

from attention_exact_reference import BF, KT, ExactCase, ExactData, census_bits, census_weight, codes, code_bits
from attention_reference import check_sequence      # noqa: F401  (the project's own bar for random data: re-exported for the GPU file)
from key_drop_reference import BIG_K, drop_words     # noqa: F401  (the word layout as a naive loop: re-exported)

# (name, D, lengths): n_heads = n_kv_heads = 2 everywhere.  257 = two full query blocks + the key-split row, five key tiles of which the last holds
# one key; 1025 = 17 tiles, four (five for wave 0) per key-split wave; [200, 64, 1]: no key split twice, then a one-row sequence that key-splits
# over a single tile
CASES = [("nc-257x2-d64", 64, [257, 257]), ("nc-257x2-d128", 128, [257, 257]), ("nc-1025-d64", 64, [1025]), ("nc-200-64-1-d64", 64, [200, 64, 1]),
         ("nc-200-64-1-d128", 128, [200, 64, 1])]
CASE_IDS = [c[0] for c in CASES]
PATTERNS = "abcdefghi"
EIGHT_WAVES = "nc-257x2-d64"        # the 8-wave form is checked once
LEAD_KEY = ("nc-257x2-d64", "nc-257x2-d128", "nc-1025-d64")      # key counts 64 j + 1: where the lead-key knob would change the unmasked walk


def make_case(name):
    n, D, lens = CASES[CASE_IDS.index(name)]
    return ExactCase(n, D, False, 2, 2, [0] * len(lens), lens)


def one_pattern(S, pattern):
    m = np.zeros(S, dtype=bool)
    if pattern == "a":          # scattered bits, the lane-boundary keys 31, 32, 63 and the tile border 64 among them
        idx = [5, 31, 32, 63, 64, 100, 127, 128, 200]
    elif pattern == "b":        # a range crossing tile borders
        idx = range(45, 109)
    elif pattern == "c":        # whole tiles: the skip path; at S = 257 every tile of key-split waves 1 and 2
        idx = range(64, 192)
    elif pattern == "d":        # the last key alone: at S = 64 j + 1 the ragged tile is left without a visible key
        idx = [S - 1]
    elif pattern == "e":        # every key but 0
        idx = range(1, S)
    elif pattern == "f":        # nothing
        idx = []
    elif pattern == "g":        # keys 0 and 33
        idx = [0, 33]
    elif pattern == "h":        # every key: the rows are zeros
        idx = range(S)
    else:
        raise ValueError(pattern)
    for j in idx:
        if 0 <= j < S:
            m[j] = True
    return m


def drop_sets(case, pattern):
    """-> [bool array over the keys of every sequence].  (i): a different pattern per sequence - a, nothing, b, in turn - so sequence 1 is unmasked."""
    if pattern == "i":
        return [one_pattern(S, "afb"[s % 3]) for s, S in enumerate(case.tot)]
    return [one_pattern(S, pattern) for S in case.tot]


def words_needed(case):
    """ceil(longest sequence / 64): what aigv_attn_check asks of ld_drop in the non-causal form."""
    return -(-max(case.tot) // KT)


def visible_count(drop):
    return int((~drop).sum())


def census(case, drops):
    """ExactCase.census under the masks: Q zero, V the one-hot of (j + phase) mod D with value 1 + kv head, K random with the dropped keys' rows BIG_K."""
    gen = torch.Generator().manual_seed(case.seed)
    q, k, v, exp = [], [], [], []
    for s, t in enumerate(case.tot):
        q.append(torch.zeros(t, case.h, case.D, dtype=BF))
        ks = (torch.randn(t, case.hk, case.D, generator=gen) * 1.5).to(BF)
        ks[torch.from_numpy(drops[s])] = BIG_K
        k.append(ks)
        vs = torch.zeros(t, case.hk, case.D, dtype=BF)
        j = torch.arange(t)
        for kh in range(case.hk):
            vs[j, kh, (j + int(case.phase[s, kh])) % case.D] = float(census_weight(kh))
        v.append(vs)
        vis = (~drops[s]).astype(np.int64)[None, :].repeat(t, 0)                 # [rows, keys]: every row sees the same keys
        l = vis.sum(1)
        e = []
        for kh in range(case.hk):
            onehot = np.zeros((t, case.D), dtype=np.int64)
            onehot[np.arange(t), (np.arange(t) + int(case.phase[s, kh])) % case.D] = census_weight(kh)
            e.append(census_bits(vis @ onehot, l, "prefill"))
        exp.append(torch.from_numpy(np.repeat(np.stack(e, 1), case.g, axis=1)))      # [rows, h, D]
    return ExactData(case, q, k, v, torch.cat(exp))


def chosen_key(s, drop):
    """c*: the last un-dropped key of an even sequence, the first of an odd one, or None."""
    keys = np.nonzero(~drop)[0]
    if not len(keys):
        return None
    return int(keys[-1] if s % 2 == 0 else keys[0])


def selector(case, drops):
    """-> ExactData with pi [rows, h] per sequence (-1: no visible key, the output is zero)."""
    gen = torch.Generator().manual_seed(case.seed + 1)
    q, k, v, exp, pis = [], [], [], [], []
    kv_of = torch.arange(case.h) // case.g
    for s, t in enumerate(case.tot):
        drop = drops[s]
        cstar = chosen_key(s, drop)
        mask = np.arange(case.hk) & ((1 << code_bits(t)) - 1)
        key_code = np.arange(t)
        if cstar is not None:
            key_code = np.where(drop, cstar, key_code)                           # the decoys
        k.append(torch.from_numpy(codes(key_code[:, None] ^ mask[None, :], t, case.D)).to(BF))
        vs = torch.randn(t, case.hk, case.D, generator=gen).to(BF)
        v.append(vs)
        pi = np.full((t, case.h), -1 if cstar is None else cstar, dtype=np.int64)
        q.append(torch.from_numpy(codes(np.maximum(pi, 0) ^ np.repeat(mask, case.g)[None, :], t, case.D)).to(BF))
        e = vs[torch.from_numpy(np.maximum(pi, 0)), kv_of[None, :]].contiguous().view(torch.int16).clone()
        e[torch.from_numpy(pi < 0)] = 0
        exp.append(e)
        pis.append(pi)
    return ExactData(case, q, k, v, torch.cat(exp), pis)


def selector_margin_octaves(case, drops):
    """The smallest lead, in octaves of the kernel's exp2 (log2(e) x pre / post), of the chosen score over every other VISIBLE key's score."""
    data = selector(case, drops)
    worst = np.inf
    for s, t in enumerate(case.tot):
        if chosen_key(s, drops[s]) is None:
            continue
        for hq in range(case.h):
            sc = data.q[s][:, hq].double() @ data.k[s][:, hq // case.g].double().T       # [rows, keys]
            sc = sc[:, torch.from_numpy(~drops[s])]
            top = sc.max(1).values
            rest = sc.masked_fill(sc == top[:, None], -np.inf).max(1).values
            if bool(torch.isfinite(rest).any()):                                           # (a lone visible key leads nothing)
                lead = (top - rest)[torch.isfinite(rest)].min().item()
                worst = min(worst, lead * case.pre / case.post * 1.4426950408889634)
            assert int((sc == top[:, None]).sum(1).max()) == 1                            # no visible tie
    return worst


def masked_attention(q, k, v, drop, pre, dtype):
    """ONE sequence, q [n, h, D], k / v [n, h, D]: non-causal attention with the keys `drop` hidden from every row.  float64 -> truth; bf16 -> the
    reference's eager rounding points (modeling_intern_vit.py:143-160: q * scale, the score matrix and the softmax in bf16).  A sequence without a
    visible key gives zeros (the kernel's convention).  -> [n, h, D] in `dtype`."""
    qq = (q.transpose(0, 1).to(dtype) * pre)
    kk, vv = k.transpose(0, 1).to(dtype), v.transpose(0, 1).to(dtype)
    hide = torch.from_numpy(np.asarray(drop))
    if bool(hide.all()):
        return torch.zeros_like(q, dtype=dtype)
    s = (qq @ kk.transpose(1, 2)).masked_fill(hide[None, None, :], float("-inf"))
    o = s.softmax(-1) @ vv
    return o.transpose(0, 1)


def random_case(case, seed=0):
    """Seeded random bf16 q / k / v of a case's shapes, with a late large key per sequence so that the online-softmax rescale runs."""
    gen = torch.Generator().manual_seed(9100 + case.seed % 1000 + seed)
    q, k, v = [], [], []
    for t in case.tot:
        q.append((torch.randn(t, case.h, case.D, generator=gen) * 1.5).to(BF))
        ks = (torch.randn(t, case.hk, case.D, generator=gen) * 1.5).to(BF)
        if t > 8:
            ks[(2 * t) // 3] *= 6.0
        k.append(ks)
        v.append(torch.randn(t, case.hk, case.D, generator=gen).to(BF))
    return ExactData(case, q, k, v, None)


# ---- the masked eager InternViT stack ---------------------------------------------------------------------------------------------------
def patch_keys(patch_drop):
    """bool [F, G, G] over patches -> bool [F, G * G + 1] over the keys of a frame: key 0 (cls) never dropped, key 1 + G y + x = patch (y, x)."""
    pd = torch.as_tensor(patch_drop)
    return torch.cat([torch.zeros(pd.shape[0], 1, dtype=torch.bool), pd.reshape(pd.shape[0], -1)], 1)


def patch_words_naive(patch_drop):
    """The words of model.vit_tokens(patch_drop=...), one bit at a time."""
    keys = patch_keys(patch_drop).numpy()
    return drop_words(list(keys), -(-keys.shape[1] // KT))


def masked_vit_attention(O, sd, cfg, prefix, x, hide):
    """oracle.vit_attention with the keys `hide` [F, S] of every frame removed from every row's softmax: the same statements in the same dtype
    (the reference's rounding points when x is bf16), one masked_fill in front of the softmax."""
    F = torch.nn.functional
    v = cfg.vision_config
    nf, n, c = x.shape
    nh = v.num_attention_heads
    d = c // nh
    qkv = F.linear(x, sd[prefix + "qkv.weight"], sd.get(prefix + "qkv.bias"))
    qkv = qkv.reshape(nf, n, 3, nh, d).permute(2, 0, 3, 1, 4)
    q, k, vv = qkv[0], qkv[1], qkv[2]
    if v.qk_normalization:
        q = O.rms_norm_cast_then_scale(q.transpose(1, 2).flatten(-2, -1), sd[prefix + "q_norm.weight"], v.layer_norm_eps).view(nf, n, nh, d).transpose(1, 2)
        k = O.rms_norm_cast_then_scale(k.transpose(1, 2).flatten(-2, -1), sd[prefix + "k_norm.weight"], v.layer_norm_eps).view(nf, n, nh, d).transpose(1, 2)
    att = (q * (d ** -0.5)) @ k.transpose(-2, -1)
    att = att.masked_fill(hide[:, None, None, :], float("-inf")).softmax(dim=-1)
    y = (att @ vv).transpose(1, 2).reshape(nf, n, c)
    return F.linear(y, sd[prefix + "proj.weight"], sd[prefix + "proj.bias"])


def masked_vit_forward(O, sd, cfg, pixel_values, patch_drop, window=None, n_layers=None):
    """oracle.vit_forward with the patches `patch_drop` [F, G, G] hidden as keys in the attention of layers lo <= l < hi (None: every layer);
    norms, MLP and layer scales are the oracle's own functions.  -> the last hidden state [F, S, Hv] after n_layers layers (None: all)."""
    n_layers = cfg.vision_config.num_hidden_layers if n_layers is None else n_layers
    lo, hi = (0, n_layers) if window is None else window
    hide = patch_keys(patch_drop)
    x = O.vit_embeddings(sd, cfg, pixel_values)
    for i in range(n_layers):
        p = f"vision_model.encoder.layers.{i}."
        h = O.vit_norm(sd, cfg, p + "norm1", x)
        a = masked_vit_attention(O, sd, cfg, p + "attn.", h, hide) if lo <= i < hi else O.vit_attention(sd, cfg, p + "attn.", h)
        x = x + a * sd[p + "ls1"]
        x = x + O.vit_mlp(sd, p + "mlp.", O.vit_norm(sd, cfg, p + "norm2", x)) * sd[p + "ls2"]
    return x
