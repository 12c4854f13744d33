"""Host references of the InternViT attention map (csrc/vitmap.hip; aigv_op_vit_attention_map / aigv_vit_attention_arm /
``model.vit_attention``), shared by tests/test_vit_attention_cpu.py and tests/test_gpu_vit_attention.py.

The mapped quantity, for frame f, head h, query row i, key j: acc_ij = the fp32 accumulation of the exact bf16 products q_i . k_j,
s_ij = acc_ij / sqrtf(D), m_i = max_j s_ij, e_ij = expf(s_ij - m_i), total_i = the fp32 sum of the e_ij, p_ij = e_ij / total_i; the head mean is
(p0 + p1 + ... in ascending h, from +0.0) / n_heads, one fp32 division.

* ``truth``: float64 softmax of every row over all S keys of its own frame, per head [n_seq, H, S, S];
* ``definition_fp32``: the quantity above evaluated step by step in fp32 on the host.  It is the kernel's result bit for bit wherever every step
  is exact or rounds once in a way that does not depend on the summation order: acc an integer below 2^24, all e_ij in {0, 1} - the census and
  the selector.  (float64 cannot serve there: exp(-128) is 2.6e-56 in float64 and exactly 0 in fp32.)
* ``head_mean_chain``: the documented fp32 chain over per-head maps;
* the census (Q = 0: every e is 1, total the integer S, p = fl(1 / S)), the one-hot selector and the random case;
* ``per_head_bound`` / ``head_mean_bound``: derived the way ``attention_map_reference.rows_bound`` derives its bound - ``mass_bound`` with every
  key its own bin (a bin of ONE key: n_seg = 1) at eps = 2 x ``score_bound`` (the MFMA accumulation's rounding mode is not documented, so a step
  of the accumulation is allowed one ulp instead of the half ulp of a correctly rounded fmaf), plus, for the mean, n_heads + 1 half-ulps of
  the mean: n_heads - 1 additions (0 + p is exact) of non-negative terms, whose running sums never exceed the final one, and one division -
  rounded up to n_heads + 1.  No measured number is involved.
* the model level: ``oracle_probs`` restates the q / k / softmax lines of ``oracle.vit_attention``; ``oracle_maps`` composes the oracle's own
  ``vit_embeddings`` / ``vit_norm`` / ``vit_layer`` around it; ``scale_qk`` is the seeded draw with its Q and K thirds scaled."""
import math

import torch

import score_attention_reference as R

BF = torch.bfloat16
# (n_seq, S, n_heads, D): one full tile plus a one-key tail, a non-power-of-two head count, a single key, both head dims, the production row count
SHAPES = [(3, 33, 4, 64), (2, 69, 3, 64), (1, 1, 2, 64), (2, 33, 2, 128), (2, 1025, 2, 64)]
SELECT_Q = 16.0
# the selected key's entry: score 16 * 64 / sqrt(64) = 128 against 0 at D = 64; at D = 128 the same entry would give 1024 / sqrt(128) = 90.5, short
# of R.EXP_UNDERFLOW = 104, so the key is 128 there: 2048 / sqrt(128) = 181.  Both are powers of two, exact in bf16, the products exact in fp32
SELECT_K = {64: 64.0, 128: 128.0}


def fused_rows(q, k, v=None):
    """q, k [n_seq, S, H, D] bf16 -> the layer's fused rows [n_seq * S, 3 H D]: Q | K | V thirds, head h at column h D of its third."""
    n, S, H, D = q.shape
    v = torch.zeros_like(q) if v is None else v
    return torch.cat([q.reshape(n * S, H * D), k.reshape(n * S, H * D), v.reshape(n * S, H * D)], 1).contiguous()


def truth(q, k):
    """float64 [n_seq, H, S, S]."""
    d = q.shape[-1]
    s = torch.einsum("nihd,njhd->nhij", q.double(), k.double()) / math.sqrt(d)
    return torch.softmax(s, -1)


def definition_fp32(q, k):
    """The documented chain in fp32 (module docstring): fp32 [n_seq, H, S, S].  acc is taken from float64 and cast - exact where acc is exactly
    representable - and the total is torch's fp32 sum: exact, so order-free, where every e is 0 or 1."""
    d = q.shape[-1]
    acc = torch.einsum("nihd,njhd->nhij", q.double(), k.double()).float()
    s = acc / torch.tensor(math.sqrt(d), dtype=torch.float32)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def head_mean_chain(p):
    """fp32 [n, H, S, S] -> fp32 [n, S, S]: p0 + p1 + ... in ascending h starting from +0.0, then ONE division by n_heads."""
    assert p.dtype == torch.float32
    acc = torch.zeros_like(p[:, 0])
    for h in range(p.shape[1]):
        acc = acc + p[:, h]
    return acc / torch.tensor(float(p.shape[1]), dtype=torch.float32)


# ---- key census -------------------------------------------------------------------------------------------------------------------------------
def census_value(S):
    """fl(1 / S): one fp32 division of 1 by the integer total."""
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(S), dtype=torch.float32)


def census_case(shape, seed=11):
    """Q = 0, random K: (q, k) bf16 [n_seq, S, H, D]."""
    n, S, H, D = shape
    gen = torch.Generator().manual_seed(seed + S + H)
    return torch.zeros(n, S, H, D, dtype=BF), torch.randn(n, S, H, D, generator=gen).to(BF)


def census_expect(shape, per_head):
    n, S, H, D = shape
    p = census_value(S).expand(n, H, S, S).contiguous()
    return p if per_head else head_mean_chain(p)


# ---- one-hot selector -------------------------------------------------------------------------------------------------------------------------
def wanted_keys(S):
    """Key 0, key S - 1 and both sides of every 32-key tile edge inside the frame."""
    return sorted({0, S - 1} | {j for t in range(32, S, 32) for j in (t - 1, t)})


def selector_keys(shape):
    """int64 [n_seq, H, S]: the key row i of (frame, head) selects.  Row i asks at column i % D, so the rows that share a column share their
    key: column c of (f, h) selects wanted_keys(S)[(c + 17 h + 33 f) % len] - heads (and frames) choose different keys, and together the rows
    select every wanted key (tests/test_vit_attention_cpu.py checks that)."""
    n, S, H, D = shape
    W = wanted_keys(S)
    sel = torch.empty(n, H, S, dtype=torch.long)
    for f in range(n):
        for h in range(H):
            for i in range(S):
                sel[f, h, i] = W[(i % D + 17 * h + 33 * f) % len(W)]
    return sel


def selector_case(shape):
    """(q, k, sel): the query of (f, i, h) is SELECT_Q at column i % D and 0 elsewhere; key sel[f, h, i] is SELECT_K[D] at that column, every other
    key 0 there.  Scores: >= 128 at the selected key, 0 at every other one, and expf(-128) is exactly 0 in fp32 (R.EXP_UNDERFLOW)."""
    n, S, H, D = shape
    sel = selector_keys(shape)
    q, k = torch.zeros(n, S, H, D, dtype=BF), torch.zeros(n, S, H, D, dtype=BF)
    assert SELECT_Q * SELECT_K[D] / math.sqrt(D) >= R.EXP_UNDERFLOW
    for i in range(S):
        q[:, i, :, i % D] = SELECT_Q
    for f in range(n):
        for h in range(H):
            for c in range(min(S, D)):
                k[f, sel[f, h, c], h, c] = SELECT_K[D]
    return q, k, sel


def selector_expect(shape, sel, per_head):
    """Exactly one-hot per head; the head mean exactly (the number of heads selecting the key) / n_heads."""
    n, S, H, D = shape
    one = torch.nn.functional.one_hot(sel, S).float()                       # [n, H, S(i), S(j)]
    return one if per_head else one.sum(1) / torch.tensor(float(H), dtype=torch.float32)


# ---- random data and the derived bound --------------------------------------------------------------------------------------------------------
def random_case(shape, seed=23):
    n, S, H, D = shape
    gen = torch.Generator().manual_seed(seed + 3 * S + H + D)
    return torch.randn(n, S, H, D, generator=gen).to(BF), torch.randn(n, S, H, D, generator=gen).to(BF)


def score_bounds(q, k):
    """float64 [n_seq, H, S]: ``score_attention_reference.score_bound`` of every row over all keys of its frame (vectorised; the CPU test holds
    it against that function row by row)."""
    d = q.shape[-1]
    mag = torch.einsum("nihd,njhd->nhij", q.double().abs(), k.double().abs()).max(-1).values
    return (d + 2) * 2.0 ** -24 * mag / math.sqrt(d)


def per_head_bound(p, eps, extra_rel=0.0):
    """p float64 [n, H, S, S], eps [n, H, S] = score_bounds -> the bound on |kernel - p| per element: ``R.mass_bound`` with every key its own bin
    (n_seg = 1: a bin of one key) over n_keys = S, at 2 x eps."""
    S = p.shape[-1]
    rel = torch.expm1(2 * (2 * eps + extra_rel))[..., None] + R.EXP_C * 2.0 ** -24 * (S + 1)
    return p * rel + 2.0 ** -24


def head_mean_bound(p, eps, extra_rel=0.0):
    """The mean over the heads of ``per_head_bound`` plus n_heads + 1 half-ulps of the mean for the chain (module docstring)."""
    H = p.shape[1]
    return per_head_bound(p, eps, extra_rel).mean(1) + (H + 1) * 2.0 ** -24 * p.mean(1)


# ---- model level ------------------------------------------------------------------------------------------------------------------------------
# What multiplies the Q and K thirds of every qkv.weight / qkv.bias of the seeded N(0, 0.02^2) draw - and, in the tower with the full-width QK
# RMSNorm, q_norm.weight and k_norm.weight, which alone set the size of Q and K there - so that the oracle's fp32 maps are not near-uniform:
# median row maximum >= 8 / S (found on the CPU; the GPU test asserts the condition; profiles/vit_attention_cost.txt records the values)
QK_SCALE = {"plain": 5.5, "qknorm": 1.15}
# the seeded draw, the synthetic frames and the tower's depth the factors were found for.  The oracle's own bf16 / fp32 difference grows with the
# peak of the maps about as fast as the difference between two frames does, so the 20 x conditions of the oracle test leave little room: these
# seeds give them about 29 x on the CPU oracle (scanned over 4 draws x 3 frame sets; the oracle's bf16 matmul differs a little from host to host)
MODEL_SEED, FRAME_SEED, MODEL_LAYERS = 74, 306, 3


def scale_qk(sd, cfg, factor):
    v = cfg.vision_config
    Hv = v.hidden_size
    out = dict(sd)
    for l in range(v.num_hidden_layers):
        p = f"vision_model.encoder.layers.{l}.attn."
        for name in ("qkv.weight", "qkv.bias"):
            if p + name in out:
                t = out[p + name].clone()
                t[:2 * Hv] = (t[:2 * Hv].float() * factor).to(t.dtype)
                out[p + name] = t
        if v.qk_normalization:
            for name in ("q_norm.weight", "k_norm.weight"):
                out[p + name] = (out[p + name].float() * factor).to(out[p + name].dtype)
    return out


def zero_q(sd, cfg):
    """The Q third of every qkv.weight and qkv.bias zeroed: every query is 0 (the QK RMSNorm of a zero row is zero), every map the census."""
    v = cfg.vision_config
    out = dict(sd)
    for l in range(v.num_hidden_layers):
        for name in ("qkv.weight", "qkv.bias"):
            key = f"vision_model.encoder.layers.{l}.attn.{name}"
            if key in out:
                t = out[key].clone()
                t[:v.hidden_size] = 0
                out[key] = t
    return out


def oracle_probs(O, sd, cfg, prefix, x):
    """The q / k / softmax lines of ``oracle.vit_attention`` (oracle/oracle.py), restated: the eager probabilities [F, n_heads, S, S] in x's
    dtype, and q, k [F, n_heads, S, d] as the softmax consumes them (q unscaled)."""
    v = cfg.vision_config
    nf, n, c = x.shape
    nh = v.num_attention_heads
    d = c // nh
    qkv = torch.nn.functional.linear(x, sd[prefix + "qkv.weight"], sd.get(prefix + "qkv.bias"))
    qkv = qkv.reshape(nf, n, 3, nh, d).permute(2, 0, 3, 1, 4)
    q, k = qkv[0], qkv[1]
    if v.qk_normalization:
        q = O.rms_norm_cast_then_scale(q.transpose(1, 2).flatten(-2, -1), sd[prefix + "q_norm.weight"], v.layer_norm_eps).view(nf, n, nh, d).transpose(1, 2)
        k = O.rms_norm_cast_then_scale(k.transpose(1, 2).flatten(-2, -1), sd[prefix + "k_norm.weight"], v.layer_norm_eps).view(nf, n, nh, d).transpose(1, 2)
    att = (q * (d ** -0.5)) @ k.transpose(-2, -1)
    return att.softmax(dim=-1), q, k


def oracle_maps(O, sd, cfg, pixel_values, layers, dtype):
    """{layer: (probabilities [F, n_heads, S, S], q, k)} of the CPU oracle run in ``dtype`` (bf16: the reference's own arithmetic; fp32: the same
    weights and frames widened), for the layers asked for."""
    sd = {k: (t.to(dtype) if t.is_floating_point() else t) for k, t in sd.items() if k.startswith("vision_model.")}
    x = O.vit_embeddings(sd, cfg, pixel_values.to(dtype))
    out = {}
    for i in range(max(layers) + 1):
        p = f"vision_model.encoder.layers.{i}."
        if i in layers:
            out[i] = oracle_probs(O, sd, cfg, p + "attn.", O.vit_norm(sd, cfg, p + "norm1", x))
        x = O.vit_layer(sd, cfg, i, x)
    return out
