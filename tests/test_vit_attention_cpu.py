"""InternViT attention map without a GPU: the ABI (header, prototypes, the op's host refusals), ``eval_utils.vit_rollout`` /
``pixel_heatmaps`` on their exact cases, and the consistency of the references of tests/vit_attention_reference.py with themselves.
tests/test_gpu_vit_attention.py runs the kernels and the armed pass."""
import ctypes
import os
import re

import pytest
import torch

import score_attention_reference as R
import vit_attention_reference as V
from aigv_assessor_amd import build, eval_utils, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aigv_vit_attention_arm", "aigv_op_vit_attention_map")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_header_prototypes_exports_and_host_refusals():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I = native._P, native._I
    assert native.PROTOTYPES["aigv_vit_attention_arm"] == (I, [P, P, I, I, I])
    assert native.PROTOTYPES["aigv_op_vit_attention_map"] == (I, [P, I, P, I, I, I, I, I, P, I, P, P])
    assert "vitmap.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vitmap.hip"))
    lib = native.load()
    for name in NAMES:
        assert name in note and hasattr(lib, name), name
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(native.PROTOTYPES[name][1]), name
    doc = header[header.index("InternViT attention map: the full, NON-causal"):header.index("int aigv_vit_attention_arm")]
    kernel = open(os.path.join(build.CSRC, "vitmap.hip")).read()
    for phrase in ("acc_ij", "s_ij", "m_i", "e_ij", "total_i", "p_ij", "starting from +0.0", "q_prescale"):
        assert phrase in doc and phrase in kernel.split("#include")[0], phrase
    for phrase in ("ALWAYS fp32", "one fp32 division", "No atomics", "select_layer", "disarms on every way out"):
        assert phrase in doc, phrase
    tiles = open(os.path.join(build.CSRC, "qk_tiles.h")).read()                                             # the score tiles' product: shared with attnmap.hip
    assert '#include "qk_tiles.h"' in kernel and "qk_tiles.h" in build.HEADERS and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in tiles
    assert "atomic" not in kernel.split('#include "kernels.h"')[1] and "atomic" not in tiles.split("#pragma once")[1]
    # host refusals: before any pointer is used (a small aligned HOST buffer stands for every operand; no accepted call is made)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    p += 16 - p % 16
    last = lambda: (lib.aigv_last_error(None) or b"").decode()
    good = dict(q=p, ldq=3 * 128, k=p, ldk=3 * 128, n_seq=1, S=33, H=2, D=64, out=p, per_head=0, stats=p)

    def call(**over):
        a = dict(good, **over)
        return lib.aigv_op_vit_attention_map(a["q"], a["ldq"], a["k"], a["ldk"], a["n_seq"], a["S"], a["H"], a["D"], a["out"], a["per_head"], a["stats"], None)

    for over, word in ((dict(q=None), "null operand"), (dict(k=None), "null operand"), (dict(out=None), "null operand"), (dict(stats=None), "null operand"),
                       (dict(D=96), "head_dim"), (dict(H=0), "n_heads"), (dict(H=65), "n_heads"), (dict(n_seq=0), "frames"), (dict(n_seq=65536), "frames"),
                       (dict(S=0), "rows of a frame"), (dict(S=32769), "rows of a frame"), (dict(ldq=120), "strides too small"), (dict(ldk=64), "strides too small"),
                       (dict(ldq=3 * 128 + 4), "multiple of 8"), (dict(q=p + 2), "16-byte aligned"), (dict(k=p + 8), "16-byte aligned"),
                       (dict(out=p + 2), "4-byte"), (dict(stats=p + 4), "8-byte")):
        assert call(**over) == -1 and word in last() and "aigv_op_vit_attention_map" in last(), (over, last())
    assert lib.aigv_vit_attention_arm(None, p, 0, 1, 0) == -1 and "null context" in last()


# ---- vit_rollout ------------------------------------------------------------------------------------------------------------------------------
def perm_matrix(perm):
    return torch.nn.functional.one_hot(torch.as_tensor(perm), len(perm)).float()


def test_vit_rollout_exact_cases_and_refusals():
    gen = torch.Generator().manual_seed(3)
    F, L, S = 2, 3, 17
    att = torch.softmax(torch.randn(F, L, S, S, generator=gen), -1)
    eye = torch.eye(S)
    assert torch.equal(eval_utils.vit_rollout(att, alpha=1.0), eye.expand(F, S, S))                        # alpha = 1: I exactly
    perms = [[torch.randperm(S, generator=gen).tolist() for _ in range(L)] for _ in range(F)]
    pm = torch.stack([torch.stack([perm_matrix(p) for p in per]) for per in perms])
    want = torch.stack([pm[f, 2] @ pm[f, 1] @ pm[f, 0] for f in range(F)])                                   # the deepest layer leftmost
    assert torch.equal(eval_utils.vit_rollout(pm, alpha=0.0), want)
    assert torch.equal(eval_utils.vit_rollout(pm, alpha=0.0, layers=[2, 0]), torch.stack([pm[f, 0] @ pm[f, 2] for f in range(F)]))      # the order given
    # against the float64 product, and rows that sum to 1 keep summing to 1
    roll = eval_utils.vit_rollout(att, alpha=0.5)
    step = lambda f, l: 0.5 * eye.double() + 0.5 * att[f, l].double()
    ref = torch.stack([step(f, 2) @ (step(f, 1) @ step(f, 0)) for f in range(F)])
    assert roll.dtype == att.dtype and tuple(roll.shape) == (F, S, S) and torch.equal(roll, ref.float())
    assert (roll.double().sum(-1) - 1).abs().max().item() <= S * 2.0 ** -23
    for bad, word in ((dict(att=att[0]), r"\[F, L, S, S\]"), (dict(att=att[..., :5]), r"\[F, L, S, S\]"), (dict(att=att, alpha=1.5), "outside 0..1"),
                      (dict(att=att, alpha=-0.1), "outside 0..1"), (dict(att=att, layers=[3]), "layers"), (dict(att=att, layers=[]), "layers")):
        with pytest.raises(ValueError, match=word):
            eval_utils.vit_rollout(**bad)


# ---- pixel_heatmaps ---------------------------------------------------------------------------------------------------------------------------
def test_pixel_heatmaps_exact_cases_invariant_and_refusals():
    gen = torch.Generator().manual_seed(4)
    B, F, g = 2, 3, 4
    n, S = 2 * g, (2 * g) ** 2 + 1
    heat = torch.rand(B, F, g, g, generator=gen)
    heat = heat / heat.sum((1, 2, 3), keepdim=True)
    eye = torch.eye(S).expand(B * F, S, S)
    pix, cls = eval_utils.pixel_heatmaps(heat, eye)
    assert pix.dtype == cls.dtype == torch.float64 and tuple(pix.shape) == (B, F, n, n) and tuple(cls.shape) == (B, F)
    quarter = (heat.double() / 4).repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(pix, quarter) and torch.equal(cls, torch.zeros(B, F, dtype=torch.float64))          # identity: heat / 4 on the cell's four patches
    for r, c in ((0, 0), (1, 2), (g - 1, g - 1)):                                                           # ... patches (2r.., 2c..), stated once without the helper
        for y, x in ((2 * r, 2 * c), (2 * r, 2 * c + 1), (2 * r + 1, 2 * c), (2 * r + 1, 2 * c + 1)):
            assert pix[1, 2, y, x] == heat[1, 2, r, c].double() / 4
    # a permutation rollout moves every quarter exactly: row i passes its share to column perm[i]
    perms = [torch.randperm(S, generator=gen) for _ in range(B * F)]
    roll = torch.stack([perm_matrix(p.tolist()) for p in perms])
    pix, cls = eval_utils.pixel_heatmaps(heat, roll)
    for i in range(B * F):
        src = torch.cat([torch.zeros(1, dtype=torch.float64), quarter.view(B * F, n * n)[i]])               # (row 0, the cls row, carries no heat)
        want = torch.zeros(S, dtype=torch.float64)
        want[perms[i]] = src
        assert torch.equal(torch.cat([cls.view(-1)[i:i + 1], pix.view(B * F, n * n)[i]]), want), i
    # the invariant wherever the rollout's rows sum to 1
    soft = torch.softmax(3 * torch.randn(B * F, S, S, generator=gen).double(), -1)                         # (float64: the rows sum to 1 to float64 rounding)
    pix, cls = eval_utils.pixel_heatmaps(heat, soft)
    assert (pix.sum((2, 3)) + cls - heat.double().sum((2, 3))).abs().max().item() <= 4 * S * 2.0 ** -53
    assert cls.min().item() > 0
    for bad, word in (((heat[0], soft), "expected"), ((heat, soft[:, :, :5]), "expected"), ((heat, soft[:5]), "needs rollout"), ((heat[..., :3, :3], soft), "needs rollout")):
        with pytest.raises(ValueError, match=word):
            eval_utils.pixel_heatmaps(*bad)


# ---- the references' own consistency ----------------------------------------------------------------------------------------------------------
SMALL = [s for s in V.SHAPES if s[1] <= 69]


@pytest.mark.parametrize("shape", V.SHAPES)
def test_selector_keys_cover_every_tile_edge_and_heads_differ(shape):
    n, S, H, D = shape
    sel = V.selector_keys(shape)
    assert set(sel.unique().tolist()) >= set(V.wanted_keys(S)) >= {0, S - 1}
    assert all(j in V.wanted_keys(S) for t in range(32, S, 32) for j in (t - 1, t))
    if S > 1:
        assert (sel[:, 0] != sel[:, 1]).any()                                                              # heads choosing different keys
    assert V.SELECT_Q * V.SELECT_K[D] / D ** 0.5 >= max(R.EXP_UNDERFLOW, 128.0 if D == 64 else 0.0)
    assert torch.exp(torch.tensor(-R.EXP_UNDERFLOW, dtype=torch.float32)).item() == 0.0


@pytest.mark.parametrize("shape", SMALL)
def test_exact_cases_of_the_definition(shape):
    """The selector's truth is exactly one-hot and the census truth exactly fl(1 / S) - by the fp32 definition, and the float64 softmax agrees
    within its own range; the head mean of the selector is exactly count / n_heads."""
    n, S, H, D = shape
    q, k, sel = V.selector_case(shape)
    p = V.definition_fp32(q, k)
    assert torch.equal(p, V.selector_expect(shape, sel, True)) and set(p.unique().tolist()) <= {0.0, 1.0}
    assert (V.truth(q, k) - p.double()).abs().max().item() <= 1e-40
    mean = V.selector_expect(shape, sel, False)
    assert torch.equal(V.head_mean_chain(p), mean)
    assert (mean.double().sum(-1) - 1).abs().max().item() <= S * 2.0 ** -24
    q, k = V.census_case(shape)
    p = V.definition_fp32(q, k)
    assert torch.equal(p, V.census_expect(shape, True)) and (p == V.census_value(S)).all()
    assert V.census_value(S).item() == float(torch.tensor(1.0 / S, dtype=torch.float64).float())           # fl(1 / S): the correctly rounded quotient
    assert (V.census_expect(shape, False).double() - 1.0 / S).abs().max().item() <= (H + 1) * 2.0 ** -24 / S


@pytest.mark.parametrize("shape", SMALL)
def test_bounds_restate_the_shared_ones(shape):
    n, S, H, D = shape
    q, k = V.random_case(shape)
    eps = V.score_bounds(q, k)
    p = V.truth(q, k)
    assert (p.sum(-1) - 1).abs().max().item() <= 1e-12
    for f, i in ((0, 0), (n - 1, S - 1), (0, S // 2)):
        want = R.score_bound(q[f, i].double(), k[f])                                                       # [H]: the shared per-row bound
        assert torch.allclose(eps[f, :, i], want, rtol=1e-12, atol=0)
        for h in range(H):
            mb = R.mass_bound(p[f, h, i][None, :], 2 * eps[f, h:h + 1, i], S, 1)
            assert torch.allclose(V.per_head_bound(p, eps)[f, h, i], mb[0], rtol=1e-12, atol=0)
    # the fp32 definition itself lies inside the bound of the float64 truth (its arithmetic is one of those the bound covers)
    d = V.definition_fp32(q, k)
    assert ((d.double() - p).abs() <= V.per_head_bound(p, eps)).all()
    assert ((V.head_mean_chain(d).double() - p.mean(1)).abs() <= V.head_mean_bound(p, eps)).all()
    assert (V.head_mean_bound(p, eps) < 0.01 * p.mean(1) + 2.0 ** -23).all()                               # ... which is no loose one
