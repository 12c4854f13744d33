"""Score-row value flow without a GPU: the yardstick of tests/test_gpu_score_values.py proven on the host - a CPU restatement of the kernel's
stated fp32 chain passes ``value_bound`` with 1, 2 and 4 key lanes, and every planted fault is refused by it - the conditions under which the
census and selector expectations ARE exact, the ABI entries and their host refusals, the option's parsing, and the ``eval_utils`` helpers
against a direct float64 einsum."""
import ctypes
import functools
import inspect
import os
import re

import pytest
import torch

import score_attention_reference as R
import score_values_reference as VR
from test_stream_patch_cpu import host_rig

from aigv_assessor_amd import dist_utils, eval_utils, native, prompts, readouts
from aigv_assessor_amd.modeling import InternVLChatModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, D, HK = R.S, R.D, R.N_KV
FAULTS = ("other_kv_head", "key_shift", "other_sequence_table", "last_key", "no_division", "boundary", "k_as_v")


@functools.lru_cache(maxsize=None)
def case(g):
    c = VR.ValuesCase(g)
    return c, R.rotate_q(c.q, c.pos, c.cos, c.sin), c.truth()


def chain_row(c, q_rot, b, r, t, lanes=2, fault=None):
    """chain_fp32 of one probe row of the random case, with the planted faults that are a matter of WHICH operand the chain is given."""
    lo, n = c.cu[b], r + 1
    keys, vals, seg = c.k[lo:lo + n], c.v[lo:lo + n], c.seg[lo:lo + n]
    if fault == "other_kv_head":
        vals = vals.flip(1)
    elif fault == "key_shift":                                       # V of the next key (the last one: of the previous)
        vals = torch.cat([vals[1:], vals[-2:-1] if n > 1 else vals[:1] * 2])
    elif fault == "other_sequence_table":
        o = c.cu[(b + 1) % len(c.lens)] if c.lens[(b + 1) % len(c.lens)] >= n else c.cu[2]
        seg = c.seg[o:o + n] if o != lo else (seg + 1)
    elif fault == "k_as_v":
        vals = keys
    return VR.chain_fp32(q_rot[t].reshape(HK * c.g, D), keys, vals, seg, S, lanes, fault if fault in ("last_key", "no_division", "boundary") else None,
                         off=R.CACHE_OFF[b])


@pytest.mark.parametrize("g", R.GROUPS)
def test_the_stated_chain_passes_the_bound_with_1_2_and_4_key_lanes(g):
    """The bound does not depend on the lane count: each version within the bound of its own count AND within the lane-free one."""
    c, q_rot, truth = case(g)
    for lanes in (1, 2, 4):
        worst = 0.0
        for b, r, t in R.probe_rows():
            got = chain_row(c, q_rot, b, r, t, lanes).double()
            val, free = truth[t]
            own = c.truth(key_lanes=lanes)[t][1] if (b, r) == (2, 512) else free
            assert (own <= free).all()
            worst = max(worst, ((got - val).abs() / own).max().item())
            assert ((got - val).abs() <= own).all() and ((got - val).abs() <= free).all(), (lanes, b, r)
        print(f"g={g} lanes={lanes}: worst |chain - fp64| / bound = {worst:.4f}")


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("g", R.GROUPS)
def test_every_planted_fault_is_refused_by_the_bound(g, fault):
    c, q_rot, truth = case(g)
    refused = 0
    for b, r, t in R.probe_rows():
        if r < 254:
            continue                                                  # (the long rows: both sides of the stride, a second sweep)
        got = chain_row(c, q_rot, b, r, t, 2, fault).double()
        val, bound = truth[t]
        refused += int(((got - val).abs() > bound).any())
    assert refused >= (4 if fault != "boundary" else 3), (fault, refused)      # (boundary: the rows of the sequences with cached keys)


def test_census_and_selector_expectations_are_exact_and_refuse_the_faults():
    """Q = 0 and |v| <= 8 integers: every partial sum is an integer <= 4104, exact in fp32 in any order - the chain restated with 1, 2 and 4 lanes
    gives the expectation bit for bit, and V from the other kv head, a shifted key or another table does not.  Selector: weight exactly 1."""
    g = 3
    T, cu = sum(R.LENS), R.cu_of(R.LENS)
    v = VR.census_v(T)
    assert v.float().abs().max() <= 8 and 8 * max(R.LENS) == 4104
    seg = R.seg_table()
    cos, sin = R.rope_table(D, R.N_POS)
    for b, r, t in R.probe_rows():
        if r not in (0, 1, 257):
            continue
        lo, n = cu[b], r + 1
        want = VR.census_values(v[lo:], seg[lo:], n, S, g)
        q0 = torch.zeros(HK * g, D, dtype=R.BF)
        k = torch.randn(n, HK, D).to(R.BF)
        for lanes in (1, 2, 4):
            got = VR.chain_fp32(q0, k, v[lo:lo + n], seg[lo:lo + n], S, lanes)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (b, r, lanes)
        if r == 257:
            assert not torch.equal(VR.chain_fp32(q0, k, v[lo:lo + n].flip(1), seg[lo:lo + n], S), want)
            assert not torch.equal(VR.chain_fp32(q0, k, v[lo + 1:lo + n + 1], seg[lo:lo + n], S), want)
            assert not torch.equal(VR.chain_fp32(q0, k, v[lo:lo + n], seg[cu[3 - b]:cu[3 - b] + n], S), want)      # (the other long sequence's table)
            assert not torch.equal(VR.chain_fp32(q0, k, v[lo:lo + n], seg[lo:lo + n], S, fault="last_key"), want)
            assert not torch.equal(VR.chain_fp32(q0, k, v[lo:lo + n], seg[lo:lo + n], S, fault="no_division"), want)
    vr = VR.random_v(T)
    for b, r, sel in ((1, 257, 255), (1, 257, 256), (2, 512, 0)):
        c = R.SelectorCase(g, b, r, sel)
        lo, n = c.cu[b], r + 1
        got = VR.chain_fp32(c.q_rot.reshape(-1, D), c.k[lo:lo + n], vr[lo:lo + n], c.seg[lo:lo + n], S)
        assert (got == VR.selector_values(c, vr)).all(), (b, r, sel)


def test_value_bound_is_derived_not_chosen():
    """c is the count of roundings the kernel header names; the bound is relative to sum p |v|, grows with the score bound, and the lane-free
    count dominates every lane count."""
    assert VR.chain_roundings(513, 2) == 4 + 12 + 257 + 1 + 1 and VR.chain_roundings(513, 4) == 4 + 12 + 129 + 3 + 1
    assert VR.chain_roundings(513) == 4 + 12 + 513 + 3 + 1 and VR.chain_roundings(1, 4) == 4 + 10 + 1 + 3 + 1
    for n in (1, 2, 3, 258, 513):
        assert all(VR.chain_roundings(n, kl) <= VR.chain_roundings(n) for kl in (1, 2, 4))
    w = torch.full((2, 3, 4), 0.5, dtype=torch.float64)
    zero = torch.zeros(2, dtype=torch.float64)
    b0 = VR.value_bound(w, zero, 513, 2) - VR.ABS_FLOOR
    assert torch.allclose(b0, w * 275 * VR.U, rtol=1e-4, atol=0)
    assert (VR.value_bound(w, torch.full((2,), 1e-3, dtype=torch.float64), 513, 2) > b0 + w * 1.9e-3).all()
    header = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "attnprobe.hip")).read()
    for phrase in ("ONE fma per", "KL - 1 additions in lane order", "ONE fp32 division", "ceil(n / KL) fmas", "0 x Inf is NaN"):
        assert phrase in header, phrase
    c, q_rot, truth = case(1)
    val, bound = truth[771]
    assert VR.ABS_FLOOR < bound.max().item() < 1e-3 and val.abs().max().item() > 0.01      # far below anything a norm or a projection shows


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_header_prototypes_and_host_refusals():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I = native._P, native._I
    arm_t, op_t = native.PROTOTYPES["aigv_score_attention_arm_tokens"], native.PROTOTYPES["aigv_op_attention_probe_tokens"]
    assert native.PROTOTYPES["aigv_score_attention_arm_values"] == (I, arm_t[1] + [P])
    assert native.PROTOTYPES["aigv_op_attention_probe_values"] == (I, op_t[1][:-1] + [P, I, P] + op_t[1][-1:])
    lib = native.load()
    for name in ("aigv_score_attention_arm_values", "aigv_op_attention_probe_values"):
        assert name in note and hasattr(lib, name), name
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(native.PROTOTYPES[name][1]) and "float* val_out" in decl, name
    # host refusals: before any pointer is used (a small aligned HOST buffer stands for every operand; no accepted call is made)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    p += 16 - p % 16
    cu = native.i32_array([0, 4])
    last = lambda: (lib.aigv_last_error(None) or b"").decode()

    def call(v=p, ldv=3 * 128, val=p, tok=None, ld_tok=0, n_seg=3, rows=(3,)):
        return lib.aigv_op_attention_probe_values(p, 3 * 128, p, 3 * 128, cu, 1, 1, 1, 3 * 128, 3 * 128, 0, None, 128, p, p, 8, native.i32_array(list(rows)), len(rows),
                                                  p, None, 0, n_seg, ctypes.cast(p, ctypes.c_void_p), tok, ld_tok, v, ldv, val, None)

    for kw, word in ((dict(v=None), "null v"), (dict(val=None), "null val_out"), (dict(v=p + 8), "16-byte aligned"), (dict(ldv=3 * 128 + 4), "multiple of 8"),
                     (dict(ldv=64), "packed V strides too small"), (dict(tok=p, ld_tok=3), "ld_tok is below"), (dict(ld_tok=4), "null tok_out"),
                     (dict(n_seg=65), "segments"), (dict(rows=tuple(range(4)) * 17), "probe rows")):
        rc = call(**kw)
        assert rc == -1 and word in last() and "aigv_op_attention_probe_values" in last(), (kw, rc, last())
    rows = native.i32_array([0])
    assert lib.aigv_score_attention_arm_values(None, rows, 1, p, None, 0, 3, p, None, 0, p) == -1 and "null context" in last()


# ---- the option ---------------------------------------------------------------------------------------------------------------------------------
def test_option_parsing_record_and_graph_key():
    V, shape = 1000, (2, 215)
    ro = readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_score_values=True)
    assert ro.score_values and ro.score_attention and not ro.token_attention and ro.runs_eagerly and not ro.touches_stream
    assert readouts.forward_kwargs(ro) == dict(return_score_attention=True, return_score_values=True)
    both = readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_score_values=True, return_token_attention=True)
    assert both.token_attention and both.score_values
    new = {"return_score_values"}
    assert not new & set(readouts.forward_kwargs(readouts.ReadOuts(logprobs=True)))
    fields = [f.name for f in readouts.ReadOuts.__dataclass_fields__.values()]
    at = fields.index("score_values")
    assert fields[at - 1] == "token_attention" and fields[at + 1] == "key_drop" and readouts.ReadOuts().score_values is False
    # calls without the flag: the key and the keywords they always had, and they still replay
    cases = (dict(), dict(return_logprobs=True), dict(candidate_ids=[1, 2, 3], top_logprobs=4), dict(return_score_attention=True),
             dict(return_token_attention=True, return_logprobs=True), dict(return_depth_lens=True))
    was = ((), ("logprobs",), ("candidates", ("top_logprobs", 4)), (("score_attention", 0),), ("logprobs", ("score_attention", 0), ("score_attention_tokens", 215)),
           ("depth_lens",))
    for kw, tail in zip(cases, was):
        r = readouts.ReadOuts.parse(V, "given", ids_shape=shape, **kw)
        assert r.key_tail(shape) == tail and not r.runs_eagerly and not r.score_values and not new & set(readouts.forward_kwargs(r)), kw
        assert readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_score_values=True, **kw).runs_eagerly
    with pytest.raises(ValueError, match="return_score_values: at most 64 clips"):
        readouts.ReadOuts.parse(V, "given", ids_shape=(65, 215), return_score_values=True)
    with pytest.raises(ValueError, match="key_drop: cannot be combined with .*return_score_values"):
        readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_score_values=True, key_drop=torch.zeros(shape, dtype=torch.bool))


def test_python_surface_and_refusals_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError."""
    for fn in (InternVLChatModel.forward, InternVLChatModel.forward_shared_prefix):
        assert inspect.signature(fn).parameters["return_score_values"].default is False
    for fn in (InternVLChatModel.generate, InternVLChatModel.generate_stage2, eval_utils.batched, dist_utils.score_clips_dp):
        assert "return_score_values" not in inspect.signature(fn).parameters, fn
    assert list(inspect.signature(eval_utils.source_writes).parameters) == ["model", "out", "direction", "layers"]
    assert list(inspect.signature(eval_utils.frame_write_saliency).parameters) == ["norms", "layers"]
    model, cfg, kw = host_rig()
    drop = torch.zeros_like(kw["input_ids"], dtype=torch.bool)
    drop[:, 20] = True
    with pytest.raises(ValueError, match="key_drop: cannot be combined with .*return_score_values"):
        model(**kw, return_score_values=True, key_drop=drop)
    many = {k: (v.repeat(33, *([1] * (v.dim() - 1))) if torch.is_tensor(v) else v) for k, v in kw.items()}
    with pytest.raises(ValueError, match="at most 64 clips"):
        model(**many, return_score_values=True)


# ---- the helpers --------------------------------------------------------------------------------------------------------------------------------
class _Weights:
    def __init__(self, wo):
        self.wo = wo

    def named_parameters(self):
        return [(f"language_model.model.layers.{l}.attention.wo.weight", torch.nn.Parameter(w, requires_grad=False)) for l, w in enumerate(self.wo)]


def test_source_writes_and_frame_write_saliency_against_float64():
    """Against a direct float64 einsum that DOES form the [B, L, n_heads, S, H] tensor; the tolerance is fp32 roundoff derived from the inner
    dimensions: a dot of K terms in fp32 is within K u sum |terms| (first order; 2 K u covers the rest), K = H + D for the direction form (two
    chained dots) and n_heads D (+ H for the norm's own sum of squares, relative) for the norm form."""
    B, L, nh, F, Dh, H = 3, 4, 6, 3, 16, 40
    Sg = F + prompts.N_TEXT_SEGMENTS
    gen = torch.Generator().manual_seed(77)
    val = torch.randn(B, L, nh, Sg + 1, Dh, generator=gen)
    val[2, :, :, :F] = 0                                              # clip 2 reads nothing from any frame
    wo = [torch.randn(H, nh * Dh, generator=gen).to(torch.bfloat16) for _ in range(L)]
    model = _Weights(wo)
    out = dict(score_values=val[..., :-1, :], score_values_rest=val[..., -1, :])
    w64 = torch.stack([w.double().view(H, nh, Dh) for w in wo])       # [L, H, nh, D]
    full = torch.einsum("lohd,blhsd->blhso", w64, out["score_values"].double())
    full_abs = torch.einsum("lohd,blhsd->blhso", w64.abs(), out["score_values"].double().abs())
    u = 2.0 ** -24
    for direction in (torch.randn(H, generator=gen), torch.randn(B, H, generator=gen)):
        d64 = direction.double().expand(B, H)
        want = torch.einsum("bo,blhso->blhs", d64, full)
        tol = 2 * (H + Dh) * u * torch.einsum("bo,blhso->blhs", d64.abs(), full_abs) + 1e-30
        got = eval_utils.source_writes(model, out, direction)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, L, nh, Sg) and ((got.double() - want).abs() <= tol).all()
        sub = eval_utils.source_writes(model, out, direction, layers=[3, 1])
        assert tuple(sub.shape) == (B, 2, nh, Sg) and torch.equal(sub, got[:, [3, 1]])
    vec = full.sum(2)                                                 # [B, L, S, H]
    want = vec.norm(dim=-1)
    tol = 2 * (nh * Dh + H) * u * full_abs.sum(2).norm(dim=-1) + 1e-30
    norms = eval_utils.source_writes(model, out)
    assert norms.dtype == torch.float32 and tuple(norms.shape) == (B, L, Sg) and ((norms.double() - want).abs() <= tol).all()
    assert torch.equal(eval_utils.source_writes(model, out, layers=[2]), norms[:, [2]])
    assert torch.equal(eval_utils.source_writes(model, out["score_values"]), norms)          # the tensor itself is taken too
    sal = eval_utils.frame_write_saliency(norms)
    ref = want[..., :F].mean(1)
    assert tuple(sal.shape) == (B, F) and torch.allclose(sal[:2].double(), (ref / ref.sum(-1, keepdim=True))[:2], rtol=1e-5, atol=0)
    assert torch.allclose(sal[:2].sum(-1), torch.ones(2)) and torch.isnan(sal[2]).all()      # no frame writes anything: nothing to renormalise
    one = eval_utils.frame_write_saliency(norms, layers=[1])
    assert torch.allclose(one[:2].double(), (want[:, 1, :F] / want[:, 1, :F].sum(-1, keepdim=True))[:2], rtol=1e-5, atol=0)
    for bad in (norms[..., :4], norms[0]):
        with pytest.raises(ValueError, match="frame_write_saliency"):
            eval_utils.frame_write_saliency(bad)
    with pytest.raises(ValueError, match="source_writes: layers"):
        eval_utils.source_writes(model, out, layers=[L])
    with pytest.raises(ValueError, match="source_writes: direction"):
        eval_utils.source_writes(model, out, torch.zeros(B + 1, H))
