"""Head knock-out and head patching without a GPU: the ABI entries, the refusals that come before any launch (native, with fake aligned addresses;
host, as ValueError from a model that lives on the host), the signatures and graph keys that stay as they were, and the reference of
tests/test_gpu_head_patch.py pinned to the existing oracle - no options is depth_lens_reference.composed_states bit for bit, a self-patch and an
all-ones scale are bit-neutral, all heads of a layer scaled to 0 is the layer function without its attention term - with the oracle condition:
on the rig, each knock-out case moves the oracle's own score by at least twice the GPU file's bar."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import depth_lens_reference as DL
import head_patch_reference as HP
from test_key_drop_cpu import bf16_ulps
from test_stream_patch_cpu import host_rig, oracle_rig, same

from aigv_assessor_amd import dist_utils, eval_utils, native, readouts
from aigv_assessor_amd.readouts import HeadPatch, HeadScale
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS, HEADS, D = 4, 4, 128
BF = torch.bfloat16
NEW = ("return_heads", "head_layers", "head_patch", "head_scale")

# (layers whose heads are scaled, the heads, the factor): the five knock-outs the GPU file compares with the oracle; the first two also compare tokens
KNOCKOUTS = (((0,), (2,), 0.0), ((2,), (0, 1, 2, 3), 0.0), ((0,), (0,), 0.0), ((3,), (0, 1, 2, 3), 0.0), ((0,), (0,), -1.0))


def scale_table(layers, heads, s):
    t = torch.ones(LAYERS, HEADS)
    for l in layers:
        for h in heads:
            t[l, h] = s
    return t


# ---- the ABI entries ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_entries():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I, I32P = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)
    U64P, FP = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_float)
    want = {"aigv_head_capture_arm": (I, [P, I32P, I, I, I, P]),
            "aigv_head_patch_arm": (I, [P, I32P, I, I, I, U64P, P]),
            "aigv_head_scale_arm": (I, [P, I32P, I, FP]),
            "aigv_op_head_rows": (I, [P, I, I, I32P, I, P, P, I, I, I, I, I, ctypes.c_uint64, FP, P])}
    for name, proto in want.items():
        assert name in note and re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == proto, name
    kernels = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert "aigv_launch_head_rows(" in kernels
    rowops = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "rowops.hip")).read()
    assert "template <int MODE>" in rowops and "head_rows_kernel" in rowops                              # the operation is a template parameter


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_native_refusals_without_a_gpu():
    """Every check of the op comes before any HIP call: AIGV_ERR_ARG and a message that starts with the op's name (fake, aligned, non-null device
    addresses: nothing is dereferenced; the host arrays are real, they are read).  The context entry points refuse a null handle."""
    lib = native.load()
    P = 0x10000
    last = lambda: (lib.aigv_last_error(None) or b"").decode()
    good = [0, 3, 9, 99]
    fl = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)

    def op(ao=P, ld=512, T=100, rows=good, n=None, idx=P, side=P, n_layers=3, layer=1, n_heads=4, D=128, mode=0, bits=0xF, scale=None):
        arr = native.i32_array(rows) if rows is not None else None
        return lib.aigv_op_head_rows(ao, ld, T, arr, len(rows or []) if n is None else n, idx, side, n_layers, layer, n_heads, D, mode, bits, fl(scale), None), last()

    cases = ((dict(ao=None), "null operand"), (dict(rows=None, n=4), "null operand"), (dict(idx=None), "null operand"),
             (dict(n=-1), "must not be negative"), (dict(ld=504), "leading dimension"), (dict(ld=516), "leading dimension"),
             (dict(ao=P + 8), "16-byte aligned"), (dict(T=-1), "must not be negative"),
             (dict(n_heads=65, ld=65 * 128), "65 heads outside 1..64"), (dict(n_heads=0), "0 heads outside 1..64"), (dict(D=96), "neither 64 nor 128"),
             (dict(mode=3), "mode 3 is none of"), (dict(mode=-1), "mode -1 is none of"),
             (dict(rows=[0, 3, 100]), "row 2 (packed row 100) outside [0, 100)"), (dict(rows=[-1, 3]), "row 0 (packed row -1) outside [0, 100)"),
             (dict(rows=[0, 9, 3]), "not strictly ascending"), (dict(rows=[0, 3, 3]), "not strictly ascending"))
    window = ((dict(side=None), "null operand"), (dict(side=P + 8), "16-byte aligned"), (dict(layer=3), "layer 3 outside the window of 3 layers"),
              (dict(layer=-1), "outside the window"), (dict(n_layers=0, layer=0), "outside the window"))
    ones = [1.0, 0.0, 1.0, 2.0]
    for mode in (0, 1, 2):
        for kw, word in cases + (window if mode < 2 else ((dict(scale=None), "null scale table"), (dict(scale=[1.0, float("nan"), 1.0, 1.0]), "scale[1] is NaN"))):
            if mode == 2 and "rows" in kw and kw["rows"] is None:
                continue                                                                      # (the scale takes no row list: every row)
            rc, msg = op(**dict(dict(mode=mode, scale=ones if mode == 2 else None), **kw))
            assert rc == -1 and word in msg and msg.startswith("aigv_op_head_rows:"), (mode, kw, rc, msg)
    rows = native.i32_array(good)
    table = fl([1.0] * 16)
    assert lib.aigv_head_capture_arm(None, rows, 4, 0, 1, P) == -1 and last().startswith("aigv_head_capture_arm: null context")
    assert lib.aigv_head_patch_arm(None, rows, 4, 0, 1, None, P) == -1 and last().startswith("aigv_head_patch_arm: null context")
    assert lib.aigv_head_scale_arm(None, rows, 4, table) == -1 and last().startswith("aigv_head_scale_arm: null context")


def test_host_refusals_come_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError.  Every message names its option."""
    model, cfg, kw = host_rig()
    ids, am = kw["input_ids"], kw["attention_mask"]
    seg = model.segment_masks(ids, am, kw["image_flags"])
    mask = seg["score_row"]                                                                   # two tokens, one per clip
    vals = lambda n=2, l=1, h=HEADS, d=D, dt=BF: torch.zeros(n, l, h, d, dtype=dt)
    ones = torch.ones(LAYERS, HEADS)

    def bad(word, **opts):
        with pytest.raises(ValueError, match=word):
            model(**kw, **opts)

    # shapes and dtypes
    bad("return_heads: shape", return_heads=mask[:, :100])
    bad("return_heads: expected a bool or integer tensor", return_heads=mask.float())
    bad("head_patch: rows: shape", head_patch=HeadPatch(mask[:, :100], vals(), (0, 1)))
    bad("head_patch: expected a readouts.HeadPatch", head_patch=(mask, vals(), (0, 1)))
    bad("head_patch: values must be a bf16 tensor", head_patch=HeadPatch(mask, vals(dt=torch.float32), (0, 1)))
    bad("head_patch: values must be a bf16 tensor", head_patch=HeadPatch(mask, vals(l=2), (0, 1)))
    bad("head_patch: values must be a bf16 tensor", head_patch=HeadPatch(mask, vals()[0], (0, 1)))
    bad(f"head_patch: values must be a bf16 tensor .*n_heads = {HEADS}, D = {D}", head_patch=HeadPatch(mask, vals(h=HEADS - 1), (0, 1)))
    bad("head_patch: values must be a bf16 tensor", head_patch=HeadPatch(mask, vals(d=64), (0, 1)))
    bad("head_patch: index must be an integer tensor", head_patch=HeadPatch(mask, vals(), (0, 1), torch.zeros(2, 3, dtype=torch.long)))
    bad("head_patch: heads must be a bool tensor", head_patch=HeadPatch(mask, vals(), (0, 1), None, torch.ones(HEADS)))
    bad("head_patch: heads must be a bool tensor", head_patch=HeadPatch(mask, vals(), (0, 1), None, torch.ones(2, HEADS, dtype=torch.bool)))
    bad("head_patch: heads must be a bool tensor", head_patch=HeadPatch(mask, vals(), (0, 1), None, torch.ones(HEADS + 1, dtype=torch.bool)))
    bad("head_scale: expected a readouts.HeadScale", head_scale=ones)
    bad(f"head_scale: scale must be a float tensor \\[L = {LAYERS}, n_heads = {HEADS}\\]", head_scale=HeadScale(ones[:3]))
    bad("head_scale: scale must be a float tensor", head_scale=HeadScale(ones[:, :3]))
    bad("head_scale: scale must be a float tensor", head_scale=HeadScale(ones.long()))
    bad("head_scale: rows: shape", head_scale=HeadScale(ones, mask[:, :100]))
    nan = ones.clone(); nan[2, 1] = float("nan")
    bad(r"head_scale: scale\[2, 1\] is NaN", head_scale=HeadScale(nan))
    # count mismatch: both counts are named
    bad("head_patch: values hold 3 rows, the mask selects 2 tokens", head_patch=HeadPatch(mask, vals(n=3), (0, 1)))
    dead = torch.zeros_like(mask); dead[:, 214] = True                                        # the closing token: behind the last consumed row, not run
    bad("head_patch: values hold 2 rows, the mask selects 0 tokens", head_patch=HeadPatch(dead, vals(), (0, 1)))
    own = torch.tensor([[0, 211], [1, 211]])
    bad("head_patch: index holds 1 pairs, the mask selects 2 tokens", head_patch=HeadPatch(mask, vals(), (0, 1), own[:1]))
    # index mismatch: the first differing pair
    bad(r"head_patch: pair 1 of index is \(clip, position\) = \(1, 210\), the pass's is \(1, 211\)",
        head_patch=HeadPatch(mask, vals(), (0, 1), torch.tensor([[0, 211], [1, 210]])))
    # a bad window
    for window in ((2, 1), (-1, 2), (0, LAYERS + 1), (0,), (0, 1, 2), 2, (0.0, 2), (False, True)):
        bad("head_layers", return_heads=mask, head_layers=window)
        bad("head_patch: layers", head_patch=HeadPatch(mask, vals(), window))
    bad("head_layers: qualifies return_heads", head_layers=(0, 2))
    # more than 64 query heads: refused when arming
    with pytest.raises(ValueError, match="the model has 65 query heads, a head mask holds at most 64"):
        readouts.head_options(return_heads=mask, n_layers=LAYERS, n_heads=65, head_dim=64)
    # what passes the host checks: the record carries the options, and forward_kwargs hands them on
    sel = torch.tensor([True, False, False, True])
    ro = readouts.ReadOuts.parse(cfg.llm_config.vocab_size, kw["labels"], ids_shape=ids.shape, n_layers=LAYERS, return_heads=mask.long(),
                                 head_patch=HeadPatch(mask, vals(l=2), [1, 3], own, sel), head_scale=HeadScale(ones.double(), mask), n_heads=HEADS, head_dim=D)
    assert torch.equal(ro.head_rows, mask) and ro.head_layers == (0, LAYERS) and ro.head_patch.layers == (1, 3) and ro.touches_stream
    assert torch.equal(ro.head_patch.heads, sel.expand(2, HEADS)) and readouts.head_bits(ro.head_patch.heads) == [9, 9]
    assert ro.head_scale.scale.dtype == torch.float32 and torch.equal(ro.head_scale.rows, mask)
    assert readouts.head_bits(torch.ones(1, 64, dtype=torch.bool)) == [2 ** 64 - 1]
    fk = readouts.forward_kwargs(ro)
    assert torch.equal(fk["return_heads"], mask) and fk["head_layers"] == (0, LAYERS) and fk["head_patch"] is ro.head_patch and fk["head_scale"] is ro.head_scale
    assert not set(NEW) & set(readouts.forward_kwargs(readouts.ReadOuts(logprobs=True)))
    fields = [f.name for f in readouts.ReadOuts.__dataclass_fields__.values()]
    assert fields[fields.index("stream_patch") + 1:] == ["head_rows", "head_layers", "head_patch", "head_scale"]     # appended after stream_patch
    # against the plan
    plan = model._plan(ids, am, kw["labels"], kw["image_flags"], 4)
    got = model._head_patch_plan(plan, ro.head_patch)
    assert got[0].tolist() == [int(r) for r in plan["score_rows"]] and got[1:4] == (1, 3, [9, 9]) and got[4] is ro.head_patch.values
    assert model._head_patch_plan(plan, HeadPatch(mask, vals(l=0), (2, 2))) is None             # an empty window: the plain pass
    assert model._head_patch_plan(plan, HeadPatch(dead, vals(n=0), (0, 1))) is None             # an empty selection likewise
    assert model._head_patch_plan(plan, HeadPatch(mask, vals(), (0, 1), None, torch.zeros(1, HEADS, dtype=torch.bool))) is None   # no head likewise


def test_the_other_entry_points_keep_their_signatures():
    model = host_rig()[0]
    for fn in (model.forward_shared_prefix, model.generate, model.generate_stage2, eval_utils.batched, dist_utils.score_clips_dp):
        assert not set(NEW) & set(inspect.signature(fn).parameters), fn
    assert set(NEW) <= set(inspect.signature(model.forward).parameters)
    sig = inspect.signature(eval_utils.head_knockout).parameters
    assert [sig[k].default for k in ("labels", "layers", "heads", "rows")] == [None] * 4 and {"pixel_values", "input_ids", "attention_mask", "image_flags"} <= set(sig)
    sig = inspect.signature(eval_utils.head_trace).parameters
    assert [sig[k].default for k in ("layers", "heads", "rows")] == [None] * 3 and {"clean", "corrupt"} <= set(sig)


def test_head_trace_applies_causal_traces_input_checks():
    model, cfg, kw = host_rig()
    for change, word in ((dict(input_ids=kw["input_ids"][:, :200]), "one token layout"),
                         (dict(attention_mask=kw["attention_mask"] & (torch.arange(215) < 214)), "attention_mask differ"),
                         (dict(pixel_values=kw["pixel_values"][:3]), "pixel_values of shape")):
        with pytest.raises(ValueError, match="head_trace: .*" + word):
            eval_utils.head_trace(model, clean=dict(kw), corrupt=dict(kw, **change))
    with pytest.raises(ValueError, match="head_trace: layers"):
        eval_utils.head_trace(model, clean=dict(kw), corrupt=dict(kw), layers=[LAYERS])
    with pytest.raises(ValueError, match="head_knockout: layers"):
        eval_utils.head_knockout(model, **{k: v for k, v in kw.items() if k != "motion_feature"}, heads=[HEADS])


# ---- the graph key ------------------------------------------------------------------------------------------------------------------
def test_key_tail_and_forward_kwargs_of_calls_without_the_options_are_what_they_were():
    V, shape = 1000, (2, 215)
    cases = (dict(), dict(return_logprobs=True), dict(candidate_ids=[1, 2, 3], top_logprobs=4), dict(return_score_attention=True),
             dict(return_token_attention=True, return_logprobs=True), dict(return_depth_lens=True))
    was = ((), ("logprobs",), ("candidates", ("top_logprobs", 4)), (("score_attention", 0),), ("logprobs", ("score_attention", 0), ("score_attention_tokens", 215)),
           ("depth_lens",))
    keys = (set(), {"return_logprobs"}, {"candidate_ids", "top_logprobs"}, {"return_score_attention"}, {"return_logprobs", "return_score_attention", "return_token_attention"},
            {"return_depth_lens"})
    mask = torch.zeros(shape, dtype=torch.bool)
    for kw, tail, names in zip(cases, was, keys):
        ro = readouts.ReadOuts.parse(V, "given", ids_shape=shape, **kw)
        assert ro.key_tail(shape) == tail and not ro.touches_stream and set(readouts.forward_kwargs(ro)) == names, kw
        assert ro.head_rows is None and ro.head_layers is None and ro.head_patch is None and ro.head_scale is None
        for opt in (dict(return_heads=mask), dict(head_patch=HeadPatch(mask, torch.zeros(0, 1, HEADS, D, dtype=BF), (0, 1))), dict(head_scale=HeadScale(torch.ones(LAYERS, HEADS)))):
            armed = readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=LAYERS, **opt, **kw)
            assert armed.key_tail(shape) == tail and armed.touches_stream, (kw, opt)                # nothing joins the key: such a call is never captured


# ---- the composed reference, pinned to the existing oracle ----------------------------------------------------------------------------
def test_reference_without_options_self_patch_and_all_ones_scale_are_the_composed_states():
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[1]
    am = one["attention_mask"]
    every = torch.ones_like(am)
    got, cap = HP.composed_states(sd, cfg, **inputs)
    assert cap is None and len(got) == LAYERS + 1 and all(same(g, p) for g, p in zip(got, plain)) and O.LLM_LINEAR_HOOK is None
    got, cap = HP.composed_states(sd, cfg, **inputs, capture=(every, (0, LAYERS)))
    assert tuple(cap.shape) == (215, LAYERS, HEADS, D) and all(same(g, p) for g, p in zip(got, plain))
    seg = model.segment_masks(one["input_ids"], am, one["image_flags"])
    for mask, layers, heads in ((every, (0, LAYERS), None), (seg["frames"], (1, 3), torch.tensor([True, False, True, False])), (seg["score_row"], (3, 4), None)):
        own = mask[0, :215].nonzero().flatten()
        values = cap[own][:, layers[0]:layers[1]]
        got, again = HP.composed_states(sd, cfg, **inputs, patches=[(mask, values, layers, heads)], capture=(mask, layers))
        assert all(same(g, p) for g, p in zip(got, plain)) and same(again, values), layers
    got, _ = HP.composed_states(sd, cfg, **inputs, scale=torch.ones(LAYERS, HEADS))
    assert all(same(g, p) for g, p in zip(got, plain))
    got, _ = HP.composed_states(sd, cfg, **inputs, scale=scale_table((1,), (2,), 0.0), scale_rows=torch.zeros_like(am))       # no row: no change
    assert all(same(g, p) for g, p in zip(got, plain))
    # a patch with a heads mask, read back by a capture: selected heads carry the values, the others the plain bits
    noise = torch.randn(215, 1, HEADS, D, generator=torch.Generator().manual_seed(5)).to(BF)
    sel = torch.tensor([False, True, False, True])
    got, back = HP.composed_states(sd, cfg, **inputs, patches=[(every, noise, (1, 2), sel)], capture=(every, (1, 2)))
    assert same(back[:, 0, sel], noise[:, 0, sel]) and same(back[:, 0, ~sel], cap[:, 1, ~sel]) and not same(got[2], plain[2]) and same(got[1], plain[1])


def test_reference_all_heads_of_a_layer_scaled_to_0_is_the_layer_without_its_attention_term():
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[1]
    eps = cfg.llm_config.rms_norm_eps
    for l in (0, 2, 3):
        got, cap = HP.composed_states(sd, cfg, **inputs, scale=scale_table((l,), range(HEADS), 0.0), capture=(torch.ones_like(one["attention_mask"]), (l, l + 1)))
        assert not cap.any()
        x = plain[l]
        x = x + torch.zeros_like(x)                                                           # wo of a zero row
        want = x + O.llm_mlp(sd, l, O.rms_norm_cast_then_scale(x, sd[f"language_model.model.layers.{l}.ffn_norm.weight"], eps))
        assert same(got[l + 1], want) and not same(got[l + 1], plain[l + 1]), l
        assert all(same(got[d], plain[d]) for d in range(l + 1))


def knockout_case(layers, heads, s):
    """-> (the oracle's plain score of clip 0 alone, its score under the scale, its near-tie answer rows, its answer rows)."""
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[0]
    am = one["attention_mask"]
    score = lambda states: float(DL.lens(sd, cfg, states, am, one["labels"], 2)["score"][0, LAYERS])
    states, _ = HP.composed_states(sd, cfg, **inputs, scale=scale_table(layers, heads, s))
    w, eps = sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps
    logits = O.lm_logits(sd, O.rms_norm_cast_then_scale(states[LAYERS], w, eps))[0, :-1]
    want = one["labels"][0, 1:] != -100
    top = logits[want].float().topk(2, -1).values
    ulp = torch.exp2(top[:, 0].abs().clamp_min(1e-30).log2().floor() - 7)
    ties = int(((top[:, 0] - top[:, 1]) <= 2 * ulp).sum())
    return score(plain), score(states), ties, int(want.sum())


@pytest.mark.parametrize("case", range(len(KNOCKOUTS)))
def test_oracle_condition_each_knockout_moves_the_oracle(case):
    """The rig of tests/test_stream_patch_cpu.py::oracle_rig (weights seed 63, tokens seed 302, 4 layers, 4 heads x 128), clip 0 alone in bf16, plain
    score 0.48047.  Measured on a host: layer 0 head 2 scaled by 0 gives 0.48828 (4 bf16 ulps from plain, 0 near-tie answer rows of 10); layer 2
    heads 0..3 by 0 0.49609 (8, 1); layer 0 head 0 by 0 0.49219 (6, 2); layer 3 heads 0..3 by 0 0.46289 (9, 4); layer 0 head 0 by -1 0.49805 (9,
    4).  A near-tie row is an answer row whose top two oracle logits lie within 2 bf16 ulps.  Each case must move the oracle's own score by at
    least 2 ulps - twice the GPU file's bar, so a no-op cannot pass there; the first two cases, whose tokens the GPU file compares with at most
    one excused row, must have at most 1 near-tie row in the oracle itself.  (Printed, not pinned: the oracle's bf16 sums follow the host's
    thread count.)"""
    layers, heads, s = KNOCKOUTS[case]
    plain, knocked, ties, rows = knockout_case(layers, heads, s)
    print(f"layers {layers} heads {heads} x {s}: oracle {knocked:.5f}, plain {plain:.5f} = {bf16_ulps(knocked, plain):.1f} bf16 ulps; {ties} near-tie answer rows of {rows}")
    assert bf16_ulps(knocked, plain) >= 2
    if case < 2:
        assert ties <= 1
