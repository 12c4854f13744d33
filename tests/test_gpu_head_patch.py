"""Head knock-out and head patching on the GPU: (a) the head-rows kernel in its three modes against torch indexing / torch arithmetic, between
fences; (b) the capture of forward(return_heads=...) against the pass itself and against the oracle's wo input; (c) the identities of
forward(head_patch=...) and forward(head_scale=...) on the 4-layer rig of tests/test_gpu_stream_patch.py - a self-patch and an all-ones scale
change nothing, a scale is capture + torch + patch, a capture reads the patch; (d) the knocked-out pass against the composed oracle of
tests/head_patch_reference.py; (e) with a key-drop window, a stream capture, in fp8 mode, under graph replay; (f) eval_utils.head_knockout and
eval_utils.head_trace; (g) the refusals of the C ABI at the pass, each by its message."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import depth_lens_reference as DL
import head_patch_reference as HP
from attention_reference import attn_truth, check_sequence
from test_gpu_key_drop import assert_levels, clip_alone, same, score_ok
from test_gpu_ops import BF, dev, lib, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import fenced, i32, ptr, same_bits, sentinel_like
from test_gpu_stream_patch import CAND, FRAMES, LAYERS, LENS_HIDDEN, READS, assert_same_outputs, only_clip, rig

from aigv_assessor_amd import eval_utils, native, synth
from aigv_assessor_amd.readouts import HeadPatch, HeadScale
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HEADS, D = 4, 128
HEAD_KEYS = ("heads", "heads_index")
CAPTURE, PATCH, SCALE = 0, 1, 2


# =================================================================================================================================
# (a) the kernel
# =================================================================================================================================
def head_masks(nh):
    """none, one (the last head: bit nh - 1), alternating, all"""
    return {"none": 0, "one": 1 << (nh - 1), "alternating": sum(1 << h for h in range(0, nh, 2)), "all": (1 << nh) - 1}


def columns(bits, nh, d):
    """bool [nh * d]: the columns of the heads whose bit is set"""
    return torch.tensor([(bits >> h) & 1 == 1 for h in range(nh)]).repeat_interleave(d)


def special_rows(t, H):
    """A NaN, a +Inf, a -Inf and a -0 payload in the first row of t [rows, >= H] (and a NaN with another payload in its last column)."""
    t[0, 5], t[0, H // 2], t[0, H // 4], t[0, 1] = float("nan"), float("inf"), float("-inf"), -0.0
    t.view(torch.int16)[0, H - 1] = 0x7FA5                                                  # a NaN with a payload of its own: the copy moves bits
    return t


def pick_rows(g, R, n, first):
    if n == 1:
        return [R - 1] if first else [0]
    inner = (torch.randperm(R - 2, generator=g)[:n - 2] + 1).sort().values.tolist()
    return [0] + inner + [R - 1]                                                            # the first and the last row, strictly ascending


@pytest.mark.parametrize("pad", [0, 64], ids=["ld=H", "ld=H+64"])
@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 130])
@pytest.mark.parametrize("nh,d", [(1, 64), (2, 64), (4, 128), (32, 128), (64, 64)])
def test_capture_and_patch_against_torch_indexing(lib, nh, d, n, n_layers, pad):
    g = torch.Generator().manual_seed(nh * d + 7 * n + n_layers + pad)
    H = nh * d
    R, ld, layer = 150, H + pad, n_layers // 2
    rows = pick_rows(g, R, n, n_layers == 1)
    at = torch.tensor(rows)
    ao = (torch.randn(R, ld, generator=g) * 3).to(BF)
    ao[rows[0]] = special_rows(ao[rows[0]:rows[0] + 1].clone(), H)[0]
    values = (torch.randn(n, n_layers, H, generator=g) * 3).to(BF)
    values[0, layer] = special_rows(values[0, layer][None].clone(), H)[0]
    idx_whole, idx_d = fenced(sentinel_like((n,), torch.int32))
    for name, bits in head_masks(nh).items():
        cols = columns(bits, nh, d)
        # capture: side(i, layer) = ao[rows[i]] in the selected heads' columns; everything else - the other heads' sentinel bytes, the other
        # layers, ao, the fences - keeps its bits
        ao_whole, ao_d = fenced(ao)
        side_whole, side_d = fenced(sentinel_like((n, n_layers, H), BF))
        sync(lib.aigv_op_head_rows(ptr(ao_d), ld, R, i32(rows), n, ptr(idx_d), ptr(side_d), n_layers, layer, nh, d, CAPTURE, bits, None, None), lib)
        want = sentinel_like((n, n_layers, H), BF)
        want[:, layer, cols] = ao[at][:, :H][:, cols]
        same_bits(side_whole, want)
        same_bits(ao_whole, ao)
        same_bits(idx_whole, at.to(torch.int32))
        # patch: ao[rows[i]] = side(i, layer) in the selected heads' columns; rows not selected, unselected heads, the padding columns, the side
        # buffer and the fences keep their bits
        ao_whole, ao_d = fenced(ao)
        side_whole, side_d = fenced(values)
        sync(lib.aigv_op_head_rows(ptr(ao_d), ld, R, i32(rows), n, ptr(idx_d), ptr(side_d), n_layers, layer, nh, d, PATCH, bits, None, None), lib)
        want = ao.clone()
        sub = want[at]
        sub[:, :H][:, cols] = values[:, layer][:, cols]
        want[at] = sub
        same_bits(ao_whole, want)
        same_bits(side_whole, values)
        assert name == "none" or not torch.equal(want.view(torch.int16), ao.view(torch.int16))
    if nh == 64:
        assert head_masks(nh)["one"] == 1 << 63                                               # bit 63 of the mask selected a head of its own above


SCALES = (0.0, 1.0, -1.0, 0.5, 1.7, 3e38)


def scaled(x, s):
    """(x.float() * s).bfloat16() of a bf16 tensor, on the host"""
    return (x.float() * s).to(BF)


def same_numbers(got, want):
    """Bit for bit wherever the expected value is a number; a NaN (0 x Inf, Inf x 0) where it is NaN - a NaN's payload is the converter's own."""
    got, want = got.cpu(), want.cpu()
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), "NaN positions differ"
    bad = (got.view(torch.int16)[~nan] != want.view(torch.int16)[~nan]).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} elements differ, first at {int(bad[0])}: {got[~nan][bad[0]].item()} vs {want[~nan][bad[0]].item()}"


@pytest.mark.parametrize("pad", [0, 64], ids=["ld=H", "ld=H+64"])
@pytest.mark.parametrize("n", [1, 5, 130, None], ids=["n=1", "n=5", "n=130", "every-row"])
@pytest.mark.parametrize("nh,d", [(1, 64), (2, 64), (4, 128), (32, 128), (64, 64)])
def test_scale_against_torch_arithmetic(lib, nh, d, n, pad):
    """ao = bf16(fp32(ao) * s[h]) for the heads whose factor is not exactly 1, over the listed rows (None: rows 0 .. T - 1, no row list); head h
    takes SCALES[h % 6], so every factor meets inputs holding +-0, subnormals, the largest finite value and +-Inf.  A head with factor 1 - and
    a head whose bit is clear - keeps its bits, NaN payloads included."""
    g = torch.Generator().manual_seed(nh * d + 7 * (n or 0) + pad)
    H = nh * d
    R, ld = 150, H + pad
    rows = list(range(R)) if n is None else pick_rows(g, R, n, False)
    at = torch.tensor(rows)
    ao = (torch.randn(R, ld, generator=g) * 3).to(BF)
    edge = torch.tensor([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x3F80, 0x0040], dtype=torch.int32).to(torch.int16)
    first = ao[rows[0]].view(torch.int16)
    for h in range(nh):                                                                       # +-0, subnormals, the smallest normal, +-max, +-Inf, 1 in every head of the first row
        first[h * d:h * d + edge.numel()] = edge
    first[H - 1] = 0x7FA5                                                                     # a NaN with a payload of its own
    for factors, bits in (([SCALES[h % 6] for h in range(nh)], (1 << nh) - 1), ([SCALES[(h + 2) % 6] for h in range(nh)], head_masks(nh)["alternating"]),
                          ([1.0] * nh, (1 << nh) - 1)):
        ao_whole, ao_d = fenced(ao)
        idx_whole, idx_d = fenced(sentinel_like((len(rows),), torch.int32))
        table = (native.C.c_float * nh)(*factors)
        sync(lib.aigv_op_head_rows(ptr(ao_d), ld, R, None if n is None else i32(rows), len(rows), None if n is None else ptr(idx_d), None, 0, 0, nh, d, SCALE, bits,
                                   table, None), lib)
        want = ao.clone()
        sub = want[at]
        touched = torch.zeros(ld, dtype=torch.bool)
        for h in range(nh):
            if (bits >> h) & 1 and factors[h] != 1.0:
                sub[:, h * d:(h + 1) * d] = scaled(sub[:, h * d:(h + 1) * d], factors[h])
                touched[h * d:(h + 1) * d] = True
        want[at] = sub
        got = ao_d.cpu()
        same_numbers(got, want)
        assert torch.equal(got.view(torch.int16)[:, ~touched], ao.view(torch.int16)[:, ~touched])     # untouched heads and the padding: their very bits, NaN payloads included
        same_bits(ao_whole, got)                                                              # (the fences)
        if n is not None:
            same_bits(idx_whole, at.to(torch.int32))
        if all(f == 1.0 for f in factors):
            same_bits(ao_whole, ao)                                                           # a table of ones: nothing moved, the NaN payload in place
        else:
            assert not torch.equal(got.view(torch.int16), ao.view(torch.int16))


# =================================================================================================================================
# model level
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def heads_rig():
    """tests/test_gpu_stream_patch.py's rig (4 layers, 4 heads x 128, two clips of 215 tokens, trimmed last layer: 11 consumed rows per clip) and
    the pass that captures the head outputs of every row at every layer."""
    model, cfg, sd, kw, seg, plain, whole = rig()
    hwhole = model(**kw, **READS, return_heads=torch.ones_like(kw["attention_mask"]))
    torch.cuda.synchronize()
    return model, cfg, sd, kw, seg, plain, whole, hwhole


def heads_of(hwhole, mask):
    """The rows of the all-rows capture that a mask [B, N] selects: (heads [n, L, n_heads, D], their index [n, 2] on the host)."""
    index = hwhole["heads_index"].cpu()
    own = mask[index[:, 0], index[:, 1]]
    return hwhole["heads"][own.to(hwhole["heads"].device)], index[own]


def table(cells, s):
    t = torch.ones(LAYERS, HEADS)
    for l, h in cells:
        t[l, h] = s
    return t


# ---- (b) the capture ----------------------------------------------------------------------------------------------------------------
def test_capture_changes_no_other_output_and_selects_rows_like_return_stream():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    assert_same_outputs(hwhole, plain, skip=HEAD_KEYS)
    n = int(hwhole["heads_index"].shape[0])
    assert hwhole["heads"].dtype == BF and tuple(hwhole["heads"].shape) == (n, LAYERS, HEADS, D) and hwhole["heads_index"].dtype == torch.long
    assert n == 2 * 214 and torch.equal(hwhole["heads_index"].cpu(), whole["stream_index"].cpu())      # padding and the dead tail skipped, return_stream's order
    # the row-trimmed last layer alone, and a window that ends in it: the capture makes that attention launch cover every row; nothing else moves
    for window in ((LAYERS - 1, LAYERS), (1, LAYERS)):
        out = model(**kw, **READS, return_heads=torch.ones_like(kw["attention_mask"]), head_layers=window)
        assert_same_outputs(out, plain, skip=HEAD_KEYS)
        assert same(out["heads"], hwhole["heads"][:, window[0]:window[1]]), window
    last = hwhole["heads"][:, LAYERS - 1].float()
    assert torch.isfinite(last).all() and not same(hwhole["heads"][:, LAYERS - 1], hwhole["heads"][:, LAYERS - 2])
    # masks and windows
    part = model(**kw, return_heads=seg["text_after"].long().cuda(), head_layers=(1, 3))
    assert same(part["heads"], heads_of(hwhole, seg["text_after"])[0][:, 1:3]) and same(part["score1"], plain["score1"])
    srow = model(**kw, return_heads=seg["score_row"])
    assert srow["heads_index"].tolist() == [[0, 211], [1, 211]] and same(srow["heads"], heads_of(hwhole, seg["score_row"])[0])
    none = model(**kw, return_heads=torch.zeros_like(seg["frames"]))
    assert tuple(none["heads"].shape) == (0, LAYERS, HEADS, D) and tuple(none["heads_index"].shape) == (0, 2)
    flat = model(**kw, return_heads=seg["score_row"], head_layers=(2, 2))
    assert tuple(flat["heads"].shape) == (2, 0, HEADS, D) and flat["heads_index"].tolist() == [[0, 211], [1, 211]]
    dead = torch.zeros_like(seg["frames"]); dead[:, 214] = True
    assert model(**kw, return_heads=dead)["heads"].shape[0] == 0


def test_capture_of_a_clip_alone_is_the_clip_in_its_batch():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    index = hwhole["heads_index"].cpu()
    for b in range(2):
        one, n = clip_alone(kw, b, frames=FRAMES)
        alone = model(**one, return_heads=torch.ones_like(one["attention_mask"]))
        own = index[:, 0] == b
        assert same(alone["heads"], hwhole["heads"][own.cuda()]), b
        assert torch.equal(alone["heads_index"].cpu()[:, 1], index[own][:, 1]) and not alone["heads_index"][:, 0].any()


@functools.lru_cache(maxsize=None)
def oracle_clip0():
    """Clip 0 alone in bf16 on the host: (the clip's inputs, the oracle's keyword inputs, its plain composed states, per layer the oracle's own wo
    input [n, n_heads, D] and the fp64 attention of the oracle's own rotated q / k / v)."""
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    one, n = clip_alone(kw, 0, frames=FRAMES)
    inputs = dict({k: v for k, v in one.items() if k != "labels"}, img_context_token_id=model.img_context_token_id)
    rec = {}

    def hook(x, w, layer, name):
        y = F.linear(x, w)
        if name == "wqkv":
            rec["qkv", layer] = y
        if name == "wo":
            rec["wo", layer] = x
        return y

    O.LLM_LINEAR_HOOK = hook
    try:
        states = DL.composed_states(sd, cfg, **inputs)
    finally:
        O.LLM_LINEAR_HOOK = None
    l = cfg.llm_config
    nkv, g = l.num_key_value_heads, l.num_attention_heads // l.num_key_value_heads
    cos, sin = O.rope_tables(D, l.rope_theta, n, BF, l.max_position_embeddings, l.rope_scaling)
    pos = torch.arange(n, dtype=torch.long).unsqueeze(0)
    layers = []
    for i in range(LAYERS):
        qkv = rec["qkv", i].view(1, n, nkv, g + 2, D)
        q, k = O.apply_rope(qkv[..., :g, :].reshape(1, n, HEADS, D).transpose(1, 2), qkv[..., g, :].transpose(1, 2), cos, sin, pos)
        truth = attn_truth(q[0].transpose(0, 1), k[0].transpose(0, 1), qkv[0, :, :, g + 1], True, 1.0, math.sqrt(D), torch.float64)
        layers.append((rec["wo", i][0].view(n, HEADS, D), truth))
    return one, inputs, states, layers


def test_every_captured_row_lies_within_the_attention_bar_of_the_oracles_wo_input():
    """Clip 0 alone, every row the pass runs, layers 0 .. L - 1 of the plain pass's capture, against the oracle's own wo input (the eager bf16
    evaluation) under the per-element half of the rule the op-level prefill-attention test applies at D = 128
    (tests/attention_reference.py::check_sequence): with the fp64 attention of the oracle's own q / k / v as truth, the kernel's largest error at
    most 2 x the eager path's largest + 2e-3, every element finite.  A last-layer row the trimmed launch had skipped would hold another layer's
    numbers (O(1) apart) and miss it by orders of magnitude.  The rule's other half compares MEANS over one set of inputs; end to end the two
    sides' layer inputs have drifted apart by the rounding of the layers in front (measured on one MI355X: mean error 1.7e-4 / 4.2e-4 / 6.7e-4 /
    7.5e-4 at layers 0 .. 3 against the eager path's 1.5e-4 / 2.6e-4 / 4.0e-4 / 4.3e-4), so it is applied where the inputs are one: the test below."""
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    one, inputs, states, layers = oracle_clip0()
    got = hwhole["heads"][(hwhole["heads_index"][:, 0] == 0)].cpu().double()
    n = got.shape[0]
    assert n == 214
    for i, (eager, truth) in enumerate(layers):
        e_hip, e_ref = (got[:, i] - truth[:n]).abs(), (eager[:n].double() - truth[:n]).abs()
        print(f"layer {i}: |hip - truth| mean {e_hip.mean():.3e} max {e_hip.max():.3e}; |eager - truth| mean {e_ref.mean():.3e} max {e_ref.max():.3e}; "
              f"|hip - eager| max {(got[:, i] - eager[:n].double()).abs().max():.3e}")
    for i, (eager, truth) in enumerate(layers):
        e_hip, e_ref = (got[:, i] - truth[:n]).abs(), (eager[:n].double() - truth[:n]).abs()
        assert torch.isfinite(got[:, i]).all() and e_hip.max() <= 2.0 * e_ref.max() + 2e-3, (i, e_hip.max().item(), e_ref.max().item())


def test_captured_heads_of_a_layer_fed_the_oracles_stream_pass_the_whole_attention_rule():
    """The same rows and layers with the layer inputs made one: the oracle's stream at depth l is patched over every row in front of layer l
    (forward(stream_patch=...)), and the heads captured at layer l - so norm, wqkv, RoPE and attention of one layer run on the oracle's very
    input - must pass check_sequence whole: mean error at most 1.5 x the eager path's + 1e-4, largest at most 2 x its largest + 2e-3.  Layer L - 1
    is the row-trimmed one.  (Measured on one MI355X: mean error 1.45e-4 / 2.57e-4 / 3.92e-4 / 4.22e-4 at layers 0 .. 3 against the eager path's
    1.51e-4 / 2.61e-4 / 3.95e-4 / 4.26e-4, largest 2.8e-3 / 4.2e-3 / 5.2e-3 / 4.4e-3 against 3.7e-3 / 5.0e-3 / 5.9e-3 / 5.5e-3.)"""
    from aigv_assessor_amd.readouts import StreamPatch
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    one, inputs, states, layers = oracle_clip0()
    every = one["attention_mask"].clone()
    every[:, -1] = False                                                                      # (the closing token is not run: the dead tail)
    n = int(every.sum())
    for i, (eager, truth) in enumerate(layers):
        out = model(**one, stream_patch=StreamPatch(every, states[i][0, :n, None].contiguous(), (i, i + 1)), return_heads=every, head_layers=(i, i + 1))
        got = out["heads"][:, 0].cpu().double()
        e_hip, e_ref = (got - truth[:n]).abs(), (eager[:n].double() - truth[:n]).abs()
        print(f"layer {i}, the oracle's input: |hip - truth| mean {e_hip.mean():.3e} max {e_hip.max():.3e}; |eager - truth| mean {e_ref.mean():.3e} max {e_ref.max():.3e}")
        check_sequence(got, truth[:n], eager[:n].double())


# ---- (c) the identities --------------------------------------------------------------------------------------------------------------
def test_self_patch_changes_no_output():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    every = torch.ones_like(kw["attention_mask"])
    some = torch.tensor([[True, False, True, False], [False, False, False, True]])
    for mask, layers, heads in ((every, (0, LAYERS), None), (seg["frames"], (1, 3), some), (seg["score_row"], (3, 4), None),
                                (seg["text_after"] | seg["motion"], (0, 1), some[0])):
        cap = model(**kw, return_heads=mask, head_layers=layers)
        for values, idx in ((cap["heads"], cap["heads_index"]), (cap["heads"].cpu(), None)):          # on the device with the index, on the host without
            out = model(**kw, **READS, head_patch=HeadPatch(mask, values, layers, idx, heads))
            assert_same_outputs(out, plain)
    # an empty window, an empty selection, no head: the plain pass
    z = lambda n, l: torch.zeros(n, l, HEADS, D, dtype=BF)
    for patch in (HeadPatch(every, z(428, 0), (2, 2)), HeadPatch(torch.zeros_like(every), z(0, 2), (1, 3)),
                  HeadPatch(every, z(428, 1), (1, 2), None, torch.zeros(HEADS, dtype=torch.bool))):
        assert_same_outputs(model(**kw, **READS, head_patch=patch), plain)


def test_all_ones_scale_changes_no_output_and_arms_nothing():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    armed = []
    keep = model._prefill
    model._prefill = lambda *a, **k: (armed.append(k.get("head_scale")), keep(*a, **k))[1]
    try:
        for rows in (None, seg["score_row"]):
            assert_same_outputs(model(**kw, **READS, head_scale=HeadScale(torch.ones(LAYERS, HEADS), rows)), plain)
        out = model(**kw, **READS, head_scale=HeadScale(table([(1, 2)], 0.0), torch.zeros_like(seg["frames"])))      # no row: the plain pass
        assert_same_outputs(out, plain)
        assert armed == [None, None, None]
        # one entry off 1: armed; the layers whose row of the table is all ones launch nothing, so the stream in front of layer 1 keeps its bits
        out = model(**kw, **READS, head_scale=HeadScale(table([(1, 2)], 0.5)))
        assert armed[-1] is not None and same(out["lens_score_hidden"][:, :2], plain["lens_score_hidden"][:, :2])
        assert not same(out["lens_score_hidden"][:, 2], plain["lens_score_hidden"][:, 2])
    finally:
        del model._prefill


@pytest.mark.parametrize("s", [0.0, -1.0, 1.7])
def test_scale_is_capture_torch_patch(s):
    """For layer l and head h: pass A captures layer l; torch computes (x.float() * s).bfloat16() on head h; pass B patches it with heads = {h};
    pass C runs head_scale.  B and C agree on every output, bit for bit - over every row, and over the rows of a mask."""
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    every = torch.ones_like(kw["attention_mask"])
    for (l, h), mask in (((1, 2), every), ((0, 3), seg["text_after"]), ((LAYERS - 1, 0), seg["score_row"])):
        a = model(**kw, return_heads=mask, head_layers=(l, l + 1))
        values = a["heads"].clone()
        values[:, 0, h] = (values[:, 0, h].float() * s).to(BF)
        only = torch.zeros(HEADS, dtype=torch.bool); only[h] = True
        b = model(**kw, **READS, return_heads=every, head_patch=HeadPatch(mask, values, (l, l + 1), a["heads_index"], only))
        c = model(**kw, **READS, return_heads=every, head_scale=HeadScale(table([(l, h)], s), None if mask is every else mask))
        assert_same_outputs(c, b)
        assert same(c["heads"][:, :l], hwhole["heads"][:, :l]) and not same(c["heads"][:, l], hwhole["heads"][:, l])


def test_patch_with_a_heads_mask_read_back_by_a_capture_in_the_same_pass():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    g = torch.Generator().manual_seed(13)
    mask = seg["text_after"]
    own, _ = heads_of(hwhole, mask)
    n = own.shape[0]
    values = torch.randn(n, 2, HEADS, D, generator=g).to(BF)
    values[0, 0, 1, 3] = float("nan")
    sel = torch.tensor([[False, True, False, True], [True, False, False, False]])
    out = model(**kw, **READS, return_heads=mask, head_layers=(1, 3), head_patch=HeadPatch(mask, values, (1, 3), None, sel))
    got = out["heads"]
    assert same(got[:, 0][:, sel[0]], values[:, 0][:, sel[0]].cuda()) and same(got[:, 1][:, sel[1]], values[:, 1][:, sel[1]].cuda())     # the selected heads carry the values
    assert same(got[:, 0][:, ~sel[0]], own[:, 1][:, ~sel[0]])                                 # the others the plain pass's bits at layer lo
    assert not same(got[:, 1][:, ~sel[1]], own[:, 2][:, ~sel[1]])                             # (behind lo they are those of the patched pass)
    assert got[0, 0, 1, 3].isnan() and not same(out["score1"], plain["score1"])
    # scale, patch, capture in one pass: the capture returns what wo consumes - the patch over the scaled rows
    both = model(**kw, return_heads=mask, head_layers=(1, 2), head_scale=HeadScale(table([(1, 0), (1, 1)], 0.0), mask),
                 head_patch=HeadPatch(mask, values[:, :1].contiguous(), (1, 2), None, sel[0]))
    assert same(both["heads"][:, 0, 1], values[:, 0, 1].cuda()) and not both["heads"][:, 0, 0].any() and same(both["heads"][:, 0, 2], own[:, 1, 2])


# ---- (d) against the composed oracle ------------------------------------------------------------------------------------------------------
KNOCKOUTS = (((0,), (2,), 0.0), ((2,), (0, 1, 2, 3), 0.0), ((0,), (0,), 0.0), ((3,), (0, 1, 2, 3), 0.0), ((0,), (0,), -1.0))


@pytest.mark.parametrize("case", range(len(KNOCKOUTS)), ids=[f"layers{ls}-heads{hs}-x{s}" for ls, hs, s in KNOCKOUTS])
def test_knocked_out_pass_against_the_composed_oracle(case):
    """Clip 0 alone; the five cases of tests/test_head_patch_cpu.py, each of which moves the oracle's own score by at least 2 bf16 ulps.  score1
    within the tiny rig's bar (1e-3 or 1 bf16 ulp of the oracle's value) for all five; for the first two - the oracle itself decides at most one
    answer row within 2 bf16 ulps there - the answer tokens identical up to at most 1 such row."""
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    one, inputs, own, _ = oracle_clip0()
    layers, heads, s = KNOCKOUTS[case]
    t = table([(l, h) for l in layers for h in heads], s)
    states, _ = HP.composed_states(sd, cfg, **inputs, scale=t)
    ref = HP.lens(sd, cfg, states, one["attention_mask"], one["labels"], 2)
    out = model(**one, head_scale=HeadScale(t))
    print(f"layers {layers} heads {heads} x {s}: plain {plain['score1'][0].item():.5f}")
    score_ok(out["score1"], ref["score"][:, LAYERS])
    assert not same(out["score1"], plain["score1"][0:1])                                       # the knocked score differs from the plain one
    if case < 2:
        w, eps = sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps
        logits = O.lm_logits(sd, O.rms_norm_cast_then_scale(states[LAYERS], w, eps))[0, :-1]
        want = one["labels"][0, 1:] != -100
        assert assert_levels(out["logit"].cpu()[want], logits[want].argmax(-1), logits[want]) <= 1


# ---- (e) combinations ----------------------------------------------------------------------------------------------------------------
def test_with_a_key_drop_window_the_lens_in_front_of_both_windows_keeps_the_plain_bits():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    knock = dict(key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(2, 4))
    t = table([(2, 1), (3, 0)], 0.0)
    out = model(**kw, **READS, **knock, head_scale=HeadScale(t, only_clip(torch.ones_like(kw["attention_mask"]), 1)))
    knocked = model(**kw, **READS, **knock)
    for key in LENS_HIDDEN + ("lens_score",):
        assert same(out[key][:, :3], plain[key][:, :3]), key                                  # layers 0 and 1 ran as they always do; depth 2 feeds the first armed layer
        assert same(out[key][0], knocked[key][0]), key                                        # clip 0 carries the key-drop only
    assert not same(out["lens_score_hidden"][1, 3:], knocked["lens_score_hidden"][1, 3:])
    assert same(out["lens_score"][:, LAYERS].to(BF), out["score1"])


def test_a_stream_capture_behind_the_layer_differs_exactly_at_the_touched_clips():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    every = torch.ones_like(kw["attention_mask"])
    l = 1
    out = model(**kw, return_stream=every, stream_depths=(l, l + 2), head_scale=HeadScale(table([(l, 0)], 0.0), only_clip(every, 1)))
    clip = whole["stream_index"][:, 0]
    assert same(out["stream"][:, 0], whole["stream"][:, l])                                   # depth l: what layer l consumes, in front of its attention
    assert same(out["stream"][clip == 0, 1], whole["stream"][clip == 0, l + 1])               # clip 0: not touched
    rows1 = (out["stream"][clip == 1, 1].view(torch.int16) != whole["stream"][clip == 1, l + 1].view(torch.int16)).any(-1)
    assert rows1.all()                                                                        # clip 1: every row of it


def test_fp8_mode_self_patch_is_bit_neutral():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    model.set_precision("fp8")
    try:
        plain8 = model(**kw, **READS)
        mask = seg["frames"] | seg["score_row"]
        cap = model(**kw, return_heads=mask, head_layers=(1, 4))
        out = model(**kw, **READS, head_patch=HeadPatch(mask, cap["heads"], (1, 4), cap["heads_index"]))
        assert_same_outputs(out, plain8)
        assert not same(plain8["lens_score_hidden"], plain["lens_score_hidden"])              # another arithmetic from layer 0 on
        assert not same(model(**kw, head_scale=HeadScale(table([(1, 1)], 0.0)))["score1"], plain8["score1"])
    finally:
        model.set_precision("bf16")
    assert_same_outputs(model(**kw, **READS), plain)


def test_graph_replay_runs_armed_calls_eagerly():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    own, idx = heads_of(hwhole, only_clip(seg["score_row"], 0))
    armed_kw = dict(return_heads=seg["text_after"], head_layers=(1, 3), head_scale=HeadScale(table([(0, 1)], 0.0)),
                    head_patch=HeadPatch(only_clip(seg["score_row"], 1), own[:, 2:3].contiguous(), (2, 3)))
    eager = model(**kw, **READS, **armed_kw)
    assert not same(eager["score1"], plain["score1"])
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    model.enable_graph_replay(True)
    try:
        graphs = lambda: sum(isinstance(v, tuple) for v in model._graphs.values())
        outs = [model(**dev_kw, **READS) for _ in range(3)]                                   # eager, capture, replay
        assert graphs() == 1 and len(model._graphs) == 1
        armed = [model(**dev_kw, **READS, **armed_kw) for _ in range(2)]
        only_capture = model(**dev_kw, **READS, return_heads=seg["text_after"], head_layers=(1, 3))
        only_scale = model(**dev_kw, **READS, head_scale=armed_kw["head_scale"])
        assert graphs() == 1 and len(model._graphs) == 1                                       # nothing captured, nothing even remembered
        again = model(**dev_kw, **READS)                                                      # replays; the armed passes before it disarmed
        assert graphs() == 1 and len(model._graphs) == 1
        torch.cuda.synchronize()
        for o in outs + [again]:
            assert_same_outputs(o, plain)
        for o in armed:
            assert_same_outputs(o, eager)
        assert_same_outputs(only_capture, plain, skip=HEAD_KEYS)
        assert same(only_capture["heads"], heads_of(hwhole, seg["text_after"])[0][:, 1:3]) and not same(only_scale["score1"], plain["score1"])
    finally:
        model.enable_graph_replay(False)
    assert_same_outputs(model(**kw, **READS), plain)


# ---- (f) head_knockout and head_trace ---------------------------------------------------------------------------------------------------
def test_head_knockout_on_the_rig():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    calls = []
    keep = model.vit_tokens
    model.vit_tokens = lambda pv: (calls.append(int(pv.shape[0])), keep(pv))[1]
    try:
        res = eval_utils.head_knockout(model, **kw, layers=[0, 2], candidate_ids=CAND)
        assert calls == [4]                                                                   # InternViT ran once
        rows = only_clip(seg["score_row"], 1)
        part = eval_utils.head_knockout(model, **kw, layers=[3], heads=[1, 3], rows=rows)
    finally:
        del model.vit_tokens
    assert res["layers"] == [0, 2] and res["heads"] == [0, 1, 2, 3] and len(res["outs"]) == 1 + 2 * 4
    assert same(res["score1"], plain["score1"].float()) and same(res["outs"][0]["cand_logprob"], plain["cand_logprob"])       # outs[0] is the plain pass
    assert tuple(res["knocked"].shape) == (2, 2, 4) and torch.isfinite(res["knocked"]).all() and same(res["delta"], res["score1"][:, None, None] - res["knocked"])
    assert (res["delta"] != 0).any()
    by_hand = model(**kw, head_scale=HeadScale(table([(2, 3)], 0.0)))                          # one cell recomputed by hand
    assert same(res["knocked"][:, 1, 3], by_hand["score1"].float())
    # rows: the knock-out restricted to clip 1's score row - NaN for the clip the mask selects no row of
    assert tuple(part["knocked"].shape) == (2, 1, 2) and part["knocked"][0].isnan().all() and torch.isfinite(part["knocked"][1]).all()
    by_hand = model(**kw, head_scale=HeadScale(table([(3, 3)], 0.0), rows))
    assert same(part["knocked"][1, 0, 1], by_hand["score1"].float()[1]) and same(by_hand["score1"][:1], plain["score1"][:1])


def test_head_trace_on_the_rig():
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    swap = torch.tensor([1, 0])
    frames = torch.tensor([2, 3, 0, 1])
    corrupt = dict(kw, input_ids=kw["input_ids"][swap], labels=kw["labels"][swap], pixel_values=kw["pixel_values"][frames], motion_feature=kw["motion_feature"][swap])
    calls = []
    keep = model.vit_tokens
    model.vit_tokens = lambda pv: (calls.append(int(pv.shape[0])), keep(pv))[1]
    try:
        res = eval_utils.head_trace(model, clean=kw, corrupt=corrupt, layers=[1, 3], candidate_ids=CAND)
        assert calls == [4, 4]                                                                # InternViT ran as often as in two passes
    finally:
        del model.vit_tokens
    assert res["layers"] == [1, 3] and res["heads"] == [0, 1, 2, 3] and len(res["outs"]) == 2 + 2 * 4
    assert same(res["clean_score"], plain["score1"].float()) and same(res["corrupt_score"], plain["score1"].float()[swap.cuda()])
    assert tuple(res["score"].shape) == (2, 2, 4) and tuple(res["restored"].shape) == (2, 2, 4)
    assert same(res["restored"], eval_utils.restored_fraction(res["score"], res["clean_score"], res["corrupt_score"]))
    assert torch.isfinite(res["restored"]).all() and (res["restored"] != 0).any()
    assert same(res["outs"][0]["heads"], hwhole["heads"]) and torch.equal(res["outs"][0]["heads_index"].cpu(), hwhole["heads_index"].cpu())
    # NaN where clean and corrupt score the same: a batch traced against itself
    own = eval_utils.head_trace(model, clean=kw, corrupt=dict(kw), layers=[0], heads=[1])
    assert own["restored"].isnan().all() and same(own["score"][:, 0, 0], plain["score1"].float())      # (and the self-patch kept the score)
    # every head of a layer patched over every row: the mask that names them all, per layer or for the window, is the one call without a mask
    every = kw["attention_mask"].clone()
    l = LAYERS - 1
    donor = res["outs"][0]
    values = donor["heads"][:, l:l + 1].contiguous()
    once = model(**corrupt, head_patch=HeadPatch(every, values, (l, l + 1), donor["heads_index"]))
    for sel in (torch.ones(HEADS, dtype=torch.bool), torch.ones(1, HEADS, dtype=torch.bool)):
        assert same(model(**corrupt, head_patch=HeadPatch(every, values, (l, l + 1), donor["heads_index"], sel))["score1"], once["score1"])
    assert not same(once["score1"], res["outs"][1]["score1"])
    again = eval_utils.head_trace(model, clean=kw, corrupt=corrupt, layers=[l], heads=[0])
    assert same(again["score"][:, 0, 0], res["score"][:, 1, 0])                               # the same cell from two sweeps


# ---- (g) refusals through the C ABI --------------------------------------------------------------------------------------------------------
def test_refusals_at_the_pass_come_with_a_message_and_no_fault(lib):
    model, cfg, sd, kw, seg, plain, whole, hwhole = heads_rig()
    ctx = model._ctx
    H = HEADS * D
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 4)
    T = plan["cu"][-1]
    buf = torch.zeros(4, 1, H, dtype=BF, device="cuda")
    ones = (native.C.c_float * (LAYERS * HEADS))(*([1.0] * (LAYERS * HEADS)))
    half = (native.C.c_float * (LAYERS * HEADS))(*([0.5] * (LAYERS * HEADS)))
    err = lambda: lib.aigv_last_error(ctx).decode()

    def plain_again():
        torch.cuda.synchronize()
        assert_same_outputs(model(**kw, **READS), plain)

    arms = {"capture": lambda rows, n, lo, hi, b: lib.aigv_head_capture_arm(ctx, rows, n, lo, hi, b),
            "patch": lambda rows, n, lo, hi, b: lib.aigv_head_patch_arm(ctx, rows, n, lo, hi, None, b),
            "scale": lambda rows, n, lo, hi, b: lib.aigv_head_scale_arm(ctx, rows, n, half)}
    # refused by the arm calls: nothing armed
    for what in ("capture", "patch"):
        for args, word in (((i32([0, 1]), -1, 0, 1, buf.data_ptr()), "-1 rows outside 0..max_tokens"), ((None, 2, 0, 1, buf.data_ptr()), "null row list"),
                           ((i32([0, 1]), 2, 0, 1, None), "null or not 16-byte aligned"), ((i32([0, 1]), 2, 0, 1, buf.data_ptr() + 8), "null or not 16-byte aligned")):
            assert arms[what](*args) == -1 and word in err() and err().startswith(f"aigv_head_{what}_arm:"), (what, args, err())
    nan = (native.C.c_float * (LAYERS * HEADS))(*([1.0] * 5 + [float("nan")] + [1.0] * (LAYERS * HEADS - 6)))
    assert lib.aigv_head_scale_arm(ctx, None, 0, nan) == -1 and "scale[1][1] is NaN" in err()
    assert lib.aigv_head_scale_arm(ctx, None, 0, None) == -1 and "null scale table" in err()
    assert lib.aigv_head_scale_arm(ctx, i32([0, 1]), -1, ones) == -1 and "-1 rows outside 0..max_tokens" in err()
    plain_again()

    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    prefill = lambda **k: model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"], **k)
    # refused by the pass, before any launch; the context disarms
    for what in ("capture", "patch", "scale"):
        cases = [([0, 5, T], 0, 1, f"row 2 \\(packed row {T}\\) outside \\[0, {T}\\)"), ([0, 9, 5], 0, 1, "rows 1 and 2 \\(packed rows 9, 5\\) are not strictly ascending"),
                 ([0, 5, 5], 0, 1, "not strictly ascending")]
        if what != "scale":                                                                   # (the scale's window is its table: [0, L))
            cases += [([0, 5, 9], 4, 5, f"depths \\[4, 5\\) outside 0 <= lo <= hi <= {LAYERS}"), ([0, 5, 9], 2, 1, "depths \\[2, 1\\) outside")]
        for rows, lo, hi, word in cases:
            assert arms[what](i32(rows), 3, lo, hi, buf.data_ptr()) == 0
            with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: the head {what} .*" + word):
                prefill()
            plain_again()
        assert arms[what](i32([0, 5, 9]), 3, 0, 1, buf.data_ptr()) == 0
        with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: keep_kv while a head {what} is armed"):
            prefill(keep_kv=True, kv_cap=256)
        plain_again()
        # a window that reaches layer L - 1 in a pass without output rows: its last attention does not run
        assert arms[what](i32([0, 5, 9]), 3, LAYERS - 1, LAYERS, buf.data_ptr()) == 0
        with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: a head option reaches layer {LAYERS - 1} and the pass has no output rows"):
            model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, None, [])
        plain_again()

    # aigv_llm_extend while armed (the shared-prefix path arms nothing itself: arm by hand behind its prefill)
    base = synth.canonical_tokens(cfg, 2, 2, seed=77)
    pp = synth.perspective_prompts(base, 2, seed=77)
    common = dict(pixel_values=synth.synthetic_frames(4, 224, seed=77), image_flags=torch.ones(4, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(2, cfg.motion_dim, seed=77))
    keep = model._prefill
    for what in ("capture", "patch", "scale"):
        def prefill_then_arm(*a, **k):
            out = keep(*a, **k)
            assert arms[what](i32([0, 5, 9]), 3, 0, 1, buf.data_ptr()) == 0
            return out

        model._prefill = prefill_then_arm
        try:
            with pytest.raises(native.NativeError, match=f"aigv_llm_extend: a head {what} is armed"):
                model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common)
        finally:
            del model._prefill
        plain_again()                                                                         # the refused continuation disarmed too
    with pytest.raises(TypeError):
        model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_heads=seg["frames"])
