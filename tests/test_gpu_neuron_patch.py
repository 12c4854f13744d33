"""MLP neuron knock-out and neuron patching on the GPU: (a) the neuron-rows kernel in its three modes and two column forms against torch indexing /
torch arithmetic, between fences; (b) the capture of forward(return_neurons=...) against the pass itself - dense, sparse, the row-trimmed last
layer - and against the oracle's w2 input; (c) the identities of forward(neuron_patch=...) and forward(neuron_scale=...) on the 4-layer rig of
tests/test_gpu_stream_patch.py - a self-patch and factors of one change nothing, a scale is capture + torch + patch, a capture reads the patch, the
order scale, patch, capture; (d) the knocked-out pass against the composed oracle of tests/neuron_patch_reference.py; (e) with a key-drop window, a
stream capture, a head capture, in fp8 mode, under graph replay; (f) eval_utils.mlp_knockout, neuron_knockout and neuron_trace; (g) the refusals
of the C ABI, each by its message."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import depth_lens_reference as DL
import neuron_patch_reference as NP
from test_gpu_key_drop import assert_levels, clip_alone, same, score_ok
from test_gpu_ops import BF, dev, lib, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import fenced, i32, ptr, same_bits, sentinel_like
from test_gpu_stream_patch import CAND, FRAMES, LAYERS, LENS_HIDDEN, READS, assert_same_outputs, only_clip, rig
from test_neuron_patch_cpu import KNOCKOUTS, TOKEN_CASES, knockout_options, neuron_scale_of, oracle_score_row_capture
from test_stream_patch_cpu import oracle_rig

from aigv_assessor_amd import eval_utils, native, synth
from aigv_assessor_amd.readouts import HeadPatch, NeuronPatch, NeuronScale, StreamPatch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INTER, HEADS, D = 768, 4, 128
NEURON_KEYS = ("neurons", "neurons_index")
CAPTURE, PATCH, SCALE = 0, 1, 2
R = 150                                                                                       # rows of the op-level activation buffer


# =================================================================================================================================
# (a) the kernel
# =================================================================================================================================
def column_lists(I):
    """None: the dense form.  The sparse lists: the first column, the last, two columns of one dword, 257 columns (the stride-256 loop wraps by
    one; from I = 264 on), every column (which must equal the dense result)."""
    lists = {"dense": None, "first": [0], "last": [I - 1], "one-dword": [6, 7], "every": list(range(I))}
    if I >= 264:
        lists["257"] = list(range(255)) + [I - 2, I - 1]                                      # (6 and 7 among them; fits I = 264)
    return lists


def special_row(row, I, payload=0x7FA5):
    """A NaN, a +Inf, a -Inf and a -0 payload in a row of >= I elements, and a signalling NaN with a payload of its own in its last column."""
    row[5], row[I // 2], row[I // 4], row[1] = float("nan"), float("inf"), float("-inf"), -0.0
    row.view(torch.int16)[I - 1] = payload                                                    # the copy moves bits; arithmetic would quiet it
    return row


def pick_rows(g, n, first):
    if n is None:
        return list(range(R))
    if n == 1:
        return [R - 1] if first else [0]
    inner = (torch.randperm(R - 2, generator=g)[:n - 2] + 1).sort().values.tolist()
    return [0] + inner + [R - 1]                                                              # the first and the last row, strictly ascending


def launch(lib, act_d, ld, rows, n, side_d, n_layers, layer, I, mode, cols=None, sidx=None, n_side=0, factors=None, factor=1.0):
    """One aigv_op_neuron_rows call; rows None: no row list (rows 0 .. R - 1).  -> the fenced device tables (whole, expected image) the op wrote."""
    tables = []

    def table(values, dtype=torch.int32):
        if values is None:
            return None
        whole, d = fenced(sentinel_like((len(values),), dtype))
        tables.append((whole, torch.tensor(values, dtype=dtype)))
        return ptr(d)

    idx_p, sidx_p, cols_p = table(rows), table(sidx), table(cols if cols else None)
    fac_p = table(factors if factors else None, torch.float32)
    sync(lib.aigv_op_neuron_rows(ptr(act_d), ld, R, None if rows is None else i32(rows), n, idx_p, None if sidx is None else i32(sidx), sidx_p, n_side,
                                 None if side_d is None else ptr(side_d), n_layers, layer, I, None if cols is None else i32(cols), 0 if cols is None else len(cols), cols_p, mode,
                                 None if factors is None else (native.C.c_float * len(factors))(*factors), fac_p, factor, None), lib)
    for whole, want in tables:
        same_bits(whole, want)                                                                # the lists went up whole, and nothing beside them
    return tables


@pytest.mark.parametrize("pad", [0, 64], ids=["ld=I", "ld=I+64"])
@pytest.mark.parametrize("n", [1, 5, 130, None], ids=["n=1", "n=5", "n=130", "no-row-list"])
@pytest.mark.parametrize("I", [8, 264, 2056, 14336])
def test_capture_and_patch_against_torch_indexing(lib, I, n, pad):
    """I = 8: a single 16-byte chunk; 2056: 257 chunks, the stride-256 loop wraps by one; 14336: the production width.  1 and 3 layers per side
    buffer, with the side rows in order and through a side-row list.  Every byte outside the selection - the other columns (5 and 8 beside [6, 7]),
    the other rows and layers, the padding, the side rows nothing names, the fences - keeps its bits; NaN, Inf and -0 payloads travel bit for bit."""
    g = torch.Generator().manual_seed(I + 7 * (n or 0) + pad)
    ld = I + pad
    act = (torch.randn(R, ld, generator=g) * 3).to(BF)
    for n_layers, with_sidx in ((1, False), (3, False), (3, True)):
        layer = n_layers // 2
        rows = pick_rows(g, n, n_layers == 1)
        m = len(rows)
        at = torch.tensor(rows)
        act[rows[0]] = special_row(act[rows[0]].clone(), I)
        n_side = m + 3 if with_sidx else m
        sidx = [n_side - 1 - i for i in range(m)] if with_sidx else None                      # the side rows backwards, three of them unnamed
        srow = torch.tensor(sidx) if with_sidx else torch.arange(m)
        dense_result = None
        for name, cols in column_lists(I).items():
            W = I if cols is None else len(cols)
            c = torch.arange(I) if cols is None else torch.tensor(cols)
            values = (torch.randn(n_side, n_layers, W, generator=g) * 3).to(BF)
            values[srow[0], layer] = special_row(values[srow[0], layer].clone(), W, 0x7FB3) if W >= 8 else values[srow[0], layer]
            if W < 8:
                values.view(torch.int16)[srow[0], layer, W - 1] = 0x7FB3
            # capture: side(si, layer) = act[rows[i]] in the selected columns
            act_whole, act_d = fenced(act)
            side_whole, side_d = fenced(sentinel_like((n_side, n_layers, W), BF))
            launch(lib, act_d, ld, None if n is None else rows, m, side_d, n_layers, layer, I, CAPTURE, cols, sidx, n_side)
            want = sentinel_like((n_side, n_layers, W), BF)
            want[srow, layer] = act[at][:, c]
            same_bits(side_whole, want)
            same_bits(act_whole, act)
            if name == "dense":
                dense_result = want
            if name == "every":
                assert torch.equal(want.view(torch.int16), dense_result.view(torch.int16))    # every column: the dense result
            # patch: act[rows[i]] = side(si, layer) in the selected columns
            act_whole, act_d = fenced(act)
            side_whole, side_d = fenced(values)
            launch(lib, act_d, ld, None if n is None else rows, m, side_d, n_layers, layer, I, PATCH, cols, sidx, n_side)
            want = act.clone()
            sub = want[at]
            sub[:, c] = values[srow, layer]
            want[at] = sub
            same_bits(act_whole, want)
            same_bits(side_whole, values)
            assert not torch.equal(want.view(torch.int16), act.view(torch.int16))
            if name == "one-dword":
                assert torch.equal(want.view(torch.int16)[:, 5], act.view(torch.int16)[:, 5])
                assert torch.equal(want.view(torch.int16).reshape(-1)[8::ld], act.view(torch.int16).reshape(-1)[8::ld])     # column 8 (I = 8: the next element in memory)


SCALES = (0.0, 1.0, -1.0, 0.5, 1.7, 3e38)
EDGE = torch.tensor([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x3F80, 0x0040], dtype=torch.int32).to(torch.int16)


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


@pytest.mark.parametrize("pad", [0, 64], ids=["ld=I", "ld=I+64"])
@pytest.mark.parametrize("n", [1, 5, 130, None], ids=["n=1", "n=5", "n=130", "no-row-list"])
@pytest.mark.parametrize("I", [8, 264, 2056, 14336])
def test_scale_against_torch_arithmetic(lib, I, n, pad):
    """act = bf16(fp32(act) * s) over the listed rows.  Dense: one factor for the row, each of SCALES in turn; the first selected row holds +-0,
    subnormals, the smallest normal, the largest finite value, +-Inf and 1 (as many as fit), and a signalling NaN with a payload in the last column.
    Sparse: column lists with factor SCALES[j % 6] for entry j; the second selected row (the first when there is one) holds the edge values in runs
    of 6 columns, so every factor meets every edge value from I = 264 on.  A factor of exactly 1 leaves its elements untouched - the dense launch
    does not happen, the sparse lane neither reads nor writes: the signalling NaN keeps its payload bits, which any arithmetic would have quieted.
    NaN results (0 x Inf) compare as NaN."""
    g = torch.Generator().manual_seed(I + 7 * (n or 0) + pad + 1)
    ld = I + pad
    rows = pick_rows(g, n, False)
    at = torch.tensor(rows)
    act = (torch.randn(R, ld, generator=g) * 3).to(BF)
    first = act[rows[0]].view(torch.int16)
    first[:min(I - 1, EDGE.numel())] = EDGE[:min(I - 1, EDGE.numel())]
    first[I - 1] = 0x7FA5
    second = act[rows[min(1, len(rows) - 1)]].view(torch.int16)
    if I >= 264:
        second[:72] = EDGE.repeat_interleave(6)
    second[I - 1] = 0x7FA5
    payload = lambda t: t.view(torch.int16)[rows[0], I - 1].item() == 0x7FA5
    for s in SCALES:                                                                          # ---- dense
        act_whole, act_d = fenced(act)
        launch(lib, act_d, ld, None if n is None else rows, len(rows), None, 0, 0, I, SCALE, factor=s)
        want = act.clone()
        if s != 1.0:
            sub = want[at]
            sub[:, :I] = scaled(sub[:, :I], s)
            want[at] = sub
        got = act_d.cpu()
        same_numbers(got, want)
        same_bits(act_whole, got)                                                             # (the fences)
        assert torch.equal(got.view(torch.int16)[:, I:], act.view(torch.int16)[:, I:])        # the padding: its very bits
        others = torch.ones(R, dtype=torch.bool); others[at] = False
        assert torch.equal(got.view(torch.int16)[others], act.view(torch.int16)[others])      # the rows not listed likewise
        if s == 1.0:
            same_bits(act_whole, act)                                                         # nothing was launched: the signalling NaN in place
            assert payload(got)
        else:
            assert not torch.equal(got.view(torch.int16), act.view(torch.int16)) and not payload(got)
    for name, cols in column_lists(I).items():                                                # ---- sparse
        if cols is None:
            continue
        factors = [SCALES[j % 6] for j in range(len(cols))]
        if name == "last":
            factors = [1.0]                                                                   # the last column by 1: its NaN payload stays
        act_whole, act_d = fenced(act)
        launch(lib, act_d, ld, None if n is None else rows, len(rows), None, 0, 0, I, SCALE, cols, factors=factors)
        want = act.clone()
        sub = want[at]
        touched = torch.zeros(ld, dtype=torch.bool)
        for col, f in zip(cols, factors):
            if f != 1.0:
                sub[:, col] = scaled(sub[:, col], f)
                touched[col] = True
        want[at] = sub
        got = act_d.cpu()
        same_numbers(got, want)
        same_bits(act_whole, got)
        assert torch.equal(got.view(torch.int16)[:, ~touched], act.view(torch.int16)[:, ~touched])      # untouched columns (factor 1 among them) and the padding: their very bits
        if name == "last":
            same_bits(act_whole, act)
            assert payload(got)
        elif name in ("every", "257"):                                                        # (a short list may meet zeros only: 0 x 0 keeps its bits)
            assert not torch.equal(got.view(torch.int16), act.view(torch.int16))


# =================================================================================================================================
# model level
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def neurons_rig():
    """tests/test_gpu_stream_patch.py's rig (4 layers, I = 768, two clips of 215 tokens, trimmed last layer: 11 consumed rows per clip - the score
    row and 10 answer rows, the score row being one of them: 10 distinct rows, one of them finished twice) and the pass that captures every neuron
    of every row at every layer; `consumed`: bool [n], the captured rows the last layer finishes."""
    model, cfg, sd, kw, seg, plain, whole = rig()
    nwhole = model(**kw, **READS, return_neurons=torch.ones_like(kw["attention_mask"]))
    torch.cuda.synchronize()
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 4)
    index = nwhole["neurons_index"].cpu()
    packed = plan["row_of"][index[:, 0], index[:, 1]]
    out_rows = torch.tensor([int(r) for r in plan["score_rows"]] + [int(r) for r in plan["logit_rows"]])
    consumed = (packed[:, None] == out_rows[None]).any(1)
    return model, cfg, sd, kw, seg, plain, whole, nwhole, consumed


def neurons_of(nwhole, mask):
    """The rows of the all-rows capture that a mask [B, N] selects: (neurons [n, L, I], their index [n, 2] on the host)."""
    index = nwhole["neurons_index"].cpu()
    own = mask[index[:, 0], index[:, 1]]
    return nwhole["neurons"][own.to(nwhole["neurons"].device)], index[own]


def layer_table(cells):
    t = torch.ones(LAYERS)
    for l, s in cells:
        t[l] = s
    return t


COLS = torch.tensor([0, 5, 6, 7, 300, INTER - 1])


# ---- (b) the capture ----------------------------------------------------------------------------------------------------------------
def test_capture_dense_and_sparse_changes_no_other_output():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    every = torch.ones_like(kw["attention_mask"])
    assert_same_outputs(nwhole, plain, skip=NEURON_KEYS)
    n = int(nwhole["neurons_index"].shape[0])
    assert nwhole["neurons"].dtype == BF and tuple(nwhole["neurons"].shape) == (n, LAYERS, INTER) and nwhole["neurons_index"].dtype == torch.long
    assert n == 2 * 214 and torch.equal(nwhole["neurons_index"].cpu(), whole["stream_index"].cpu())      # padding and the dead tail skipped, return_stream's order
    # the sparse capture: the matching columns of the dense one, and no other output moves
    sparse = model(**kw, **READS, return_neurons=every, neuron_ids=COLS)
    assert_same_outputs(sparse, plain, skip=NEURON_KEYS)
    assert tuple(sparse["neurons"].shape) == (n, LAYERS, COLS.numel()) and same(sparse["neurons"], nwhole["neurons"][:, :, COLS.cuda()].contiguous())
    assert torch.equal(sparse["neurons_index"], nwhole["neurons_index"])
    # the row-trimmed last layer alone, and a window that ends in it
    for window in ((LAYERS - 1, LAYERS), (1, LAYERS)):
        for ids in (None, COLS):
            out = model(**kw, **READS, return_neurons=every, neuron_layers=window, neuron_ids=ids)
            assert_same_outputs(out, plain, skip=NEURON_KEYS)
            want = nwhole["neurons"][:, window[0]:window[1]]
            assert same(out["neurons"], (want if ids is None else want[:, :, COLS.cuda()]).contiguous()), (window, ids)
    # masks and windows
    part = model(**kw, return_neurons=seg["text_after"].long().cuda(), neuron_layers=(1, 3))
    assert same(part["neurons"], neurons_of(nwhole, seg["text_after"])[0][:, 1:3].contiguous()) and same(part["score1"], plain["score1"])
    srow = model(**kw, return_neurons=seg["score_row"])
    assert srow["neurons_index"].tolist() == [[0, 211], [1, 211]] and same(srow["neurons"], neurons_of(nwhole, seg["score_row"])[0])
    assert torch.isfinite(srow["neurons"].float()).all()                                      # the score row is a consumed row: layer L - 1 included
    none = model(**kw, return_neurons=torch.zeros_like(seg["frames"]))
    assert tuple(none["neurons"].shape) == (0, LAYERS, INTER) and tuple(none["neurons_index"].shape) == (0, 2)
    flat = model(**kw, return_neurons=seg["score_row"], neuron_layers=(2, 2))
    assert tuple(flat["neurons"].shape) == (2, 0, INTER) and flat["neurons_index"].tolist() == [[0, 211], [1, 211]]
    no_col = model(**kw, return_neurons=seg["score_row"], neuron_ids=torch.zeros(0, dtype=torch.long))
    assert tuple(no_col["neurons"].shape) == (2, LAYERS, 0) and same(no_col["score1"], plain["score1"])
    dead = torch.zeros_like(seg["frames"]); dead[:, 214] = True
    assert model(**kw, return_neurons=dead)["neurons"].shape[0] == 0


def test_capture_at_the_trimmed_last_layer_consumed_rows_hold_numbers_the_others_nan():
    """Layer L - 1 runs for the consumed rows of each clip only (10 distinct ones) - on the weight-streaming path, from its 64-row buffer.  Their captured rows
    are finite and differ from layer L - 2's; every other row has no MLP activation there: NaN, written by the host.  Layers 0 .. L - 2: finite."""
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 4)
    assert len(plan["score_rows"]) + len(plan["logit_rows"]) == 2 * 11 and int(consumed.sum()) == len(set(int(r) for r in list(plan["score_rows"]) + list(plan["logit_rows"]))) == 2 * 10
    got = nwhole["neurons"].float().cpu()
    assert torch.isfinite(got[:, :LAYERS - 1]).all()
    assert torch.isfinite(got[consumed, LAYERS - 1]).all() and got[~consumed, LAYERS - 1].isnan().all()
    last, before = nwhole["neurons"][consumed.cuda(), LAYERS - 1], nwhole["neurons"][consumed.cuda(), LAYERS - 2]
    assert (last.view(torch.int16) != before.view(torch.int16)).any(-1).all()                 # every consumed row: its own layer's numbers
    assert (last.float().abs().amax(-1) > 0).all()


def test_capture_of_a_clip_alone_is_the_clip_in_its_batch():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    index = nwhole["neurons_index"].cpu()
    for b in range(2):
        one, n = clip_alone(kw, b, frames=FRAMES)
        for ids in (None, COLS):
            alone = model(**one, return_neurons=torch.ones_like(one["attention_mask"]), neuron_ids=ids)
            own = index[:, 0] == b
            want = nwhole["neurons"][own.cuda()]
            assert same(alone["neurons"], (want if ids is None else want[:, :, COLS.cuda()]).contiguous()), b      # (NaN slices included: the host's fill)
            assert torch.equal(alone["neurons_index"].cpu()[:, 1], index[own][:, 1]) and not alone["neurons_index"][:, 0].any()


@functools.lru_cache(maxsize=None)
def oracle_clip0():
    """Clip 0 alone in bf16 on the host: (the clip's inputs, the oracle's keyword inputs, its plain composed states, per layer the oracle's own wo
    input [n, H] and w2 input [n, I])."""
    model, cfg, sd, clips = oracle_rig()
    one, inputs, _ = clips[0]
    rec = {}

    def hook(x, w, layer, name):
        if name in ("wo", "w2"):
            rec[name, layer] = x[0]
        return F.linear(x, w)

    O.LLM_LINEAR_HOOK = hook
    try:
        states = DL.composed_states(sd, cfg, **inputs)
    finally:
        O.LLM_LINEAR_HOOK = None
    return one, inputs, states, [(rec["wo", i], rec["w2", i]) for i in range(LAYERS)]


def capture_error(x, ref):
    """The largest |x - ref| in units of a |ref| + b (row maximum of |ref|), a = b = 2^-8: half a bf16 ulp of the element plus half a bf16 ulp
    of its row's largest element (the fp32 sums a SwiGLU output rounds from scale with the row, not with the element)."""
    x, ref = x.double().cpu(), ref.double().cpu()
    unit = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * ref.abs().amax(-1, keepdim=True)
    return float(((x - ref).abs() / unit).max())


# twice the largest error of the eager torch bf16 restatement (torch ops on the device, the same weights, the oracle's own layer inputs) against
# the oracle's w2 input over every row of the layer, per layer, in capture_error's units; the factor 2 covers the difference in summation order
# between torch's GEMM and the tile kernel.  Measured on one MI355X (the docstring below): restatement 0.549 / 0.769 / 0.338 / 0.416 at layers
# 0 .. 3 -> the bars (rounded down)
CAPTURE_BAR = (1.098, 1.537, 0.674, 0.832)


def test_every_captured_row_lies_within_the_capture_bar_of_the_oracles_w2_input():
    """Clip 0 alone, layer by layer with the layer's inputs made one: the oracle's stream at depth l patched over every row in front of layer l
    (stream_patch) and the oracle's wo input over every head (head_patch), so wo, the residual, ffn_norm, w1|w3 and the SwiGLU epilogue of ONE
    layer run on the oracle's very inputs; the neurons captured at layer l against the oracle's own w2 input, per element.  Layer L - 1 is the
    row-trimmed one: its 10 distinct consumed rows come from the weight-streaming path, the others are NaN and left out.  The bar is not chosen: it is twice
    the error of an eager torch bf16 restatement of the same half layer on the device (F.linear / rms norm / F.silu on the same weights and
    inputs - not the code under test) against the oracle's rows of that layer, in capture_error's units.  The restatement is not row-trimmed, so
    its error is taken over all 214 rows of every layer: the ten rows the trimmed layer captures are too few to estimate a largest error from
    (over those ten alone the restatement happens to read 0.000 and the kernel 0.001 - one bf16 step on one small element).  Measured on one
    MI355X, layers 0 .. 3: restatement 0.549 / 0.769 / 0.338 / 0.416, bars 1.098 / 1.537 / 0.674 / 0.832, the kernel 0.549 / 0.769 / 0.338 / 0.001
    (layers 0 .. 2: the tile kernel's largest error is the restatement's).  End to end (no patched inputs) the figures are printed only, 2.46 /
    2.93 / 3.45 / 2.01: there the layers in front have drifted."""
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    one, inputs, states, layers = oracle_clip0()
    every = one["attention_mask"].clone()
    every[:, -1] = False                                                                      # (the closing token is not run: the dead tail)
    n = int(every.sum())
    eps = cfg.llm_config.rms_norm_eps
    end_to_end = nwhole["neurons"][(nwhole["neurons_index"][:, 0] == 0)]
    figures = []
    for i, (wo_in, w2_in) in enumerate(layers):
        p = f"language_model.model.layers.{i}."
        x, ao = states[i][0, :n].cuda(), wo_in[:n].cuda()
        h = x + F.linear(ao, sd[p + "attention.wo.weight"].cuda())
        t = O.rms_norm_cast_then_scale(h, sd[p + "ffn_norm.weight"].cuda(), eps)
        eager = F.silu(F.linear(t, sd[p + "feed_forward.w1.weight"].cuda())) * F.linear(t, sd[p + "feed_forward.w3.weight"].cuda())
        out = model(**one, stream_patch=StreamPatch(every, states[i][0, :n, None].contiguous(), (i, i + 1)),
                    head_patch=HeadPatch(every, wo_in[:n].reshape(n, 1, HEADS, D).contiguous(), (i, i + 1)), return_neurons=every, neuron_layers=(i, i + 1))
        got = out["neurons"][:, 0].cpu()
        rows = torch.isfinite(got.float()).all(-1)
        assert int(rows.sum()) == (10 if i == LAYERS - 1 else n), (i, int(rows.sum()))
        e_hip, e_eager, e_eager_own = capture_error(got[rows], w2_in[:n][rows]), capture_error(eager.cpu(), w2_in[:n]), capture_error(eager.cpu()[rows], w2_in[:n][rows])
        e2e_rows = torch.isfinite(end_to_end[:, i].float().cpu()).all(-1)
        figures.append((i, e_hip, e_eager))
        print(f"layer {i}: {int(rows.sum())} rows; hip {e_hip:.3f}, eager restatement {e_eager:.3f} over the layer's {n} oracle rows ({e_eager_own:.3f} over the captured ones) -> bar {2 * e_eager:.3f}, pinned {CAPTURE_BAR[i]}; "
              f"end to end hip {capture_error(end_to_end[:, i].cpu()[e2e_rows], w2_in[:n][e2e_rows]):.3f}")
    for i, e_hip, e_eager in figures:
        assert e_hip <= CAPTURE_BAR[i], (i, e_hip, e_eager, CAPTURE_BAR[i])


# ---- (c) the identities --------------------------------------------------------------------------------------------------------------
def test_self_patch_changes_no_output_the_trimmed_layer_included():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    every = torch.ones_like(kw["attention_mask"])
    for mask, layers, ids in ((every, (0, LAYERS), None), (seg["frames"], (1, 3), COLS), (seg["score_row"], (3, 4), None), (every, (2, 4), COLS),
                              (seg["text_after"] | seg["motion"], (0, 1), torch.tensor([6, 7]))):
        cap = model(**kw, return_neurons=mask, neuron_layers=layers, neuron_ids=ids)
        for values, idx in ((cap["neurons"], cap["neurons_index"]), (cap["neurons"].cpu(), None)):    # on the device with the index, on the host without
            out = model(**kw, **READS, neuron_patch=NeuronPatch(mask, values, layers, idx, ids))
            assert_same_outputs(out, plain)
    # an empty window, an empty selection, no neuron: the plain pass
    z = lambda n, l, w=INTER: torch.zeros(n, l, w, dtype=BF)
    for patch in (NeuronPatch(every, z(428, 0), (2, 2)), NeuronPatch(torch.zeros_like(every), z(0, 2), (1, 3)),
                  NeuronPatch(every, z(428, 1, 0), (1, 2), None, torch.zeros(0, dtype=torch.long))):
        assert_same_outputs(model(**kw, **READS, neuron_patch=patch), plain)
    # a patch of the trimmed layer over rows it does not consume: no MLP runs for them, nothing moves
    frames_only = NeuronPatch(seg["frames"], torch.full((int((seg["frames"] & kw["attention_mask"].bool()).sum()), 1, INTER), 9.0, dtype=BF), (LAYERS - 1, LAYERS))
    assert_same_outputs(model(**kw, **READS, neuron_patch=frames_only), plain)


def test_factors_of_one_change_no_output_and_arm_nothing():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    armed = []
    keep = model._prefill
    model._prefill = lambda *a, **k: (armed.append(k.get("neuron_scale")), keep(*a, **k))[1]
    try:
        for rows in (None, seg["score_row"]):
            assert_same_outputs(model(**kw, **READS, neuron_scale=NeuronScale(torch.ones(LAYERS), None, rows)), plain)
            assert_same_outputs(model(**kw, **READS, neuron_scale=NeuronScale(torch.ones(2), torch.tensor([[1, 5], [3, 9]]), rows)), plain)
        out = model(**kw, **READS, neuron_scale=NeuronScale(layer_table([(1, 0.0)]), None, torch.zeros_like(seg["frames"])))      # no row: the plain pass
        assert_same_outputs(out, plain)
        assert armed == [None] * 5
        # one entry off 1: armed; the layers whose factor is 1 launch nothing, so the stream in front of layer 2 keeps its bits
        out = model(**kw, **READS, neuron_scale=NeuronScale(layer_table([(2, 0.5)])))
        assert armed[-1] is not None and same(out["lens_score_hidden"][:, :3], plain["lens_score_hidden"][:, :3])
        assert not same(out["lens_score_hidden"][:, 3], plain["lens_score_hidden"][:, 3])
        # the trimmed layer scaled at rows it does not consume: armed, and nothing moves
        assert_same_outputs(model(**kw, **READS, neuron_scale=NeuronScale(layer_table([(LAYERS - 1, 0.0)]), None, seg["frames"])), plain)
        assert armed[-1] is not None
    finally:
        del model._prefill


@pytest.mark.parametrize("s", [0.0, -1.0, 1.7])
def test_scale_is_capture_torch_patch(s):
    """For layer l: pass A captures layer l; torch computes (x.float() * s).bfloat16(); pass B patches it; pass C runs neuron_scale.  B and C agree
    on every output, bit for bit - dense and sparse, over every row and over the rows of a mask, the trimmed layer included."""
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    every = torch.ones_like(kw["attention_mask"])
    sparse = torch.tensor([5, 6, 7, 300])
    for l, ids, mask in ((1, None, every), (0, sparse, seg["text_after"]), (LAYERS - 1, None, seg["score_row"]), (LAYERS - 1, sparse, every), (2, sparse, every)):
        a = model(**kw, return_neurons=mask, neuron_layers=(l, l + 1), neuron_ids=ids)
        values = (a["neurons"].float() * s).to(BF)
        b = model(**kw, **READS, return_neurons=every, neuron_patch=NeuronPatch(mask, values, (l, l + 1), a["neurons_index"], ids))
        scale = (NeuronScale(layer_table([(l, s)]), None, None if mask is every else mask) if ids is None else
                 NeuronScale(torch.full((ids.numel(),), s), torch.stack([torch.full_like(ids, l), ids], 1), None if mask is every else mask))
        c = model(**kw, **READS, return_neurons=every, neuron_scale=scale)
        assert_same_outputs(c, b)
        assert same(c["neurons"][:, :l], nwhole["neurons"][:, :l]) and not same(c["neurons"][:, l], nwhole["neurons"][:, l]), (l, ids)


def test_sparse_patch_read_back_by_a_capture_and_the_order_scale_patch_capture():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    g = torch.Generator().manual_seed(13)
    mask = seg["text_after"]
    own, _ = neurons_of(nwhole, mask)
    n = own.shape[0]
    ids = torch.tensor([6, 7, 300])
    values = torch.randn(n, 2, 3, generator=g).to(BF)
    values[0, 0, 1] = float("nan")
    out = model(**kw, **READS, return_neurons=mask, neuron_layers=(1, 3), neuron_patch=NeuronPatch(mask, values, (1, 3), None, ids))
    got = out["neurons"]
    rest = torch.ones(INTER, dtype=torch.bool); rest[ids] = False
    assert same(got[:, :, ids.cuda()].contiguous(), values.cuda())                            # the selected neurons carry the values, at both layers
    assert same(got[:, 0][:, rest.cuda()].contiguous(), own[:, 1][:, rest.cuda()].contiguous())      # the others the plain pass's bits at layer lo (5 and 8 beside 6, 7)
    assert not same(got[:, 1][:, rest.cuda()].contiguous(), own[:, 2][:, rest.cuda()].contiguous())  # (behind lo they are those of the patched pass)
    assert got[0, 0, 7].isnan() and not same(out["score1"], plain["score1"])
    # scale, patch, capture armed on one neuron: the capture returns what w2 consumes - the patch over the scaled value; its neighbours the scaled ones
    three = torch.full((n, 1, 1), 3.0, dtype=BF)
    both = model(**kw, return_neurons=mask, neuron_layers=(1, 2), neuron_ids=torch.tensor([5, 6, 7]),
                 neuron_scale=NeuronScale(torch.tensor([0.0, -1.0]), torch.tensor([[1, 6], [1, 7]]), mask), neuron_patch=NeuronPatch(mask, three, (1, 2), None, torch.tensor([6])))
    assert same(both["neurons"][:, 0, 0], own[:, 1, 5]) and same(both["neurons"][:, 0, 1], three[:, 0, 0].cuda())
    assert same(both["neurons"][:, 0, 2], (-own[:, 1, 7].float()).to(BF))
    # ... and with the patch off: the scale's zero shows
    only = model(**kw, return_neurons=mask, neuron_layers=(1, 2), neuron_ids=torch.tensor([6]), neuron_scale=NeuronScale(torch.tensor([0.0]), torch.tensor([[1, 6]]), mask))
    assert not only["neurons"].any()


# ---- (d) against the composed oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(KNOCKOUTS)), ids=["-".join(str(v) for v in c) for c in KNOCKOUTS])
def test_knocked_out_pass_against_the_composed_oracle(case):
    """Clip 0 alone; the cases of tests/test_neuron_patch_cpu.py, each of which moves the oracle's own score by at least 2 bf16 ulps - twice the
    bar here.  score1 within the tiny rig's bar (1e-3 or 1 bf16 ulp of the oracle's value, tests/test_gpu_head_patch.py) for all of them; for
    TOKEN_CASES - the oracle itself decides at most one answer row of ten within 2 bf16 ulps there - the answer tokens identical up to at most
    1 such row."""
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    one, inputs, own, _ = oracle_clip0()
    options = knockout_options(KNOCKOUTS[case], oracle_score_row_capture())
    states, _ = NP.composed_states(sd, cfg, **inputs, **options)
    ref = NP.lens(sd, cfg, states, one["attention_mask"], one["labels"], 2)
    out = model(**one, neuron_scale=neuron_scale_of(options))
    print(f"{KNOCKOUTS[case]}: plain {plain['score1'][0].item():.5f}")
    score_ok(out["score1"], ref["score"][:, LAYERS])
    assert not same(out["score1"], plain["score1"][0:1])                                       # the knocked score differs from the plain one
    if case in TOKEN_CASES:
        w, eps = sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps
        logits = O.lm_logits(sd, O.rms_norm_cast_then_scale(states[LAYERS], w, eps))[0, :-1]
        want = one["labels"][0, 1:] != -100
        assert int(want.sum()) == 10 and assert_levels(out["logit"].cpu()[want], logits[want].argmax(-1), logits[want]) <= 1


# ---- (e) combinations ----------------------------------------------------------------------------------------------------------------
def test_with_a_key_drop_window_the_lens_in_front_of_both_windows_keeps_the_plain_bits():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    knock = dict(key_drop=seg["frames"], key_drop_rows=seg["text_after"], key_drop_layers=(2, 4))
    out = model(**kw, **READS, **knock, neuron_scale=NeuronScale(layer_table([(2, 0.0), (3, 0.0)]), None, only_clip(torch.ones_like(kw["attention_mask"]), 1)))
    knocked = model(**kw, **READS, **knock)
    for key in LENS_HIDDEN + ("lens_score",):
        assert same(out[key][:, :3], plain[key][:, :3]), key                                  # layers 0 and 1 ran as they always do; depth 2 feeds the first armed layer
        assert same(out[key][0], knocked[key][0]), key                                        # clip 0 carries the key-drop only
    assert not same(out["lens_score_hidden"][1, 3:], knocked["lens_score_hidden"][1, 3:])
    assert same(out["lens_score"][:, LAYERS].to(BF), out["score1"])


def test_a_stream_capture_and_a_head_capture_behind_the_layer_see_the_modified_pass():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    every = torch.ones_like(kw["attention_mask"])
    l = 1
    base = model(**kw, return_heads=every, head_layers=(l, l + 2))
    out = model(**kw, return_stream=every, stream_depths=(l, l + 2), return_heads=every, head_layers=(l, l + 2),
                neuron_scale=NeuronScale(layer_table([(l, 0.0)]), None, only_clip(every, 1)))
    clip = whole["stream_index"][:, 0]
    assert same(out["stream"][:, 0], whole["stream"][:, l])                                   # depth l: what layer l consumes, in front of its MLP
    assert same(out["stream"][clip == 0, 1], whole["stream"][clip == 0, l + 1])               # clip 0: not touched
    rows1 = (out["stream"][clip == 1, 1].view(torch.int16) != whole["stream"][clip == 1, l + 1].view(torch.int16)).any(-1)
    assert rows1.all()                                                                        # clip 1: every row of it
    assert same(out["heads"][:, 0], base["heads"][:, 0])                                      # layer l's heads: in front of its MLP
    assert same(out["heads"][clip == 0, 1], base["heads"][clip == 0, 1]) and not same(out["heads"][clip == 1, 1], base["heads"][clip == 1, 1])


ROW_KEYS = ("stream", "stream_index", "heads", "heads_index") + NEURON_KEYS
ALL_EIGHT = ("stream_patch", "stream_capture", "head_scale", "head_patch", "head_capture", "neuron_scale", "neuron_patch", "neuron_capture")


@functools.lru_cache(maxsize=None)
def oracle_score_with_layer_2_mlp_negated():
    """KNOCKOUTS[3] - layer 2's MLP x -1, exactly representable, 6 bf16 ulps off the oracle's plain score (tests/test_neuron_patch_cpu.py) - on clip 0
    alone: (the product's option, the composed oracle's score [1])."""
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    one, inputs, own, _ = oracle_clip0()
    options = knockout_options(KNOCKOUTS[3], oracle_score_row_capture())
    states, _ = NP.composed_states(sd, cfg, **inputs, **options)
    return neuron_scale_of(options), NP.lens(sd, cfg, states, one["attention_mask"], one["labels"], 2)["score"][:, LAYERS]


@pytest.mark.parametrize("form", ["trimmed", "mixed", "full_logits"])
def test_all_eight_row_options_armed_in_one_pass(form):
    """Stream, head and neuron patch, capture and scale - and the lens - in ONE pass, over the three forms of the last layer: trimmed (11 consumed rows
    per clip), mixed (clip 1 with 12 more answer rows: 23 > 16, its rows finish on the tile kernels, clip 0's on the streaming path), every row
    (full_logits).  Five rows per clip: the first token, a token of each frame, the score row, the last answer row.  Pass one captures them over the
    full windows.  Pass two patches every capture back in - three self-patches - beside the three captures and both scales, all factors 1: every
    output is the plain pass's and every capture pass one's, bit for bit.  forward() arms no scale whose factors are all 1, so the unit tables are
    handed to _prefill itself: the pass then runs with all eight armed, which _prefill's arguments show.  Pass three: one factor off 1 - layer 2's MLP
    x -1 (no inverse anywhere) - with the patches cut to the windows in front of it (behind it they would put the plain pass back); clip 0's score
    against the composed oracle's under score_ok's bar, the captures in front of the factor pass one's bits, the neurons of layer 2 their negation."""
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    kw, extra = dict(kw), {}
    if form == "mixed":
        free = (seg["text_after"][1] & (kw["labels"][1] == -100)).nonzero().flatten()[1:13]      # (a label at p makes p - 1 a consumed row)
        kw["labels"] = kw["labels"].clone()
        kw["labels"][1, free] = kw["input_ids"][1, free]
        plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 4)
        per_clip = [sum(plan["cu"][b] <= int(r) < plan["cu"][b + 1] for r in list(plan["score_rows"]) + list(plan["logit_rows"])) for b in range(2)]
        assert per_clip == [11, 23], per_clip
    if form == "full_logits":
        extra["full_logits"] = True
    base = plain if form == "trimmed" else model(**kw, **READS, **extra)
    mask = seg["score_row"].clone()
    mask[:, [0, 70, 130, 213]] = True
    every = dict(return_stream=mask, return_heads=mask, return_neurons=mask)
    first = model(**kw, **READS, **every, **extra)
    assert first["stream_index"].tolist() == [[b, p] for b in range(2) for p in (0, 70, 130, 211, 213)]
    assert_same_outputs(first, base, skip=ROW_KEYS)

    def patches(d_stream, d_head, d_neuron):      # pass one's captures cut to the windows [0, d)
        cut = lambda key, d: first[key][:, :d].contiguous()
        return dict(stream_patch=StreamPatch(mask, cut("stream", d_stream), (0, d_stream), first["stream_index"]),
                    head_patch=HeadPatch(mask, cut("heads", d_head), (0, d_head), first["heads_index"]),
                    neuron_patch=NeuronPatch(mask, cut("neurons", d_neuron), (0, d_neuron), first["neurons_index"]))

    seen = []
    keep = model._prefill

    def prefill_with_unit_scales(*a, **k):
        if k.get("head_scale") is None:
            k["head_scale"] = (None, torch.ones(LAYERS, HEADS))
        if k.get("neuron_scale") is None:
            k["neuron_scale"] = (None, torch.ones(LAYERS), None, None, None)
        seen.append([name for name in ALL_EIGHT if k.get(name) is not None] + (["lens"] if k.get("lens") is not None else []))
        return keep(*a, **k)

    model._prefill = prefill_with_unit_scales
    try:
        second = model(**kw, **READS, **every, **patches(LAYERS, LAYERS, LAYERS), **extra)
        scale, want = oracle_score_with_layer_2_mlp_negated()
        third = model(**kw, **READS, **every, **patches(3, 3, 2), neuron_scale=scale, **extra)
    finally:
        del model._prefill
    assert seen == [list(ALL_EIGHT) + ["lens"]] * 2, seen
    assert_same_outputs(second, base, skip=ROW_KEYS)
    for key in ROW_KEYS:
        assert same(second[key], first[key]), key
    score_ok(third["score1"][0:1], want)
    assert not same(third["score1"], base["score1"])
    assert same(third["stream"][:, :3], first["stream"][:, :3]) and same(third["heads"][:, :3], first["heads"][:, :3]) and same(third["neurons"][:, :2], first["neurons"][:, :2])
    assert same(third["neurons"][:, 2], (-first["neurons"][:, 2].float()).to(BF)) and not same(third["stream"][:, 3], first["stream"][:, 3])
    assert_same_outputs(model(**kw, **READS, **extra), base)                                  # every option disarmed with its pass


def test_fp8_mode_self_patch_is_bit_neutral():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    model.set_precision("fp8")
    try:
        plain8 = model(**kw, **READS)
        mask = seg["frames"] | seg["score_row"]
        for ids in (None, COLS):
            cap = model(**kw, return_neurons=mask, neuron_layers=(1, 4), neuron_ids=ids)
            out = model(**kw, **READS, neuron_patch=NeuronPatch(mask, cap["neurons"], (1, 4), cap["neurons_index"], ids))
            assert_same_outputs(out, plain8)
        assert not same(plain8["lens_score_hidden"], plain["lens_score_hidden"])              # another arithmetic from layer 0 on
        assert not same(model(**kw, neuron_scale=NeuronScale(layer_table([(1, 0.0)])))["score1"], plain8["score1"])
    finally:
        model.set_precision("bf16")
    assert_same_outputs(model(**kw, **READS), plain)


def test_graph_replay_runs_armed_calls_eagerly():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    own, idx = neurons_of(nwhole, only_clip(seg["score_row"], 0))
    armed_kw = dict(return_neurons=seg["text_after"], neuron_layers=(1, 3), neuron_ids=COLS, neuron_scale=NeuronScale(layer_table([(0, 0.0)])),
                    neuron_patch=NeuronPatch(only_clip(seg["score_row"], 1), own[:, 2:3].contiguous(), (2, 3)))
    eager = model(**kw, **READS, **armed_kw)
    assert not same(eager["score1"], plain["score1"])
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    model.enable_graph_replay(True)
    try:
        graphs = lambda: sum(isinstance(v, tuple) for v in model._graphs.values())
        outs = [model(**dev_kw, **READS) for _ in range(3)]                                   # eager, capture, replay
        assert graphs() == 1 and len(model._graphs) == 1
        armed = [model(**dev_kw, **READS, **armed_kw) for _ in range(2)]
        only_capture = model(**dev_kw, **READS, return_neurons=seg["text_after"], neuron_layers=(1, 3))
        only_scale = model(**dev_kw, **READS, neuron_scale=armed_kw["neuron_scale"])
        assert graphs() == 1 and len(model._graphs) == 1                                       # nothing captured, nothing even remembered
        again = model(**dev_kw, **READS)                                                      # replays; the armed passes before it disarmed
        assert graphs() == 1 and len(model._graphs) == 1
        torch.cuda.synchronize()
        for o in outs + [again]:
            assert_same_outputs(o, plain)
        for o in armed:
            assert_same_outputs(o, eager)
        assert_same_outputs(only_capture, plain, skip=NEURON_KEYS)
        assert same(only_capture["neurons"], neurons_of(nwhole, seg["text_after"])[0][:, 1:3].contiguous()) and not same(only_scale["score1"], plain["score1"])
    finally:
        model.enable_graph_replay(False)
    assert_same_outputs(model(**kw, **READS), plain)


# ---- (f) the sweeps -------------------------------------------------------------------------------------------------------------------
def test_mlp_knockout_and_neuron_knockout_on_the_rig():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    calls = []
    keep = model.vit_tokens
    model.vit_tokens = lambda pv: (calls.append(int(pv.shape[0])), keep(pv))[1]
    try:
        res = eval_utils.mlp_knockout(model, **kw, candidate_ids=CAND)
        assert calls == [4]                                                                   # InternViT ran once
        rows = only_clip(seg["score_row"], 1)
        part = eval_utils.mlp_knockout(model, **kw, layers=[3, 1], rows=rows)
        pairs = torch.tensor([[2, 251], [0, 5], [3, 700]])
        single = eval_utils.neuron_knockout(model, pairs, **kw)
        assert calls == [4, 4, 4]
    finally:
        del model.vit_tokens
    assert res["layers"] == [0, 1, 2, 3] and len(res["outs"]) == 1 + LAYERS
    assert same(res["score1"], plain["score1"].float()) and same(res["outs"][0]["cand_logprob"], plain["cand_logprob"])       # outs[0] is the plain pass
    assert tuple(res["knocked"].shape) == (2, LAYERS) and torch.isfinite(res["knocked"]).all() and same(res["delta"], res["score1"][:, None] - res["knocked"])
    assert (res["delta"] != 0).any()
    by_hand = model(**kw, neuron_scale=NeuronScale(layer_table([(2, 0.0)])))                   # one cell recomputed by hand
    assert same(res["knocked"][:, 2], by_hand["score1"].float())
    # rows: the knock-out restricted to clip 1's score row - NaN for the clip the mask selects no row of; the trimmed layer consumes that row
    assert part["layers"] == [3, 1] and tuple(part["knocked"].shape) == (2, 2) and part["knocked"][0].isnan().all() and torch.isfinite(part["knocked"][1]).all()
    by_hand = model(**kw, neuron_scale=NeuronScale(layer_table([(3, 0.0)]), None, rows))
    assert same(part["knocked"][1, 0], by_hand["score1"].float()[1]) and same(by_hand["score1"][:1], plain["score1"][:1])
    assert not same(by_hand["score1"][1:], plain["score1"][1:])                               # the last layer's MLP of the score row: knocked out on the streaming path
    # single neurons
    assert torch.equal(single["neurons"], pairs) and len(single["outs"]) == 4 and tuple(single["knocked"].shape) == (2, 3)
    assert same(single["delta"], single["score1"][:, None] - single["knocked"]) and torch.isfinite(single["knocked"]).all()
    by_hand = model(**kw, neuron_scale=NeuronScale(torch.zeros(1), torch.tensor([[2, 251]])))
    assert same(single["knocked"][:, 0], by_hand["score1"].float())


def test_neuron_trace_on_the_rig():
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    swap = torch.tensor([1, 0])
    frames = torch.tensor([2, 3, 0, 1])
    corrupt = dict(kw, input_ids=kw["input_ids"][swap], labels=kw["labels"][swap], pixel_values=kw["pixel_values"][frames], motion_feature=kw["motion_feature"][swap])
    calls = []
    keep = model.vit_tokens
    model.vit_tokens = lambda pv: (calls.append(int(pv.shape[0])), keep(pv))[1]
    try:
        res = eval_utils.neuron_trace(model, clean=kw, corrupt=corrupt, layers=(2, 4), top=3, candidate_ids=CAND)
        assert calls == [4, 4]                                                                # InternViT ran as often as in two passes
    finally:
        del model.vit_tokens
    assert res["layers"] == (2, 4) and tuple(res["neurons"].shape) == (2, 3) and len(res["outs"]) == 2 + 2 * 3
    assert same(res["clean_score"], plain["score1"].float()) and same(res["corrupt_score"], plain["score1"].float()[swap.cuda()])
    assert tuple(res["score"].shape) == (2, 2, 3) and tuple(res["restored"].shape) == (2, 2, 3)
    assert same(res["restored"], eval_utils.restored_fraction(res["score"], res["clean_score"], res["corrupt_score"])) and torch.isfinite(res["restored"]).all()
    # rows default to the score row; the ranking is rank_neurons of the two captures; the donor is the plain capture
    donor, base = res["outs"][0], res["outs"][1]
    assert donor["neurons_index"].tolist() == [[0, 211], [1, 211]] and same(donor["neurons"], neurons_of(nwhole, seg["score_row"])[0][:, 2:4].contiguous())
    assert torch.equal(res["neurons"], eval_utils.rank_neurons(donor["neurons"], base["neurons"], 3))
    # one cell by hand: the clean neuron patched into the corrupt batch at the score rows
    w, r = 1, 0
    j = int(res["neurons"][w, r])
    by_hand = model(**corrupt, neuron_patch=NeuronPatch(seg["score_row"], donor["neurons"][:, w:w + 1, j:j + 1].contiguous(), (3, 4), donor["neurons_index"], torch.tensor([j])))
    assert same(res["score"][:, w, r], by_hand["score1"].float())
    # a batch traced against itself: nothing to restore - NaN - and the self-patch kept the score
    own = eval_utils.neuron_trace(model, clean=kw, corrupt=dict(kw), layers=(0, 1), top=2)
    assert own["restored"].isnan().all() and same(own["score"][:, 0, 0], plain["score1"].float()) and own["neurons"].tolist() == [[0, 1]]


# ---- (g) refusals through the C ABI --------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message_and_no_fault(lib):
    model, cfg, sd, kw, seg, plain, whole, nwhole, consumed = neurons_rig()
    ctx = model._ctx
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 4)
    T = plan["cu"][-1]
    buf = torch.zeros(4, 1, INTER, dtype=BF, device="cuda")
    fl = lambda v: (native.C.c_float * len(v))(*v)
    half = fl([0.5] * LAYERS)
    err = lambda: lib.aigv_last_error(ctx).decode()

    def plain_again():
        torch.cuda.synchronize()
        assert_same_outputs(model(**kw, **READS), plain)

    arms = {"capture": lambda rows, n, lo, hi, b, cols=None, m=0: lib.aigv_neuron_capture_arm(ctx, rows, n, lo, hi, cols, m, b),
            "patch": lambda rows, n, lo, hi, b, cols=None, m=0: lib.aigv_neuron_patch_arm(ctx, rows, n, lo, hi, cols, m, b),
            "scale": lambda rows, n, lo, hi, b, cols=None, m=0: lib.aigv_neuron_scale_arm(ctx, rows, n, half, None, None, None, 0)}
    # refused by the arm calls: nothing armed
    for what in ("capture", "patch"):
        for args, word in (((i32([0, 1]), -1, 0, 1, buf.data_ptr()), "-1 rows outside 0..max_tokens"), ((None, 2, 0, 1, buf.data_ptr()), "null row list"),
                           ((i32([0, 1]), 2, 0, 1, None), "null or not 16-byte aligned"), ((i32([0, 1]), 2, 0, 1, buf.data_ptr() + 8), "null or not 16-byte aligned"),
                           ((i32([0, 1]), 2, 0, 1, buf.data_ptr(), i32([0, INTER]), 2), f"column {INTER} \\(entry 1\\) outside 0..{INTER - 1}"),
                           ((i32([0, 1]), 2, 0, 1, buf.data_ptr(), i32([-1, 4]), 2), "column -1 \\(entry 0\\) outside"),
                           ((i32([0, 1]), 2, 0, 1, buf.data_ptr(), i32([4, 4]), 2), "columns not strictly ascending at entry 1"),
                           ((i32([0, 1]), 2, 0, 1, buf.data_ptr(), i32([9, 4]), 2), "columns not strictly ascending at entry 1"),
                           ((i32([0, 1]), 2, 0, 1, buf.data_ptr(), i32(list(range(4097))), 4097), "4097 columns outside 0..4096")):
            assert arms[what](*args) == -1 and re.search(word, err()) and err().startswith(f"aigv_neuron_{what}_arm:"), (what, args, err())
    scale = lambda rows=None, n=0, table=half, ls=None, cs=None, fs=None, m=0: lib.aigv_neuron_scale_arm(ctx, rows, n, table, ls, cs, fs, m)
    assert scale(table=fl([1.0, float("nan"), 1.0, 1.0])) == -1 and "layer_scale[1] is NaN" in err()
    assert scale(table=None) == -1 and "neither a per-layer table nor a selection" in err()
    assert scale(rows=i32([0, 1]), n=-1) == -1 and "-1 rows outside 0..max_tokens" in err()
    assert scale(table=None, ls=i32([1]), cs=i32([5]), fs=fl([float("nan")]), m=1) == -1 and "factor 0 is NaN" in err()
    assert scale(table=None, ls=i32([LAYERS]), cs=i32([5]), fs=fl([0.0]), m=1) == -1 and f"layer {LAYERS} (entry 0) outside" in err()
    assert scale(table=None, ls=i32([1]), cs=i32([INTER]), fs=fl([0.0]), m=1) == -1 and f"column {INTER} (entry 0) outside" in err()
    assert scale(table=None, ls=i32([1, 1]), cs=i32([5, 5]), fs=fl([0.0, 0.0]), m=2) == -1 and "not strictly ascending in (layer, column) at entry 1" in err()
    assert scale(table=None, ls=i32([2, 1]), cs=i32([5, 6]), fs=fl([0.0, 0.0]), m=2) == -1 and "not strictly ascending in (layer, column) at entry 1" in err()
    assert scale(table=None, ls=i32([1]), cs=None, fs=fl([0.0]), m=1) == -1 and "null selection list" in err()
    assert scale(table=None, ls=i32([0] * 4097), cs=i32(list(range(4097))), fs=fl([0.0] * 4097), m=4097) == -1 and "4097 selected neurons outside 0..4096" in err()
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
            with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: the neuron {what} .*" + word):
                prefill()
            plain_again()
        assert arms[what](i32([0, 5, 9]), 3, 0, 1, buf.data_ptr()) == 0
        with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: keep_kv while a neuron {what} is armed"):
            prefill(keep_kv=True, kv_cap=256)
        plain_again()
        # an option that reaches layer L - 1 in a pass without output rows: its last MLP does not run
        assert arms[what](i32([0, 5, 9]), 3, LAYERS - 1, LAYERS, buf.data_ptr()) == 0
        with pytest.raises(native.NativeError, match=f"aigv_llm_prefill: a neuron option reaches layer {LAYERS - 1} and the pass has no output rows"):
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
            with pytest.raises(native.NativeError, match=f"aigv_llm_extend: a neuron {what} is armed"):
                model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common)
        finally:
            del model._prefill
        plain_again()                                                                         # the refused continuation disarmed too
    with pytest.raises(TypeError):
        model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_neurons=seg["frames"])
