"""Activation patching without a GPU: the ABI entries, the refusals that come before any launch (native, with fake aligned addresses; host, as
ValueError from a model that lives on the host), the signatures and graph keys that stay as they were, eval_utils.restored_fraction on hand-made
inputs, and the reference of tests/test_gpu_stream_patch.py pinned to the existing oracle - an empty patch and a self-patch are
depth_lens_reference.composed_states bit for bit, a transplant of every row turns the recipient into the donor from that depth on - with the
oracle condition: on the rig, patching the score row moves the oracle's own score by at least twice the GPU file's bar."""
import ctypes
import functools
import inspect
import os
import re

import pytest
import torch

import depth_lens_reference as DL
import stream_patch_reference as SP
from test_key_drop_cpu import bf16_ulps, two_clips
from test_key_drop_rows_cpu import one_clip

import aigv_assessor_amd as pkg
from aigv_assessor_amd import dist_utils, eval_utils, native, readouts, synth
from aigv_assessor_amd.readouts import StreamPatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = 4
FRAMES = (2, 2)
BF = torch.bfloat16


# ---- the ABI entries ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_entries():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I, I32P = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)
    want = {"aigv_stream_capture_arm": (I, [P, I32P, I, I, I, P]),
            "aigv_stream_patch_arm": (I, [P, I32P, I, I, I, P]),
            "aigv_op_stream_rows": (I, [P, I, I, I32P, I, P, P, I, I, I, I, P])}
    for name, proto in want.items():
        assert name in note and re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == proto, name
    kernels = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert "aigv_launch_stream_rows(" in kernels
    rowops = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "rowops.hip")).read()
    assert "template <bool TO_STREAM>" in rowops and "stream_rows_kernel" in rowops                      # the direction is a template parameter


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_native_refusals_without_a_gpu():
    """Every check of the op comes before any HIP call: AIGV_ERR_ARG and a message that starts with the op's name (fake, aligned, non-null device
    addresses: nothing is dereferenced; the row list is a real host array, it is read).  The context entry points refuse a null handle."""
    lib = native.load()
    P = 0x10000
    last = lambda: (lib.aigv_last_error(None) or b"").decode()
    good = [0, 3, 9, 99]

    def op(stream=P, ld=128, T=100, rows=good, n=None, idx=P, side=P, n_depths=3, depth=1, H=128, to_stream=0):
        arr = native.i32_array(rows) if rows is not None else None
        return lib.aigv_op_stream_rows(stream, ld, T, arr, len(rows or []) if n is None else n, idx, side, n_depths, depth, H, to_stream, None), last()

    cases = ((dict(stream=None), "null operand"), (dict(side=None), "null operand"), (dict(rows=None, n=4), "null operand"), (dict(idx=None), "null operand"),
             (dict(n=-1), "must not be negative"), (dict(H=100), "multiple of 8"), (dict(ld=120), "leading dimension"), (dict(ld=132), "leading dimension"),
             (dict(stream=P + 8), "16-byte aligned"), (dict(side=P + 8), "16-byte aligned"), (dict(H=16392, ld=16392), "above 16384"),
             (dict(T=-1), "must not be negative"),
             (dict(rows=[0, 3, 100]), "row 2 (packed row 100) outside [0, 100)"), (dict(rows=[-1, 3]), "row 0 (packed row -1) outside [0, 100)"),       # range
             (dict(rows=[0, 9, 3]), "not strictly ascending"), (dict(rows=[0, 3, 3]), "not strictly ascending"),                                         # ordering
             (dict(depth=3), "depth 3 outside the window of 3 depths"), (dict(depth=-1), "outside the window"), (dict(n_depths=0, depth=0), "outside the window"))
    for to_stream in (0, 1):
        for kw, word in cases:
            rc, msg = op(to_stream=to_stream, **kw)
            assert rc == -1 and word in msg and msg.startswith("aigv_op_stream_rows:"), (kw, rc, msg)
    rows = native.i32_array(good)
    assert lib.aigv_stream_capture_arm(None, rows, 4, 0, 1, P) == -1 and last().startswith("aigv_stream_capture_arm: null context")
    assert lib.aigv_stream_patch_arm(None, rows, 4, 0, 1, P) == -1 and last().startswith("aigv_stream_patch_arm: null context")


@functools.lru_cache(maxsize=None)
def host_rig():
    """The tiny stage-2 rig with four LLM layers on the host, tokens seed 302, two clips of two frames each: both of 215 tokens."""
    from aigv_assessor_amd.modeling import InternVLChatModel
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=LAYERS)
    model = InternVLChatModel(cfg, stage=2)
    kw, ctx_id = two_clips(cfg, 302, frames=FRAMES)
    model.img_context_token_id = ctx_id
    return model, cfg, kw


def test_host_refusals_come_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError.  Every message names its option."""
    model, cfg, kw = host_rig()
    ids, am = kw["input_ids"], kw["attention_mask"]
    H = cfg.llm_config.hidden_size
    seg = model.segment_masks(ids, am, kw["image_flags"])
    mask = seg["score_row"]                                                                   # two tokens, one per clip
    vals = lambda n=2, d=1, h=H, dt=BF: torch.zeros(n, d, h, dtype=dt)

    def bad(word, **opts):
        with pytest.raises(ValueError, match=word):
            model(**kw, **opts)

    # shape
    bad("return_stream: shape", return_stream=mask[:, :100])
    bad("return_stream: expected a bool or integer tensor", return_stream=mask.float())
    bad("return_stream: expected a bool or integer tensor", return_stream=mask[0])
    bad("stream_patch: rows: shape", stream_patch=StreamPatch(mask[:, :100], vals(), (0, 1)))
    bad("stream_patch: expected a readouts.StreamPatch", stream_patch=(mask, vals(), (0, 1)))
    bad("stream_patch: values must be a bf16 tensor", stream_patch=StreamPatch(mask, vals(dt=torch.float32), (0, 1)))
    bad("stream_patch: values must be a bf16 tensor", stream_patch=StreamPatch(mask, vals(d=2), (0, 1)))
    bad("stream_patch: values must be a bf16 tensor", stream_patch=StreamPatch(mask, vals()[0], (0, 1)))
    bad(f"stream_patch: values of width {H - 8}, the residual stream has H = {H}", stream_patch=StreamPatch(mask, vals(h=H - 8), (0, 1)))
    bad("stream_patch: index must be an integer tensor", stream_patch=StreamPatch(mask, vals(), (0, 1), torch.zeros(2, 3, dtype=torch.long)))
    # count mismatch: both counts are named
    bad("stream_patch: values hold 3 rows, the mask selects 2 tokens", stream_patch=StreamPatch(mask, vals(n=3), (0, 1)))
    dead = torch.zeros_like(mask); dead[:, 214] = True                                        # the closing token: behind the last consumed row, not run
    bad("stream_patch: values hold 2 rows, the mask selects 0 tokens", stream_patch=StreamPatch(dead, vals(), (0, 1)))
    own = torch.tensor([[0, 211], [1, 211]])
    assert torch.equal(mask.nonzero(), own)
    bad("stream_patch: index holds 1 pairs, the mask selects 2 tokens", stream_patch=StreamPatch(mask, vals(), (0, 1), own[:1]))
    # index mismatch: the first differing pair
    bad(r"stream_patch: pair 1 of index is \(clip, position\) = \(1, 210\), the pass's is \(1, 211\)",
        stream_patch=StreamPatch(mask, vals(), (0, 1), torch.tensor([[0, 211], [1, 210]])))
    # a bad window
    for window in ((2, 1), (-1, 2), (0, LAYERS + 1), (0,), (0, 1, 2), 2, (0.0, 2), (False, True)):
        bad("stream_depths", return_stream=mask, stream_depths=window)
        bad("stream_patch: depths", stream_patch=StreamPatch(mask, vals(), window))
    # stream_depths without return_stream
    bad("stream_depths: qualifies return_stream", stream_depths=(0, 2))
    # what passes the host checks: the record carries the options, and forward_kwargs hands them on
    ro = readouts.ReadOuts.parse(cfg.llm_config.vocab_size, kw["labels"], ids_shape=ids.shape, n_layers=LAYERS, return_stream=mask.long(),
                                 stream_patch=StreamPatch(mask, vals(d=2), [1, 3], own))
    assert torch.equal(ro.stream_rows, mask) and ro.stream_depths == (0, LAYERS) and ro.stream_patch.depths == (1, 3) and ro.touches_stream
    fk = readouts.forward_kwargs(ro)
    assert torch.equal(fk["return_stream"], mask) and fk["stream_depths"] == (0, LAYERS) and fk["stream_patch"] is ro.stream_patch
    assert not {"return_stream", "stream_depths", "stream_patch"} & set(readouts.forward_kwargs(readouts.ReadOuts(logprobs=True)))
    # the mask-to-rows mapping goes through the plan: padding and the dead tail are skipped, clip-major and position-ascending
    plan = model._plan(ids, am, kw["labels"], kw["image_flags"], 4)
    every = torch.ones_like(mask)
    rows, index = model._stream_rows(plan, every)
    assert rows.dtype == torch.int32 and rows.tolist() == list(range(plan["cu"][-1])) and index.shape == (len(rows), 2) and index[0].tolist() == [0, 0] and index[-1].tolist() == [1, 213]
    assert model._stream_rows(plan, dead)[0].tolist() == [] and model._stream_rows(plan, mask)[0].tolist() == [int(r) for r in plan["score_rows"]]
    got = model._stream_patch_plan(plan, ro.stream_patch)
    assert got[0].tolist() == [int(r) for r in plan["score_rows"]] and got[1:3] == (1, 3) and got[3] is ro.stream_patch.values
    assert model._stream_patch_plan(plan, StreamPatch(mask, vals(d=0), (2, 2))) is None       # an empty window: the plain pass
    assert model._stream_patch_plan(plan, StreamPatch(dead, vals(n=0), (0, 1))) is None       # an empty selection likewise


def test_the_other_entry_points_keep_their_signatures():
    model = host_rig()[0]
    for fn in (model.forward_shared_prefix, model.generate, model.generate_stage2, eval_utils.batched, dist_utils.score_clips_dp):
        assert not {"return_stream", "stream_depths", "stream_patch"} & set(inspect.signature(fn).parameters), fn
    assert {"return_stream", "stream_depths", "stream_patch"} <= set(inspect.signature(model.forward).parameters)
    sig = inspect.signature(eval_utils.causal_trace).parameters
    assert [sig[k].default for k in ("groups", "width", "stride")] == [None, 1, 1] and {"clean", "corrupt"} <= set(sig)


def test_causal_trace_refuses_two_layouts():
    model, cfg, kw = host_rig()
    clean = dict(kw)
    for change, word in ((dict(input_ids=kw["input_ids"][:, :200]), "one token layout"),
                         (dict(attention_mask=kw["attention_mask"] & (torch.arange(215) < 214)), "attention_mask differ"),
                         (dict(pixel_values=kw["pixel_values"][:3]), "pixel_values of shape")):
        with pytest.raises(ValueError, match="causal_trace: .*" + word):
            eval_utils.causal_trace(model, clean=clean, corrupt=dict(kw, **change))
    moved = kw["input_ids"].clone()
    at = (moved[0] == model.img_context_token_id).nonzero().flatten()
    moved[0, at[0]], moved[0, at[0] - 1] = moved[0, at[0] - 1].item(), moved[0, at[0]].item()           # one <IMG_CONTEXT> token one place to the left
    with pytest.raises(ValueError, match="causal_trace: .*<IMG_CONTEXT> tokens at different positions"):
        eval_utils.causal_trace(model, clean=clean, corrupt=dict(kw, input_ids=moved))
    with pytest.raises(ValueError, match="causal_trace: width"):
        eval_utils.causal_trace(model, clean=clean, corrupt=dict(kw), width=LAYERS + 1)


# ---- the graph key ------------------------------------------------------------------------------------------------------------------
def test_key_tail_of_calls_without_the_options_is_the_tuple_it_was():
    V, shape = 1000, (2, 215)
    cases = (dict(), dict(return_logprobs=True), dict(candidate_ids=[1, 2, 3], top_logprobs=4), dict(return_score_attention=True),
             dict(return_token_attention=True, return_logprobs=True), dict(return_depth_lens=True))
    was = ((), ("logprobs",), ("candidates", ("top_logprobs", 4)), (("score_attention", 0),), ("logprobs", ("score_attention", 0), ("score_attention_tokens", 215)),
           ("depth_lens",))
    mask = torch.zeros(shape, dtype=torch.bool)
    for kw, tail in zip(cases, was):
        ro = readouts.ReadOuts.parse(V, "given", ids_shape=shape, **kw)
        assert ro.key_tail(shape) == tail and not ro.touches_stream, kw
        # the options add nothing to the key: a call that carries one is never captured
        armed = readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=LAYERS, return_stream=mask, stream_patch=StreamPatch(mask, torch.zeros(0, 1, 8, dtype=BF), (0, 1)),
                                        **kw)
        assert armed.key_tail(shape) == tail and armed.touches_stream, kw


# ---- restored_fraction -----------------------------------------------------------------------------------------------------------------
def test_restored_fraction_on_hand_made_inputs():
    clean = torch.tensor([0.75, 0.50, 0.25])
    corrupt = torch.tensor([0.25, 0.50, 0.75])
    score = torch.tensor([[0.25, 0.50, 0.75, 1.00], [0.50, 0.25, 0.75, 0.50], [0.75, 0.50, 0.25, 0.875]])
    got = eval_utils.restored_fraction(score, clean, corrupt)
    assert got.dtype == torch.float32 and got[0].tolist() == [0.0, 0.5, 1.0, 1.5] and got[2].tolist() == [0.0, 0.5, 1.0, -0.25]
    assert got[1].isnan().all()                                                               # a zero denominator: NaN, also where the score did not move
    cube = eval_utils.restored_fraction(score.view(3, 2, 2).to(BF), clean.to(BF), corrupt.to(BF))
    assert cube.shape == (3, 2, 2) and cube[0].flatten().tolist() == [0.0, 0.5, 1.0, 1.5] and cube[1].isnan().all()
    assert eval_utils.restored_fraction(clean, clean, corrupt).tolist()[::2] == [1.0, 1.0]
    for bad in (lambda: eval_utils.restored_fraction(score, clean[:2], corrupt[:2]), lambda: eval_utils.restored_fraction(score, clean, corrupt[:2]),
                lambda: eval_utils.restored_fraction(score, clean[None], corrupt[None])):
        with pytest.raises(ValueError, match="restored_fraction"):
            bad()


# ---- the composed reference, pinned to the existing oracle ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rig():
    """Weights seed 63 on the host rig, every clip alone in bf16 -> model, cfg, sd, per clip: (the clip's inputs with labels, the oracle's keyword
    inputs, its plain composed states)."""
    model, cfg, kw = host_rig()
    sd = synth.make_state_dict(cfg, seed=63, rich=True)
    clips = []
    for b in range(2):
        one, n = one_clip(kw, b, frames=FRAMES)
        inputs = dict({k: v for k, v in one.items() if k != "labels"}, img_context_token_id=model.img_context_token_id)
        clips.append((one, inputs, DL.composed_states(sd, cfg, **inputs)))
    return model, cfg, sd, clips


def same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_the_two_clips_share_a_token_layout():
    model, cfg, kw = host_rig()
    assert kw["attention_mask"].sum(1).tolist() == [215, 215]
    ctx = kw["input_ids"] == model.img_context_token_id
    assert torch.equal(ctx[0], ctx[1]) and not torch.equal(kw["input_ids"][0], kw["input_ids"][1])


def test_reference_empty_patch_and_self_patch_are_the_composed_states():
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[1]
    am = one["attention_mask"]
    every = torch.ones_like(am)
    none = torch.zeros_like(am)
    H = plain[0].shape[-1]
    for patches in ((), [(none, torch.zeros(0, 2, H, dtype=BF), (1, 3))], [(every, torch.zeros(215, 0, H, dtype=BF), (2, 2))]):
        got = SP.composed_states(sd, cfg, **inputs, patches=patches)
        assert len(got) == LAYERS + 1 and all(same(g, p) for g, p in zip(got, plain))
    seg = model.segment_masks(one["input_ids"], am, one["image_flags"])
    for mask, depths in ((every, (0, LAYERS)), (seg["frames"], (1, 3)), (seg["score_row"], (3, 4))):
        values, index = SP.capture(plain, mask, am, depths)
        assert tuple(values.shape) == (int(mask.sum()), depths[1] - depths[0], H) and index.shape == (int(mask.sum()), 2)
        got = SP.composed_states(sd, cfg, **inputs, patches=[(mask, values, depths)])
        assert all(same(g, p) for g, p in zip(got, plain)), depths
        again, _ = SP.capture(got, mask, am, depths)                                           # the capture reads the stream as the layer consumes it
        assert same(again, values)


def test_reference_transplant_of_every_row_turns_the_recipient_into_the_donor():
    model, cfg, sd, clips = oracle_rig()
    (_, _, donor), (one, inputs, own) = clips
    every = torch.ones_like(one["attention_mask"])
    assert not same(donor[0], own[0])
    for d in range(LAYERS):
        values, _ = SP.capture(donor, every, one["attention_mask"], (d, d + 1))
        got = SP.composed_states(sd, cfg, **inputs, patches=[(every, values, (d, d + 1))])
        for depth in range(LAYERS + 1):
            assert same(got[depth], (donor if depth >= d else own)[depth]), (d, depth)


def test_oracle_condition_patching_the_score_row_moves_the_oracle():
    """Weights seed 63, tokens seed 302, two clips of two frames, every clip alone in bf16; clip 0 the donor, clip 1 the recipient.  Measured on
    the host: the donor scores 0.48047, the recipient 0.50000; the donor's score row patched into the recipient in front of layer 1 gives
    0.48633 (3.5 bf16 ulps from the recipient's plain score), of layer 2 0.48828 (3.0), of layer 3 0.48242 (4.5); all rows patched at any one
    depth give the donor's 0.48047.  Each score-row case must lie at least 2 ulps from the plain score - twice the GPU file's bar: a patch that
    did nothing could not pass there.  (The table is printed, not pinned: the oracle's bf16 sums follow the host's thread count.)"""
    model, cfg, sd, clips = oracle_rig()
    (d_one, _, donor), (one, inputs, own) = clips
    am = one["attention_mask"]
    score = lambda states: float(SP.lens(sd, cfg, states, am, one["labels"], 2)["score"][0, LAYERS])
    donor_score, plain_score = score(donor), score(own)
    print(f"donor (clip 0) {donor_score:.5f}, recipient (clip 1) {plain_score:.5f}")
    assert bf16_ulps(donor_score, plain_score) >= 2
    row = model.segment_masks(one["input_ids"], am, one["image_flags"])["score_row"]
    assert row.nonzero().tolist() == [[0, 211]]
    every = torch.ones_like(am)
    for d in (1, 2, 3):
        values, _ = SP.capture(donor, row, am, (d, d + 1))
        got = score(SP.composed_states(sd, cfg, **inputs, patches=[(row, values, (d, d + 1))]))
        print(f"score row patched over [{d}, {d + 1}): {got:.5f} = {bf16_ulps(got, plain_score):.1f} bf16 ulps from the recipient's plain score")
        assert bf16_ulps(got, plain_score) >= 2, d
    for d in range(LAYERS):
        values, _ = SP.capture(donor, every, am, (d, d + 1))
        assert score(SP.composed_states(sd, cfg, **inputs, patches=[(every, values, (d, d + 1))])) == donor_score, d
