"""The host side of the pass options without a GPU: ``forward()`` checks every armed option once (``ReadOuts.parse`` runs once, and each of the
functions it is made of at most once), and a call with one fault raises exactly the text it always raised - one per kind of check (capture,
qualifier without its capture, patch type, window, values layout, index, scale type, scale shape, NaN) and per family (stream, head, neuron),
the families' own extras and the two ``key_drop`` qualifiers.  On the host rig of tests/test_stream_patch_cpu.py: a model that lives on the host,
where anything that reached a launch would raise NativeError, not ValueError."""
import pytest
import torch

from test_stream_patch_cpu import host_rig

from aigv_assessor_amd import readouts
from aigv_assessor_amd.readouts import HeadPatch, HeadScale, NeuronPatch, NeuronScale, StreamPatch

LAYERS, HEADS, D = 4, 4, 128
BF = torch.bfloat16
COUNTED = ("key_drop_mask", "key_drop_qualifiers", "stream_options", "head_options", "neuron_options")


class Stop(Exception):
    """Raised in place of the first step of ``forward()`` that would touch the device."""


def no_prefetch(pixel_values, visual_tokens, motion_feature):
    """``_take_ahead`` of a call that hands plain ``pixel_values`` in, without its look at the device's streams (the rig has no device)."""
    return pixel_values, visual_tokens, motion_feature


def rig():
    model, cfg, kw = host_rig()
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    return model, cfg, kw, seg["score_row"], units[:, 0]             # (the score rows: two tokens, one per clip; frame 0 of both clips)


def everything_armed(cfg, mask, keys):
    """All eight row options plus ``key_drop`` and its two qualifiers, every one of them valid on the rig."""
    H, I = cfg.llm_config.hidden_size, cfg.llm_config.intermediate_size
    return dict(key_drop=keys, key_drop_rows=mask, key_drop_layers=(0, 2),
                return_stream=mask, stream_patch=StreamPatch(mask, torch.zeros(2, 1, H, dtype=BF), (0, 1)),
                return_heads=mask, head_patch=HeadPatch(mask, torch.zeros(2, 1, HEADS, D, dtype=BF), (1, 2)), head_scale=HeadScale(torch.full((LAYERS, HEADS), 0.5)),
                return_neurons=mask, neuron_patch=NeuronPatch(mask, torch.zeros(2, 1, I, dtype=BF), (2, 3)), neuron_scale=NeuronScale(torch.full((LAYERS,), 0.5), None, mask))


@pytest.mark.parametrize("stop_at", ("_take_ahead", "_motion_feature"))
def test_forward_checks_every_armed_option_once(monkeypatch, stop_at):
    """``_take_ahead`` is the first step that may wait for the device, ``_motion_feature`` the first that launches: the call ends there.  In front of
    the first every option has been checked - the record exists -, and up to the second nothing has been checked again."""
    model, cfg, kw, mask, keys = rig()
    counts = dict.fromkeys(COUNTED + ("parse",), 0)

    def counted(name, fn):
        def wrapper(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapper
    for name in COUNTED:
        monkeypatch.setattr(readouts, name, counted(name, getattr(readouts, name)))
    parse = readouts.ReadOuts.parse.__func__
    monkeypatch.setattr(readouts.ReadOuts, "parse", classmethod(counted("parse", parse)))

    def stop(*a, **k):
        raise Stop
    if stop_at != "_take_ahead":
        monkeypatch.setattr(model, "_take_ahead", no_prefetch)
    monkeypatch.setattr(model, stop_at, stop)
    with pytest.raises(Stop):
        model(**kw, **everything_armed(cfg, mask, keys))
    print(stop_at, counts)
    assert all(counts[name] >= 1 for name in COUNTED), counts                    # the call did reach every one of them
    assert counts["parse"] == 1 and all(counts[name] <= 1 for name in COUNTED), counts


def test_the_armed_call_parses_to_the_record_forward_works_with():
    """What ``forward()`` reads from: every option of the armed call in its checked form, and ``forward_kwargs`` hands all of them on."""
    model, cfg, kw, mask, keys = rig()
    llm = cfg.llm_config
    opts = everything_armed(cfg, mask, keys)
    ro = readouts.ReadOuts.parse(llm.vocab_size, kw["labels"], ids_shape=kw["input_ids"].shape, n_layers=LAYERS, n_heads=HEADS, head_dim=D, n_inter=llm.intermediate_size, **opts)
    assert torch.equal(ro.key_drop, keys) and torch.equal(ro.key_drop_rows, mask) and ro.key_drop_layers == (0, 2)
    assert (ro.stream_depths, ro.head_layers, ro.neuron_layers) == ((0, LAYERS),) * 3 and ro.neuron_ids is None
    assert (ro.stream_patch.depths, ro.head_patch.layers, ro.neuron_patch.layers) == ((0, 1), (1, 2), (2, 3))
    assert all(torch.equal(t, mask) for t in (ro.stream_rows, ro.head_rows, ro.neuron_rows, ro.stream_patch.rows, ro.head_patch.rows, ro.neuron_patch.rows, ro.neuron_scale.rows))
    assert ro.head_scale.rows is None and ro.head_scale.scale.dtype == ro.neuron_scale.scale.dtype == torch.float32
    assert ro.touches_stream and ro.runs_eagerly and set(readouts.forward_kwargs(ro)) == set(opts) | {"stream_depths", "head_layers", "neuron_layers"}     # (the defaulted windows)
    assert [f for f in readouts.ReadOuts.__dataclass_fields__][11:] == ["neuron_rows", "neuron_layers", "neuron_ids", "neuron_patch", "neuron_scale", "stream_rows", "stream_depths",
                                                                       "stream_patch", "head_rows", "head_layers", "head_patch", "head_scale"]


def single_faults():
    """(what the fault is, the options of the call, the exact text) - a call with one fault, on the rig."""
    model, cfg, kw, mask, keys = rig()
    H, I = cfg.llm_config.hidden_size, cfg.llm_config.intermediate_size
    short, shape = mask[:, :100], "shape (2, 100) differs from input_ids (2, 215)"
    a_mask = "expected a bool or integer tensor [B, N] laid out like input_ids"
    sv = lambda n=2, d=1, h=H, dt=BF: torch.zeros(n, d, h, dtype=dt)
    hv = lambda n=2, l=1, h=HEADS, d=D, dt=BF: torch.zeros(n, l, h, d, dtype=dt)
    nv = lambda n=2, l=1, w=I, dt=BF: torch.zeros(n, l, w, dtype=dt)
    ones, per_layer = torch.ones(LAYERS, HEADS), torch.ones(LAYERS)
    nan2, nan1 = ones.clone(), per_layer.clone()
    nan2[2, 1] = nan1[2] = float("nan")
    bad_index, pair = torch.zeros(2, 3, dtype=torch.long), torch.tensor([[1, 5]])
    return (
        # a capture
        ("stream capture", dict(return_stream=short), f"return_stream: {shape}"),
        ("head capture", dict(return_heads=mask.float()), f"return_heads: {a_mask}"),
        ("neuron capture", dict(return_neurons=short), f"return_neurons: {shape}"),
        # a qualifier without its capture
        ("stream qualifier", dict(stream_depths=(0, 2)), "stream_depths: qualifies return_stream and needs one"),
        ("head qualifier", dict(head_layers=(0, 2)), "head_layers: qualifies return_heads and needs one"),
        ("neuron qualifier", dict(neuron_layers=(0, 2)), "neuron_layers: qualifies return_neurons and needs one"),
        ("neuron ids qualifier", dict(neuron_ids=torch.tensor([1])), "neuron_ids: qualifies return_neurons and needs one"),
        ("key_drop_rows alone", dict(key_drop_rows=mask), "key_drop_rows: qualifies key_drop and needs one"),
        ("key_drop_layers alone", dict(key_drop_layers=(0, 2)), "key_drop_layers: qualifies key_drop and needs one"),
        # the type of a patch record
        ("stream patch type", dict(stream_patch=(mask, sv(), (0, 1))), "stream_patch: expected a readouts.StreamPatch, got tuple"),
        ("head patch type", dict(head_patch=StreamPatch(mask, sv(), (0, 1))), "head_patch: expected a readouts.HeadPatch, got StreamPatch"),
        ("neuron patch type", dict(neuron_patch=[mask]), "neuron_patch: expected a readouts.NeuronPatch, got list"),
        # a window
        ("stream capture window", dict(return_stream=mask, stream_depths=(2, 1)), "stream_depths: (2, 1) outside 0 <= lo <= hi <= 4"),
        ("stream patch window", dict(stream_patch=StreamPatch(mask, sv(), (0, LAYERS + 1))), "stream_patch: depths: (0, 5) outside 0 <= lo <= hi <= 4"),
        ("head capture window", dict(return_heads=mask, head_layers=2), "head_layers: expected a pair of ints (lo, hi), got 2"),
        ("head patch window", dict(head_patch=HeadPatch(mask, hv(), (-1, 2))), "head_patch: layers: (-1, 2) outside 0 <= lo <= hi <= 4"),
        ("neuron capture window", dict(return_neurons=mask, neuron_layers=(False, True)), "neuron_layers: expected a pair of ints (lo, hi), got (False, True)"),
        ("neuron patch window", dict(neuron_patch=NeuronPatch(mask, nv(), (0, 1, 2))), "neuron_patch: layers: expected a pair of ints (lo, hi), got (0, 1, 2)"),
        ("key_drop window", dict(key_drop=keys, key_drop_layers=(3, 2)), "key_drop_layers: (3, 2) outside 0 <= lo <= hi <= 4"),
        ("key_drop window type", dict(key_drop=keys, key_drop_layers=(0.0, 2)), "key_drop_layers: expected a pair of ints (lo, hi), got (0.0, 2)"),
        ("key_drop mask", dict(key_drop=keys[0]), f"key_drop: {a_mask}"),
        ("key_drop shape", dict(key_drop=keys[:, :100]), f"key_drop: {shape}"),
        ("key_drop rows", dict(key_drop=keys, key_drop_rows=mask.float()), f"key_drop_rows: {a_mask}"),
        ("key_drop rows shape", dict(key_drop=keys, key_drop_rows=short), f"key_drop_rows: {shape}"),
        # the layout of a patch's values
        ("stream values dtype", dict(stream_patch=StreamPatch(mask, sv(dt=torch.float32), (0, 1))),
         f"stream_patch: values must be a bf16 tensor [n, hi - lo = 1, H] laid out like a captured stream, got (2, 1, {H}) torch.float32"),
        ("stream values window", dict(stream_patch=StreamPatch(mask, sv(d=2), (1, 2))),
         f"stream_patch: values must be a bf16 tensor [n, hi - lo = 1, H] laid out like a captured stream, got (2, 2, {H}) torch.bfloat16"),
        ("stream values no tensor", dict(stream_patch=StreamPatch(mask, [1.0], (0, 2))),
         "stream_patch: values must be a bf16 tensor [n, hi - lo = 2, H] laid out like a captured stream, got list"),
        ("head values heads", dict(head_patch=HeadPatch(mask, hv(h=3), (0, 1))),
         "head_patch: values must be a bf16 tensor [n, hi - lo = 1, n_heads = 4, D = 128] laid out like captured heads, got (2, 1, 3, 128) torch.bfloat16"),
        ("head values rank", dict(head_patch=HeadPatch(mask, hv()[0], (0, 1))),
         "head_patch: values must be a bf16 tensor [n, hi - lo = 1, n_heads = 4, D = 128] laid out like captured heads, got (1, 4, 128) torch.bfloat16"),
        ("neuron values width", dict(neuron_patch=NeuronPatch(mask, nv(w=8), (0, 1))),
         f"neuron_patch: values must be a bf16 tensor [n, hi - lo = 1, I = {I}] laid out like captured neurons, got (2, 1, 8) torch.bfloat16"),
        ("neuron values sparse width", dict(neuron_patch=NeuronPatch(mask, nv(), (0, 1), None, torch.tensor([3, 700]))),
         f"neuron_patch: values must be a bf16 tensor [n, hi - lo = 1, m = 2] laid out like captured neurons, got (2, 1, {I}) torch.bfloat16"),
        # a donor's index
        ("stream index", dict(stream_patch=StreamPatch(mask, sv(), (0, 1), bad_index)),
         "stream_patch: index must be an integer tensor [n, 2] of (clip, position) pairs (a donor's stream_index)"),
        ("head index", dict(head_patch=HeadPatch(mask, hv(), (0, 1), bad_index[:, :2].float())),
         "head_patch: index must be an integer tensor [n, 2] of (clip, position) pairs (a donor's heads_index)"),
        ("neuron index", dict(neuron_patch=NeuronPatch(mask, nv(), (0, 1), [[0, 211], [1, 211]])),
         "neuron_patch: index must be an integer tensor [n, 2] of (clip, position) pairs (a donor's neurons_index)"),
        # a patch's row mask
        ("stream patch rows", dict(stream_patch=StreamPatch(short, sv(), (0, 1))), f"stream_patch: rows: {shape}"),
        ("head patch rows", dict(head_patch=HeadPatch(mask[0], hv(), (0, 1))), f"head_patch: rows: {a_mask}"),
        ("neuron patch rows", dict(neuron_patch=NeuronPatch(short, nv(), (0, 1))), f"neuron_patch: rows: {shape}"),
        # the families' own extras
        ("head patch heads", dict(head_patch=HeadPatch(mask, hv(), (0, 1), None, torch.ones(HEADS))),
         "head_patch: heads must be a bool tensor [n_heads = 4] or [hi - lo = 1, n_heads = 4], got (4,) torch.float32"),
        ("neuron patch list", dict(neuron_patch=NeuronPatch(mask, nv(w=2), (0, 1), None, torch.tensor([7, 3]))), "neuron_patch: neurons: neuron numbers must be strictly ascending"),
        ("neuron patch list range", dict(neuron_patch=NeuronPatch(mask, nv(w=1), (0, 1), None, torch.tensor([I]))), f"neuron_patch: neurons: neuron numbers outside 0..{I - 1}"),
        ("neuron ids", dict(return_neurons=mask, neuron_ids=torch.tensor([0.5])), "neuron_ids: expected an integer tensor [m] of neuron numbers"),
        # the type of a scale record
        ("head scale type", dict(head_scale=ones), "head_scale: expected a readouts.HeadScale, got Tensor"),
        ("neuron scale type", dict(neuron_scale=HeadScale(ones)), "neuron_scale: expected a readouts.NeuronScale, got HeadScale"),
        # the shape of a scale
        ("head scale shape", dict(head_scale=HeadScale(ones[:3])), "head_scale: scale must be a float tensor [L = 4, n_heads = 4], got (3, 4) torch.float32"),
        ("head scale dtype", dict(head_scale=HeadScale(ones.long())), "head_scale: scale must be a float tensor [L = 4, n_heads = 4], got (4, 4) torch.int64"),
        ("head scale no tensor", dict(head_scale=HeadScale(1.0)), "head_scale: scale must be a float tensor [L = 4, n_heads = 4], got float"),
        ("neuron scale shape", dict(neuron_scale=NeuronScale(per_layer[:3])), "neuron_scale: scale must be a float tensor [L = 4] when neurons is None, got (3,) torch.float32"),
        ("neuron scale sparse shape", dict(neuron_scale=NeuronScale(torch.zeros(2), pair)), "neuron_scale: scale must be a float tensor [m = 1] beside neurons [m, 2], got (2,) torch.float32"),
        ("neuron scale pairs", dict(neuron_scale=NeuronScale(torch.zeros(1), pair[0])), "neuron_scale: neurons must be an integer tensor [m, 2] of (layer, neuron) pairs"),
        ("neuron scale range", dict(neuron_scale=NeuronScale(torch.zeros(1), torch.tensor([[LAYERS, 0]]))),
         f"neuron_scale: a (layer, neuron) pair outside layers 0..{LAYERS - 1}, neurons 0..{I - 1}"),
        ("neuron scale unique", dict(neuron_scale=NeuronScale(torch.zeros(2), pair.expand(2, 2))), "neuron_scale: the (layer, neuron) pairs must be unique"),
        # a NaN factor
        ("head scale NaN", dict(head_scale=HeadScale(nan2)), "head_scale: scale[2, 1] is NaN"),
        ("neuron scale NaN", dict(neuron_scale=NeuronScale(nan1)), "neuron_scale: scale[2] is NaN"),
        ("neuron scale sparse NaN", dict(neuron_scale=NeuronScale(nan1[2:3], pair)), "neuron_scale: scale[0] is NaN"),
        # a scale's row mask
        ("head scale rows", dict(head_scale=HeadScale(ones, short)), f"head_scale: rows: {shape}"),
        ("neuron scale rows", dict(neuron_scale=NeuronScale(per_layer, None, mask.float())), f"neuron_scale: rows: {a_mask}"),
        # against the plan
        ("stream patch count", dict(stream_patch=StreamPatch(mask, sv(n=3), (0, 1))), "stream_patch: values hold 3 rows, the mask selects 2 tokens the pass runs"),
        ("stream patch width", dict(stream_patch=StreamPatch(mask, sv(h=H - 8), (0, 1))), f"stream_patch: values of width {H - 8}, the residual stream has H = {H}"),
        ("head patch count", dict(head_patch=HeadPatch(mask, hv(), (0, 1), torch.tensor([[0, 211]]))), "head_patch: index holds 1 pairs, the mask selects 2 tokens the pass runs"),
        ("neuron patch pair", dict(neuron_patch=NeuronPatch(mask, nv(), (0, 1), torch.tensor([[0, 211], [1, 210]]))),
         "neuron_patch: pair 1 of index is (clip, position) = (1, 210), the pass's is (1, 211)"),
        # the read-outs that share the record
        ("candidates", dict(candidate_ids=torch.zeros(2, 2, dtype=torch.long)), "candidate_ids: expected 1..64 integer token ids in one dimension, got (2, 2) torch.int64"),
        ("top-k", dict(top_logprobs=17), "top_logprobs: expected an int in 1..16, got 17"),
    )


FAULTS = single_faults()


@pytest.mark.parametrize("case", range(len(FAULTS)), ids=[f[0].replace(" ", "_") for f in FAULTS])
def test_a_call_with_one_fault_raises_the_text_it_always_raised(monkeypatch, case):
    model, cfg, kw = host_rig()
    monkeypatch.setattr(model, "_take_ahead", no_prefetch)
    _, opts, text = FAULTS[case]
    with pytest.raises(ValueError) as err:
        model(**kw, **opts)
    assert str(err.value) == text


def test_plan_free_faults_of_two_options_come_in_the_order_of_the_checks(monkeypatch):
    """The key-drop qualifiers, key_drop, stream, head, neuron, candidates, top-k: of two plan-free faults the earlier wins."""
    model, cfg, kw, mask, keys = rig()
    monkeypatch.setattr(model, "_take_ahead", no_prefetch)
    order = (("key_drop_rows", dict(key_drop_rows=mask)), ("key_drop:", dict(key_drop=keys[0])), ("stream_depths", dict(stream_depths=(0, 1))),
             ("head_scale", dict(head_scale=1.0)), ("neuron_ids", dict(neuron_ids=torch.tensor([1]))), ("candidate_ids", dict(candidate_ids=[])), ("top_logprobs", dict(top_logprobs=0)))
    for i, (first, a) in enumerate(order):
        for _, b in order[i + 1:]:
            if set(a) & set(b) or ("key_drop_rows" in a and "key_drop" in b):
                continue
            with pytest.raises(ValueError) as err:
                model(**kw, **a, **b)
            assert str(err.value).startswith(first), (first, b, str(err.value))
