"""The eight sweeps of eval_utils without a GPU, against a recording stand-in for the model: the host rig's model (so ``unit_masks``,
``segment_masks`` and ``config`` are real) whose ``forward``, ``vit_tokens`` and ``motion_feature`` log their arguments and return canned tensors -
``score1`` follows from the call number.  Per sweep: the exact sequence of ``forward`` calls (which option, which window or (layer, head) or (layer,
neuron), which masks, which other keywords), InternViT and SlowFast once, and the returned tensors - shapes, values from the canned scores, NaN
positions, ``restored`` against ``restored_fraction``."""
import pytest
import torch

from test_key_drop_cpu import two_clips
from test_stream_patch_cpu import host_rig

from aigv_assessor_amd import eval_utils
from aigv_assessor_amd.readouts import HeadPatch, HeadScale, NeuronPatch, NeuronScale, StreamPatch

LAYERS, HEADS = 4, 4
WIDTH = 8            # the trailing width of the canned captures
NAN = float("nan")
INPUTS = {"input_ids", "attention_mask", "image_flags", "labels", "visual_tokens", "motion_feature"}


class Recorder:
    """``forward`` call n returns ``score1 = score(n)`` and, for a capture option, a tensor that follows from n and the mask."""

    def __init__(self, monkeypatch, model, score=lambda n: [float(n), 2.0 * n + 0.5]):
        self.calls, self.front, self.outs, self.score = [], [], [], score
        self.tokens, self.motion = torch.full((1,), 11.0), torch.full((1,), 13.0)
        monkeypatch.setattr(model, "forward", self.forward)
        monkeypatch.setattr(model, "vit_tokens", lambda pixel_values: self.front.append(("vit_tokens", pixel_values)) or self.tokens)
        monkeypatch.setattr(model, "motion_feature", lambda pixel_values, batch: self.front.append(("motion_feature", pixel_values, batch)) or self.motion)

    def forward(self, **kw):
        n = len(self.calls)
        self.calls.append(kw)
        out = {"score1": torch.tensor(self.score(n))}
        for opt, name, lead in (("return_stream", "stream", (LAYERS,)), ("return_heads", "heads", (LAYERS, HEADS)), ("return_neurons", "neurons", None)):
            if opt in kw:
                index = kw[opt].nonzero()
                lo, hi = kw.get("neuron_layers", (0, LAYERS))
                shape = (len(index),) + ((hi - lo,) if lead is None else lead) + (WIDTH,)
                cells = torch.arange(int(torch.tensor(shape).prod())).view(shape)
                out[name] = ((cells * (2 * n + 3) + cells // WIDTH) % 31).to(torch.bfloat16)     # (differs by call, row, layer and column)
                out[name + "_index"] = index
        self.outs.append(out)
        return out

    def ran_the_front_once(self, pixel_values, B=2, motion=True):
        want = (["motion_feature"] if motion else []) + ["vit_tokens"]
        return [f[0] for f in self.front] == want and all(f[1] is pixel_values for f in self.front) and (not motion or self.front[0][2] == B)

    def scores(self, first, *shape):
        return torch.tensor([self.score(n) for n in range(first, len(self.calls))]).t().reshape(2, *shape)


def eq(a, b):
    """Equal shapes, dtypes and values, NaN at the same places."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def same_mask(got, want):
    return want is None if got is None else tuple(got.shape) == tuple(want.shape) and torch.equal(got.bool(), want.bool())


def rig():
    model, cfg, kw = host_rig()
    seg = model.segment_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    clip0 = seg["score_row"].clone()
    clip0[1] = False                                                          # selects no row of clip 1: the NaN rule
    return model, cfg, kw, seg, clip0


def recipient_calls_carry(rec, calls, corrupt, extra):
    """Every pass of the recipient: the corrupt inputs without ``pixel_values``, the tokens and the feature of the one front-end run, ``extra``."""
    for kw in calls:
        assert "pixel_values" not in kw and kw["visual_tokens"] is rec.tokens and kw["motion_feature"] is rec.motion
        assert all(kw[k] is corrupt[k] for k in ("input_ids", "attention_mask", "image_flags", "labels")) and all(kw[k] == v for k, v in extra.items())


def the_trace_block(res, rec, *shape):
    """``clean_score / corrupt_score / score / restored`` from the canned scores; clip 1's clean and corrupt scores are equal: NaN there."""
    clean, corrupt, score = torch.tensor(rec.score(0)), torch.tensor(rec.score(1)), rec.scores(2, *shape)
    assert eq(res["clean_score"], clean) and eq(res["corrupt_score"], corrupt) and eq(res["score"], score)
    assert eq(res["restored"], eval_utils.restored_fraction(score, clean, corrupt)) and res["restored"][1].isnan().all() and not res["restored"][0].isnan().any()
    assert eq(res["restored"][0], (score[0] - corrupt[0]) / (clean[0] - corrupt[0]))


TRACE_SCORE = lambda n: [float(n * n), 7.0]


# ---- the knock-out sweeps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given_motion", (False, True))
def test_frame_ablation(monkeypatch, given_motion):
    model, cfg, _ = host_rig()
    kw, _ = two_clips(cfg, 302, frames=(2, 1))                                # clip 1 lacks frame 1: the NaN rule
    given = kw.pop("motion_feature")
    rec = Recorder(monkeypatch, model)
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    res = eval_utils.frame_ablation(model, **kw, **(dict(motion_feature=given) if given_motion else {}), return_logprobs=True)
    assert rec.ran_the_front_once(kw["pixel_values"], motion=not given_motion)
    assert len(rec.calls) == 4 and res["outs"] == rec.outs and torch.equal(res["units"], units) and tuple(units.shape) == (2, 3, 215)
    for u, call in enumerate(rec.calls):
        assert set(call) == INPUTS | {"return_logprobs"} | ({"key_drop"} if u else set()) and call["return_logprobs"] is True
        assert call["visual_tokens"] is rec.tokens and call["motion_feature"] is (given if given_motion else rec.motion) and call["labels"] is kw["labels"]
        assert u == 0 or torch.equal(call["key_drop"], units[:, u - 1])
    ablated = rec.scores(1, 3)
    ablated[1, 1] = NAN
    assert eq(res["score1"], torch.tensor(rec.score(0))) and eq(res["ablated"], ablated) and eq(res["delta"], res["score1"][:, None] - ablated)


def test_flow_knockout(monkeypatch):
    model, cfg, kw, seg, clip0 = rig()
    inputs = {k: v for k, v in kw.items() if k != "motion_feature"}
    keys0 = seg["frames"].clone()
    keys0[0] = False                                                          # no key in clip 0
    paths = [("a", seg["frames"].long(), seg["score_row"]), ("every row", seg["frames"], None), ("no key", keys0, None), ("no row", seg["frames"], clip0)]
    rec = Recorder(monkeypatch, model)
    res = eval_utils.flow_knockout(model, **inputs, paths=paths, width=3, stride=2, top_logprobs=2)
    assert rec.ran_the_front_once(kw["pixel_values"])
    assert res["windows"] == [(0, 3), (2, 4)] and [p[0] for p in res["paths"]] == [p[0] for p in paths] and res["outs"] == rec.outs and len(rec.calls) == 9
    assert set(rec.calls[0]) == INPUTS | {"top_logprobs"}
    for i, call in enumerate(rec.calls[1:]):
        (_, keys, rows), window = paths[i // 2], res["windows"][i % 2]
        assert set(call) == INPUTS | {"top_logprobs", "key_drop", "key_drop_rows", "key_drop_layers"} and call["top_logprobs"] == 2 and call["visual_tokens"] is rec.tokens
        assert same_mask(call["key_drop"], keys) and call["key_drop"].dtype == torch.bool and same_mask(call["key_drop_rows"], rows) and call["key_drop_layers"] == window
    knocked = rec.scores(1, 4, 2)
    knocked[0, 2], knocked[1, 3] = NAN, NAN
    assert eq(res["score1"], torch.tensor(rec.score(0))) and eq(res["knocked"], knocked) and eq(res["delta"], res["score1"][:, None, None] - knocked)
    # the default paths, a window list of one, a given motion feature
    rec = Recorder(monkeypatch, model)
    res = eval_utils.flow_knockout(model, **kw, width=LAYERS)
    assert rec.ran_the_front_once(kw["pixel_values"], motion=False) and res["windows"] == [(0, LAYERS)] and len(rec.calls) == 4
    want = (("frames->score_row", seg["frames"], seg["score_row"]), ("frames->text_after", seg["frames"], seg["text_after"]),
            ("text_after->score_row", seg["text_after"] & ~seg["score_row"], seg["score_row"]))
    for call, (name, keys, rows), got in zip(rec.calls[1:], want, res["paths"]):
        assert got[0] == name and same_mask(call["key_drop"], keys) and same_mask(call["key_drop_rows"], rows) and call["motion_feature"] is kw["motion_feature"]
    assert tuple(res["knocked"].shape) == (2, 3, 1) and not res["knocked"].isnan().any()
    with pytest.raises(ValueError, match=f"flow_knockout: width = 5 outside 1..{LAYERS} or stride = 5 below 1"):
        eval_utils.flow_knockout(model, **kw, width=5)
    with pytest.raises(ValueError, match=f"flow_knockout: width = 1 outside 1..{LAYERS} or stride = 0 below 1"):
        eval_utils.flow_knockout(model, **kw, width=1, stride=0)


def test_head_knockout(monkeypatch):
    model, cfg, kw, seg, clip0 = rig()
    inputs = {k: v for k, v in kw.items() if k != "motion_feature"}
    rec = Recorder(monkeypatch, model)
    res = eval_utils.head_knockout(model, **inputs, layers=[3, 1], heads=[0, 2], rows=clip0.long())
    assert rec.ran_the_front_once(kw["pixel_values"]) and res["layers"] == [3, 1] and res["heads"] == [0, 2] and res["outs"] == rec.outs and len(rec.calls) == 5
    assert set(rec.calls[0]) == INPUTS
    for call, (l, h) in zip(rec.calls[1:], ((3, 0), (3, 2), (1, 0), (1, 2))):
        q = call["head_scale"]
        scale = torch.ones(LAYERS, HEADS)
        scale[l, h] = 0.0
        assert set(call) == INPUTS | {"head_scale"} and isinstance(q, HeadScale) and torch.equal(q.scale, scale) and same_mask(q.rows, clip0) and q.rows.dtype == torch.bool
        assert call["visual_tokens"] is rec.tokens and call["motion_feature"] is rec.motion
    knocked = rec.scores(1, 2, 2)
    knocked[1] = NAN
    assert eq(res["score1"], torch.tensor(rec.score(0))) and eq(res["knocked"], knocked) and eq(res["delta"], res["score1"][:, None, None] - knocked)
    # every row, an empty sweep
    rec = Recorder(monkeypatch, model)
    res = eval_utils.head_knockout(model, **kw, layers=[2], heads=[])
    assert len(rec.calls) == 1 and rec.ran_the_front_once(kw["pixel_values"], motion=False) and tuple(res["knocked"].shape) == (2, 1, 0)
    res = eval_utils.head_knockout(model, **kw, layers=[2], heads=[1])
    assert rec.calls[-1]["head_scale"].rows is None and not res["knocked"].isnan().any()


def test_mlp_knockout_and_neuron_knockout(monkeypatch):
    model, cfg, kw, seg, clip0 = rig()
    inputs = {k: v for k, v in kw.items() if k != "motion_feature"}
    rec = Recorder(monkeypatch, model)
    res = eval_utils.mlp_knockout(model, **inputs, layers=[2, 0], rows=clip0, return_logprobs=True)
    assert rec.ran_the_front_once(kw["pixel_values"]) and res["layers"] == [2, 0] and res["outs"] == rec.outs and len(rec.calls) == 3
    assert set(rec.calls[0]) == INPUTS | {"return_logprobs"}
    for call, l in zip(rec.calls[1:], (2, 0)):
        q = call["neuron_scale"]
        scale = torch.ones(LAYERS)
        scale[l] = 0.0
        assert set(call) == INPUTS | {"return_logprobs", "neuron_scale"} and isinstance(q, NeuronScale) and torch.equal(q.scale, scale) and q.neurons is None and same_mask(q.rows, clip0)
    knocked = rec.scores(1, 2)
    knocked[1] = NAN
    assert eq(res["score1"], torch.tensor(rec.score(0))) and eq(res["knocked"], knocked) and eq(res["delta"], res["score1"][:, None] - knocked)
    with pytest.raises(ValueError, match=r"mlp_knockout: layers \[4\] outside 0..3"):
        eval_utils.mlp_knockout(model, **kw, layers=[LAYERS])

    rec = Recorder(monkeypatch, model)
    pairs = [[3, 5], [0, 700]]
    res = eval_utils.neuron_knockout(model, pairs, **kw, rows=clip0)
    assert rec.ran_the_front_once(kw["pixel_values"], motion=False) and torch.equal(res["neurons"], torch.tensor(pairs)) and res["outs"] == rec.outs and len(rec.calls) == 3
    for call, pair in zip(rec.calls[1:], pairs):
        q = call["neuron_scale"]
        assert set(call) == INPUTS | {"neuron_scale"} and torch.equal(q.scale, torch.zeros(1)) and q.neurons.tolist() == [pair] and same_mask(q.rows, clip0)
        assert call["motion_feature"] is kw["motion_feature"] and call["visual_tokens"] is rec.tokens
    knocked = rec.scores(1, 2)
    knocked[1] = NAN
    assert eq(res["knocked"], knocked) and eq(res["delta"], res["score1"][:, None] - knocked)
    res = eval_utils.neuron_knockout(model, torch.zeros(0, 2, dtype=torch.long), **kw)
    assert tuple(res["knocked"].shape) == (2, 0)


# ---- the donor / recipient sweeps ---------------------------------------------------------------------------------------------------------
def two_batches(kw):
    clean = dict(kw)
    corrupt = dict(kw, pixel_values=kw["pixel_values"].flip(0), labels=kw["labels"].clone())
    del corrupt["motion_feature"]
    return clean, corrupt


def test_causal_trace(monkeypatch):
    model, cfg, kw, seg, clip0 = rig()
    clean, corrupt = two_batches(kw)
    text = seg["text_before"].clone()
    text[1] = False
    groups = [("score", seg["score_row"].long()), ("text of clip 0", text)]
    rec = Recorder(monkeypatch, model, TRACE_SCORE)
    res = eval_utils.causal_trace(model, clean=clean, corrupt=corrupt, groups=groups, width=3, stride=2, return_depth_lens=True)
    assert rec.ran_the_front_once(corrupt["pixel_values"])
    assert res["windows"] == [(0, 3), (2, 4)] and res["names"] == ["score", "text of clip 0"] and res["outs"] == rec.outs and len(rec.calls) == 6
    donor = rec.calls[0]
    assert set(donor) == set(clean) | {"return_stream", "return_depth_lens"} and all(donor[k] is clean[k] for k in clean)
    assert same_mask(donor["return_stream"], seg["score_row"] | text)
    assert set(rec.calls[1]) == INPUTS | {"return_depth_lens"}
    recipient_calls_carry(rec, rec.calls[1:], corrupt, dict(return_depth_lens=True))
    stream, index = rec.outs[0]["stream"], rec.outs[0]["stream_index"]
    for i, call in enumerate(rec.calls[2:]):
        (_, mask), (lo, hi) = groups[i // 2], res["windows"][i % 2]
        p = call["stream_patch"]
        own = mask.bool()[index[:, 0], index[:, 1]]
        assert set(call) == INPUTS | {"return_depth_lens", "stream_patch"} and isinstance(p, StreamPatch) and same_mask(p.rows, mask) and p.depths == (lo, hi)
        assert torch.equal(p.values, stream[own][:, lo:hi]) and p.values.is_contiguous() and torch.equal(p.index, index[own]) and int(own.sum()) == (2, int(text.sum()))[i // 2]
    the_trace_block(res, rec, 2, 2)
    # the default groups
    rec = Recorder(monkeypatch, model, TRACE_SCORE)
    res = eval_utils.causal_trace(model, clean=clean, corrupt=dict(kw), width=LAYERS, stride=LAYERS)
    assert res["names"] == ["frame0", "frame1", "motion", "text_before", "text_after", "score_row"] and rec.ran_the_front_once(kw["pixel_values"], motion=False)
    assert len(rec.calls) == 8 and tuple(res["score"].shape) == (2, 6, 1) and same_mask(rec.calls[-1]["stream_patch"].rows, seg["score_row"])
    assert all(call["motion_feature"] is kw["motion_feature"] for call in rec.calls[1:])
    with pytest.raises(ValueError, match=f"causal_trace: width = 0 outside 1..{LAYERS} or stride = 1 below 1"):
        eval_utils.causal_trace(model, clean=clean, corrupt=corrupt, width=0)


def test_head_trace(monkeypatch):
    model, cfg, kw, seg, clip0 = rig()
    clean, corrupt = two_batches(kw)
    rows = seg["score_row"]
    rec = Recorder(monkeypatch, model, TRACE_SCORE)
    res = eval_utils.head_trace(model, clean=clean, corrupt=corrupt, layers=[2, 0], heads=[1, 3], rows=rows.long(), candidate_ids=[1, 2])
    assert rec.ran_the_front_once(corrupt["pixel_values"]) and res["layers"] == [2, 0] and res["heads"] == [1, 3] and res["outs"] == rec.outs and len(rec.calls) == 6
    donor = rec.calls[0]
    assert set(donor) == set(clean) | {"return_heads", "candidate_ids"} and all(donor[k] is clean[k] for k in clean) and same_mask(donor["return_heads"], rows)
    assert set(rec.calls[1]) == INPUTS | {"candidate_ids"}
    recipient_calls_carry(rec, rec.calls[1:], corrupt, dict(candidate_ids=[1, 2]))
    heads, index = rec.outs[0]["heads"], rec.outs[0]["heads_index"]
    for call, (l, h) in zip(rec.calls[2:], ((2, 1), (2, 3), (0, 1), (0, 3))):
        p = call["head_patch"]
        only = torch.zeros(HEADS, dtype=torch.bool)
        only[h] = True
        assert set(call) == INPUTS | {"candidate_ids", "head_patch"} and isinstance(p, HeadPatch) and same_mask(p.rows, rows) and p.layers == (l, l + 1)
        assert torch.equal(p.values, heads[:, l:l + 1]) and p.values.is_contiguous() and torch.equal(p.index, index) and torch.equal(p.heads, only)
    the_trace_block(res, rec, 2, 2)
    # every token by default; an empty sweep
    rec = Recorder(monkeypatch, model, TRACE_SCORE)
    res = eval_utils.head_trace(model, clean=clean, corrupt=dict(kw), layers=[], heads=[0])
    assert len(rec.calls) == 2 and bool(rec.calls[0]["return_heads"].all()) and tuple(res["score"].shape) == (2, 0, 1) and rec.ran_the_front_once(kw["pixel_values"], motion=False)


def test_neuron_trace(monkeypatch):
    model, cfg, kw, seg, clip0 = rig()
    clean, corrupt = two_batches(kw)
    rows = seg["score_row"] | clip0.roll(-1, 1)
    rec = Recorder(monkeypatch, model, TRACE_SCORE)
    res = eval_utils.neuron_trace(model, clean=clean, corrupt=corrupt, layers=(1, 3), top=2, rows=rows, return_logprobs=True)
    assert rec.ran_the_front_once(corrupt["pixel_values"]) and res["layers"] == (1, 3) and res["outs"] == rec.outs and len(rec.calls) == 6
    donor, base = rec.calls[:2]
    assert set(donor) == set(clean) | {"return_neurons", "neuron_layers", "return_logprobs"} and all(donor[k] is clean[k] for k in clean)
    assert set(base) == INPUTS | {"return_neurons", "neuron_layers", "return_logprobs"}
    assert all(same_mask(c["return_neurons"], rows) and c["neuron_layers"] == (1, 3) for c in (donor, base))
    recipient_calls_carry(rec, rec.calls[1:], corrupt, dict(return_logprobs=True))
    neurons, index = rec.outs[0]["neurons"], rec.outs[0]["neurons_index"]
    ranked = eval_utils.rank_neurons(neurons, rec.outs[1]["neurons"], 2)
    assert torch.equal(res["neurons"], ranked) and tuple(ranked.shape) == (2, 2) and ranked[0].tolist() != ranked[1].tolist()
    for i, call in enumerate(rec.calls[2:]):
        w, j = i // 2, int(ranked[i // 2, i % 2])
        p = call["neuron_patch"]
        assert set(call) == INPUTS | {"return_logprobs", "neuron_patch"} and isinstance(p, NeuronPatch) and same_mask(p.rows, rows) and p.layers == (1 + w, 2 + w)
        assert torch.equal(p.values, neurons[:, w:w + 1, j:j + 1]) and p.values.is_contiguous() and torch.equal(p.index, index) and p.neurons.tolist() == [j]
    the_trace_block(res, rec, 2, 2)
    # the score row by default, every layer by default
    rec = Recorder(monkeypatch, model, TRACE_SCORE)
    res = eval_utils.neuron_trace(model, clean=clean, corrupt=dict(kw), top=1)
    assert len(rec.calls) == 2 + LAYERS and same_mask(rec.calls[0]["return_neurons"], seg["score_row"]) and rec.calls[0]["neuron_layers"] == (0, LAYERS)
    assert tuple(res["score"].shape) == (2, LAYERS, 1) and rec.ran_the_front_once(kw["pixel_values"], motion=False)
