"""MLP neuron knock-out and neuron patching without a GPU: the ABI entries, the refusals that come before any launch (native, with fake aligned
addresses; host, as ValueError from a model that lives on the host), the signatures and graph keys that stay as they were, neuron_trace's ranking on
a hand-made capture, and the reference of tests/test_gpu_neuron_patch.py pinned to the existing oracle - no options is
depth_lens_reference.composed_states bit for bit, a self-patch and factors of one are bit-neutral, a layer's MLP scaled by 0 is the layer function
without its MLP term - with the oracle condition: on the rig, each knock-out the GPU file compares moves the oracle's own score by at least twice
that file's score bar."""
import ctypes
import functools
import inspect
import os
import re

import pytest
import torch

import depth_lens_reference as DL
import neuron_patch_reference as NP
from test_key_drop_cpu import bf16_ulps
from test_stream_patch_cpu import host_rig, oracle_rig, same

from aigv_assessor_amd import dist_utils, eval_utils, native, readouts
from aigv_assessor_amd.readouts import NeuronPatch, NeuronScale
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS, INTER = 4, 768
BF = torch.bfloat16
NEW = ("return_neurons", "neuron_layers", "neuron_ids", "neuron_patch", "neuron_scale")

# The knock-outs the GPU file compares with the oracle, clip 0 alone.  ("mlp", layer, factor): every neuron of that layer; ("neuron", layer, rank,
# factor): the neuron of rank `rank` by |activation| at the score row of that layer IN THE ORACLE'S OWN PLAIN PASS (rank 0: the largest);
# ("group", layer, count, factor): the `count` <= 16 largest likewise.  The first is the whole-MLP knock-out of a middle layer; two single neurons
# qualify (layer 2's largest by x 0, and by x -1); the group of 16 of layer 1 is there for a sparse list of more than one column.
KNOCKOUTS = (("mlp", 2, 0.0), ("mlp", 0, 0.0), ("neuron", 2, 0, 0.0), ("mlp", 2, -1.0), ("group", 1, 16, 0.0), ("neuron", 2, 0, -1.0))
TOKEN_CASES = (0, 3, 5)  # the cases whose answer tokens the GPU file compares too
LARGEST_AT_LAYER_2 = 251  # the neuron ("neuron", 2, 0, .) resolves to on the rig


def knockout_options(case, score_row_capture):
    """A case of KNOCKOUTS and the oracle's plain capture of clip 0's score row [1, L, I] -> the reference's keywords (layer_scale | sel, sel_factors)."""
    kind, layer = case[0], case[1]
    if kind == "mlp":
        t = torch.ones(LAYERS)
        t[layer] = case[2]
        return dict(layer_scale=t)
    order = score_row_capture[0, layer].float().abs().sort(descending=True, stable=True).indices
    cols = (order[case[2]:case[2] + 1] if kind == "neuron" else order[:case[2]]).sort().values
    return dict(sel=torch.stack([torch.full_like(cols, layer), cols], 1), sel_factors=torch.full((cols.numel(),), case[3]))


def neuron_scale_of(options):
    """The reference's keywords -> the product's option."""
    return NeuronScale(options["layer_scale"]) if "layer_scale" in options else NeuronScale(options["sel_factors"], options["sel"])


# ---- the ABI entries ----------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_entries():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I, I32P, FP, F = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float), ctypes.c_float
    want = {"aigv_neuron_capture_arm": (I, [P, I32P, I, I, I, I32P, I, P]),
            "aigv_neuron_patch_arm": (I, [P, I32P, I, I, I, I32P, I, P]),
            "aigv_neuron_scale_arm": (I, [P, I32P, I, FP, I32P, I32P, FP, I]),
            "aigv_op_neuron_rows": (I, [P, I, I, I32P, I, P, I32P, P, I, P, I, I, I, I32P, I, P, I, FP, P, F, P])}
    for name, proto in want.items():
        assert name in note and re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == proto, name
    kernels = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    assert "aigv_launch_neuron_rows(" in kernels and re.search(r"#define AIGV_MAX_NEURON_SEL 4096\b", kernels) and readouts.MAX_NEURON_SEL == 4096
    rowops = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "rowops.hip")).read()
    assert "template <int MODE>" in rowops and "neuron_rows_kernel" in rowops                            # the operation is a template parameter


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_native_refusals_without_a_gpu():
    """Every check of the op comes before any HIP call: AIGV_ERR_ARG and a message that starts with the op's name (fake, aligned, non-null device
    addresses: nothing is dereferenced; the host arrays are real, they are read).  The context entry points refuse a null handle."""
    lib = native.load()
    P = 0x10000
    last = lambda: (lib.aigv_last_error(None) or b"").decode()
    good = [0, 3, 9, 99]
    fl = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)
    arr = lambda v: None if v is None else native.i32_array(v)

    def op(act=P, ld=776, T=100, rows=good, n=None, idx=P, sidx=None, sidx_dev=P, n_side=4, side=P, n_layers=3, layer=1, I=768, cols=None, cols_dev=P, mode=0,
           factors=None, factors_dev=P, factor=0.5):
        return lib.aigv_op_neuron_rows(act, ld, T, arr(rows), len(rows or []) if n is None else n, idx, arr(sidx), sidx_dev, n_side, side, n_layers, layer, I, arr(cols),
                                       len(cols or []), cols_dev, mode, fl(factors), factors_dev, factor, None), last()

    cases = ((dict(act=None), "null operand"), (dict(idx=None), "null operand"), (dict(n=-1), "must not be negative"), (dict(ld=760), "leading dimension"),
             (dict(ld=772), "leading dimension"), (dict(I=764, ld=764), "not a positive multiple of 8"), (dict(act=P + 8), "16-byte aligned"),
             (dict(T=-1), "must not be negative"), (dict(mode=3), "mode 3 is none of"), (dict(mode=-1), "mode -1 is none of"),
             (dict(rows=[0, 3, 100]), "row 2 (packed row 100) outside [0, 100)"), (dict(rows=[-1, 3]), "row 0 (packed row -1) outside [0, 100)"),
             (dict(rows=[0, 9, 3]), "not strictly ascending"), (dict(rows=[0, 3, 3]), "not strictly ascending"),
             (dict(cols=[0, 768]), "column 768 (entry 1) outside 0..767"), (dict(cols=[-1, 5]), "column -1 (entry 0) outside 0..767"),
             (dict(cols=[5, 5]), "columns not strictly ascending at entry 1"), (dict(cols=[9, 5]), "columns not strictly ascending at entry 1"),
             (dict(cols=list(range(9)), I=8, ld=8), "9 columns outside 0..I = 8"), (dict(cols=[1, 2], cols_dev=None), "null operand"))
    window = ((dict(side=None), "null operand"), (dict(side=P + 8), "16-byte aligned"), (dict(layer=3), "layer 3 outside the window of 3 layers"),
              (dict(layer=-1), "outside the window"), (dict(n_layers=0, layer=0), "outside the window"),
              (dict(sidx=[0, 1, 2, 4]), "side row 4 (entry 3) outside 0..3"), (dict(sidx=[0, 1, 2, 3], sidx_dev=None), "null operand"))
    scale = ((dict(factor=float("nan")), "the factor is NaN"), (dict(cols=[1, 2], factors=None), "null factor list"),
             (dict(cols=[1, 2], factors=[1.0, float("nan")]), "factor 1 is NaN"))
    for mode in (0, 1, 2):
        for kw, word in cases + (window if mode < 2 else scale):
            kw = dict(dict(mode=mode), **kw)
            if mode == 2 and "cols" in kw and "factors" not in kw:
                kw["factors"] = [0.5] * len(kw["cols"])
            rc, msg = op(**kw)
            assert rc == -1 and word in msg and msg.startswith("aigv_op_neuron_rows:"), (mode, kw, rc, msg)
    rows = native.i32_array(good)
    assert lib.aigv_neuron_capture_arm(None, rows, 4, 0, 1, None, 0, P) == -1 and last().startswith("aigv_neuron_capture_arm: null context")
    assert lib.aigv_neuron_patch_arm(None, rows, 4, 0, 1, None, 0, P) == -1 and last().startswith("aigv_neuron_patch_arm: null context")
    assert lib.aigv_neuron_scale_arm(None, rows, 4, fl([1.0] * 4), None, None, None, 0) == -1 and last().startswith("aigv_neuron_scale_arm: null context")


def test_host_refusals_come_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError.  Every message names its option."""
    model, cfg, kw = host_rig()
    ids, am = kw["input_ids"], kw["attention_mask"]
    seg = model.segment_masks(ids, am, kw["image_flags"])
    mask = seg["score_row"]                                                                   # two tokens, one per clip
    vals = lambda n=2, l=1, w=INTER, dt=BF: torch.zeros(n, l, w, dtype=dt)
    ones = torch.ones(LAYERS)
    pairs = torch.tensor([[2, 5], [0, 9]])

    def bad(word, **opts):
        with pytest.raises(ValueError, match=word):
            model(**kw, **opts)

    # shapes and dtypes
    bad("return_neurons: shape", return_neurons=mask[:, :100])
    bad("return_neurons: expected a bool or integer tensor", return_neurons=mask.float())
    bad("neuron_ids: expected an integer tensor", return_neurons=mask, neuron_ids=torch.tensor([1.0]))
    bad("neuron_ids: expected an integer tensor", return_neurons=mask, neuron_ids=torch.tensor([[1, 2]]))
    bad(f"neuron_ids: neuron numbers outside 0..{INTER - 1}", return_neurons=mask, neuron_ids=torch.tensor([1, INTER]))
    bad("neuron_ids: neuron numbers outside", return_neurons=mask, neuron_ids=torch.tensor([-1, 4]))
    bad("neuron_ids: neuron numbers must be strictly ascending", return_neurons=mask, neuron_ids=torch.tensor([4, 4]))
    bad("neuron_ids: neuron numbers must be strictly ascending", return_neurons=mask, neuron_ids=torch.tensor([9, 4]))
    bad("neuron_patch: rows: shape", neuron_patch=NeuronPatch(mask[:, :100], vals(), (0, 1)))
    bad("neuron_patch: expected a readouts.NeuronPatch", neuron_patch=(mask, vals(), (0, 1)))
    bad("neuron_patch: values must be a bf16 tensor", neuron_patch=NeuronPatch(mask, vals(dt=torch.float32), (0, 1)))
    bad("neuron_patch: values must be a bf16 tensor", neuron_patch=NeuronPatch(mask, vals(l=2), (0, 1)))
    bad("neuron_patch: values must be a bf16 tensor", neuron_patch=NeuronPatch(mask, vals()[0], (0, 1)))
    bad(f"neuron_patch: values must be a bf16 tensor .*I = {INTER}", neuron_patch=NeuronPatch(mask, vals(w=INTER - 8), (0, 1)))
    bad("neuron_patch: values must be a bf16 tensor .*m = 2", neuron_patch=NeuronPatch(mask, vals(w=3), (0, 1), None, torch.tensor([1, 2])))
    bad("neuron_patch: neurons: neuron numbers must be strictly ascending", neuron_patch=NeuronPatch(mask, vals(w=2), (0, 1), None, torch.tensor([2, 1])))
    bad("neuron_patch: index must be an integer tensor", neuron_patch=NeuronPatch(mask, vals(), (0, 1), torch.zeros(2, 3, dtype=torch.long)))
    bad("neuron_scale: expected a readouts.NeuronScale", neuron_scale=ones)
    bad(f"neuron_scale: scale must be a float tensor \\[L = {LAYERS}\\]", neuron_scale=NeuronScale(ones[:3]))
    bad("neuron_scale: scale must be a float tensor", neuron_scale=NeuronScale(ones.long()))
    bad("neuron_scale: scale must be a float tensor \\[m = 2\\]", neuron_scale=NeuronScale(ones, pairs))
    bad("neuron_scale: neurons must be an integer tensor \\[m, 2\\]", neuron_scale=NeuronScale(ones[:2], pairs.float()))
    bad("neuron_scale: neurons must be an integer tensor \\[m, 2\\]", neuron_scale=NeuronScale(ones[:2], pairs[:, 0]))
    bad("neuron_scale: a \\(layer, neuron\\) pair outside", neuron_scale=NeuronScale(ones[:2], torch.tensor([[LAYERS, 0], [0, 0]])))
    bad("neuron_scale: a \\(layer, neuron\\) pair outside", neuron_scale=NeuronScale(ones[:2], torch.tensor([[0, INTER], [0, 0]])))
    bad("neuron_scale: the \\(layer, neuron\\) pairs must be unique", neuron_scale=NeuronScale(ones[:2], torch.tensor([[1, 7], [1, 7]])))
    bad("neuron_scale: rows: shape", neuron_scale=NeuronScale(ones, None, mask[:, :100]))
    nan = ones.clone(); nan[2] = float("nan")
    bad(r"neuron_scale: scale\[2\] is NaN", neuron_scale=NeuronScale(nan))
    bad(r"neuron_scale: scale\[1\] is NaN", neuron_scale=NeuronScale(torch.tensor([0.0, float("nan")]), pairs))
    with pytest.raises(ValueError, match="neuron_ids: 4097 neurons, at most 4096"):
        readouts.neuron_options(return_neurons=mask, neuron_ids=torch.arange(4097))
    with pytest.raises(ValueError, match="neuron_scale: 4097 neurons, at most 4096"):
        readouts.neuron_options(neuron_scale=NeuronScale(torch.zeros(4097), torch.stack([torch.zeros(4097, dtype=torch.long), torch.arange(4097)], 1)))
    # count mismatch: both counts are named
    bad("neuron_patch: values hold 3 rows, the mask selects 2 tokens", neuron_patch=NeuronPatch(mask, vals(n=3), (0, 1)))
    dead = torch.zeros_like(mask); dead[:, 214] = True                                        # the closing token: behind the last consumed row, not run
    bad("neuron_patch: values hold 2 rows, the mask selects 0 tokens", neuron_patch=NeuronPatch(dead, vals(), (0, 1)))
    own = torch.tensor([[0, 211], [1, 211]])
    bad("neuron_patch: index holds 1 pairs, the mask selects 2 tokens", neuron_patch=NeuronPatch(mask, vals(), (0, 1), own[:1]))
    # index mismatch: the first differing pair
    bad(r"neuron_patch: pair 1 of index is \(clip, position\) = \(1, 210\), the pass's is \(1, 211\)",
        neuron_patch=NeuronPatch(mask, vals(), (0, 1), torch.tensor([[0, 211], [1, 210]])))
    # a bad window
    for window in ((2, 1), (-1, 2), (0, LAYERS + 1), (0,), (0, 1, 2), 2, (0.0, 2), (False, True)):
        bad("neuron_layers", return_neurons=mask, neuron_layers=window)
        bad("neuron_patch: layers", neuron_patch=NeuronPatch(mask, vals(), window))
    bad("neuron_layers: qualifies return_neurons", neuron_layers=(0, 2))
    bad("neuron_ids: qualifies return_neurons", neuron_ids=torch.tensor([1]))
    # what passes the host checks: the record carries the options, and forward_kwargs hands them on
    ro = readouts.ReadOuts.parse(cfg.llm_config.vocab_size, kw["labels"], ids_shape=ids.shape, n_layers=LAYERS, return_neurons=mask.long(), neuron_ids=torch.tensor([3, 700]),
                                 neuron_patch=NeuronPatch(mask, vals(l=2, w=2), [1, 3], own, torch.tensor([6, 7], dtype=torch.int32)),
                                 neuron_scale=NeuronScale(torch.tensor([0.5, 0.0], dtype=torch.float64), pairs, mask), n_inter=INTER)
    assert torch.equal(ro.neuron_rows, mask) and ro.neuron_layers == (0, LAYERS) and ro.neuron_ids.tolist() == [3, 700] and ro.touches_stream
    assert ro.neuron_patch.layers == (1, 3) and ro.neuron_patch.neurons.tolist() == [6, 7] and ro.neuron_patch.neurons.dtype == torch.long
    assert ro.neuron_scale.scale.dtype == torch.float32 and torch.equal(ro.neuron_scale.rows, mask)
    assert ro.neuron_scale.neurons.tolist() == [[0, 9], [2, 5]] and ro.neuron_scale.scale.tolist() == [0.0, 0.5]      # sorted by (layer, neuron), the factors with them
    fk = readouts.forward_kwargs(ro)
    assert torch.equal(fk["return_neurons"], mask) and fk["neuron_layers"] == (0, LAYERS) and fk["neuron_ids"] is ro.neuron_ids
    assert fk["neuron_patch"] is ro.neuron_patch and fk["neuron_scale"] is ro.neuron_scale
    assert not set(NEW) & set(readouts.forward_kwargs(readouts.ReadOuts(logprobs=True)))
    fields = [f.name for f in readouts.ReadOuts.__dataclass_fields__.values()]
    at = fields.index("neuron_rows")                                                          # one group, in front of the stream options: the head test pins the record's tail
    assert fields[at:at + 5] == ["neuron_rows", "neuron_layers", "neuron_ids", "neuron_patch", "neuron_scale"] and fields[at - 1] == "depth_lens" and fields[at + 5] == "stream_rows"
    dense = readouts.neuron_options(neuron_scale=NeuronScale(ones.double()), n_layers=LAYERS)[4]
    assert dense.neurons is None and dense.rows is None and dense.scale.dtype == torch.float32
    # against the plan
    plan = model._plan(ids, am, kw["labels"], kw["image_flags"], 4)
    got = model._neuron_patch_plan(plan, ro.neuron_patch)
    assert got[0].tolist() == [int(r) for r in plan["score_rows"]] and got[1:3] == (1, 3) and got[3].tolist() == [6, 7] and got[3].dtype == torch.int32
    assert got[4] is ro.neuron_patch.values
    assert model._neuron_patch_plan(plan, NeuronPatch(mask, vals(), (0, 1)))[3] is None         # dense: no column list
    assert model._neuron_patch_plan(plan, NeuronPatch(mask, vals(l=0), (2, 2))) is None          # an empty window: the plain pass
    assert model._neuron_patch_plan(plan, NeuronPatch(dead, vals(n=0), (0, 1))) is None          # an empty selection likewise
    assert model._neuron_patch_plan(plan, NeuronPatch(mask, vals(w=0), (0, 1), None, torch.zeros(0, dtype=torch.long))) is None   # no neuron likewise


def test_the_other_entry_points_keep_their_signatures():
    model = host_rig()[0]
    for fn in (model.forward_shared_prefix, model.generate, model.generate_stage2, eval_utils.batched, dist_utils.score_clips_dp):
        assert not set(NEW) & set(inspect.signature(fn).parameters), fn
    assert set(NEW) <= set(inspect.signature(model.forward).parameters)
    front = {"pixel_values", "input_ids", "attention_mask", "image_flags"}
    sig = inspect.signature(eval_utils.mlp_knockout).parameters
    assert [sig[k].default for k in ("labels", "layers", "rows")] == [None] * 3 and front <= set(sig)
    sig = inspect.signature(eval_utils.neuron_knockout).parameters
    assert list(sig)[:2] == ["model", "neurons"] and [sig[k].default for k in ("labels", "rows")] == [None] * 2 and front <= set(sig)
    sig = inspect.signature(eval_utils.neuron_trace).parameters
    assert [sig[k].default for k in ("layers", "top", "rows")] == [None, 16, None] and {"clean", "corrupt"} <= set(sig)


def test_the_sweeps_apply_their_input_checks():
    model, cfg, kw = host_rig()
    for change, word in ((dict(input_ids=kw["input_ids"][:, :200]), "one token layout"),
                         (dict(attention_mask=kw["attention_mask"] & (torch.arange(215) < 214)), "attention_mask differ"),
                         (dict(pixel_values=kw["pixel_values"][:3]), "pixel_values of shape")):
        with pytest.raises(ValueError, match="neuron_trace: .*" + word):
            eval_utils.neuron_trace(model, clean=dict(kw), corrupt=dict(kw, **change))
    for bad in (dict(layers=(0, LAYERS + 1)), dict(layers=(3, 2)), dict(top=0), dict(top=INTER + 1)):
        with pytest.raises(ValueError, match="neuron_trace: layers"):
            eval_utils.neuron_trace(model, clean=dict(kw), corrupt=dict(kw), **bad)
    with pytest.raises(ValueError, match="neuron_trace: rows has shape"):
        eval_utils.neuron_trace(model, clean=dict(kw), corrupt=dict(kw), rows=torch.zeros(2, 100, dtype=torch.bool))
    front = {k: v for k, v in kw.items() if k != "motion_feature"}
    with pytest.raises(ValueError, match="mlp_knockout: layers"):
        eval_utils.mlp_knockout(model, **front, layers=[LAYERS])
    for neurons, word in (([[LAYERS, 0]], "pair outside"), ([[0, INTER]], "pair outside"), ([[0, -1]], "pair outside"), ([1, 2], "must be an integer tensor"),
                          ([[0.5, 1.0]], "must be an integer tensor")):
        with pytest.raises(ValueError, match="neuron_knockout: .*" + word):
            eval_utils.neuron_knockout(model, neurons, **front)


def test_rank_neurons_on_a_hand_made_capture():
    """[n = 3 rows, W = 2 layers, I = 6]: per layer the largest summed |clean - corrupt| first, in fp32 (a difference bf16 would round away still
    ranks), equals by the lower neuron number, a NaN difference counted as 0."""
    clean = torch.zeros(3, 2, 6, dtype=BF)
    corrupt = torch.zeros(3, 2, 6, dtype=BF)
    # layer 0: neuron 4 differs by 1 + 2 + 0.5 = 3.5, neuron 1 by 3 in one row, neuron 5 by -2 and +1 (absolute values: 3), neuron 0 by 0.25
    clean[:, 0, 4] = torch.tensor([1.0, 2.0, 0.5]).to(BF)
    corrupt[0, 0, 1] = 3.0
    clean[0, 0, 5], corrupt[1, 0, 5] = -2.0, 1.0
    clean[2, 0, 0] = 0.25
    # layer 1: 256 + 1 against 256: the sums 257 and 256 differ in fp32 and tie in bf16; neuron 3 is NaN in one row and 255 in another
    clean[0, 1, 2], clean[1, 1, 2] = 256.0, 1.0
    corrupt[0, 1, 0] = 256.0
    clean[0, 1, 3], clean[1, 1, 3] = float("nan"), 255.0
    got = eval_utils.rank_neurons(clean, corrupt, 4)
    assert got.dtype == torch.long and got.tolist() == [[4, 1, 5, 0], [2, 0, 3, 1]]
    assert eval_utils.rank_neurons(clean, corrupt, 1).tolist() == [[4], [2]]
    assert eval_utils.rank_neurons(clean, clean, 3)[0].tolist() == [0, 1, 2]                    # all equal: the lower numbers


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
        assert ro.neuron_rows is None and ro.neuron_layers is None and ro.neuron_ids is None and ro.neuron_patch is None and ro.neuron_scale is None
        for opt in (dict(return_neurons=mask), dict(neuron_patch=NeuronPatch(mask, torch.zeros(0, 1, INTER, dtype=BF), (0, 1))), dict(neuron_scale=NeuronScale(torch.ones(LAYERS))),
                    dict(neuron_scale=NeuronScale(torch.zeros(1), torch.tensor([[1, 2]])))):
            armed = readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=LAYERS, n_inter=INTER, **opt, **kw)
            assert armed.key_tail(shape) == tail and armed.touches_stream, (kw, opt)                # nothing joins the key: such a call is never captured


# ---- the composed reference, pinned to the existing oracle ----------------------------------------------------------------------------
def test_reference_without_options_self_patch_and_factors_of_one_are_the_composed_states():
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[1]
    am = one["attention_mask"]
    every = torch.ones_like(am)
    got, cap = NP.composed_states(sd, cfg, **inputs)
    assert cap is None and len(got) == LAYERS + 1 and all(same(g, p) for g, p in zip(got, plain)) and O.LLM_LINEAR_HOOK is None
    got, cap = NP.composed_states(sd, cfg, **inputs, capture=(every, (0, LAYERS), None))
    assert tuple(cap.shape) == (215, LAYERS, INTER) and all(same(g, p) for g, p in zip(got, plain)) and O.LLM_LINEAR_HOOK is None
    cols = torch.tensor([0, 6, 7, 300, INTER - 1])
    _, sparse = NP.composed_states(sd, cfg, **inputs, capture=(every, (1, 3), cols))
    assert same(sparse, cap[:, 1:3][:, :, cols])                                              # the sparse capture: those columns of the dense one
    seg = model.segment_masks(one["input_ids"], am, one["image_flags"])
    for mask, layers, neurons in ((every, (0, LAYERS), None), (seg["frames"], (1, 3), cols), (seg["score_row"], (3, 4), None)):
        own = mask[0, :215].nonzero().flatten()
        values = cap[own][:, layers[0]:layers[1]]
        values = values if neurons is None else values[:, :, neurons]
        got, again = NP.composed_states(sd, cfg, **inputs, patches=[(mask, values, layers, neurons)], capture=(mask, layers, neurons))
        assert all(same(g, p) for g, p in zip(got, plain)) and same(again, values), layers
    got, _ = NP.composed_states(sd, cfg, **inputs, layer_scale=torch.ones(LAYERS), sel=torch.tensor([[1, 5]]), sel_factors=torch.ones(1))
    assert all(same(g, p) for g, p in zip(got, plain))
    zero = torch.ones(LAYERS); zero[1] = 0.0
    got, _ = NP.composed_states(sd, cfg, **inputs, layer_scale=zero, scale_rows=torch.zeros_like(am))      # no row: no change
    assert all(same(g, p) for g, p in zip(got, plain))
    # scale, patch, capture on one neuron: the capture returns the patch's value, its neighbours the scaled ones
    noise = torch.full((215, 1, 1), 3.0, dtype=BF)
    got, back = NP.composed_states(sd, cfg, **inputs, sel=torch.tensor([[1, 6], [1, 7]]), sel_factors=torch.tensor([0.0, -1.0]), patches=[(every, noise, (1, 2), torch.tensor([6]))],
                                   capture=(every, (1, 2), torch.tensor([5, 6, 7])))
    assert same(back[:, 0, 0], cap[:, 1, 5]) and same(back[:, 0, 1], noise[:, 0, 0]) and same(back[:, 0, 2], -cap[:, 1, 7])
    assert not same(got[2], plain[2]) and same(got[1], plain[1])


def test_reference_a_layers_mlp_scaled_by_0_is_the_layer_without_its_mlp_term():
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[1]
    mask = O.additive_mask(one["attention_mask"], 215, 0, plain[0].dtype)
    pos = torch.arange(215, dtype=torch.long).unsqueeze(0)
    for l in (0, 2, 3):
        t = torch.ones(LAYERS); t[l] = 0.0
        got, cap = NP.composed_states(sd, cfg, **inputs, layer_scale=t, capture=(torch.ones_like(one["attention_mask"]), (l, l + 1), None))
        assert not cap.any()
        x = plain[l]
        a, _ = O.llm_attention(sd, cfg, l, O.rms_norm_cast_then_scale(x, sd[f"language_model.model.layers.{l}.attention_norm.weight"], cfg.llm_config.rms_norm_eps), mask, pos)
        want = x + a
        want = want + torch.zeros_like(want)                                                  # w2 of a zero row
        assert same(got[l + 1], want) and not same(got[l + 1], plain[l + 1]), l
        assert all(same(got[d], plain[d]) for d in range(l + 1))


@functools.lru_cache(maxsize=None)
def oracle_score_row_capture():
    """The oracle's plain capture of clip 0's score row, every layer: [1, L, I]."""
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[0]
    seg = model.segment_masks(one["input_ids"], one["attention_mask"], one["image_flags"])
    return NP.composed_states(sd, cfg, **inputs, capture=(seg["score_row"], (0, LAYERS), None))[1]


def knockout_case(case):
    """-> (the oracle's plain score of clip 0 alone, its score under the knock-out, its near-tie answer rows, its answer rows)."""
    model, cfg, sd, clips = oracle_rig()
    one, inputs, plain = clips[0]
    am = one["attention_mask"]
    score = lambda states: float(DL.lens(sd, cfg, states, am, one["labels"], 2)["score"][0, LAYERS])
    states, _ = NP.composed_states(sd, cfg, **inputs, **knockout_options(case, oracle_score_row_capture()))
    w, eps = sd["language_model.model.norm.weight"], cfg.llm_config.rms_norm_eps
    logits = O.lm_logits(sd, O.rms_norm_cast_then_scale(states[LAYERS], w, eps))[0, :-1]
    want = one["labels"][0, 1:] != -100
    top = logits[want].float().topk(2, -1).values
    ulp = torch.exp2(top[:, 0].abs().clamp_min(1e-30).log2().floor() - 7)
    ties = int(((top[:, 0] - top[:, 1]) <= 2 * ulp).sum())
    return score(plain), score(states), ties, int(want.sum())


@pytest.mark.parametrize("case", range(len(KNOCKOUTS)), ids=["-".join(str(v) for v in c) for c in KNOCKOUTS])
def test_oracle_condition_each_knockout_moves_the_oracle(case):
    """The rig of tests/test_stream_patch_cpu.py::oracle_rig (weights seed 63, tokens seed 302, 4 layers, I = 768), clip 0 alone in bf16, plain score
    0.48047; the GPU file's score bar is 1e-3 or 1 bf16 ulp of the oracle's value - 1 ulp = 1.95e-3 here.  Measured on a host (with 1, 2, 4 and 8
    threads alike): layer 2's MLP x 0 gives 0.48438 (2 bf16 ulps from plain, 1 near-tie answer row of 10); layer 0's MLP x 0 0.49023 (5, 3);
    layer 2's largest neuron at the score row (number 251, |activation| 0.957) x 0 0.48438 (2, 2); layer 2's MLP x -1 0.49219 (6, 1); the 16
    largest of layer 1 x 0 0.48438 (2, 3); neuron 251 of layer 2 x -1 0.48633 (3, 0).  Single neurons: of the two largest of every layer only layer 2's largest moves the oracle by 2 ulps when knocked out
    (the others: 0 or 1) - hence the group of 16.  Each case must move the oracle's own score by at least 2 ulps - twice the GPU file's bar, so an
    inert kernel cannot pass there; the cases whose tokens the GPU file compares (TOKEN_CASES, at most one row in ten excused) must have at most 1
    near-tie answer row - one whose top two oracle logits lie within 2 bf16 ulps - in the oracle itself."""
    plain, knocked, ties, rows = knockout_case(KNOCKOUTS[case])
    print(f"{KNOCKOUTS[case]}: oracle {knocked:.5f}, plain {plain:.5f} = {bf16_ulps(knocked, plain):.1f} bf16 ulps; {ties} near-tie answer rows of {rows}")
    assert bf16_ulps(knocked, plain) >= 2 and abs(knocked - plain) >= 2 * max(1e-3, 2.0 ** -9)
    if case in TOKEN_CASES:
        assert ties <= 1 and rows == 10


def test_oracle_condition_the_single_neuron_is_the_largest_at_the_score_row():
    cap = oracle_score_row_capture()
    assert int(cap[0, 2].float().abs().argmax()) == LARGEST_AT_LAYER_2
    opt = knockout_options(("neuron", 2, 0, 0.0), cap)
    assert opt["sel"].tolist() == [[2, LARGEST_AT_LAYER_2]] and opt["sel_factors"].tolist() == [0.0]
    grp = knockout_options(("group", 1, 16, 0.0), cap)
    assert tuple(grp["sel"].shape) == (16, 2) and bool((grp["sel"][1:, 1] > grp["sel"][:-1, 1]).all()) and not grp["sel_factors"].any()
