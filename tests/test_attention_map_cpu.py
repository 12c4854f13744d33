"""The attention flow map without a GPU: the ABI entries and their host refusals, the options' parsing and refusals before any launch,
``eval_utils.flow_segments``, ``segment_flow`` and ``attention_rollout`` on hand-made tensors, and the consistency of the references
tests/test_gpu_attention_map.py measures the kernels with (tests/attention_map_reference.py): every row's bins and dropped mass sum to 1, the
all-rows truth is ``score_attention_reference``'s row by row, the census IS the truth within 2^-24, and the fold's fp32 chain lies within its
stated distance of the float64 mean."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import attention_map_reference as M
import score_attention_reference as R
from test_stream_patch_cpu import host_rig

from aigv_assessor_amd import build, dist_utils, eval_utils, native, prompts, readouts
from aigv_assessor_amd.modeling import InternVLChatModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, D, HK = R.S, R.D, R.N_KV
NAMES = ("aigv_attention_map_arm", "aigv_op_attention_map")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_header_prototypes_exports_and_host_refusals():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    note = header[header.index("#define AIGV_ABI_VERSION"):header.index("added symbols only")]
    P, I, I32P = native._P, native._I, native._I32P
    assert native.PROTOTYPES["aigv_attention_map_arm"] == (I, [P, P, I, P, P, P, I, I])
    assert native.PROTOTYPES["aigv_op_attention_map"] == (I, [P, I, P, I, I32P, I, I, I, I, I, I, P, P, I, P, I, P, P, P])
    assert "attnmap.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "attnmap.hip"))
    lib = native.load()
    for name in NAMES:
        assert name in note and hasattr(lib, name), name
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(native.PROTOTYPES[name][1]), name
    doc = header[header.index("Attention flow map: where EVERY query row"):header.index("int aigv_attention_map_arm")]
    for phrase in ("ALWAYS fp32", "one fp32 division", "no atomics", "does not know the mask", "keep_kv", "NaN where clip b has no row"):
        assert phrase in doc, phrase
    kernel = open(os.path.join(build.CSRC, "attnmap.hip")).read()
    tiles = open(os.path.join(build.CSRC, "qk_tiles.h")).read()                                             # the score tiles' product: shared with vitmap.hip
    assert '#include "qk_tiles.h"' in kernel and "qk_tiles.h" in build.HEADERS and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in tiles
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in kernel and "atomic" not in kernel.split('#include "kernels.h"')[1] and "atomic" not in tiles.split("#pragma once")[1]
    # host refusals: before any pointer is used (a small aligned HOST buffer stands for every operand; no accepted call is made)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    p += 16 - p % 16
    last = lambda: (lib.aigv_last_error(None) or b"").decode()

    def call(q=p, ldq=3 * 128, k=p, ldk=3 * 128, cu=(0, 4), n_heads=1, n_kv=1, qgs=3 * 128, khs=3 * 128, d=128, cos=p, max_pos=8, seg=p, n_seg=3, rows=p):
        return lib.aigv_op_attention_map(q, ldq, k, ldk, native.i32_array(list(cu)), len(cu) - 1, n_heads, n_kv, qgs, khs, d, cos, p, max_pos, seg, n_seg, rows, None, None)

    for kw, word in ((dict(q=None), "null operand"), (dict(seg=None), "null operand"), (dict(rows=None), "null operand"), (dict(d=96), "head_dim must be 64 or 128"),
                     (dict(n_seg=0), "segments"), (dict(n_seg=65), "segments"), (dict(k=p + 8), "16-byte aligned"), (dict(q=p + 8), "16-byte aligned"),
                     (dict(ldk=3 * 128 + 4), "multiples of 8"), (dict(ldq=64), "q strides too small"), (dict(khs=64), "K strides too small"), (dict(cos=p + 2), "RoPE tables"),
                     (dict(n_heads=3, n_kv=2), "multiple of n_kv_heads"), (dict(cu=(0, 4, 4)), "empty sequence"), (dict(cu=(1, 4)), "cu[0]"), (dict(cu=(0, 9)), "longer than the RoPE table"),
                     (dict(max_pos=0), "max_pos"), (dict(cu=tuple(range(129))), "sequences")):
        rc = call(**kw)
        assert rc == -1 and word in last() and "aigv_op_attention_map" in last(), (kw, rc, last())
    assert lib.aigv_attention_map_arm(None, p, 3, p, p, None, 0, 0) == -1 and "null context" in last()


# ---- the options ----------------------------------------------------------------------------------------------------------------------------------
def test_option_parsing_record_and_graph_key():
    V, shape = 1000, (2, 215)
    ro = readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=4, return_segment_attention=True)
    assert ro.attention_map == readouts.AttentionMap(True, None) and ro.runs_eagerly and not ro.touches_stream and not ro.score_attention
    assert ro.key_tail(shape) == () and readouts.forward_kwargs(ro) == dict(return_segment_attention=True)
    rows = readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=4, return_row_attention=[1, 3])
    assert rows.attention_map == readouts.AttentionMap(False, (1, 3)) and rows.runs_eagerly and readouts.forward_kwargs(rows) == dict(return_row_attention=(1, 3))
    table = torch.zeros(shape, dtype=torch.long)
    both = readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=4, return_segment_attention=True, return_row_attention=(0, 4), attention_segments=table,
                                   return_score_attention=True, return_logprobs=True)
    assert both.segments is table and both.score_attention and both.key_tail(shape) == ("logprobs", ("score_attention", 1))      # nothing added to the key
    assert set(readouts.forward_kwargs(both)) == {"return_logprobs", "return_score_attention", "attention_segments", "return_segment_attention", "return_row_attention"}
    alone = readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_segment_attention=True, attention_segments=table)
    assert alone.segments is table and alone.map_segments(shape, 0) == 1                                                          # the table travels without the probe too
    # a call without the options: the record, the key and the keywords it always had
    new = {"return_segment_attention", "return_row_attention"}
    for kw in (dict(), dict(return_logprobs=True), dict(return_score_attention=True), dict(return_depth_lens=True)):
        r = readouts.ReadOuts.parse(V, "given", ids_shape=shape, **kw)
        assert r.attention_map is None and not r.runs_eagerly and not new & set(readouts.forward_kwargs(r)), kw
    assert readouts.ReadOuts().attention_map is None and readouts.ReadOuts(logprobs=True).attention_map is None
    assert "attention_map" not in readouts.ReadOuts.__dataclass_fields__                 # (the field list is pinned from both ends by other tests: a plain attribute)
    # refusals that need no plan
    for window, word in (((3, 2), r"\(3, 2\) outside 0 <= lo <= hi <= 4"), ((0, 5), "outside 0 <= lo <= hi <= 4"), ((-1, 2), "outside"), ((0,), "pair of ints"), ((0, True), "pair of ints"),
                         (2, "pair of ints")):
        with pytest.raises(ValueError, match="return_row_attention: .*" + word):
            readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=4, return_row_attention=window)
    drop = torch.zeros(shape, dtype=torch.bool)
    for kw in (dict(return_segment_attention=True), dict(return_row_attention=(0, 1))):
        with pytest.raises(ValueError, match="key_drop: cannot be combined with return_segment_attention / return_row_attention .*does not know the mask"):
            readouts.ReadOuts.parse(V, "given", ids_shape=shape, n_layers=4, key_drop=drop, **kw)
    with pytest.raises(ValueError, match="65 segments, outside 1..64"):
        readouts.ReadOuts.parse(V, "given", ids_shape=shape, return_segment_attention=True, attention_segments=torch.full(shape, 64)).map_segments(shape, 0)
    with pytest.raises(ValueError, match="65 segments"):
        ro.map_segments(shape, 65)                                                       # the default table of a clip with 61 frames


def test_clip_limit_and_the_copy_that_keeps_the_map():
    """More than 127 clips - the kernels' sequence table - is a ValueError from ``parse``, before any plan or launch, for either option and for
    neither without them; ``ReadOuts.with_`` is ``dataclasses.replace`` that keeps ``attention_map`` (which is no field, so ``replace`` drops it)."""
    import dataclasses
    V = 1000
    for kw in (dict(return_segment_attention=True), dict(return_row_attention=(0, 1))):
        with pytest.raises(ValueError, match="at most 127 clips per pass, got 128"):
            readouts.ReadOuts.parse(V, "given", ids_shape=(128, 215), n_layers=4, **kw)
        assert readouts.ReadOuts.parse(V, "given", ids_shape=(127, 215), n_layers=4, **kw).attention_map is not None
    assert readouts.ReadOuts.parse(V, "given", ids_shape=(128, 215), n_layers=4, return_logprobs=True).attention_map is None
    assert readouts.MAX_MAP_CLIPS == 127
    ro = readouts.ReadOuts.parse(V, "given", ids_shape=(2, 215), n_layers=4, return_segment_attention=True, return_row_attention=(1, 2), return_logprobs=True)
    table = torch.zeros(2, 215, dtype=torch.long)
    copy = ro.with_(segments=table)
    assert copy is not ro and copy.attention_map == ro.attention_map == readouts.AttentionMap(True, (1, 2)) and copy.segments is table and copy.logprobs and copy.runs_eagerly
    assert dataclasses.replace(ro, segments=table).attention_map is None                  # what with_ is there for
    plain = readouts.ReadOuts(logprobs=True).with_(topk=3)
    assert plain.attention_map is None and plain.topk == 3 and plain.logprobs
    graphs = open(os.path.join(ROOT, "aigv-assessor_amd", "graphs.py")).read()
    assert "ro.with_(" in graphs and "replace(ro" not in graphs


def test_python_surface_and_refusals_before_any_launch():
    """The model lives on the host: anything that reached a launch would raise NativeError, not ValueError."""
    params = inspect.signature(InternVLChatModel.forward).parameters
    assert params["return_segment_attention"].default is False and params["return_row_attention"].default is None
    for fn in (InternVLChatModel.forward_shared_prefix, InternVLChatModel.generate, InternVLChatModel.generate_stage2, eval_utils.batched, dist_utils.score_clips_dp):
        assert not {"return_segment_attention", "return_row_attention"} & set(inspect.signature(fn).parameters), fn
    assert list(inspect.signature(eval_utils.flow_segments).parameters) == ["model", "input_ids", "attention_mask", "image_flags"]
    assert list(inspect.signature(eval_utils.segment_flow).parameters) == ["seg_att", "layers", "heads"]
    assert list(inspect.signature(eval_utils.attention_rollout).parameters) == ["seg_att", "alpha", "layers"] and inspect.signature(eval_utils.attention_rollout).parameters["alpha"].default == 0.5
    model, cfg, kw = host_rig()
    L = cfg.llm_config.num_hidden_layers
    drop = torch.zeros_like(kw["input_ids"], dtype=torch.bool)
    drop[:, 20] = True
    for opts, word in ((dict(return_segment_attention=True, key_drop=drop), "does not know the mask"), (dict(return_row_attention=(0, 1), key_drop=drop), "does not know the mask"),
                       (dict(return_row_attention=(0, L + 1)), f"outside 0 <= lo <= hi <= {L}"), (dict(return_row_attention=(2, 1)), "outside 0 <= lo <= hi"),
                       (dict(return_segment_attention=True, attention_segments=torch.full_like(kw["input_ids"], 64)), "65 segments, outside 1..64"),
                       (dict(return_row_attention=(0, 1), attention_segments=torch.zeros(2, 3, dtype=torch.long)), "attention_segments: expected an integer tensor shaped like input_ids")):
        with pytest.raises(ValueError, match=word):
            model(**kw, **opts)
    with pytest.raises(TypeError):
        model.forward_shared_prefix([], return_segment_attention=True)


# ---- flow_segments --------------------------------------------------------------------------------------------------------------------------------
def test_flow_segments_is_the_default_table_with_the_score_row_apart():
    model, cfg, kw = host_rig()
    ids, am, flags = kw["input_ids"], kw["attention_mask"], kw["image_flags"]
    table = eval_utils.flow_segments(model, ids, am, flags)
    assert table.dtype == torch.long and tuple(table.shape) == tuple(ids.shape)
    F = 2
    assert int(table.max()) + 1 == F + prompts.N_TEXT_SEGMENTS + 1 and int(table.min()) >= 0        # S = F + 5; both clips fill the whole width
    groups, units = model.segment_masks(ids, am, flags), model.unit_masks(ids, am, flags)
    assert (table == F + 4).sum(1).tolist() == [1, 1] and torch.equal(table == F + 4, groups["score_row"])
    for u in range(F + 1):
        assert torch.equal(table == u, units[:, u])
    assert torch.equal(table == F + 1, groups["first"]) and torch.equal(table == F + 2, groups["text_before"])
    assert torch.equal((table == F + 3) | (table == F + 4), groups["text_after"])
    # the packed default table, apart from the score row, is what the probe bins by
    plan = model._plan(ids, am, kw["labels"], flags, 4)
    seg, S = model._default_segments(plan)
    packed = table[plan["row_of"] >= 0]
    assert S == F + 4 and torch.equal(torch.where(packed == F + 4, torch.full_like(packed, F + 3), packed), seg.long())
    # padding: a clip cut short is -1 behind its end
    am2 = am.clone()
    am2[1, -7:] = False
    short = eval_utils.flow_segments(model, ids, am2, flags)
    assert (short[1, -7:] == -1).all() and (short[0] >= 0).all()


# ---- segment_flow, attention_rollout ------------------------------------------------------------------------------------------------------------
def test_segment_flow_and_rollout_on_hand_made_tensors():
    B, L, nh, Sg = 2, 3, 4, 5
    gen = torch.Generator().manual_seed(3)
    att = torch.softmax(torch.randn(B, L, nh, Sg, Sg, generator=gen), -1)
    flow = eval_utils.segment_flow(att)
    assert tuple(flow.shape) == (B, Sg, Sg) and torch.allclose(flow, att.double().mean((1, 2)).float(), atol=0, rtol=0)
    assert torch.equal(eval_utils.segment_flow(att, layers=[1], heads=[2]), att[:, 1, 2])
    assert torch.allclose(eval_utils.segment_flow(att, layers=[0, 2]), att[:, [0, 2]].double().mean((1, 2)).float(), atol=0, rtol=0)
    for bad in (dict(layers=[3]), dict(heads=[-1]), dict(layers=[])):
        with pytest.raises(ValueError, match="segment_flow"):
            eval_utils.segment_flow(att, **bad)
    with pytest.raises(ValueError, match=r"expected \[B, L, n_heads, S, S\]"):
        eval_utils.segment_flow(att[..., :4])
    eye = torch.eye(Sg)
    # alpha = 1: only the residual path - I, exactly
    assert torch.equal(eval_utils.attention_rollout(att, alpha=1.0), eye.expand(B, Sg, Sg))
    # permutation matrices, alpha = 0: the product, deepest layer leftmost, exactly
    perms = [torch.randperm(Sg, generator=gen) for _ in range(L)]
    P = torch.stack([eye[p] for p in perms])                                              # [L, S, S]
    pa = P[None, :, None].expand(B, L, nh, Sg, Sg).contiguous()
    want = P[2] @ P[1] @ P[0]
    assert torch.equal(eval_utils.attention_rollout(pa, alpha=0.0), want.expand(B, Sg, Sg))
    assert torch.equal(eval_utils.attention_rollout(pa, alpha=0.0, layers=[0, 2]), (P[2] @ P[0]).expand(B, Sg, Sg))
    # against the definition, float64
    a = 0.3
    step = a * eye.double() + (1 - a) * att.double().mean(2)
    ref = step[:, 2] @ step[:, 1] @ step[:, 0]
    got = eval_utils.attention_rollout(att, alpha=a)
    assert torch.allclose(got.double(), ref, rtol=0, atol=2.0 ** -23) and torch.allclose(got.double().sum(-1), torch.ones(B, Sg, dtype=torch.float64), atol=1e-6)
    # an empty segment (NaN row in every layer and head): the identity's row - and nothing leaks into the other rows
    holed = att.clone()
    holed[0, :, :, 1] = float("nan")
    out = eval_utils.attention_rollout(holed, alpha=a)
    assert torch.equal(out[0, 1], eye[1]) and torch.isfinite(out).all() and torch.equal(out[1], got[1])
    assert torch.isnan(eval_utils.segment_flow(holed)[0, 1]).all() and torch.isfinite(eval_utils.segment_flow(holed)[0, 0]).all()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="alpha"):
            eval_utils.attention_rollout(att, alpha=bad)


# ---- the references' own consistency ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_all_rows_truth_sums_to_one_and_is_the_probe_reference_row_by_row(g):
    c = R.RandomCase(g)
    q_rot = R.rotate_q(c.q, c.pos, c.cos, c.sin)
    mass, dropped, eps = M.rows_truth(q_rot, c.k, c.seg, R.LENS, S)
    assert tuple(mass.shape) == (c.T, HK * g, S) and (mass >= 0).all()
    assert (mass.sum(-1) + dropped - 1).abs().max().item() <= 2.0 ** -48                 # float64: every row's bins and dropped mass sum to 1
    assert dropped.max().item() > 0.1                                                    # (the table does drop keys)
    bound = M.rows_bound(mass, eps, R.LENS, S)
    for t, (want, want_bound) in c.truth(q_rot).items():                                 # score_attention_reference's own rows
        assert (mass[t] - want).abs().max().item() <= 2.0 ** -48, t
        qr = q_rot[t].reshape(HK * g, D)
        b = max(i for i in range(len(R.LENS)) if c.cu[i] <= t)
        assert torch.allclose(eps[t], R.score_bound(qr, c.k[c.cu[b]:t + 1]), rtol=1e-12, atol=0)
        assert (bound[t] >= want_bound).all() and (bound[t] <= 2.5 * want_bound).all()   # eps doubled: wider than the probe's, by about the factor
    assert M.key_counts(R.LENS).tolist() == [1] + list(range(1, 259)) + list(range(1, 514))


@pytest.mark.parametrize("n_seg", [S, 33, 64])
def test_census_is_the_truth_within_one_rounding(n_seg):
    """Q = 0: every visible key weighs exactly 1, so the float64 truth is count / n; the census is its ONE fp32 rounding - and the probe
    reference's census at its rows."""
    seg = R.seg_table(R.LENS, n_seg)
    got = M.census(seg, R.LENS, n_seg)
    q = torch.zeros(sum(R.LENS), HK, 1, D, dtype=R.BF)
    k = torch.randn(sum(R.LENS), HK, D, generator=torch.Generator().manual_seed(1)).to(R.BF)
    mass, dropped, eps = M.rows_truth(q, k, seg, R.LENS, n_seg)
    assert eps.abs().max().item() == 0 and (got.double()[:, None] - mass).abs().max().item() <= 2.0 ** -24
    assert (got.double().sum(-1) + dropped[:, 0] - 1).abs().max().item() <= n_seg * 2.0 ** -24
    for t, want in R.census_expect(R.LENS, n_seg, seg).items():
        assert torch.equal(got[t], want), t
    counts = M.segment_rows(seg, R.LENS, n_seg)
    assert counts.sum(1).tolist() == [int(((seg[a:b] >= 0) & (seg[a:b] < n_seg)).sum()) for a, b in zip(R.cu_of(R.LENS)[:-1], R.cu_of(R.LENS)[1:])]


def test_fold_chain_against_the_float64_mean():
    """The documented fp32 chain (ascending rows, one division) lies within n 2^-24 relative of the float64 mean of non-negative rows (n roundings: n - 1 additions - 0 + x is exact - and the division); an empty
    segment is NaN in both; an exactly representable case is exact."""
    c = R.RandomCase(3)
    mass, _, _ = M.rows_truth(R.rotate_q(c.q, c.pos, c.cos, c.sin), c.k, c.seg, R.LENS, S)
    rows = mass.float()
    chain, truth = M.fold_chain(rows, c.seg, R.LENS, S), M.fold_truth(rows, c.seg, R.LENS, S)
    counts = M.segment_rows(c.seg, R.LENS, S)
    empty = (counts == 0)[:, None, :, None].expand_as(chain)
    assert empty.any() and torch.isnan(chain[empty]).all() and torch.isnan(truth[empty]).all() and torch.isfinite(chain[~empty]).all()
    tol = counts.double()[:, None, :, None] * 2.0 ** -24 * truth
    assert ((chain.double() - truth).abs()[~empty] <= tol[~empty]).all()
    ones = torch.full((sum(R.LENS), 2, S), 0.25)
    assert torch.equal(M.fold_chain(ones, c.seg, R.LENS, S)[~empty[:, :2]], torch.full_like(ones[0, 0, 0], 0.25).expand(int((~empty[:, :2]).sum())))
