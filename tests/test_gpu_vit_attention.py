"""InternViT attention map on the MI355X.  Op level (aigv_op_vit_attention_map, no model) on the shapes of
tests/vit_attention_reference.py: key census and one-hot selector (bit-exact), random data against float64 within the derived bound, a
frame alone against the same frame in the pack, the head mean against the documented chain over the per-head output, output fencing and
refusals.  Model level (``model.vit_attention``; tiny towers at 224 x 224, S = 257, LayerNorm without QK-norm and RMSNorm with it): the armed
pass changes no other bit, windows, ``select_layer``, a frame alone across a ``vit_chunk`` boundary (65 frames), the exact census through the
model, the CPU oracle's eager probabilities, and the rollout-to-pixels invariant.  tests/test_vit_attention_cpu.py holds, without a GPU, the
references' own consistency."""
import copy
import ctypes
import functools

import pytest
import torch

import aigv_assessor_amd as pkg
import vit_attention_reference as V
from aigv_assessor_amd import eval_utils, native, synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 0x7FA5A5A5      # a NaN bit pattern the kernels cannot produce
PAD = 64                   # floats in front of and behind every output
IDS = [f"{n}x{S}x{H}x{D}" for n, S, H, D in V.SHAPES]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


def bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a.detach().cpu().reshape(-1).view(torch.uint8), b.detach().cpu().reshape(-1).view(torch.uint8))


def fenced(n):
    whole = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, ctypes.c_void_p(whole.data_ptr() + 4 * PAD)


def unfenced(whole, n, what, written=True):
    w = whole.cpu()
    assert (w[:PAD] == SENTINEL).all() and (w[PAD + n:] == SENTINEL).all(), f"the map wrote outside {what}"
    if written:
        assert (w[PAD:PAD + n] != SENTINEL).all(), f"the map left part of {what} unwritten"
    else:
        assert (w[PAD:PAD + n] == SENTINEL).all(), f"a refused call wrote to {what}"
    return w[PAD:PAD + n].view(torch.float32).clone()


def vmap(lib, fused_d, shape, per_head, refused=None, **over):
    """aigv_op_vit_attention_map on fused rows [n_seq S, 3 H D] (Q | K | V thirds).  The output and the stats scratch each sit between two
    sentinel pads inside an allocation that starts as the sentinel: returns fp32 [n_seq, (H,) S, S] after checking that the pads kept their
    bits and that every element was written.  refused: the call must fail with that word in its message and write nothing; over: arguments
    replaced for such a call."""
    n, S, H, D = shape
    n_out, n_stats = n * (H if per_head else 1) * S * S, 2 * n * H * S
    out_w, out_p = fenced(n_out)
    st_w, st_p = fenced(n_stats)
    a = dict(q=fused_d.data_ptr(), ldq=3 * H * D, k=fused_d.data_ptr() + 2 * H * D, ldk=3 * H * D, n_seq=n, S=S, H=H, D=D, out=out_p, per_head=int(per_head), stats=st_p)
    a.update(over)
    rc = lib.aigv_op_vit_attention_map(a["q"], a["ldq"], a["k"], a["ldk"], a["n_seq"], a["S"], a["H"], a["D"], a["out"], a["per_head"], a["stats"], native.stream_ptr())
    torch.cuda.synchronize()
    if refused is not None:
        msg = lib.aigv_last_error(None).decode()
        assert rc == -1 and refused in msg and "aigv_op_vit_attention_map" in msg, (rc, msg)
        unfenced(out_w, n_out, "out", written=False)
        unfenced(st_w, n_stats, "the stats scratch", written=False)
        return None
    native.check(rc)
    unfenced(st_w, n_stats, "the stats scratch")
    return unfenced(out_w, n_out, "out").view((n, H, S, S) if per_head else (n, S, S))


# ---- 1. key census ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.SHAPES, ids=IDS)
def test_op_key_census_is_exact_and_reads_nothing_else(lib, shape):
    """Q = 0: every e is 1, the total the integer S: per head fl(1 / S) everywhere, the head mean the documented chain of it, bit for bit -
    and again with NaN in everything a row must not read: the rows of the other frames, the columns behind K in the fused row, and Q's
    columns of the other heads."""
    n, S, H, D = shape
    q, k = V.census_case(shape)
    fused = V.fused_rows(q, k).cuda()
    per, mean = vmap(lib, fused, shape, True), vmap(lib, fused, shape, False)
    assert torch.equal(bits(per), bits(V.census_expect(shape, True)))
    assert torch.equal(bits(mean), bits(V.census_expect(shape, False)))
    nan = float("nan")
    for f in range(n):
        poisoned = torch.full_like(fused, nan).view(n, S, 3, H, D)
        poisoned[f, :, :2] = fused.view(n, S, 3, H, D)[f, :, :2]              # the frame's own Q and K; V and the other frames stay NaN
        assert torch.equal(bits(vmap(lib, poisoned.view_as(fused), shape, False)[f]), bits(mean[f])), f
        for h in range(H):
            mine = poisoned.clone()
            mine[f, :, 0] = nan
            mine[f, :, 0, h] = 0                                              # Q of the other heads: NaN
            assert torch.equal(bits(vmap(lib, mine.view_as(fused), shape, True)[f, h]), bits(per[f, h])), (f, h)


# ---- 2. one-hot selector ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.SHAPES, ids=IDS)
def test_op_one_hot_selector_is_exactly_one_hot(lib, shape):
    """The selected key leads by a margin at which expf underflows to 0: exactly 1.0 at it, 0.0 elsewhere, per head; with the heads selecting
    different keys the head mean is exactly count / n_heads.  The selected keys include key 0, key S - 1 and both sides of every tile edge."""
    q, k, sel = V.selector_case(shape)
    fused = V.fused_rows(q, k).cuda()
    assert torch.equal(bits(vmap(lib, fused, shape, True)), bits(V.selector_expect(shape, sel, True)))
    assert torch.equal(bits(vmap(lib, fused, shape, False)), bits(V.selector_expect(shape, sel, False)))


# ---- 3. random data: float64, a frame alone, the chain ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_maps(shape):
    q, k = V.random_case(shape)
    fused = V.fused_rows(q, k, torch.randn(q.shape).to(BF)).cuda()
    lib = native.load()
    return fused, vmap(lib, fused, shape, True), vmap(lib, fused, shape, False)


@pytest.mark.parametrize("shape", V.SHAPES, ids=IDS)
def test_op_random_data_against_float64_within_the_derived_bound(lib, shape):
    q, k = V.random_case(shape)
    _, per, mean = random_maps(shape)
    p, eps = V.truth(q, k), V.score_bounds(q, k)
    r_per = ((per.double() - p).abs() / V.per_head_bound(p, eps)).max().item()
    r_mean = ((mean.double() - p.mean(1)).abs() / V.head_mean_bound(p, eps)).max().item()
    print(f"{shape}: worst |p - fp64| / bound = {r_per:.4f} per head, {r_mean:.4f} head mean; worst |row sum - 1| = {(per.double().sum(-1) - 1).abs().max().item():.3e}")
    assert r_per <= 1.0 and r_mean <= 1.0
    if shape[1] > 1:                                                         # (the bound does tell the keys of another head from the right ones)
        wrong = V.truth(q, k.roll(1, 2))
        assert ((wrong - p).abs() / V.per_head_bound(p, eps)).max().item() > 1.0


@pytest.mark.parametrize("shape", V.SHAPES, ids=IDS)
def test_op_frame_alone_is_frame_in_the_pack(lib, shape):
    n, S, H, D = shape
    fused, per, mean = random_maps(shape)
    for f in range(n):
        alone = fused[f * S:(f + 1) * S].contiguous()
        assert torch.equal(bits(vmap(lib, alone, (1, S, H, D), True)[0]), bits(per[f])), f
        assert torch.equal(bits(vmap(lib, alone, (1, S, H, D), False)[0]), bits(mean[f])), f
    order = list(range(n))[::-1]                                             # ... and in another order
    moved = torch.cat([fused[f * S:(f + 1) * S] for f in order]).contiguous()
    assert torch.equal(bits(vmap(lib, moved, shape, False)), bits(mean[order]))


@pytest.mark.parametrize("shape", V.SHAPES, ids=IDS)
def test_op_head_mean_is_the_chain_over_the_per_head_output(lib, shape):
    _, per, mean = random_maps(shape)
    assert torch.equal(bits(mean), bits(V.head_mean_chain(per)))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_op_refusals_leave_every_buffer_untouched(lib):
    shape = V.SHAPES[0]
    n, S, H, D = shape
    fused, per, mean = random_maps(shape)
    qp = fused.data_ptr()
    for over, word in ((dict(D=96), "head_dim"), (dict(D=0), "head_dim"), (dict(H=0), "n_heads"), (dict(H=65), "n_heads"), (dict(n_seq=0), "frames"), (dict(n_seq=65536), "frames"),
                       (dict(S=0), "rows of a frame"), (dict(S=-3), "rows of a frame"), (dict(S=32769), "rows of a frame"), (dict(ldq=H * D - 8), "strides too small"),
                       (dict(ldk=H * D - 8), "strides too small"), (dict(ldq=3 * H * D + 4), "multiple of 8"), (dict(ldk=3 * H * D + 2), "multiple of 8"),
                       (dict(q=qp + 2), "16-byte aligned"), (dict(k=qp + 2 * H * D + 8), "16-byte aligned"), (dict(q=None), "null operand"), (dict(k=None), "null operand")):
        for per_head in (False, True):
            assert vmap(lib, fused, shape, per_head, refused=word, **over) is None
    whole, ptr = fenced(n * S * S)
    for a_out, a_stats, word in ((None, ptr, "null operand"), (ptr, None, "null operand"), (ctypes.c_void_p(ptr.value + 2), ptr, "4-byte"), (ptr, ctypes.c_void_p(ptr.value + 4), "8-byte")):
        rc = lib.aigv_op_vit_attention_map(qp, 3 * H * D, qp + 2 * H * D, 3 * H * D, n, S, H, D, a_out, 0, a_stats, native.stream_ptr())
        assert rc == -1 and word in lib.aigv_last_error(None).decode()
    torch.cuda.synchronize()
    unfenced(whole, n * S * S, "out", written=False)
    assert torch.equal(bits(vmap(lib, fused, shape, False)), bits(mean))     # and the next good call is the good call


# =================================================================================================================================
# model level: tiny towers of three layers at 224 x 224 (a 16 x 16 patch grid, S = 257), two heads of 64
# =================================================================================================================================
from test_gpu_score_attention import clip_alone, make_model, two_clips      # noqa: E402

FLAVOURS = {"plain": dict(), "qknorm": dict(norm_type="rms_norm", qk_norm=True)}
L, S_M = V.MODEL_LAYERS, 257


def tower_cfg(flavour, select_layer=-1):
    cfg = pkg.tiny(image_size=224, vit_layers=L, llm_layers=2, **FLAVOURS[flavour])
    cfg.select_layer = select_layer
    return cfg


@functools.lru_cache(maxsize=None)
def weights(flavour):
    """The seeded N(0, 0.02^2) draw with its Q and K scaled by the committed factor (vit_attention_reference.QK_SCALE)."""
    cfg = tower_cfg(flavour)
    return V.scale_qk(synth.make_state_dict(cfg, seed=V.MODEL_SEED), cfg, V.QK_SCALE[flavour])


@functools.lru_cache(maxsize=None)
def vrig(flavour, select_layer=-1, zero_q=False):
    cfg = tower_cfg(flavour, select_layer)
    sd = V.zero_q(weights(flavour), cfg) if zero_q else weights(flavour)
    model = make_model(cfg, sd, 2)
    kw, ctx_id = two_clips(cfg, V.FRAME_SEED)
    model.img_context_token_id = ctx_id
    return model, cfg, sd, kw


@functools.lru_cache(maxsize=None)
def full_maps(flavour):
    model, cfg, sd, kw = vrig(flavour)
    out = model.vit_attention(kw["pixel_values"])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def frames65():
    return synth.synthetic_frames(65, 224, seed=V.FRAME_SEED + 1)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_armed_pass_changes_no_other_bit(flavour):
    model, cfg, sd, kw = vrig(flavour)
    pv = kw["pixel_values"]
    before = model(**kw)
    tokens = model.vit_tokens(pv)
    out = full_maps(flavour)
    att = out["vit_attention"]
    assert set(out) == {"vit_attention", "tokens"} and same_bits(out["tokens"], tokens)
    assert att.dtype == torch.float32 and tuple(att.shape) == (3, L, S_M, S_M) and model.vit_layers_run() == L
    assert torch.isfinite(att).all() and (att >= 0).all() and (att.double().sum(-1) - 1).abs().max().item() <= (S_M + 4) * 2.0 ** -24
    per = model.vit_attention(pv, per_head=True)
    assert tuple(per["vit_attention"].shape) == (3, L, 2, S_M, S_M) and same_bits(per["tokens"], tokens)
    assert torch.equal(bits(att), bits(V.head_mean_chain(per["vit_attention"].cpu().flatten(0, 1)).view(3, L, S_M, S_M)))
    assert same_bits(model.vit_tokens(pv), tokens)                           # the context disarmed itself
    after = model(**kw)
    assert set(after) == set(before) and all(v is None or same_bits(after[key], v) for key, v in before.items())


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_window_is_the_slice_of_the_full_run(flavour):
    model, cfg, sd, kw = vrig(flavour)
    pv, full = kw["pixel_values"], full_maps(flavour)
    for lo, hi in ((0, 1), (1, 3), (2, 3)):
        got = model.vit_attention(pv, layers=(lo, hi))
        assert same_bits(got["vit_attention"], full["vit_attention"][:, lo:hi].contiguous()) and same_bits(got["tokens"], full["tokens"]), (lo, hi)
    per = model.vit_attention(pv, per_head=True)["vit_attention"]
    assert same_bits(model.vit_attention(pv, layers=(1, 2), per_head=True)["vit_attention"], per[:, 1:2].contiguous())
    for bad in ((0, 0), (2, 1), (-1, 2), (0, L + 1), (1,), 3):
        with pytest.raises(ValueError, match="layers the pass runs"):
            model.vit_attention(pv, layers=bad)
    with pytest.raises(ValueError, match=r"\d{12,} bytes"):                 # more than any device holds: refused with the byte count, nothing allocated
        model.vit_attention(pv[:1].expand(1 << 20, -1, -1, -1), per_head=True)       # (a view: one frame's memory)
    keep = model._capture_keep                                              # never inside a graph capture (the package's own mark of one underway)
    try:
        model._capture_keep = []
        with pytest.raises(RuntimeError, match="graph capture"):
            model.vit_attention(pv)
    finally:
        model._capture_keep = keep
    assert same_bits(model.vit_attention(pv)["vit_attention"], full["vit_attention"])


def test_model_select_layer_bounds_the_window(lib):
    model, cfg, sd, kw = vrig("plain", select_layer=-2)
    pv, full = kw["pixel_values"], full_maps("plain")
    assert model.vit_layers_run() == L - 1
    got = model.vit_attention(pv)
    assert same_bits(got["vit_attention"], full["vit_attention"][:, :L - 1].contiguous())
    tokens = model.vit_tokens(pv)
    assert same_bits(got["tokens"], tokens)
    with pytest.raises(ValueError, match=f"hi <= {L - 1}"):
        model.vit_attention(pv, layers=(0, L))
    # the C ABI's own refusal: armed by hand in front of the pass, which knows how many layers it runs
    n = 3 * L * S_M * S_M
    whole, ptr = fenced(n)
    _, ctx = model._native(n_frames=3)
    for lo, hi in ((0, L), (1, 1), (-1, 1), (2, 1)):
        native.check(lib.aigv_vit_attention_arm(ctx, ptr, lo, hi, 0), ctx)
        with pytest.raises(native.NativeError, match="layers the pass runs"):
            model.vit_tokens(pv)
        torch.cuda.synchronize()
        assert same_bits(model.vit_tokens(pv), tokens)                       # the refused pass disarmed: a plain pass runs
    assert lib.aigv_vit_attention_arm(ctx, None, 0, 1, 0) == -1 and "null out_dev" in lib.aigv_last_error(ctx).decode()
    torch.cuda.synchronize()
    unfenced(whole, n, "out_dev", written=False)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_frame_alone_is_frame_among_others_across_a_chunk_boundary(flavour):
    """65 frames: vit_chunk is 64, so frame 64 runs as a chunk of its own behind a full one - and every map of the 65 lands at its absolute
    frame number."""
    model, cfg, sd, kw = vrig(flavour)
    pv = frames65()
    both = model.vit_attention(pv)
    assert tuple(both["vit_attention"].shape) == (65, L, S_M, S_M) and same_bits(both["tokens"], model.vit_tokens(pv))
    for f in (0, 63, 64):
        alone = model.vit_attention(pv[f:f + 1])
        assert same_bits(alone["vit_attention"][0], both["vit_attention"][f]) and same_bits(alone["tokens"][0], both["tokens"][f]), f
    assert not torch.equal(both["vit_attention"][63], both["vit_attention"][64])
    assert same_bits(model.vit_attention(kw["pixel_values"])["vit_attention"], full_maps(flavour)["vit_attention"])      # (the larger context changes no bit)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_census_is_exact_in_every_layer_frame_and_chunk(flavour):
    """The Q third of every qkv.weight and qkv.bias zeroed: every map of every layer of all 65 frames is the census value - no tolerance."""
    model, cfg, sd, kw = vrig(flavour, zero_q=True)
    mean = model.vit_attention(frames65())["vit_attention"]
    want = V.census_expect((1, S_M, 2, 64), False)[0]
    assert torch.equal(bits(mean), bits(want.expand(65, L, S_M, S_M)))
    per = model.vit_attention(kw["pixel_values"], layers=(1, L), per_head=True)["vit_attention"]
    assert torch.equal(bits(per), bits(V.census_value(S_M).expand(3, L - 1, 2, S_M, S_M)))


@functools.lru_cache(maxsize=None)
def oracle_head_means(flavour, qk_norm=None):
    """{dtype: {layer: (head-mean map float64 [F, S, S], probabilities, q, k)}} of the CPU oracle for layer 0 and the last layer."""
    from oracle import oracle as O
    cfg = tower_cfg(flavour)
    if qk_norm is not None:
        cfg = copy.deepcopy(cfg)
        cfg.vision_config.qk_normalization = qk_norm
    pv = two_clips(cfg, V.FRAME_SEED)[0]["pixel_values"]
    out = {}
    for dtype in (torch.float32, BF):
        maps = V.oracle_maps(O, weights(flavour), cfg, pv, (0, L - 1), dtype)
        out[dtype] = {l: (p.double().mean(1), p, q, k) for l, (p, q, k) in maps.items()}
    return out


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_maps_against_the_cpu_oracle(flavour):
    """The right Q and K are read: layer 0 and the last layer against the oracle's eager probabilities (fp32 weights-widened run).  The bar is
    3 x d_ref + the op-level bound, d_ref = max |oracle bf16 - oracle fp32| over the head-mean maps of the layer, measured here on the CPU
    (triangle inequality: 2 x; the extra half for the HIP path's different rounding points).  Conditions that keep it from passing vacuously:
    the oracle's fp32 maps have a median row maximum >= 8 / S, two frames differ by >= 20 x the bar and, with the QK norm, the map differs
    from the same weights' map without it by >= 20 x the bar.
    Measured (MI355X; profiles/vit_attention_cost.txt): d_ref 2.5e-3 .. 4.0e-3, worst |hip - oracle fp32| 0.24 .. 0.29 x the bar; two frames differ by
    29 .. 35 x the bar, the QK norm on / off by 30 .. 34 x."""
    got = full_maps(flavour)["vit_attention"].cpu().double()
    ref = oracle_head_means(flavour)
    for l in (0, L - 1):
        a32, p32, _, _ = ref[torch.float32][l]
        a16, _, q16, k16 = ref[BF][l]
        d_ref = (a16 - a32).abs().max().item()
        bound = V.head_mean_bound(p32.double(), V.score_bounds(q16.transpose(1, 2), k16.transpose(1, 2)))
        bar = 3 * d_ref + bound
        top = 3 * d_ref + bound.max().item()
        median_max = a32.max(-1).values.median().item()
        frames = max((a32[i] - a32[j]).abs().max().item() for i in range(3) for j in range(i))
        err = (got[:, l] - a32).abs()
        print(f"{flavour} layer {l}: d_ref = {d_ref:.3e}, op bound <= {bound.max().item():.2e}, worst |hip - oracle fp32| = {err.max().item():.3e} = {(err / bar).max().item():.3f} x the bar; "
              f"median row max = {median_max * S_M / 8:.2f} x 8/S; two frames differ by {frames / top:.1f} x the bar")
        assert median_max >= 8.0 / S_M
        assert frames >= 20 * top
        if flavour == "qknorm":
            no_norm = oracle_head_means(flavour, qk_norm=False)[torch.float32][l][0]
            print(f"    with / without the QK norm differ by {(a32 - no_norm).abs().max().item() / top:.1f} x the bar")
            assert (a32 - no_norm).abs().max().item() >= 20 * top
        assert (err <= bar).all()


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_rollout_carries_the_heat_map_to_the_pixels(flavour):
    """heat -> rollout -> pixel map on a real pass: pix.sum + cls == heat.sum to float64 rounding, per frame."""
    model, cfg, sd, kw = vrig(flavour)
    one = clip_alone(kw, 0)                                                  # one clip of two frames
    out = model(**one, return_token_attention=True)
    pos = model.visual_token_positions(one["input_ids"], one["attention_mask"], one["image_flags"])
    heat = eval_utils.frame_heatmaps(out["score_attention_tokens"], pos).cpu()
    roll = eval_utils.vit_rollout(model.vit_attention(one["pixel_values"])["vit_attention"]).cpu()
    assert tuple(heat.shape) == (1, 2, 8, 8) and tuple(roll.shape) == (2, S_M, S_M)
    rows = roll.double().sum(-1)
    assert (rows - 1).abs().max().item() <= L * (S_M + 4) * 2.0 ** -24      # every layer's rows sum to 1 to fp32 rounding, and so does their product
    pix, cls = eval_utils.pixel_heatmaps(heat, roll)
    assert tuple(pix.shape) == (1, 2, 16, 16) and tuple(cls.shape) == (1, 2) and (pix >= 0).all() and (cls > 0).all()
    # exactly: the heat split in quarters over the rollout's rows, each row passing on its row sum
    want = ((heat.double() / 4).repeat_interleave(2, 2).repeat_interleave(2, 3).reshape(2, 256) * rows[:, 1:]).sum(-1)
    assert ((pix.sum((2, 3)) + cls)[0] - want).abs().max().item() <= 4 * S_M * 2.0 ** -53
    assert ((pix.sum((2, 3)) + cls) - heat.double().sum((2, 3))).abs().max().item() <= L * (S_M + 4) * 2.0 ** -24
