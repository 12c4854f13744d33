"""Score-row value flow on the MI355X: the VALUES form of the probe kernel through aigv_op_attention_probe_values (no model) on the
constructions of tests/score_attention_reference.py - census and one-hot selector exact, random data against float64 within the derived bound
(tests/score_values_reference.py), the bins and dense rows of the same launch bit-equal to the plain and dense calls, a row's bits its own,
the limits, the host refusals - every call inside a sentinel fence around all three outputs; then ``forward(return_score_values=True)`` and
``forward_shared_prefix`` through the model, completeness against the pass's own flash output (``return_heads``), and the ``eval_utils``
helpers.  tests/test_score_values_cpu.py holds, without a GPU, what these expectations rest on."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import depth_lens_reference as DL
import score_attention_reference as R
import score_values_reference as VR
import test_gpu_score_attention as G          # the tiny model rig of the score-attention tests (cached: one model for the three files)
import test_gpu_score_attention_tokens as GT
from aigv_assessor_amd import eval_utils, native, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D, S, HK = R.D, R.S, R.N_KV
SENTINEL, PAD = G.SENTINEL, G.PAD
bits = G.bits
ROWS = [t for _, _, t in R.probe_rows()]
KL = {128: 2, 64: 4}                          # the kernel's key lanes, 256 / D


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


def fenced(n):
    whole = torch.full((PAD + max(n, 1) + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole.data_ptr() + 4 * PAD


def probe_values(lib, fused_d, g, rows, seg_new_d, lens=R.LENS, cache=None, n_seg=S, d=D, dense=False, extra=0, refused=None, v_ptr=None, ldv=None,
                 null_val=False, null_v=False):
    """aigv_op_attention_probe_values on fused rows [T, HK (g + 2) d] (V: the fused rows' own V columns); cache = (kc, vc, cap, kv_off list,
    seg_cached_d, ld_cached) for the cache form.  out, tok (dense=True) and val each sit between two sentinel pads inside an allocation that
    starts as the sentinel.  Returns (out [rows, heads, n_seg], tok [rows, heads, ld_tok] or None, val [rows, heads, n_seg + 1, d]) after checking
    that every pad kept its bits and that every element of every output was written.  refused = a word of the expected message: the call must
    return AIGV_ERR_ARG and leave every allocation untouched."""
    h, ld = HK * g, HK * (g + 2) * d
    kv_off = cache[3] if cache is not None else None
    ld_tok = GT.need_of(rows, lens, kv_off) + extra if dense else 0
    nr = min(len(rows), 64)
    n, nt, nv = nr * h * n_seg, nr * h * ld_tok, nr * h * (n_seg + 1) * d
    (w_o, p_o), (w_t, p_t), (w_v, p_v) = fenced(n), fenced(nt), fenced(nv)
    cos, sin = GT.tables(d)
    cu = native.i32_array(R.cu_of(lens))
    if cache is None:
        k_ptr, ldk, hs, ss, off, segc, ldc = fused_d.data_ptr() + 2 * g * d, ld, (g + 2) * d, 0, None, None, 0
        v0, ldv0 = fused_d.data_ptr() + 2 * (g + 1) * d, ld
    else:
        kc, vc, cap, _, segc_d, ldc = cache
        k_ptr, ldk, hs, ss, off, segc = kc.data_ptr(), d, cap * d, HK * cap * d, native.i32_array(kv_off), segc_d.data_ptr()
        v0, ldv0 = vc.data_ptr(), d
    v_ptr = None if null_v else v0 if v_ptr is None else v_ptr(v0)
    rc = lib.aigv_op_attention_probe_values(fused_d.data_ptr(), ld, k_ptr, ldk, cu, len(lens), h, HK, (g + 2) * d, hs, ss, off, d, cos.data_ptr(), sin.data_ptr(),
                                            cos.shape[0], native.i32_array(rows), len(rows), seg_new_d.data_ptr(), segc, ldc, n_seg, ctypes.c_void_p(p_o),
                                            ctypes.c_void_p(p_t) if dense else None, ld_tok, v_ptr, ldv0 if ldv is None else ldv,
                                            None if null_val else ctypes.c_void_p(p_v), native.stream_ptr())
    torch.cuda.synchronize()
    w, wt, wv = w_o.cpu(), w_t.cpu(), w_v.cpu()
    if refused is not None:
        msg = lib.aigv_last_error(None).decode()
        assert rc == -1 and refused in msg and "aigv_op_attention_probe_values" in msg, (rc, msg)
        assert (w == SENTINEL).all() and (wt == SENTINEL).all() and (wv == SENTINEL).all(), "a refused call wrote something"
        return None, None, None
    assert rc == 0, lib.aigv_last_error(None).decode()
    for name, a, m in (("bin", w, n), ("dense", wt, nt), ("value", wv, nv)):
        assert (a[:PAD] == SENTINEL).all() and (a[PAD + m:] == SENTINEL).all(), f"the probe wrote outside its {name} output"
        assert (a[PAD:PAD + m] != SENTINEL).all(), f"the probe left part of its {name} output unwritten"
    return (w[PAD:PAD + n].view(torch.float32).view(len(rows), h, n_seg).clone(),
            wt[PAD:PAD + nt].view(torch.float32).view(len(rows), h, ld_tok).clone() if dense else None,
            wv[PAD:PAD + nv].view(torch.float32).view(len(rows), h, n_seg + 1, d).clone())


def cache_form(lib, fused, seg, g, d=D, n_seg=S, dense=False, poison=False):
    """The op-level case in CACHE form (test_gpu_score_attention.cache_form_probe, with V): K and V of every token stored at their position by
    aigv_op_kv_store, the rest of both caches NaN; the pass = the rows behind CACHE_OFF[b].  poison: the fused rows the call is given carry NaN
    in their own K and V columns - the cache form must read the caches.  Returns ([(index into probe_rows(), packed row of the shortened pass)],
    out, tok, val)."""
    cu, off, cap, T = R.cu_of(R.LENS), R.CACHE_OFF, R.CACHE_CAP, sum(R.LENS)
    kc = torch.full((len(R.LENS), HK, cap, d), float("nan"), dtype=BF, device="cuda")
    vc = torch.full_like(kc, float("nan"))
    seq = torch.repeat_interleave(torch.arange(len(R.LENS)), torch.tensor(R.LENS)).to(torch.int32).cuda()
    pos_d = R.positions().cuda()
    native.check(lib.aigv_op_kv_store(fused.data_ptr(), fused.shape[1], seq.data_ptr(), pos_d.data_ptr(), kc.data_ptr(), vc.data_ptr(), T, HK, g, d, cap,
                                      native.stream_ptr()))
    new_lens = [n - o for n, o in zip(R.LENS, off)]
    keep = torch.cat([torch.arange(cu[b] + off[b], cu[b + 1]) for b in range(len(R.LENS))])
    cu_new = R.cu_of(new_lens)
    ldc = max(off) + 3
    segc = torch.full((len(R.LENS), ldc), -1, dtype=torch.int32)
    for b in range(len(R.LENS)):
        segc[b, :off[b]] = seg[cu[b]:cu[b] + off[b]]
    picks = [(i, cu_new[b] + r - off[b]) for i, (b, r, t) in enumerate(R.probe_rows()) if r >= off[b]]
    assert {R.probe_rows()[i][0] for i, _ in picks} == {0, 1, 2} and len(picks) >= 10
    rows_d = fused[keep.cuda()].contiguous()
    if poison:
        rows_d.view(-1, HK, g + 2, d)[:, :, g:] = float("nan")
    return (picks,) + probe_values(lib, rows_d, g, [t for _, t in picks], seg[keep].cuda(), lens=new_lens, cache=(kc, vc, cap, off, segc.cuda(), ldc), n_seg=n_seg,
                                   d=d, dense=dense)


# ---- 1. census --------------------------------------------------------------------------------------------------------------------------------
def census_check(lib, g, d=D):
    gen = torch.Generator().manual_seed(5 + g)
    T, cu = sum(R.LENS), R.cu_of(R.LENS)
    q = torch.zeros(T, HK, g, d, dtype=BF)
    k = torch.randn(T, HK, d, generator=gen).to(BF)
    v = VR.census_v(T, d=d, seed=g)
    seg = R.seg_table()
    seg_d = seg.cuda()
    _, _, val = probe_values(lib, R.fused(q, k, v).cuda(), g, ROWS, seg_d, d=d)
    want = {t: VR.census_values(v[cu[b]:], seg[cu[b]:], r + 1, S, g) for b, r, t in R.probe_rows()}
    for i, (b, r, t) in enumerate(R.probe_rows()):
        assert torch.equal(bits(val[i]), bits(want[t])), (b, r, val[i, 0, :, 0].tolist(), want[t][0, :, 0].tolist())
    picks, _, _, cached = cache_form(lib, R.fused(q, k, v).cuda(), seg, g, d=d, poison=True)
    for j, (i, _) in enumerate(picks):
        assert torch.equal(bits(cached[j]), bits(val[i])), ("cache form", R.probe_rows()[i])
    # every row alone, NaN in every K and V row it must not read: behind it, and the other sequences'
    for i, (b, r, t) in enumerate(R.probe_rows()):
        kp, vp = k.clone(), v.clone()
        for x in (kp, vp):
            x[:cu[b]] = float("nan")
            x[t + 1:] = float("nan")
        _, _, one = probe_values(lib, R.fused(q, kp, vp).cuda(), g, [t], seg_d, d=d)
        assert torch.equal(bits(one[0]), bits(want[t])), (b, r)


@pytest.mark.parametrize("g", R.GROUPS)
def test_op_census_every_slot_holds_the_integer_sum_over_n(lib, g):
    """Q = 0, V small integers: val[s][c] is fp32(sum of v_j[c] over the slot's keys) / fp32(n) bit for bit - packed form, cache form (V from the
    V cache: the fused rows' own K / V columns are NaN there), and every row alone with NaN in every K and V row it must not read."""
    census_check(lib, g)


def test_op_head_dim_64_census_and_random_data(lib):
    """The D = 64 instantiation (four key lanes, another thread-to-column map): the census bit-exact, random data within the derived bound - and
    on that random data the bins and the dense rows bit-equal to the plain and the dense call, the values the same beside the dense rows."""
    g, d = 2, 64
    census_check(lib, g, d=d)
    gen = torch.Generator().manual_seed(6400)
    T, cu = sum(R.LENS), R.cu_of(R.LENS)
    q, k, v = (torch.randn(T, HK, *s, generator=gen).to(BF) for s in ((g, d), (d,), (d,)))
    cos, sin = R.rope_table(d, R.N_POS)
    seg = R.seg_table()
    fused, seg_d = R.fused(q, k, v).cuda(), seg.cuda()
    out, _, val = probe_values(lib, fused, g, ROWS, seg_d, d=d)
    out_d, tok_d, val_d = probe_values(lib, fused, g, ROWS, seg_d, d=d, dense=True)
    assert torch.equal(bits(out_d), bits(out)) and torch.equal(bits(val_d), bits(val))
    assert torch.equal(bits(out), bits(G.probe(lib, fused, g, ROWS, seg_d, cos_sin=GT.tables(d), d=d)))
    out_t, tok_t = GT.probe_tokens(lib, fused, g, ROWS, seg_d, d=d)
    assert torch.equal(bits(out), bits(out_t)) and torch.equal(bits(tok_d), bits(tok_t))
    q_rot = R.rotate_q(q, R.positions(), cos, sin)
    worst = 0.0
    for i, (b, r, t) in enumerate(R.probe_rows()):
        lo, qr = cu[b], q_rot[t].reshape(HK * g, d)
        truth, weight = VR.row_truth(qr, k[lo:lo + r + 1], v[lo:lo + r + 1], seg[lo:lo + r + 1], S)
        bound = VR.value_bound(weight, R.score_bound(qr, k[lo:lo + r + 1]), r + 1, KL[d])
        worst = max(worst, ((val[i].double() - truth).abs() / bound).max().item())
    print(f"D=64: worst |val - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- 2. one-hot selector ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_one_hot_selector_hands_out_the_selected_keys_v_row(lib, g):
    """The selected key's slot holds V[sel] exactly, every other slot is 0 (by value) - the selected key at the first position, the last, and on
    both sides of the 256 stride; packed form, and cache form wherever the row lies behind its sequence's CACHE_OFF."""
    v = VR.random_v(sum(R.LENS), seed=g)
    n_cache = 0
    for b, r, sel in R.selector_cases():
        c = R.SelectorCase(g, b, r, sel)
        fused = R.fused(c.q, c.k, v).cuda()
        out, _, val = probe_values(lib, fused, g, [c.row], c.seg.cuda())
        want = VR.selector_values(c, v)
        assert (val[0] == want).all(), (b, r, sel, val[0, 0].abs().sum(-1).tolist())
        assert torch.equal(bits(out[0]), bits(c.expect()))
        if r >= R.CACHE_OFF[b]:
            picks, _, _, valc = cache_form(lib, fused, c.seg, g)
            j = [j for j, (i, _) in enumerate(picks) if R.probe_rows()[i][2] == c.row][0]
            assert (valc[j] == want).all(), ("cache form", b, r, sel)
            n_cache += 1
    assert n_cache >= 9


# ---- 3. random data against float64 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def values_case(g):
    return VR.ValuesCase(g)


@functools.lru_cache(maxsize=None)
def random_run(g, table="seg"):
    """(bins, dense rows, values) of the random case in packed form, all probe rows in one launch: computed once, shared, never modified."""
    c = values_case(g)
    return probe_values(native.load(), R.fused(c.q, c.k, c.v).cuda(), g, ROWS, (c.seg if table == "seg" else c.runs).cuda(), dense=True, extra=GT.extra_of(g))


@pytest.mark.parametrize("table", ["seg", "runs"])
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_random_data_against_float64_within_the_derived_bound(lib, g, table):
    """|val - val64| <= (sum p |v|) (e^(2 eps) (1 + gamma_c) - 1) + 2^-126 per (slot, column) (score_values_reference.value_bound: derived, not
    chosen), over seg_table - the id changes at every key, ids -1 and S feed the rest slot - and over a table of contiguous runs; and the S + 1
    slots sum to the float64 head output within the summed bounds."""
    c = values_case(g)
    _, _, val = random_run(g, table)
    truth = c.truth(seg=c.seg if table == "seg" else c.runs, key_lanes=KL[D])
    worst = worst_sum = 0.0
    for i, t in enumerate(ROWS):
        want, bound = truth[t]
        worst = max(worst, ((val[i].double() - want).abs() / bound).max().item())
        worst_sum = max(worst_sum, ((val[i].double().sum(1) - want.sum(1)).abs() / bound.sum(1)).max().item())
    rest = val[:, :, S].abs().sum().item()
    assert (rest > 0) == (table == "seg")                                  # seg_table drops keys into the rest slot, the runs cover every key
    print(f"g={g} {table}: worst |val - fp64| / bound = {worst:.4f}; worst |sum of slots - head output| / bound = {worst_sum:.4f}")
    assert worst <= 1.0 and worst_sum <= 1.0


# ---- 4. the bins and the dense rows of the VALUES launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_bins_and_dense_rows_are_the_plain_and_dense_calls(lib, g):
    c = values_case(g)
    out, tok, _ = random_run(g)
    fused = R.fused(c.q, c.k, c.v).cuda()
    assert torch.equal(bits(out), bits(G.probe(lib, fused, g, ROWS, c.seg.cuda())))
    out_t, tok_t = GT.probe_tokens(lib, fused, g, ROWS, c.seg.cuda(), extra=GT.extra_of(g))
    assert torch.equal(bits(out), bits(out_t)) and torch.equal(bits(tok), bits(tok_t))
    bins_only, none, _ = probe_values(lib, fused, g, ROWS, c.seg.cuda())    # without the dense rows: the same bins
    assert none is None and torch.equal(bits(bins_only), bits(out))


# ---- 5. a row's bits are its own ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", R.GROUPS)
def test_op_cache_form_and_batch_mates_change_no_bit(lib, g):
    c = values_case(g)
    fused = R.fused(c.q, c.k, c.v).cuda()
    seg_d = c.seg.cuda()
    _, _, base = random_run(g)
    picks, _, _, got = cache_form(lib, fused, c.seg, g, poison=True)
    for j, (i, _) in enumerate(picks):
        assert torch.equal(bits(got[j]), bits(base[i])), ("cache form", R.probe_rows()[i])
    many = [ROWS[i % len(ROWS)] for i in range(64)]
    _, _, crowd = probe_values(lib, fused, g, many, seg_d)
    for i, t in enumerate(ROWS):
        _, _, alone = probe_values(lib, fused, g, [t], seg_d)
        for at in range(i, 64, len(ROWS)):
            assert torch.equal(bits(alone[0]), bits(crowd[at])), ("row alone", t, at)
        assert torch.equal(bits(alone[0]), bits(base[i]))
    cu = c.cu
    for b, n in enumerate(R.LENS):                                          # a sequence alone (re-packed from row 0) against the sequences side by side
        mine = [(i, r) for i, (bb, r, _) in enumerate(R.probe_rows()) if bb == b]
        _, _, alone = probe_values(lib, fused[cu[b]:cu[b + 1]].contiguous(), g, [r for _, r in mine], c.seg[cu[b]:cu[b + 1]].cuda(), lens=[n])
        for j, (i, _) in enumerate(mine):
            assert torch.equal(bits(alone[j]), bits(base[i])), ("sequence alone", b)


# ---- 6. the limits and the refusals ---------------------------------------------------------------------------------------------------------------
def test_op_fences_at_the_limits(lib):
    """S = 1 and S = 64 (the LDS maximum), 1 and 64 rows, n_keys = 1: every element written, nothing outside (probe_values' fences), within the
    derived bound, and the slots sum to the head output."""
    g = 1
    c = values_case(g)
    fused = R.fused(c.q, c.k, c.v).cuda()
    q_rot = R.rotate_q(c.q, c.pos, c.cos, c.sin)
    for n_seg, seg, rows in ((64, (torch.arange(c.T) % 66 - 1).to(torch.int32), [ROWS[i % len(ROWS)] for i in range(64)]),
                             (1, (torch.arange(c.T) % 2).to(torch.int32), [ROWS[-1]]), (64, (torch.arange(c.T) % 64).to(torch.int32), [ROWS[0]]),
                             (1, torch.zeros(c.T, dtype=torch.int32), ROWS)):
        _, tok, val = probe_values(lib, fused, g, rows, seg.cuda(), n_seg=n_seg, dense=n_seg == 64)
        assert tuple(val.shape) == (len(rows), HK * g, n_seg + 1, D)
        for i, t in enumerate(rows[:len(ROWS)]):
            b, r, _ = R.probe_rows()[ROWS.index(t)]
            lo, qr = c.cu[b], q_rot[t].reshape(HK * g, D)
            truth, weight = VR.row_truth(qr, c.k[lo:lo + r + 1], c.v[lo:lo + r + 1], seg[lo:lo + r + 1], n_seg)
            bound = VR.value_bound(weight, R.score_bound(qr, c.k[lo:lo + r + 1]), r + 1, KL[D])
            assert ((val[i].double() - truth).abs() <= bound).all(), (n_seg, t)
            if r == 0:                                                      # one key: weight exactly 1, the slot is the key's V row
                assert (val[i].sum(1) == c.v[lo].float().repeat_interleave(g, 0)).all()


def test_op_refusals_are_host_side_and_write_nothing(lib):
    c = values_case(1)
    fused, seg_d = R.fused(c.q, c.k, c.v).cuda(), c.seg.cuda()
    probe_values(lib, fused, 1, ROWS, seg_d, null_v=True, refused="null v")
    probe_values(lib, fused, 1, ROWS, seg_d, null_val=True, refused="null val_out")                # a half-given pair, either half
    probe_values(lib, fused, 1, ROWS, seg_d, v_ptr=lambda p: p + 8, refused="16-byte aligned")
    probe_values(lib, fused, 1, ROWS, seg_d, ldv=fused.shape[1] + 4, refused="multiple of 8")
    probe_values(lib, fused, 1, ROWS, seg_d, ldv=D, refused="packed V strides too small")         # a stride that does not hold both kv heads
    probe_values(lib, fused, 1, [ROWS[i % len(ROWS)] for i in range(65)], seg_d, refused="probe rows")
    probe_values(lib, fused, 1, ROWS, seg_d, n_seg=65, refused="segments")
    _, _, val = probe_values(lib, fused, 1, ROWS, seg_d)                                           # and the accepted call next to them
    assert torch.equal(bits(val), bits(random_run(1)[2]))


# =====================================================================================================================================================
# model level: the tiny configuration of the score-attention tests, two clips of (2, 1) frames
# =====================================================================================================================================================
OPTS = dict(return_logprobs=True, top_logprobs=3)


def probe_mask(model, kw):
    """bool [B, N]: every clip's probe row (the score row; in a stage-1 model the row that predicts the first answer token)."""
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], kw["pixel_values"].shape[0])
    mask = torch.zeros_like(kw["input_ids"], dtype=torch.bool)
    for b, r in enumerate(model._probe_rows(plan)):
        mask[b] = plan["row_of"][b] == r
    assert mask.sum(1).tolist() == [1] * mask.shape[0]
    return mask


@functools.lru_cache(maxsize=None)
def flagged(stage):
    """(model, cfg, sd, kw, the rig's pass WITHOUT the flag, the same pass WITH it and with the heads of the probe rows captured)."""
    model, cfg, sd, kw, base = G.rig(stage)
    on = model(**kw, return_score_values=True, return_heads=probe_mask(model, kw), **OPTS)
    torch.cuda.synchronize()
    return model, cfg, sd, kw, base, on


@pytest.mark.parametrize("stage", [2, 1])
def test_model_the_flag_changes_nothing_else(stage):
    model, cfg, sd, kw, base, on = flagged(stage)
    assert set(on) == set(base) | {"score_values", "score_values_rest", "heads", "heads_index"}
    for key in base:                                                         # score_attention included
        if torch.is_tensor(base[key]):
            assert torch.equal(on[key], base[key]) or torch.equal(bits(on[key]), bits(base[key])), key
    llm, val, rest = cfg.llm_config, on["score_values"], on["score_values_rest"]
    Sg = base["score_attention"].shape[-1]
    assert val.dtype == torch.float32 and tuple(val.shape) == (2, llm.num_hidden_layers, llm.num_attention_heads, Sg, llm.head_dim)
    assert tuple(rest.shape) == (2, llm.num_hidden_layers, llm.num_attention_heads, llm.head_dim) and (rest == 0).all() and torch.isfinite(val).all()
    assert val.untyped_storage().data_ptr() == rest.untyped_storage().data_ptr()      # two views of one buffer
    assert (val[1, :, :, 1] == 0).all() and (val[0, :, :, 1] != 0).any()               # clip 1 has one frame: its frame slot 1 stays empty
    both = model(**kw, return_score_values=True, return_token_attention=True)          # beside the dense rows: every probe output keeps its bits
    tokens = GT.flagged(stage)[5]["score_attention_tokens"]
    assert torch.equal(bits(both["score_values"]), bits(val)) and torch.equal(bits(both["score_attention_tokens"]), bits(tokens))
    assert torch.equal(bits(both["score_attention"]), bits(base["score_attention"]))
    snap = val.clone()                                                       # the context disarmed itself: a plain pass writes no stale tensor
    again = model(**kw)
    torch.cuda.synchronize()
    assert "score_values" not in again and "score_attention" not in again and torch.equal(val, snap)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_clip_alone_is_clip_in_batch(stage):
    model, cfg, sd, kw, base, on = flagged(stage)
    for b in range(2):
        alone = model(**G.clip_alone(kw, b), return_score_values=True)
        batch = on["score_values"][b]
        if alone["score_values"].shape[3] != batch.shape[2]:                 # clip 1 alone has F = 1: one frame slot fewer, the same bits behind it
            batch = torch.cat([batch[:, :, :1], batch[:, :, 2:]], 2)
        assert torch.equal(bits(alone["score_values"][0]), bits(batch)), b


@pytest.mark.parametrize("stage", [2, 1])
def test_model_layer0_from_first_principles(lib, stage):
    """RMSNorm -> wqkv -> RoPE of layer 0 restated in float64 from the weights and the embedded rows, as test_gpu_score_attention does for the
    mass: the layer-0 values lie within value_bound widened by the bf16 roundings the pass has and the restatement has not.  For q and k that
    test's term: a further score error of 2 * 2^-8 sum |q||k| / sqrt(D), through the exponent.  For v, per element: the stored v_j[c] is the bf16
    rounding of a dot of the bf16 normed row with the weights - 2^-8 |v_j[c]| for the output's rounding, and 2 * 2^-8 sum_i |xn_ji| |w_ci| for the
    normed row's two roundings (the norm casts to bf16, then scales by its weight and rounds again), which is NOT relative to |v_j[c]|: a small v
    that is the difference of large products moves by the products' size.  Both enter sum_j p_j |dv_j[c]| per slot; x 1.01 for second order."""
    model, cfg, sd, kw, base, on = flagged(stage)
    llm = cfg.llm_config
    H, nh, nkv = llm.hidden_size, llm.num_attention_heads, llm.num_key_value_heads
    d, g = H // nh, nh // nkv
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], kw["pixel_values"].shape[0])
    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    T = plan["cu"][-1]
    x = torch.empty(T, H, dtype=BF, device="cuda")
    emb = sd["language_model.model.tok_embeddings.weight"].to(BF).cuda()
    ids_d, slot_d = plan["ids_packed"].to(torch.long).cuda(), plan["slot"].to(torch.int32).cuda()
    native.check(lib.aigv_op_embed(ids_d.data_ptr(), slot_d.data_ptr(), emb.data_ptr(), vis.data_ptr(), motion.data_ptr(), plan["n_vis"], x.data_ptr(), T, H,
                                   native.stream_ptr()))
    torch.cuda.synchronize()
    x = x.cpu().double()
    w_n = sd["language_model.model.layers.0.attention_norm.weight"].double()
    w = sd["language_model.model.layers.0.attention.wqkv.weight"].double()
    xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + llm.rms_norm_eps) * w_n
    qkv = (xn @ w.T).view(T, nkv, g + 2, d)
    prod = (xn.abs() @ w.abs().T).view(T, nkv, g + 2, d)[:, :, g + 1]                       # [T, nkv, d]: sum_i |xn_i| |w_ci| of the V columns
    from aigv_assessor_amd.modeling import rope_tables
    cos, sin = rope_tables(d, llm.rope_theta, max(plan["lens"]), llm.max_position_embeddings, getattr(llm, "rope_scaling", None))
    cos, sin = torch.cat([cos, cos], -1).double(), torch.cat([sin, sin], -1).double()

    def rot(v, pos):
        r = torch.cat((-v[..., d // 2:], v[..., : d // 2]), -1)
        shape = (len(pos),) + (1,) * (v.dim() - 2) + (d,)
        return v * cos[pos].view(shape) + r * sin[pos].view(shape)

    seg, n_seg = model._default_segments(plan)
    got = torch.cat([on["score_values"], on["score_values_rest"][:, :, :, None]], 3).cpu()
    worst = 0.0
    for b, t in enumerate(model._probe_rows(plan)):
        lo = plan["cu"][b]
        pos = torch.arange(t - lo + 1)
        q = rot(qkv[t:t + 1, :, :g], pos[-1:])[0].reshape(nh, d)
        k = rot(qkv[lo:t + 1, :, g], pos)
        truth, weight = VR.row_truth(q, k, qkv[lo:t + 1, :, g + 1], seg[lo:t + 1], n_seg)
        _, products = VR.row_truth(q, k, prod[lo:t + 1], seg[lo:t + 1], n_seg)              # sum_j p_j sum_i |xn_ji| |w_ci| per slot
        eps = R.score_bound(q, k)
        bound = VR.value_bound(weight, eps, t - lo + 1, KL[d], extra_rel=eps / ((d + 2) * 2.0 ** -24) * 2 * 2.0 ** -8) + 1.01 * 2.0 ** -8 * (weight + 2 * products)
        worst = max(worst, ((got[b, 0].double() - truth).abs() / bound).max().item())
    print(f"stage {stage}: layer 0 worst |val - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("stage", [2, 1])
def test_model_shared_prefix_against_separate_passes(stage):
    """Each prompt's values from forward_shared_prefix (V read from the KV cache by the continuation pass) lie within 1.3 x the project's yardstick
    for 'the same up to summation order' of the separate forward of that prompt - test_gpu_score_attention's bound for the mass, applied to the
    values: the distance between two forward calls that differ only in GEMM mode (1 against 2), measured here on the values."""
    model, cfg, sd, kw, base = G.rig(stage)
    B, T = 2, 2
    toks = synth.canonical_tokens(cfg, B, T, seed=500 + stage)
    pp = synth.perspective_prompts(toks, 3, seed=500 + stage)
    common = dict(pixel_values=synth.synthetic_frames(B * T, 224, seed=500), image_flags=torch.ones(B * T, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(B, cfg.motion_dim, seed=500))
    sep = lambda p: model(**common, input_ids=p["input_ids"], attention_mask=p["attention_mask"], labels=p["labels"], return_score_values=True)
    whole = lambda o: torch.cat([o["score_values"], o["score_values_rest"][:, :, :, None]], 3).double()
    try:
        model.set_gemm_mode(1)
        m1 = [whole(sep(p)) for p in pp]
        model.set_gemm_mode(2)
        m2 = [whole(sep(p)) for p in pp]
    finally:
        model.set_gemm_mode(-1)
    yard = max((a - b).abs().max().item() for a, b in zip(m1, m2))
    separate = [sep(p) for p in pp]
    shared = model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_score_values=True)
    plain = model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common, return_score_attention=True)
    torch.cuda.synchronize()
    dist = max((whole(s) - whole(f)).abs().max().item() for s, f in zip(shared, separate))
    print(f"stage {stage}: shared-prefix distance of the values {dist:.3e}, GEMM-mode yardstick {yard:.3e}")
    for s, f, pl in zip(shared, separate, plain):
        assert tuple(s["score_values"].shape) == tuple(f["score_values"].shape) and (s["score_values_rest"] == 0).all()
        assert torch.equal(bits(s["score_attention"]), bits(pl["score_attention"]))           # the bins keep their bits beside the values
    assert dist <= 1.3 * yard


def test_model_graph_replay_runs_the_call_eagerly():
    model, cfg, sd, kw, base, on = flagged(2)
    dev_kw = lambda seed: dict(kw, pixel_values=synth.synthetic_frames(3, 224, seed=seed).cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    seeds = [431, 432, 433]
    eager = [model(**dev_kw(s), return_score_values=True) for s in seeds]
    torch.cuda.synchronize()
    assert not torch.equal(eager[0]["score_values"], eager[1]["score_values"])
    model.enable_graph_replay(True)
    try:
        before = dict(model._graphs)
        for s, e in zip(seeds + seeds, eager + eager):
            r = model(**dev_kw(s), return_score_values=True)
            for k in ("score_values", "score_values_rest", "score_attention", "score1"):
                assert torch.equal(bits(r[k]), bits(e[k])), k
        assert dict(model._graphs) == before, "a call with return_score_values captured a graph"
    finally:
        model.enable_graph_replay(False)


def test_model_refusals(lib):
    model, cfg, sd, kw, base = G.rig(2)
    many, _ = G.two_clips(cfg, 900, frames=(1,) * 65)
    with pytest.raises(ValueError, match="at most 64"):
        model(**many, return_score_values=True)
    drop = torch.zeros_like(kw["input_ids"], dtype=torch.bool)
    drop[:, 20] = True
    with pytest.raises(ValueError, match="return_score_values"):
        model(**kw, return_score_values=True, key_drop=drop)
    ctx, llm = model._ctx, cfg.llm_config
    seg = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert lib.aigv_score_attention_arm_values(ctx, native.i32_array([0]), 1, seg.data_ptr(), None, 0, 3, out.data_ptr(), None, 0, None) == -1      # null val_out_dev
    assert "null val_out_dev" in lib.aigv_last_error(ctx).decode()
    assert lib.aigv_score_attention_arm_values(ctx, native.i32_array([0]), 1, seg.data_ptr(), None, 0, 3, out.data_ptr(), None, 5, out.data_ptr()) == -1
    assert "score_values" not in model(**kw) and float(out.abs().sum()) == 0.0     # neither refusal armed the context


# ---- completeness against the pass's own flash output ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_bar(stage):
    """Per layer, e_ref: the distance, on the SAME tiny model and clips, between the composed oracle's bf16 head capture at the probe rows
    (head_patch_reference.composed_states, capture=) and the float64 decomposition of the oracle's own wqkv outputs (taken through
    LLM_LINEAR_HOOK; rotated with the oracle's own RoPE) - what bf16 attention arithmetic alone puts between a head output and its exact split."""
    import head_patch_reference as HP
    model, cfg, sd, kw, base, on = flagged(stage)
    llm = cfg.llm_config
    L, nh, nkv, d = llm.num_hidden_layers, llm.num_attention_heads, llm.num_key_value_heads, llm.head_dim
    g = nh // nkv
    mask = probe_mask(model, kw)
    inputs = dict({k: v for k, v in kw.items() if k != "labels"}, img_context_token_id=model.img_context_token_id)
    rec = {}

    def hook(x, w, layer, name):
        y = F.linear(x, w)
        if name == "wqkv":
            rec[layer] = y
        return y

    O.LLM_LINEAR_HOOK = hook
    try:
        DL.composed_states(sd, cfg, **inputs)
    finally:
        O.LLM_LINEAR_HOOK = None
    _, cap = HP.composed_states(sd, cfg, **inputs, capture=(mask, (0, L)))            # [B, L, n_heads, D] bf16
    N = kw["input_ids"].shape[1]
    cos, sin = O.rope_tables(d, llm.rope_theta, N, BF, llm.max_position_embeddings, llm.rope_scaling)
    pos = torch.arange(N, dtype=torch.long).unsqueeze(0)
    e_ref = torch.zeros(L, dtype=torch.float64)
    for l in range(L):
        for b in range(mask.shape[0]):
            t = int(mask[b].nonzero())
            qkv = rec[l][b:b + 1].view(1, N, nkv, g + 2, d)
            q, k = O.apply_rope(qkv[..., :g, :].reshape(1, N, nh, d).transpose(1, 2), qkv[..., g, :].transpose(1, 2), cos, sin, pos)
            truth, _ = VR.row_truth(q[0, :, t].double(), k[0].transpose(0, 1)[:t + 1].double(), qkv[0, :t + 1, :, g + 1], torch.zeros(t + 1, dtype=torch.int32), 1)
            e_ref[l] = max(e_ref[l], (cap[b, l].double() - truth.sum(1)).abs().max())
    return e_ref


@pytest.mark.parametrize("stage", [2, 1])
def test_model_the_slots_sum_to_the_pass_own_head_output(stage):
    """In ONE pass with ``return_heads`` at the probe rows: score_values.sum(3) + score_values_rest against heads.float(), per layer.  The two
    differ by the flash kernel's bf16 roundings; the bar is measured on the oracle side (oracle_bar), per layer 2 e_ref + 2e-3 - the factor and the
    floor of attention_reference.check_sequence."""
    model, cfg, sd, kw, base, on = flagged(stage)
    e_ref = oracle_bar(stage)
    idx = on["heads_index"].cpu()
    assert idx[:, 0].tolist() == [0, 1]
    total = (on["score_values"].sum(3) + on["score_values_rest"]).double().cpu()        # [B, L, n_heads, D]
    heads = on["heads"].float().double().cpu()
    dist = (total - heads).abs().amax((0, 2, 3))
    for l in range(dist.numel()):
        print(f"stage {stage} layer {l}: |sum of slots - heads| = {dist[l].item():.3e}, e_ref = {e_ref[l].item():.3e}, bar = {2 * e_ref[l].item() + 2e-3:.3e}")
    assert (dist <= 2 * e_ref + 2e-3).all()


@pytest.mark.parametrize("stage", [2, 1])
def test_model_source_writes_add_up_to_the_heads_write_along_a_direction(stage):
    """source_writes(...).sum over (heads, sources) along a direction equals <direction, wo_l . heads_row> from the ``return_heads`` capture,
    within the completeness bar pushed through |direction @ wo_l| (its 1-norm times the per-element bar) plus the fp32 roundoff of both dots."""
    model, cfg, sd, kw, base, on = flagged(stage)
    e_ref = oracle_bar(stage)
    llm = cfg.llm_config
    H, nh, d = llm.hidden_size, llm.num_attention_heads, llm.head_dim
    gen = torch.Generator().manual_seed(90 + stage)
    for direction in (torch.randn(H, generator=gen), torch.randn(2, H, generator=gen)):
        got = eval_utils.source_writes(model, on, direction.cuda())
        assert tuple(got.shape) == (2, llm.num_hidden_layers, nh, on["score_values"].shape[3]) and got.dtype == torch.float32
        norms = eval_utils.source_writes(model, on)
        sal = eval_utils.frame_write_saliency(norms)
        assert tuple(norms.shape) == (2, llm.num_hidden_layers, got.shape[-1]) and tuple(sal.shape) == (2, 2) and sal[1, 1] == 0
        assert torch.allclose(sal.sum(-1).cpu(), torch.ones(2), atol=1e-6)
        for l in range(llm.num_hidden_layers):
            wo = sd[f"language_model.model.layers.{l}.attention.wo.weight"].to(BF).double()
            dw = direction.double().expand(2, H) @ wo                                        # [B, n_heads D]
            want = (dw * on["heads"][:, l].float().double().cpu().reshape(2, nh * d)).sum(-1)
            bar = dw.abs().sum(-1) * (2 * e_ref[l] + 2e-3 + 2 * (H + nh * d) * 2.0 ** -24 * on["heads"][:, l].float().abs().max().item())
            err = (got[:, l].double().sum((1, 2)).cpu() - want).abs()
            print(f"stage {stage} layer {l}: |sum of writes - heads' write| / bar = {(err / bar).max().item():.4f}")
            assert (err <= bar).all(), l
