"""Patch occlusion inside InternViT on the MI355X: the NON-causal key-drop form of the prefill flash kernel.  Op level through
aigv_op_attention_nc_drop on the cases and patterns of tests/vit_key_drop_reference.py: the masked key census and one-hot selector (bit-exact,
both score numerics), random data against float64 under the project's own bar (attention_reference.check_sequence), the empty mask against
aigv_op_attention_ex, a per-sequence mask, the 8-wave form, the lead-key knob, fencing, NaN where nothing may read, the refusals.  Model level
(``model.vit_tokens(patch_drop=...)`` on the tiny towers of tests/test_gpu_vit_attention.py: 224 x 224, S = 257, LayerNorm without QK-norm and
RMSNorm with it): the empty mask, invisibility of the hidden patches' pixels, per-frame masks across a ``vit_chunk`` boundary, layer windows
against the masked eager stack, disarming, the map + mask refusal, and ``eval_utils.patch_occlusion``.

Model-level bar restated from tests/test_gpu_e2e.py (test_stage2_tiny_224, the ViT tokens against the oracle): mean |d| <= 0.01 and max |d| <=
0.25 of the expected tokens' mean size.  tests/test_vit_key_drop_cpu.py holds, without a GPU, the conditions the constructions rest on and that
the window mask used here moves the eager tokens by several times that bar."""
import numpy as np
import pytest
import torch

import vit_key_drop_reference as V
from attention_exact_reference import BF
from test_gpu_vit_attention import FLAVOURS, L, frames65, same_bits, vrig, weights      # the tiny towers (helpers only)
from test_vit_key_drop_cpu import MAX_TOL, MEAN_TOL, WINDOW, window_mask

from aigv_assessor_amd import eval_utils, native

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5          # a NaN bit pattern no kernel produces
POISON = 0x7FB3            # NaN: rows nothing may read
PAD = 3                    # sentinel rows in front of and behind the output, poisoned rows behind the pack
AIGV_ERR_ARG = -1
G_M, T_M = 16, 8           # the tiny towers' patch grid and token grid


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(t):
    d = t.cuda().contiguous()
    _KEEP.append(d)
    return d


def sync(rc):
    native.check(rc)
    torch.cuda.synchronize()


def pattern(shape, bits):
    t = torch.full(shape, bits, dtype=torch.int16, device="cuda").view(BF)
    _KEEP.append(t)
    return t


class Staged:
    """One case's tensors on the device: the fused rows [tokens, 2 x (q | K | V) x D] are q, k and v at once, NaN rows behind the last sequence."""

    def __init__(self, case, data, fused=None):
        c = self.case = case
        self.D = c.D
        self.ld = c.hk * (c.g + 2) * c.D
        rows = data.fused() if fused is None else fused
        poison = torch.full((PAD, self.ld), POISON, dtype=torch.int16).view(BF)
        self.x = dev(torch.cat([rows, poison]))
        self.T = sum(c.cnts)
        self.cu = dev(torch.tensor([0] + list(np.cumsum(c.cnts)), dtype=torch.int32))

    def args(self, out, round_scores, lead_key=False, **over):
        c, D = self.case, self.D
        a = dict(q=self.x.data_ptr(), k=self.x.data_ptr() + c.g * D * 2, v=self.x.data_ptr() + (c.g + 1) * D * 2, o=out.data_ptr() + PAD * c.h * D * 2, cu=native.ptr(self.cu),
                 n_seq=len(c.cnts), max_len=max(c.cnts), kv_seq_stride=0, kv_off=None, head_dim=D, flags=(4 if round_scores else 0) | (8 if lead_key else 0), q_tail=0)
        a.update(over)
        return (a["q"], self.ld, a["k"], self.ld, a["v"], self.ld, a["o"], c.h * D, a["cu"], a["n_seq"], a["max_len"], c.h, c.hk, (c.g + 2) * D, (c.g + 2) * D,
                a["kv_seq_stride"], a["kv_off"], a["head_dim"], a["flags"], c.post, c.pre, None, None, None, 0, a["q_tail"])

    def attend(self, lib, words, round_scores, plain=False, lead_key=False):
        """-> the WHOLE output allocation [PAD + T + PAD, h * D]; the word buffer holds exactly n_seq * ld_drop words."""
        out = pattern((self.T + 2 * PAD, self.case.h * self.D), SENTINEL)
        a = self.args(out, round_scores, lead_key)
        if plain:
            sync(lib.aigv_op_attention_ex(*a, None))
        else:
            w = dev(words)
            assert w.numel() == len(self.case.cnts) * words.shape[1]
            sync(lib.aigv_op_attention_nc_drop(*a, w.data_ptr(), words.shape[1], None))
        return out


def expect_whole(expect):
    e = expect.reshape(expect.shape[0], -1)
    pad = torch.full((PAD, e.shape[1]), SENTINEL, dtype=torch.int16)
    return torch.cat([pad, e, pad])


def assert_bits(got, want, case, what):
    got = got.cpu().view(torch.int16)
    if torch.equal(got, want):
        return
    h, D = case.h, case.D
    bad = (got != want).view(got.shape[0], h, D)
    rows = bad.any(-1).any(-1).nonzero().flatten()
    r = int(rows[0])
    hq = int(bad[r].any(-1).nonzero()[0])
    cols = bad[r, hq].nonzero().flatten().tolist()[:4]
    g16, w16 = got.view(-1, h, D)[r, hq], want.view(-1, h, D)[r, hq]
    raise AssertionError(f"{case.name} {what}: {int(bad.sum())} elements of {len(rows)} rows differ; first: allocation row {r} (PAD = {PAD}) head {hq} columns "
                         f"{cols}: got {[hex(int(g16[c]) & 0xffff) for c in cols]} want {[hex(int(w16[c]) & 0xffff) for c in cols]}; rows {rows.tolist()[:12]}")


def tuned(lib, knob):
    sync(lib.aigv_tune_attention(knob))


# =================================================================================================================================
# op level
# =================================================================================================================================
@pytest.mark.parametrize("construction", ["census", "selector"])
@pytest.mark.parametrize("name", V.CASE_IDS)
def test_op_masked_census_and_selector_are_exact(lib, name, construction):
    """1.  Every un-dropped key counted once by every row and no dropped one; the chosen V row with every dropped key a decoy that ties it.  Over
    the nine patterns: bits on the lane boundaries, a range across tile borders, whole tiles (the skip, also as the first tile of a key-split
    wave's walk), the ragged last tile left without a visible key, every key but 0, nothing, key 0, every key (zero rows), one mask per sequence.
    Both score numerics; the whole allocation is compared, so the sentinel pads are too."""
    case = V.make_case(name)
    ld = V.words_needed(case)
    for pat in V.PATTERNS:
        drops = V.drop_sets(case, pat)
        data = (V.census if construction == "census" else V.selector)(case, drops)
        st = Staged(case, data)
        words = V.drop_words(drops, ld)
        for rs in (True, False):
            assert_bits(st.attend(lib, words, rs), expect_whole(data.expect), case, f"{construction} pattern {pat} round_scores {rs}")
        _KEEP.clear()


def test_op_eight_wave_form_once(lib):
    """2.  aigv_tune_attention(8) at [257, 257]: 256-row workgroups, no key split - the same census and selector bits."""
    case = V.make_case(V.EIGHT_WAVES)
    ld = V.words_needed(case)
    try:
        tuned(lib, 8)
        for pat in V.PATTERNS:
            drops = V.drop_sets(case, pat)
            for make in (V.census, V.selector):
                data = make(case, drops)
                assert_bits(Staged(case, data).attend(lib, V.drop_words(drops, ld), False), expect_whole(data.expect), case, f"8 waves {make.__name__} pattern {pat}")
            _KEEP.clear()
    finally:
        tuned(lib, 0)


@pytest.mark.parametrize("name", V.CASE_IDS)
def test_op_empty_mask_has_the_bits_of_the_unmasked_kernel(lib, name):
    """3.  Pattern (f) through the masked form against aigv_op_attention_ex on the same random inputs: the same bits, whole allocation, both score
    numerics and both wave counts."""
    case = V.make_case(name)
    st = Staged(case, V.random_case(case))
    words = V.drop_words(V.drop_sets(case, "f"), V.words_needed(case))
    try:
        for knob in (0, 8):
            tuned(lib, knob)
            for rs in (True, False):
                a, b = st.attend(lib, words, rs), st.attend(lib, None, rs, plain=True)
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (knob, rs)
                assert not (a.view(torch.int16)[PAD:PAD + st.T] == SENTINEL).any()
    finally:
        tuned(lib, 0)


@pytest.mark.parametrize("name", V.LEAD_KEY)
def test_op_lead_key_knob_changes_no_bit_of_the_masked_form(lib, name):
    """4.  Key counts 64 j + 1 with the lead-key bit set: the masked form runs without the lead key, so its output has the bits it has with the
    bit clear - and, under the empty mask, those of the unmasked kernel with the bit clear."""
    case = V.make_case(name)
    st = Staged(case, V.random_case(case))
    ld = V.words_needed(case)
    for pat in "adf":
        words = V.drop_words(V.drop_sets(case, pat), ld)
        for rs in (True, False):
            off, on = st.attend(lib, words, rs), st.attend(lib, words, rs, lead_key=True)
            assert torch.equal(on.view(torch.int16), off.view(torch.int16)), (pat, rs)
            if pat == "f":
                assert torch.equal(on.view(torch.int16), st.attend(lib, None, rs, plain=True).view(torch.int16)), rs


@pytest.mark.parametrize("name", V.CASE_IDS)
def test_op_random_data_against_float64_under_the_projects_bar(lib, name):
    """5.  attention_reference.check_sequence per sequence: at least as accurate against the float64 masked softmax as the eager bf16 restatement.
    Sequences left without a visible key are zeros on both sides and compared as such."""
    case = V.make_case(name)
    data = V.random_case(case)
    st = Staged(case, data)
    ld = V.words_needed(case)
    for pat in [p for p in V.PATTERNS if p != "f"]:
        drops = V.drop_sets(case, pat)
        words = V.drop_words(drops, ld)
        refs = [(V.masked_attention(data.q[s], data.k[s], data.v[s], drops[s], case.pre, torch.float64),
                 V.masked_attention(data.q[s], data.k[s], data.v[s], drops[s], case.pre, BF).double()) for s in range(len(case.cnts))]
        for rs in (True, False):
            out = st.attend(lib, words, rs)
            whole = out.cpu().view(torch.int16)
            assert (whole[:PAD] == SENTINEL).all() and (whole[PAD + st.T:] == SENTINEL).all()
            got = out[PAD:PAD + st.T].cpu().double().view(st.T, case.h, case.D)
            row = 0
            for s, n in enumerate(case.cnts):
                if V.visible_count(drops[s]) == 0:
                    assert (whole[PAD + row:PAD + row + n] == 0).all(), (pat, s)
                else:
                    V.check_sequence(got[row:row + n], *refs[s])
                row += n


@pytest.mark.parametrize("name", ["nc-200-64-1-d64", "nc-257x2-d128"])
def test_op_per_sequence_masks_stay_with_their_sequence(lib, name):
    """6.  Pattern (i): the unmasked sequence keeps the bits the unmasked kernel gives it, and every sequence alone - its own words in a launch of
    its own - keeps the bits it has in the pack."""
    case = V.make_case(name)
    data = V.random_case(case)
    st = Staged(case, data)
    drops = V.drop_sets(case, "i")
    assert not drops[1].any() and drops[0].any()
    ld = V.words_needed(case)
    for rs in (True, False):
        pack = st.attend(lib, V.drop_words(drops, ld), rs).cpu().view(torch.int16)[PAD:PAD + st.T]
        plain = st.attend(lib, None, rs, plain=True).cpu().view(torch.int16)[PAD:PAD + st.T]
        row = 0
        for s, n in enumerate(case.cnts):
            if s == 1:
                assert torch.equal(pack[row:row + n], plain[row:row + n]), rs
            elif drops[s].any():
                assert not torch.equal(pack[row:row + n], plain[row:row + n]), (rs, s)
            one = V.ExactCase(f"{case.name}-seq{s}", case.D, False, 2, 2, [0], [n])
            alone = Staged(one, V.ExactData(one, [data.q[s]], [data.k[s]], [data.v[s]], None))
            got = alone.attend(lib, V.drop_words([drops[s]], V.words_needed(one)), rs).cpu().view(torch.int16)[PAD:PAD + n]
            assert torch.equal(got, pack[row:row + n]), (rs, s)
            row += n


def test_op_fences_and_nan_where_nothing_may_read(lib):
    """7.  The word buffer is exactly n_seq * ld_drop words at the SMALLEST ld_drop the check admits; the K / V rows behind the pack are NaN (the
    ragged last tile re-reads its last VALID row, never the next one); and with NaN in the V rows of every OTHER sequence a sequence keeps its bits."""
    for name in ("nc-200-64-1-d64", "nc-257x2-d128"):
        case = V.make_case(name)
        drops = V.drop_sets(case, "d")
        data = V.census(case, drops)
        ld = V.words_needed(case)
        words = V.drop_words(drops, ld)
        assert words.numel() == len(case.cnts) * ld and ld == -(-max(case.cnts) // 64)
        out = Staged(case, data).attend(lib, words, False)
        assert_bits(out, expect_whole(data.expect), case, "fence")
        rnd = V.random_case(case)
        base = Staged(case, rnd).attend(lib, words, False).cpu().view(torch.int16)
        row = 0
        for s, n in enumerate(case.cnts):
            fused = rnd.fused().clone().view(-1, case.hk, case.g + 2, case.D)
            other = torch.ones(fused.shape[0], dtype=torch.bool)
            other[row:row + n] = False
            fused.view(torch.int16)[other, :, case.g + 1] = POISON                # V of the other sequences
            got = Staged(case, rnd, fused.view(-1, case.hk * (case.g + 2) * case.D)).attend(lib, words, False).cpu().view(torch.int16)
            assert torch.equal(got[PAD + row:PAD + row + n], base[PAD + row:PAD + row + n]), (name, s)
            row += n


def test_op_refusals_come_with_a_message_and_no_launch(lib):
    """8.  AIGV_ERR_ARG and a message naming the entry, nothing launched; then a clean launch.  The causal entry keeps refusing the same calls."""
    case = V.make_case("nc-257x2-d64")
    drops = V.drop_sets(case, "a")
    data = V.census(case, drops)
    st = Staged(case, data)
    ld = V.words_needed(case)
    words = dev(V.drop_words(drops, ld + 1))
    out = pattern((st.T + 2 * PAD, case.h * case.D), SENTINEL)
    fake = dev(torch.zeros(2, dtype=torch.int32))

    def refused(word, key_drop=words.data_ptr(), ld_drop=ld + 1, entry="aigv_op_attention_nc_drop", **over):
        rc = getattr(lib, entry)(*st.args(out, False, **over), key_drop, ld_drop, None)
        msg = (lib.aigv_last_error(None) or b"").decode()
        assert rc == AIGV_ERR_ARG and word in msg and msg.startswith(entry + ":"), (rc, msg)

    refused("causal != 0", flags=1)
    refused("ld_drop", ld_drop=ld - 1)
    refused("ld_drop", ld_drop=0)
    refused("8-byte aligned", key_drop=words.data_ptr() + 4, ld_drop=ld)
    refused("packed layout", kv_seq_stride=64 * 300)
    refused("packed layout", kv_off=native.ptr(fake), kv_seq_stride=64 * 300)
    refused("q_tail", q_tail=4)
    refused("causal head_dim 128", entry="aigv_op_attention_drop")                   # non-causal d = 64 through the causal entry: its old words
    refused("causal head_dim 128", entry="aigv_op_attention_drop", flags=1)          # causal d = 64
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == SENTINEL).all()                                  # nothing was launched
    assert_bits(st.attend(lib, V.drop_words(drops, ld), False), expect_whole(data.expect), case, "after the refusals")


# =================================================================================================================================
# model level: the tiny towers of tests/test_gpu_vit_attention.py (three layers at 224 x 224, a 16 x 16 patch grid, S = 257, two heads of 64)
# =================================================================================================================================
def some_patches(n_frames, seed=0):
    """A region that cuts through cells (patch rows 3..6 x columns 5..8) plus scattered single patches, per frame."""
    gen = torch.Generator().manual_seed(500 + seed)
    pd = torch.rand(n_frames, G_M, G_M, generator=gen) < 0.06
    pd[:, 3:7, 5:9] = True
    return pd


def clean_cells(pd):
    """bool [F, T * T]: the visual tokens whose cell holds no hidden patch."""
    return ~pd.view(-1, T_M, 2, T_M, 2).any(4).any(2).reshape(-1, T_M * T_M)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_empty_mask_and_full_window_are_the_plain_call(flavour):
    model, cfg, sd, kw = vrig(flavour)
    pv = kw["pixel_values"]
    tokens = model.vit_tokens(pv)
    none = torch.zeros(3, G_M, G_M, dtype=torch.bool)
    assert same_bits(model.vit_tokens(pv, patch_drop=none), tokens)
    assert same_bits(model.vit_tokens(pv, patch_drop=none, patch_drop_layers=(1, 2)), tokens)
    pd = some_patches(3)
    masked = model.vit_tokens(pv, patch_drop=pd)
    assert not same_bits(masked, tokens) and torch.isfinite(masked.float()).all()
    assert same_bits(model.vit_tokens(pv, patch_drop=pd, patch_drop_layers=(0, L)), masked)      # the window (0, n) is None
    assert same_bits(model.vit_tokens(pv), tokens)                                               # the pass after an armed pass runs unmasked
    for bad in (pd.long(), pd[:2], pd[:, :, :-1], pd.view(3, -1), [[True]]):
        with pytest.raises(ValueError, match="patch_drop"):
            model.vit_tokens(pv, patch_drop=bad)
    for bad in ((0, 0), (2, 1), (-1, 2), (0, L + 1), (1,), 3):
        with pytest.raises(ValueError, match="layers the pass runs"):
            model.vit_tokens(pv, patch_drop=pd, patch_drop_layers=bad)
    with pytest.raises(ValueError, match="needs one"):
        model.vit_tokens(pv, patch_drop_layers=(0, 1))
    keep = model._capture_keep                                                                   # never inside a graph capture
    try:
        model._capture_keep = []
        with pytest.raises(RuntimeError, match="graph capture"):
            model.vit_tokens(pv, patch_drop=pd)
    finally:
        model._capture_keep = keep
    assert same_bits(model.vit_tokens(pv), tokens)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_hidden_patches_are_invisible_to_the_rest_of_the_frame(flavour):
    """Exact and reference-free: with a set P of patches dropped in every layer, other (finite) pixels under P change no bit of any token whose cell
    holds no patch of P - no row outside P ever reads a row of P.  Without the mask the same replacement does change those tokens."""
    model, cfg, sd, kw = vrig(flavour)
    pv = kw["pixel_values"]
    pd = some_patches(3, seed=1)
    pv2 = pv.clone()
    under = pd.repeat_interleave(14, 1).repeat_interleave(14, 2)[:, None].expand_as(pv)
    pv2[under] = (-pv.float()[under] * 0.7 + 0.3).to(pv.dtype)
    assert not torch.equal(pv2[under], pv[under]) and torch.equal(pv2[~under], pv[~under]) and torch.isfinite(pv2.float()).all()
    a, b = model.vit_tokens(pv, patch_drop=pd), model.vit_tokens(pv2, patch_drop=pd)
    clean = clean_cells(pd).cuda()
    assert int(clean.sum()) > 3 * 20 and int((~clean).sum()) >= 3 * 4
    assert torch.equal(a[clean].view(torch.int16), b[clean].view(torch.int16))
    assert all(not torch.equal(a[f][~clean[f]], b[f][~clean[f]]) for f in range(3))             # the hidden patches' own rows still carry their pixels
    plain_a, plain_b = model.vit_tokens(pv), model.vit_tokens(pv2)
    changed = (plain_a != plain_b).any(-1)
    assert bool((changed & clean).any(1).all()) and int((changed & clean).sum()) > int(clean.sum()) // 2      # unmasked, the clean cells do read P


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_per_frame_masks_across_a_chunk_boundary(flavour):
    """65 frames, one mask each: vit_chunk is 64, so frame 64 runs as a chunk of its own and must read ITS words - each frame equal to itself alone."""
    model, cfg, sd, kw = vrig(flavour)
    pv = frames65()
    pd = some_patches(65, seed=2)
    pd[63, 8:, :] = True
    pd[64, :, 8:] = True
    both = model.vit_tokens(pv, patch_drop=pd)
    for f in (0, 63, 64):
        assert same_bits(model.vit_tokens(pv[f:f + 1], patch_drop=pd[f:f + 1])[0], both[f]), f
    assert not same_bits(model.vit_tokens(pv[64:65], patch_drop=pd[63:64])[0], both[64])        # (frame 64 under frame 63's words is something else)
    assert same_bits(model.vit_tokens(pv), model.vit_tokens(pv, patch_drop=torch.zeros_like(pd)))


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_model_window_against_the_masked_eager_stack(flavour):
    """The window (1, 3) and the whole depth against tests/vit_key_drop_reference.masked_vit_forward (bf16, the reference's rounding points) under
    the bar of the existing ViT comparison; the CPU file shows that ignoring the mask or the window misses it by a factor."""
    from oracle import oracle as O
    model, cfg, sd, kw = vrig(flavour)
    pv = kw["pixel_values"]
    pd = window_mask(3)
    for window in (WINDOW, None):
        got = model.vit_tokens(pv, patch_drop=pd, patch_drop_layers=window).float().cpu()
        want = O.shuffled_tokens(V.masked_vit_forward(O, weights(flavour), cfg, pv, pd, window)).float()
        assert got.shape == want.shape and torch.isfinite(got).all()
        scale = want.abs().mean().clamp_min(1e-6)
        err = (got - want).abs()
        print(f"{flavour} window {window}: mean rel err {(err.mean() / scale).item():.4g} (bar {MEAN_TOL}), max rel err {(err.max() / scale).item():.4g} (bar {MAX_TOL})")
        assert err.mean() / scale <= MEAN_TOL and err.max() / scale <= MAX_TOL


def test_model_refused_pass_disarms_and_the_map_refuses_a_mask(lib):
    model, cfg, sd, kw = vrig("plain")
    pv = kw["pixel_values"]
    tokens = model.vit_tokens(pv)
    _, ctx = model._native(n_frames=3)
    words = dev(V.patch_words_naive(some_patches(3)))
    ld = int(words.shape[1])
    for lo, hi in ((0, L + 1), (1, 1), (-1, 1), (2, 1)):                                        # the C ABI's own refusal: the pass knows how many layers it runs
        native.check(lib.aigv_vit_key_drop_arm(ctx, words.data_ptr(), ld, lo, hi), ctx)
        with pytest.raises(native.NativeError, match="layers the pass runs"):
            model.vit_tokens(pv)
        torch.cuda.synchronize()
        assert same_bits(model.vit_tokens(pv), tokens)                                          # the refused pass disarmed: a plain pass runs
    for args, word in (((None, ld, 0, 1), "null words_dev"), ((words.data_ptr() + 4, ld, 0, 1), "8-byte aligned"), ((words.data_ptr(), ld - 1, 0, 1), "ld_words")):
        assert lib.aigv_vit_key_drop_arm(ctx, *args) == AIGV_ERR_ARG and word in lib.aigv_last_error(ctx).decode()
    assert same_bits(model.vit_tokens(pv), tokens)                                              # a refused arm arms nothing
    att = torch.empty(3, 1, 257, 257, dtype=torch.float32, device="cuda")
    native.check(lib.aigv_vit_attention_arm(ctx, att.data_ptr(), 0, 1, 0), ctx)
    native.check(lib.aigv_vit_key_drop_arm(ctx, words.data_ptr(), ld, 0, L), ctx)
    with pytest.raises(native.NativeError, match="does not know the mask"):
        model.vit_tokens(pv)
    torch.cuda.synchronize()
    assert same_bits(model.vit_tokens(pv), tokens)                                              # both disarmed
    with pytest.raises(TypeError):
        model.vit_attention(pv, patch_drop=some_patches(3))                                     # vit_attention does not take the option


def test_patch_occlusion_sweep(monkeypatch):
    """Two clips (two frames and one), cell = half the token grid: shapes, NaN for the missing frame, every variant equal to a by-hand
    vit_tokens(patch_drop=...) + forward(visual_tokens=..., key_drop=...), and delta == 0 exactly for an empty block mask."""
    model, cfg, sd, kw = vrig("plain")
    cell = T_M // 2
    res = eval_utils.patch_occlusion(model, cell=cell, **kw)
    B, F, nb = 2, 2, 2
    assert set(res) == {"outs", "blocks", "score1", "control", "occluded", "delta"}
    assert res["blocks"].dtype == torch.bool and tuple(res["blocks"].shape) == (nb, nb, T_M, T_M) and (res["blocks"].sum((0, 1)) == 1).all()
    assert len(res["outs"]) == 1 + F * (nb * nb + 1)
    assert tuple(res["score1"].shape) == (B,) and tuple(res["control"].shape) == (B, F) and tuple(res["occluded"].shape) == tuple(res["delta"].shape) == (B, F, nb, nb)
    occ, ctl = res["occluded"].cpu(), res["control"].cpu()
    assert torch.isnan(occ[1, 1]).all() and torch.isnan(ctl[1, 1]) and torch.isnan(res["delta"][1, 1]).all()      # clip 1 has one frame
    assert torch.isfinite(occ[0]).all() and torch.isfinite(occ[1, 0]).all()
    base = model(**kw)
    assert same_bits(res["score1"], base["score1"].float()) and same_bits(res["outs"][0]["score1"], base["score1"])
    assert torch.equal(ctl[0], res["score1"].cpu()[:1].expand(2)) and ctl[1, 0] == res["score1"].cpu()[1]          # (lead-key knob off: the control is the base)
    assert (res["delta"].cpu()[0] != 0).any()
    # by hand
    pv = kw["pixel_values"]
    common = {k: v for k, v in kw.items() if k != "pixel_values"}
    base_tokens = model.vit_tokens(pv)
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"], n_frames=3)
    frame_of = {(0, 0): 0, (0, 1): 1, (1, 0): 2}
    for f in range(F):
        clips = [b for b in range(B) if (b, f) in frame_of]
        for i in range(nb * nb + 1):
            tokens = base_tokens.clone()
            keys = torch.zeros_like(kw["attention_mask"], dtype=torch.bool)
            for b in clips:
                src = frame_of[(b, f)]
                pd = torch.zeros(1, G_M, G_M, dtype=torch.bool)
                if i > 0:
                    r, c = divmod(i - 1, nb)
                    pd[0, 2 * cell * r:2 * cell * (r + 1), 2 * cell * c:2 * cell * (c + 1)] = True
                    where = units[b, f].nonzero().flatten().view(T_M, T_M)[cell * r:cell * (r + 1), cell * c:cell * (c + 1)]
                    keys[b, where.flatten()] = True
                tokens[src] = model.vit_tokens(pv[src:src + 1], patch_drop=pd)[0]
            want = model(visual_tokens=tokens, **(dict(key_drop=keys) if i > 0 else {}), **common)
            got = res["outs"][1 + f * (nb * nb + 1) + i]
            assert set(got) == set(want) and all(v is None or same_bits(got[k], v) for k, v in want.items()), (f, i)
            if i > 0:
                r, c = divmod(i - 1, nb)
                for b in clips:
                    assert occ[b, f, r, c] == want["score1"].float().cpu()[b]
    # the same sweep without the token masks, and then with EMPTY block masks: no patch is hidden, the variants are their control
    loose = eval_utils.patch_occlusion(model, cell=cell, hide_tokens=False, frames=[1], **kw)
    assert torch.isnan(loose["occluded"].cpu()[:, 0]).all() and torch.isfinite(loose["occluded"].cpu()[0, 1]).all() and len(loose["outs"]) == 1 + nb * nb + 1
    assert not torch.equal(loose["occluded"].cpu()[0, 1], occ[0, 1])
    monkeypatch.setattr(eval_utils, "cell_patches", lambda cells: torch.zeros(*cells.shape[:-2], 2 * cells.shape[-2], 2 * cells.shape[-1], dtype=torch.bool))
    empty = eval_utils.patch_occlusion(model, cell=cell, hide_tokens=False, **kw)
    d = empty["delta"].cpu()
    assert (d[0] == 0).all() and (d[1, 0] == 0).all() and torch.isnan(d[1, 1]).all()
    for bad in (3, 0, 16):
        with pytest.raises(ValueError, match="cell"):
            eval_utils.patch_occlusion(model, cell=bad, **kw)
    with pytest.raises(ValueError, match="frames"):
        eval_utils.patch_occlusion(model, cell=cell, frames=[2], **kw)
