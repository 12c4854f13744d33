"""Key-drop attention on the MI355X: the prefill flash kernel's per-key "dropped" mask (AttnArgs::key_drop) at op level through
aigv_op_attention_drop - bit-exact on the masked key census and one-hot selector of tests/key_drop_reference.py over the drop patterns,
both score numerics and both wave counts, in the packed form (with row trimming) and the cache form; an all-zero mask against
aigv_op_attention_ex; random data against float64 under the project's own bar; fencing; the refusals - and at model level on the tiny rig:
forward(key_drop=...) against oracle.forward_eval(attention_mask & ~drop), the no-op mask, a clip alone, graph replay, the refusals and
eval_utils.frame_ablation.

Score bar restated from tests/test_gpu_e2e.py (tiny configurations): |d| <= 1e-3 or <= 1 bf16 ulp of the expected value; level tokens
identical except on rows where the oracle's own top two logits lie within 2 bf16 ulps.
tests/test_key_drop_cpu.py holds, without a GPU, the conditions the constructions and the oracle comparison rest on."""
import functools

import numpy as np
import pytest
import torch

import key_drop_reference as R
from attention_exact_reference import BF
from attention_reference import check_sequence, rope_table

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5          # a NaN bit pattern no kernel produces
CACHE_FILL = 0x7FB3        # NaN: cache rows and K / V slots nothing may read
PAD = 3                    # sentinel rows in front of and behind the output
D = R.D
N_POS = 320                # rows of the rotary tables: past the longest sequence (294 keys)
AIGV_ERR_ARG = -1


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


def cu_of(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)


def tables(construction):
    """Census: the real rotary tables (a rotated zero is zero); selector: cos = 1, sin = 0 - the rotation is then the identity in bf16.  The
    queries are rotated by the kernel (fused query RoPE, computed position); K is taken as stored."""
    if construction == "census":
        return rope_table(D, N_POS)
    return torch.ones(N_POS, D // 2, dtype=BF), torch.zeros(N_POS, D // 2, dtype=BF)


class Staged:
    """One case's tensors on the device, in the packed form (fused rows are q, k and v at once; NaN rows behind the last sequence) or the
    cache form (the packed new rows with NaN K / V slots; caches [n_seq][hk][cap][D] of NaN holding every sequence's keys in rows 0 .. tot - 1)."""

    def __init__(self, case, data, rope):
        c = self.case = case
        g, hk = c.g, c.hk
        self.ld = hk * (g + 2) * D
        self.cache = bool(c.cap)
        rows = data.fused()                                                   # [sum tot, ld]
        if self.cache:
            new = rows[c.new_idx].clone().view(-1, hk, g + 2, D)
            new.view(torch.int16)[:, :, g:] = CACHE_FILL
            self.x = dev(new.view(-1, self.ld))
            self.kc, self.vc = pattern((len(c.tot), hk, c.cap, D), CACHE_FILL), pattern((len(c.tot), hk, c.cap, D), CACHE_FILL)
            for b, (k, v) in enumerate(zip(data.k, data.v)):
                self.kc[b, :, : k.shape[0]] = k.transpose(0, 1).cuda()
                self.vc[b, :, : v.shape[0]] = v.transpose(0, 1).cuda()
            self.kv_off = dev(torch.tensor(c.offs, dtype=torch.int32))
        else:
            poison = torch.full((PAD, self.ld), CACHE_FILL, dtype=torch.int16).view(BF)
            self.x = dev(torch.cat([rows, poison]))
        self.T = sum(c.cnts)
        self.cu = dev(cu_of(c.cnts))
        self.cos, self.sin = (None, None) if rope is None else (dev(rope[0]), dev(rope[1]))
        self.zeros = dev(torch.zeros(self.T, dtype=torch.int32))

    def args(self, out, round_scores, q_tail):
        """The arguments aigv_op_attention_ex and aigv_op_attention_drop share (the latter appends key_drop, ld_drop in front of the stream)."""
        c, ptr = self.case, native.ptr
        flags = 1 | (4 if round_scores else 0)
        rope = (ptr(self.zeros), ptr(self.cos), ptr(self.sin), 1) if self.cos is not None else (None, None, None, 0)
        o = out.data_ptr() + PAD * c.h * D * 2
        if self.cache:
            return (ptr(self.x), self.ld, ptr(self.kc), D, ptr(self.vc), D, o, c.h * D, ptr(self.cu), len(c.cnts), max(c.cnts), c.h, c.hk, (c.g + 2) * D,
                    c.cap * D, c.hk * c.cap * D, ptr(self.kv_off), D, flags, c.post, 1.0, *rope, q_tail)
        base = self.x.data_ptr()
        return (base, self.ld, base + c.g * D * 2, self.ld, base + (c.g + 1) * D * 2, self.ld, o, c.h * D, ptr(self.cu), len(c.cnts), max(c.cnts), c.h, c.hk,
                (c.g + 2) * D, (c.g + 2) * D, 0, None, D, flags, c.post, 1.0, *rope, q_tail)

    def attend(self, lib, words, round_scores, q_tail=0, plain=False):
        """-> the WHOLE output allocation [PAD + T + PAD, h * D]; the word buffer holds exactly n_seq * ld_drop words."""
        out = pattern((self.T + 2 * PAD, self.case.h * D), SENTINEL)
        a = self.args(out, round_scores, q_tail)
        if plain:
            sync(lib.aigv_op_attention_ex(*a, None))
        else:
            w = dev(words)
            assert w.numel() == len(self.case.cnts) * words.shape[1]
            sync(lib.aigv_op_attention_drop(*a, w.data_ptr(), words.shape[1], None))
        return out


def expect_whole(expect, written=None):
    T = expect.shape[0]
    e = expect.reshape(T, -1).clone()
    if written is not None:
        e[~written] = torch.tensor(SENTINEL, dtype=torch.int16)
    pad = torch.full((PAD, e.shape[1]), SENTINEL, dtype=torch.int16)
    return torch.cat([pad, e, pad])


def assert_bits(got, want, case, what):
    got = got.cpu().view(torch.int16)
    if torch.equal(got, want):
        return
    h = case.h
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


CASES = [("packed", g) for g in R.GROUPS] + [("cache", g) for g in R.GROUPS]


def make_case(form, g):
    return R.packed_case(g) if form == "packed" else R.cache_case(g)


def patterns_of(form):
    return [p for p in R.PATTERNS if p != "g" or form == "cache"]


# =================================================================================================================================
# op level
# =================================================================================================================================
@pytest.mark.parametrize("construction", ["census", "selector"])
@pytest.mark.parametrize("form,g", CASES)
def test_op_masked_census_and_selector_are_exact(lib, form, g, construction):
    """1.  Every un-dropped visible key counted once and no dropped one (scattered bits on the lane boundaries, a range across tile borders,
    whole tiles - the skip path -, the ragged last tile, key 0 - a first row of all-zero bits -, no bit, cached keys); the chosen V row with
    every dropped key a decoy that ties it.  Both score numerics, both wave counts, q_tail 0 and 4 (packed), fused query RoPE."""
    case = make_case(form, g)
    ld = R.words_needed(case)
    rope = tables(construction)
    try:
        for pat in patterns_of(form):
            drops = R.drop_sets(case, pat)
            data = (R.census if construction == "census" else R.selector)(case, drops)
            st = Staged(case, data, rope)
            words = R.drop_words(drops, ld)
            for knob in (0, 8):
                tuned(lib, knob)
                for rs in (True, False):
                    for q_tail in (R.Q_TAILS if form == "packed" else (0,)):
                        want = expect_whole(data.expect, R.waves_written(case.cnts, q_tail))
                        assert_bits(st.attend(lib, words, rs, q_tail), want, case, f"{construction} pattern {pat} knob {knob} round_scores {rs} q_tail {q_tail}")
            _KEEP.clear()
    finally:
        tuned(lib, 0)


@pytest.mark.parametrize("form,g", CASES)
def test_op_all_zero_words_equal_the_unmasked_kernel(lib, form, g):
    """2.  Pattern (f) through the key-drop form against aigv_op_attention_ex on the same inputs: the same bits, whole allocation."""
    case = make_case(form, g)
    data = R.random_case(case)
    st = Staged(case, data, rope_table(D, N_POS))
    words = R.drop_words(R.drop_sets(case, "f"), R.words_needed(case))
    try:
        for knob in (0, 8):
            tuned(lib, knob)
            for rs in (True, False):
                for q_tail in R.Q_TAILS:
                    a, b = st.attend(lib, words, rs, q_tail), st.attend(lib, None, rs, q_tail, plain=True)
                    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (knob, rs, q_tail)
                    assert not (a.view(torch.int16)[PAD:PAD + st.T][R.waves_written(case.cnts, q_tail).cuda()] == SENTINEL).any()
    finally:
        tuned(lib, 0)


@pytest.mark.parametrize("form,g", CASES)
def test_op_random_data_against_float64_under_the_projects_bar(lib, form, g):
    """3.  attention_reference.check_sequence per sequence: at least as accurate against the float64 masked softmax as the eager bf16
    restatement of the reference's additive mask.  Patterns that keep key 0 (the eager softmax of a fully masked row is uniform, the
    kernel's is zero: not comparable)."""
    case = make_case(form, g)
    data = R.random_case(case)
    st = Staged(case, data, None)                                             # (no rotation: q and k are used as stored on both sides)
    ld = R.words_needed(case)
    try:
        for pat in [p for p in patterns_of(form) if p not in "ef"]:
            drops = R.drop_sets(case, pat)
            words = R.drop_words(drops, ld)
            refs = [(R.masked_attention(data.q[s], data.k[s], data.v[s], case.offs[s], drops[s], R.POST, torch.float64),
                     R.masked_attention(data.q[s], data.k[s], data.v[s], case.offs[s], drops[s], R.POST, BF).double()) for s in range(len(case.cnts))]
            for knob in (0, 8):
                tuned(lib, knob)
                for rs in (True, False):
                    out = st.attend(lib, words, rs)
                    whole = out.cpu().view(torch.int16)
                    assert (whole[:PAD] == SENTINEL).all() and (whole[PAD + st.T:] == SENTINEL).all()
                    got = out[PAD:PAD + st.T].cpu().double().view(st.T, case.h, D)
                    row = 0
                    for s, n in enumerate(case.cnts):
                        check_sequence(got[row:row + n], *refs[s])
                        row += n
    finally:
        tuned(lib, 0)


def test_op_fences(lib):
    """4.  The output sits between sentinel pads (every test above compares the whole allocation); here: the word buffer is exactly
    n_seq * ld_drop words at the SMALLEST ld_drop the check admits, K / V beyond every sequence is NaN, and nothing of it shows."""
    for form in ("packed", "cache"):
        case = make_case(form, 3)
        drops = R.drop_sets(case, "d")
        data = R.census(case, drops)
        st = Staged(case, data, rope_table(D, N_POS))
        ld = R.words_needed(case)
        words = R.drop_words(drops, ld)
        assert words.numel() == len(case.cnts) * ld
        out = st.attend(lib, words, False)
        assert_bits(out, expect_whole(data.expect), case, f"fence {form}")
        assert torch.isfinite(out[PAD:PAD + st.T].float()).all()


def test_op_refusals_come_with_a_message_and_no_fault(lib):
    """5.  Every aigv_attn_check refusal of the new fields: AIGV_ERR_ARG and a message, nothing launched; then a clean launch."""
    case = R.packed_case(1)
    drops = R.drop_sets(case, "a")
    data = R.census(case, drops)
    st = Staged(case, data, None)
    ld = R.words_needed(case)
    words = dev(R.drop_words(drops, ld + 1))
    out = pattern((st.T + 2 * PAD, case.h * D), SENTINEL)
    a = list(st.args(out, False, 0))
    I_HEAD_DIM, I_CAUSAL = 17, 18

    def refused(args, key_drop, ld_drop, word):
        rc = lib.aigv_op_attention_drop(*args, key_drop, ld_drop, None)
        msg = (lib.aigv_last_error(None) or b"").decode()
        assert rc == AIGV_ERR_ARG and word in msg and "aigv_op_attention_drop" in msg, (rc, msg)

    non_causal = list(a); non_causal[I_CAUSAL] = 0
    refused(non_causal, words.data_ptr(), ld + 1, "causal head_dim 128")
    d64 = list(a); d64[I_HEAD_DIM] = 64
    refused(d64, words.data_ptr(), ld + 1, "causal head_dim 128")
    refused(a, words.data_ptr(), ld - 1, "ld_drop")
    refused(a, words.data_ptr(), 0, "ld_drop")
    refused(a, words.data_ptr() + 4, ld, "8-byte aligned")
    # the cache form: ld_drop must cover the largest key offset + the longest count, not just the longest sequence
    ccase = R.cache_case(1)
    cdrops = R.drop_sets(ccase, "g")
    cdata = R.census(ccase, cdrops)
    cst = Staged(ccase, cdata, None)
    cwords = dev(R.drop_words(cdrops, R.words_needed(ccase)))
    cout = pattern((cst.T + 2 * PAD, ccase.h * D), SENTINEL)
    ca = cst.args(cout, False, 0)
    assert -(-max(ccase.tot) // 64) < R.words_needed(ccase)
    refused(ca, cwords.data_ptr(), R.words_needed(ccase) - 1, "ld_drop")
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == SENTINEL).all() and (cout.view(torch.int16) == SENTINEL).all()      # nothing was launched
    # a clean launch afterwards, on both
    assert_bits(st.attend(lib, R.drop_words(drops, ld), False), expect_whole(data.expect), case, "after the refusals")
    assert_bits(cst.attend(lib, R.drop_words(cdrops, R.words_needed(ccase)), False), expect_whole(cdata.expect), ccase, "after the refusals (cache)")


# =================================================================================================================================
# model level
# =================================================================================================================================
FRAMES = (2, 1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32 if t.dtype == torch.float32 else t.dtype)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_model(cfg, sd, stage):
    from aigv_assessor_amd.modeling import InternVLChatModel
    m = InternVLChatModel(cfg, stage=stage)
    m.load_state_dict(sd)
    return m.eval().cuda()


def two_clips(cfg, seed, frames=FRAMES):
    ts = [synth.canonical_tokens(cfg, 1, f, seed=seed + i) for i, f in enumerate(frames)]
    n = max(t["input_ids"].shape[1] for t in ts)
    ids = torch.zeros(len(ts), n, dtype=torch.long)
    labels = torch.full((len(ts), n), -100)
    am = torch.zeros(len(ts), n, dtype=torch.bool)
    for i, t in enumerate(ts):
        k = t["input_ids"].shape[1]
        ids[i, :k], labels[i, :k], am[i, :k] = t["input_ids"][0], t["labels"][0], True
    F = sum(frames)
    return dict(pixel_values=synth.synthetic_frames(F, 224, seed=seed), input_ids=ids, attention_mask=am, image_flags=torch.ones(F, 1, dtype=torch.long),
                labels=labels, motion_feature=synth.synthetic_motion(len(ts), cfg.motion_dim, seed=seed)), ts[0]["img_context_token_id"]


@functools.lru_cache(maxsize=None)
def rig(stage):
    """The tiny rig of tests/test_key_drop_cpu.py (weights seed 61 + stage, tokens seed 300 + stage): two clips of 2 and 1 frames, N = 215.
    -> model, cfg, sd, kw, the unit masks, the plain pass, the pass with frame 0 of every clip hidden."""
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    sd = synth.make_state_dict(cfg, seed=61 + stage, rich=True)
    model = make_model(cfg, sd, stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    plain = model(**kw, return_logprobs=True)
    masked = model(**kw, return_logprobs=True, key_drop=units[:, 0])
    torch.cuda.synchronize()
    return model, cfg, sd, kw, units, plain, masked


def clip_alone(kw, b, frames=FRAMES):
    f0 = sum(frames[:b])
    n = int(kw["attention_mask"][b].sum())
    return dict(pixel_values=kw["pixel_values"][f0:f0 + frames[b]], input_ids=kw["input_ids"][b:b + 1, :n], attention_mask=kw["attention_mask"][b:b + 1, :n],
                image_flags=kw["image_flags"][f0:f0 + frames[b]], labels=kw["labels"][b:b + 1, :n], motion_feature=kw["motion_feature"][b:b + 1]), n


def score_ok(got, want):
    """tests/test_gpu_e2e.py's bar for the tiny configurations: |d| <= 1e-3 or <= 1 bf16 ulp of the expected value."""
    got, want = got.float().cpu(), want.float().cpu()
    d = (got - want).abs()
    ulp = want.abs().clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -7
    print("score1 hip", got.tolist(), "oracle", want.tolist(), f"= {(d / ulp).max().item():.2f} bf16 ulps (bar 1)")
    assert bool(((d <= 1e-3) | (d <= ulp * 1.001)).all()), f"score differs: {got.tolist()} vs {want.tolist()}"


def assert_levels(got_ids, want_ids, ref_logits_rows):
    """Identical, except rows where the ORACLE's own logits of the two tokens lie within 2 bf16 ulps (tests/test_gpu_e2e.py)."""
    bad = (got_ids != want_ids).nonzero().flatten().tolist()
    for r in bad:
        a, b = ref_logits_rows[r, want_ids[r]].item(), ref_logits_rows[r, got_ids[r]].item()
        ulp = 2.0 ** (torch.tensor(abs(a)).clamp_min(1e-30).log2().floor().item() - 7)
        print(f"level row {r}: oracle id {want_ids[r].item()} ({a}) vs hip id {got_ids[r].item()} ({b}); gap {abs(a - b) / ulp:.2f} ulp")
        assert abs(a - b) <= 2 * ulp, f"row {r}: argmax differs beyond a rounding tie"
    return len(bad)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_masked_pass_against_the_oracle(stage):
    """6.  Frame 0 of each clip hidden: oracle.forward_eval(attention_mask & ~drop), every clip on its own (hidden[:, -4] is then its score
    row), against the batched masked pass."""
    model, cfg, sd, kw, units, plain, masked = rig(stage)
    N = kw["input_ids"].shape[1]
    got_logit = masked["logit"].cpu().view(2, N - 1)
    plain_logit = plain["logit"].cpu().view(2, N - 1)
    moved = 0
    for b in range(2):
        one, n = clip_alone(kw, b)
        am = one.pop("attention_mask")
        ref = O.forward_eval(sd, cfg, attention_mask=am & ~units[b:b + 1, 0, :n], img_context_token_id=model.img_context_token_id, stage=stage,
                             return_intermediates=True, **one)
        want = ref["label"] != -100
        rows = ref["logits"][0, :-1][want]
        ties = assert_levels(got_logit[b, :n - 1][want], ref["logit"][want], rows)
        assert ties <= max(1, int(want.sum()) // 10)
        moved += int((got_logit[b, :n - 1][want] != plain_logit[b, :n - 1][want]).sum())
        if stage == 2:
            score_ok(masked["score1"][b:b + 1], ref["score1"])
    assert moved > 0                                                                          # the masked result differs from the unmasked one
    if stage == 2:
        assert not torch.equal(bits(masked["score1"]), bits(plain["score1"]))
    assert not same(masked["logprob"], plain["logprob"])


@pytest.mark.parametrize("stage", [2, 1])
def test_model_all_false_mask_changes_no_bit(stage):
    """7."""
    model, cfg, sd, kw, units, plain, masked = rig(stage)
    for empty in (torch.zeros_like(units[:, 0]), torch.zeros_like(kw["input_ids"]).cuda()):
        out = model(**kw, return_logprobs=True, key_drop=empty)
        assert set(out) == set(plain)
        for key in out:
            assert out[key] is None and plain[key] is None or same(out[key], plain[key]), key


@pytest.mark.parametrize("stage", [2, 1])
def test_model_clip_alone_is_clip_in_batch_under_a_mask(stage):
    """8."""
    model, cfg, sd, kw, units, plain, masked = rig(stage)
    N = kw["input_ids"].shape[1]
    for b in range(2):
        one, n = clip_alone(kw, b)
        alone = model(**one, return_logprobs=True, key_drop=units[b:b + 1, 0, :n])
        if stage == 2:
            assert same(alone["score1"], masked["score1"][b:b + 1]), b
        for key in ("logit", "logprob"):
            assert same(alone[key], masked[key].view(2, N - 1)[b, :n - 1]), (b, key)


def test_model_graph_replay_runs_masked_calls_eagerly():
    """9.  With replay enabled: a masked call has the eager bits and captures nothing; the unmasked calls around it keep replaying and keep
    the baseline bits; a plain pass right after a masked one is plain again (the pass disarmed)."""
    model, cfg, sd, kw, units, plain, masked = rig(2)
    dev_kw = dict(kw, pixel_values=kw["pixel_values"].cuda().to(BF), motion_feature=kw["motion_feature"].cuda().to(BF))
    drop = units[:, 0]
    model.enable_graph_replay(True)
    try:
        outs = [model(**dev_kw, return_logprobs=True) for _ in range(3)]                       # eager, capture, replay
        graphs = lambda: sum(isinstance(v, tuple) for v in model._graphs.values())
        assert graphs() == 1 and len(model._graphs) == 1
        m1 = model(**dev_kw, return_logprobs=True, key_drop=drop)
        m2 = model(**dev_kw, return_logprobs=True, key_drop=drop)
        assert graphs() == 1 and len(model._graphs) == 1                                       # nothing captured, nothing even remembered
        again = model(**dev_kw, return_logprobs=True)                                          # replays; the masked pass before it disarmed
        assert graphs() == 1
        torch.cuda.synchronize()
        for o in outs + [again]:
            for key in ("score1", "logit", "logprob"):
                assert same(o[key], plain[key]), key
        for m in (m1, m2):
            for key in ("score1", "logit", "logprob"):
                assert same(m[key], masked[key]), key
    finally:
        model.enable_graph_replay(False)
    eager_after = model(**kw, return_logprobs=True)
    assert same(eager_after["score1"], plain["score1"]) and same(eager_after["logprob"], plain["logprob"])


def test_model_refusals_come_with_a_message_and_no_fault(lib):
    """10.  The host refusals (ValueError before any launch), the pass's own (too few words), aigv_llm_extend under an armed mask; a plain
    pass after each shows that the context disarmed."""
    model, cfg, sd, kw, units, plain, masked = rig(2)
    ok = units[:, 0]
    first = ok.clone(); first[0, 0] = True
    score_row = ok.clone(); score_row[1, int(kw["attention_mask"][1].sum()) - 4] = True
    for mask, extra, word in ((ok[:, :50], {}, "shape"), (first, {}, "first token"), (score_row, {}, "consumed row"),
                              (ok, dict(return_score_attention=True), "return_score_attention"), (ok, dict(return_token_attention=True), "return_score_attention")):
        with pytest.raises(ValueError, match=word):
            model(**kw, key_drop=mask, **extra)
    ctx = model._ctx
    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], kw["image_flags"], 3)
    words = model._key_drop_words(plan, ok).cuda()

    def plain_again():
        torch.cuda.synchronize()
        out = model(**kw, return_logprobs=True)
        assert same(out["score1"], plain["score1"]) and same(out["logprob"], plain["logprob"])

    # armed with fewer words per clip than the longest clip needs: the pass refuses before its first layer, and disarms
    vis, motion = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    native.check(lib.aigv_key_drop_arm(ctx, words.data_ptr(), words.shape[1] - 1), ctx)
    with pytest.raises(native.NativeError, match="words per clip"):
        model._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vis, plan["n_vis"], motion, plan["score_rows"], plan["logit_rows"])
    plain_again()
    for bad_args, word in (((None, 4), "null"), ((words.data_ptr(), 0), "ld_words")):
        assert lib.aigv_key_drop_arm(ctx, *bad_args) == AIGV_ERR_ARG and word in lib.aigv_last_error(ctx).decode()
    plain_again()
    # aigv_llm_extend under an armed mask (the shared-prefix path arms nothing itself: arm by hand behind its prefill)
    base = synth.canonical_tokens(cfg, 2, 2, seed=77)
    pp = synth.perspective_prompts(base, 2, seed=77)
    common = dict(pixel_values=synth.synthetic_frames(4, 224, seed=77), image_flags=torch.ones(4, 1, dtype=torch.long),
                  motion_feature=synth.synthetic_motion(2, cfg.motion_dim, seed=77))
    keep = model._prefill

    def prefill_then_arm(*a, **k):
        out = keep(*a, **k)
        native.check(lib.aigv_key_drop_arm(ctx, words.data_ptr(), words.shape[1]), ctx)
        return out

    model._prefill = prefill_then_arm
    try:
        with pytest.raises(native.NativeError, match="aigv_llm_extend: a key-drop mask is armed"):
            model.forward_shared_prefix([(p["input_ids"], p["attention_mask"], p["labels"]) for p in pp], **common)
    finally:
        del model._prefill
    plain_again()                                                                              # the refused continuation disarmed too
    ok_again = model(**kw, return_logprobs=True, key_drop=ok)
    assert same(ok_again["score1"], masked["score1"]) and same(ok_again["logprob"], masked["logprob"])


@pytest.mark.parametrize("stage", [2, 1])
def test_model_frame_ablation(stage):
    """11.  Each outs[i] is bit for bit the manual forward(key_drop=unit_masks[:, i]); absent frames are NaN; the ViT ran once."""
    model, cfg, sd, kw, units, plain, masked = rig(stage)
    calls = []
    keep = model.vit_tokens

    def counted(pv):
        calls.append(tuple(pv.shape))
        return keep(pv)

    model.vit_tokens = counted
    try:
        res = eval_utils.frame_ablation(model, **kw, return_logprobs=True)
    finally:
        del model.vit_tokens
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0][0] == 3
    U = units.shape[1]
    assert len(res["outs"]) == U + 1 and torch.equal(res["units"], units) and U == 3
    keys = (["score1"] if stage == 2 else []) + ["logit", "logprob"]
    for key in keys:
        assert same(res["outs"][0][key], plain[key]), key
        assert same(res["outs"][1][key], masked[key]), key
    for u in range(U):
        manual = model(**kw, return_logprobs=True, key_drop=units[:, u])
        for key in keys:
            assert same(res["outs"][1 + u][key], manual[key]), (u, key)
    if stage == 2:
        ab, delta = res["ablated"].cpu(), res["delta"].cpu()
        assert tuple(ab.shape) == (2, U) and same(res["score1"].cpu(), plain["score1"].float().cpu())
        absent = ~units.any(-1)
        assert absent.tolist() == [[False, False, False], [False, True, False]]
        assert torch.isnan(ab[absent]).all() and torch.isfinite(ab[~absent]).all() and torch.isnan(delta[absent]).all()
        want = torch.stack([res["outs"][1 + u]["score1"].float().cpu() for u in range(U)], 1)
        assert torch.equal(ab[~absent], want[~absent]) and torch.equal(delta[~absent], (plain["score1"].float().cpu()[:, None] - want)[~absent])
    else:
        assert "ablated" not in res and "score1" not in res
