"""Key-drop through the KV cache on the MI355X.

Op level: the masked form of the split-KV decode attention through aigv_op_attention_decode_drop - bit-exact on the key census and the one-hot
selector (tests/attention_exact_reference.py, tests/key_drop_reference.py) over the drop patterns, with g = 1, 4, 5, 8 query heads per KV head
and the cached lengths 1, 64, 127, 128, 129, 300, 1000 mixed in one launch; an all-zero mask against aigv_op_attention_decode; a sequence alone
against the batch, at two capacities; the refusals; a sequence without a visible key; random data against a float64 masked softmax under the
bar of tests/test_gpu_decode_ops.py.

Pass level, on the tiny rig (stage 2 and stage 1; the weight seeds are chosen in tests/test_key_drop_cache_cpu.py): generate_stage2(key_drop=...)
against a one-piece teacher-forced forward(key_drop=..., labels=...), the continuation pass on a masked cache, fork and reorder, the mask
dropped by the next plain generation, the host refusals, eval_utils.frame_ablation_generate."""
import functools
import math

import numpy as np
import pytest
import torch

import key_drop_reference as R
from attention_exact_reference import BF, ExactData, census_bits, census_weight, decode_case
from test_gpu_decode_ops import _caches, _decode_case, _held_to_the_eager_bar
from test_gpu_key_drop import bits, clip_alone, make_model, same, two_clips
from test_key_drop_cache_cpu import NEW_TOKENS, UNIT, WEIGHT_SEED

import aigv_assessor_amd as pkg
from aigv_assessor_amd import eval_utils, native, synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5          # a NaN bit pattern no kernel produces
CACHE_FILL = 0x7FB3        # NaN: cache rows nothing may read
PAD = 3                    # sentinel rows behind the output
D = 128
AIGV_ERR_ARG = -1
GROUPS = [1, 4, 5, 8]
N_KV = 2
LENS = [1, 64, 127, 128, 129, 300, 1000]
CAPS = (1100, 1283)        # two capacities, neither a multiple of the 128-key chunk
PATTERNS = ["none", "one", "k127_128", "chunk1", "word1", "all_but_0", "last", "beyond"]


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


def sync(rc):
    native.check(rc)
    torch.cuda.synchronize()


def pattern(shape, bits_):
    t = torch.full(shape, bits_, dtype=torch.int16, device="cuda").view(BF)
    _KEEP.append(t)
    return t


# =================================================================================================================================
# op level
# =================================================================================================================================
def drop_sets(lens, pat):
    """-> [bool array over the keys of every sequence]; every sequence keeps a visible key.  none; one key (the middle one); keys 127 and 128 (a
    chunk border); the whole aligned chunk 128..255 (length 129: its one valid key - an empty chunk either way); one whole 64-bit word inside a
    chunk, 64..127 (a half-empty chunk); everything but key 0; the last cached key; beyond: nothing below the length (the bits past it are set
    by words_of)."""
    out = []
    for n in lens:
        m = np.zeros(n, dtype=bool)
        if pat == "one":
            idx = [n // 2] if n > 1 else []
        elif pat == "k127_128":
            idx = [127, 128]
        elif pat == "chunk1":
            idx = range(128, 256)
        elif pat == "word1":
            idx = range(64, 128)
        elif pat == "all_but_0":
            idx = range(1, n)
        elif pat == "last":
            idx = [n - 1] if n > 1 else []
        else:
            assert pat in ("none", "beyond"), pat
            idx = []
        for j in idx:
            if 0 < j < n:
                m[j] = True
        out.append(m)
    return out


def words_of(drops, ld, beyond=False):
    """key_drop_reference.drop_words; ``beyond``: every bit at or past a sequence's length set as well - the kernel must ignore them."""
    if beyond:
        drops = [np.concatenate([m, np.ones(64 * ld - len(m), dtype=bool)]) for m in drops]
    return R.drop_words(drops, ld)


def census(case, drops):
    """key_drop_reference.census with the decode merge pass's normalisation (a division, where the prefill epilogue multiplies by the reciprocal)."""
    data = R.census(case, drops)
    exp = []
    for s, t in enumerate(case.tot):
        vis = R.visible_sets(case, s, drops[s])
        e = []
        for kh in range(case.hk):
            onehot = np.zeros((t, case.D), dtype=np.int64)
            onehot[np.arange(t), (np.arange(t) + int(case.phase[s, kh])) % case.D] = census_weight(kh)
            e.append(census_bits(vis.astype(np.int64) @ onehot, vis.sum(1), "decode"))
        exp.append(torch.from_numpy(np.repeat(np.stack(e, 1), case.g, axis=1)))
    return ExactData(case, data.q, data.k, data.v, torch.cat(exp))


def caches(case, data, poison=None):
    """[n_seq][n_kv][cap][D] caches of CACHE_FILL holding sequence b's keys / values in rows 0 .. len - 1.  ``poison`` [bool per key]: the K rows
    of those keys become NaN (a dropped key's K row is never read)."""
    kc, vc = pattern((len(case.tot), case.hk, case.cap, D), CACHE_FILL), pattern((len(case.tot), case.hk, case.cap, D), CACHE_FILL)
    for b, (k, v) in enumerate(zip(data.k, data.v)):
        k = k.clone()
        if poison is not None:
            k[torch.from_numpy(poison[b])] = float("nan")
        kc[b, :, : k.shape[0]] = k.transpose(0, 1).cuda()
        vc[b, :, : v.shape[0]] = v.transpose(0, 1).cuda()
    return kc, vc


def run(lib, case, q, kc, vc, words, plain=False, max_kv_len=None, seqs=None, word_offset=0, ld=None, check=True):
    """q [n_seq, h, D] in fused rows whose K / V slots are NaN, a NaN workspace.  -> the WHOLE output allocation [n_seq + PAD, h * D] (sentinel
    where nothing was written); with check = False -> (return code, output).  ``seqs``: run only these sequences of the case, as a batch of their own."""
    seqs = list(range(len(case.tot))) if seqs is None else seqs
    n_seq, n_kv, g, cap = len(seqs), case.hk, case.g, kc.shape[2]
    fused = torch.full((n_seq, n_kv, g + 2, D), float("nan"), dtype=BF, device="cuda")
    fused[:, :, :g] = q.view(-1, n_kv, g, D)[seqs].cuda()
    o = pattern((n_seq + PAD, n_kv * g * D), SENTINEL)
    nws = lib.aigv_op_attention_decode_ws_floats(n_seq, n_kv, g, cap)
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    lens = [case.tot[s] for s in seqs]
    dlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kcs, vcs = (kc, vc) if len(seqs) == len(case.tot) else (kc[seqs].contiguous(), vc[seqs].contiguous())
    _KEEP.extend([fused, ws, dlens, kcs, vcs])
    args = (fused.data_ptr(), n_kv * (g + 2) * D, (g + 2) * D, kcs.data_ptr(), vcs.data_ptr(), dlens.data_ptr(), cap, o.data_ptr(), n_kv * g * D, n_seq, n_kv, g, D,
            math.sqrt(D), max_kv_len or max(lens), ws.data_ptr(), nws)
    if plain:
        rc = lib.aigv_op_attention_decode(*args, None)
    elif words is None:
        rc = lib.aigv_op_attention_decode_drop(*args, None, 0, None)
    else:
        w = words[seqs].contiguous().cuda()
        _KEEP.append(w)
        rc = lib.aigv_op_attention_decode_drop(*args, w.data_ptr() + word_offset, words.shape[1] if ld is None else ld, None)
    if not check:
        torch.cuda.synchronize()
        return rc, o
    sync(rc)
    return o


def expect_whole(expect):
    e = expect.reshape(expect.shape[0], -1)
    return torch.cat([e, torch.full((PAD, e.shape[1]), SENTINEL, dtype=torch.int16)])


def assert_bits(got, want, what):
    got = got.cpu().view(torch.int16)
    if torch.equal(got, want):
        return
    bad = (got != want)
    rows = bad.any(-1).nonzero().flatten().tolist()
    c = bad[rows[0]].nonzero().flatten().tolist()[:4]
    raise AssertionError(f"{what}: {int(bad.sum())} elements of rows {rows} differ; first: row {rows[0]} columns {c}: got "
                         f"{[hex(int(got[rows[0], x]) & 0xffff) for x in c]} want {[hex(int(want[rows[0], x]) & 0xffff) for x in c]}")


@pytest.mark.parametrize("construction", ["census", "selector"])
@pytest.mark.parametrize("g", GROUPS)
def test_op_masked_census_and_selector_are_exact(lib, g, construction):
    """Every un-dropped key below the length counted once and no dropped one - whose K rows are 3.0e38 in the cache (census) or decoys that tie
    the chosen key (selector) -; chunks left empty or half empty; bits past the length ignored."""
    case = decode_case(g, N_KV, LENS, CAPS[0])
    ld = -(-max(LENS) // 64)
    for pat in PATTERNS:
        drops = drop_sets(LENS, pat)
        data = census(case, drops) if construction == "census" else R.selector(case, drops)
        kc, vc = caches(case, data)
        out = run(lib, case, torch.cat(data.q), kc, vc, words_of(drops, ld, beyond=pat == "beyond"))
        assert_bits(out, expect_whole(data.expect), f"{case.name} {construction} pattern {pat}")
        _KEEP.clear()


@pytest.mark.parametrize("g", GROUPS)
def test_op_all_zero_words_equal_the_unmasked_op(lib, g):
    """An all-zero mask, and a NULL one, through aigv_op_attention_decode_drop against aigv_op_attention_decode on random data: the same bits."""
    case = decode_case(g, N_KV, LENS, CAPS[0])
    data = R.random_case(case)
    kc, vc = caches(case, data)
    q = torch.cat(data.q)
    ld = -(-max(LENS) // 64)
    plain = run(lib, case, q, kc, vc, None, plain=True)
    assert not (plain[:len(LENS)].view(torch.int16) == SENTINEL).any() and (plain[len(LENS):].view(torch.int16) == SENTINEL).all()
    assert torch.equal(bits(run(lib, case, q, kc, vc, words_of(drop_sets(LENS, "none"), ld))), bits(plain))
    assert torch.equal(bits(run(lib, case, q, kc, vc, words_of(drop_sets(LENS, "none"), ld + 3))), bits(plain))
    assert torch.equal(bits(run(lib, case, q, kc, vc, None)), bits(plain))


def mixed_drops():
    """One pattern per sequence: an empty chunk (129, 300, 1000), a half-empty one (127, 128), single keys."""
    pats = ["none", "one", "word1", "word1", "chunk1", "chunk1", "chunk1"]
    drops = [drop_sets([n], p)[0] for n, p in zip(LENS, pats)]
    drops[6][64:128] = True                          # the longest sequence: a half-empty chunk in front of the empty one, and scattered keys
    drops[6][[300, 511, 512, 999]] = True
    return drops


def test_op_bits_do_not_depend_on_batch_mates_or_capacity(lib):
    """Under a mask: a sequence alone (n_seq = 1, max_kv_len = its own length) has the bits it has in the ragged batch, at two capacities."""
    g = 4
    case = decode_case(g, N_KV, LENS, CAPS[0])
    data = R.random_case(case)
    drops = mixed_drops()
    ld = -(-max(LENS) // 64)
    words = words_of(drops, ld)
    q = torch.cat(data.q)
    kc, vc = caches(case, data, poison=drops)
    batch = run(lib, case, q, kc, vc, words)
    assert torch.isfinite(batch[:len(LENS)].float()).all()
    big = decode_case(g, N_KV, LENS, CAPS[1])
    kc2, vc2 = caches(big, data, poison=drops)
    assert torch.equal(bits(run(lib, big, q, kc2, vc2, words)), bits(batch))
    for b in (0, 2, 4, 5, 6):
        for c, k, v in ((case, kc, vc), (big, kc2, vc2)):
            alone = run(lib, c, q, k, v, words, seqs=[b])
            assert torch.equal(bits(alone[0]), bits(batch[b])), (b, c.cap)
    # the same words row at a larger ld_drop
    assert torch.equal(bits(run(lib, case, q, kc, vc, words_of(drops, ld + 2))), bits(batch))


def test_op_refusals_come_with_a_message_and_no_fault(lib):
    """A misaligned key_drop and ld_drop < ceil(max_kv_len / 64): AIGV_ERR_ARG and a message that names the op, nothing launched; then a clean launch."""
    case = decode_case(4, N_KV, LENS, CAPS[0])
    drops = drop_sets(LENS, "k127_128")
    data = census(case, drops)
    kc, vc = caches(case, data)
    q = torch.cat(data.q)
    ld = -(-max(LENS) // 64)
    for kw, word in ((dict(word_offset=4), "8-byte aligned"), (dict(ld=ld - 1), "ld_drop"), (dict(ld=0), "ld_drop")):
        rc, out = run(lib, case, q, kc, vc, words_of(drops, ld + 1), check=False, **kw)
        msg = (lib.aigv_last_error(None) or b"").decode()
        assert rc == AIGV_ERR_ARG and word in msg and "aigv_op_attention_decode_drop" in msg, (rc, msg)
        assert (out.view(torch.int16) == SENTINEL).all()                                       # nothing was launched
    assert_bits(run(lib, case, q, kc, vc, words_of(drops, ld)), expect_whole(data.expect), "after the refusals")
    # ld_drop is held against max_kv_len, not the capacity: exactly ceil(max_kv_len / 64) words per sequence serve
    assert ld == 16 and -(-CAPS[0] // 64) > ld


def test_op_a_sequence_without_a_visible_key_is_zeros_and_its_neighbours_keep_their_bits(lib):
    """Sequences 1 (64 keys) and 5 (300 keys) with every key dropped and NaN in every K row: all-zero outputs; the others are bit for bit what
    they are when those two are not masked."""
    g = 5
    case = decode_case(g, N_KV, LENS, CAPS[0])
    data = R.random_case(case)
    q = torch.cat(data.q)
    ld = -(-max(LENS) // 64)
    base_drops = mixed_drops()
    base_drops[1][:] = False
    base_drops[5][:] = False
    kc, vc = caches(case, data, poison=base_drops)
    base = run(lib, case, q, kc, vc, words_of(base_drops, ld))
    drops = [m.copy() for m in base_drops]
    drops[1][:] = True
    drops[5][:] = True
    kc2, vc2 = caches(case, data, poison=drops)
    out = run(lib, case, q, kc2, vc2, words_of(drops, ld))
    want = bits(base).clone()
    want[[1, 5]] = 0
    assert torch.equal(bits(out), want)
    assert not (bits(base)[[1, 5]] == 0).all()


@pytest.mark.parametrize("g,n_kv", [(1, 2), (4, 2), (5, 2), (8, 2)])
def test_op_random_data_against_float64_under_the_decode_bar(lib, g, n_kv):
    """The masked op against a float64 softmax over the visible keys, under the checker and the bar of
    tests/test_gpu_decode_ops.py::test_decode_attention_matches_fp64_at_ragged_lengths (a softmax over the visible keys IS the masked softmax);
    empty and half-empty chunks among the patterns, NaN in the K rows of the dropped keys, a late dominant key."""
    q, ks, vs = _decode_case(n_kv, g, LENS, seed=500 * g + n_kv, late_key=(6, 900))
    drops = mixed_drops()
    assert not drops[6][900]
    ld = -(-max(LENS) // 64)
    kp = [k.clone() for k in ks]
    for k, m in zip(kp, drops):
        k[:, torch.from_numpy(m).cuda()] = float("nan")
    kc, vc = _caches(kp, vs, CAPS[0])
    n_seq = len(LENS)
    fused = torch.full((n_seq, n_kv, g + 2, D), float("nan"), dtype=BF, device="cuda")
    fused[:, :, :g] = q
    o = torch.full((n_seq, n_kv * g * D), float("nan"), dtype=BF, device="cuda")
    nws = lib.aigv_op_attention_decode_ws_floats(n_seq, n_kv, g, CAPS[0])
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    dlens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    words = words_of(drops, ld).cuda()
    sync(lib.aigv_op_attention_decode_drop(fused.data_ptr(), n_kv * (g + 2) * D, (g + 2) * D, kc.data_ptr(), vc.data_ptr(), dlens.data_ptr(), CAPS[0], o.data_ptr(),
                                           n_kv * g * D, n_seq, n_kv, g, D, math.sqrt(D), max(LENS), ws.data_ptr(), nws, words.data_ptr(), ld, None))
    vis = [torch.from_numpy(~m).cuda() for m in drops]
    _held_to_the_eager_bar(o.view(n_seq, n_kv, g, D), q, [k[:, v] for k, v in zip(ks, vis)], [x[:, v] for x, v in zip(vs, vis)])


# =================================================================================================================================
# pass level
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def rig(stage):
    """The tiny rig of tests/test_gpu_key_drop.py - two clips of 2 and 1 frames, N = 215, tokens seed 300 + stage - under the weights chosen in
    tests/test_key_drop_cache_cpu.py.  -> model, cfg, kw (labels taken out: generation has none), the unit masks."""
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    sd = synth.make_state_dict(cfg, seed=WEIGHT_SEED[stage], rich=True)
    model = make_model(cfg, sd, stage)
    kw, ctx_id = two_clips(cfg, 300 + stage)
    model.img_context_token_id = ctx_id
    units = model.unit_masks(kw["input_ids"], kw["attention_mask"], kw["image_flags"])
    kw = dict(kw)
    kw.pop("labels")
    return model, cfg, kw, units


def gen(model, kw, **extra):
    out = model.generate_stage2(kw["pixel_values"], kw["input_ids"], kw["attention_mask"], kw["image_flags"], kw["motion_feature"], max_new_tokens=NEW_TOKENS, **extra)
    torch.cuda.synchronize()
    return out


def teacher_forced(model, kw, seq, key_drop=None):
    """One-piece forward on prompt + the generated tokens ``seq`` [B, T], every generated token a label.  -> per clip and step: the answer-row
    argmax [B, T], its log-probability under the labels [B, T], the pass's own top-2 log-probabilities [B, T, 2]."""
    ids, am = kw["input_ids"], kw["attention_mask"]
    B, N = ids.shape
    T = seq.shape[1]
    ids2 = torch.cat([ids, torch.zeros(B, T, dtype=torch.long)], 1)
    am2 = torch.cat([am, torch.zeros(B, T, dtype=torch.bool)], 1)
    labels = torch.full((B, N + T), -100)
    lens = am.sum(1).tolist()
    for b, n in enumerate(lens):
        ids2[b, n:n + T] = seq[b].cpu()
        labels[b, n:n + T] = seq[b].cpu()
        am2[b, n:n + T] = True
    extra = {} if key_drop is None else dict(key_drop=torch.cat([key_drop, torch.zeros(B, T, dtype=torch.bool)], 1))
    out = model(pixel_values=kw["pixel_values"], input_ids=ids2, attention_mask=am2, image_flags=kw["image_flags"], labels=labels,
                motion_feature=kw["motion_feature"], return_logprobs=True, top_logprobs=2, **extra)
    torch.cuda.synchronize()
    rows = torch.tensor([[b * (N + T - 1) + n - 1 + i for i in range(T)] for b, n in enumerate(lens)])
    return out["logit"].cpu()[rows], out["logprob"].cpu()[rows], out["top_logprob"].cpu()[rows]


@pytest.mark.parametrize("stage", [2, 1])
def test_model_generation_against_the_one_piece_masked_pass(stage):
    """generate_stage2(key_drop = frame 0 of every clip) against forward(key_drop=..., labels=...) teacher-forced on prompt + the generated tokens
    (that pass is pinned against the oracle by tests/test_gpu_key_drop.py): every generated token is the one-piece pass's answer-row argmax,
    except on rows where that pass's own top two log-probabilities are closer than 2 x the largest |log-probability difference| between
    generate and the one-piece pass WITHOUT a mask (measured here, printed).  At most 1 row in 6 is excused; the unmasked pair excuses none."""
    model, cfg, kw, units = rig(stage)
    plain = gen(model, kw, return_logprobs=True, top_logprobs=2)
    p_arg, p_lp, p_top = teacher_forced(model, kw, plain.sequences)
    assert tuple(plain.sequences.shape) == (2, NEW_TOKENS)
    gap = float((plain.logprobs.cpu() - p_lp).abs().max())
    print(f"stage {stage}: unmasked generate vs one-piece: max |d logprob| = {gap:.3e}; tokens {plain.sequences.tolist()} one-piece argmax {p_arg.tolist()}; "
          f"one-piece top-2 gaps {(p_top[..., 0] - p_top[..., 1]).tolist()}")
    assert torch.equal(plain.sequences.cpu(), p_arg), "the unmasked pair differs: nothing may be excused there"
    drop = units[:, UNIT]
    masked = gen(model, kw, return_logprobs=True, top_logprobs=2, key_drop=drop)
    m_arg, m_lp, m_top = teacher_forced(model, kw, masked.sequences, key_drop=drop)
    top2 = m_top[..., 0] - m_top[..., 1]
    differ = masked.sequences.cpu() != m_arg
    print(f"stage {stage}: masked generate {masked.sequences.tolist()} one-piece argmax {m_arg.tolist()}; max |d logprob| = "
          f"{float((masked.logprobs.cpu() - m_lp).abs().max()):.3e}; one-piece top-2 gaps {top2.tolist()}; rows that differ {differ.nonzero().tolist()}")
    assert bool((top2[differ] < 2 * gap).all()), "a generated token differs from the one-piece masked pass beyond a near tie"
    assert int(differ.sum()) <= differ.numel() // 6
    assert not torch.equal(masked.sequences, plain.sequences)                                  # the mask reached the reply
    assert same(masked.top_logprobs[..., 0], masked.logprobs)


def staged(model, kw, n_frames=3):
    plan = model._plan(kw["input_ids"], kw["attention_mask"], None, kw["image_flags"], n_frames, drop_dead_tail=False)
    vis, mot = model._visual_inputs(kw["pixel_values"].cuda().to(BF), None, kw["motion_feature"].cuda().to(BF), plan)
    return plan, vis, mot


def decode_step(lib, model, tok):
    """One aigv_decode_step_logprob -> (next tokens, their log-probabilities, the final hidden rows)."""
    ctx, n = model._ctx, tok.numel()
    tok = tok.contiguous()
    new, lp = torch.empty_like(tok), torch.empty(n, dtype=torch.float32, device="cuda")
    native.check(lib.aigv_decode_step_logprob(ctx, tok.data_ptr(), new.data_ptr(), lp.data_ptr(), None), ctx)
    hid = model.last_hidden_rows(n)
    torch.cuda.synchronize()
    return new, lp, hid


@pytest.mark.parametrize("stage", [2, 1])
def test_model_continuation_on_a_masked_cache(lib, stage):
    """A masked keep_kv prefill of prompt[:-k] + aigv_llm_extend(prompt[-k:]) + a decode step against the one-piece masked prefill of the prompt +
    that step - the comparison of the unmasked continuation tests (tests/test_gpu_e2e.py: identical next tokens, one rounding tie may flip).
    With an all-zero mask the masked route (key-drop forms of the prefill, the continuation and the decode attention) gives the unmasked bits."""
    model, cfg, kw, units = rig(stage)
    plan, vis, mot = staged(model, kw)
    B, cu, k, lens = 2, plan["cu"], 7, plan["lens"]
    cap = max(lens) + 8
    last_rows = [cu[b + 1] - 1 for b in range(B)]
    ids_p = torch.cat([plan["ids_packed"][cu[b]:cu[b + 1] - k] for b in range(B)])
    slot_p = torch.cat([plan["slot"][cu[b]:cu[b + 1] - k] for b in range(B)])
    cu_p = [0, lens[0] - k, lens[0] + lens[1] - 2 * k]
    tail = torch.cat([plan["ids_packed"][cu[b + 1] - k:cu[b + 1]] for b in range(B)]).to(torch.long).cuda()

    def one_piece(words):
        _, nxt = model._prefill(plan["ids_packed"], plan["slot"], cu, vis, plan["n_vis"], mot, None, last_rows, keep_kv=True, kv_cap=cap, drop_words=words)
        return nxt.clone(), decode_step(lib, model, nxt)

    def two_pieces(words_p):
        model._prefill(ids_p, slot_p, cu_p, vis, plan["n_vis"], mot, None, [], keep_kv=True, kv_cap=cap, drop_words=words_p)
        ctx = model._ctx
        nxt = torch.empty(B, dtype=torch.long, device="cuda")
        native.check(lib.aigv_llm_extend(ctx, tail.data_ptr(), native.i32_array([0, k, 2 * k]), B, None, None, native.i32_array([k - 1, 2 * k - 1]), B,
                                         nxt.data_ptr(), 1, None), ctx)
        hid = model.last_hidden_rows(B)
        return nxt.clone(), hid, decode_step(lib, model, nxt)

    drop = units[:, UNIT]
    words = model._gen_drop_words(drop, kw["input_ids"].shape, cu, plan["row_of"])
    words_p = R.drop_words([drop[b, :lens[b] - k].numpy() for b in range(B)], words.shape[1])
    assert torch.equal(words_p, words)                                                         # frame 0 lies inside the prefix
    full_nxt, (full_new, _, full_hid) = one_piece(words)
    ext_nxt, _, (ext_new, _, ext_hid) = two_pieces(words_p)
    flips = int((full_nxt != ext_nxt).sum()) + int((full_new != ext_new).sum())
    print(f"stage {stage}: masked one-piece {full_nxt.tolist()} {full_new.tolist()} continuation {ext_nxt.tolist()} {ext_new.tolist()}; "
          f"max |d hidden| after the step {float((full_hid.float() - ext_hid.float()).abs().max()):.3e}")
    assert flips <= 1, flips
    # not the unmasked result, and the no-op mask: the unmasked continuation's bits
    zero = torch.zeros_like(words_p)
    u_nxt, u_hid, (u_new, u_lp, u_hid2) = two_pieces(None)
    z_nxt, z_hid, (z_new, z_lp, z_hid2) = two_pieces(zero)
    assert same(z_nxt, u_nxt) and same(z_hid, u_hid) and same(z_new, u_new) and same(z_lp, u_lp) and same(z_hid2, u_hid2)
    assert not same(ext_hid, u_hid2)
    # the continuation takes no mask of its own, and the probe does not know the cache's
    model._prefill(ids_p, slot_p, cu_p, vis, plan["n_vis"], mot, None, [], keep_kv=True, kv_cap=cap, drop_words=words_p)
    ctx = model._ctx
    wd = words_p.cuda()
    native.check(lib.aigv_key_drop_arm(ctx, wd.data_ptr(), wd.shape[1]), ctx)
    nxt = torch.empty(B, dtype=torch.long, device="cuda")
    ext = lambda: lib.aigv_llm_extend(ctx, tail.data_ptr(), native.i32_array([0, k, 2 * k]), B, None, None, native.i32_array([k - 1, 2 * k - 1]), B, nxt.data_ptr(), 0, None)
    assert ext() == AIGV_ERR_ARG and "aigv_llm_extend: a key-drop mask is armed" in lib.aigv_last_error(ctx).decode()
    seg = torch.zeros(2 * k, dtype=torch.int32, device="cuda")
    seg_c = torch.zeros(B, cap, dtype=torch.int32, device="cuda")
    att = torch.empty(B, cfg.llm_config.num_hidden_layers, cfg.llm_config.num_attention_heads, 1, dtype=torch.float32, device="cuda")
    native.check(lib.aigv_score_attention_arm(ctx, native.i32_array([k - 1, 2 * k - 1]), B, seg.data_ptr(), seg_c.data_ptr(), cap, 1, att.data_ptr()), ctx)
    assert ext() == AIGV_ERR_ARG and "the probe does not know the mask" in lib.aigv_last_error(ctx).decode()
    native.check(ext(), ctx)                                                                   # both refusals disarmed: the masked continuation runs
    torch.cuda.synchronize()
    assert same(nxt, ext_nxt)


@pytest.mark.parametrize("stage", [2, 1])
def test_model_fork_and_reorder_carry_the_mask(lib, stage):
    """aigv_kv_fork x 2 behind a masked prefill, then one decode step: the copies give the originals' bits.  aigv_kv_reorder swapping two
    sequences of one length under different masks (the same clip twice, frame 0 hidden from one and frame 1 from the other) swaps their outputs."""
    model, cfg, kw, units = rig(stage)
    plan, vis, mot = staged(model, kw)
    cu, lens = plan["cu"], plan["lens"]
    words = model._gen_drop_words(units[:, UNIT], kw["input_ids"].shape, cu, plan["row_of"])
    model._native(seq_len=max(lens), n_clips=4, out_rows=4)

    def prefill(w):
        _, nxt = model._prefill(plan["ids_packed"], plan["slot"], cu, vis, plan["n_vis"], mot, None, [cu[1] - 1, cu[2] - 1], keep_kv=True, kv_cap=max(lens) + 8,
                                drop_words=w)
        return nxt.clone()

    nxt = prefill(words)
    new, lp, hid = decode_step(lib, model, nxt)
    nxt2 = prefill(words)
    assert same(nxt, nxt2)
    native.check(lib.aigv_kv_fork(model._ctx, 2, None), model._ctx)
    new4, lp4, hid4 = decode_step(lib, model, torch.cat([nxt, nxt]))
    for part in (slice(0, 2), slice(2, 4)):
        assert same(new4[part], new) and same(lp4[part], lp) and same(hid4[part], hid), part
    u_new, u_lp, u_hid = decode_step(lib, model, prefill(None))
    assert not same(u_hid, hid)                                                                # (a copy without its mask row would be this)

    # the same clip twice, under two masks
    one, n = clip_alone(dict(kw, labels=kw["input_ids"]), 0)
    twice = {key: torch.cat([one[key], one[key]]) for key in ("pixel_values", "input_ids", "attention_mask", "image_flags", "motion_feature")}
    plan2, vis2, mot2 = staged(model, twice, n_frames=4)
    cu2 = plan2["cu"]
    drop2 = torch.stack([units[0, 0, :n], units[0, 1, :n]])
    words2 = model._gen_drop_words(drop2, twice["input_ids"].shape, cu2, plan2["row_of"])

    def prefill2():
        _, t = model._prefill(plan2["ids_packed"], plan2["slot"], cu2, vis2, plan2["n_vis"], mot2, None, [cu2[1] - 1, cu2[2] - 1], keep_kv=True, kv_cap=n + 8,
                              drop_words=words2)
        return t.clone()

    t = prefill2()
    a_new, a_lp, a_hid = decode_step(lib, model, t)
    assert not same(a_hid[0], a_hid[1])
    t = prefill2()
    native.check(lib.aigv_kv_reorder(model._ctx, native.i32_array([1, 0]), native.i32_array([n, n]), 2, None), model._ctx)
    b_new, b_lp, b_hid = decode_step(lib, model, t.flip(0))
    assert same(b_new, a_new.flip(0)) and same(b_lp, a_lp.flip(0)) and same(b_hid, a_hid.flip(0))


@pytest.mark.parametrize("stage", [2, 1])
def test_model_a_plain_generation_after_a_masked_one_is_plain(stage):
    """The next unmasked keep_kv prefill clears the cache's mask: plain, masked, plain - the two plain replies are bit-identical.  Beam search and
    sampling under a mask run, and the mask reaches them."""
    model, cfg, kw, units = rig(stage)
    before = gen(model, kw, return_logprobs=True, candidate_ids=[5, 6, 7])
    masked = gen(model, kw, return_logprobs=True, candidate_ids=[5, 6, 7], key_drop=units[:, UNIT].cuda().long())
    after = gen(model, kw, return_logprobs=True, candidate_ids=[5, 6, 7])
    for key in ("sequences", "logprobs", "cand_logprobs"):
        assert same(before[key], after[key]), key
    assert not same(before["logprobs"], masked["logprobs"])
    beams_plain = gen(model, kw, num_beams=2, return_dict_in_generate=True)
    beams_masked = gen(model, kw, num_beams=2, return_dict_in_generate=True, key_drop=units[:, UNIT])
    assert not same(beams_plain.sequences_scores, beams_masked.sequences_scores)
    g0 = torch.Generator(device="cuda").manual_seed(5)
    sampled = gen(model, kw, do_sample=True, top_k=8, generator=g0, return_logprobs=True, key_drop=units[:, UNIT])
    assert tuple(sampled.sequences.shape) == (2, NEW_TOKENS) and torch.isfinite(sampled.logprobs).all()
    assert same(gen(model, kw, return_logprobs=True)["logprobs"], before["logprobs"])


def test_model_host_refusals_leave_the_context_alone():
    """ValueError before any launch (tests/test_key_drop_cache_cpu.py runs the same calls on a host model); a plain reply afterwards is unchanged."""
    model, cfg, kw, units = rig(2)
    before = gen(model, kw, return_logprobs=True)
    ok = units[:, UNIT]
    first = ok.clone(); first[0, 0] = True
    last = ok.clone(); last[1, int(kw["attention_mask"][1].sum()) - 1] = True
    for mask, word in ((ok[:, :50], "shape"), (ok.float(), "bool or integer"), (first, "first token"), (last, "last prompt token")):
        with pytest.raises(ValueError, match=word):
            gen(model, kw, key_drop=mask)
    with pytest.raises(ValueError, match="return_score_attention"):
        model(**kw, key_drop=ok, return_score_attention=True)
    assert same(gen(model, kw, return_logprobs=True)["logprobs"], before["logprobs"])


@pytest.mark.parametrize("stage", [2, 1])
def test_model_frame_ablation_generate(stage):
    """Row 0 is the plain generate_stage2, row u + 1 generate_stage2(key_drop=units[:, u]); units a clip does not have are pad / NaN; InternViT ran once."""
    model, cfg, kw, units = rig(stage)
    cand = [11, 12, 13]
    calls = []
    keep = model.vit_tokens

    def counted(pv):
        calls.append(tuple(pv.shape))
        return keep(pv)

    model.vit_tokens = counted
    try:
        res = eval_utils.frame_ablation_generate(model, **kw, max_new_tokens=NEW_TOKENS, candidate_ids=cand)
    finally:
        del model.vit_tokens
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0][0] == 3
    U = units.shape[1]
    pad = cfg.llm_config.pad_token_id
    seqs, clp = res["sequences"], res["cand_logprobs"]
    assert tuple(seqs.shape) == (2, U + 1, NEW_TOKENS) and tuple(clp.shape) == (2, U + 1, NEW_TOKENS, 3) and torch.equal(res["units"], units) and U == 3
    plain = gen(model, kw, candidate_ids=cand)
    assert same(seqs[:, 0], plain.sequences) and same(clp[:, 0], plain.cand_logprobs)
    absent = ~units.any(-1)
    assert absent.tolist() == [[False, False, False], [False, True, False]]
    for u in range(U):
        manual = gen(model, kw, candidate_ids=cand, key_drop=units[:, u])
        for b in range(2):
            if absent[b, u]:
                assert bool((seqs[b, u + 1] == pad).all()) and bool(torch.isnan(clp[b, u + 1]).all())
            else:
                assert same(seqs[b, u + 1], manual.sequences[b]) and same(clp[b, u + 1], manual.cand_logprobs[b]), (b, u)
    assert not same(seqs[:, 1], seqs[:, 0])
    no_cand = eval_utils.frame_ablation_generate(model, **kw, max_new_tokens=NEW_TOKENS)
    assert set(no_cand) == {"sequences", "units"} and same(no_cand["sequences"], seqs)
