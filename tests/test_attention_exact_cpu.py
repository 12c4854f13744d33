"""The conditions the exact attention tests (tests/test_gpu_attention_exact.py) rest on, without a GPU, for every case that file runs:
the census phases are distinct, the selector's lead is hundreds of octaves under both score numerics with bf16-exact raw scores and the
suite's own references return V[pi] bit for bit, the census expectation is fp64 count / n to within one bf16 ulp, and - a condition, not a
measurement - the census expectation of EVERY row changes when one visible key is removed, when the first invisible key is added, and
when the neighbouring kv head's V is read (the phase rotates the columns, which a row with a multiple of D visible keys cannot show: the
one-hot's value, 1 + kv head, shows it there).  The selector's expectation changes under that swap on every row too."""
import functools
import math

import numpy as np
import pytest
import torch

from attention_exact_reference import (BF, DECODE_LENS, DECODE_PAIRS, DECODE_ROUNDS, EX_NAMES, PACKED, ROPE, all_cases, bf16_bits, census_bits,
                                       census_counts, census_weight, ex_case)
from attention_reference import COUNTS, OFFSETS, attn_truth

CASES = all_cases()
IDS = [c[0] for c in CASES]
FORMS = ("prefill", "decode")           # the sensitivity condition runs in both normalisation forms for every case


def test_the_case_lists_are_the_ones_the_exact_tests_must_run():
    assert [(c[1], c[2], c[3], c[4], c[5]) for c in PACKED[:4]] == [(64, False, 2, 2, [1025, 1025]), (64, False, 2, 2, [257, 65, 1]),
                                                                     (64, False, 2, 2, [512, 300, 33]), (64, False, 2, 2, [63, 64, 65, 127, 128, 129])]
    assert PACKED[0][6] and PACKED[0][7] == (False, True) and PACKED[1][7] == (False, True)
    causal = [(c[3], c[4], c[5]) for c in PACKED if c[1] == 128 and c[2]]
    assert causal == [(4, 2, [200, 77]), (8, 2, [513, 64, 1]), (3, 1, [300, 129]), (10, 2, [257, 64]), (6, 1, [513, 64, 1]), (7, 1, [200, 77]),
                      (8, 1, [385]), (2, 2, [63, 64, 65, 127, 128, 129]), (4, 2, [2176]), (48, 8, [300, 77, 129])]
    assert {h // hk for h, hk, _ in causal} >= set(range(1, 9))
    assert [(c[3], c[4], c[5]) for c in PACKED if c[1] == 128 and not c[2]] == [(2, 2, [384, 129])]
    assert ROPE[1:] == (128, True, 8, 2, [300, 77, 129])
    pairs = {(o, n) for name in EX_NAMES for o, n in zip(ex_case(name).offs, ex_case(name).cnts)}
    assert all((o, n) in pairs for o in OFFSETS for n in COUNTS)
    assert {"ragged-2176-63-0", "ragged-g3", "scoring-g6x8"} <= set(EX_NAMES)
    assert DECODE_LENS == [1, 127, 128, 129, 2177, 8191, 8192, 8193, 16384] and len(DECODE_PAIRS) == 9 and {g for g, _ in DECODE_PAIRS} == set(range(1, 9))
    assert len(set(IDS)) == len(IDS)


def test_the_generators_use_nothing_of_the_package_under_test():
    """Every module the generators hold, and the module every function and class they hold was defined in, this file's imports of
    attention_reference included: math, numpy, torch and the two reference modules themselves."""
    import types
    import attention_exact_reference as R
    import attention_reference as A
    allowed = {"math", "numpy", "torch", "builtins", R.__name__, A.__name__}
    for mod in (R, A):
        for name, val in vars(mod).items():
            if name.startswith("__"):
                continue
            origin = val.__name__ if isinstance(val, types.ModuleType) else getattr(val, "__module__", None) or "builtins"
            assert origin.split(".")[0] in allowed, (mod.__name__, name, origin)


def test_bf16_rounding_is_round_to_nearest_even():
    x = torch.randn(100000, generator=torch.Generator().manual_seed(0)) * torch.logspace(-6, 3, 100000)
    x = torch.cat([x, torch.tensor([1.00390625, 1.01171875, 0.0, 1.0 / 3.0])])          # two ties (down to even, up to even)
    assert torch.equal(torch.from_numpy(bf16_bits(x.numpy())), x.to(BF).view(torch.int16))


@pytest.mark.parametrize("name", IDS)
def test_census_phases_are_pairwise_distinct(name):
    case = CASES[IDS.index(name)][1]()
    ph = case.phase.reshape(-1)
    assert len(set(ph.tolist())) == len(ph) == len(case.cnts) * case.hk and ph.min() >= 0 and ph.max() < case.D


@functools.lru_cache(maxsize=None)
def _key_sensitive(D, l, form, w):
    """Phase 0 (any other phase rotates the columns of everything below alike), one-hot value w.  -> (removing any one visible key changes
    the row, adding key l changes the row)."""
    cnt = census_counts([l], 0, D)                                # [1, D]
    base = census_bits(w * cnt, [l], form)
    less = census_bits(w * (cnt - np.eye(D, dtype=np.int64)), [l - 1] * D, form)     # row c: one key of column c removed
    held = cnt[0] > 0
    removed = ((less != base).any(1) | ~held).all()
    more = cnt.copy()
    more[0, l % D] += 1
    return bool(removed), bool((census_bits(w * more, [l + 1], form) != base).any())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", IDS)
def test_census_changes_with_every_single_key_on_every_row(name, form):
    """No row is exempt: removing any one visible key, adding the key behind the last visible one (the key after the diagonal, key kv_len),
    adding the first key of the next packed sequence, and reading the neighbouring kv head's V each change at least one expected bf16
    pattern of the row."""
    case = CASES[IDS.index(name)][1]()
    D = case.D
    packed = not any(case.offs) and not case.cap
    for s in range(len(case.cnts)):
        vis = case.visible(s)
        for w in sorted({census_weight(kh) for kh in range(case.hk)}):
            for l in sorted(set(vis.tolist())):
                assert _key_sensitive(D, l, form, w) == (True, True), (name, s, l, w)
        for kh in range(case.hk):
            w = census_weight(kh)
            cnt = w * census_counts(vis, case.phase[s, kh], D)
            base = census_bits(cnt, vis, form)
            if packed and s + 1 < len(case.cnts):                  # the row behind a packed sequence's last key: the next sequence's key 0
                more = cnt.copy()
                more[:, case.phase[s + 1, kh] % D] += w
                assert (census_bits(more, vis + 1, form) != base).any(1).all(), (name, s, kh)
            for other in range(case.hk):             # any other kv head, the neighbours among them
                if other != kh:
                    swapped = census_bits(census_weight(other) * census_counts(vis, case.phase[s, other], D), vis, form)
                    assert (swapped != base).any(1).all(), (name, s, kh, other)


@pytest.mark.parametrize("name", IDS)
def test_census_expectation_is_the_fp64_quotient_to_one_ulp(name):
    case = CASES[IDS.index(name)][1]()
    data = case.census()
    assert all((q == 0).all() for q in data.q) and all(torch.isfinite(k.float()).all() for k in data.k)
    row = 0
    for s, n in enumerate(case.cnts):
        vis = case.visible(s)
        for kh in range(case.hk):
            # the count, from the V tensor itself
            cnt = np.stack([data.v[s][:l, kh].double().sum(0).numpy() for l in vis])
            assert np.array_equal(cnt, census_weight(kh) * census_counts(vis, case.phase[s, kh], case.D))
            want = cnt / vis[:, None]
            got = data.expect[row: row + n, kh * case.g].view(BF).double().numpy()
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(want, 1e-30))) - 7)
            assert (np.abs(got - want) <= ulp).all() and ((want > 0) == (got > 0)).all(), (name, s, kh)
            for a in range(1, case.g):
                assert torch.equal(data.expect[row: row + n, kh * case.g + a], data.expect[row: row + n, kh * case.g])
            for other in (kh - 1, kh + 1):       # the neighbouring kv head's expectation differs on every row
                if 0 <= other < case.hk:
                    assert (data.expect[row: row + n, kh * case.g] != data.expect[row: row + n, other * case.g]).any(-1).all(), (name, s, kh, other)
        row += n


def _rb(x):
    return x.to(BF).double()


def _selector_checks(case, data, eager=True):
    """-> the smallest lead of the selected score, in octaves of the softmax's exp2, over both score numerics."""
    D, g = case.D, case.g
    pow2 = math.frexp(case.post)[0] == 0.5
    worst = float("inf")
    row = 0
    for s, (o, n) in enumerate(zip(case.offs, case.cnts)):
        q, k, v, pi = data.q[s], data.k[s], data.v[s], torch.from_numpy(data.pi[s])
        vis = torch.from_numpy(case.visible(s))
        assert (pi >= 0).all() and (pi < vis[:, None]).all()
        for a in range(case.h):                    # different heads of one group choose different keys, where that many are visible
            for b in range(a - a % g, a):
                assert ((pi[:, a] != pi[:, b]) | (vis <= a % g)).all(), (case.name, s, a, b)
        hidden = torch.arange(k.shape[0])[None, None, :] >= vis[None, :, None]
        for kh in range(case.hk):
            kk = k[:, kh].double().t()                                                  # [D, t]
            qh, ph = q[:, kh * g: (kh + 1) * g].transpose(0, 1), pi[:, kh * g: (kh + 1) * g].t()[:, :, None]     # [g, n, D], [g, n, 1]
            raw = qh.double() @ kk                                                      # [g, n, t]
            assert torch.equal(_rb(raw), raw), "a raw score is not a bf16 number"
            sc = raw if case.pre == 1.0 else _rb(qh.float() * case.pre) @ kk            # the kernel's q pre-scale rounds to bf16
            for rs in (False, True):
                e = sc
                if rs:
                    e = _rb(e)
                    e = e / case.post if pow2 else _rb(e / case.post)
                else:
                    e = e / case.post
                sel = e.gather(2, ph)[:, :, 0]
                rest = e.masked_fill(hidden, -float("inf")).scatter(2, ph, -float("inf")).amax(2)
                worst = min(worst, ((sel - rest) * math.log2(math.e)).min().item())
        # reading the neighbouring kv head's V changes the expectation of every row
        vb = v.contiguous().view(torch.int16)
        for a in range(case.h):
            for other in (a // g - 1, a // g + 1):
                if 0 <= other < case.hk:
                    assert (vb[pi[:, a], other] != data.expect[row: row + n, a]).any(-1).all(), (case.name, s, a, other)
        # the suite's eager bf16 path returns the selected V row, bit for bit
        if eager:
            got = attn_truth(q, k, v, case.causal, case.pre, case.post, BF, kv_off=o)
            assert torch.equal(got.contiguous().view(torch.int16), data.expect[row: row + n]), (case.name, s)
        row += n
    return worst


@pytest.mark.parametrize("name", [n for n in IDS if not n.startswith("decode")])
def test_selector_margin_and_the_eager_reference(name):
    case = CASES[IDS.index(name)][1]()
    data = case.selector()
    lead = _selector_checks(case, data)
    print(f"{name}: the selected score leads by {lead:.0f} octaves at least")
    assert lead >= 200.0
    aims = set()
    for s, pi in enumerate(data.pi):
        vis = case.visible(s)[:, None]
        aims |= {"zero"} if (pi == 0).any() else set()
        aims |= {"last"} if (pi == vis - 1).any() else set()
        if vis.max() > 128:
            aims |= {a for a, m in (("tile0", pi % 64 == 0), ("tile63", pi % 64 == 63), ("chunk0", (pi % 128 == 0) & (pi > 0)), ("chunk127", pi % 128 == 127)) if m.any()}
    assert {"zero", "last"} <= aims and (max(case.tot) <= 128 or len(aims) == 6), aims


@pytest.mark.parametrize("name", [n for n in IDS if n.startswith("decode")])
def test_decode_selector_margin_and_the_decode_tests_reference(name):
    import test_gpu_decode_ops as G              # (imports without a GPU: nothing touches the device at import time)
    case = CASES[IDS.index(name)][1]()
    seen = [set() for _ in case.cnts]
    data = None
    for rnd in range(DECODE_ROUNDS):              # every round the GPU file launches
        data = case.selector(rnd, base=data)
        lead = _selector_checks(case, data, eager=rnd == 0)
        print(f"{name} round {rnd}: the selected score leads by {lead:.0f} octaves at least")
        assert lead >= 200.0
        for s in range(len(case.tot)):     # _attention_refs' arithmetic (scores -> bf16, / sqrt(d) -> bf16, fp32 softmax -> bf16, P.V)
            seen[s] |= set(data.pi[s].reshape(-1).tolist())
            q = data.q[s].view(case.hk, case.g, case.D)
            _, eager = G._attention_refs(q, data.k[s].transpose(0, 1), data.v[s].transpose(0, 1))
            assert torch.equal(eager, data.expect[s].view(BF).double().view(case.hk, case.g, case.D)), (name, s, rnd)
    for s, n in enumerate(case.tot):            # every launch's rounds together: keys 0, 127, 128, len - 1 and one of the last chunk
        want = {x for x in (0, 127, 128, n - 1) if x < n}
        assert want <= seen[s], (name, s, want - seen[s])
        assert any(x >= 128 * ((n - 1) // 128) for x in seen[s])


def test_decode_lengths_and_pairs_are_the_decode_tests_own():
    """Compared as data: the parametrize mark of the decode test (tests/test_gpu_decode_ops.py keeps its pairs there, not under a name)."""
    import test_gpu_decode_ops as G
    assert G.LENS == DECODE_LENS
    marks = [m for m in G.test_decode_attention_matches_fp64_at_ragged_lengths.pytestmark if m.name == "parametrize" and m.args[0] == "g,n_kv"]
    assert len(marks) == 1 and [tuple(p) for p in marks[0].args[1]] == DECODE_PAIRS
