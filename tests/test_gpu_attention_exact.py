"""Bit-exact tests (MI355X only) of the attention kernels on the two constructions of tests/attention_exact_reference.py, whose softmax is
exact in every correct evaluation order: the key census (Q = 0: the output is the COUNT of visible keys per column over their number - a
dropped or extra key, another sequence's or kv head's V flips bits) and the one-hot selector (the output is the selected V row - a wrong
K row, head map or rescale flips bits).  The statistical bar of the other attention tests cannot see one key in a thousand.

Staged as tests/test_gpu_ops.py::run_attention, tests/test_gpu_attention_forms.py::Staged and tests/test_gpu_decode_ops.py::_decode_attention
stage their cases.  Outputs start as the 0x7FA5 sentinel with pad rows behind the last sequence, caches as 0x7FB3, the decode workspace as
NaN; the WHOLE output allocation is compared with torch.equal on its int16 view.  tests/test_attention_exact_cpu.py holds, without a
GPU, the conditions both constructions rest on."""
import contextlib
import functools
import math

import pytest
import torch

from attention_exact_reference import (BF, DECODE_CAP, DECODE_LONG, DECODE_PAIRS, DECODE_ROUNDS, EX_NAMES, ONCE, PACKED, PACKED_IDS, Q_TAILS,
                                       TRIM_CASE, decode_case, ex_case, packed_case, rope_case)
from attention_reference import N_POS, rope_table

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5          # a NaN bit pattern no kernel produces
CACHE_FILL = 0x7FB3        # another one, for cache rows and slots nothing may read
PAD = 3                    # output rows behind the last sequence
CONSTRUCTIONS = ["census", "selector"]


@pytest.fixture(scope="module")
def lib():
    from aigv_assessor_amd import native
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(t):
    """Upload and KEEP a reference until the test ends: kernels run asynchronously on raw pointers."""
    d = t.cuda().contiguous()
    _KEEP.append(d)
    return d


def sync(rc):
    from aigv_assessor_amd import native
    native.check(rc)
    torch.cuda.synchronize()


def pattern(shape, bits):
    t = torch.full(shape, bits, dtype=torch.int16, device="cuda").view(BF)
    _KEEP.append(t)
    return t


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


@contextlib.contextmanager
def tuned(lib, knob):
    """aigv_tune_attention: 0 = the default form (4 waves per workgroup), 8 = the 8-wave form kept for A/B; restored afterwards."""
    sync(lib.aigv_tune_attention(knob))
    try:
        yield
    finally:
        sync(lib.aigv_tune_attention(0))


@functools.lru_cache(maxsize=2)        # (the parameters that share a case's host tensors are adjacent)
def host(kind, name, construction):
    case = {"packed": packed_case, "ex": ex_case, "rope": lambda _: rope_case()}[kind](name)
    data = case.census() if construction == "census" else case.selector()
    return case, data, data.fused()


def identity_table(d, n_pos):
    return torch.ones(n_pos, d // 2, dtype=BF), torch.zeros(n_pos, d // 2, dtype=BF)


def tables(case, construction, n_pos):
    """The census runs with the real rotary tables (a rotated zero is zero; K may be anything), the selector with cos = 1, sin = 0: the
    rotation x * 1 + rot * 0 is then the identity in bf16."""
    return rope_table(case.D, n_pos) if construction == "census" else identity_table(case.D, n_pos)


def expect_whole(expect, written=None):
    """The expected bits of the whole allocation [rows + PAD, h * D]: unwritten rows and the pad keep the sentinel."""
    T = expect.shape[0]
    e = expect.reshape(T, -1).clone()
    if written is not None:
        e[~written] = torch.tensor(SENTINEL, dtype=torch.int16)
    return torch.cat([e, torch.full((PAD, e.shape[1]), SENTINEL, dtype=torch.int16)])


def assert_bits(got, want, case, what):
    got = got.cpu().view(torch.int16)
    if torch.equal(got, want):
        return
    T, h, D = got.shape[0], case.h, case.D
    bad = (got != want).view(T, h, D)
    rows = bad.any(-1).any(-1).nonzero().flatten()
    r = int(rows[0])
    hq = int(bad[r].any(-1).nonzero()[0])
    cols = bad[r, hq].nonzero().flatten().tolist()[:4]
    g16, w16 = got.view(T, h, D)[r, hq], want.view(T, h, D)[r, hq]
    raise AssertionError(f"{case.name} {what}: {int(bad.sum())} elements of {len(rows)} rows differ; first: row {r} head {hq} columns {cols}: "
                         f"got {[hex(int(g16[c]) & 0xffff) for c in cols]} want {[hex(int(w16[c]) & 0xffff) for c in cols]}; rows {rows.tolist()[:12]}")


# ---------------------------------------------------------------------------------------------------------
# packed prefill: aigv_op_attention / aigv_op_attention_rope
# ---------------------------------------------------------------------------------------------------------
def run_packed(lib, case, rows, flags, rope=None):
    """As run_attention: the fused rows are q, k and v at once.  -> the whole output allocation [T + PAD, h * D]."""
    from aigv_assessor_amd.native import ptr
    d, g, h, hk, lens = case.D, case.g, case.h, case.hk, case.cnts
    T, ld = rows.shape[0], hk * (g + 2) * d
    x = dev(rows.clone())
    out = pattern((T + PAD, h * d), SENTINEL)
    base = x.data_ptr()
    args = (base, ld, base + g * d * 2, ld, base + (g + 1) * d * 2, ld, ptr(out), h * d, ptr(dev(cu_of(lens))), len(lens), max(lens), h, hk,
            (g + 2) * d, (g + 2) * d, d, flags, case.post, case.pre)
    if rope is None:
        sync(lib.aigv_op_attention(*args, None))
    else:
        pos, cos, sin = dev(case.pos), dev(rope[0]), dev(rope[1])
        sync(lib.aigv_op_rope(base + g * d * 2, ld, ptr(pos), ptr(cos), ptr(sin), T, 1, g + 2, hk, d, None))      # K rotated in memory, Q in the kernel
        sync(lib.aigv_op_attention_rope(*args, ptr(pos), ptr(cos), ptr(sin), None))
    return out


PACKED_PARAMS = [(n, lead) for n, *_, leads in PACKED for lead in leads if n != ONCE]


@pytest.mark.parametrize("knob", [0, 8])
@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("construction", CONSTRUCTIONS)
@pytest.mark.parametrize("name,lead_key", PACKED_PARAMS, ids=[f"{n}{'-lead' if lead else ''}" for n, lead in PACKED_PARAMS])
def test_packed_prefill_is_exact(lib, name, lead_key, construction, round_scores, knob):
    """Every visible key counted once and no other (ragged last tile, causal diagonal, the key-split 1025th row, the lead key, the last
    partial query block, every group size of the causal block remap), from the row's own sequence and kv head; the selected V row of
    the selected kv head under a maximum that arrives anywhere in the key range."""
    _packed_exact(lib, name, lead_key, construction, round_scores, knob)


@pytest.mark.parametrize("construction", CONSTRUCTIONS)
def test_the_canonical_clip_is_exact(lib, construction):
    """2176 rows, 34 key tiles, 17 query blocks: once per construction (default kernel, fp32 scores)."""
    _packed_exact(lib, ONCE, False, construction, False, 0)


def _packed_exact(lib, name, lead_key, construction, round_scores, knob):
    case, data, rows = host("packed", name, construction)
    uniform = PACKED[PACKED_IDS.index(name)][6] and knob == 0
    flags = int(case.causal) | (2 if uniform else 0) | (4 if round_scores else 0) | (8 if lead_key else 0)
    with tuned(lib, knob):
        out = run_packed(lib, case, rows, flags)
    assert_bits(out, expect_whole(data.expect), case, f"{construction} knob {knob} round_scores {round_scores} lead {lead_key}")


@pytest.mark.parametrize("knob", [0, 8])
@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("construction", CONSTRUCTIONS)
def test_prefill_with_fused_query_rope_is_exact(lib, construction, round_scores, knob):
    case, data, rows = host("rope", "", construction)
    with tuned(lib, knob):
        out = run_packed(lib, case, rows, 1 | (4 if round_scores else 0), rope=tables(case, construction, max(case.cnts)))
    assert_bits(out, expect_whole(data.expect), case, f"{construction} knob {knob} round_scores {round_scores}")


# ---------------------------------------------------------------------------------------------------------
# continuation over the KV cache: aigv_op_attention_ex
# ---------------------------------------------------------------------------------------------------------
class StagedEx:
    """As test_gpu_attention_forms.Staged: all tokens' fused rows with the K slot rotated by aigv_op_rope, caches [n_seq + 1 slots][hk][cap][D]
    of CACHE_FILL written by aigv_op_kv_store, the packed new rows with their K / V slots overwritten by CACHE_FILL."""

    def __init__(self, lib, case, rows, rope):
        from aigv_assessor_amd.native import ptr
        c = self.case = case
        g, hk, cap, D = c.g, c.hk, c.cap, c.D
        self.ld = ld = hk * (g + 2) * D
        self.cos, self.sin = dev(rope[0]), dev(rope[1])
        pos_all = dev(c.pos)
        x = dev(rows.clone())
        T_all = x.shape[0]
        sync(lib.aigv_op_rope(x.data_ptr() + g * D * 2, ld, ptr(pos_all), ptr(self.cos), ptr(self.sin), T_all, 1, g + 2, hk, D, None))
        n_seq = len(c.offs)
        self.kc = pattern((n_seq + 1, hk, cap, D), CACHE_FILL)
        self.vc = pattern((n_seq + 1, hk, cap, D), CACHE_FILL)
        sync(lib.aigv_op_kv_store(ptr(x), ld, ptr(dev(c.seq)), ptr(pos_all), ptr(self.kc), ptr(self.vc), T_all, hk, g, D, cap, None))
        new = x[c.new_idx.cuda()].clone().view(-1, hk, g + 2, D)
        new.view(torch.int16)[:, :, g:] = CACHE_FILL
        self.new = new.view(-1, ld)
        _KEEP.append(self.new)
        self.cu = dev(cu_of(c.cnts))
        self.kv_off = dev(torch.tensor(c.offs, dtype=torch.int32))
        self.pos_new = dev(c.pos[c.new_idx])
        self.zeros = dev(torch.zeros(len(c.new_idx), dtype=torch.int32))

    def attend(self, lib, round_scores, pos_is_row, q_tail=0):
        from aigv_assessor_amd.native import ptr
        c, D = self.case, self.case.D
        T = self.new.shape[0]
        out = pattern((T + PAD, c.h * D), SENTINEL)
        # the computed position is handed a table of zeros it must not read; the table form the positions kv_off + row
        sync(lib.aigv_op_attention_ex(ptr(self.new), self.ld, ptr(self.kc), D, ptr(self.vc), D, ptr(out), c.h * D, ptr(self.cu), len(c.cnts),
                                      max(c.cnts), c.h, c.hk, (c.g + 2) * D, c.cap * D, c.hk * c.cap * D, ptr(self.kv_off), D,
                                      1 | (4 if round_scores else 0), c.post, 1.0, ptr(self.zeros if pos_is_row else self.pos_new), ptr(self.cos),
                                      ptr(self.sin), 1 if pos_is_row else 0, q_tail, None))
        return out


@pytest.mark.parametrize("knob", [0, 8])
@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("construction", CONSTRUCTIONS)
@pytest.mark.parametrize("name", EX_NAMES)
def test_continuation_over_the_cache_is_exact(lib, name, construction, round_scores, knob):
    """New row r of every sequence counts exactly the keys 0 .. kv_off + r of ITS cache slot and kv head (cache layout, kv_off, both forms
    of the rotary position), and hands back the selected cached or new V row."""
    case, data, rows = host("ex", name, construction)
    st = StagedEx(lib, case, rows, tables(case, construction, N_POS))
    want = expect_whole(data.expect)
    with tuned(lib, knob):
        for pos_is_row in (1, 0):
            assert_bits(st.attend(lib, round_scores, pos_is_row), want, case, f"{construction} knob {knob} round_scores {round_scores} pos_is_row {pos_is_row}")


def waves_written(lens, q_tail):
    """kernels.h AttnArgs::q_tail: waves are cut every 32 rows from a sequence's first row; a wave that ends at or in front of the first
    consumed row (len - q_tail) writes nothing, every other row is computed.  (attn_fwd_kernel in csrc/attention.hip: the block return
    `q0 + QB <= len - p.q_tail` and `trimmed = p.q_tail > 0 && qw + 32 <= len - p.q_tail`, 32 query rows per wave in both kernel forms.
    A change of the wave height changes this contract: it is then this expectation that moves, with kernels.h.)"""
    keep = []
    for n in lens:
        r = torch.arange(n)
        keep.append((r // 32) * 32 + 32 > n - q_tail)
    return torch.cat(keep)


@pytest.mark.parametrize("knob", [0, 8])
@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("construction", CONSTRUCTIONS)
def test_row_trimming_behind_a_cache_offset_is_exact(lib, construction, round_scores, knob):
    """q_tail: the consumed rows are exact, the whole 32-row waves in front of them still hold the sentinel, the rest is exact as untrimmed."""
    case, data, rows = host("ex", TRIM_CASE, construction)
    st = StagedEx(lib, case, rows, tables(case, construction, N_POS))
    with tuned(lib, knob):
        for q_tail in Q_TAILS:
            want = expect_whole(data.expect, waves_written(case.cnts, q_tail))
            assert_bits(st.attend(lib, round_scores, 1, q_tail), want, case, f"{construction} knob {knob} round_scores {round_scores} q_tail {q_tail}")


# ---------------------------------------------------------------------------------------------------------
# decode: aigv_op_attention_decode
# ---------------------------------------------------------------------------------------------------------
def run_decode(lib, case, q, kc, vc, max_kv_len):
    """As _decode_attention: q [n_seq, h, D] in fused rows whose K / V slots are NaN, a NaN workspace.  -> [n_seq + PAD, h * D]."""
    n_seq, n_kv, g, D, cap = len(case.tot), case.hk, case.g, case.D, case.cap
    fused = torch.full((n_seq, n_kv, g + 2, D), float("nan"), dtype=BF, device="cuda")
    fused[:, :, :g] = q.view(n_seq, n_kv, g, D).cuda()
    o = pattern((n_seq + PAD, n_kv * g * D), SENTINEL)
    nws = lib.aigv_op_attention_decode_ws_floats(n_seq, n_kv, g, cap)
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    dlens = torch.tensor(case.tot, dtype=torch.int32, device="cuda")
    _KEEP.extend([fused, ws, dlens])
    sync(lib.aigv_op_attention_decode(fused.data_ptr(), n_kv * (g + 2) * D, (g + 2) * D, kc.data_ptr(), vc.data_ptr(), dlens.data_ptr(), cap,
                                      o.data_ptr(), n_kv * g * D, n_seq, n_kv, g, D, math.sqrt(D), max_kv_len, ws.data_ptr(), nws, None))
    return o


def decode_caches(case, data):
    """[n_seq][n_kv][cap][D] caches of CACHE_FILL holding sequence b's keys / values in rows 0 .. len - 1."""
    kc = pattern((len(case.tot), case.hk, case.cap, case.D), CACHE_FILL)
    vc = pattern((len(case.tot), case.hk, case.cap, case.D), CACHE_FILL)
    for b, (k, v) in enumerate(zip(data.k, data.v)):
        kc[b, :, : k.shape[0]] = k.transpose(0, 1).cuda()
        vc[b, :, : v.shape[0]] = v.transpose(0, 1).cuda()
    return kc, vc


def _decode_exact(lib, case, construction):
    data = case.census() if construction == "census" else case.selector()
    kc, vc = decode_caches(case, data)
    for rnd in range(1 if construction == "census" else DECODE_ROUNDS):      # the selector's rounds rotate every head over every aim
        if rnd:
            data = case.selector(rnd, base=data)
        out = run_decode(lib, case, torch.cat(data.q), kc, vc, max(case.tot))
        assert_bits(out, expect_whole(data.expect), case, f"{construction} round {rnd}")


@pytest.mark.parametrize("construction", CONSTRUCTIONS)
@pytest.mark.parametrize("g,n_kv", DECODE_PAIRS)
def test_decode_is_exact_at_ragged_lengths(lib, g, n_kv, construction):
    """Every instantiation over the ragged lengths in one launch with max_kv_len < cap: every key below kv_len in every 128-key chunk and
    every chunk in the merge counted once; keys 0, 127, 128, len - 1 and one of the last chunk selected in turn."""
    _decode_exact(lib, decode_case(g, n_kv), construction)


@pytest.mark.parametrize("construction", CONSTRUCTIONS)
def test_decode_is_exact_past_16k_cached_tokens(lib, construction):
    g, n_kv, lens, cap = DECODE_LONG
    _decode_exact(lib, decode_case(g, n_kv, lens, cap), construction)
