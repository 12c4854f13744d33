"""Op-level parity tests (MI355X only) of the address and mask forms of the prefill attention kernel that the scoring passes use and
aigv_op_attention / aigv_op_attention_rope cannot reach: keys in front of the first query row (kv_off: aigv_llm_extend, the shared-prefix
scoring), K / V read from the KV cache layout (kv_seq_stride), last-layer row trimming (q_tail) and the computed rotary position
(rope_pos_is_row).  Everything goes through aigv_op_attention_ex, which fills AttnArgs as the passes do, and the cache is written by
aigv_op_kv_store, the passes' own append kernel.

Continuations are held against fp64 truth with the rule of tests/test_gpu_ops.py::_attention_case (attention_reference.check_sequence: at
least as accurate as the reference's eager bf16 path; with round_scores much closer to that path than it is to truth) - no other tolerance.
Everything else is bit-exact: two forms of the same arithmetic must give the same bits.

Every cache is filled with NaN bit patterns before the keys are stored, every output with a NaN sentinel of its own bit pattern: a key read
from outside the visible range, or a row written that belongs to no sequence, shows."""
import math

import pytest
import torch

from attention_reference import BF, CASE_IDS, D, check_sequence, continuation_case, rope_table

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5          # a NaN bit pattern no kernel produces (arithmetic NaNs are the quiet 0x7FC0 / 0xFFC0)
CACHE_FILL = 0x7FB3        # another one, for cache rows and slots nothing may read
POST = math.sqrt(D)


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
    """A device bf16 tensor of one 16-bit pattern."""
    t = torch.full(shape, bits, dtype=torch.int16, device="cuda").view(BF)
    _KEEP.append(t)
    return t


def bits(t):
    return t.contiguous().view(torch.int16)


def is_pattern(t, b):
    return bits(t) == b


@pytest.fixture(params=[0, 8], ids=["waves4", "waves8"])
def kernel(request, lib):
    """aigv_tune_attention: 0 = the default form (4 waves per workgroup), 8 = the 8-wave form kept for A/B; restored afterwards."""
    sync(lib.aigv_tune_attention(request.param))
    try:
        yield request.param
    finally:
        sync(lib.aigv_tune_attention(0))


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


class Staged:
    """One continuation case on the device: all tokens' fused rows with the K slot rotated (aigv_op_rope), the caches [n_seq + 1 slots]
    [hk][cap][D] filled with NaN patterns and then written by aigv_op_kv_store for the tokens 0 .. off + n - 1 of every sequence (the last
    slot belongs to no sequence), and the packed new rows with their K / V slots overwritten by NaN patterns (a continuation reads K / V
    from the cache only)."""

    def __init__(self, lib, case):
        from aigv_assessor_amd.native import ptr
        c = self.case = case
        g, hk, cap = c.g, c.hk, c.cap
        self.ld = ld = hk * (g + 2) * D
        self.cos, self.sin = dev(c.cos), dev(c.sin)
        self.pos_all = dev(c.pos)
        self.rows = dev(c.rows.clone())
        T_all = self.rows.shape[0]
        sync(lib.aigv_op_rope(self.rows.data_ptr() + g * D * 2, ld, ptr(self.pos_all), ptr(self.cos), ptr(self.sin), T_all, 1, g + 2, hk, D, None))
        n_seq = len(c.offs)
        self.kc = pattern((n_seq + 1, hk, cap, D), CACHE_FILL)
        self.vc = pattern((n_seq + 1, hk, cap, D), CACHE_FILL)
        sync(lib.aigv_op_kv_store(ptr(self.rows), ld, ptr(dev(c.seq)), ptr(self.pos_all), ptr(self.kc), ptr(self.vc), T_all, hk, g, D, cap, None))
        new = self.rows[c.new_idx.cuda()].clone().view(-1, hk, g + 2, D)
        bits(new)[:, :, g:] = CACHE_FILL
        self.new = new.view(-1, ld)
        _KEEP.append(self.new)
        self.cu = dev(cu_of(c.cnts))
        self.kv_off = dev(torch.tensor(c.offs, dtype=torch.int32))
        self.pos_new = dev(c.pos[c.new_idx])          # = kv_off[seq] + row

    def attend(self, lib, round_scores, q_tail=0, pos_is_row=True, pos=None, pad=3):
        """The new rows over the cached keys plus their own.  Returns [T + pad, h, D] (cpu): the pad rows belong to no sequence."""
        from aigv_assessor_amd.native import ptr
        c = self.case
        T = self.new.shape[0]
        out = pattern((T + pad, c.h * D), SENTINEL)
        sync(lib.aigv_op_attention_ex(ptr(self.new), self.ld, ptr(self.kc), D, ptr(self.vc), D, ptr(out), c.h * D, ptr(self.cu), len(c.cnts),
                                      max(c.cnts), c.h, c.hk, (c.g + 2) * D, c.cap * D, c.hk * c.cap * D, ptr(self.kv_off), D,
                                      1 | (4 if round_scores else 0), POST, 1.0, ptr(self.pos_new if pos is None else pos), ptr(self.cos),
                                      ptr(self.sin), 1 if pos_is_row else 0, q_tail, None))
        return out.cpu().view(T + pad, c.h, D)

    def prefill(self, lib, round_scores):
        """The same tokens as ONE packed prefill through aigv_op_attention_rope (K / V: the packed rows).  Returns the new rows' outputs."""
        from aigv_assessor_amd.native import ptr
        c = self.case
        g, ld = c.g, self.ld
        lens = [o + n for o, n in zip(c.offs, c.cnts)]
        T_all = self.rows.shape[0]
        out = pattern((T_all, c.h * D), SENTINEL)
        base = self.rows.data_ptr()
        sync(lib.aigv_op_attention_rope(base, ld, base + g * D * 2, ld, base + (g + 1) * D * 2, ld, ptr(out), c.h * D, ptr(dev(cu_of(lens))), len(lens),
                                        max(lens), c.h, c.hk, (g + 2) * D, (g + 2) * D, D, 1 | (4 if round_scores else 0), POST, 1.0,
                                        ptr(self.pos_all), ptr(self.cos), ptr(self.sin), None))
        return out.cpu().view(T_all, c.h, D)[c.new_idx]


def check_continuation(case, got, round_scores):
    """got [T + pad, h, D]: every sequence against fp64 truth with the suite's acceptance rule; rows of no sequence untouched."""
    T = sum(case.cnts)
    assert is_pattern(got[T:], SENTINEL).all(), "rows behind the last sequence were written"
    assert torch.isfinite(got[:T].float()).all(), "a result row is not finite: something outside the visible keys was read"
    near = far = 0.0
    off = 0
    for (truth, eager), n in zip(case.references(), case.cnts):
        dn, df = check_sequence(got[off: off + n].double(), truth, eager)
        near += dn
        far += df
        off += n
    print(f"{case.name}: sum |hip - eager bf16| / sum |eager bf16 - fp64 truth| = {near / max(far, 1e-30):.3f} (round_scores={round_scores})")
    if round_scores:
        assert near <= 0.75 * far, (near, far)


@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("name", CASE_IDS)
def test_continuation_matches_fp64_truth_and_reads_nothing_outside_the_visible_keys(lib, kernel, name, round_scores):
    """New rows behind keys in the KV cache (kv_off, kv_seq_stride, computed rotary positions), each sequence against float64 truth over
    the concatenated keys with the mask "new row r sees keys 0 .. kv_off + r".  The cache rows at and past kv_off + len of every sequence,
    the slot of no sequence, and the K / V slots of the packed query rows hold NaN patterns: a finite result that meets the rule has read
    none of them; the output rows of no sequence still hold their sentinel."""
    case = continuation_case(name)
    st = Staged(lib, case)
    check_continuation(case, st.attend(lib, round_scores), round_scores)
    # the staging itself: the cache rows past every sequence and the spare slot still hold the fill
    for s, (o, n) in enumerate(zip(case.offs, case.cnts)):
        assert is_pattern(st.kc[s, :, o + n:], CACHE_FILL).all() and is_pattern(st.vc[s, :, o + n:], CACHE_FILL).all()
    assert is_pattern(st.kc[-1], CACHE_FILL).all() and is_pattern(st.vc[-1], CACHE_FILL).all()


TRIM_CASE = "ragged-g3"
PREFILL_CASES = ["off0-g1", "off64-g6", "off128-g3", "off2176-g6", "ragged-2176-63-0", "scoring-g6x8", "off63-g4", "off2177-g8", "ragged-2169-2176"]


@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("name", PREFILL_CASES)
def test_continuation_equals_the_one_piece_prefill(lib, kernel, name, round_scores):
    """The same tokens as one packed prefill (aigv_op_attention_rope) and as prefix-in-cache plus continuation: the continuation's rows.

    What the tile loop bears out: a query row runs the 64-key tiles 0 .. (its wave's last visible key) / 64 in order in both runs (the
    block's tile count is never below that, and tiles in a wave's causal future are skipped per wave), masked keys enter as exp2(-inf) = 0
    and as exact zeros of the P V product, and keys past the sequence are never loaded (the last tile re-reads the last valid row).  ONE
    thing depends on a row's neighbours: the lazy rescale moves the running maximum of all 32 rows of a wave when ANY of them sees a
    jump (__any), and a row's un-normalised P rounds to bf16 relative to that maximum.  Waves are cut every 32 rows from the first QUERY
    row, so the two runs group the rows alike exactly when the key offset is a multiple of 32: then the bits must be equal.  For other
    offsets a row has other wave mates, the same softmax is evaluated against another reference maximum, and the results differ by
    rounding noise: the bound of the lead-key test (another evaluation order of the same softmax) applies - within one bf16 ulp of the
    row's scale, mean difference below 2^-10 of the mean magnitude."""
    case = continuation_case(name)
    st = Staged(lib, case)
    T = sum(case.cnts)
    a = st.attend(lib, round_scores)[:T]
    b = st.prefill(lib, round_scores)
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    off = 0
    for o, n in zip(case.offs, case.cnts):
        x, y = a[off: off + n], b[off: off + n]
        if o % 32 == 0:
            assert torch.equal(x, y), (name, o, n, (x.float() - y.float()).abs().max().item())
        else:
            x, y = x.float(), y.float()
            scale = y.abs().amax(-1, keepdim=True).clamp_min(1e-3)
            assert ((x - y).abs() <= 2.0 ** -7 * scale).all(), (name, o, n, ((x - y).abs() / scale).max().item())
            assert (x - y).abs().mean().item() <= 2.0 ** -10 * y.abs().mean().item(), (name, o, n)
        off += n


def waves_written(lens, q_tail):
    """Row trimming's contract (kernels.h AttnArgs::q_tail): waves are cut every 32 rows from a sequence's first row; the rows of a wave
    that ends at or in front of the first consumed row (len - q_tail) are left unwritten, every other row is computed."""
    keep = []
    for n in lens:
        r = torch.arange(n)
        keep.append((r // 32) * 32 + 32 > n - q_tail)
    return torch.cat(keep)


def check_trimmed(full, got, lens, q_tail, what):
    """full / got [T, h, D] of the q_tail = 0 launch and the trimmed one."""
    same = (bits(full) == bits(got)).all(-1).all(-1)
    untouched = is_pattern(got, SENTINEL).all(-1).all(-1)
    off = 0
    for n in lens:
        assert same[off + max(0, n - q_tail): off + n].all(), f"{what}: a consumed row differs from the untrimmed launch"
        off += n
    assert (same | untouched).all(), f"{what}: a row is neither the untrimmed launch's nor left alone"
    want = waves_written(lens, q_tail)
    assert torch.equal(same, want) and torch.equal(untouched, ~want), f"{what}: rows written {same.nonzero().flatten().tolist()[:8]}.."


Q_TAILS = [1, 4, 16, 33, 128, 129]


@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("h,hk,lens", [(8, 2, [2176]), (6, 1, [513, 64, 1]), (8, 2, [300, 77, 129])])
def test_row_trimming_computes_the_consumed_rows_and_leaves_the_rest(lib, kernel, h, hk, lens, round_scores):
    """q_tail (the default form of every scoring pass's last layer) on a packed prefill: the last q_tail rows of every sequence carry the
    bits of the q_tail = 0 launch; every other row either carries them too (a wave that computes extra rows computes them correctly) or
    was left alone - and which ones is the contract: whole 32-row waves in front of the consumed rows write nothing."""
    from aigv_assessor_amd.native import ptr
    g = h // hk
    T, ld = sum(lens), hk * (g + 2) * D
    gen = torch.Generator().manual_seed(11 + T + h)
    qkv = torch.randn(T, ld, generator=gen).to(BF)
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32)
    cos, sin = rope_table(D, max(lens))
    x, dpos, dcos, dsin, dcu = dev(qkv), dev(pos), dev(cos), dev(sin), dev(cu_of(lens))
    base = x.data_ptr()
    sync(lib.aigv_op_rope(base + g * D * 2, ld, ptr(dpos), ptr(dcos), ptr(dsin), T, 1, g + 2, hk, D, None))

    def run(q_tail):
        out = pattern((T, h * D), SENTINEL)
        sync(lib.aigv_op_attention_ex(base, ld, base + g * D * 2, ld, base + (g + 1) * D * 2, ld, ptr(out), h * D, ptr(dcu), len(lens), max(lens),
                                      h, hk, (g + 2) * D, (g + 2) * D, 0, None, D, 1 | (4 if round_scores else 0), POST, 1.0, ptr(dpos), ptr(dcos),
                                      ptr(dsin), 1, q_tail, None))
        return out.cpu().view(T, h, D)
    full = run(0)
    assert torch.isfinite(full.float()).all()
    for q_tail in Q_TAILS + [max(lens), max(lens) + 7]:
        check_trimmed(full, run(q_tail), lens, q_tail, f"lens {lens} q_tail {q_tail}")


@pytest.mark.parametrize("round_scores", [True, False])
def test_row_trimming_behind_a_cache_offset(lib, kernel, round_scores):
    """The early return of the trimmed blocks and waves counts QUERY rows, the causal limit and the tile count count keys: both at once."""
    case = continuation_case(TRIM_CASE)
    st = Staged(lib, case)
    T = sum(case.cnts)
    full = st.attend(lib, round_scores)
    check_continuation(case, full, round_scores)
    for q_tail in (1, 16, 33, 129):
        got = st.attend(lib, round_scores, q_tail=q_tail)
        assert is_pattern(got[T:], SENTINEL).all()
        check_trimmed(full[:T], got[:T], case.cnts, q_tail, f"{case.name} q_tail {q_tail}")


ROPE_CASES = ["off0-g1", "ragged-2176-63-0", "ragged-g3"]


@pytest.mark.parametrize("round_scores", [True, False])
@pytest.mark.parametrize("name", ROPE_CASES)
def test_computed_rotary_position_equals_the_position_table(lib, kernel, name, round_scores):
    """rope_pos_is_row (the default of every prefill and continuation): position = kv_off[seq] + row computed by the kernel, against the
    table form fed exactly those positions - the same bits.  The computed form is handed a table of zeros: it must not read it.
    off0-g1 is the packed-prefill situation (offset 0), the ragged cases mix offsets in one launch."""
    case = continuation_case(name)
    st = Staged(lib, case)
    zeros = dev(torch.zeros(sum(case.cnts), dtype=torch.int32))
    a = st.attend(lib, round_scores, pos_is_row=True, pos=zeros)
    b = st.attend(lib, round_scores, pos_is_row=False, pos=st.pos_new)
    assert torch.isfinite(a[: sum(case.cnts)].float()).all()
    assert torch.equal(bits(a), bits(b))
    if any(case.offs) or max(case.cnts) > 1:       # and the table IS what the table form reads
        c = st.attend(lib, round_scores, pos_is_row=False, pos=zeros)
        assert not torch.equal(bits(a), bits(c))


def test_computed_rotary_position_on_a_packed_prefill(lib, kernel):
    """The same on packed K / V (no cache, no offset): aigv_op_attention_ex with pos_is_row against aigv_op_attention_rope with the table."""
    from aigv_assessor_amd.native import ptr
    h, hk, lens = 6, 1, [300, 77, 129]
    g = h // hk
    T, ld = sum(lens), hk * (g + 2) * D
    qkv = torch.randn(T, ld, generator=torch.Generator().manual_seed(5)).to(BF)
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32)
    cos, sin = rope_table(D, max(lens))
    x, dpos, dcos, dsin, dcu = dev(qkv), dev(pos), dev(cos), dev(sin), dev(cu_of(lens))
    zeros = dev(torch.zeros(T, dtype=torch.int32))
    base = x.data_ptr()
    sync(lib.aigv_op_rope(base + g * D * 2, ld, ptr(dpos), ptr(dcos), ptr(dsin), T, 1, g + 2, hk, D, None))
    a, b = pattern((T, h * D), SENTINEL), pattern((T, h * D), SENTINEL)
    head = (base, ld, base + g * D * 2, ld, base + (g + 1) * D * 2, ld)
    mid = (ptr(dcu), len(lens), max(lens), h, hk, (g + 2) * D, (g + 2) * D)
    sync(lib.aigv_op_attention_ex(*head, ptr(a), h * D, *mid, 0, None, D, 5, POST, 1.0, ptr(zeros), ptr(dcos), ptr(dsin), 1, 0, None))
    sync(lib.aigv_op_attention_rope(*head, ptr(b), h * D, *mid, D, 5, POST, 1.0, ptr(dpos), ptr(dcos), ptr(dsin), None))
    assert torch.isfinite(a.float()).all()
    assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("g,hk,cap", [(1, 2, 2441), (4, 2, 333), (6, 1, 2441), (6, 8, 97)])
def test_kv_store_is_a_scatter(lib, g, hk, cap):
    """aigv_op_kv_store against a torch scatter, bit for bit: ragged seq / pos (sequences in any order, positions with gaps, the last row
    of the capacity), capacities that are no multiple of 64; every cache row that is not addressed keeps its sentinel."""
    from aigv_assessor_amd.native import ptr
    gen = torch.Generator().manual_seed(g * 100 + hk)
    n_seq, ld = 4, hk * (g + 2) * D + 8        # (a row stride with padding behind the last group)
    seq, pos = [], []
    for s, (first, n) in enumerate([(0, min(70, cap)), (cap - 1, 1), (5, min(33, cap - 5)), (min(63, cap - 3), 2)]):
        if s == 2:
            continue                           # a slot no token addresses
        seq += [s] * n
        pos += list(range(first, first + n))
    perm = torch.randperm(len(seq), generator=gen)
    seq, pos = torch.tensor(seq, dtype=torch.int32)[perm], torch.tensor(pos, dtype=torch.int32)[perm]
    T = len(seq)
    qkv = torch.randn(T, ld, generator=gen).to(BF)
    kc, vc = pattern((n_seq, hk, cap, D), SENTINEL), pattern((n_seq, hk, cap, D), SENTINEL)
    want_k, want_v = kc.cpu().clone(), vc.cpu().clone()
    rows = qkv[:, : hk * (g + 2) * D].view(T, hk, g + 2, D)
    want_k[seq.long(), :, pos.long()] = rows[:, :, g]
    want_v[seq.long(), :, pos.long()] = rows[:, :, g + 1]
    src = dev(qkv)
    sync(lib.aigv_op_kv_store(ptr(src), ld, ptr(dev(seq)), ptr(dev(pos)), ptr(kc), ptr(vc), T, hk, g, D, cap, None))
    assert torch.equal(bits(kc.cpu()), bits(want_k)) and torch.equal(bits(vc.cpu()), bits(want_v))
    assert is_pattern(kc[2], SENTINEL).all() and torch.equal(bits(src.cpu()), bits(qkv))
