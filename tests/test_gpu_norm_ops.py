"""Op-level tests (MI355X only) of the normalisation kernels - layernorm_kernel, layernorm_wave_kernel<2> and <4>, rmsnorm_kernel in its plain,
row-index, strided and in-place forms, lens_tap_kernel and rmsnorm_quant_fp8_kernel - against the fp64 truth of tests/norm_reference.py, under
the acceptance rules tests/test_norm_reference_cpu.py proves: a faithful float32 evaluation passes them in either order of summation and with
rsqrt moved by +-2 ulps, and a kernel that loses one column, chunk or wave of its sum, divides by H - 1, ignores or misreads eps, rounds in
the wrong place or drops the bias does not.

Every output sits between two fences and keeps sentinel padding columns where ldy > H; the WHOLE allocation is compared (the normalised
columns under the rule, everything else bit for bit).  Padding columns of an input hold NaN: reading one poisons the row's statistics.  No
non-finite value is fed to an operand."""
import numpy as np
import pytest
import torch

import norm_reference as N
from test_gpu_ops import BF, dev, lib, sync, _quant_ref, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import fenced, ptr, same_bits, sentinel_like

pytestmark = pytest.mark.gpu


def padded_input(x, ld):
    """[R, H] bf16 -> device [R, ld] with NaN padding columns."""
    R, H = x.shape
    xp = torch.full((R, ld), float("nan"), dtype=BF)
    xp[:, :H] = x
    return dev(xp)


def take_output(whole, y, H):
    """The [R, :H] region of a fenced output as a float32 array, after the rest of the allocation - fences and padding columns - has been compared
    with the sentinel bit for bit."""
    got = y.cpu()
    image = sentinel_like(tuple(got.shape), got.dtype)
    image[:, :H] = got[:, :H]
    same_bits(whole, image)
    return N.to_np(got[:, :H].contiguous())


def launch(lib, c, rows, ldx=None, ldy=None, row_idx=None):
    """One launch of the op of case c on rows `rows` (a list) of its operand.  row_idx (RMSNorm): the operand is handed over whole and the kernel
    picks the rows itself."""
    H, op = c["H"], c["op"]
    ldx, ldy = ldx or H, ldy or H
    x = padded_input(c["x"] if row_idx else c["x"][rows], ldx)
    w = dev(c["w"])
    whole, y = fenced(sentinel_like((len(rows), ldy), BF))
    if op == "ln":
        sync(lib.aigv_op_layernorm(ptr(x), ldx, ptr(w), ptr(dev(c["b"])), ptr(y), ldy, len(rows), H, c["eps"], None), lib)
    else:
        idx = ptr(dev(torch.tensor(rows, dtype=torch.int32))) if row_idx else None
        sync(lib.aigv_op_rmsnorm(ptr(x), ldx, ptr(w), ptr(y), ldy, len(rows), H, c["eps"], idx, None), lib)
    return take_output(whole, y, H)


def accept(c, rule, got, rows, what):
    why = rule(c, got, rows)
    differ = int((N.bits(got) != N.bits(N.to_np(c["want"][rows]))).sum())
    print(f"{c['op']} H={c['H']} eps={c['eps']:g} {what}: {differ} of {got.size} elements not bit-equal")
    assert why is None, f"{c['op']} H={c['H']} eps={c['eps']:g} {what}: {why}"


ALL = list(range(N.DENSE_ROWS))
FIVE = list(range(9, 14))           # 4 + 1: the second block of a 4-rows-per-block kernel holds one row
ONE = [4]                           # the mean-40 row, alone


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("op,H", [("ln", H) for H in N.LN_H] + [("rms", H) for H in N.RMS_H])
def test_dense_rows_against_the_fp64_truth(lib, op, H, eps):
    """rows = 37, 5 and 1 (9 blocks + 1 row, 1 block + 1 row, and a lone row of the wave kernels), contiguous and with ldx = H + 24, ldy = H + 16.
    The rule is applied to the case as a whole: all the launches' rows together."""
    c = N.dense_case(op, H, eps)
    plain = launch(lib, c, ALL)
    strided = launch(lib, c, ALL, ldx=H + 24, ldy=H + 16)
    assert np.array_equal(N.bits(plain), N.bits(strided)), "the leading dimensions changed the result"
    five = launch(lib, c, FIVE, ldx=H + 24, ldy=H + 16)
    one = launch(lib, c, ONE)
    assert np.array_equal(N.bits(five), N.bits(plain[FIVE])) and np.array_equal(N.bits(one), N.bits(plain[ONE])), "the row count changed the result"
    accept(c, N.check_dense, np.concatenate([plain, five, one]), ALL + FIVE + ONE, "rows 37 + 5 + 1")
    cls = N.classes_of(op, H)
    zeros = [r for r in ALL if cls[r % len(cls)] == "zeros"]
    want_zero = c["b"] if op == "ln" else torch.zeros(H, dtype=BF) * c["w"]             # 0 * w keeps the sign of w
    assert np.array_equal(N.bits(plain[zeros]), N.bits(N.to_np(want_zero.expand(len(zeros), H))))
    if op == "ln" and "ones" in cls:
        ones = [r for r in ALL if cls[r % len(cls)] == "ones"]
        assert np.array_equal(N.bits(plain[ones]), N.bits(N.to_np(c["b"].expand(len(ones), H)))), "a constant row must give the bias bit for bit"


@pytest.mark.parametrize("op,H", [("ln", H) for H in N.LN_SPARSE_H] + [("rms", H) for H in N.RMS_SPARSE_H])
def test_sparse_rows_every_column_decides_one_row(lib, op, H):
    c = N.sparse_case(op, H)
    rows = list(range(c["x"].shape[0]))
    accept(c, N.check_sparse, launch(lib, c, rows, ldx=H + 24, ldy=H + 16), rows, f"sparse, {len(rows)} rows")


@pytest.mark.parametrize("H", [8, 4096, 16384])
def test_rmsnorm_row_index_form(lib, H):
    """Repeated and descending indices, a strided operand: row i of the result is the norm of row idx[i] - the bits of the plain launch on those rows."""
    c = N.dense_case("rms", H, 1e-5)
    idx = [36, 36, 20, 7, 7, 4, 0]
    got = launch(lib, c, idx, ldx=H + 24, ldy=H + 16, row_idx=True)
    assert np.array_equal(N.bits(got), N.bits(launch(lib, c, idx))), "the row index changed the result"
    accept(c, N.check_dense, got, idx, "row_idx")


@pytest.mark.parametrize("H", [128, 3200])
def test_rmsnorm_in_place_on_the_middle_third_of_qkv_rows(lib, H):
    """The InternViT qk-norm's call: x == y, ld = 3 H, the operand starts at column H.  77 rows; the other two thirds of every row keep their bits."""
    rows, eps = 77, 1e-6
    c = N.dense_case("rms", H, eps, rows)
    g = torch.Generator().manual_seed(H)
    qkv = torch.randn(rows, 3 * H, generator=g).to(BF)
    qkv[:, H:2 * H] = c["x"]
    whole, d = fenced(qkv)
    mid = d[:, H:]
    assert mid.data_ptr() == d.data_ptr() + 2 * H and mid.data_ptr() % 16 == 0
    sync(lib.aigv_op_rmsnorm(mid.data_ptr(), 3 * H, ptr(dev(c["w"])), mid.data_ptr(), 3 * H, rows, H, eps, None, None), lib)
    got = d.cpu()
    image = qkv.clone()
    image[:, H:2 * H] = got[:, H:2 * H]
    same_bits(whole, image)                                                           # q, v and the fences: untouched
    accept(c, N.check_dense, N.to_np(got[:, H:2 * H].contiguous()), list(range(rows)), "in place, ld = 3 H")
    out_of_place = launch(lib, c, list(range(rows)))
    assert np.array_equal(N.bits(N.to_np(got[:, H:2 * H].contiguous())), N.bits(out_of_place)), "in place and out of place differ"


@pytest.mark.parametrize("H", [4096, 6144])
def test_lens_tap_against_the_truth(lib, H):
    """raw: the source rows bit for bit; normed: under the RMSNorm rule - directly, not through aigv_op_rmsnorm."""
    c = N.sparse_case("rms", H)
    n = c["x"].shape[0]
    idx = list(range(n - 1, -1, -1))
    idx[3] = idx[2]                                                                    # descending, with a repeat
    src = padded_input(c["x"], H + 24)
    raw_whole, raw = fenced(sentinel_like((n, H), BF))
    normed_whole, normed = fenced(sentinel_like((n, H), BF))
    sync(lib.aigv_op_lens_tap(ptr(src), H + 24, ptr(dev(torch.tensor(idx, dtype=torch.int32))), n, ptr(dev(c["w"])), ptr(raw), ptr(normed), H, c["eps"], None), lib)
    same_bits(raw_whole, c["x"][idx].contiguous())
    accept(c, N.check_sparse, take_output(normed_whole, normed, H), idx, "lens tap")


def _some_accepted_row_quantises_to(c, r, q_row, scale):
    """Is (q_row, scale) what _quant_ref gives for row r of the truth with ONE of its live elements moved by -2 .. +2 bf16 steps?"""
    want = c["want"][r]
    for j in c["cols"][r].tolist():
        for step in (-2, -1, 1, 2):
            row = want.clone()
            row.view(torch.int16)[j] += step                 # live elements are normal numbers far from zero: a step of the bits is a step of the value
            q, s = _quant_ref(row[None])
            if torch.equal(q.view(torch.uint8)[0], q_row) and s.view(torch.int32)[0] == scale.view(torch.int32):
                return True
    return False


@pytest.mark.parametrize("H", [4096, 6144])
def test_rmsnorm_quant_fp8_against_the_truth(lib, H):
    """The bytes and scales of the row quantisation (test_gpu_ops._quant_ref) applied to the truth's bf16 rows.  A row may differ only where the bf16
    row in front of the quantisation may: under the RMSNorm rule that is FLIP_LIMIT of the live elements, each in a row of its own at the worst.  Such
    a row must still be the quantisation of SOME bf16 row the sparse rule accepts: the truth's with one live element moved by at most 2 ulps."""
    c = N.sparse_case("rms", H)
    n, ldq = c["x"].shape[0], H + 16
    want_q, want_s = _quant_ref(c["want"])
    want_q = want_q.view(torch.uint8)
    q_whole, q = fenced(sentinel_like((n, ldq), torch.uint8))
    s_whole, s = fenced(sentinel_like((n,), torch.float32))
    sync(lib.aigv_op_rmsnorm_quant_fp8(ptr(padded_input(c["x"], H + 24)), H + 24, ptr(dev(c["w"])), ptr(q), ldq, ptr(s), n, H, c["eps"], None), lib)
    got_q, got_s = q.cpu(), s.cpu()
    image = sentinel_like((n, ldq), torch.uint8)
    image[:, :H] = got_q[:, :H]
    same_bits(q_whole, image)
    same_bits(s_whole, got_s)                                                          # (the fences; the values are compared below)
    zero_cols = c["x"] == 0
    assert torch.equal(got_q[:, :H][zero_cols], want_q[zero_cols]), "a zero column must quantise to a (signed) zero byte"
    affected = ((got_q[:, :H] != want_q).any(dim=1) | (got_s.view(torch.int32) != want_s.view(torch.int32))).sum().item()
    allowed = int(N.FLIP_LIMIT * int((~zero_cols).sum()))
    print(f"rmsnorm_quant_fp8 H={H}: {affected} of {n} rows differ (allowed {allowed})")
    assert affected <= allowed, (affected, allowed)
    differs = (got_q[:, :H] != want_q).any(dim=1) | (got_s.view(torch.int32) != want_s.view(torch.int32))
    for r in differs.nonzero().flatten().tolist():
        assert _some_accepted_row_quantises_to(c, r, got_q[r, :H], got_s[r]), f"row {r} is the quantisation of no row within 2 ulps of the truth in one element"
    assert torch.isfinite(got_s).all() and (got_s > 0).all()
