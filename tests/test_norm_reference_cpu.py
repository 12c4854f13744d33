"""The conditions tests/test_gpu_norm_ops.py rests on, without a GPU: the fp64 truth of tests/norm_reference.py is torch's LayerNorm and the
oracle's RMSNorm, the case generators build what they promise, a faithful float32 evaluation of the kernels' arithmetic passes every
acceptance rule on every committed case - in either order of summation, with rsqrt moved by +-2 fp32 ulps - and every fault of the list
is refused.  The measurements the rules' constants come from are redone here and held to the numbers written in norm_reference.py."""
import numpy as np
import pytest
import torch

import norm_reference as N

F64 = np.float64
SWITCHES = [(o, s) for o in N.ORDERS for s in N.RSTD_SHIFTS]
OPS_H = [("rms", H) for H in N.RMS_H] + [("ln", H) for H in N.LN_H]
EPS_OF = {"rms": N.RMS_EPS, "ln": N.LN_EPS}
SPARSE_H = {"rms": N.RMS_SPARSE_H, "ln": N.LN_SPARSE_H}
FAULTS_OF = {"rms": N.RMS_FAULTS, "ln": N.LN_FAULTS}
# The one-pass variance E[x^2] - mean^2 in float32 at H = 8: a bf16 operand has 8 significant bits, its square 16, the sum of 8 of them at most 19 + the
# spread of their exponents; on every row class here whose values share a binade or two (where alone the subtraction cancels) these sums, the mean
# (11 bits) and its square (22) are exact in fp32, so the one-pass variance IS the two-pass one: test_every_fault... asserts the fault's result equal to the
# faithful one bit for bit there, in place of a refusal.  At every other width the fault is refused in both orders of summation.
VAR_E2_EXACT_AT = 8


def test_bf16_rounding_helpers():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-30, 30, (4096,), generator=g), torch.tensor([0.0, -0.0, 1.00390625, 1.01171875, 3.4e38])])
    want = x.to(N.BF).float().numpy()
    assert np.array_equal(N.bits(N.round_bf16_f32(x.numpy())), N.bits(want))
    assert np.array_equal(N.bits(N.round_bf16_f64(x.double().numpy()).astype(np.float32)), N.bits(want))
    # one rounding, not two: just above the tie 1 + 2^-8 by less than half a float32 ulp - through float32 it would land ON the tie and round to even (down)
    v = 1.0 + 2.0 ** -8 + 2.0 ** -30
    assert np.float32(v) == np.float32(1.0 + 2.0 ** -8) and float(torch.tensor(v, dtype=torch.float64).float().to(N.BF)) == 1.0
    assert N.round_bf16_f64(np.array([v]))[0] == 1.0 + 2.0 ** -7
    assert N.round_bf16_f64(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]           # ties to even
    assert N.round_bf16_f64(np.array([2.0 ** -133 * 0.51, 2.0 ** -133 * 0.5]))[0] == 2.0 ** -133                            # subnormals: steps of 2^-133
    assert N.ulp_bf16(np.array([1.0, 1.99, 0.0, -3.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -133, 2.0 ** -6]
    a = np.array([1.0, -0.0, 1.0, np.inf], dtype=np.float32)
    b = np.array([1.0 + 2.0 ** -6, 0.0, -2.0 ** -133, 1.0], dtype=np.float32)
    assert N.ulp_steps(a, b).tolist() == [2, 0, 0x3F80 + 1, 1 << 16]


@pytest.mark.parametrize("H,eps", [(8, 1e-6), (2304, 1e-5), (4096, 1e-6)])
def test_layernorm_truth_is_torch_in_fp64(H, eps):
    c = N.dense_case("ln", H, eps)
    x, w, b = (c[k].double() for k in ("x", "w", "b"))
    ref = torch.nn.functional.layer_norm(x, (H,), w, b, float(np.float32(eps))).numpy()
    mine = N.ln_terms(N.to_np(c["x"]), N.to_np(c["w"]), eps) + N.to_np(c["b"]).astype(F64)
    scale = np.abs(N.ln_terms(N.to_np(c["x"]), N.to_np(c["w"]), eps)).max(axis=1, keepdims=True) + np.abs(N.to_np(c["b"])).max()
    assert (np.abs(mine - ref) <= 1e-12 * scale).all()
    differ = N.bits(N.round_bf16_f64(ref).astype(np.float32)) != N.bits(N.to_np(c["want"]))
    assert differ.sum() == 0, int(differ.sum())                      # two fp64 evaluations round to one bf16 number (a tie within 1e-12 would show here)


@pytest.mark.parametrize("H,eps", [(8, 1e-5), (3200, 1e-6), (4096, 1e-5)])
def test_rmsnorm_truth_against_the_oracle(H, eps):
    """oracle.rms_norm_cast_then_scale is float32 torch with the same two rounding points: held to the dense rule like a kernel."""
    from oracle import oracle as O
    c = N.dense_case("rms", H, eps)
    got = O.rms_norm_cast_then_scale(c["x"], c["w"], float(np.float32(eps)))
    assert got.dtype == N.BF
    assert N.check_dense(c, N.to_np(got)) is None


@pytest.mark.parametrize("op,H", OPS_H)
def test_dense_cases_hold_every_row_class(op, H):
    c = N.dense_case(op, H, EPS_OF[op][0])
    x, w = c["x"].float(), c["w"].float()
    cls = N.classes_of(op, H)
    assert ("mean250" in cls) == (op == "ln")
    assert x.shape == (N.DENSE_ROWS, H) and ("ones" in cls) == (H & (H - 1) == 0) and len(cls) >= 7 and N.DENSE_ROWS >= 4 * len(cls)
    assert torch.isfinite(x).all() and (w == 0).any() and (w < 0).any() and w[H - 1] == 1.25
    rms = x.double().pow(2).mean(1).sqrt()
    for r in range(N.DENSE_ROWS):
        k = cls[r % len(cls)]
        if k in ("normal3", "tiny9", "tiny20", "huge40") and H >= 128:
            assert 0.7 < rms[r] / (3 * {"normal3": 1.0, "tiny9": 2.0 ** -9, "tiny20": 2.0 ** -20, "huge40": 2.0 ** 40}[k]) < 1.4
        elif k == "mean40":
            assert 35 < x[r].mean() < 45
        elif k == "mean250":
            assert op == "ln" and 245 < x[r].mean() < 255 and (H == 8 or 1 < x[r].double().std() < 3)
        elif k == "outlier":
            assert x[r, H - 1] == 300 and (H == 8 or x[r, :H - 1].abs().max() < 0.5)
        elif k == "zeros":
            assert (x[r] == 0).all()
        elif k == "ones":
            assert (x[r] == 1).all()
    for eps in EPS_OF[op]:                                         # eps carries the statistic of the small rows, and its two values tell apart there
        tiny = [r for r in range(N.DENSE_ROWS) if cls[r % len(cls)] == "tiny20"]
        assert (rms[tiny] ** 2 < 1e-3 * eps).all()
    assert float(x.double().pow(2).sum(1).max()) < 3e38             # the 2^40 rows: no fp32 overflow of the sum of squares
    if "ones" in cls and op == "ln":
        ones = [r for r in range(N.DENSE_ROWS) if cls[r % len(cls)] == "ones"]
        assert torch.equal(c["want"][ones].view(torch.int16), c["b"].expand(len(ones), H).contiguous().view(torch.int16))      # the bias bit for bit


@pytest.mark.parametrize("op,H", [(op, H) for op in ("rms", "ln") for H in SPARSE_H[op]])
def test_sparse_cases_make_every_column_decide_one_row(op, H):
    c = N.sparse_case(op, H)
    n = N.sparse_per_row(H)
    x = c["x"].double()
    assert x.shape == (H // n, H) and n == (16 if H > 6144 else 8)
    nz = x != 0
    assert (nz.sum(1) == n).all() and (nz.sum(0) == 1).all()                                      # a permutation of the columns, dealt n to a row
    assert torch.equal(torch.sort(c["cols"].reshape(-1)).values, torch.arange(H))
    sq = x.pow(2)
    share = torch.where(nz, sq / sq.sum(1, keepdim=True), torch.ones_like(sq))
    assert share.min() >= 1 / 32                                                                  # every non-zero holds at least 1/32 of its row's sum of squares
    mant = x[nz].abs() / torch.exp2(torch.floor(torch.log2(x[nz].abs())))
    assert set(mant.tolist()) == {1.0, 1.25, 1.5, 1.75}
    assert (x.sum(1) == 0).all()                                                                  # the signs cancel: mean exactly 0
    assert (sq.mean(1) > 100 * 1e-5).all()                                                        # eps is below 1 % of the statistic: a lost column is not hidden behind it
    # the sums are exact in float32 in either order, so the fp32 statistics are the truth's up to one division and one rsqrt
    xf = N.to_np(c["x"][:64])
    for order in N.ORDERS:
        assert np.array_equal(N._reduce(xf, True, order, N.threads_of(op, H)).astype(F64), (xf.astype(F64) ** 2).sum(1))
        assert (N._reduce(xf, False, order, N.threads_of(op, H)) == 0).all()
    if op == "ln":                                                                                # LayerNorm of a zero column of a mean-0 row is the bias itself
        want = torch.where(nz, torch.zeros_like(c["want"]), c["want"])
        bias = torch.where(nz, torch.zeros_like(c["want"]), c["b"].expand_as(c["want"]))
        assert torch.equal(want.view(torch.int16), bias.view(torch.int16))


@pytest.mark.parametrize("op,H", OPS_H)
def test_a_faithful_float32_evaluation_passes_every_case_under_every_switch(op, H):
    cases = [(N.dense_case(op, H, eps), N.check_dense) for eps in EPS_OF[op]]
    if H in SPARSE_H[op]:
        cases.append((N.sparse_case(op, H), N.check_sparse))
    for c, rule in cases:
        for order, shift in SWITCHES:
            got = N.fp32_of(c, order=order, rstd_shift=shift)
            why = rule(c, got)
            assert why is None, (op, H, c["eps"], order, shift, why)
            if op == "ln":
                worst = float(N.ln_excess(c, got).max())
                assert worst <= N.MEASURED_LN_A, (H, c["eps"], order, shift, worst)           # MEASURED_LN_A is the worst over all of these


def test_the_layernorm_constant_is_four_times_its_measurement():
    assert N.LN_A == 4 * N.MEASURED_LN_A and 0 < N.LN_A < 2.0 ** -12
    assert N.FLIP_LIMIT == 1e-3


def _refused(c, rule, fault, at, orders=N.ORDERS):
    return [order for order in orders if rule(c, N.fp32_of(c, order=order, fault=fault, at=at)) is not None]


@pytest.mark.parametrize("op,H", OPS_H)
def test_every_fault_is_refused_at_every_width(op, H):
    """By at least one dense case of the width, in BOTH orders of summation (the fault, not the order, is what is refused); the sparse cases
    have a test of their own below.  The lost column and chunk are the LAST ones here - at the outlier's column, where a dense row shows them most
    clearly; that a lost INTERIOR column is refused is shown by the sparse cases, i.e. at their widths only (LayerNorm 1024, 2048, 4096, 12800,
    RMSNorm 4096, 6144, 16384), as the issue scopes them."""
    cases = [(N.dense_case(op, H, eps), N.check_dense) for eps in EPS_OF[op]]
    for fault in FAULTS_OF[op]:
        seen = set()
        for c, rule in cases:
            seen.update(_refused(c, rule, fault, H - 1))
        if fault == "var_e2" and H == VAR_E2_EXACT_AT:
            for c, _ in cases:                    # not a fault at this width: the same bits as the two-pass form (see VAR_E2_EXACT_AT)
                for order in N.ORDERS:
                    assert np.array_equal(N.bits(N.fp32_of(c, order=order, fault=fault)), N.bits(N.fp32_of(c, order=order))), (H, order)
            continue
        assert seen == set(N.ORDERS), (op, H, fault, seen)


@pytest.mark.parametrize("op,H", [(op, H) for op in ("rms", "ln") for H in SPARSE_H[op]])
def test_the_sparse_cases_alone_refuse_a_lost_column_chunk_or_wave(op, H):
    c = N.sparse_case(op, H)
    for fault, places in (("column", (0, H // 2 + 3, H - 1)), ("chunk", (H // 2 + 3,)), ("wave", (H - 1,))):
        for at in places:
            assert _refused(c, N.check_sparse, fault, at, orders=("tree",)) == ["tree"], (op, H, fault, at)
    # ... and the lost column is told by exactly the row it decides: every other row of the result is the truth's
    at = H // 2 + 3
    got = N.fp32_of(c, order="tree", fault="column", at=at)
    differ = (N.bits(got) != N.bits(N.to_np(c["want"]))).sum(1)
    row = int((c["cols"] == at).nonzero()[0, 0])
    assert differ[row] >= 2 and (np.delete(differ, row) <= 1).all()


@pytest.mark.parametrize("H", [1024, 2048, 4096, 12800, 16384])
def test_measured_flip_fractions(H):
    """The measurement FLIP_LIMIT rests on, redone: 256 rows of the dense classes, both eps, every switch.  Prints the fractions."""
    for op in ("rms", "ln"):
        for eps in EPS_OF[op]:
            c = N.dense_case.__wrapped__(op, H, eps, 256)
            want = N.bits(N.to_np(c["want"]))
            for order, shift in SWITCHES:
                frac = float((N.bits(N.fp32_of(c, order=order, rstd_shift=shift)) != want).mean())
                print(f"{op} H={H} eps={eps:g} {order} rstd{shift:+d}: {frac:.3g} not bit-equal")
                assert frac <= N.MEASURED_FLIPS[op, order], (op, H, eps, order, shift, frac)
                if order == "tree" and shift == 0:
                    assert frac <= N.MEASURED_FLIPS_EXACT_RSQRT[op], (op, H, eps, frac)
    assert max(N.MEASURED_FLIPS.values()) < N.FLIP_LIMIT
