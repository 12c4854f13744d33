"""The GEMM rounding cases without a GPU (tests/gemm_rounding_reference.py): every case tests/test_gpu_gemm_rounding.py runs is exact at every
fp32 add of its chain, ``want`` agrees with round-to-nearest-even restated on exact rationals and with torch's cast, every class sits where
the kernels' code paths meet it, and every wrong rounding chain changes ``want`` in every band of 128 rows and in the last row.  A case that
fails here is a broken CASE: the GPU test would accuse a kernel of the test's own mistake, or let a mistake pass.

The class census and the elements each mutant changes per band are printed per case, whether output is captured or not."""
import numpy as np
import torch

import gemm_exact_reference as GX
import gemm_rounding_reference as GR

BF = torch.bfloat16
TILE, SKINNY, FP8, SKINNY_FP8 = GR.tile_cases(), GR.skinny_cases(), GR.fp8_cases(), GR.skinny_fp8_cases()


def every_case():
    for c in TILE + SKINNY:
        yield c, GR.rounding_case(*c)
    for c in FP8:
        yield c + ("fp8",), GR.fp8_case(*c)
    for c in SKINNY_FP8:
        yield c + ("fp8", "pilot"), GR.fp8_case(*c, pilot=True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_every_case_is_exact_at_every_rounding_point():
    for c, case in every_case():
        bad = {k: v for k, v in GR.exactness(case).items() if v}
        assert not bad, f"{c}: elements that break the exactness bound, by stage: {bad} - the case is broken, not a kernel"
        assert case["want"].shape == (case["M"], GX.n_out(case["N"], case["epi"])) and case["want"].dtype == BF
        # the accumulator read off the slots IS A W^T + bias
        dense = case["A"].double() @ case["W"].double().t()
        if case["bias"] is not None:
            dense = dense + case["bias"].double()
        assert np.array_equal(bits(dense.numpy() + 0.0), bits(GR.linear(case) + 0.0)), c


def test_an_exact_case_has_one_accumulator_in_every_order_of_summation():
    """The point of the bound: fp32 sums over any split of K, in any order, give the float64 accumulator - underflow and overflow columns
    included (partial sums of normal numbers that end as an fp32 subnormal, or just below 2^128)."""
    for epi in (0, 2, 4):
        case = GR.rounding_case(520, 256, 512, epi)
        A, W = case["A"].float(), case["W"].float()
        want = torch.from_numpy(GR.terms(case).sum(0))
        for order in ((0, 1, 2, 3, 4, 5, 6, 7), (7, 3, 5, 1, 6, 2, 4, 0), (4, 5, 6, 7, 0, 1, 2, 3)):
            acc = torch.zeros(520, 256)
            for t in order:                                              # eight slabs of 64, each one summed column by column
                for k in range(64 * t, 64 * t + 64):
                    acc = acc + A[:, k:k + 1] * W[:, k][None, :]
            assert torch.equal(acc.double(), want), (epi, order)
        for S in (2, 4):                                                 # split-K: slabs summed on their own, then added in slice order
            slabs = [sum((A[:, k:k + 1] * W[:, k][None, :] for k in range(s * 512 // S, (s + 1) * 512 // S)), torch.zeros(520, 256)) for s in range(S)]
            assert torch.equal(sum(slabs[1:], slabs[0]).double(), want), (epi, S)


def test_the_terms_of_an_element_land_in_different_k_tiles_and_split_k_slices():
    """The fp8 form too: its four normal terms (the FINE slot included) in four K tiles, both 128-wide slices of aigv_op_gemm_fp8's split-K
    form, and all four waves' K quarters of the weight-streaming e4m3 kernel."""
    bf16_slots, fp8_slots = ((GR.BASE, GR.TAIL, GR.STICKY), (GR.U1, GR.U2), (GR.O1, GR.O2)), ((GR.BASE, GR.TAIL, GR.STICKY, GR.FINE),)
    cases = [(c, GR.rounding_case(*c), bf16_slots) for c in TILE] + [(c, GR.fp8_case(*c), fp8_slots) for c in FP8]
    cases += [(c, GR.fp8_case(*c, pilot=True), fp8_slots) for c in SKINNY_FP8]
    for (M, N, K, epi), case, slot_sets in cases:
        T = K // 64
        for m in range(M):
            for slots in slot_sets:
                cols = [GR.slot_column(m, s, K) for s in slots]
                assert all(c % 8 == s and 0 <= c < K for c, s in zip(cols, slots))
                assert len({c // 64 for c in cols}) == min(len(slots), T), (M, N, K, m, cols)
                for S in (2, 3, 4):
                    if T % S == 0:
                        assert len({c * S // K for c in cols}) == min(len(slots), S), (M, N, K, m, S, cols)
            if case["pilot"]:
                assert GR.pilot_column(m, K) % 8 == GR.U1 and 0 <= GR.pilot_column(m, K) < K
        if M > 8:
            used = np.flatnonzero((case["A"].float().numpy() != 0).any(0))
            assert len({int(k) // 64 for k in used}) == T and len({int(k) % 64 for k in used}) >= 24       # every K tile, many lanes of it


def test_want_is_round_to_nearest_even_on_exact_rationals():
    """Every value that meets a rounding point in any case, rounded by ``round_bf16`` (what ``want`` is made of), by integer arithmetic on
    exact rationals, and by torch's double -> bf16 cast: the three agree bit for bit (signed zeros and Inf included)."""
    seen = 0
    for c, case in every_case():
        epi, y = case["epi"], GR.linear(case)
        points = [y]
        y1 = GR.round_bf16(y)
        with np.errstate(over="ignore", invalid="ignore"):
            if epi == 2:
                points.append(y1 * case["ls"].double().numpy())
                y1 = GR.round_bf16(points[-1])
            if epi in (2, 3):
                points.append(case["resid"].double().numpy() + y1)
            if epi == 5:
                points.append(y1 + case["pos"].double().numpy()[(np.arange(case["M"]) % case["np"]) + 1])
        for p in points:
            u = np.unique(bits(p)).view(np.float64)                     # by bit pattern: -0 and +0 are two values
            mine = GR.round_bf16(u)
            exact = np.array([GR.rne_fraction(float(v)) for v in u])
            cast = torch.from_numpy(u.copy()).to(BF).double().numpy()
            assert np.array_equal(bits(mine), bits(exact)), c
            assert np.array_equal(bits(mine), bits(cast)), c
            seen += len(u)
    assert seen > 10000


def test_want_is_the_chain_of_the_exact_sum_cases_in_torch():
    """``want`` against tests/gemm_exact_reference.py's statement of the same chain (float64, one ``.to(bfloat16)`` per rounding point, torch's
    own bf16 GELU), fed with this module's accumulator."""
    for c, case in every_case():
        y = torch.from_numpy(GR.linear(case))
        real = GX.linear
        GX.linear = lambda _case: y
        try:
            ref = GX.want(case)
        finally:
            GX.linear = real
        assert torch.equal(ref.view(torch.int16), case["want"].view(torch.int16)), c


def test_classes_sit_where_the_kernels_meet_them_and_every_mutant_shows(capsys):
    with capsys.disabled():
        print()
        for c, case in every_case():
            holes = GR.placement_holes(case)
            assert not holes, f"{c}: the case is broken, not a kernel: {holes[:8]}"
            if case["M"] > 8 and "fp8" not in c:
                assert GX.distinguishes_positions(case, case["want"]), c
            cen = GR.census(case)
            for name in GR.required_classes(case):
                assert cen[name] > 0, (c, name)
            counts = GR.mutant_counts(case)
            assert set(counts) == set(GR.mutants_of(case))
            print(f"{c}: " + " ".join(f"{k}={v}" for k, v in cen.items()))
            for name, per_band in counts.items():
                print(f"    {name:<22} changes, per band of 128 rows and in the last row: {per_band}")
                assert min(per_band) > 0, f"{c}: the case is broken, not a kernel: it cannot tell '{name}' from the contract in band {per_band.index(0)}"


def test_the_mutants_apply_where_they_should():
    bf16 = GR.rounding_case(520, 256, 512, 2)
    assert GR.mutants_of(bf16) == list(GR.MUTANTS)
    assert GR.mutants_of(GR.rounding_case(520, 256, 512, 0)) == ["truncate", "round_half_up", "round_half_away", "flush_subnormals", "saturate", "drop_zero_sign"]
    assert GR.mutants_of(GR.rounding_case(520, 256, 512, 4)) == ["truncate", "round_half_up", "round_half_away", "skip_linear_rounding"]
    # the worked examples of the classes
    x = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -12, 1 + 2.0 ** -8 - 2.0 ** -12, 2 - 2.0 ** -7 + 2.0 ** -8,
                  2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -134 + 2.0 ** -140, -2.0 ** -140, 2.0 ** 128 - 2.0 ** 119, 2.0 ** 128 - 2.0 ** 119 - 2.0 ** 111, 0.0])
    want = [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1.0, 2.0, 0.0, 2.0 ** -132, 2.0 ** -133, -0.0, np.inf, GR.BF_MAX, 0.0]
    assert np.array_equal(bits(GR.round_bf16(x)), bits(np.array(want)))
    assert np.array_equal(bits(GR.round_bf16(-x)), bits(-np.array(want)))
    cls, carry = GR.classify(x)
    assert [GR.CLASSES[i] for i in cls] == ["tie_even_down", "tie_even_up", "above_tie", "below_tie", "tie_even_up", "underflow", "underflow",
                                            "underflow", "underflow", "overflow", "overflow", "zero"]
    assert carry.tolist() == [False] * 4 + [True] + [False] * 7


def test_exactness_refuses_a_broken_case():
    case = GR.rounding_case(129, 128, 192, 3)
    assert GR.is_exact(case)
    wide = dict(case, W=case["W"].clone())
    wide["W"][0, GR.STICKY::8] = 2.0 ** -20                                        # a sticky term 2^20 below its base: 21 significant bits
    assert GR.exactness(wide)["accumulator"] > 0
    far = dict(case, resid=case["resid"].clone())
    far["resid"][0, 0] = 2.0 ** 20
    assert GR.exactness(far)["residual add"] > 0
    sub = dict(case, A=case["A"].clone())
    sub["A"][0, GR.slot_column(0, GR.U2, 192)] = 2.0 ** -130                        # a subnormal bf16 operand
    assert GR.exactness(sub)["subnormal operand"] > 0
    gelu = GR.rounding_case(64, 288, 512, 1)
    big = dict(gelu, bias=gelu["bias"].clone())
    big["bias"][:] = 8.0
    assert GR.exactness(big)["gelu argument"] > 0


def test_the_fp8_operands_are_e4m3_numbers_that_reproduce_the_bf16_case():
    for c, case in every_case():
        if "fp8" not in c:
            continue
        ops = case["fp8"]
        assert not GR.fp8_holes(case), (c, GR.fp8_holes(case))
        # what the kernels compute, in float64: (sum of the e4m3 products * row scale) * column scale IS the bf16 case's accumulator
        acc = (ops["A8"].double() @ ops["W8"].double().t()) * ops["row_scale"].double()[:, None] * ops["col_scale"].double()[None, :]
        assert torch.equal(acc, case["A"].double() @ case["W"].double().t()), c
        assert not case["special"] and GR.is_exact(case)
        if case["pilot"]:
            # the kernel's own quantisation, restated: x * (448 / amax) in fp32, cast to e4m3, gives A8; amax / 448 gives the row scale
            x = case["A"].float()
            amax = x.abs().amax(1, keepdim=True)
            assert torch.equal((x * (torch.tensor(448.0) / amax)).to(torch.float8_e4m3fn).view(torch.uint8), ops["A8"].view(torch.uint8)), c
            assert torch.equal((amax / torch.tensor(448.0)).reshape(-1), ops["row_scale"]), c
    bad = dict(GR.fp8_case(*SKINNY_FP8[1], pilot=True))
    bad["A"] = bad["A"].clone()
    bad["A"][0, GR.pilot_column(0, bad["K"])] = 300.0                                # an amax that is no 448 x power of two
    assert GR.fp8_holes(bad)
