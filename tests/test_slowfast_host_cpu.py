"""Host arithmetic of the SlowFast-R50 branch (csrc/slowfast.hip), without a device: the slow pathway's frame indices, the head pools'
separable weights and the split-K planner - the functions aigv_slowfast_create / aigv_slowfast_finalize call, through the C ABI."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from aigv_assessor_amd import synth


@pytest.fixture(scope="module")
def lib():
    from aigv_assessor_amd import build, native
    build.build()
    return native.load()


@pytest.mark.parametrize("T", list(range(8, 33, 4)))
def test_slow_indices_are_torch_linspace(lib, T):
    idx = (C.c_int32 * 64)(*([-1] * 64))
    n = lib.aigv_slowfast_slow_indices(T, idx)
    assert n == T // 4
    assert list(idx)[:n] == torch.linspace(0, T - 1, T // 4).long().tolist()
    assert all(v == -1 for v in list(idx)[n:])                                   # nothing written past the count


def test_slow_indices_reject_bad_frame_counts(lib):
    idx = (C.c_int32 * 64)()
    assert lib.aigv_slowfast_slow_indices(10, idx) < 0 and lib.aigv_slowfast_slow_indices(0, idx) < 0 and lib.aigv_slowfast_slow_indices(8, None) < 0


def _pool_weights(lib, frames, H, W, window):
    wt, wy, wx = (C.c_float * 32)(), (C.c_float * 32)(), (C.c_float * 32)()
    from aigv_assessor_amd.native import check
    check(lib.aigv_slowfast_pool_weights(frames, H, W, window, wt, wy, wx))
    f = lambda a, n: torch.tensor(list(a)[:n], dtype=torch.float32)
    return f(wt, frames), f(wy, H), f(wx, W)


POOL_CASES = [(fr, 8, h, w) for fr in (2, 3, 8) for h, w in ((7, 7), (8, 7), (7, 32), (32, 32))] + \
             [(fr, 32, h, w) for fr in (8, 12, 32) for h, w in ((7, 7), (8, 7), (7, 32), (32, 32))]


@pytest.mark.parametrize("frames,window,H,W", POOL_CASES)
def test_head_pool_weights_are_the_three_modules(lib, frames, window, H, W):
    """repeat_interleave(4, 2) -> AvgPool3d((window, 7, 7), stride 1) -> AdaptiveAvgPool3d(1) in float64 == the weighted mean with the
    library's separable fp32 weights, to 1e-6 relative to the sum of |w x| (the weights are fp32, three factors of half an ulp each: 1.8e-7);
    each axis sums to 1."""
    wt, wy, wx = _pool_weights(lib, frames, H, W, window)
    for w in (wt, wy, wx):
        assert bool((w > 0).all())
        assert abs(float(w.double().sum()) - 1.0) <= (w.numel() + 1) * 2.0 ** -24       # n fp32 divisions, each half an ulp of a value < 1
    g = torch.Generator().manual_seed(frames * 1000 + H * 32 + W + window)
    x = torch.randn(1, 3, frames, H, W, generator=g, dtype=torch.float64)
    want = F.adaptive_avg_pool3d(F.avg_pool3d(x.repeat_interleave(4, 2), (window, 7, 7), 1), 1).flatten()
    w3 = wt.double()[:, None, None] * wy.double()[None, :, None] * wx.double()[None, None, :]
    got = (x[0] * w3).sum((1, 2, 3))
    mag = (x[0].abs() * w3).sum((1, 2, 3))
    assert bool(((got - want).abs() <= 1e-6 * mag).all()), ((got - want).abs() / mag).max()


def test_head_pool_weights_reject_what_the_kernel_cannot_hold(lib):
    a = (C.c_float * 32)()
    for frames, H, W, window in ((33, 7, 7, 32), (1, 7, 7, 8), (8, 6, 7, 8), (8, 7, 33, 8), (0, 7, 7, 1)):
        assert lib.aigv_slowfast_pool_weights(frames, H, W, window, a, a, a) < 0


def _plan_shapes(T=8, H=224, W=224):
    """(rows per clip, CoutPad, Kp, name) of every convolution of the plan at T x H x W, from synth.slowfast_conv_shapes(): the stems run
    as 4-tap pair convs over 8 channels (K = kt * 7 * 4 * 8), every other conv has K = taps * Cin."""
    out = []
    for conv, _norm, (cout, cin, kt, kh, kw) in synth.slowfast_conv_shapes():
        b = int(conv.split(".")[0])
        fusion = "fusion" in conv
        frames = T if ".multipathway_blocks.1" in conv else T // 4                              # a fusion conv's output has the slow frame count
        K = kt * 7 * 4 * 8 if (b == 0 and not fusion) else kt * kh * kw * cin
        if b == 0:
            div = 4 if fusion else 2                                                            # stem output at 1/2, max-pooled to 1/4
        else:
            div = 4 << (b - 1)                                                                  # res2 at 1/4 ... res5 at 1/32
            if b > 1 and ".res_blocks.0." in conv and conv.endswith("conv_a"):
                div //= 2                                                                       # in front of the block's strided conv_b
        out.append((frames * (H // div) * (W // div), (cout + 15) // 16 * 16, (K + 63) // 64 * 64, conv))
    return out


def test_plan_shapes_helper_names_the_documented_layers():
    """the three examples of the split-K planner's own documentation, so that the grid below provably holds the real plan's shapes"""
    shapes = {name: (rows, cp, kp) for rows, cp, kp, name in _plan_shapes()}
    assert shapes["2.multipathway_blocks.0.res_blocks.1.branch2.conv_b"] == (1568, 128, 1152)
    assert shapes["3.multipathway_blocks.0.res_blocks.1.branch2.conv_b"] == (392, 256, 2304)
    assert shapes["4.multipathway_blocks.0.res_blocks.1.branch2.conv_a"] == (98, 512, 6144)
    assert shapes["0.multipathway_blocks.1.conv"] == (8 * 112 * 112, 16, 1152)
    assert len(shapes) == len(synth.slowfast_conv_shapes())


def test_conv_k_slices_properties(lib):
    ks = lib.aigv_slowfast_conv_k_slices
    grid = [(r, cp, kp) for r in (1, 31, 98, 128, 392, 1568, 6272, 8192, 8193, 25088, 100352) for cp in (16, 32, 48, 64, 80, 128, 512, 2048)
            for kp in (64, 512, 960, 1024, 1088, 1152, 1536, 2304, 4608, 6144, 6208)]
    grid += [(r, cp, kp) for r, cp, kp, _ in _plan_shapes()]
    seen = set()
    for rows, cp, kp in grid:
        S = ks(rows, cp, kp)
        seen.add(S)
        steps = kp // 64
        assert 1 <= S <= 8, (rows, cp, kp, S)
        assert steps % S == 0, (rows, cp, kp, S)
        if S > 1:
            assert steps // S >= 4, (rows, cp, kp, S)
        if rows > 8192 or kp < 1024:
            assert S == 1, (rows, cp, kp, S)
    assert {1, 3, 6, 8} <= seen
    # the documented picks of the real plan at T = 8, 224 x 224
    assert ks(1568, 128, 1152) == 3 and ks(392, 256, 2304) == 6 and ks(98, 512, 6144) == 8
    # ... and res5's shortcut (98 rows, K = 1280: 20 K-steps, which neither 8 nor 6 divides) takes 4
    assert ks(98, 2048, 1280) == 4 and {ks(r, cp, kp) for r, cp, kp, _ in _plan_shapes()} == {1, 3, 4, 6, 8}
    assert ks(0, 64, 1024) < 0 and ks(128, 60, 1024) < 0 and ks(128, 64, 1000) < 0
