"""Op-level tests (MI355X only) of the ViT front end - pixel_shuffle, im2col, cls_rows, frame_ingest and the two resize passes - at the sizes
where they can go wrong and no other op-level test goes: grid-stride loops that wrap (pixel_shuffle's 2048 blocks, frame_ingest's and the
horizontal resize pass' 8192, the vertical passes' 16384), source rows that are no whole number of dwords and start off a dword boundary,
the largest row the horizontal pass stages in LDS, padding shorter and longer than one sweep of a workgroup.

Everything is bit-exact against the oracle's CPU restatement and fenced as in tests/test_gpu_row_ops.py: the whole allocation of every
output is compared with an image that holds a sentinel wherever the kernel must not write."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_ops import BF, dev, lib, sync, _release_device_tensors  # noqa: F401  (the fixtures are used by name)
from test_gpu_row_ops import FENCE, SENTINEL, fenced, ptr, same_bits, sentinel_like

pytestmark = pytest.mark.gpu

MEAN = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
STD = (ctypes.c_float * 3)(0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------------------------------
# pixel shuffle, im2col, cls rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_,grid,Hv", [(8, 32, 1024), (2, 32, 3200), (3, 2, 8)], ids=["loop-wraps", "vit-6b-width", "smallest"])
def test_pixel_shuffle(lib, F_, grid, Hv):
    """(8, 32, 1024) is 1,048,576 16-byte chunks against 2048 blocks x 256 threads: every thread takes two.  The cls rows hold NaN and are dropped."""
    from oracle import oracle as O
    if (F_, grid, Hv) == (8, 32, 1024):
        assert F_ * (grid // 2) ** 2 * (4 * Hv // 8) == 2 * 2048 * 256
    g = torch.Generator().manual_seed(F_ * 1000 + grid + Hv)
    vit = torch.randn(F_, grid * grid + 1, Hv, generator=g).to(BF)
    vit[:, 0] = float("nan")
    want = O.shuffled_tokens(vit)
    assert want.shape == (F_, (grid // 2) ** 2, 4 * Hv) and not torch.isnan(want).any()
    whole, out = fenced(sentinel_like(tuple(want.shape), BF))
    sync(lib.aigv_op_pixel_shuffle(ptr(dev(vit)), grid, Hv, ptr(out), F_, None), lib)
    same_bits(whole, want.contiguous())


@pytest.mark.parametrize("S,P,C,Kp,F_,pad", [(448, 14, 3, 640, 2, "short"), (336, 14, 3, 640, 1, "short"), (64, 16, 3, 768, 2, "none"), (28, 14, 1, 200, 3, "short"),
                                             (28, 14, 3, 1024, 3, "long")], ids=["448-two-frames", "336", "no-padding", "padding-of-4", "padding-longer-than-a-sweep"])
def test_im2col(lib, S, P, C, Kp, F_, pad):
    """Against unfold.  A workgroup sweeps a row 256 columns at a time: no padding columns, fewer than one sweep, and more."""
    K = C * P * P
    assert {"none": Kp == K, "short": 0 < Kp - K < 256, "long": Kp - K > 256}[pad]
    g = torch.Generator().manual_seed(S + P + C + Kp)
    fr = torch.randn(F_, C, S, S, generator=g).to(BF)
    rows = F_ * (S // P) ** 2
    want = torch.zeros(rows, Kp, dtype=BF)                                               # the padding columns must be zero
    want[:, :K] = torch.nn.functional.unfold(fr.float(), P, stride=P).transpose(1, 2).reshape(rows, K).to(BF)
    whole, out = fenced(sentinel_like((rows, Kp), BF))
    sync(lib.aigv_op_im2col(ptr(dev(fr)), F_, C, S, P, Kp, ptr(out), None), lib)
    same_bits(whole, want)


@pytest.mark.parametrize("tpf", [1, 1025])
@pytest.mark.parametrize("H", [8, 1024, 3200], ids=["1-chunk", "128-chunks", "400-chunks"])
def test_cls_rows_chunks_against_threads(lib, H, tpf):
    """128 threads per frame: fewer chunks than threads, exactly as many, and more; frames of one token and of the ViT's 1025.  Every other row keeps its bits."""
    F_ = 3
    g = torch.Generator().manual_seed(H + tpf)
    before = torch.randn(F_ * tpf, H, generator=g).to(BF)
    cls = torch.randn(H, generator=g).to(BF)
    want = before.clone()
    want[::tpf] = cls
    whole, x = fenced(before)
    sync(lib.aigv_op_cls_rows(ptr(dev(cls)), ptr(x), F_, tpf, H, None), lib)
    same_bits(whole, want)


# ---------------------------------------------------------------------------------------------------------
# frame ingest
# ---------------------------------------------------------------------------------------------------------
def _ingest(lib, u, want):
    n, h, w, _ = u.shape
    whole, out = fenced(sentinel_like((n, 3, h, w), BF))
    sync(lib.aigv_op_frame_ingest(ptr(dev(u)), n, h, w, MEAN, STD, ptr(out), None), lib)
    same_bits(whole, want)


def test_frame_ingest_every_byte_value_in_every_channel(lib):
    from oracle import oracle as O
    p = torch.arange(256)
    u = torch.stack([(p * m + o) % 256 for m, o in ((1, 0), (77, 85), (203, 170))], dim=-1).to(torch.uint8).reshape(1, 16, 16, 3)
    for c in range(3):
        assert u[..., c].unique().numel() == 256
    _ingest(lib, u, O.normalize_frames_u8(u))


def test_frame_ingest_of_one_pixel_quad(lib):
    from oracle import oracle as O
    u = torch.tensor([[0, 255, 128], [1, 2, 3], [254, 127, 129], [255, 0, 64]], dtype=torch.uint8).reshape(1, 2, 2, 3)
    _ingest(lib, u, O.normalize_frames_u8(u))


def test_frame_ingest_grid_stride_loop_wraps(lib):
    """48 frames of 448 x 448: 2,408,448 pixel quads against 8192 blocks x 256 threads.  4 distinct frames, each 12 times."""
    from oracle import oracle as O
    assert 48 * 448 * 448 // 4 > 8192 * 256
    g = torch.Generator().manual_seed(48)
    four = torch.randint(0, 256, (4, 448, 448, 3), generator=g, dtype=torch.uint8)
    _ingest(lib, four.repeat(12, 1, 1, 1), O.normalize_frames_u8(four).repeat(12, 1, 1, 1))


# ---------------------------------------------------------------------------------------------------------
# resize + ingest
# ---------------------------------------------------------------------------------------------------------
def _frames(distinct, ih, iw, seed):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (distinct, ih, iw, 3), dtype=np.uint8)
    fr[0, : max(ih // 2, 1)] = np.where(rng.random((max(ih // 2, 1), iw, 3)) < 0.5, 0, 255)          # hard edges in one frame
    return fr


def _resize(lib, distinct, repeat, oh, ow, offset=0):
    """distinct [d, ih, iw, 3] uint8 frames, each `repeat` times in a row of d * repeat frames -> both outputs, fenced, against the oracle (computed once per
    distinct frame).  offset: the frames start that many bytes into their allocation."""
    from oracle import oracle as O
    from oracle.resize import resize_bicubic_u8
    d, ih, iw, _ = distinct.shape
    n = d * repeat
    want_u8 = torch.from_numpy(np.stack([resize_bicubic_u8(distinct[i], oh, ow) for i in range(d)]))
    want_pv = O.normalize_frames_u8(want_u8)
    src = torch.from_numpy(distinct).repeat(repeat, 1, 1, 1).reshape(-1)
    buf = torch.full((offset + src.numel(),), 0x5A, dtype=torch.uint8)
    buf[offset:] = src
    dbuf = dev(buf)
    frames = dbuf[offset:]
    assert frames.data_ptr() % 4 == offset % 4
    tmp_whole, tmp = fenced(sentinel_like((n * ih * ow * 3,), torch.uint8))
    u8_whole, u8 = fenced(sentinel_like((n, oh, ow, 3), torch.uint8))
    pv_whole, pv = fenced(sentinel_like((n, 3, oh, ow), BF))
    sync(lib.aigv_op_frame_resize_ingest(frames.data_ptr(), n, ih, iw, oh, ow, MEAN, STD, ptr(tmp), ptr(u8), ptr(pv), None), lib)
    same_bits(u8_whole, want_u8.repeat(repeat, 1, 1, 1))
    same_bits(pv_whole, want_pv.repeat(repeat, 1, 1, 1))
    t = tmp_whole.cpu()
    assert (t[:FENCE] == SENTINEL[torch.uint8]).all() and (t[-FENCE:] == SENTINEL[torch.uint8]).all(), "written outside the scratch buffer"
    assert torch.equal(dbuf.cpu(), buf), "the source frames were written"


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("iw", [1277, 1278, 1279])
def test_resize_source_rows_that_are_no_whole_dwords(lib, iw, offset):
    """Row pitches of 3831, 3834 and 3837 bytes: the rows start at every residue mod 4, and the last row's staging ends at the last byte of the
    allocation, or one to three bytes short of a dword.  offset 1: row 0 itself starts off a dword boundary."""
    assert (iw * 3) % 4 != 0
    _resize(lib, _frames(2, 7, iw, iw), 1, 5, 448, offset)


def test_resize_widest_row_the_horizontal_pass_stages(lib):
    """in_w = 16384: 49,152 bytes of LDS, the largest the operator accepts."""
    _resize(lib, _frames(1, 3, 16384, 16384), 1, 2, 448)


def test_resize_horizontal_pass_wraps(lib):
    """72 frames of 128 rows: 9216 source rows against 8192 blocks."""
    fr = _frames(4, 128, 16, 72)
    assert 72 * 128 > 8192
    _resize(lib, fr, 18, 64, 64)


@pytest.mark.parametrize("ow", [448, 447], ids=["dword-kernel", "byte-kernel"])
def test_resize_vertical_pass_wraps(lib, ow):
    """28 frames of 32 x 32 -> 448 x 448: 4,214,784 output dwords against 16384 blocks x 256 threads; at out_w = 447 a row is no whole number of
    dwords and the byte kernel runs, 5,607,168 pixels against the same grid."""
    assert 28 * 448 * 448 * 3 // 4 > 16384 * 256 and 28 * 448 * 447 > 16384 * 256 and (447 * 3) % 4 != 0 and (448 * 3) % 4 == 0
    _resize(lib, _frames(4, 32, 32, ow), 7, 448, ow)
