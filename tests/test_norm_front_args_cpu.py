"""The test entry points of the normalisation kernels and the ViT front end without a GPU: every host-side argument check refuses with
AIGV_ERR_ARG and a message that starts with the op's name - before anything reaches the device (the device pointers below are never
dereferenced: there is no device memory behind them).  The passes call the launchers directly; these checks guard the tests' own calls."""
import ctypes
import re

import pytest

from aigv_assessor_amd import native

FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it: a call that reached the device would fault or fail with a HIP error
MEAN = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
STD = (ctypes.c_float * 3)(0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def lib():
    return native.load()


def _refused(lib, rc, op, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG, not AIGV_ERR_HIP
    assert msg.startswith(op + ":") and re.search(what, msg), msg


@pytest.mark.parametrize("op", ["aigv_op_layernorm", "aigv_op_rmsnorm"])
def test_norms_refuse_bad_arguments_on_the_host(lib, op):
    ln = op == "aigv_op_layernorm"

    def call(x=FAKE, ldx=None, w=FAKE, b=FAKE, y=FAKE, ldy=None, rows=3, H=4096, idx=None):
        ldx, ldy = H if ldx is None else ldx, H if ldy is None else ldy
        if ln:
            return lib.aigv_op_layernorm(x, ldx, w, b, y, ldy, rows, H, 1e-6, None)
        return lib.aigv_op_rmsnorm(x, ldx, w, y, ldy, rows, H, 1e-6, idx, None)
    _refused(lib, call(x=None), op, r"null operand")
    _refused(lib, call(w=None), op, r"null operand")
    _refused(lib, call(y=None), op, r"null operand")
    if ln:
        _refused(lib, call(b=None), op, r"null operand")
        _refused(lib, call(b=FAKE + 8), op, r"16-byte aligned")
    else:
        _refused(lib, call(idx=FAKE + 2), op, r"row_idx must be 4-byte aligned")
    _refused(lib, call(rows=-1), op, r"rows = -1")
    _refused(lib, call(H=4100), op, r"H = 4100 is not a multiple of 8")
    _refused(lib, call(H=0), op, r"H = 0")
    _refused(lib, call(H=16392), op, r"H = 16392 .* 8\.\.16384")
    _refused(lib, call(ldx=4088), op, r"leading dimension \(ldx 4088, ldy 4096")
    _refused(lib, call(ldx=4100), op, r"leading dimension")
    _refused(lib, call(ldy=4088), op, r"leading dimension \(ldx 4096, ldy 4088")
    _refused(lib, call(ldy=4100), op, r"leading dimension")
    _refused(lib, call(x=FAKE + 2), op, r"16-byte aligned")
    _refused(lib, call(w=FAKE + 8), op, r"16-byte aligned")
    _refused(lib, call(y=FAKE + 4), op, r"16-byte aligned")


def test_pixel_shuffle_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_pixel_shuffle"

    def call(vit=FAKE, grid=32, Hv=1024, out=FAKE, frames=2):
        return lib.aigv_op_pixel_shuffle(vit, grid, Hv, out, frames, None)
    _refused(lib, call(vit=None), op, r"null operand")
    _refused(lib, call(out=None), op, r"null operand")
    _refused(lib, call(frames=-1), op, r"-1 frames")
    _refused(lib, call(grid=31), op, r"grid = 31 is not an even number")
    _refused(lib, call(grid=0), op, r"grid = 0")
    _refused(lib, call(Hv=1028), op, r"vit_hidden = 1028 is not a multiple of 8")
    _refused(lib, call(Hv=0), op, r"vit_hidden = 0")
    _refused(lib, call(Hv=16392), op, r"vit_hidden = 16392 .* 8\.\.16384")
    _refused(lib, call(vit=FAKE + 8), op, r"16-byte aligned")
    _refused(lib, call(out=FAKE + 2), op, r"16-byte aligned")


def test_im2col_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_im2col"

    def call(frames=FAKE, n=2, C=3, S=448, P=14, Kp=640, out=FAKE):
        return lib.aigv_op_im2col(frames, n, C, S, P, Kp, out, None)
    _refused(lib, call(frames=None), op, r"null operand")
    _refused(lib, call(out=None), op, r"null operand")
    _refused(lib, call(n=-2), op, r"-2 frames")
    _refused(lib, call(S=450), op, r"image_size = 450 is not a multiple of patch = 14")
    _refused(lib, call(Kp=587), op, r"kp = 587 below channels \* patch\^2 = 588")
    _refused(lib, call(P=0), op, r"patch \(0\)")
    _refused(lib, call(C=0), op, r"channels \(0\)")
    _refused(lib, call(S=7), op, r"image_size \(7\)")
    _refused(lib, call(frames=FAKE + 2), op, r"16-byte aligned")
    _refused(lib, call(out=FAKE + 8), op, r"16-byte aligned")


def test_frame_ingest_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_frame_ingest"

    def call(src=FAKE, n=2, h=448, w=448, mean=MEAN, std=STD, out=FAKE):
        return lib.aigv_op_frame_ingest(src, n, h, w, mean, std, out, None)
    _refused(lib, call(src=None), op, r"null operand")
    _refused(lib, call(out=None), op, r"null operand")
    _refused(lib, call(mean=None), op, r"null operand")
    _refused(lib, call(std=None), op, r"null operand")
    _refused(lib, call(n=-1), op, r"-1 frames")
    _refused(lib, call(h=3, w=3), op, r"height \* width = 9 is not a multiple of 4")
    _refused(lib, call(h=0), op, r"0 x 448 frames")
    _refused(lib, call(w=16385), op, r"448 x 16385 frames")
    _refused(lib, call(src=FAKE + 1), op, r"4-byte aligned")
    _refused(lib, call(src=FAKE + 2), op, r"4-byte aligned")
    _refused(lib, call(out=FAKE + 4), op, r"8-byte aligned")
    assert call(n=0, src=None, out=None) == 0                       # an empty batch has no buffers: nothing to refuse, nothing launched


def test_frame_resize_refuses_widths_above_16384(lib):
    """The operator's own size check.  It keeps every accepted source row (at most 48 KB) inside what the horizontal pass can stage in LDS, so the
    launcher's refusal of a row that would not fit cannot be reached through any entry point, and is not tested."""
    op = "aigv_op_frame_resize_ingest"
    _refused(lib, lib.aigv_op_frame_resize_ingest(FAKE, 1, 4, 16385, 4, 448, MEAN, STD, FAKE, FAKE, None, None), op, r"sizes above 16384")
