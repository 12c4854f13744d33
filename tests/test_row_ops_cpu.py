"""The test entry points of the score head and the row kernels (ABI 3) without a GPU: header, ctypes prototypes and exports agree, and
every host-side argument check refuses with AIGV_ERR_ARG and a message that starts with the op's name - before anything reaches the
device (the device pointers below are never dereferenced: there is no device memory behind them)."""
import ctypes
import os
import re

import pytest

from aigv_assessor_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = native._P, native._I, native._F
I32P, PP = native._I32P, ctypes.POINTER(native._P)
NEW = {
    "aigv_op_score_head": [P, I, I, I, I32P, PP, PP, P, ctypes.c_int64, P, P],
    "aigv_op_rmsnorm_quant_fp8": [P, I, P, P, I, P, I, I, F, P],
    "aigv_op_rope_slots": [P, I, P, P, P, I, I, I, I, I, I, P],
    "aigv_op_embed": [P, P, P, P, P, I, P, I, I, P],
    "aigv_op_seqpos": [I32P, I, I32P, P, P, P, I, P],
    "aigv_op_gather_rows": [P, I, P, I, P, I, P],
    "aigv_op_scatter_rows": [P, P, I, P, I, I, P],
    "aigv_op_cls_rows": [P, P, I, I, I, P],
    "aigv_op_write_ints": [I32P, I, P, P],
}
FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it: a call that reached the device would fault or fail with a HIP error


@pytest.fixture(scope="module")
def lib():
    return native.load()


def _refused(lib, rc, op, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG, not AIGV_ERR_HIP
    assert msg.startswith(op + ":") and re.search(what, msg), msg


def test_abi_3_declares_and_exports_the_row_operators():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3
    lib = ctypes.CDLL(native.LIB_PATH)
    assert lib.aigv_abi_version() == 3
    for name, args in NEW.items():
        assert re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name][0] is I and native.PROTOTYPES[name][1] == args, name
        getattr(lib, name)


def _score(lib, dims=(4096, 1024, 256, 64, 16, 1), B=2, x=FAKE, ldx=None, scratch=FAKE, scratch_bytes=None, w=FAKE, b=FAKE, score=FAKE, n_layers=None):
    n = len(dims) - 1 if n_layers is None else n_layers
    m = max(n, 1)
    d = native.i32_array(dims)
    wp, bp = (native._P * m)(*[w] * m), (native._P * m)(*[b] * m)
    if scratch_bytes is None:
        scratch_bytes = 3 * max(B, 1) * max(dims) * 2
    return lib.aigv_op_score_head(x, dims[0] if ldx is None else ldx, B, n, d, wp, bp, scratch, scratch_bytes, score, None)


def test_score_head_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_score_head"
    _refused(lib, _score(lib, B=0), op, r"B = 0 outside 1\.\.64")
    _refused(lib, _score(lib, B=65), op, r"B = 65 outside 1\.\.64")
    _refused(lib, _score(lib, n_layers=0), op, r"n_layers = 0 outside 1\.\.8")
    _refused(lib, _score(lib, dims=(128,) * 9 + (1,)), op, r"n_layers = 9 outside 1\.\.8")
    _refused(lib, _score(lib, dims=(4096, 1024, 0, 64, 16, 1)), op, r"dims\[2\] = 0")
    _refused(lib, _score(lib, dims=(4096, -4, 1)), op, r"dims\[1\] = -4")
    need = 3 * 2 * 4096 * 2
    _refused(lib, _score(lib, scratch_bytes=need - 1), op, rf"scratch of {need - 1} bytes, needs {need}")
    _refused(lib, _score(lib, dims=(4096, 1)), op, r"tail dim dims\[0\] = 4096 above 1024")              # the last layer is a tail layer: fan-in above 1024
    _refused(lib, _score(lib, dims=(4096, 2048, 1)), op, r"tail dim dims\[1\] = 2048 above 1024")
    _refused(lib, _score(lib, dims=(256, 2050, 1)), op, r"tail dim dims\[1\] = 2050 above 1024")         # 2050 % 4 != 0: layer 0 would be a tail layer
    _refused(lib, _score(lib, dims=(4096, 1024, 256, 64)), op, r"no tail layer")                         # every layer would run as a GEMM
    _refused(lib, _score(lib, x=None), op, r"null operand")
    _refused(lib, _score(lib, score=None), op, r"null operand")
    _refused(lib, _score(lib, w=None), op, r"null weight or bias of layer 0")
    _refused(lib, _score(lib, ldx=4095), op, r"ldx = 4095 below dims\[0\] = 4096")
    _refused(lib, _score(lib, scratch=FAKE + 8), op, r"16-byte aligned")
    _refused(lib, _score(lib, w=FAKE + 2), op, r"weight of GEMM layer 0")


def test_rmsnorm_quant_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_rmsnorm_quant_fp8"

    def call(x=FAKE, ldx=None, w=FAKE, q=FAKE, ldq=None, scale=FAKE, rows=3, H=4096):
        return lib.aigv_op_rmsnorm_quant_fp8(x, H if ldx is None else ldx, w, q, H if ldq is None else ldq, scale, rows, H, 1e-5, None)
    _refused(lib, call(H=4100), op, r"H = 4100 is not a multiple of 8")
    _refused(lib, call(H=16392), op, r"H = 16392 .* 8\.\.16384")
    _refused(lib, call(H=0), op, r"H = 0")
    _refused(lib, call(ldq=4100), op, r"leading dimension \(ldx 4096, ldq 4100")
    _refused(lib, call(ldq=4088), op, r"leading dimension")
    _refused(lib, call(ldx=4100), op, r"leading dimension")
    _refused(lib, call(rows=-1), op, r"rows = -1")
    _refused(lib, call(scale=None), op, r"null operand")
    _refused(lib, call(x=FAKE + 2), op, r"misaligned")
    _refused(lib, call(q=FAKE + 4), op, r"misaligned")


def test_rope_slots_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_rope_slots"

    def call(qkv=FAKE, ld=2 * 6 * 128, pos=FAKE, cos=FAKE, sin=FAKE, tokens=5, first=4, n_rot=1, slots=6, groups=2, D=128):
        return lib.aigv_op_rope_slots(qkv, ld, pos, cos, sin, tokens, first, n_rot, slots, groups, D, None)
    _refused(lib, call(first=4, n_rot=3), op, r"first_rot \+ n_rot <= slots \(6\)")
    _refused(lib, call(first=6, n_rot=1), op, r"first_rot \(6\)")
    _refused(lib, call(first=-1), op, r"first_rot \(-1\)")
    _refused(lib, call(n_rot=0), op, r"n_rot \(0\)")
    _refused(lib, call(D=120, ld=2 * 6 * 120), op, r"head_dim = 120 is not a positive multiple of 16")
    _refused(lib, call(D=8, ld=2 * 6 * 8), op, r"head_dim = 8")
    _refused(lib, call(ld=2 * 6 * 128 - 8), op, r"leading dimension")
    _refused(lib, call(ld=2 * 6 * 128 + 4), op, r"leading dimension")
    _refused(lib, call(tokens=-1), op, r"tokens = -1")
    _refused(lib, call(pos=None), op, r"null operand")
    _refused(lib, call(cos=FAKE + 2), op, r"16-byte aligned")


def test_embed_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_embed"

    def call(ids=FAKE, slot=FAKE, emb=FAKE, vis=FAKE, motion=FAKE, n_vis=4, out=FAKE, tokens=9, H=4096):
        return lib.aigv_op_embed(ids, slot, emb, vis, motion, n_vis, out, tokens, H, None)
    _refused(lib, call(H=4100), op, r"H = 4100 is not a positive multiple of 8")
    _refused(lib, call(H=0), op, r"H = 0")
    _refused(lib, call(vis=None), op, r"n_vis = 4 needs a visual table")
    _refused(lib, call(n_vis=-1), op, r"n_vis = -1")
    _refused(lib, call(slot=None), op, r"null operand")
    _refused(lib, call(tokens=-2), op, r"tokens = -2")
    _refused(lib, call(out=FAKE + 8), op, r"16-byte aligned")


def test_seqpos_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_seqpos"

    def call(cu, n_seq=None, tokens=None, pos=FAKE, seq=FAKE, cu_dev=FAKE):
        n_seq = len(cu) - 1 if n_seq is None else n_seq
        return lib.aigv_op_seqpos(native.i32_array(cu), n_seq, None, pos, seq, cu_dev, cu[-1] if tokens is None else tokens, None)
    _refused(lib, call(list(range(129))), op, r"n_seq = 128 outside 1\.\.127")
    _refused(lib, call([0, 4], n_seq=0), op, r"n_seq = 0 outside")
    _refused(lib, call([1, 4]), op, r"cu\[0\] = 0")
    _refused(lib, call([0, 4, 9], tokens=8), op, r"cu\[n_seq\] = tokens = 8")
    _refused(lib, call([0, 0], tokens=0), op, r"tokens = 0 >= 1")
    _refused(lib, call([0, 5, 3, 9]), op, r"cu decreases at sequence 1")
    _refused(lib, call([0, 4], pos=None), op, r"null operand")


def test_row_movers_refuse_bad_arguments_on_the_host(lib):
    g, s, c, w = "aigv_op_gather_rows", "aigv_op_scatter_rows", "aigv_op_cls_rows", "aigv_op_write_ints"
    for H, ld, what in [(1028, 1032, r"H = 1028 is not a positive multiple of 8"), (0, 8, r"H = 0"), (1024, 1028, r"leading dimension \(ld 1028"),
                        (1024, 1016, r"leading dimension \(ld 1016")]:
        _refused(lib, lib.aigv_op_gather_rows(FAKE, ld, FAKE, 3, FAKE, H, None), g, what)
        _refused(lib, lib.aigv_op_scatter_rows(FAKE, FAKE, 3, FAKE, ld, H, None), s, what)
    _refused(lib, lib.aigv_op_gather_rows(FAKE, 1024, None, 3, FAKE, 1024, None), g, r"null operand")
    _refused(lib, lib.aigv_op_gather_rows(FAKE, 1024, FAKE, -1, FAKE, 1024, None), g, r"-1 rows")
    _refused(lib, lib.aigv_op_gather_rows(FAKE + 2, 1024, FAKE, 3, FAKE, 1024, None), g, r"16-byte aligned")
    _refused(lib, lib.aigv_op_scatter_rows(FAKE, FAKE, 3, None, 1024, 1024, None), s, r"null operand")
    _refused(lib, lib.aigv_op_scatter_rows(FAKE, FAKE, 3, FAKE + 8, 1024, 1024, None), s, r"16-byte aligned")
    _refused(lib, lib.aigv_op_cls_rows(FAKE, FAKE, 3, 5, 1020, None), c, r"H = 1020 is not a positive multiple of 8")
    _refused(lib, lib.aigv_op_cls_rows(FAKE, FAKE, 3, 0, 1024, None), c, r"tokens_per_frame = 0")
    _refused(lib, lib.aigv_op_cls_rows(None, FAKE, 3, 5, 1024, None), c, r"null operand")
    _refused(lib, lib.aigv_op_cls_rows(FAKE, FAKE, -3, 5, 1024, None), c, r"-3 rows")
    _refused(lib, lib.aigv_op_write_ints(native.i32_array([1, 2]), -1, FAKE, None), w, r"n = -1")
    _refused(lib, lib.aigv_op_write_ints(native.i32_array([1, 2]), 2, None, None), w, r"null operand")
    _refused(lib, lib.aigv_op_write_ints(None, 2, FAKE, None), w, r"null operand")
