"""The decode-step operators of ABI 3 without a GPU: header, ctypes prototypes and exports, the workspace formula of the split-KV
decode attention, and the host-side argument checks - a refused call returns AIGV_ERR_ARG with a message that names the op, before
anything reaches the device (the device pointers below are never dereferenced: there is no device memory behind them)."""
import ctypes
import os
import re

import pytest

from aigv_assessor_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = native._P, native._I, native._F
NEW = {
    "aigv_op_attention_decode": [P, I, I, P, P, P, I, P, I, I, I, I, I, F, I, P, ctypes.c_int64, P],
    "aigv_op_attention_decode_ws_floats": [I, I, I, I],
    "aigv_op_skinny_rope_kv": [P, I, I, P, I, I, I, P, I, P, P, P, P, P, P, I, I, I, P, F, I, P],
    "aigv_op_skinny_swiglu_normed": [P, I, I, P, I, I, I, P, I, P, F, I, P],
    "aigv_op_skinny_rope_kv_fp8": [P, I, I, P, I, P, I, I, P, I, P, P, P, P, P, P, I, I, I, P, F, I, P],
}
MAX_KV = 262144
FAKE = 1 << 20          # a 16-byte-aligned address with nothing behind it: a call that reached the device would fault or fail with a HIP error


@pytest.fixture(scope="module")
def lib():
    return native.load()


def _refused(lib, rc, op, what):
    msg = lib.aigv_last_error(None).decode()
    assert rc == -1, (rc, msg)                                     # AIGV_ERR_ARG, not AIGV_ERR_HIP
    assert msg.startswith(op + ":") and re.search(what, msg), msg


def test_abi_3_declares_and_exports_the_decode_operators():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3
    assert re.search(rf"#define AIGV_MAX_KV_CAPACITY {MAX_KV}\b", header)
    lib = ctypes.CDLL(native.LIB_PATH)
    assert lib.aigv_abi_version() == 3
    for name, args in NEW.items():
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
        assert native.PROTOTYPES[name][1] == args, name
        getattr(lib, name)
    assert native.PROTOTYPES["aigv_op_attention_decode_ws_floats"][0] is ctypes.c_int64


def test_decode_attention_workspace_formula(lib):
    f = lib.aigv_op_attention_decode_ws_floats
    for n_seq, n_kv, g, cap in [(1, 1, 1, 1), (9, 8, 4, 16512), (3, 2, 7, 20480), (64, 8, 8, MAX_KV)]:
        assert f(n_seq, n_kv, g, cap) == n_seq * n_kv * -(-cap // 128) * g * 130
    for bad in [(0, 1, 1, 128), (1, 0, 1, 128), (1, 1, 0, 128), (1, 1, 9, 128), (1, 1, 1, 0), (1, 1, 1, MAX_KV + 1)]:
        assert f(*bad) == -1, bad


def _attn(lib, **kw):
    a = dict(q=FAKE, ldq=6 * 128 * 2, qgs=6 * 128, kc=FAKE, vc=FAKE, lens=FAKE, cap=4096, o=FAKE, ldo=2 * 4 * 128, n_seq=3, n_kv=2, g=4,
             hd=128, post=128 ** 0.5, max_kv=4000, ws=FAKE, ws_floats=None)
    a.update(kw)
    if a["ws_floats"] is None:
        a["ws_floats"] = max(lib.aigv_op_attention_decode_ws_floats(a["n_seq"], a["n_kv"], max(1, min(a["g"], 8)), max(1, min(a["cap"], MAX_KV))), 0)
    return lib.aigv_op_attention_decode(a["q"], a["ldq"], a["qgs"], a["kc"], a["vc"], a["lens"], a["cap"], a["o"], a["ldo"], a["n_seq"], a["n_kv"],
                                        a["g"], a["hd"], a["post"], a["max_kv"], a["ws"], a["ws_floats"], None)


def test_decode_attention_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_attention_decode"
    _refused(lib, _attn(lib, g=9), op, r"g = 9")
    _refused(lib, _attn(lib, g=0), op, r"g = 0")
    _refused(lib, _attn(lib, hd=64), op, r"head_dim must be 128")
    need = lib.aigv_op_attention_decode_ws_floats(3, 2, 4, 4096)
    _refused(lib, _attn(lib, ws_floats=need - 1), op, rf"workspace of {need - 1} floats, needs {need}")
    _refused(lib, _attn(lib, max_kv=4097), op, r"max_kv_len")
    _refused(lib, _attn(lib, max_kv=0), op, r"max_kv_len")
    _refused(lib, _attn(lib, cap=MAX_KV + 128, max_kv=100), op, rf"<= {MAX_KV}")
    _refused(lib, _attn(lib, ws=None), op, r"null operand")
    _refused(lib, _attn(lib, lens=None), op, r"null operand")
    _refused(lib, _attn(lib, n_seq=0), op, r"n_seq 0")
    _refused(lib, _attn(lib, ldo=2 * 4 * 128 - 1), op, r"strides too small")
    _refused(lib, _attn(lib, qgs=3 * 128), op, r"strides too small")
    _refused(lib, _attn(lib, kc=FAKE + 2), op, r"16-byte aligned")


def _rope_kv(lib, fp8=False, **kw):
    a = dict(x=FAKE, ldx=4096, R=1, W=FAKE, ldw=4096, N=2 * 6 * 128, K=4096, qkv=FAKE, ldo=2 * 6 * 128, pos=FAKE, seq=FAKE, cos=FAKE, sin=FAKE,
             kc=FAKE, vc=FAKE, g=4, n_kv=2, cap=512, norm=FAKE, eps=1e-5, p=1)
    a.update(kw)
    head = (a["x"], a["ldx"], a["R"], a["W"], a["ldw"])
    tail = (a["N"], a["K"], a["qkv"], a["ldo"], a["pos"], a["seq"], a["cos"], a["sin"], a["kc"], a["vc"], a["g"], a["n_kv"], a["cap"], a["norm"],
            a["eps"], a["p"], None)
    if fp8:
        return lib.aigv_op_skinny_rope_kv_fp8(*head, a.get("w_scale", FAKE), *tail)
    return lib.aigv_op_skinny_rope_kv(*head, *tail)


@pytest.mark.parametrize("fp8", [False, True])
def test_rope_kv_gemv_refuses_bad_arguments_on_the_host(lib, fp8):
    op = "aigv_op_skinny_rope_kv_fp8" if fp8 else "aigv_op_skinny_rope_kv"
    _refused(lib, _rope_kv(lib, fp8, R=5), op, r"R <= 4 rows \(got 5\)")                       # more than 4 rows with the fused norm
    _refused(lib, _rope_kv(lib, fp8, K=2048, ldx=2048, ldw=2048), op, r"K = 4096 or 6144 \(got 2048\)")
    _refused(lib, _rope_kv(lib, fp8, K=8192, ldx=8192, ldw=8192), op, r"K = 4096 or 6144 \(got 8192\)")
    _refused(lib, _rope_kv(lib, fp8, g=9, N=2 * 11 * 128, ldo=2 * 11 * 128), op, r"g \(9\)")
    _refused(lib, _rope_kv(lib, fp8, N=2 * 6 * 128 - 128), op, r"N = 1408")
    _refused(lib, _rope_kv(lib, fp8, p=3), op, r"p must be 1, 2 or 4")
    _refused(lib, _rope_kv(lib, fp8, p=4, R=5, norm=None), op, r"R = 5 rows outside 1..4")
    _refused(lib, _rope_kv(lib, fp8, R=0), op, r"R = 0 rows")
    _refused(lib, _rope_kv(lib, fp8, cap=0), op, r"cap = 0")
    _refused(lib, _rope_kv(lib, fp8, kc=None), op, r"null operand")
    _refused(lib, _rope_kv(lib, fp8, ldo=2 * 6 * 128 - 4), op, r"leading dimension")
    if fp8:
        _refused(lib, _rope_kv(lib, fp8, norm=None), op, r"needs norm_w")
        _refused(lib, _rope_kv(lib, fp8, w_scale=None), op, r"w_scale")
    else:
        _refused(lib, _rope_kv(lib, fp8, R=65, norm=None), op, r"R = 65 rows outside 1..64")
        _refused(lib, _rope_kv(lib, fp8, K=200, ldx=256, ldw=256, norm=None), op, r"K = 200")


def test_swiglu_normed_gemv_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_skinny_swiglu_normed"

    def call(x=FAKE, R=2, N=1024, K=4096, ldo=512, norm=FAKE, p=1):
        return lib.aigv_op_skinny_swiglu_normed(x, K, R, FAKE, K, N, K, FAKE, ldo, norm, 1e-5, p, None)
    _refused(lib, call(R=5), op, r"1..4 rows \(got 5\)")
    _refused(lib, call(K=2048), op, r"K = 4096 or 6144 \(got 2048\)")
    _refused(lib, call(norm=None), op, r"norm_w is required")
    _refused(lib, call(N=1000), op, r"N = 1000")
    _refused(lib, call(p=8), op, r"p must be 1, 2 or 4")
    _refused(lib, call(ldo=500), op, r"leading dimension")
