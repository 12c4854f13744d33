"""aigv_op_attention_ex and aigv_op_kv_store without a GPU: header, ctypes prototypes and exports, and the host-side argument checks - a
refused call returns AIGV_ERR_ARG with a message that names the op, before anything reaches the device (the device pointers below are
never dereferenced: there is no device memory behind them).  And the references of tests/test_gpu_attention_forms.py themselves: the
acceptance rule there is relative to the eager bf16 path's own error against fp64 truth, so both must be finite and that error a real,
non-zero number for every case."""
import ctypes
import math
import os
import re

import pytest
import torch

from aigv_assessor_amd import native
from attention_reference import BF, CASE_IDS, COUNTS, CONTINUATION_CASES, D, OFFSETS, attn_truth, continuation_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = native._P, native._I, native._F
NEW = {
    "aigv_op_attention_ex": [P, I, P, I, P, I, P, I, P, I, I, I, I, I, I, ctypes.c_int64, P, I, I, F, F, P, P, P, I, I, P],
    "aigv_op_kv_store": [P, I, P, P, P, P, I, I, I, I, I, P],
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


def test_header_bindings_and_library_agree_on_the_two_operators():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3      # added symbols only
    lib = ctypes.CDLL(native.LIB_PATH)
    assert lib.aigv_abi_version() == 3
    for name, args in NEW.items():
        assert re.search(r"\bint " + name + r"\(", header), name
        assert native.PROTOTYPES[name] == (I, args), name
        getattr(lib, name)
    # the header's parameter lists, type by type
    for name, args in NEW.items():
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1)
        kinds = [I if re.match(r"\s*int \w+$", a) else F if re.match(r"\s*float \w+$", a) else ctypes.c_int64 if re.match(r"\s*int64_t \w+$", a) else P
                 for a in decl.split(",")]
        assert kinds == args, (name, decl)


def _ex(lib, **kw):
    """A continuation of 3 sequences, 8 query heads over 2 KV heads, keys in a cache of 2441 rows."""
    g, hk, cap = 4, 2, 2441
    a = dict(q=FAKE, ldq=hk * (g + 2) * D, k=FAKE, ldk=D, v=FAKE, ldv=D, o=FAKE, ldo=hk * g * D, cu=FAKE, n_seq=3, max_len=210, h=hk * g, hk=hk,
             qgs=(g + 2) * D, kvhs=cap * D, kvss=hk * cap * D, kv_off=FAKE, hd=D, causal=5, post=math.sqrt(D), pre=1.0, pos=FAKE, cos=FAKE, sin=FAKE,
             pos_is_row=1, q_tail=0)
    a.update(kw)
    return lib.aigv_op_attention_ex(a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["o"], a["ldo"], a["cu"], a["n_seq"], a["max_len"], a["h"],
                                    a["hk"], a["qgs"], a["kvhs"], a["kvss"], a["kv_off"], a["hd"], a["causal"], a["post"], a["pre"], a["pos"], a["cos"],
                                    a["sin"], a["pos_is_row"], a["q_tail"], None)


def test_attention_ex_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_attention_ex"
    _refused(lib, _ex(lib, q_tail=-1), op, r"q_tail = -1")
    _refused(lib, _ex(lib, kvss=0), op, r"key offset needs K/V in cache layout")                   # kv_off without a cache stride
    _refused(lib, _ex(lib, kvss=-8), op, r"kv_seq_stride = -8")
    _refused(lib, _ex(lib, kvss=2 * 2441 * D + 4), op, r"cache stride")                            # misaligned cache stride
    for operand in ("q", "k", "v", "o", "cu"):
        _refused(lib, _ex(lib, **{operand: None}), op, r"null operand")
    for stride, bad in (("ldq", 6 * D * 2 + 4), ("ldk", D + 4), ("ldv", D - 4), ("ldo", 8 * D + 2), ("qgs", 6 * D + 4), ("kvhs", 2441 * D + 4)):
        _refused(lib, _ex(lib, **{stride: bad}), op, r"strides must keep 16-byte alignment")
    # everything aigv_attn_check refuses
    _refused(lib, _ex(lib, hd=96), op, r"head_dim must be 64 or 128")
    _refused(lib, _ex(lib, n_seq=0), op, r"empty problem")
    _refused(lib, _ex(lib, max_len=0), op, r"empty problem")
    _refused(lib, _ex(lib, h=7), op, r"multiple of n_kv_heads")
    _refused(lib, _ex(lib, hk=0), op, r"multiple of n_kv_heads")
    _refused(lib, _ex(lib, sin=None), op, r"query RoPE needs positions, cos and sin")
    _refused(lib, _ex(lib, pos=None), op, r"query RoPE needs positions, cos and sin")
    _refused(lib, _ex(lib, cos=None, sin=None), op, r"pos_is_row .* needs cos and sin")
    # (accepted forms are launched by the GPU tests; nothing here may reach the device)


def _store(lib, **kw):
    a = dict(qkv=FAKE, ld=2 * 6 * D, seq=FAKE, pos=FAKE, kc=FAKE, vc=FAKE, tokens=100, n_kv=2, g=4, hd=D, cap=2441)
    a.update(kw)
    return lib.aigv_op_kv_store(a["qkv"], a["ld"], a["seq"], a["pos"], a["kc"], a["vc"], a["tokens"], a["n_kv"], a["g"], a["hd"], a["cap"], None)


def test_kv_store_refuses_bad_arguments_on_the_host(lib):
    op = "aigv_op_kv_store"
    for operand in ("qkv", "seq", "pos", "kc", "vc"):
        _refused(lib, _store(lib, **{operand: None}), op, r"null operand")
    _refused(lib, _store(lib, tokens=-1), op, r"tokens = -1")
    _refused(lib, _store(lib, g=0), op, r"g = 0")
    _refused(lib, _store(lib, g=9, ld=2 * 11 * D), op, r"g = 9")
    _refused(lib, _store(lib, n_kv=0), op, r"n_kv = 0")
    _refused(lib, _store(lib, hd=0), op, r"head_dim = 0")
    _refused(lib, _store(lib, hd=100), op, r"head_dim = 100")
    _refused(lib, _store(lib, cap=0), op, r"cap = 0")
    _refused(lib, _store(lib, cap=MAX_KV + 1), op, rf"cap = {MAX_KV + 1} outside 1..{MAX_KV}")
    _refused(lib, _store(lib, ld=2 * 6 * D - 8), op, r"leading dimension")
    _refused(lib, _store(lib, ld=2 * 6 * D + 4), op, r"leading dimension")
    _refused(lib, _store(lib, kc=FAKE + 8), op, r"16-byte aligned")
    _refused(lib, _store(lib, qkv=FAKE + 2), op, r"16-byte aligned")


def test_the_continuation_cases_cover_what_they_must():
    pairs = {(o, n) for _, offs, cnts, _, _, _ in CONTINUATION_CASES for o, n in zip(offs, cnts)}
    assert all((o, n) in pairs for o in OFFSETS for n in COUNTS)
    assert {h // hk for _, _, _, h, hk, _ in CONTINUATION_CASES} >= {1, 3, 4, 6, 8}
    assert any(cap % 64 for *_, cap in CONTINUATION_CASES) and any(cap % 64 == 0 for *_, cap in CONTINUATION_CASES)
    assert any(len(set(offs)) > 1 and len(set(cnts)) > 1 for _, offs, cnts, _, _, _ in CONTINUATION_CASES)
    assert any(o == 2176 and 20 <= n <= 210 for o, n in pairs)                                     # the scoring shape


def test_the_gpu_file_names_only_cases_that_exist():
    import test_gpu_attention_forms as G       # (imports without a GPU: nothing touches the device at import time)
    assert set(G.PREFILL_CASES) | set(G.ROPE_CASES) | {G.TRIM_CASE} <= set(CASE_IDS)
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    offs = {o for n in G.PREFILL_CASES for o in continuation_case(n).offs}
    assert any(o % 32 == 0 and o > 0 for o in offs) and any(o % 32 for o in offs)      # both the bit-equal and the bounded comparison run


def test_the_offset_mask_of_the_truth_is_the_square_mask_cut_at_the_offset():
    """attn_truth(kv_off = o) of the last n rows = the last n rows of the plain causal evaluation of all o + n rows (fp64: same sums)."""
    g = torch.Generator().manual_seed(1)
    o, n = 37, 21
    q, k, v = (torch.randn(o + n, 4, D, generator=g).to(BF), torch.randn(o + n, 2, D, generator=g).to(BF), torch.randn(o + n, 2, D, generator=g).to(BF))
    whole = attn_truth(q, k, v, True, 1.0, math.sqrt(D), torch.float64)
    tail = attn_truth(q[o:], k, v, True, 1.0, math.sqrt(D), torch.float64, kv_off=o)
    assert torch.allclose(whole[o:], tail, rtol=1e-12, atol=1e-14)
    # and row r depends on keys 0 .. o + r only
    k2, v2 = k.clone(), v.clone()
    k2[o + 5:] = 100.0
    v2[o + 5:] = 100.0
    assert torch.equal(attn_truth(q[o: o + 5], k2, v2, True, 1.0, math.sqrt(D), torch.float64, kv_off=o), tail[:5])


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_references_of_every_case_are_finite_and_non_degenerate(name):
    case = continuation_case(name)
    for (truth, eager), o, n in zip(case.references(), case.offs, case.cnts):
        assert truth.shape == eager.shape == (n, case.h, D)
        assert torch.isfinite(truth).all() and torch.isfinite(eager).all()
        e = (eager - truth).abs()
        print(f"{name} off {o} rows {n}: eager error mean {e.mean().item():.3g} max {e.max().item():.3g}; truth mean |o| {truth.abs().mean().item():.3g}")
        # bf16 rounding noise of O(1) outputs: a relative 2^-9 per rounding point on values below ~4 - and never nothing, except for the
        # one-key sequence (offset 0, one row), whose output IS its V row in every evaluation
        assert e.mean().item() < 2e-2 and e.max().item() < 0.25, (name, o, n, e.mean().item(), e.max().item())
        assert e.mean().item() > 1e-5 or o + n == 1, (name, o, n, e.mean().item())
        assert truth.abs().mean().item() > 1e-2, (name, o, n)
