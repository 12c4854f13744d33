"""Score-row attention by segment without a GPU: the segment table (prompts.attention_segments) against a hand-written one, frame_saliency
on a constructed tensor, the float64 reference's own invariants, the C ABI the feature adds (header, ctypes prototypes, limits), and the
conditions under which the two exact constructions of tests/score_attention_reference.py ARE exact (in the style of
tests/test_attention_exact_cpu.py) - so that a bit that differs on the GPU is the kernel's."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import score_attention_reference as R
from aigv_assessor_amd import eval_utils, native, prompts
from aigv_assessor_amd.modeling import InternVLChatModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def appendix_a_clip(n_frames, tpf=4, first_slot=0, motion_slot=0):
    """(slot map, hand-written segment ids for F frame bins given later) of ONE clip in the Appendix-A layout:
    <s> system | 'Frame i: <img>' ctx x tpf '</img>\\n' per frame | 'Motion Feature: <img>' ctx '</img>' | question | answer."""
    slot, kind = [], []

    def text(n, k):
        slot.extend([-1] * n)
        kind.extend([k] * n)

    text(1, "first")
    text(3, "before")                                   # system prompt
    for f in range(n_frames):
        text(2, "before")                               # "Frame f: <img>"
        slot.extend(range(first_slot + f * tpf, first_slot + (f + 1) * tpf))
        kind.extend([f] * tpf)
        text(1, "before" if f < n_frames - 1 else "after")   # "</img>\n": the one behind the LAST visual token is already 'after'
    text(2, "after")                                    # "Motion Feature: <img>"
    slot.append(motion_slot)
    kind.append("motion")
    text(1, "after")                                    # "</img>"
    text(5, "after")                                    # question + answer
    return slot, kind


def ids_of(kind, F):
    names = {"motion": F, "first": F + 1, "before": F + 2, "after": F + 3}
    return [names.get(k, k) for k in kind]


def test_attention_segments_match_the_hand_written_table_of_the_appendix_a_prompt():
    slot, kind = appendix_a_clip(2, motion_slot=8)
    want = [3,  4, 4, 4,  4, 4, 0, 0, 0, 0, 4,  4, 4, 1, 1, 1, 1, 5,  5, 5, 2, 5,  5, 5, 5, 5, 5]       # F = 2: motion 2, first 3, before 4, after 5
    assert ids_of(kind, 2) == want
    got = prompts.attention_segments(torch.tensor(slot), [0, len(slot)], 2, 4)
    assert got.dtype == torch.int32 and got.tolist() == want
    assert prompts.attention_segments(slot, [0, len(slot)], [2], 4).tolist() == want
    # more frame bins than the clip has frames: the ids behind the frames move up, the clip's frames keep theirs
    assert prompts.attention_segments(slot, [0, len(slot)], 3, 4).tolist() == ids_of(kind, 3)


def test_attention_segments_of_ragged_clips_in_one_packed_batch():
    a, ka = appendix_a_clip(2, first_slot=0, motion_slot=12)          # clips of 2 and 1 frames: 12 visual slots, then the two motion slots
    b, kb = appendix_a_clip(1, first_slot=8, motion_slot=13)
    cu = [0, len(a), len(a) + len(b)]
    got = prompts.attention_segments(a + b, cu, [2, 1], 4)
    assert got.tolist() == ids_of(ka, 2) + ids_of(kb, 2)              # F = the largest count: the shorter clip leaves frame bin 1 empty
    assert 1 not in got[cu[1]:].tolist()
    for bad in (dict(n_frames=[2, 2]), dict(n_frames=[2]), dict(n_frames=1), dict(tokens_per_frame=3), dict(cu=[0, 5])):
        kw = dict(slot=a + b, cu=cu, n_frames=[2, 1], tokens_per_frame=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            prompts.attention_segments(**kw)


def test_frame_saliency_on_a_constructed_tensor():
    B, L, H, F = 2, 3, 2, 3
    att = torch.zeros(B, L, H, F + prompts.N_TEXT_SEGMENTS)
    att[..., F + 1] = 0.5                                              # the sink takes half everywhere
    att[0, :, :, 0], att[0, :, :, 2] = 0.1, 0.3                        # clip 0: frames 0 and 2 at 1 : 3
    att[1, 0, :, 1] = 0.4                                              # clip 1: only layer 0 looks at a frame
    s = eval_utils.frame_saliency(att)
    assert s.shape == (B, F) and s.dtype == att.dtype
    assert torch.allclose(s[0], torch.tensor([0.25, 0.0, 0.75])) and torch.allclose(s[1], torch.tensor([0.0, 1.0, 0.0]))
    assert torch.allclose(eval_utils.frame_saliency(att, layers=[0])[1], torch.tensor([0.0, 1.0, 0.0]))
    assert torch.isnan(eval_utils.frame_saliency(att, layers=[1, 2])[1]).all()        # no mass on any frame: nothing to renormalise
    with pytest.raises(ValueError):
        eval_utils.frame_saliency(att[..., :prompts.N_TEXT_SEGMENTS])


def test_float64_reference_sums_to_one_over_bins_plus_dropped_keys():
    c = R.RandomCase(3)
    q_rot = R.rotate_q(c.q, c.pos, c.cos, c.sin)
    seen_dropped = False
    for b, r, t in R.probe_rows():
        keys, seg = c.k[c.cu[b]:c.cu[b] + r + 1], c.seg[c.cu[b]:c.cu[b] + r + 1]
        mass, dropped = R.row_truth(q_rot[t].reshape(-1, R.D), keys, seg, R.S)
        assert mass.shape == (R.N_KV * 3, R.S) and (mass >= 0).all()
        assert torch.allclose(mass.sum(-1) + dropped, torch.ones(R.N_KV * 3, dtype=torch.float64), atol=1e-13)
        seen_dropped |= bool((dropped > 0).any())
    assert seen_dropped                                               # the table does hold ids outside [0, S)
    assert {int(v) for v in c.seg.unique()} == set(range(-1, R.S + 1))


def test_the_op_level_case_covers_the_stride_edges():
    rows = R.probe_rows()
    assert [(b, r) for b, r, _ in rows] == [(0, 0)] + [(1, r) for r in (0, 1, 254, 255, 256, 257)] + [(2, r) for r in R.LOCALS]
    assert [t for _, _, t in rows] == [0, 1, 2, 255, 256, 257, 258, 259, 260, 513, 514, 515, 516, 771]
    assert max(R.LENS) < R.N_POS and max(R.LENS) <= R.CACHE_CAP
    # cache form: every offset leaves the sequence's probe rows behind it or on it, and two sequences differ in theirs
    assert all(off < n for off, n in zip(R.CACHE_OFF, R.LENS)) and len(set(R.CACHE_OFF)) == len(R.CACHE_OFF)


def test_census_is_exact_counts_below_2_pow_24_and_one_division():
    """Q = 0: every score is +-0, the row maximum 0, every exp exactly 1 - a bin is a sum of ones, exact in fp32 in ANY order while it stays
    below 2^24; the result is then ONE correctly rounded division of two exact integers."""
    assert max(R.LENS) < 2 ** 24
    assert torch.exp(torch.zeros(1)).item() == 1.0 and torch.exp(-torch.zeros(1)).item() == 1.0
    ones = torch.ones(max(R.LENS), dtype=torch.float32)
    assert ones.sum().item() == max(R.LENS) and ones.flip(0).cumsum(0)[-1].item() == max(R.LENS)
    exp = R.census_expect()
    seg, cu = R.seg_table(), R.cu_of(R.LENS)
    for b, r, t in R.probe_rows():
        assert exp[t].dtype == torch.float32
        dropped = int(((seg[cu[b]:cu[b] + r + 1] < 0) | (seg[cu[b]:cu[b] + r + 1] >= R.S)).sum())
        assert abs(exp[t].double().sum().item() + dropped / (r + 1) - 1.0) < 1e-6
    assert exp[0].tolist() == [1.0 if s == int(seg[0]) else 0.0 for s in range(R.S)]       # one key: its bin holds everything
    # a rotated zero is zero in the RoPE kernel's arithmetic: the census may run with the real tables
    z = R.rotate_q(torch.zeros(4, 1, 1, R.D, dtype=R.BF), torch.arange(4), *R.rope_table(R.D, 8))
    assert (z == 0).all()


def test_selector_margin_underflows_exp_to_exactly_zero():
    """The selected key leads every other visible key by more than EXP_UNDERFLOW in float64 (with slack for the kernel's fp32 score error),
    and exp of minus that is exactly 0 in fp32: the total is exactly 1, the selected bin exactly 1.0, every other 0.0."""
    assert torch.exp(torch.tensor(-R.EXP_UNDERFLOW, dtype=torch.float32)).item() == 0.0
    assert torch.exp(torch.tensor(-103.0, dtype=torch.float32)).item() > 0.0          # (the bound is not slack by much)
    assert float(torch.tensor(R.SELECT_SCALE).to(R.BF)) == R.SELECT_SCALE
    for g in (1, 4):
        for b, r, sel in R.selector_cases():
            c = R.SelectorCase(g, b, r, sel)
            assert c.margin() >= R.EXP_UNDERFLOW + 16.0, (b, r, sel, c.margin())
            assert torch.equal((c.q_rot.float() * R.SELECT_SCALE).to(R.BF).float(), c.q_rot.float() * R.SELECT_SCALE)     # the scaling is exact
            if c.comp is not None:
                # with q left UNROTATED the competitor (scale * q itself) scores |q|^2 scale / sqrt(D) - at least the selected key's score: the
                # construction tells a skipped rotation from a done one
                k = c.k[c.cu[b]:c.row + 1].double()
                s = torch.einsum("kgd,nkd->kgn", c.q[c.row].double(), k)
                assert (s[..., c.comp] >= s[..., sel]).all() and int(c.seg[c.cu[b] + c.comp]) != int(c.seg[c.cu[b] + sel])
            e = c.expect()
            assert set(e.flatten().tolist()) <= {0.0, 1.0} and (e.sum(-1) <= 1).all()
    assert any(R.SelectorCase(1, b, r, sel).expect().sum() > 0 for b, r, sel in R.selector_cases())


def test_mass_bound_is_derived_not_chosen():
    """The op-level tolerance grows with the score bound eps and with n + S, and is never below one fp32 rounding of the mass."""
    mass = torch.full((2, 3), 0.25, dtype=torch.float64)
    b0 = R.mass_bound(mass, torch.zeros(2, dtype=torch.float64), 1, 3)
    assert (b0 >= mass * 2.0 ** -24).all() and (b0 < 1e-5).all()
    assert (R.mass_bound(mass, torch.full((2,), 1e-3, dtype=torch.float64), 1, 3) > b0 + mass * 1.9e-3).all()
    assert (R.mass_bound(mass, torch.zeros(2, dtype=torch.float64), 513, 3) > b0).all()
    c = R.RandomCase(1)
    q_rot = R.rotate_q(c.q, c.pos, c.cos, c.sin)
    eps = R.score_bound(q_rot[771].reshape(-1, R.D), c.k[c.cu[2]:])
    assert (eps > 0).all() and (eps < 1e-3).all()                  # ~ (D + 2) 2^-24 x 100 / 11: far below anything that matters to a user


def test_abi_of_the_probe_header_prototypes_and_limits():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    kernels = open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read()
    for name, value in (("AIGV_MAX_ATTN_SEGMENTS", 64), ("AIGV_MAX_PROBE_ROWS", 64)):
        assert re.search(rf"#define {name} {value}\b", header) and re.search(rf"#define {name} {value}\b", kernels)
    assert InternVLChatModel.MAX_ATTN_SEGMENTS == 64 and InternVLChatModel.MAX_PROBE_ROWS == 64
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3
    P, I, I32P = native._P, native._I, native._I32P
    assert native.PROTOTYPES["aigv_score_attention_arm"] == (I, [P, I32P, I, P, P, I, I, P])
    assert native.PROTOTYPES["aigv_op_attention_probe"] == (I, [P, I, P, I, I32P, I, I, I, I, I, ctypes.c_int64, I32P, I, P, P, I, I32P, I, P, P, I, I, P, P])
    for name in ("aigv_score_attention_arm", "aigv_op_attention_probe"):
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(native.PROTOTYPES[name][1]), name
    lib = native.load()
    assert hasattr(lib, "aigv_score_attention_arm") and hasattr(lib, "aigv_op_attention_probe")
    # documented: fp32 scores whatever the pass's numerics; decode out of scope
    doc = header[header.index("Score-row attention by segment"):header.index("int aigv_score_attention_arm")]
    assert "ALWAYS fp32" in doc and "aigv_decode_step ignores" in doc


def test_python_surface_takes_the_flag_where_the_issue_says():
    for fn in (InternVLChatModel.forward, InternVLChatModel.forward_shared_prefix):
        assert inspect.signature(fn).parameters["return_score_attention"].default is False
    assert "attention_segments" in inspect.signature(InternVLChatModel.forward).parameters
    from aigv_assessor_amd import dist_utils
    for fn in (eval_utils.batched, dist_utils.score_clips_dp, InternVLChatModel.generate):
        assert "return_score_attention" not in inspect.signature(fn).parameters


def test_op_refuses_bad_arguments_on_the_host():
    """Every refusal of aigv_op_attention_probe happens before any HIP call: it can be exercised without a device."""
    lib = native.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    cu = native.i32_array([0, 4])

    def call(n_seg=3, rows=(3,), head_dim=128, kv_seq_stride=0, kv_off=None, ldk=3 * 128, max_pos=8, n_heads=1, q=p):
        return lib.aigv_op_attention_probe(q, 3 * 128, p, ldk, cu, 1, n_heads, 1, 3 * 128, 3 * 128, kv_seq_stride, kv_off, head_dim, p, p, max_pos,
                                           native.i32_array(list(rows)), len(rows), p, None, 0, n_seg, ctypes.cast(p, ctypes.c_void_p), None)

    for kw, word in ((dict(n_seg=65), "segments"), (dict(n_seg=0), "segments"), (dict(rows=tuple(range(4)) * 17), "probe rows"),
                     (dict(rows=(4,)), "outside the pass"), (dict(rows=(-1,)), "outside the pass"), (dict(head_dim=96), "head_dim"),
                     (dict(kv_off=native.i32_array([2])), "cache layout"), (dict(ldk=3 * 128 + 4), "aligned"), (dict(max_pos=3), "RoPE table"),
                     (dict(n_heads=0), "positive"), (dict(q=None), "null")):
        rc = call(**kw)
        msg = lib.aigv_last_error(None).decode()
        assert rc != 0 and word in msg and "aigv_op_attention_probe" in msg, (kw, rc, msg)
