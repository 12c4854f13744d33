"""Score-row attention per token without a GPU: the C ABI the dense form adds (header, ctypes prototypes, Python signatures), the host
geometry - prompts.visual_token_positions against a hand-written table, eval_utils.frame_heatmaps on constructed tensors, and the token ->
image-patch map pinned against the oracle's pixel-shuffle - and the conditions under which the dense expectations of the census and the
selector ARE exact, with the per-key tolerance shown to be a derivation (tests/score_attention_tokens_reference.py)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import score_attention_reference as R
import score_attention_tokens_reference as TR
from aigv_assessor_amd import eval_utils, native, prompts
from aigv_assessor_amd.modeling import InternVLChatModel
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_dense_form_header_prototypes_and_signatures():
    header = open(os.path.join(ROOT, "include", "aigv_amd.h")).read()
    assert re.search(r"#define AIGV_ABI_VERSION 3\b", header) and native.ABI_VERSION == 3                  # added symbols only
    version_note = header[header.index("#define AIGV_ABI_VERSION"):header.index("#define AIGV_MAX_CANDIDATES")]
    P, I, I32P = native._P, native._I, native._I32P
    arm, op = native.PROTOTYPES["aigv_score_attention_arm"], native.PROTOTYPES["aigv_op_attention_probe"]
    assert native.PROTOTYPES["aigv_score_attention_arm_tokens"] == (I, arm[1] + [P, I])                   # arm's arguments + tok_out_dev, ld_tok
    assert native.PROTOTYPES["aigv_op_attention_probe_tokens"] == (I, op[1][:-1] + [P, I] + op[1][-1:])   # probe's + tok_out, ld_tok in front of the stream
    lib = native.load()
    for name in ("aigv_score_attention_arm_tokens", "aigv_op_attention_probe_tokens"):
        assert name in version_note, name
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(native.PROTOTYPES[name][1]), name
        assert "float* tok_out" in decl and "int ld_tok" in decl
        assert hasattr(lib, name)
    doc = header[header.index("Score-row attention per KEY"):header.index("int aigv_score_attention_arm_tokens")]
    assert "AIGV_MAX_KV_CAPACITY" in doc and "aigv_decode_step ignores" in doc and "+0.0" in doc
    assert re.search(r"#define AIGV_MAX_KV_CAPACITY 262144\b", header)
    assert re.search(r"#define AIGV_MAX_KV_CAPACITY 262144\b", open(os.path.join(ROOT, "aigv-assessor_amd", "csrc", "kernels.h")).read())


def test_python_surface_takes_the_flag_where_the_issue_says():
    for fn in (InternVLChatModel.forward, InternVLChatModel.forward_shared_prefix):
        assert inspect.signature(fn).parameters["return_token_attention"].default is False
    from aigv_assessor_amd import dist_utils
    for fn in (eval_utils.batched, dist_utils.score_clips_dp, InternVLChatModel.generate):
        assert "return_token_attention" not in inspect.signature(fn).parameters
    assert list(inspect.signature(prompts.visual_token_positions).parameters) == ["slot", "cu", "n_frames", "tokens_per_frame"]
    assert list(inspect.signature(InternVLChatModel.visual_token_positions).parameters) == ["self", "input_ids", "attention_mask", "image_flags", "n_frames"]
    assert list(inspect.signature(eval_utils.frame_heatmaps).parameters) == ["tok_att", "positions", "layers"]
    assert "28r" in eval_utils.frame_heatmaps.__doc__ and "2r" in eval_utils.frame_heatmaps.__doc__       # the pixel rectangle is stated


def test_op_refuses_the_dense_arguments_on_the_host():
    """The dense arguments are refused by aigv_probe_check / fill_rows, on the host, before any pointer is used and before any HIP call - as
    tests/test_score_attention_cpu.py exercises the bin form's refusals.  The operands here are a small HOST buffer: every case below is one
    that the host checks turn down from the integers alone (ld_tok, the row count, a null tok_out); no accepted call is made, and the same
    refusals run against fenced device buffers in tests/test_gpu_score_attention_tokens.py."""
    lib = native.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    p += 16 - p % 16
    cu = native.i32_array([0, 4])

    def call(rows=(3,), tok=p, ld_tok=4):
        return lib.aigv_op_attention_probe_tokens(p, 3 * 128, p, 3 * 128, cu, 1, 1, 1, 3 * 128, 3 * 128, 0, None, 128, p, p, 8, native.i32_array(list(rows)),
                                                  len(rows), p, None, 0, 3, ctypes.cast(p, ctypes.c_void_p), tok, ld_tok, None)

    for kw, word in ((dict(ld_tok=3), "ld_tok is below"), (dict(ld_tok=-1), "ld_tok"), (dict(ld_tok=262145), "AIGV_MAX_KV_CAPACITY"),
                     (dict(tok=None), "null tok_out"), (dict(rows=tuple(range(4)) * 17), "probe rows")):
        rc = call(**kw)
        msg = lib.aigv_last_error(None).decode()
        assert rc == -1 and word in msg and "aigv_op_attention_probe_tokens" in msg, (kw, rc, msg)


# ---- visual_token_positions -------------------------------------------------------------------------------------------------------------
def test_visual_token_positions_match_the_hand_written_table_of_the_appendix_a_prompt():
    slot = TR.appendix_a_clip(2, motion_slot=8)
    got = prompts.visual_token_positions(torch.tensor(slot), [0, len(slot)], 2, 4)
    assert got.dtype == torch.long and tuple(got.shape) == (1, 2, 4) and got[0].tolist() == TR.APPENDIX_A_POSITIONS
    assert prompts.visual_token_positions(slot, [0, len(slot)], [2], 4).tolist() == [TR.APPENDIX_A_POSITIONS]
    # more frames allowed than the clip has: the missing frame is -1
    assert prompts.visual_token_positions(slot, [0, len(slot)], 3, 4)[0].tolist() == TR.APPENDIX_A_POSITIONS + [[-1] * 4]


def test_visual_token_positions_of_ragged_clips_and_their_segment_ids():
    a = TR.appendix_a_clip(2, first_slot=0, motion_slot=12)
    b = TR.appendix_a_clip(1, first_slot=8, motion_slot=13)
    cu = [0, len(a), len(a) + len(b)]
    pos = prompts.visual_token_positions(a + b, cu, [2, 1], 4)
    assert pos.tolist() == [TR.APPENDIX_A_POSITIONS, [TR.APPENDIX_A_POSITIONS[0], [-1] * 4]]             # positions are local to the clip
    seg = prompts.attention_segments(a + b, cu, [2, 1], 4)
    n_checked = 0
    for c in range(2):
        for f in range(2):
            for t in range(4):
                if pos[c, f, t] >= 0:
                    assert int(seg[cu[c] + int(pos[c, f, t])]) == f
                    n_checked += 1
    assert n_checked == 12 and n_checked == int((seg < 2).sum())                                          # every visual token, and no other
    for bad in (dict(n_frames=[2, 2]), dict(n_frames=[2]), dict(n_frames=1), dict(tokens_per_frame=3), dict(cu=[0, 5])):   # attention_segments' validation
        kw = dict(slot=a + b, cu=cu, n_frames=[2, 1], tokens_per_frame=4)
        kw.update(bad)
        with pytest.raises(ValueError, match="visual_token_positions"):
            prompts.visual_token_positions(**kw)


# ---- frame_heatmaps ---------------------------------------------------------------------------------------------------------------------
def heat_case(g=4):
    """Two clips of (2, 1) frames of g * g tokens in the Appendix-A layout; a dense tensor with the sink taking half of every row."""
    tpf = g * g
    a = TR.appendix_a_clip(2, tpf, first_slot=0, motion_slot=3 * tpf)
    b = TR.appendix_a_clip(1, tpf, first_slot=2 * tpf, motion_slot=3 * tpf + 1)
    pos = prompts.visual_token_positions(a + b, [0, len(a), len(a) + len(b)], [2, 1], tpf)
    tok = torch.zeros(2, 3, 2, len(a))
    tok[..., 0] = 0.5
    return tok, pos


def test_frame_heatmaps_puts_planted_mass_in_the_cell_divmod_t_g():
    g = 4
    tok, pos = heat_case(g)
    t = 6                                                               # token 6 of a 4 x 4 frame: row 1, column 2 - a transposed grid would light (2, 1)
    tok[0, :, :, pos[0, 1, t]] = 0.25
    tok[1, 0, :, pos[1, 0, 11]] = 0.4                                   # clip 1: only layer 0 looks at a frame
    heat = eval_utils.frame_heatmaps(tok, pos)
    assert tuple(heat.shape) == (2, 2, g, g) and heat.dtype == tok.dtype
    want = torch.zeros(2, 2, g, g)
    want[0, 1, 1, 2] = 1.0
    want[1, 0, 2, 3] = 1.0                                              # divmod(11, 4); the frame clip 1 does not have stays 0
    assert divmod(t, g) == (1, 2) and torch.equal(heat, want)
    # two cells at 1 : 3, in two frames: renormalised over ALL of the clip's visual tokens
    tok[0, :, :, pos[0, 0, 0]] = 0.75
    heat = eval_utils.frame_heatmaps(tok, pos)
    assert torch.allclose(heat[0, 0, 0, 0], torch.tensor(0.75)) and torch.allclose(heat[0, 1, 1, 2], torch.tensor(0.25))
    assert torch.allclose(heat[0].sum(), torch.tensor(1.0))
    # layers=: clip 1's only mass is in layer 0
    assert torch.equal(eval_utils.frame_heatmaps(tok, pos, layers=[0])[1], want[1])
    assert torch.isnan(eval_utils.frame_heatmaps(tok, pos, layers=[1, 2])[1]).all()        # no visual mass: nothing to renormalise
    assert not torch.isnan(eval_utils.frame_heatmaps(tok, pos, layers=[1, 2])[0]).any()


def test_frame_heatmaps_sums_to_frame_saliency_and_refuses_a_non_square_frame():
    g = 4
    tok, pos = heat_case(g)
    gen = torch.Generator().manual_seed(3)
    tok = torch.rand(tok.shape, generator=gen)
    tok = tok / tok.sum(-1, keepdim=True)
    F = 2
    att = torch.zeros(2, 3, 2, F + prompts.N_TEXT_SEGMENTS, dtype=torch.float64)
    for c in range(2):
        for f in range(F):
            if pos[c, f, 0] >= 0:
                att[c, :, :, f] = tok[c][..., pos[c, f]].double().sum(-1)
    heat = eval_utils.frame_heatmaps(tok, pos)
    assert torch.allclose(heat.double().sum((2, 3)), eval_utils.frame_saliency(att), atol=1e-6)
    assert (heat[1, 1] == 0).all()
    with pytest.raises(ValueError, match="perfect square"):
        eval_utils.frame_heatmaps(tok, pos.view(2, 2, g * g)[..., :8])
    with pytest.raises(ValueError):
        eval_utils.frame_heatmaps(tok[..., :20], pos)                   # positions outside the dense row


# ---- token -> image geometry, pinned against the oracle ------------------------------------------------------------------------------------
def test_token_t_holds_the_patches_2r_2r1_x_2c_2c1_of_the_oracles_pixel_shuffle():
    """What frame_heatmaps' orientation rests on: after pixel-shuffle v2 token t = 16 r + c of a 448^2 frame (32 x 32 patches) is built from
    exactly the patches of rows {2r, 2r + 1} x columns {2c, 2c + 1}."""
    n = 32
    rows = torch.arange(n).view(n, 1).expand(n, n)
    cols = torch.arange(n).view(1, n).expand(n, n)
    x = torch.stack([rows, cols], -1).view(1, n, n, 2).float()          # channel 0: the patch's row, channel 1: its column
    tokens = O.pixel_shuffle_v2(x).reshape(1, -1, 8)                    # [1, 256, 4 patches x (row, col)]
    assert tokens.shape[1] == 256
    g = 16
    for t in range(256):
        r, c = divmod(t, g)
        patches = {(int(a), int(b)) for a, b in tokens[0, t].view(4, 2).tolist()}
        assert patches == {(2 * r + dr, 2 * c + dc) for dr in (0, 1) for dc in (0, 1)}, t
    # the same through the oracle's token path (cls drop, fold, shuffle, flatten)
    vit_out = torch.cat([torch.full((1, 1, 2), -1.0), x.view(1, n * n, 2)], 1)
    assert torch.equal(O.shuffled_tokens(vit_out), tokens)


# ---- the exact constructions, per key ---------------------------------------------------------------------------------------------------
def test_census_per_key_is_one_over_n_in_one_rounding():
    """Q = 0: every e_j is exactly 1, the total exactly n (< 2^24, any order); a key's value is then ONE correctly rounded division 1 / n."""
    for b, r, t in R.probe_rows():
        n = r + 1
        row = TR.census_dense(n, n + TR.EXTRA_LD)
        assert row.dtype == torch.float32 and (row[n:] == 0).all() and (row[n:].view(torch.int32) == 0).all()       # +0.0 bits
        exact = 1.0 / n                                                 # float64: within 2^-53 of the quotient - cannot move the fp32 rounding of 1 / n
        assert row[0].item() == torch.tensor(exact, dtype=torch.float64).float().item() and (row[:n] == row[0]).all()
        assert abs(row[:n].double().sum().item() - 1.0) <= TR.row_sum_bound(n)
    for n in (r + 1 + off for off in R.CACHE_OFF for r in R.LOCALS):
        assert n < 2 ** 24


def test_selector_losers_underflow_to_exactly_zero_per_key():
    """The selected key's e is exp(0) = 1; every other visible key trails by more than EXP_UNDERFLOW, where fp32 exp is exactly 0: the total is
    exactly 1, the selected key 1 / 1 = 1.0, every other key 0 / 1 = +0.0."""
    assert torch.exp(torch.tensor(-R.EXP_UNDERFLOW, dtype=torch.float32)).item() == 0.0
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    assert (one / one).item() == 1.0 and (zero / one).view(torch.int32).item() == 0
    for b, r, sel in R.selector_cases():
        c = R.SelectorCase(3, b, r, sel)
        assert c.margin() >= R.EXP_UNDERFLOW + 16.0
        p = TR.row_truth(c.q_rot.reshape(-1, R.D), c.k[c.cu[b]:c.row + 1])
        assert (p[:, sel] == 1.0).all() and p.sum(-1).max().item() == 1.0          # float64 agrees: nothing else is left


def test_key_bound_is_derived_not_chosen():
    """The per-key tolerance is the count of roundings it names: c = 4 (two exps of 1 ulp) + ceil(n / 256) + 9 + 1, grows with the score bound
    and with n, and is never below one fp32 rounding of the value."""
    p = torch.full((2, 3), 1e-3, dtype=torch.float64)
    zero = torch.zeros(2, dtype=torch.float64)
    assert TR.total_additions(1) == 10 and TR.total_additions(256) == 10 and TR.total_additions(257) == 11 and TR.total_additions(513) == 12
    b0 = TR.key_bound(p, zero, 1) - TR.ABS_FLOOR
    assert (b0 >= p * 15 * TR.U).all() and (b0 <= p * 15.001 * TR.U).all()
    assert torch.allclose(TR.key_bound(p, zero, 513) - TR.key_bound(p, zero, 1), p * 2 * TR.U, rtol=1e-3, atol=0)
    assert (TR.key_bound(p, torch.full((2,), 1e-3, dtype=torch.float64), 1) > b0 + p * 1.9e-3).all()
    assert (TR.key_bound(p, zero, 1, extra_rel=1e-3) > b0 + p * 1.9e-3).all()
    assert TR.ABS_FLOOR < 1e-37 and TR.row_sum_bound(513) == 515 * TR.U and TR.bin_bound(1.0, 513) == 14 * TR.U
    c = R.RandomCase(1)
    q_rot = R.rotate_q(c.q, c.pos, c.cos, c.sin)
    keys = c.k[c.cu[2]:]
    pt = TR.row_truth(q_rot[771].reshape(-1, R.D), keys)
    assert torch.allclose(pt.sum(-1), torch.ones(2, dtype=torch.float64), atol=1e-13)
    # the float64 row folds to the bin reference of score_attention_reference: the two truths are one
    mass, dropped = R.row_truth(q_rot[771].reshape(-1, R.D), keys, c.seg[c.cu[2]:], R.S)
    for s in range(R.S):
        assert torch.allclose(pt[:, c.seg[c.cu[2]:] == s].sum(-1), mass[:, s], atol=1e-13)
    bound = TR.key_bound(pt, R.score_bound(q_rot[771].reshape(-1, R.D), keys), 513)
    assert (bound / pt).max().item() < 2e-3                             # a relative 1e-3 at most: far below anything a heat map shows


def test_one_key_bins_give_chosen_keys_a_bin_each():
    seg, keys = TR.one_key_bins()
    cu = R.cu_of(R.LENS)
    assert [len(k) for k in keys] == [1, 63, 63]
    for b, chosen in enumerate(keys):
        part = seg[cu[b]:cu[b + 1]]
        assert len(set(chosen)) == len(chosen) and [int(part[j]) for j in chosen] == list(range(len(chosen)))
        assert int((part >= 0).sum()) == len(chosen) and int(part.min()) >= -1
    assert {0, 255, 256, 257} <= set(keys[1]) and {0, 255, 256, 512} <= set(keys[2])
