"""The SlowFast-R50 branch (csrc/slowfast.hip) ONE PLANNED OP AT A TIME, through the C ABI's plan walk (aigv_slowfast_plan_op / _run_ops /
_buffer_read / _buffer_write), each op against a float64 CPU reference computed from the input the device really had.

Teacher-forced: an op's reference starts from the bits its input buffer held, so errors do not accumulate and the tolerance is that of ONE
layer - a wrong border tap, a dropped K slice, an off-by-one stride or channel offset shows at the op and the element where it happens
(test_gpu_slowfast.py's end-to-end feature averages such things away).  Tolerances are derived, not measured:

  conv       2^-8 |ref| + K 2^-24 A     one bf16 output rounding + the first-order worst case of fp32 accumulation in any order,
                                        K = taps x Cin, A = the same convolution over |x| and |w|, + |bias| + |residual|
  head pool  2^-8 |ref| + n 2^-24 sum|w x|,  n = T H W
  max-pool, repack                      exact (a maximum / a copy of bf16 values)

PARITY with pytorchvideo itself stays UNPINNED, as in test_gpu_slowfast.py: the references here are torch's own conv3d / pools on the
published architecture's geometry as the plan states it."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 0x4B4B          # bf16 bits of 13303808.0: finite, never the result of an op on O(1) data
BLOCKS = ["block0", "res2", "res3", "res4", "res5", "head"]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16).view(BF)


class Branch:
    """One native handle (a geometry at a clip capacity), its plan, and the frames it is walked on."""

    def __init__(self, T, H, W, clips=1, seed=3):
        from aigv_assessor_amd import native, synth
        from aigv_assessor_amd.slowfast import SlowFastR50
        sd = synth.slowfast_state_dict(seed=seed)
        self.sd = {k[len(synth.SLOWFAST_PREFIX):]: v for k, v in sd.items()}
        self.sf = SlowFastR50(sd)
        self.T, self.H, self.W, self.clips = T, H, W, clips
        self.lib, self.h = self.sf.prepare(torch.device("cuda", torch.cuda.current_device()), clips, T, H, W)
        self.native = native
        self.plan = native.slowfast_plan(self.h)
        self.names = [(op.conv_name.decode() or ["repack", "", "max-pool", "head pool"][op.kind]) for op in self.plan]
        g = torch.Generator().manual_seed(1000 * T + H + clips)
        self.frames = torch.randn(clips * T, 3, H, W, generator=g).clamp(-2.5, 2.5).to(BF)
        self.frames_d = self.frames.cuda()
        self.feature = _sentinel((clips, 2304)).cuda()

    def run(self, first, last, clips=1):
        self.native.check(self.lib.aigv_slowfast_run_ops(self.h, self.frames_d.data_ptr(), clips, self.feature.data_ptr(), first, last, self.native.stream_ptr()))

    def read(self, buf, elems, clips=1):
        out = torch.empty(clips * elems, dtype=BF, device="cuda")
        self.native.check(self.lib.aigv_slowfast_buffer_read(self.h, buf, elems, clips, out.data_ptr(), self.native.stream_ptr()))
        return out.cpu()

    def write(self, buf, t, clips=1):
        d = t.contiguous().cuda()
        assert d.dtype == BF and d.numel() % clips == 0
        self.native.check(self.lib.aigv_slowfast_buffer_write(self.h, buf, d.numel() // clips, clips, d.data_ptr(), self.native.stream_ptr()))
        torch.cuda.synchronize()

    def block_of(self, i):
        op = self.plan[i]
        if op.kind == self.native.SlowFastOp.CONV:
            return int(op.conv_name.decode().split(".")[0])
        return 5 if op.kind == self.native.SlowFastOp.HEADPOOL else 0

    def split_k(self):
        return sorted({op.k_slices for op in self.plan if op.k_slices > 1})


_BRANCHES = {}


@pytest.fixture(scope="module")
def branch():
    """branch(T, H, W, clips): one handle per geometry for the whole module."""
    def get(T, H, W, clips=1):
        key = (T, H, W, clips)
        if key not in _BRANCHES:
            _BRANCHES[key] = Branch(T, H, W, clips)
        return _BRANCHES[key]
    yield get
    _BRANCHES.clear()


# ---- references ------------------------------------------------------------------------------------------------------------------------
def folded_weights(sd, op):
    """The host's BatchNorm fold restated with its operation order (Builder::conv): scale = g / sqrt(var + 1e-5f), w * scale rounded to bf16
    nearest-even, bias = b - mean * scale, every operation an IEEE fp32 one.  Each is computed in float64 and rounded to fp32, which IS the
    correctly rounded fp32 result for + - * / sqrt (53 >= 2 * 24 + 2 bits) on any CPU: torch's own fp32 sqrt is not - on some CPUs its
    vectorised kernel returns a neighbour of the correctly rounded root, the scale moves by an ulp and one weight in ~10^5 lands on the
    other side of a bf16 tie (seen as 95 elements of one output channel of res3's shortcut 4 bf16 ulps off; the library's weight, from
    std::sqrt, was the right one).  Returns float64 [Cout, Cin, kt, kh, kw] and [Cout]."""
    conv, norm = op.conv_name.decode(), op.norm_name.decode()
    w, g, b, mu, var = (sd[conv + ".weight"], sd[norm + ".weight"], sd[norm + ".bias"], sd[norm + ".running_mean"], sd[norm + ".running_var"])
    assert all(t.dtype == torch.float32 for t in (w, g, b, mu, var))
    f32 = lambda t64: t64.float().double()                       # one fp32 rounding
    eps = torch.tensor(1e-5, dtype=torch.float32).double()       # 1e-5f
    scale = f32(g.double() / f32(torch.sqrt(f32(var.double() + eps))))
    return f32(w.double() * scale.view(-1, 1, 1, 1, 1)).to(BF).double(), f32(b.double() - f32(mu.double() * scale))


def conv_reference(sd, op, x_in, res):
    """x_in: the op's input buffer as read (flat bf16), res: its residual buffer or None -> (ref, tol), float64 [rows, Cout]."""
    w, bias = folded_weights(sd, op)
    if op.pair_stem:       # against the ORIGINAL 3-channel [kt, 7, 7] kernel, stride (1, 2, 2), pad (kt / 2, 3, 3), on the three real channels
        x = x_in.view(op.Ti, op.Hi, op.Wi * 2, 4)[..., :3]
        stride, pad = (1, 2, 2), (w.shape[2] // 2, 3, 3)
        assert tuple(w.shape[1:]) == (3, op.kt, 7, 7)
    else:
        x = x_in.view(op.Ti, op.Hi, op.Wi, op.ld_in)[..., :op.Cin]
        stride, pad = (op.st, op.sh, op.sw), (op.pt, op.ph, op.pw)
        assert tuple(w.shape[1:]) == (op.Cin, op.kt, op.kh, op.kw)
    x = x.double().permute(3, 0, 1, 2).unsqueeze(0)
    rows = op.To * op.Ho * op.Wo
    flat = lambda y: y[0].permute(1, 2, 3, 0).reshape(rows, op.Cout)
    ref = flat(F.conv3d(x, w, None, stride, pad)) + bias
    mag = flat(F.conv3d(x.abs(), w.abs(), None, stride, pad)) + bias.abs()
    if res is not None:
        r = res.view(rows, op.ld_res)[:, :op.Cout].double()
        ref, mag = ref + r, mag + r.abs()
    if op.relu:
        ref = ref.relu()
    K = w.shape[1] * w.shape[2] * w.shape[3] * w.shape[4]
    return ref, 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * mag


def _worst(d, tol):
    i = int((d - tol).argmax())
    return f"row {i // d.shape[1]} channel {i % d.shape[1]}: |got - ref| = {float(d.flatten()[i]):.6g} > tol {float(tol.flatten()[i]):.6g}; {int((d > tol).sum())} of {d.numel()} elements over"


# ---- one op ----------------------------------------------------------------------------------------------------------------------------
def conv_window(br, i):
    """Where conv i has to write, from the data flow and NOT from its own c_off: a fusion conv appends to the channels the previous writer
    of its output rows owns (the slow pathway's conv_c, or the max-pool) and fills the row; every other conv starts at channel 0."""
    op, lo = br.plan[i], 0
    if "fusion" in br.names[i]:
        prev = next(br.plan[j] for j in range(i - 1, -1, -1) if br.plan[j].out_buf == op.out_buf)
        lo = prev.Cout if prev.kind == br.native.SlowFastOp.CONV else prev.C
        assert prev.ld_out == op.ld_out == lo + op.Cout, f"op {i} {br.names[i]}: rows of {op.ld_out} channels, {lo} slow + {op.Cout} fused expected"
        reader = next(br.plan[j] for j in range(i + 1, len(br.plan)) if br.plan[j].in_buf == op.out_buf)
        assert reader.Cin == lo + op.Cout, f"op {i} {br.names[i]}: the next block reads {reader.Cin} channels"
    return slice(lo, lo + op.Cout)


def check_conv(br, i):
    op, who = br.plan[i], f"op {i} conv {br.names[i]} (k_slices {br.plan[i].k_slices})"
    rows, own = op.To * op.Ho * op.Wo, conv_window(br, i)
    x_in = br.read(op.in_buf, op.in_elems)
    res = br.read(op.res_buf, op.res_elems) if op.res_buf >= 0 else None
    before = br.read(op.out_buf, op.out_elems).view(rows, op.ld_out).clone()
    before[:, own.stop:] = _sentinel((rows, op.ld_out - own.stop))       # the tail it does not own; the channels in front keep their real data
    br.write(op.out_buf, before)
    br.run(i, i)
    out = br.read(op.out_buf, op.out_elems).view(rows, op.ld_out)
    keep = torch.ones(op.ld_out, dtype=torch.bool)
    keep[own] = False
    assert torch.equal(_bits(out[:, keep]), _bits(before[:, keep])), f"{who}: wrote outside channels [{own.start}, {own.stop}) of its output rows (its c_off is {op.c_off})"
    ref, tol = conv_reference(br.sd, op, x_in, res)
    d = (out[:, own].double() - ref).abs()
    assert bool((d <= tol).all()), f"{who}: {_worst(d, tol)}"
    if op.pair_stem:       # finite junk in the fourth channel: zero weights there (and in the phantom dx = -1 tap) leave every bit alone
        g = torch.Generator().manual_seed(i)
        junk = x_in.view(-1, 4).clone()
        junk[:, 3] = (torch.randn(junk.shape[0], generator=g) * 64).to(BF)
        br.write(op.in_buf, junk)
        br.run(i, i)
        again = br.read(op.out_buf, op.out_elems).view(rows, op.ld_out)
        br.write(op.in_buf, x_in)
        assert torch.equal(_bits(again), _bits(out)), f"{who}: the zero channel of the pair stem's input reaches the output"


def _signed_with_negative_borders(T, H, W, C, seed):
    x = torch.randn(T, H, W, C, generator=torch.Generator().manual_seed(seed))
    for band in (x[:, :2], x[:, -2:], x[:, :, :2], x[:, :, -2:]):
        band.copy_(-band.abs() - 0.01)
    return x.to(BF)


def check_maxpool(br, i):
    op, who = br.plan[i], f"op {i} max-pool of buffer {br.plan[i].in_buf}"
    rows = op.T * op.Ho * op.Wo
    real = br.read(op.in_buf, op.in_elems)
    for name, x in (("signed data, negative borders", _signed_with_negative_borders(op.T, op.H, op.W, op.C, i)), ("the branch's own data", real.view(op.T, op.H, op.W, op.C))):
        br.write(op.in_buf, x)
        before = br.read(op.out_buf, op.out_elems).view(rows, op.ld_out).clone()
        before[:, op.C:] = _sentinel((rows, op.ld_out - op.C))
        br.write(op.out_buf, before)
        br.run(i, i)
        out = br.read(op.out_buf, op.out_elems).view(rows, op.ld_out)
        want = F.max_pool3d(x.float().permute(3, 0, 1, 2).unsqueeze(0), (1, 3, 3), (1, 2, 2), (0, 1, 1))[0].permute(1, 2, 3, 0).reshape(rows, op.C)
        bad = out[:, :op.C].float() != want
        assert not bool(bad.any()), f"{who} on {name}: {int(bad.sum())} elements differ, first at row {int(bad.any(1).float().argmax())}"
        assert torch.equal(_bits(out[:, op.C:]), _bits(before[:, op.C:])), f"{who}: wrote channels [{op.C}, {op.ld_out}) of its output rows"


def check_repack(br, i):
    op = br.plan[i]
    assert (op.T, op.H, op.W, op.To) == (br.T, br.H, br.W, br.T // 4)
    br.write(op.out_buf, _sentinel((op.out_elems,)))
    br.write(op.out2_buf, _sentinel((op.out2_elems,)))
    br.run(i, i)
    fast = br.read(op.out_buf, op.out_elems).view(op.T, op.H, op.W, 4)
    slow = br.read(op.out2_buf, op.out2_elems).view(op.To, op.H, op.W, 4)
    want = br.frames[:op.T].permute(0, 2, 3, 1)
    idx = torch.linspace(0, op.T - 1, op.T // 4).long()
    assert torch.equal(_bits(fast[..., :3]), _bits(want)), f"op {i} repack: fast pathway differs from the frames"
    assert torch.equal(_bits(slow[..., :3]), _bits(want[idx])), f"op {i} repack: slow pathway is not frames {idx.tolist()}"
    assert not bool(_bits(fast[..., 3]).any()) and not bool(_bits(slow[..., 3]).any()), f"op {i} repack: the fourth channel is not zero"


def check_headpool(br, i):
    op, who = br.plan[i], f"op {i} head pool (window {br.plan[i].window}) of buffer {br.plan[i].in_buf}"
    x = (torch.randn(op.T, op.H, op.W, op.C, generator=torch.Generator().manual_seed(i)) * 2).to(BF)
    br.write(op.in_buf, x)
    br.feature.copy_(_sentinel((br.clips, 2304)))
    br.run(i, i)
    got = br.feature.cpu()
    lo = {2048: 0, 256: 2048}[op.C]                               # the feature is cat(slow 2048, fast 256), whatever the op's c_off says
    own = slice(lo, lo + op.C)
    keep = torch.ones(2304, dtype=torch.bool)
    keep[own] = False
    assert bool((_bits(got[:, keep]) == SENTINEL).all()), f"{who}: wrote feature columns outside [{own.start}, {own.stop}) (its c_off is {op.c_off})"
    x5 = x.double().permute(3, 0, 1, 2).unsqueeze(0)
    pools = lambda y: F.adaptive_avg_pool3d(F.avg_pool3d(y.repeat_interleave(4, 2), (op.window, 7, 7), 1), 1).flatten()
    ref, mag = pools(x5), pools(x5.abs())
    d = (got[0, own].double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + op.T * op.H * op.W * 2.0 ** -24 * mag
    assert bool((d <= tol).all()), f"{who}: channel {int((d - tol).argmax())}: |got - ref| = {float(d.max()):.6g}, {int((d > tol).sum())} of {d.numel()} over"


def check_op(br, i):
    K = br.native.SlowFastOp
    {K.REPACK: check_repack, K.CONV: check_conv, K.MAXPOOL: check_maxpool, K.HEADPOOL: check_headpool}[br.plan[i].kind](br, i)


# ---- the walk at T = 8, 224 x 224: every op ---------------------------------------------------------------------------------------------
def test_plan_describes_the_branch(branch):
    """the plan as the walk needs it: the blocks partition it in order (so that the six block cases below cover EVERY op), it holds split-K
    convolutions, and each conv's planned slices are what the host planner answers for its per-clip shape"""
    br = branch(8, 224, 224)
    K = br.native.SlowFastOp
    blocks = [br.block_of(i) for i in range(len(br.plan))]
    assert blocks == sorted(blocks) and set(blocks) == set(range(6)), blocks
    kinds = [op.kind for op in br.plan]
    assert (kinds.count(K.REPACK), kinds.count(K.MAXPOOL), kinds.count(K.HEADPOOL)) == (1, 2, 2)
    from aigv_assessor_amd import synth
    assert sorted(op.conv_name.decode() for op in br.plan if op.kind == K.CONV) == sorted(c for c, _n, _s in synth.slowfast_conv_shapes())
    assert sum(blocks.count(b) for b in range(6)) == len(br.plan) == 5 + len(synth.slowfast_conv_shapes())
    for op in br.plan:
        if op.kind == K.CONV:
            assert op.k_slices == br.lib.aigv_slowfast_conv_k_slices(op.To * op.Ho * op.Wo, (op.Cout + 15) // 16 * 16, op.Kp), op.conv_name
            assert (op.pair_stem == 1) == (op.conv_name.decode() in ("0.multipathway_blocks.0.conv", "0.multipathway_blocks.1.conv"))
    assert len(br.split_k()) > 0 and max(br.split_k()) <= 8, f"split-K slice counts in the plan: {br.split_k()}"
    assert {3, 6, 8} <= set(br.split_k()), f"split-K slice counts in the plan: {br.split_k()}"


@pytest.mark.parametrize("block", range(6), ids=BLOCKS)
def test_walk_every_op_t8(branch, block):
    """T = 8, 224 x 224, one clip: every op of the block against its reference (the ops in front of it run unchecked: the other cases hold
    them).  The case counts what it compared against the plan's ops of its block and fails on a gap."""
    br = branch(8, 224, 224)
    mine = [i for i in range(len(br.plan)) if br.block_of(i) == block]
    assert mine == list(range(mine[0], mine[-1] + 1))
    if mine[0] > 0:
        br.run(0, mine[0] - 1)
    checked, walked_s = 0, set()
    for i in mine:
        try:
            check_op(br, i)
        except AssertionError as e:
            raise AssertionError(f"[{BLOCKS[block]}; split-K slice counts walked so far {sorted(walked_s)} of the plan's {br.split_k()}] {e}") from None
        checked += 1
        if br.plan[i].k_slices > 1:
            walked_s.add(br.plan[i].k_slices)
    assert checked == len(mine) == sum(1 for i in range(len(br.plan)) if br.block_of(i) == block)
    want_s = {br.plan[i].k_slices for i in mine if br.plan[i].k_slices > 1}
    assert walked_s == want_s, (sorted(walked_s), sorted(want_s))


# ---- the other geometries: every op runs, references for the repack, the fusion convs, the split-K convs and the head pools --------------
@pytest.mark.parametrize("T,H,W", [(12, 256, 224), (32, 224, 224)])
def test_walk_subset_other_geometries(branch, T, H, W):
    """T = 12, 256 x 224: non-square with an 8 x 7 final map, three slow frames (0, 5, 11), five temporal windows in the slow head pool.
    T = 32: the upper limit of aigv_slowfast_create - the fast head pool runs over L = 128 repeated frames with window 32, where the host's
    cover table (128 entries) and the kernel's per-frame weights (32 entries) are exactly full."""
    br = branch(T, H, W)
    K = br.native.SlowFastOp
    pools = [op for op in br.plan if op.kind == K.HEADPOOL]
    assert [(p.T, p.H, p.W, p.C, p.window, p.c_off) for p in pools] == [(T // 4, H // 32, W // 32, 2048, 8, 0), (T, H // 32, W // 32, 256, 32, 2048)]
    n = {"repack": 0, "fusion": 0, "split": 0, "head": 0}
    for i, op in enumerate(br.plan):
        fusion = op.kind == K.CONV and "fusion" in br.names[i]
        if op.kind in (K.REPACK, K.HEADPOOL) or fusion or op.k_slices > 1:
            try:
                check_op(br, i)
            except AssertionError as e:
                raise AssertionError(f"[T={T} {H}x{W}; the plan's split-K slice counts {br.split_k()}] {e}") from None
            n["repack" if op.kind == K.REPACK else "head" if op.kind == K.HEADPOOL else "fusion" if fusion else "split"] += 1
        else:
            br.run(i, i)
    assert (n["repack"], n["fusion"], n["head"]) == (1, 4, 2) and n["split"] == sum(1 for op in br.plan if op.k_slices > 1) > 0, n


# ---- batch mates -----------------------------------------------------------------------------------------------------------------------
def test_split_k_bits_do_not_depend_on_batch_mates(branch):
    """S is decided from the per-clip shape: clip 0's output of every split-K conv is the same bits alone and beside another clip."""
    br = branch(8, 224, 224, clips=2)
    assert not torch.equal(br.frames[:8], br.frames[8:])
    split = [i for i, op in enumerate(br.plan) if op.k_slices > 1]
    assert split, "no split-K conv in the plan"

    def outputs(clips):
        outs, at = [], 0
        for i in split:
            br.run(at, i, clips)
            at = i + 1
            op = br.plan[i]
            outs.append(br.read(op.out_buf, op.out_elems, 1).view(-1, op.ld_out)[:, op.c_off:op.c_off + op.Cout].clone())      # clip 0 sits in front
        return outs
    alone, beside = outputs(1), outputs(2)
    for i, a, b in zip(split, alone, beside):
        assert torch.equal(_bits(a), _bits(b)), f"op {i} conv {br.names[i]} (k_slices {br.plan[i].k_slices}): clip 0 differs beside a batch mate"


def test_run_ops_rejects_bad_ranges_and_missing_pointers(branch):
    br = branch(8, 224, 224)
    n = len(br.plan)
    run = lambda frames, feat, first, last, clips=1: br.lib.aigv_slowfast_run_ops(br.h, frames, clips, feat, first, last, None)
    fr, ft = br.frames_d.data_ptr(), br.feature.data_ptr()
    assert run(fr, ft, -1, 0) != 0 and run(fr, ft, 3, 2) != 0 and run(fr, ft, 0, n) != 0 and run(fr, ft, 0, 0, clips=2) != 0
    assert run(None, ft, 0, 0) != 0 and run(fr, None, n - 1, n - 1) != 0          # the repack needs the frames, a head pool the feature
    assert run(None, None, 1, 1) == 0                                            # a conv needs neither
    op = br.plan[1]
    t = torch.empty(op.out_elems + 8, dtype=BF, device="cuda")
    assert br.lib.aigv_slowfast_buffer_read(br.h, 14, 8, 1, t.data_ptr(), None) != 0 and br.lib.aigv_slowfast_buffer_read(br.h, -1, 8, 1, t.data_ptr(), None) != 0
    assert br.lib.aigv_slowfast_buffer_read(br.h, op.out_buf, op.out_elems, 2, t.data_ptr(), None) != 0      # two clips from a one-clip handle
    assert br.lib.aigv_slowfast_buffer_write(br.h, op.out_buf, 1 << 40, 1, t.data_ptr(), None) != 0
    bad = br.native.SlowFastOp()
    assert br.lib.aigv_slowfast_plan_op(br.h, n, C.byref(bad), C.sizeof(bad)) != 0 and br.lib.aigv_slowfast_plan_op(br.h, 0, C.byref(bad), C.sizeof(bad) - 4) != 0
    torch.cuda.synchronize()
