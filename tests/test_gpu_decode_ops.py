"""Per-kernel parity tests of the decode step (MI355X only): the split-KV decode attention, the wqkv GEMV with RoPE and the KV-cache
append in its epilogue (bf16 and e4m3 forms) and the w1|w3 GEMV with the RMSNorm fused in front, each called through its ABI 3 entry
point and compared with a plain high-precision reference of the same operation.

Every output, cache and workspace starts out as NaN or sentinel bits, so an unwritten element, a stray write or a read of a key past
a sequence's length shows up.  The RoPE epilogues are checked in two launches of the same GEMV: one with identity tables (cos 1,
sin 0), which hands back the kernel's own bf16(x W^T) - held to the fp32 (fp8: oracle/fp8.py) reference up to summation order -, and
one with real tables, which must equal the reference's three RoPE rounding points applied to those values bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = 128
SENT = 0x7FC1                 # a NaN bit pattern that no kernel writes
MAX_KV = 262144               # AIGV_MAX_KV_CAPACITY


@pytest.fixture(scope="module")
def lib():
    from aigv_assessor_amd import native
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return native.load()


def rb(t):  # one bf16 rounding point
    return t.to(BF).float()


def ulp_check(got, want, frac=0.03, max_ulps=2, atol_rel=2e-5):
    """As tests/test_gpu_ops.py: differences at the 1-2 ulp level (fp32 summation order) on a small fraction of the elements."""
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape
    assert torch.isfinite(got).all()
    ulp = (want.abs().clamp_min(1e-30)).log2().floor().exp2() * 2.0 ** -7
    err = (got - want).abs()
    atol = atol_rel * float(want.abs().max())
    nbad = (err > atol).float().mean().item()
    worst = ((err - atol).clamp_min(0) / ulp).max().item()
    assert worst <= max_ulps + 1e-3, f"worst error {worst:.2f} ulp"
    assert nbad <= frac, f"{nbad:.4f} of elements differ"


def check(rc):
    from aigv_assessor_amd import native
    native.check(rc)
    torch.cuda.synchronize()


def sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int16, device="cuda").view(BF)


def is_sentinel(t):
    return t.contiguous().view(torch.int16) == SENT


# ---------------------------------------------------------------------------------------------------------
# split-KV decode attention
# ---------------------------------------------------------------------------------------------------------
def _caches(ks, vs, cap):
    """[n_seq][n_kv][cap][128] caches holding sequence b's keys / values in rows 0 .. len - 1 and NaN after them."""
    n_kv = ks[0].shape[0]
    kc = torch.full((len(ks), n_kv, cap, D), float("nan"), dtype=BF, device="cuda")
    vc = torch.full_like(kc, float("nan"))
    for b, (k, v) in enumerate(zip(ks, vs)):
        kc[b, :, : k.shape[1]] = k
        vc[b, :, : v.shape[1]] = v
    return kc, vc


def _decode_attention(lib, q, ks, vs, cap, max_kv_len=None):
    """q [n_seq, n_kv, g, 128] placed in fused wqkv rows (K / V slots NaN: the kernel must read the query slots only)."""
    n_seq, n_kv, g, _ = q.shape
    lens = [k.shape[1] for k in ks]
    kc, vc = _caches(ks, vs, cap)
    fused = torch.full((n_seq, n_kv, g + 2, D), float("nan"), dtype=BF, device="cuda")
    fused[:, :, :g] = q
    o = torch.full((n_seq, n_kv * g * D), float("nan"), dtype=BF, device="cuda")
    nws = lib.aigv_op_attention_decode_ws_floats(n_seq, n_kv, g, cap)
    ws = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    dlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    check(lib.aigv_op_attention_decode(fused.data_ptr(), n_kv * (g + 2) * D, (g + 2) * D, kc.data_ptr(), vc.data_ptr(), dlens.data_ptr(), cap,
                                       o.data_ptr(), n_kv * g * D, n_seq, n_kv, g, D, math.sqrt(D), max_kv_len or max(lens), ws.data_ptr(), nws, None))
    return o.view(n_seq, n_kv, g, D)


def _attention_refs(q, k, v):
    """One sequence: q [n_kv, g, 128], k / v [n_kv, L, 128] -> (fp64 truth, the reference's eager bf16 path: scores -> bf16,
    / sqrt(128) -> bf16, fp32 softmax -> bf16, P.V -> bf16; modeling_internlm2.py:407-424)."""
    s = (q.double() @ k.double().transpose(1, 2)) / math.sqrt(D)
    truth = torch.softmax(s, -1) @ v.double()
    sb = (q @ k.transpose(1, 2)) / math.sqrt(D)
    eager = torch.softmax(sb, -1, dtype=torch.float32).to(BF) @ v
    return truth, eager.double()


def _held_to_the_eager_bar(got, q, ks, vs):
    """test_attention_matches_eager_reference's bar with round_scores=True, per sequence and over the launch."""
    near, far = 0.0, 0.0
    for b in range(q.shape[0]):
        truth, eager = _attention_refs(q[b], ks[b], vs[b])
        g = got[b].double()
        assert torch.isfinite(g).all(), f"sequence {b} (length {ks[b].shape[1]}): non-finite output"
        e_hip, e_ref = (g - truth).abs(), (eager - truth).abs()
        assert e_hip.mean() <= 1.5 * e_ref.mean() + 1e-4, (b, ks[b].shape[1], e_hip.mean().item(), e_ref.mean().item())
        assert e_hip.max() <= 2.0 * e_ref.max() + 2e-3, (b, ks[b].shape[1], e_hip.max().item(), e_ref.max().item())
        near += (g - eager).abs().sum().item()
        far += e_ref.sum().item()
    assert near <= 0.75 * far, (near, far)


LENS = [1, 127, 128, 129, 2177, 8191, 8192, 8193, 16384]


def _decode_case(n_kv, g, lens, seed, late_key=None, equal_keys=None):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    q = (torch.randn(len(lens), n_kv, g, D, generator=gen, device="cuda") * 1.5).to(BF)
    ks = [(torch.randn(n_kv, n, D, generator=gen, device="cuda") * 1.5).to(BF) for n in lens]
    vs = [torch.randn(n_kv, n, D, generator=gen, device="cuda").to(BF) for n in lens]
    if late_key is not None:                      # a dominant key in a late chunk: the merge must rescale every earlier chunk
        b, pos = late_key
        ks[b][:, pos] *= 6.0
    if equal_keys is not None:                    # every key of one sequence the same: a uniform softmax over 2177 keys
        ks[equal_keys] = ks[equal_keys][:, :1].expand_as(ks[equal_keys]).contiguous()
    return q, ks, vs


@pytest.mark.parametrize("g,n_kv", [(1, 1), (2, 2), (3, 8), (4, 1), (5, 2), (6, 8), (7, 1), (8, 2), (4, 8)])
def test_decode_attention_matches_fp64_at_ragged_lengths(lib, g, n_kv):
    """Every instantiation (1..8 query heads per KV head) over ragged lengths in one launch - chunk boundaries, the 64-chunk loops
    of the merge pass (8192 / 8193 / 16384 keys) - with max_kv_len < cap, a late dominant key and an all-equal-keys sequence."""
    q, ks, vs = _decode_case(n_kv, g, LENS, seed=100 * g + n_kv, late_key=(8, 15000), equal_keys=4)
    got = _decode_attention(lib, q, ks, vs, cap=16384 + 128)
    _held_to_the_eager_bar(got, q, ks, vs)


def test_decode_attention_bits_do_not_depend_on_batch_mates_or_capacity(lib):
    """A sequence's output has the same bits alone (n_seq = 1, max_kv_len = its own length, two capacities) as in the ragged batch,
    and the whole batch has the same bits at two capacities."""
    g, n_kv = 4, 2
    q, ks, vs = _decode_case(n_kv, g, LENS, seed=7, late_key=(7, 8000))
    batch = _decode_attention(lib, q, ks, vs, cap=16384 + 128)
    assert torch.equal(batch, _decode_attention(lib, q, ks, vs, cap=16384 + 3 * 128 + 5))
    for b in (0, 3, 7, 8):
        n = LENS[b]
        for cap in (n, n + 1000):
            alone = _decode_attention(lib, q[b: b + 1], ks[b: b + 1], vs[b: b + 1], cap=cap, max_kv_len=n)
            assert torch.equal(alone[0], batch[b]), (n, cap)


def test_decode_attention_past_16k_cached_tokens(lib):
    """A capacity above 16 384 tokens (more than 128 chunks: the merge pass once held a fixed 128 in LDS and the launch was refused with
    'invalid argument'), a sequence of 20 000 keys with its dominant key near the end, at the same fp64 bar."""
    g, n_kv = 4, 2
    q, ks, vs = _decode_case(n_kv, g, [20000, 1, 16385, 300], seed=11, late_key=(0, 19500))
    got = _decode_attention(lib, q, ks, vs, cap=20480)
    _held_to_the_eager_bar(got, q, ks, vs)


# ---------------------------------------------------------------------------------------------------------
# wqkv GEMV with RoPE + KV-cache append (bf16 and e4m3), w1|w3 GEMV with the fused RMSNorm
# ---------------------------------------------------------------------------------------------------------
def _rope_ref(y, pos, cos, sin):
    """The reference's rotary embedding on bf16 slot vectors y [R, ..., 128] at positions pos [R]: three bf16 roundings
    (modeling_internlm2.py:247-261), as test_rope_matches_reference_rounding."""
    shape = [y.shape[0]] + [1] * (y.dim() - 2) + [D]
    c = torch.cat([cos, cos], -1)[pos.long()].view(shape)
    s = torch.cat([sin, sin], -1)[pos.long()].view(shape)
    rot = torch.cat((-y[..., D // 2:], y[..., : D // 2]), dim=-1)
    return (y * c) + (rot * s)


def _rows(R, n_seq, cap):
    """Per row its cache sequence and position: different slots and positions for every row."""
    seq = torch.arange(R) % n_seq
    pos = (111 * torch.arange(R) + 5) % cap          # 111 is odd: distinct positions among the rows of one sequence (cap = 512)
    return seq.to(torch.int32), pos.to(torch.int32)


def _launch_rope_kv(lib, x, W, g, n_kv, seq, pos, cos, sin, cap, n_seq, p, norm_w=None, eps=1e-5, fp8_scale=None):
    """One launch on sentinel-filled outputs: -> (qkv [R + 1, N] (the last row must stay untouched), kc, vc)."""
    R, K = x.shape
    N = n_kv * (g + 2) * D
    qkv = sentinel(R + 1, N)
    kc, vc = sentinel(n_seq, n_kv, cap, D), sentinel(n_seq, n_kv, cap, D)
    dseq, dpos = seq.cuda(), pos.cuda()
    args = (qkv.data_ptr(), N, dpos.data_ptr(), dseq.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), g, n_kv, cap,
            norm_w.data_ptr() if norm_w is not None else None, eps, p, None)
    if fp8_scale is None:
        check(lib.aigv_op_skinny_rope_kv(x.data_ptr(), K, R, W.data_ptr(), K, N, K, *args))
    else:
        check(lib.aigv_op_skinny_rope_kv_fp8(x.data_ptr(), K, R, W.data_ptr(), K, fp8_scale.data_ptr(), N, K, *args))
    return qkv, kc, vc


def _gathered(qkv, kc, vc, seq, pos, g, n_kv):
    """[R, n_kv, g + 2, 128]: the query slots from the qkv rows, K and V from the cache rows the epilogue appended."""
    R = seq.shape[0]
    out = qkv[:R].view(R, n_kv, g + 2, D).clone()
    s, p = seq.long().cuda(), pos.long().cuda()
    out[:, :, g] = kc[s, :, p]
    out[:, :, g + 1] = vc[s, :, p]
    return out


def _check_untouched(qkv, kc, vc, seq, pos, g, n_kv):
    R = seq.shape[0]
    assert is_sentinel(qkv[R]).all(), "a row past R was written"
    assert is_sentinel(qkv[:R].view(R, n_kv, g + 2, D)[:, :, g:]).all(), "the K / V columns of the qkv rows were written"
    written = torch.zeros(kc.shape[:3], dtype=torch.bool, device="cuda")
    written[seq.long().cuda(), :, pos.long().cuda()] = True
    for c in (kc, vc):
        assert is_sentinel(c[~written]).all(), "a cache element outside the appended rows changed"


def _rope_kv_case(lib, x, W, g, n_kv, p, want_y, n_seq=3, cap=512, fp8_scale=None, norm_w=None, ulps=None):
    """The identity-table launch must give want_y up to summation order, the real-table launch RoPE of those very values."""
    from aigv_assessor_amd.modeling import rope_tables
    R = x.shape[0]
    seq, pos = _rows(R, n_seq, cap)
    cos, sin = (t.cuda() for t in rope_tables(D, 1e6, cap))
    one, zero = torch.ones_like(cos), torch.zeros_like(sin)
    runs = []
    for c, s in ((one, zero), (cos, sin)):
        qkv, kc, vc = _launch_rope_kv(lib, x, W, g, n_kv, seq, pos, c, s, cap, n_seq, p, norm_w=norm_w, fp8_scale=fp8_scale)
        _check_untouched(qkv, kc, vc, seq, pos, g, n_kv)
        runs.append((qkv, kc, vc))
    y = _gathered(*runs[0], seq, pos, g, n_kv)
    ulp_check(y.reshape(R, -1), want_y.reshape(R, -1), **(ulps or {}))
    want = y.clone()
    want[:, :, : g + 1] = _rope_ref(y[:, :, : g + 1], pos.cuda(), cos, sin)     # query slots and K rotated, V as it is
    got = _gathered(*runs[1], seq, pos, g, n_kv)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    return runs[1]


def _rmsnorm(lib, x, w, eps=1e-5):
    R, K = x.shape
    y = sentinel(R, K)
    check(lib.aigv_op_rmsnorm(x.data_ptr(), K, w.data_ptr(), y.data_ptr(), K, R, K, eps, None, None))
    xf = x.float()
    ulp_check(y, rb(w.float() * rb(xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))))
    return y


def _inputs(R, N, K, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, K, generator=gen) * 0.5).to(BF)
    W = (torch.randn(N, K, generator=gen) / math.sqrt(K)).to(BF)
    gw = (torch.rand(K, generator=gen) + 0.5).to(BF)
    return x.cuda(), W.cuda(), gw.cuda()


@pytest.mark.parametrize("R,p,K,g,n_kv", [(1, 1, 512, 4, 2), (3, 1, 512, 4, 2), (4, 1, 1024, 4, 2), (17, 1, 512, 6, 1), (64, 1, 384, 1, 3), (33, 1, 128, 1, 1),
                                          (8, 2, 1024, 4, 2), (3, 2, 512, 2, 2), (4, 4, 1024, 4, 2), (1, 4, 2048, 8, 1)])
def test_rope_kv_gemv_matches_reference(lib, R, p, K, g, n_kv):
    """Rows with their own cache sequence and position: query slots rotated into the qkv row, K rotated and V as computed into
    [seq][kvh][pos] of the caches, nothing else written."""
    N = n_kv * (g + 2) * D
    x, W, _ = _inputs(R, N, K, seed=R * 7 + p + K)
    want_y = rb(x.float() @ W.float().t()).view(R, n_kv, g + 2, D)
    _rope_kv_case(lib, x, W, g, n_kv, p, want_y)


@pytest.mark.parametrize("R,p,K", [(1, 1, 4096), (4, 1, 6144), (3, 2, 4096), (4, 4, 6144), (2, 4, 4096), (2, 2, 6144)])
def test_rope_kv_gemv_fused_norm_is_rmsnorm_then_the_gemv(lib, R, p, K):
    """norm_w: the kernel normalises the raw residual rows itself - the same bits as aigv_op_rmsnorm followed by the plain form."""
    g, n_kv = 4, 2
    N = n_kv * (g + 2) * D
    x, W, gw = _inputs(R, N, K, seed=R + p + K)
    xn = _rmsnorm(lib, x, gw)
    want_y = rb(xn.float() @ W.float().t()).view(R, n_kv, g + 2, D)
    plain = _rope_kv_case(lib, xn, W, g, n_kv, p, want_y)
    fused = _rope_kv_case(lib, x, W, g, n_kv, p, want_y, norm_w=gw)
    for a, b in zip(plain, fused):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("R,p,K,N", [(1, 1, 4096, 1024), (4, 2, 6144, 512), (3, 4, 4096, 768), (2, 1, 6144, 256), (2, 2, 4096, 64), (4, 4, 6144, 64)])
def test_swiglu_normed_gemv_is_rmsnorm_then_the_swiglu_gemv(lib, R, p, K, N):
    x, W, gw = _inputs(R, N, K, seed=3 * R + p + K + N)
    xn = _rmsnorm(lib, x, gw)
    fused = sentinel(R + 1, N // 2)
    check(lib.aigv_op_skinny_swiglu_normed(x.data_ptr(), K, R, W.data_ptr(), K, N, K, fused.data_ptr(), N // 2, gw.data_ptr(), 1e-5, p, None))
    plain = sentinel(R + 1, N // 2)
    try:
        assert lib.aigv_tune_skinny(p) == 0
        check(lib.aigv_op_skinny_gemm(xn.data_ptr(), K, R, W.data_ptr(), K, N, K, None, None, 0, plain.data_ptr(), N // 2, 2, None))
    finally:
        lib.aigv_tune_skinny(0)
    assert is_sentinel(fused[R]).all() and is_sentinel(plain[R]).all()
    assert torch.equal(fused.view(torch.int16), plain.view(torch.int16))
    blk = (xn.float() @ W.float().t()).view(R, N // 32, 2, 16)          # w1 / w3 interleaved in 16-row blocks
    gate, up = rb(blk[:, :, 0]).reshape(R, -1), rb(blk[:, :, 1]).reshape(R, -1)
    ulp_check(fused[:R], rb(rb(torch.nn.functional.silu(gate)) * up), frac=0.03, max_ulps=4)


def _quant_ref(x_bf16):
    """oracle/fp8.py's row / channel quantisation (tests/test_gpu_ops.py)."""
    x = x_bf16.float()
    amax = x.abs().amax(dim=-1, keepdim=True)
    inv = torch.where(amax > 0, torch.full_like(amax, 448.0) / amax, torch.ones_like(amax))
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x * inv).to(torch.float8_e4m3fn), scale.reshape(-1)


@pytest.mark.parametrize("R,p,K", [(1, 1, 4096), (4, 1, 6144), (3, 2, 4096), (2, 2, 6144), (4, 4, 4096), (1, 4, 6144)])
def test_fp8_rope_kv_gemv_matches_its_arithmetic(lib, R, p, K):
    """The fp8 mode's wqkv GEMV (aigv_skinny_fp8 epi 7): RMSNorm and per-row quantisation inside the kernel, exact e4m3 products,
    y = bf16((acc * row scale) * channel scale), then the bf16 form's RoPE / KV-append epilogue - same cache and sentinel checks."""
    g, n_kv = 4, 2
    N = n_kv * (g + 2) * D
    x, W, gw = _inputs(R, N, K, seed=5 * R + p + K)
    x = x.clone()
    x[:, 5] *= 6.0                                                  # an outlier per row: the amax is not a typical element
    xf = x.float().cpu()
    xin = (gw.float().cpu() * rb(xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))).to(BF)
    qa, sa = _quant_ref(xin)
    qw, sw = _quant_ref(W.cpu())
    acc = ((qa.float().double() @ qw.float().double().t()).float() * sa[:, None]) * sw[None, :]
    want_y = rb(acc).view(R, n_kv, g + 2, D)
    _rope_kv_case(lib, x, qw.view(torch.uint8).cuda(), g, n_kv, p, want_y, fp8_scale=sw.cuda(), norm_w=gw)


# ---------------------------------------------------------------------------------------------------------
# through the model
# ---------------------------------------------------------------------------------------------------------
def test_generate_after_the_kv_capacity_grew_past_16k():
    """generate() gives the same token bits before and after the context's KV capacity has grown past 16 384 tokens (the decode
    attention's merge pass was limited to 128 chunks: every decode step of such a context failed with 'invalid argument');
    a capacity above AIGV_MAX_KV_CAPACITY is refused with a message that says so."""
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    cfg = pkg.tiny(image_size=224)
    seed = 21
    sd = synth.make_state_dict(cfg, seed=seed, rich=True)
    toks = synth.canonical_tokens(cfg, 2, 2, seed=seed)
    n_prompt = int((toks["labels"][0] == -100).sum())
    ids = toks["input_ids"][:, :n_prompt].clone()
    ctx = toks["img_context_token_id"]
    for b in range(2):   # generate() prompts carry no motion slot: turn the lone trailing <IMG_CONTEXT> into text
        ids[b, (ids[b] == ctx).nonzero()[-1]] = 7
    pv = synth.synthetic_frames(4, 224, seed=seed)
    model = InternVLChatModel(cfg, stage=2)
    model.load_state_dict(sd)
    model = model.eval().cuda()
    model.img_context_token_id = ctx

    def gen():
        return model.generate(pixel_values=pv, input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=6, do_sample=False).cpu()
    before = gen()
    assert model._cap["kv"] < 16384
    model._native(kv_cap=20480)
    assert model._cap["kv"] == 20480
    after = gen()
    assert model._cap["kv"] == 20480
    assert torch.equal(before, after), (before.tolist(), after.tolist())
    with pytest.raises(native.NativeError, match="AIGV_MAX_KV_CAPACITY"):
        model._native(kv_cap=MAX_KV + 1)
