"""CPU side of the score-head parity tests (tests/test_gpu_row_ops.py): the truth chain, and inputs whose arithmetic is exact.

The head is a chain of ReLU(bf16(x W^T + b)) (modeling_internvl_chat.py:82-94) behind a NaN guard (:469-473).  ``chain`` states it with
fp64 sums and the same bf16 rounding points; ``exact_case`` draws weights, biases and inputs for which every sum is a bf16 number, so
that the result does not depend on the order of summation and a kernel must reproduce it bit for bit."""
import functools

import torch

BF = torch.bfloat16


def chain(x, Ws, bs, rounded=True):
    """fp64 sums; ``rounded``: one bf16 rounding after every Linear, as the kernels and the reference have it.  NaN and Inf propagate
    (torch.relu keeps a NaN)."""
    h = x.double()
    for W, b in zip(Ws, bs):
        h = h @ W.double().t() + b.double()
        if rounded:
            h = h.to(BF).double()
        h = torch.relu(h)
    return h[:, 0]


def guard(x):
    """CHAT:469-473: nan_to_num of the whole batch slice as soon as one element is NaN."""
    return torch.nan_to_num(x, nan=0.0, posinf=1e9, neginf=-1e9) if torch.isnan(x).any() else x


@functools.lru_cache(maxsize=None)
def exact_weights(dims, seed=1):
    """8 non-zeros per output row in the first layer, 4 in the others, from {+-1, +-0.5} (+-1 from the third layer on: every 0.5 halves the
    grid the values live on, and a bf16 number has 8 bits); where the fan-in allows it every input column is used equally often, so no
    input is ignored.  Biases are multiples of 2^-2.  Whether the draw is exact is not assumed: the tests assert ``is_exact`` first."""
    g = torch.Generator().manual_seed(1000 + seed + sum(dims))
    Ws, bs = [], []
    for layer, (din, dout) in enumerate(zip(dims[:-1], dims[1:])):
        nnz = min(8 if layer == 0 else 4, din)
        vals = torch.tensor([1.0, -1.0, 0.5, -0.5] if layer < 2 else [1.0, -1.0])
        if din % nnz == 0:
            need = dout * nnz
            cols = torch.cat([torch.randperm(din, generator=g) for _ in range(-(-need // din))])[:need].view(dout, nnz)
        else:
            cols = torch.stack([torch.randperm(din, generator=g)[:nnz] for _ in range(dout)])
        W = torch.zeros(dout, din)
        W.scatter_(1, cols, vals[torch.randint(0, len(vals), (dout, nnz), generator=g)])
        Ws.append(W.to(BF))
        bs.append((torch.randint(-1, 3, (dout,), generator=g) * 0.25).to(BF))
    return tuple(Ws), tuple(bs)


def exact_inputs(B, H, seed=0):
    g = torch.Generator().manual_seed(77 + 131 * B + H + seed)
    return (torch.randint(-2, 3, (B, H), generator=g) * 0.25).to(BF)


def is_exact(x, Ws, bs):
    """No bf16 rounding point of the chain rounds: the fp64 chain without roundings gives the same numbers (fp32 partial sums of these
    few small dyadic terms are exact in any order)."""
    return torch.equal(chain(x, Ws, bs, rounded=False), chain(x, Ws, bs, rounded=True))


def single_big_term(x, Ws, bs, big=2.0 ** 20, small=2.0 ** 10):
    """The guarded inputs carry +-1e9 next to the small dyadic numbers, and 1e9 + 0.25 is no fp32 number.  The result is still independent
    of the summation order if every sum holds AT MOST ONE big term, a bf16 number times +-1 or +-0.5, and the rest stays small: the sum
    then rounds to that term (half a bf16 ulp of 2^20 is 2^12).  True if that holds at every unit of the chain."""
    h = x.double()
    for W, b in zip(Ws, bs):
        Wd = W.double()
        is_big = h.abs() >= big
        if ((is_big.double() @ (Wd != 0).double().t()) > 1).any():
            return False
        rest = torch.where(is_big, torch.zeros_like(h), h).abs() @ Wd.abs().t() + b.double().abs()
        if (rest >= small).any():
            return False
        h = torch.relu((h @ Wd.t() + b.double()).to(BF).double())
    return True
