"""One SHA-256 per case over the raw output bytes of the GEMM family, every epilogue over every route the op-level ABI can force: two builds
of the library compute the same bits exactly when their listings are identical (AIGV_AMD_LIB=<other libaigv_amd.so> selects the build),
e.g. the parent commit's when the epilogues are reshaped (csrc/epilogue.h).  The tests hold the kernels against torch and against each
other; this holds them against another build.

python scripts/gemm_epilogue_bits.py [--out FILE]

Routes: the 128 kernel; the 256 kernel in its three schedule variants (direct, LDS-staged + residual prefetch, balanced direct); the
co-resident kernel in both shipped schedules and its lone form; split-K on both tiles with 2 and 4 slices; row plans at the defaults, with
fused tails and with a lone body; the skinny kernel at p = 1 / 2 / 4 in its four epilogues; the e4m3 tile kernel, its split-K form and the
e4m3 GEMV.  Inputs are synth.hashed_uniform's (the same bits on every device and build): random data is the right kind here, the digest
compares a build with its parent, not with torch.  M = 520 has a ragged last tile of the 128 and 256 kernels, the row list 257 + 3 + 260 a
tiny tail, 40 + 480 a ragged tile tail whose K slices the fused launch takes; M = 77 is one ragged tile; one problem has no bias."""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aigv_assessor_amd import native, synth  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
TUNE_TAIL_SLICES, TUNE_FUSE_TAILS, TUNE_LONE_BODY = 7, 12, 13          # AIGV_TUNE_* (include/aigv_amd.h)
DEFAULT_WORD = 0 + 32                                                  # cost-model dispatch, the shipped schedule
# (M, N, K, with a bias)
PROBLEMS = ((520, 256, 512, True), (77, 512, 128, True), (600, 256, 256, False))
R_TAB_FUSED, R_TAB_LONE, R_TINY = 512, 1024, 8192                      # AIGV_ROUTE_* bits a row-plan case must show (aigv_gemm_route)
# per M: (name, (tail slices, fuse tails, lone body), sequence lengths, route bits the dispatcher must report).  A knob that is silently
# ignored would give a duplicate digest that looks like coverage: the script stops instead.
ROW_CASES = {
    520: (("defaults", (0, 0, 1), (257, 3, 260), R_TINY), ("fused tails", (2, 2, 1), (40, 480), R_TAB_FUSED), ("lone body", (0, 0, 2), (257, 3, 260), R_TAB_LONE)),
    77: (("defaults", (0, 0, 1), (77,), 0),),
    600: (("defaults", (0, 0, 1), (40, 560), 0), ("lone body", (0, 0, 2), (40, 560), R_TAB_LONE)),
}
TILE_ROUTES = (("128", 1), ("256 direct", 2 + 16), ("256 staged", 2 + 32), ("256 balanced direct", 2 + 64),
               ("co-resident blocks", 4 + 16), ("co-resident interleaved", 4 + 32), ("co-resident lone", 4 + 112))
SK_OF = {0: 0, 3: 1, 4: 2, 1: 3}                                       # GEMM epilogue -> aigv_op_skinny_gemm epilogue


def digest(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def n_out(N, epi):
    return N // 2 if epi == 4 else N


class Problem:
    """The operands of one (M, N, K): the same tensors for every epilogue and route."""

    def __init__(self, M, N, K, with_bias, key):
        self.M, self.N, self.K = M, N, K
        self.A = synth.hashed_uniform((M, K), key=key, std=1.0, device=DEV)
        self.W = synth.hashed_uniform((N, K), key=key + 1, std=K ** -0.5, device=DEV)
        self.bias = synth.hashed_uniform((N,), key=key + 2, std=0.5, device=DEV) if with_bias else None
        self.ls = synth.hashed_uniform((N,), key=key + 3, std=0.5, device=DEV)
        self.resid = synth.hashed_uniform((M, N), key=key + 4, std=1.0, device=DEV)
        self.np = M // next(d for d in range(2, M + 1) if M % d == 0)          # patches per frame: several frames wherever M is composite
        self.pos = synth.hashed_uniform((self.np + 1, N), key=key + 5, std=0.5, device=DEV)

    def out(self, epi, rows=None):
        rows = self.M if rows is None else rows
        if epi == 5:
            rows += rows // self.np
        return torch.full((rows, n_out(self.N, epi)), 7.0, dtype=BF, device=DEV)

    def args(self, C, epi):
        """(A, lda, W, ldw, C, ldc, bias, ls, resid, ldr): the leading arguments of aigv_op_gemm and its siblings."""
        no = n_out(self.N, epi)
        r = self.resid[:, :no].contiguous() if epi in (2, 3) else None
        self.keep = r                                                          # alive until the next call
        bias = self.bias
        return (self.A.data_ptr(), self.K, self.W.data_ptr(), self.K, C.data_ptr(), no, bias.data_ptr() if bias is not None else None,
                self.ls.data_ptr() if epi == 2 else None, r.data_ptr() if r is not None else None, no if r is not None else 0)


def restore(lib):
    native.check(lib.aigv_tune_gemm(DEFAULT_WORD, 0.0))
    native.check(lib.aigv_tune_co_gemm(0))
    native.check(lib.aigv_tune_default(TUNE_TAIL_SLICES, 0))
    native.check(lib.aigv_tune_default(TUNE_FUSE_TAILS, 0))
    native.check(lib.aigv_tune_default(TUNE_LONE_BODY, 1))
    native.check(lib.aigv_tune_skinny(0))


def tile_cases(lib, emit, P):
    tag = f"M={P.M} N={P.N} K={P.K} bias={int(P.bias is not None)}"
    for name, word in TILE_ROUTES:
        if (word & 7) == 2 and P.N % 256:
            continue
        for epi in range(6):
            C = P.out(epi)
            try:
                native.check(lib.aigv_tune_gemm(word, 0.0))
                native.check(lib.aigv_op_gemm(*P.args(C, epi), P.pos.data_ptr() if epi == 5 else None, P.np if epi == 5 else 0, P.M, P.N, P.K, epi,
                                              native.stream_ptr()))
            finally:
                restore(lib)
            emit(f"gemm {name} epi={epi} {tag}", C)
    for tile256 in (False, True):
        op = lib.aigv_op_gemm_splitk256 if tile256 else lib.aigv_op_gemm_splitk
        for S in (2, 4):
            if (P.K // 64) % S:
                continue
            ws = torch.zeros(S * P.M * P.N, dtype=torch.float32, device=DEV)
            for epi in range(5):
                C = P.out(epi)
                native.check(op(*P.args(C, epi), P.M, P.N, P.K, epi, S, ws.data_ptr(), native.stream_ptr()))
                emit(f"splitk {'256' if tile256 else '128'} S={S} epi={epi} {tag}", C)
    for name, (tail_slices, fuse, lone), lens, must in ROW_CASES[P.M]:
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        assert cu[-1] == P.M and (tail_slices < 2 or ((P.K // 64) % tail_slices == 0 and P.K // 64 // tail_slices >= 4))
        for epi in range(5):
            C = P.out(epi)
            try:
                native.check(lib.aigv_tune_default(TUNE_TAIL_SLICES, tail_slices))
                native.check(lib.aigv_tune_default(TUNE_FUSE_TAILS, fuse))
                native.check(lib.aigv_tune_default(TUNE_LONE_BODY, lone))
                lib.aigv_gemm_route(1)
                native.check(lib.aigv_op_gemm_rows(*P.args(C, epi), (ctypes.c_int32 * len(cu))(*cu), len(lens), P.N, P.K, epi, native.stream_ptr()))
                route = lib.aigv_gemm_route(1)
            finally:
                restore(lib)
            if route & must != must:
                raise SystemExit(f"rows {name} lens={lens} epi={epi} {tag}: the dispatcher reports route {route:#x}, the case is meant to show {must:#x}")
            emit(f"rows {name} lens={'+'.join(map(str, lens))} route={route:#x} epi={epi} {tag}", C)


def skinny_cases(lib, emit, P):
    tag = f"N={P.N} K={P.K} bias={int(P.bias is not None)}"
    for p, R in ((1, 64), (1, 5), (2, 8), (2, 3), (4, 4), (4, 1)):
        if P.K % (128 * p):
            continue
        for epi in (0, 3, 4, 1):
            if p > 1 and epi == 1:
                continue                                                       # the sub-slab forms have no GELU epilogue
            no = n_out(P.N, epi)
            out = P.out(epi, R)
            r = P.resid[:R, :no].contiguous() if epi == 3 else None
            try:
                native.check(lib.aigv_tune_skinny(p))
                native.check(lib.aigv_op_skinny_gemm(P.A.data_ptr(), P.K, R, P.W.data_ptr(), P.K, P.N, P.K, P.bias.data_ptr() if P.bias is not None else None,
                                                     r.data_ptr() if r is not None else None, no if r is not None else 0, out.data_ptr(), no, SK_OF[epi],
                                                     native.stream_ptr()))
            finally:
                restore(lib)
            emit(f"skinny p={p} R={R} epi={epi} {tag}", out)


def quantised(lib, x):
    """aigv_op_quant_fp8_rows: e4m3 bytes and row scales of bf16 rows."""
    rows, K = x.shape
    q = torch.zeros((rows, K), dtype=torch.uint8, device=DEV)
    s = torch.zeros((rows,), dtype=torch.float32, device=DEV)
    native.check(lib.aigv_op_quant_fp8_rows(x.data_ptr(), K, rows, K, q.data_ptr(), K, s.data_ptr(), native.stream_ptr()))
    return q, s


def fp8_cases(lib, emit, P):
    if P.N % 256 or P.K % 128:
        return
    tag = f"M={P.M} N={P.N} K={P.K} bias={int(P.bias is not None)}"
    A8, rs = quantised(lib, P.A)
    W8, cs = quantised(lib, P.W)
    for S in (0, 2):
        if S and (P.K // 128) % S:
            continue
        ws = torch.zeros(max(S, 1) * P.M * P.N, dtype=torch.float32, device=DEV)
        for epi in range(5):
            no = n_out(P.N, epi)
            C = P.out(epi)
            r = P.resid[:, :no].contiguous() if epi in (2, 3) else None
            bias = None if epi == 4 else P.bias
            native.check(lib.aigv_op_gemm_fp8(A8.data_ptr(), P.K, W8.data_ptr(), P.K, C.data_ptr(), no, rs.data_ptr(), cs.data_ptr(),
                                              bias.data_ptr() if bias is not None else None, P.ls.data_ptr() if epi == 2 else None,
                                              r.data_ptr() if r is not None else None, no if r is not None else 0, P.M, P.N, P.K, epi, S,
                                              ws.data_ptr() if S else None, native.stream_ptr()))
            emit(f"fp8 gemm slices={S} epi={epi} {tag}", C)


def fp8_gemv_cases(lib, emit):
    """The e4m3 decode GEMV: residual (K = 4096, no norm) and SwiGLU behind its RMSNorm (K = 4096), at p = 1 / 2 / 4."""
    N, K = 256, 4096
    x = synth.hashed_uniform((4, K), key=7001, std=0.7, device=DEV)
    W8, cs = quantised(lib, synth.hashed_uniform((N, K), key=7002, std=K ** -0.5, device=DEV))
    gw = synth.hashed_uniform((K,), key=7003, std=0.25, device=DEV) + 1.0
    resid = synth.hashed_uniform((4, N), key=7004, std=1.0, device=DEV)
    for p, R in ((1, 4), (2, 3), (4, 1)):
        for epi in (1, 2):
            no = N // 2 if epi == 2 else N
            out = torch.full((R, no), 7.0, dtype=BF, device=DEV)
            native.check(lib.aigv_op_skinny_gemm_fp8(x.data_ptr(), K, R, W8.data_ptr(), K, ctypes.cast(cs.data_ptr(), ctypes.POINTER(ctypes.c_float)), N, K,
                                                     resid.data_ptr() if epi == 1 else None, N if epi == 1 else 0, out.data_ptr(), no, epi,
                                                     gw.data_ptr() if epi == 2 else None, 1e-5, p, native.stream_ptr()))
            emit(f"fp8 gemv p={p} R={R} epi={epi} N={N} K={K}", out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="", help="also write the listing to this file")
    args = ap.parse_args()
    lib = native.load()
    lines = []

    def emit(name, t):
        torch.cuda.synchronize()
        lines.append(f"{digest(t)}  {name}")
        print(lines[-1], flush=True)

    restore(lib)
    for i, (M, N, K, with_bias) in enumerate(PROBLEMS):
        P = Problem(M, N, K, with_bias, key=5000 + 10 * i)
        tile_cases(lib, emit, P)
        skinny_cases(lib, emit, P)
        fp8_cases(lib, emit, P)
    fp8_gemv_cases(lib, emit)
    print(f"{len(lines)} cases; sha256 of the listing: {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
