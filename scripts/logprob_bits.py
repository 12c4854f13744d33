"""One SHA-256 per case over the raw output bytes of the four op-level log-probability entry points (aigv_op_label_logprob,
aigv_op_cand_logprob, aigv_op_lm_head_argmax_logprob, aigv_op_lm_head_argmax_cand_logprob): two builds of the library compute the same bits
exactly when their listings are identical.  The existing tests hold the kernels against each other and against fp64; this holds them against
another build (AIGV_AMD_LIB=<other libaigv_amd.so> selects it), e.g. the parent commit's when the reduction is reshaped.

python scripts/logprob_bits.py [--out FILE]

Inputs are synth.hashed_uniform's (the same bits on every device and build), scaled so that a row spans several units of logit.  V < 1024
leaves threads with an empty (-inf, 0) pair, V = 17 whole waves; C = 17 crosses the candidate GEMV's 16-candidate workgroup; 64 rows is
the launchers' cap; ldo = V runs the scalar load form, ldo = ceil4(V) the vector form.  At V = 2053 some rows carry a -inf column, a row of
all-equal values, an out-of-range label and an out-of-range candidate id."""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aigv_assessor_amd import native, synth  # noqa: E402

VOCABS = (1, 17, 515, 2053, 92553)
ROWS = (1, 3, 64)
CANDS = (1, 5, 16, 17, 64)
HIDDENS = (384, 640)
PLANTED_V = 2053
DEV = "cuda"


def digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def labels_of(V: int, rows: int) -> torch.Tensor:
    lab = torch.tensor([(131 * r + 7) % V for r in range(rows)], dtype=torch.long)
    if V == PLANTED_V and rows > 2:
        lab[2] = -100                                  # an out-of-range label: NaN
    return lab.to(DEV)


def cands_of(V: int, C: int) -> torch.Tensor:
    cand = torch.tensor([(7919 * i + 3) % V for i in range(C)], dtype=torch.long)
    if V == PLANTED_V and C > 1:
        cand[1] = V + 5                                # an out-of-range candidate: a NaN column
    return cand.to(DEV)


def logits_of(V: int, ldo: int) -> torch.Tensor:
    x = synth.hashed_uniform((64, ldo), key=1000 + V, std=3.0, device=DEV)
    if ldo > V:
        x[:, V:] = 100.0                               # padding columns must not count
    if V == PLANTED_V:
        x[0, 1234] = float("-inf")
        x[1, :V] = 0.75                                # a row of all-equal values
    return x.contiguous()


def logits_cases(lib, emit):
    for V in VOCABS:
        for ldo in sorted({V, (V + 3) // 4 * 4}):
            x = logits_of(V, ldo)
            for rows in ROWS:
                out = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV)
                native.check(lib.aigv_op_label_logprob(x.data_ptr(), rows, V, ldo, labels_of(V, rows).data_ptr(), out.data_ptr(), native.stream_ptr()))
                emit(f"label_logprob V={V} ldo={ldo} rows={rows}", out)
                for C in CANDS:
                    out = torch.full((rows, C), 7.0, dtype=torch.float32, device=DEV)
                    native.check(lib.aigv_op_cand_logprob(x.data_ptr(), rows, V, ldo, cands_of(V, C).data_ptr(), C, out.data_ptr(), native.stream_ptr()))
                    emit(f"cand_logprob V={V} ldo={ldo} rows={rows} C={C}", out)


def lm_head_cases(lib, emit):
    for V in VOCABS:
        for H in HIDDENS:
            h = synth.hashed_uniform((64, H), key=2000 + V + H, std=1.0, device=DEV)
            W = synth.hashed_uniform((V, H), key=3000 + V + H, std=0.15, device=DEV)     # logits of standard deviation 0.15 sqrt(H): about 3
            if V == PLANTED_V:
                h[1] = 0                               # a row of all-equal (zero) logits
            for rows in ROWS:
                hr = h[:rows].contiguous()

                def outputs():
                    return (torch.full((rows,), -7, dtype=torch.long, device=DEV), torch.full((rows,), 7.0, dtype=torch.float32, device=DEV),
                            torch.full((rows,), 7.0, dtype=torch.float32, device=DEV))

                nbytes = lib.aigv_op_lm_head_argmax_logprob_scratch_bytes(rows, V)
                scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
                idx, val, lp = outputs()
                native.check(lib.aigv_op_lm_head_argmax_logprob(hr.data_ptr(), rows, H, W.data_ptr(), V, scratch.data_ptr(), nbytes, idx.data_ptr(),
                                                                val.data_ptr(), lp.data_ptr(), native.stream_ptr()))
                emit(f"lm_head_argmax_logprob V={V} H={H} rows={rows}", idx, val, lp)
                nbytes = lib.aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(rows, V)
                for C in CANDS:
                    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
                    idx, val, lp = outputs()
                    clp = torch.full((rows, C), 7.0, dtype=torch.float32, device=DEV)
                    native.check(lib.aigv_op_lm_head_argmax_cand_logprob(hr.data_ptr(), rows, H, W.data_ptr(), V, cands_of(V, C).data_ptr(), C, scratch.data_ptr(),
                                                                         nbytes, idx.data_ptr(), val.data_ptr(), lp.data_ptr(), clp.data_ptr(), native.stream_ptr()))
                    emit(f"lm_head_argmax_cand_logprob V={V} H={H} rows={rows} C={C}", idx, val, lp, clp)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="", help="also write the listing to this file")
    args = ap.parse_args()
    lib = native.load()
    lines = []

    def emit(name, *tensors):
        torch.cuda.synchronize()
        lines.append(f"{digest(*tensors)}  {name}")
        print(lines[-1], flush=True)

    logits_cases(lib, emit)
    lm_head_cases(lib, emit)
    print(f"{len(lines)} cases; sha256 of the listing: {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
