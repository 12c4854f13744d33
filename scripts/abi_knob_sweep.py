"""Two builds of libaigv_amd.so answer the tuning entry points and the GEMM planner alike, call for call.

    python scripts/abi_knob_sweep.py <lib A> <lib B> [--ctx]

Each library is driven in a child process of its own through one fixed sequence of calls: aigv_tune_default over knob -1..15 and the
values below, aigv_tune_skinny / _attention / _co_gemm over the same values, aigv_tune_gemm over its packed mode words, and
aigv_plan_gemm over a grid of problems under process modes 0, 1, 2.  Recorded per call: the return code and aigv_last_error(NULL) (the
text is not cleared by a successful call - hence ONE sequence for both), for the planner the seven plan words and the bits of est_us.
None of that needs a GPU.  --ctx (on an MI355X) adds aigv_ctx_tune over the same knobs and values on one tiny context, with
aigv_last_error(ctx).  Prints the number of calls and "0 differences", or the first differing calls; exit status 1 if any.
"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = [-2, -1] + list(range(18)) + [63, 64, 100, 1000, 5095, 5096, 65536, 65600]
KNOBS = list(range(-1, 16))
MODE_WORDS = list(range(6)) + [16 * v for v in range(9)] + [2 | f << 10 for f in range(16)] + [32 | b << 14 for b in range(4)]
PLAN_M = [1, 64, 257, 1025, 2177, 8200, 8708]
PLAN_N = [128, 1024, 3072, 3200, 4096, 6144, 28672]
PLAN_K = [640, 1024, 4096, 14336]
N_EPI = 6   # kernels.h EPI_COUNT


def child(path: str, with_ctx: bool) -> None:
    import torch  # noqa: F401  (first: the library binds to the HIP runtime torch has loaded)
    sys.path.insert(0, ROOT)
    from aigv_assessor_amd import native
    lib = C.CDLL(path)
    for name, (res, args) in native.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    out = []

    def rec(tag, rc, ctx=None, extra=None):
        out.append([tag, rc, (lib.aigv_last_error(ctx) or b"").decode(), extra])

    for k in KNOBS:
        for v in VALUES:
            rec(f"default {k} {v}", lib.aigv_tune_default(k, v))
    for name in ("aigv_tune_skinny", "aigv_tune_attention", "aigv_tune_co_gemm"):
        for v in VALUES:
            rec(f"{name} {v}", getattr(lib, name)(v))
    for w in MODE_WORDS:
        rec(f"aigv_tune_gemm {w}", lib.aigv_tune_gemm(w, 0.0))
    plan, est = (C.c_int * 7)(), C.c_double()
    for mode in (0, 1, 2):
        rec(f"aigv_tune_gemm {mode}", lib.aigv_tune_gemm(mode, 0.0))
        for m in PLAN_M:
            for n in PLAN_N:
                for kk in PLAN_K:
                    for epi in range(N_EPI):
                        for i in range(7):
                            plan[i] = -99
                        est.value = -1.0
                        rc = lib.aigv_plan_gemm(m, n, kk, epi, plan, C.byref(est))
                        rec(f"plan {mode} {m} {n} {kk} {epi}", rc, None, [list(plan), struct.pack("<d", est.value).hex()])
    lib.aigv_tune_gemm(0, 0.0)
    if with_ctx:
        import aigv_assessor_amd as pkg
        cfg = pkg.tiny(image_size=224)
        v, l = cfg.vision_config, cfg.llm_config
        c = native.AigvConfig()
        c.vit_hidden, c.vit_inter, c.vit_heads, c.vit_layers = v.hidden_size, v.intermediate_size, v.num_attention_heads, v.num_hidden_layers
        c.image_size, c.patch_size, c.num_channels = 224, v.patch_size, v.num_channels
        c.vit_norm_rms, c.vit_qk_norm, c.vit_qkv_bias, c.vit_eps = 0, int(v.qk_normalization), int(v.qkv_bias), v.layer_norm_eps
        c.select_layer, c.shuffle = -1, 2
        c.llm_hidden, c.llm_inter, c.llm_heads, c.llm_kv_heads = l.hidden_size, l.intermediate_size, l.num_attention_heads, l.num_key_value_heads
        c.llm_layers, c.vocab, c.rms_eps, c.max_positions, c.motion_dim = l.num_hidden_layers, l.vocab_size, l.rms_norm_eps, 64, cfg.motion_dim
        c.n_score_layers = 1
        c.score_dims[0] = 1
        c.max_frames, c.vit_chunk, c.max_tokens, c.max_seqs, c.max_out_rows, c.kv_capacity = 1, 1, 64, 1, 1, 0
        h = C.c_void_p()
        rc = lib.aigv_ctx_create(0, C.byref(c), C.byref(h))
        rec("aigv_ctx_create", rc)
        if rc == 0:
            for k in KNOBS:
                for val in VALUES:
                    rec(f"ctx {k} {val}", lib.aigv_ctx_tune(h, k, val), h)
            for val in VALUES:
                rec(f"aigv_set_gemm_mode {val}", lib.aigv_set_gemm_mode(h, val), h)
            lib.aigv_ctx_destroy(h)
    json.dump(out, sys.stdout)


def main() -> int:
    if sys.argv[1] == "--child":
        child(sys.argv[2], "--ctx" in sys.argv)
        return 0
    libs = [os.path.abspath(a) for a in sys.argv[1:] if not a.startswith("--")]
    assert len(libs) == 2, __doc__
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    runs = []
    for p in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", p] + flags, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(f"{p}: child failed ({r.returncode})\n{r.stderr[-2000:]}")
            return 2
        runs.append(json.loads(r.stdout))
    a, b = runs
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    if len(a) != len(b):
        print(f"call counts differ: {len(a)} vs {len(b)}")
        return 1
    n_ctx = sum(1 for x in a if x[0].startswith("ctx "))
    for x, y in bad[:20]:
        print(f"A {x}\nB {y}")
    print(f"{len(a)} calls per library ({n_ctx} of them aigv_ctx_tune); {sum(1 for x in a if x[1] != 0)} refused by A: {len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
