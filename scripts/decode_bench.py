"""generate() throughput on the 8B model: prefill + greedy decode steps (HBM-bound weight streaming).
python scripts/decode_bench.py [batch] [new tokens] [num_beams]   (num_beams > 1: HF beam search, all beams in one decode step per token)
LOGPROBS=1: greedy decode in three variants, alternated in one process - flags off, return_logprobs (the log-sum-exp fused into the
decode step's lm-head argmax) and a two-pass form (aigv_out_row_logprob after every decode step: the lm-head streamed a second time)."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aigv_assessor_amd as pkg
from aigv_assessor_amd import synth
from aigv_assessor_amd.modeling import InternVLChatModel
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
new = int(sys.argv[2]) if len(sys.argv) > 2 else 33
beams = int(sys.argv[3]) if len(sys.argv) > 3 else 1
gen = dict(num_beams=beams) if beams > 1 else {}
cfg = pkg.internvl2_8b()
dev = torch.device('cuda', 0)
model = InternVLChatModel(cfg, device=dev, max_clips=B)
model.load_state_dict(synth.make_state_dict(cfg, seed=0, device=dev, rich=True))
if os.environ.get("PREC") == "fp8":            # fp8 mode of the InternLM2 linears: the decode GEMVs stream the e4m3 copies
    model.set_precision("fp8")
toks = synth.canonical_tokens(cfg, B, 8, seed=0)
model.img_context_token_id = toks["img_context_token_id"]
n_prompt = int((toks["labels"][0] == -100).sum())
ids = toks["input_ids"][:, :n_prompt].clone()
for b in range(B):
    ids[b, (ids[b] == model.img_context_token_id).nonzero()[-1]] = 7
pv = synth.synthetic_frames(B * 8, 448, seed=0, device=dev)
if os.environ.get("LOGPROBS") == "1":
    from aigv_assessor_amd import native
    lib = native.load()
    plain_step = lib.aigv_decode_step
    lp_buf = torch.empty(B, dtype=torch.float32, device=dev)

    def two_pass_step(ctx, ids_p, next_p, stream):   # the decode step, then the separate lm-head + log-softmax of its token
        rc = plain_step(ctx, ids_p, next_p, stream)
        return rc or lib.aigv_out_row_logprob(ctx, 0, B, next_p, lp_buf.data_ptr(), stream)

    def run(variant, n):
        lib.aigv_decode_step = two_pass_step if variant == "two-pass" else plain_step
        try:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.generate(pixel_values=pv, input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=n, do_sample=False,
                           **({"return_logprobs": True} if variant == "fused" else {}))
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        finally:
            lib.aigv_decode_step = plain_step
    variants = ("off", "fused", "two-pass")
    times = {v: [] for v in variants}
    for rep in range(4):
        for v in variants:
            t = (run(v, new) - run(v, 1)) / (new - 1)
            if rep:                                   # rep 0 warms every shape up
                times[v].append(t)
    for v in variants:
        ts = sorted(times[v])
        print(f"B={B} {v:8s} decode {1e3*ts[len(ts)//2]:.3f} ms/token (min {1e3*ts[0]:.3f}, max {1e3*ts[-1]:.3f})", flush=True)
    sys.exit(0)
for rep in range(2):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = model.generate(pixel_values=pv, input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=1, **gen)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    out = model.generate(pixel_values=pv, input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=new, **gen)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    per_tok = ((t2 - t1) - (t1 - t0)) / (new - 1)
    wbytes = sum(p.numel() for n, p in model.named_parameters() if n.startswith("language_model.model.layers") or n == "language_model.output.weight") * 2
    print(f"B={B} beams={beams} prefill+1 {1e3*(t1-t0):.1f} ms; decode {1e3*per_tok:.2f} ms/token ({B/per_tok:.1f} tok/s), weights streamed {wbytes/1e9:.1f} GB -> {wbytes/per_tok/1e12:.2f} TB/s", flush=True)
print(out[0].tolist()[:10])
