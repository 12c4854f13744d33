"""What the attention flow map (``forward(return_segment_attention=True)``; csrc/attnmap.hip) costs at the headline shape (InternVL2-8B sizes,
4 clips x 8 frames, SlowFast motion branch, synthetic weights - bench.py's step), in ONE process on one box:

* the pass: ms per eager step, unarmed | armed with the matrix (``eval_utils.flow_segments``' table, S = F + 5) | armed with the matrix and the
  rows of one layer (``return_row_attention=(0, 1)``) - the variants alternating block by block so that drift hits all of them; medians,
  minima and maxima of the per-step times (device-synchronised host clock around every step).  The unarmed variant launches exactly what the
  pass launched before the map existed: it is that code path.  Eager only: a call with either flag runs eagerly under graph replay too;
* the kernels, per layer: ``aigv_op_attention_map`` (the all-rows MFMA kernel + the fold) on fused rows of the pass's shape and the pass's own
  table, against THE ALTERNATIVE IT REPLACES - the same rows read by the score-row probe, ``aigv_op_attention_probe``, in ceil(T / 64) launches
  of 64 rows - alternating, device events around ``--reps`` back-to-back repetitions of each.  The ratio is reported as measured, whichever
  way it falls; no cost is a bar.
* the largest distance between the two kernels' rows (they sum in different orders).

Usage: python scripts/attention_map_cost.py [--steps 10] [--blocks 5] [--reps 10] [--model 8b|tiny] [--out profiles/attention_map_cost.txt]
       (appends its report to --out; needs an MI355X)."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--reps", type=int, default=10, help="kernel repetitions per timed window")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import eval_utils, native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel, rope_tables
    from aigv_assessor_amd.slowfast import SlowFastR50
    if not torch.cuda.is_available():
        raise SystemExit("attention_map_cost.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.tiny(image_size=448)
    B, T = args.clips, args.frames
    N = synth.canonical_len(cfg, T)
    toks = synth.canonical_tokens(cfg, B, T, seed=0)
    model = InternVLChatModel(cfg, device=dev, max_clips=B, max_frames=B * T, max_tokens=B * N)
    model.load_state_dict(synth.make_state_dict(cfg, seed=0, device=dev, rich=True))
    model.img_context_token_id = toks["img_context_token_id"]
    model.eval()
    model.slowfast_model = SlowFastR50(synth.slowfast_state_dict(seed=0))
    pv = synth.synthetic_frames(B * T, cfg.image_size, seed=0).to(dev)
    flags = torch.ones(B * T, 1, dtype=torch.long)
    kw = dict(mos=None, pixel_values=pv, input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags, labels=toks["labels"])
    llm = cfg.llm_config
    L, nh, nkv, D = llm.num_hidden_layers, llm.num_attention_heads, llm.num_key_value_heads, llm.head_dim
    table = eval_utils.flow_segments(model, kw["input_ids"], kw["attention_mask"], flags)
    S = int(table.max()) + 1
    variants = (("unarmed", {}), ("matrix", dict(return_segment_attention=True, attention_segments=table)),
                ("matrix + rows of 1 layer", dict(return_segment_attention=True, return_row_attention=(0, 1), attention_segments=table)))

    def step(flag_kw):
        t0 = time.perf_counter()
        out = model(**kw, **flag_kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    plan = model._plan(kw["input_ids"], kw["attention_mask"], kw["labels"], flags, B * T)
    Tt = plan["cu"][-1]
    lines = [f"attention_map_cost: model {args.model}, {B} clips x {T} frames, {Tt} packed tokens run ({N} per clip), {L} layers, {nh} heads ({nkv} kv) x {D}, S = {S} segments; "
             f"eager, {args.blocks} alternating blocks x {args.steps} steps per variant",
             f"device: {torch.cuda.get_device_name(0)}"]
    for _, flag_kw in variants:            # warm-up: every kernel loaded
        for _ in range(3):
            step(flag_kw)
    times = {name: [] for name, _ in variants}
    for _ in range(args.blocks):
        for name, flag_kw in variants:
            times[name] += [step(flag_kw)[0] for _ in range(args.steps)]
    med = {n: statistics.median(v) for n, v in times.items()}
    for n, _ in variants:
        lines.append(f"  {n:26s} {med[n]:8.3f} ms/step (min {min(times[n]):.3f}, max {max(times[n]):.3f}, {len(times[n])} steps)")
    spread = f"the unarmed pass's own spread: {min(times['unarmed']) - med['unarmed']:+.3f} .. {max(times['unarmed']) - med['unarmed']:+.3f} ms"
    for n, _ in variants[1:]:
        lines.append(f"  {n} - unarmed {med[n] - med['unarmed']:+.3f} ms ({100 * (med[n] / med['unarmed'] - 1):+.2f} %) = {(med[n] - med['unarmed']) / L:+.3f} ms per layer, host side included; {spread}")
    _, off = step({})
    _, on = step(variants[2][1])
    same = all(torch.equal(on[k], off[k]) for k in ("score1", "logit"))
    sa = on["segment_attention"]
    sums = sa.double().sum(-1)
    lines.append(f"armed pass: score1 / logit bits {'unchanged' if same else 'CHANGED'}; segment_attention {tuple(sa.shape)}, segment_rows[0] {on['segment_rows'][0].tolist()}, "
                 f"largest |row sum - 1| over the non-empty rows {float((sums[~torch.isnan(sums)] - 1).abs().max()):.2e}; row_attention {tuple(on['row_attention'].shape)}")

    # ---- the kernels alone, per layer: random fused rows of the pass's shape, the pass's table and sequences -----------------------------------------
    lib = native.load()
    g = nh // nkv
    ld = nkv * (g + 2) * D
    fused = torch.randn(Tt, ld, device=dev, dtype=torch.float32).to(torch.bfloat16)
    cos, sin = rope_tables(D, llm.rope_theta, max(plan["lens"]), llm.max_position_embeddings, getattr(llm, "rope_scaling", None))
    cos, sin = cos.to(torch.bfloat16).to(dev).contiguous(), sin.to(torch.bfloat16).to(dev).contiguous()
    seg_d = table[plan["row_of"] >= 0].to(torch.int32).to(dev)
    cu = native.i32_array(plan["cu"])
    rows_map = torch.empty(Tt, nh, S, dtype=torch.float32, device=dev)
    fold = torch.empty(B, nh, S, S, dtype=torch.float32, device=dev)
    rows_probe = torch.empty(Tt, nh, S, dtype=torch.float32, device=dev)
    k_ptr = fused.data_ptr() + 2 * g * D
    chunks = [native.i32_array(list(range(r0, min(r0 + 64, Tt)))) for r0 in range(0, Tt, 64)]

    def run_map(with_fold=True):
        native.check(lib.aigv_op_attention_map(fused.data_ptr(), ld, k_ptr, ld, cu, B, nh, nkv, (g + 2) * D, (g + 2) * D, D, cos.data_ptr(), sin.data_ptr(), cos.shape[0],
                                               seg_d.data_ptr(), S, rows_map.data_ptr(), fold.data_ptr() if with_fold else None, native.stream_ptr()))

    def run_probe():
        for i, rows in enumerate(chunks):
            native.check(lib.aigv_op_attention_probe(fused.data_ptr(), ld, k_ptr, ld, cu, B, nh, nkv, (g + 2) * D, (g + 2) * D, 0, None, D, cos.data_ptr(), sin.data_ptr(),
                                                     cos.shape[0], rows, len(rows), seg_d.data_ptr(), None, 0, S, rows_probe.data_ptr() + 4 * 64 * i * nh * S, native.stream_ptr()))

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    kernels = (("map + fold", run_map), ("map alone", lambda: run_map(False)), (f"probe, {len(chunks)} launches of 64 rows", run_probe))
    for _, fn in kernels:
        fn()
    torch.cuda.synchronize()
    kt = {n: [] for n, _ in kernels}
    for _ in range(args.blocks):
        for n, fn in kernels:
            kt[n].append(timed(fn, args.reps if fn is not run_probe else max(1, args.reps // 5)))
    kmed = {n: statistics.median(v) for n, v in kt.items()}
    lines.append(f"kernels alone, one layer ({Tt} rows x {nh} heads, random bf16 rows, device events, {args.blocks} alternating windows):")
    for n, _ in kernels:
        lines.append(f"  {n:36s} {kmed[n]:9.3f} ms (min {min(kt[n]):.3f}, max {max(kt[n]):.3f})")
    probe_name = kernels[2][0]
    ratio = kmed[probe_name] / kmed["map + fold"]
    lines.append(f"  the chunked probe over the map kernel with its fold: {ratio:.1f} x - the map kernel is {'FASTER' if ratio > 1 else 'NOT faster'} per layer than the alternative it replaces")
    keys = sum(n * (n + 1) // 2 for n in plan["lens"])
    lines.append(f"  map alone: {2.0 * keys * nh * D / (kmed['map alone'] * 1e-3) / 1e12:.1f} TFLOP/s of Q.K^T counted once ({keys} (row, key) pairs x {nh} heads x 2 D; the kernel forms every score twice)")
    lines.append(f"  largest |map - probe| over all rows: {float((rows_map - rows_probe).abs().max()):.3e}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
