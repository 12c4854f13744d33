"""What ``forward(return_score_values=True)`` costs at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames, SlowFast motion branch,
synthetic weights - bench.py's step): ms per eager step for THREE variants - unarmed | armed with the bins only (``return_score_attention``) |
armed with the bins and the value vectors (``return_score_values``) - in ONE process on one box, the variants alternating block by block so
that drift hits all of them; medians, minima and maxima over the blocks' per-step times (device-synchronised host clock around every step).
Eager only: a call with the flag runs eagerly under graph replay too.  The armed costs have no bar - they are reported, each against the unarmed
variant's own spread - and the report ends with the completeness distance at this shape: the value vectors summed over the sources against the
pass's own head outputs (``return_heads`` at the score rows), per layer.
Usage: python scripts/score_values_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--out profiles/score_values_cost.txt]
       (appends its report to --out; needs an MI355X)."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = (("unarmed", {}), ("bins", dict(return_score_attention=True)), ("bins + values", dict(return_score_values=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import eval_utils, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.slowfast import SlowFastR50
    if not torch.cuda.is_available():
        raise SystemExit("score_values_cost.py measures on the GPU: no device, no number")
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

    def step(flag_kw):
        t0 = time.perf_counter()
        out = model(**kw, **flag_kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    lines = [f"score_values_cost: model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), {llm.num_hidden_layers} layers, "
             f"{llm.num_attention_heads} heads x {llm.head_dim}; eager, {args.blocks} alternating blocks x {args.steps} steps per variant",
             f"device: {torch.cuda.get_device_name(0)}"]
    for _, flag_kw in VARIANTS:            # warm-up: every kernel loaded
        for _ in range(3):
            step(flag_kw)
    times = {name: [] for name, _ in VARIANTS}
    for _ in range(args.blocks):
        for name, flag_kw in VARIANTS:
            times[name] += [step(flag_kw)[0] for _ in range(args.steps)]
    med = {n: statistics.median(v) for n, v in times.items()}
    for n, _ in VARIANTS:
        lines.append(f"  {n:14s} {med[n]:8.3f} ms/step (min {min(times[n]):.3f}, max {max(times[n]):.3f}, {len(times[n])} steps)")
    spread = f"the unarmed pass's own spread: {min(times['unarmed']) - med['unarmed']:+.3f} .. {max(times['unarmed']) - med['unarmed']:+.3f} ms"
    for n in ("bins", "bins + values"):
        lines.append(f"  {n} - unarmed {med[n] - med['unarmed']:+.3f} ms ({100 * (med[n] / med['unarmed'] - 1):+.2f} %); {spread}")
    per_layer = (med["bins + values"] - med["bins"]) / llm.num_hidden_layers
    lines.append(f"  values - bins {med['bins + values'] - med['bins']:+.3f} ms = {1e3 * per_layer:+.1f} us per layer ({B} x {llm.num_attention_heads} workgroups per launch)")
    _, off = step({})
    _, bins_on = step(VARIANTS[1][1])
    rows = model.segment_masks(kw["input_ids"], kw["attention_mask"], flags)["score_row"]
    _, on = step(dict(return_score_values=True, return_heads=rows))
    same = all(torch.equal(on[k], off[k]) for k in ("score1", "logit"))
    same_bins = torch.equal(on["score_attention"].view(torch.int32), bins_on["score_attention"].view(torch.int32))
    val, rest = on["score_values"], on["score_values_rest"]
    lines.append(f"armed pass: score1 / logit bits {'unchanged' if same else 'CHANGED'}; score_attention bits beside the values {'unchanged' if same_bins else 'CHANGED'}; "
                 f"score_values {tuple(val.shape)}, score_values_rest all zero: {bool((rest == 0).all())}")
    dist = ((val.sum(3) + rest).double() - on["heads"].float().double()).abs().amax((0, 2, 3))
    scale = on["heads"].float().abs().amax((0, 2, 3))
    lines.append("completeness, max |score_values.sum(3) + score_values_rest - heads| per layer (largest |heads| element of that layer in brackets): "
                 + ", ".join(f"{d:.2e} [{s:.2f}]" for d, s in zip(dist.tolist(), scale.tolist())))
    norms = eval_utils.source_writes(model, on)
    sal_w, sal_a = eval_utils.frame_write_saliency(norms), eval_utils.frame_saliency(on["score_attention"])
    lines.append(f"clip 0 (synthetic weights - the shape of the read-out, not a finding): frame_saliency {[round(v, 3) for v in sal_a[0].tolist()]}, "
                 f"frame_write_saliency {[round(v, 3) for v in sal_w[0].tolist()]}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
