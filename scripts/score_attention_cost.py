"""What ``forward(return_score_attention=True)`` costs at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames, SlowFast motion branch,
synthetic weights - bench.py's step): ms per step ARMED (the probe kernel behind every layer's wqkv + RoPE) against UNARMED, eager and under
graph replay, in ONE process on one box, the two variants alternating block by block so that drift hits both; medians over the blocks'
per-step times (device-synchronised host clock around every step).  The unarmed pass enters no new code; the armed cost has no bar - it is
reported.  Usage: python scripts/score_attention_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--out profiles/score_attention_cost.txt]
(appends its report to --out; needs an MI355X)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.slowfast import SlowFastR50
    if not torch.cuda.is_available():
        raise SystemExit("score_attention_cost.py measures on the GPU: no device, no number")
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

    def step(armed):
        t0 = time.perf_counter()
        out = model(**kw, return_score_attention=armed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    lines = [f"score_attention_cost: model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), {args.blocks} alternating blocks x {args.steps} steps per variant",
             f"device: {torch.cuda.get_device_name(0)}"]
    for mode in ("eager", "graph replay"):
        model.enable_graph_replay(mode != "eager")
        for armed in (False, True):            # warm-up: every kernel loaded, both call shapes captured (first call eager, second captured)
            for _ in range(4):
                step(armed)
        times = {False: [], True: []}
        for _ in range(args.blocks):
            for armed in (False, True):
                times[armed] += [step(armed)[0] for _ in range(args.steps)]
        med = {a: statistics.median(v) for a, v in times.items()}
        lo = {a: min(v) for a, v in times.items()}
        lines.append(f"{mode:13s} unarmed {med[False]:8.3f} ms/step (min {lo[False]:.3f})   armed {med[True]:8.3f} ms/step (min {lo[True]:.3f})   "
                     f"armed - unarmed {med[True] - med[False]:+.3f} ms ({100 * (med[True] / med[False] - 1):+.2f} %)")
    model.enable_graph_replay(False)
    _, on = step(True)
    _, off = step(False)
    same = all(torch.equal(on[k], off[k]) for k in ("score1", "logit"))
    att = on["score_attention"]
    lines.append(f"armed pass: score1 / logit bits {'unchanged' if same else 'CHANGED'}; score_attention {tuple(att.shape)}, max |sum over bins - 1| = "
                 f"{(att.double().sum(-1) - 1).abs().max().item():.3g}")
    from aigv_assessor_amd import eval_utils
    lines.append("frame saliency of clip 0 (synthetic weights - shape of the read-out, not a finding): " +
                 " ".join(f"{v:.3f}" for v in eval_utils.frame_saliency(att)[0].tolist()))
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
