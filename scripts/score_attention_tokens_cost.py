"""What ``forward(return_token_attention=True)`` costs at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames, SlowFast motion branch,
synthetic weights - bench.py's step): ms per step for THREE variants - unarmed | armed with the bins only (``return_score_attention``) | armed
with the bins and the dense per-key rows (``return_token_attention``) - eager and under graph replay, in ONE process on one box, the variants
alternating block by block so that drift hits all of them; medians over the blocks' per-step times (device-synchronised host clock around
every step).  ``--parent-root DIR`` adds the unarmed figure of ANOTHER checkout (the parent commit, built beside this one) from the same box
and session: a fresh child process runs this file against that tree (``--root DIR --unarmed-only``: it passes no flag the parent lacks).
The unarmed pass enters no new code; the armed costs have no bar - they are reported.
Usage: python scripts/score_attention_tokens_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--parent-root DIR]
       [--out profiles/score_attention_tokens_cost.txt]   (appends its report to --out; needs an MI355X)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = (("unarmed", {}), ("bins", dict(return_score_attention=True)), ("bins + tokens", dict(return_token_attention=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--unarmed-only", action="store_true", help="measure the unarmed variant alone (what a parent checkout can run)")
    ap.add_argument("--parent-root", default="", help="also report the unarmed figure of this checkout (child process, same box)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.slowfast import SlowFastR50
    if not torch.cuda.is_available():
        raise SystemExit("score_attention_tokens_cost.py measures on the GPU: no device, no number")
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
    variants = VARIANTS[:1] if args.unarmed_only else VARIANTS

    def step(flag_kw):
        t0 = time.perf_counter()
        out = model(**kw, **flag_kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    where = "this checkout" if os.path.abspath(args.root) == HERE else f"checkout {os.path.basename(os.path.abspath(args.root))}"
    lines = [f"score_attention_tokens_cost ({where}): model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), "
             f"{args.blocks} alternating blocks x {args.steps} steps per variant",
             f"device: {torch.cuda.get_device_name(0)}"]
    for mode in ("eager", "graph replay"):
        model.enable_graph_replay(mode != "eager")
        for _, flag_kw in variants:            # warm-up: every kernel loaded, every call shape captured (first call eager, second captured)
            for _ in range(4):
                step(flag_kw)
        times = {name: [] for name, _ in variants}
        for _ in range(args.blocks):
            for name, flag_kw in variants:
                times[name] += [step(flag_kw)[0] for _ in range(args.steps)]
        med = {n: statistics.median(v) for n, v in times.items()}
        lo = {n: min(v) for n, v in times.items()}
        line = f"{mode:13s}" + "   ".join(f"{n} {med[n]:8.3f} ms/step (min {lo[n]:.3f})" for n, _ in variants)
        if not args.unarmed_only:
            line += "".join(f"   {n} - unarmed {med[n] - med['unarmed']:+.3f} ms ({100 * (med[n] / med['unarmed'] - 1):+.2f} %)" for n, _ in variants[1:])
            line += f"   tokens - bins {med['bins + tokens'] - med['bins']:+.3f} ms"
        lines.append(line)
    model.enable_graph_replay(False)
    if not args.unarmed_only:
        _, tok_on = step(VARIANTS[2][1])
        _, bins_on = step(VARIANTS[1][1])
        _, off = step({})
        same = all(torch.equal(tok_on[k], off[k]) for k in ("score1", "logit"))
        same_bins = torch.equal(tok_on["score_attention"].view(torch.int32), bins_on["score_attention"].view(torch.int32))
        tok = tok_on["score_attention_tokens"]
        lines.append(f"armed pass: score1 / logit bits {'unchanged' if same else 'CHANGED'}; score_attention bits beside the dense rows "
                     f"{'unchanged' if same_bins else 'CHANGED'}; score_attention_tokens {tuple(tok.shape)}, max |row sum - 1| = "
                     f"{(tok.double().sum(-1) - 1).abs().max().item():.3g}")
        from aigv_assessor_amd import eval_utils
        pos = model.visual_token_positions(kw["input_ids"], kw["attention_mask"], flags)
        heat = eval_utils.frame_heatmaps(tok, pos)
        sal = eval_utils.frame_saliency(tok_on["score_attention"])
        lines.append(f"frame_heatmaps {tuple(heat.shape)}: max |heat.sum((2, 3)) - frame_saliency| = {(heat.double().sum((2, 3)) - sal.double()).abs().max().item():.3g}; "
                     f"hottest cell of clip 0, frame 0 (synthetic weights - shape of the read-out, not a finding): {divmod(int(heat[0, 0].argmax()), heat.shape[-1])}")
    if args.parent_root:
        cmd = [sys.executable, os.path.abspath(__file__), "--root", args.parent_root, "--unarmed-only", "--steps", str(args.steps), "--blocks", str(args.blocks),
               "--clips", str(B), "--frames", str(T), "--model", args.model]
        try:         # (a limit of its own: model set-up + 2 modes x blocks x steps of ~0.12 s, with room - a hung child must not hang the job)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300 + 2 * args.blocks * args.steps)
            if r.returncode != 0:
                lines.append(f"parent checkout: the child process failed ({r.returncode}): {r.stderr[-400:]}")
            else:
                lines += ["parent checkout, same box, same session (child process, unarmed only):"] + ["  " + l for l in r.stdout.strip().splitlines()]
        except subprocess.TimeoutExpired:
            lines.append("parent checkout: the child process ran into its time limit and was ended: no figure")
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
