"""What ``generate*(key_drop=...)`` and ``eval_utils.frame_ablation_generate`` cost at the 8B shape (InternVL2-8B sizes, 1 clip x 8 frames,
synthetic weights, the motion feature an input), eager, in ONE process on one box, the variants alternating block by block; medians over
the blocks (device-synchronised host clock around every call):

  decode            generate_stage2(...)                          ms/token: (time of ``--new`` tokens - time of 1 token) / (new - 1)
  decode, frame off the same with key_drop = unit_masks[:, 0]     one frame (256 tokens: two whole 128-key chunks and parts of two more) hidden
  ablation          eval_utils.frame_ablation_generate            8 frames: 10 replies, InternViT once
  10 x generate     ten separate generate_stage2(pixel_values=..) what the loop costs without the helper (InternViT ten times)

The unmasked decode of the parent commit against this tree is a separate A/B (scripts/decode_bench.py from either tree, alternated).
No bar is set for any of these: they are recorded.
Usage: python scripts/key_drop_cache_cost.py [--new 33] [--blocks 3] [--model 8b|tiny] [--out profiles/key_drop_cache_cost.txt]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=33, help="new tokens of the decode measurement")
    ap.add_argument("--reply", type=int, default=8, help="new tokens of every reply of the ablation measurement")
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import eval_utils, native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    if not torch.cuda.is_available():
        raise SystemExit("key_drop_cache_cost.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.tiny(image_size=448)
    T = args.frames
    toks = synth.canonical_tokens(cfg, 1, T, seed=0)
    model = InternVLChatModel(cfg, device=dev, max_clips=1, max_frames=T)
    model.load_state_dict(synth.make_state_dict(cfg, seed=0, device=dev, rich=True))
    model.img_context_token_id = toks["img_context_token_id"]
    model.eval()
    n_prompt = int((toks["labels"][0] == -100).sum())
    ids = toks["input_ids"][:, :n_prompt].clone()
    am = torch.ones_like(ids, dtype=torch.bool)
    flags = torch.ones(T, 1, dtype=torch.long)
    pv = synth.synthetic_frames(T, cfg.image_size, seed=0).to(dev)
    mf = synth.synthetic_motion(1, cfg.motion_dim, seed=0).to(dev).to(torch.bfloat16)
    units = model.unit_masks(ids, am, flags)
    tokens = model.vit_tokens(pv)
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def reply(n, **kw):
        return lambda: model.generate_stage2(None, ids, am, flags, mf, visual_tokens=tokens, max_new_tokens=n, **kw)

    def per_token(**kw):
        return (timed(reply(args.new, **kw)) - timed(reply(1, **kw))) / (args.new - 1)

    abl = lambda: eval_utils.frame_ablation_generate(model, pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=flags, max_new_tokens=args.reply,
                                                     motion_feature=mf)

    def ten():
        model.generate_stage2(pv, ids, am, flags, mf, max_new_tokens=args.reply)
        for u in range(units.shape[1]):
            model.generate_stage2(pv, ids, am, flags, mf, max_new_tokens=args.reply, key_drop=units[:, u])

    variants = {"decode": lambda: per_token(), "decode, frame off": lambda: per_token(key_drop=units[:, 0]), "ablation": lambda: timed(abl), "10 x generate": lambda: timed(ten)}
    for fn in variants.values():
        fn()                                                    # warms every shape up
    times = {name: [] for name in variants}
    for _ in range(args.blocks):
        for name, fn in variants.items():
            times[name].append(fn())
    med = {n: statistics.median(v) for n, v in times.items()}
    unit = {n: "ms/token" if n.startswith("decode") else "ms/call" for n in variants}
    lines = [f"key_drop_cache_cost (library {os.path.relpath(native.LIB_PATH, HERE)}): model {args.model}, 1 clip x {T} frames, prompt {n_prompt} tokens, eager, "
             f"{args.blocks} alternating blocks; decode over {args.new} new tokens, replies of {args.reply}",
             f"device: {torch.cuda.get_device_name(0)}"]
    lines += [f"  {n:18s} {med[n]:9.3f} {unit[n]} (min {min(times[n]):.3f}, max {max(times[n]):.3f}, {len(times[n])} blocks)" for n in variants]
    lines.append(f"  decode, frame off - decode {med['decode, frame off'] - med['decode']:+.3f} ms/token ({100 * (med['decode, frame off'] / med['decode'] - 1):+.2f} %); "
                 f"hidden tokens: {int(units[0, 0].sum())} of {n_prompt}")
    lines.append(f"  ablation / 10 x generate {med['ablation'] / med['10 x generate']:.2f} ({T + 2} replies each)")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
