"""What ``vit_tokens(patch_drop=...)`` and ``eval_utils.patch_occlusion`` cost at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames,
SlowFast motion branch, synthetic weights - bench.py's step), eager, in ONE process on one box, with scripts/key_drop_cost.py's method: the
variants alternate block by block so that drift hits all of them; medians over the blocks' per-call times (device-synchronised host clock around
every call):

  vit               vit_tokens(pixel_values)                                   the unmasked tower: what a masked pass is compared with
  vit, empty mask   the same with patch_drop all False                         the masked kernel in every layer, every word zero (host word build + upload too)
  vit, one block    one 4 x 4 block of visual tokens (64 of 1024 patches)      what one variant of the sweep runs: the mask loop on a few tiles
  vit, half frame   the left half of every frame (512 of 1024 patches)         mask loop on every tile
  vit, all but 4x4  every patch but one block                                  the whole-tile skip on most tiles
  step              forward(pixel_values=...)                                  the whole unmasked step, for scale
  occlusion         eval_utils.patch_occlusion, cell = 4 (16 blocks per frame) once: 8 masked ViT batches of 4 x 17 frames, 1 + 8 x 17 LLM passes

No bar is set for any of these: they are recorded.
Usage: python scripts/vit_key_drop_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--out profiles/vit_key_drop_cost.txt]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import eval_utils, native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.slowfast import SlowFastR50
    if not torch.cuda.is_available():
        raise SystemExit("vit_key_drop_cost.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.tiny(image_size=448)
    B, T = args.clips, args.frames
    N = synth.canonical_len(cfg, T)
    toks = synth.canonical_tokens(cfg, B, T, seed=0)
    g = int(round(model_tokens(cfg) ** 0.5))
    n_var = (g // args.cell) ** 2 + 1
    model = InternVLChatModel(cfg, device=dev, max_clips=B, max_frames=max(B * T, B * n_var), max_tokens=B * N)
    model.load_state_dict(synth.make_state_dict(cfg, seed=0, device=dev, rich=True))
    model.img_context_token_id = toks["img_context_token_id"]
    model.eval()
    model.slowfast_model = SlowFastR50(synth.slowfast_state_dict(seed=0))
    pv = synth.synthetic_frames(B * T, cfg.image_size, seed=0).to(dev)
    flags = torch.ones(B * T, 1, dtype=torch.long)
    text = dict(input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags, labels=toks["labels"])
    G = 2 * g
    none = torch.zeros(B * T, G, G, dtype=torch.bool)
    block, half, most = none.clone(), none.clone(), ~none
    block[:, 2 * args.cell:4 * args.cell, 2 * args.cell:4 * args.cell] = True
    half[:, :, :G // 2] = True
    most[:, :2 * args.cell, :2 * args.cell] = False
    mf = model.motion_feature(pv, B)
    torch.cuda.synchronize()

    calls = {"vit": lambda: model.vit_tokens(pv), "vit, empty mask": lambda: model.vit_tokens(pv, patch_drop=none), "vit, one block": lambda: model.vit_tokens(pv, patch_drop=block),
             "vit, half frame": lambda: model.vit_tokens(pv, patch_drop=half), "vit, all but 4x4": lambda: model.vit_tokens(pv, patch_drop=most),
             "step": lambda: model(pixel_values=pv, **text)}

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for fn in calls.values():
        for _ in range(2):
            timed(fn)
    times = {name: [] for name in calls}
    for _ in range(args.blocks):
        for name, fn in calls.items():
            times[name] += [timed(fn)[0] for _ in range(args.steps)]
    med = {n: statistics.median(v) for n, v in times.items()}
    lines = [f"vit_key_drop_cost (library {os.path.relpath(native.LIB_PATH, HERE)}): model {args.model}, {B} clips x {T} frames = {B * T} frames of {G} x {G} patches, "
             f"{B * N} packed tokens ({N} per clip), eager, {args.blocks} alternating blocks x {args.steps} calls per variant",
             f"device: {torch.cuda.get_device_name(0)}"]
    lines += [f"  {n:18s} {med[n]:9.3f} ms/call (min {min(times[n]):.3f}, max {max(times[n]):.3f}, {len(times[n])} calls)" for n in calls]
    for n in list(calls)[1:5]:
        lines.append(f"  {n} - vit {med[n] - med['vit']:+.3f} ms ({100 * (med[n] / med['vit'] - 1):+.2f} %)")
    sweep = lambda: eval_utils.patch_occlusion(model, pixel_values=pv, cell=args.cell, motion_feature=mf, **text)      # noqa: E731
    ms, res = timed(sweep)
    n_pass = 1 + T * n_var
    lines.append(f"  occlusion          {ms:9.1f} ms for one sweep, cell = {args.cell}: {T} masked ViT batches of {B} x {n_var} frames, {n_pass} LLM passes "
                 f"({ms / med['step']:.1f} x step; {n_pass} x step = {n_pass * med['step']:.0f} ms is what re-running the whole step per variant would cost)")
    lines.append(f"  patch_occlusion: occluded {tuple(res['occluded'].shape)}, finite {bool(torch.isfinite(res['occluded']).all())}, control == score1 "
                 f"{bool((res['control'] == res['score1'][:, None]).all())}; largest |delta| of clip 0 (synthetic weights - the shape of the read-out, not a finding): "
                 f"{float(res['delta'][0].abs().max()):.4f}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


def model_tokens(cfg):
    """Visual tokens per frame: (image_size / patch_size)^2 / 4 (pixel-shuffle 0.5)."""
    return (cfg.image_size // cfg.vision_config.patch_size) ** 2 // 4


if __name__ == "__main__":
    main()
