"""What activation patching costs at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames, synthetic weights - bench.py's step without its
visual front), eager, in ONE process on one box, the variants alternating block by block so that drift hits all of them; medians over the
blocks' per-call times (device-synchronised host clock around every call) - the method of scripts/depth_lens_cost.py:

  llm                 forward(visual_tokens=..., motion_feature=...)                 projector + InternLM2 + heads, unarmed: what the armed passes are compared with
  llm, capture        the same with return_stream=<every frame token>                + one row-copy launch per layer: the frame rows of every clip at all L depths
  llm, patch 4        the same with stream_patch over four middle layers             + one row-copy launch in front of each of the four layers, the frame rows of
                                                                                       every clip overwritten (with the rows a capture returned: the pass's own)

No bar is set: both are opt-in; the figures are recorded.
Usage: python scripts/stream_patch_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--out profiles/stream_patch_cost.txt]"""
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
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.readouts import StreamPatch
    if not torch.cuda.is_available():
        raise SystemExit("stream_patch_cost.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.tiny(image_size=448)
    B, T = args.clips, args.frames
    N = synth.canonical_len(cfg, T)
    L, H = cfg.llm_config.num_hidden_layers, cfg.llm_config.hidden_size
    toks = synth.canonical_tokens(cfg, B, T, seed=0)
    model = InternVLChatModel(cfg, device=dev, max_clips=B, max_frames=B * T, max_tokens=B * N)
    model.load_state_dict(synth.make_state_dict(cfg, seed=0, device=dev, rich=True))
    model.img_context_token_id = toks["img_context_token_id"]
    model.eval()
    pv = synth.synthetic_frames(B * T, cfg.image_size, seed=0).to(dev)
    flags = torch.ones(B * T, 1, dtype=torch.long)
    tokens = model.vit_tokens(pv)
    mf = synth.synthetic_motion(B, cfg.motion_dim, seed=0).to(dev)
    torch.cuda.synchronize()
    kw = dict(input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags, labels=toks["labels"], visual_tokens=tokens, motion_feature=mf)
    frames = model.segment_masks(toks["input_ids"], toks["attention_mask"], flags)["frames"]
    lo = max(0, L // 2 - 2)
    window = (lo, min(L, lo + 4))
    base = model(**kw, return_stream=frames)
    n = int(base["stream_index"].shape[0])
    patch = StreamPatch(frames, base["stream"][:, window[0]:window[1]].contiguous(), window, base["stream_index"])
    score1 = base["score1"].clone()
    del base
    torch.cuda.synchronize()
    calls = {"llm": lambda: model(**kw), "llm, capture": lambda: model(**kw, return_stream=frames), "llm, patch 4": lambda: model(**kw, stream_patch=patch)}

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
    med = {name: statistics.median(v) for name, v in times.items()}
    neutral = bool(torch.equal(timed(calls["llm, patch 4"])[1]["score1"].view(torch.int16), score1.view(torch.int16)))
    gb = lambda depths: n * depths * H * 2 / 1e9
    lines = [f"stream_patch_cost (library {os.path.relpath(native.LIB_PATH, HERE)}): model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), "
             f"{L} layers; {n} frame rows: the capture copies {n} x {L} rows ({gb(L):.3f} GB) in {L} launches, the patch over layers [{window[0]}, {window[1]}) writes "
             f"{n} x {window[1] - window[0]} rows ({gb(window[1] - window[0]):.3f} GB) in {window[1] - window[0]} launches; eager, {args.blocks} alternating blocks x "
             f"{args.steps} calls per variant", f"device: {torch.cuda.get_device_name(0)}"]
    lines += [f"  {name:14s} {med[name]:9.3f} ms/call (min {min(times[name]):.3f}, max {max(times[name]):.3f}, {len(times[name])} calls)" for name in calls]
    for name in ("llm, capture", "llm, patch 4"):
        lines.append(f"  {name} - llm  {med[name] - med['llm']:+.3f} ms ({100 * (med[name] / med['llm'] - 1):+.2f} %)")
    lines.append(f"  the self-patch leaves score1 bit for bit: {neutral}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
