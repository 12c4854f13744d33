"""What ``forward(key_drop=...)`` and ``eval_utils.frame_ablation`` cost at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames,
SlowFast motion branch, synthetic weights - bench.py's step), eager, in ONE process on one box, the variants alternating block by block so
that drift hits all of them; medians over the blocks' per-call times (device-synchronised host clock around every call):

  step              forward(pixel_values=...)                                  the whole unmasked step (ViT, SlowFast, projector, InternLM2, heads)
  llm               forward(visual_tokens=..., motion_feature=...)             projector + InternLM2 + heads, unmasked: what a masked pass is compared with
  llm, frame 0 off  the same with key_drop = unit_masks[:, 0]                  one frame (256 tokens) of every clip hidden
  llm, frames->text the same with key_drop = segment_masks["frames"],           the row-selective form in all layers: the text behind the frames cannot
                    key_drop_rows = segment_masks["text_after"]                read them (every frame token a dropped key, mixed and unselected waves)
  ablation          eval_utils.frame_ablation (8 frames: 10 passes, ViT once)  next to 10 x step, what the loop would cost without the helper

``--variant-lib PATH`` repeats the two llm variants in a child process on another build of the library (``AIGV_AMD_LIB``; the diagnostic
build with -DAIGV_ATTN_DROP_NO_SKIP, made by ``--build-no-skip PATH`` on a machine with hipcc): the A/B that prices the whole-tile skip.
No bar is set for any of these: they are recorded.
Usage: python scripts/key_drop_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--variant-lib PATH] [--out profiles/key_drop_cost.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_no_skip(out):
    """attention.hip with -DAIGV_ATTN_DROP_NO_SKIP, linked with the tree's other objects into `out` (needs the tree built)."""
    sys.path.insert(0, os.path.join(HERE, "aigv-assessor_amd"))
    import build as b
    b.build()
    obj = out + ".attention.o"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + b.FLAGS + b.EXTRA_FLAGS["attention.hip"] + ["-DAIGV_ATTN_DROP_NO_SKIP", "-c", os.path.join(b.CSRC, "attention.hip"), "-o", obj], check=True)
    objs = [obj if s == "attention.hip" else b._obj(s) for s in b.SOURCES]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs, check=True)
    os.remove(obj)
    print(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed calls per block (the ablation: a fifth of it)")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "tiny"])
    ap.add_argument("--llm-only", action="store_true", help="the llm variants alone (the child process of --variant-lib)")
    ap.add_argument("--variant-lib", default="", help="also measure the two llm variants on this build of the library (child process, same box)")
    ap.add_argument("--build-no-skip", default="", metavar="PATH", help="build the no-skip diagnostic library to PATH and exit (no GPU needed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.build_no_skip:
        return build_no_skip(os.path.abspath(args.build_no_skip))
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import eval_utils, native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.slowfast import SlowFastR50
    if not torch.cuda.is_available():
        raise SystemExit("key_drop_cost.py measures on the GPU: no device, no number")
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
    text = dict(input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags, labels=toks["labels"])
    units = model.unit_masks(text["input_ids"], text["attention_mask"], flags)
    tokens = model.vit_tokens(pv)
    mf = model.motion_feature(pv, B)
    torch.cuda.synchronize()
    llm_kw = dict(text, visual_tokens=tokens, motion_feature=mf)

    seg = model.segment_masks(text["input_ids"], text["attention_mask"], flags)
    calls = {"llm": lambda: model(**llm_kw), "llm, frame 0 off": lambda: model(**llm_kw, key_drop=units[:, 0]),
             "llm, frames->text": lambda: model(**llm_kw, key_drop=seg["frames"], key_drop_rows=seg["text_after"])}
    if not args.llm_only:
        calls = dict({"step": lambda: model(pixel_values=pv, **text)}, **calls,
                     ablation=lambda: eval_utils.frame_ablation(model, pixel_values=pv, **text))
    reps = {name: max(1, args.steps // 5) if name == "ablation" else args.steps for name in calls}

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
            times[name] += [timed(fn)[0] for _ in range(reps[name])]
    med = {n: statistics.median(v) for n, v in times.items()}
    lines = [f"key_drop_cost (library {os.path.relpath(native.LIB_PATH, HERE)}): model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), eager, "
             f"{args.blocks} alternating blocks x {args.steps} calls per variant ({reps.get('ablation', 0)} for the ablation)",
             f"device: {torch.cuda.get_device_name(0)}"]
    lines += [f"  {n:18s} {med[n]:9.3f} ms/call (min {min(times[n]):.3f}, max {max(times[n]):.3f}, {len(times[n])} calls)" for n in calls]
    lines.append(f"  llm, frame 0 off - llm {med['llm, frame 0 off'] - med['llm']:+.3f} ms ({100 * (med['llm, frame 0 off'] / med['llm'] - 1):+.2f} %); "
                 f"dropped tokens per clip: {int(units[0, 0].sum())} of {N}")
    lines.append(f"  llm, frames->text - llm {med['llm, frames->text'] - med['llm']:+.3f} ms ({100 * (med['llm, frames->text'] / med['llm'] - 1):+.2f} %); "
                 f"dropped keys per clip: {int(seg['frames'][0].sum())}, selected rows per clip: {int(seg['text_after'][0].sum())} of {N}, all layers")
    if not args.llm_only:
        lines.append(f"  ablation / step {med['ablation'] / med['step']:.2f} ({T + 2} passes; {T + 2} x step = {(T + 2) * med['step']:.1f} ms)")
        res = timed(calls["ablation"])[1]
        lines.append(f"  frame_ablation: ablated {tuple(res['ablated'].shape)}, finite {bool(torch.isfinite(res['ablated']).all())}; delta of clip 0 (synthetic weights - the shape "
                     f"of the read-out, not a finding): {[round(float(x), 4) for x in res['delta'][0]]}")
    if args.variant_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--llm-only", "--steps", str(args.steps), "--blocks", str(args.blocks), "--clips", str(B), "--frames", str(T),
               "--model", args.model]
        try:        # (a limit of its own: a hung child must not hang the job)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240 + 2 * args.blocks * args.steps, env=dict(os.environ, AIGV_AMD_LIB=os.path.abspath(args.variant_lib)))
            lines += ([f"variant library: the child process failed ({r.returncode}): {r.stderr[-400:]}"] if r.returncode else
                      ["variant library, same box, same session (child process):"] + ["  " + l for l in r.stdout.strip().splitlines()])
        except subprocess.TimeoutExpired:
            lines.append("variant library: the child process ran into its time limit and was ended: no figure")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
