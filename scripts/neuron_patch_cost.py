"""What MLP neuron knock-out and neuron patching cost at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames, synthetic weights - bench.py's
step without its visual front), eager, in ONE process on one box, the variants alternating block by block so that drift hits all of them; medians
over the blocks' per-call times (device-synchronised host clock around every call) - the method of scripts/head_patch_cost.py:

  llm                   forward(visual_tokens=..., motion_feature=...)                 projector + InternLM2 + heads, unarmed: what the armed passes are compared with
  llm, dense score      the same with return_neurons=<the score rows>                  + one dense neuron-rows launch per layer, one row per clip, I columns each
  llm, sparse frames    the same with return_neurons=<every frame row>, 16 neuron_ids  + one sparse neuron-rows launch per layer, every frame row, 16 columns each
  llm, MLP knock-out    the same with neuron_scale: one middle layer's MLP x 0         + one dense neuron-rows launch in that layer, every row
  llm, neuron knock-out the same with neuron_scale: one neuron of that layer x 0       + one sparse neuron-rows launch in that layer, every row, one column

and, with --sweep, the wall time of one full eval_utils.mlp_knockout (L passes + the base pass) for the batch.  No bar is set on the armed figures:
they are opt-in and are recorded against the unarmed pass's own min..max.
Usage: python scripts/neuron_patch_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--sweep] [--out profiles/neuron_patch_cost.txt]"""
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
    ap.add_argument("--sweep", action="store_true", help="also time one full mlp_knockout sweep")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, HERE)

    import torch
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import eval_utils, native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    from aigv_assessor_amd.readouts import NeuronScale
    if not torch.cuda.is_available():
        raise SystemExit("neuron_patch_cost.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.tiny(image_size=448)
    B, T = args.clips, args.frames
    N = synth.canonical_len(cfg, T)
    L, I = cfg.llm_config.num_hidden_layers, cfg.llm_config.intermediate_size
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
    seg = model.segment_masks(toks["input_ids"], toks["attention_mask"], flags)
    ids = torch.arange(16) * (I // 16) + 3
    mid = L // 2
    block = torch.ones(L)
    block[mid] = 0.0
    mlp, neuron = NeuronScale(block), NeuronScale(torch.zeros(1), torch.tensor([[mid, I // 2]]))
    base = model(**kw)
    score1 = base["score1"].clone()
    n_frames = int(model(**kw, return_neurons=seg["frames"], neuron_layers=(0, 1), neuron_ids=ids)["neurons_index"].shape[0])
    torch.cuda.synchronize()
    calls = {"llm": lambda: model(**kw), "llm, dense score": lambda: model(**kw, return_neurons=seg["score_row"]),
             "llm, sparse frames": lambda: model(**kw, return_neurons=seg["frames"], neuron_ids=ids), "llm, MLP knock-out": lambda: model(**kw, neuron_scale=mlp),
             "llm, neuron knock-out": lambda: model(**kw, neuron_scale=neuron)}

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
    neutral = all(bool(torch.equal(timed(calls[name])[1]["score1"].view(torch.int16), score1.view(torch.int16))) for name in ("llm, dense score", "llm, sparse frames"))
    moved = not torch.equal(timed(calls["llm, MLP knock-out"])[1]["score1"].view(torch.int16), score1.view(torch.int16))
    lines = [f"neuron_patch_cost (library {os.path.relpath(native.LIB_PATH, HERE)}): model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), "
             f"{L} layers, I = {I}; the dense capture copies {B} score rows x {L} layers x {I} ({B * L * I * 2 / 1e6:.2f} MB) in {L} launches, the sparse one 16 neurons of "
             f"{n_frames} frame rows x {L} layers ({n_frames * L * 16 * 2 / 1e6:.2f} MB; dense it would be {n_frames * L * I * 2 / 1e9:.2f} GB) in {L} launches, the MLP knock-out "
             f"scales layer {mid} over every row in 1 launch, the neuron knock-out neuron {I // 2} of it; eager, {args.blocks} alternating blocks x {args.steps} calls per variant",
             f"device: {torch.cuda.get_device_name(0)}"]
    lines += [f"  {name:22s} {med[name]:9.3f} ms/call (min {min(times[name]):.3f}, max {max(times[name]):.3f}, {len(times[name])} calls)" for name in calls]
    for name in list(calls)[1:]:
        lines.append(f"  {name} - llm  {med[name] - med['llm']:+.3f} ms ({100 * (med[name] / med['llm'] - 1):+.2f} %); the unarmed pass's own spread: "
                     f"{min(times['llm']) - med['llm']:+.3f} .. {max(times['llm']) - med['llm']:+.3f} ms")
    lines.append(f"  the captures leave score1 bit for bit: {neutral}; the MLP knock-out moves it: {moved}")
    if args.sweep:
        t0 = time.perf_counter()
        res = eval_utils.mlp_knockout(model, pixel_values=pv, input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags, labels=toks["labels"],
                                      motion_feature=mf)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append(f"  eval_utils.mlp_knockout, every layer: {len(res['outs'])} passes (InternViT once) in {dt:.1f} s = {1e3 * dt / len(res['outs']):.1f} ms per pass; "
                     f"delta of {tuple(res['delta'].shape)}, largest |delta| {res['delta'].abs().max().item():.4f}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
