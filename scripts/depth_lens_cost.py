"""What ``forward(return_depth_lens=True)`` costs at the headline shape (InternVL2-8B sizes, 4 clips x 8 frames, synthetic weights - bench.py's
step without its visual front), eager, in ONE process on one box, the variants alternating block by block so that drift hits all of them;
medians over the blocks' per-call times (device-synchronised host clock around every call) - the method of scripts/key_drop_cost.py:

  llm               forward(visual_tokens=..., motion_feature=...)            projector + InternLM2 + heads, unarmed: what the armed pass is compared with
  llm, lens         the same with return_depth_lens=True                       + one tap launch per depth (L + 1), the grouped score head over every depth's
                                                                                score rows, the lm-head read-out of the (L + 1) x clips token rows, 64 at a time
  llm, cand         the unarmed pass with candidate_ids (five ids)
  llm, cand, lens   the armed pass with them: + the candidates' columns at every depth, from the same logits

No bar is set: the read-out is opt-in; the figures are recorded.
Usage: python scripts/depth_lens_cost.py [--steps 10] [--blocks 5] [--model 8b|tiny] [--out profiles/depth_lens_cost.txt]"""
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
    from aigv_assessor_amd import eval_utils, native, synth
    from aigv_assessor_amd.modeling import InternVLChatModel
    if not torch.cuda.is_available():
        raise SystemExit("depth_lens_cost.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.tiny(image_size=448)
    B, T = args.clips, args.frames
    N = synth.canonical_len(cfg, T)
    L = cfg.llm_config.num_hidden_layers
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
    cand = torch.tensor([11, 222, 3333, 4444, 5555], device=dev) % cfg.llm_config.vocab_size
    calls = {"llm": lambda: model(**kw), "llm, lens": lambda: model(**kw, return_depth_lens=True),
             "llm, cand": lambda: model(**kw, candidate_ids=cand), "llm, cand, lens": lambda: model(**kw, candidate_ids=cand, return_depth_lens=True)}

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
    out = timed(calls["llm, cand, lens"])[1]
    same = bool(torch.equal(out["lens_score"][:, L].to(torch.bfloat16).view(torch.int16), out["score1"].view(torch.int16)))
    lines = [f"depth_lens_cost (library {os.path.relpath(native.LIB_PATH, HERE)}): model {args.model}, {B} clips x {T} frames, {B * N} packed tokens ({N} per clip), "
             f"{L} layers: {L + 1} tap launches, {(L + 1) * B} score rows and {(L + 1) * B} token rows per armed pass; eager, {args.blocks} alternating blocks x {args.steps} "
             f"calls per variant", f"device: {torch.cuda.get_device_name(0)}"]
    lines += [f"  {n:18s} {med[n]:9.3f} ms/call (min {min(times[n]):.3f}, max {max(times[n]):.3f}, {len(times[n])} calls)" for n in calls]
    lines.append(f"  llm, lens - llm             {med['llm, lens'] - med['llm']:+.3f} ms ({100 * (med['llm, lens'] / med['llm'] - 1):+.2f} %)")
    lines.append(f"  llm, cand, lens - llm, cand {med['llm, cand, lens'] - med['llm, cand']:+.3f} ms ({100 * (med['llm, cand, lens'] / med['llm, cand'] - 1):+.2f} %)")
    lines.append(f"  lens_score[:, L] is score1 bit for bit: {same}; settling depth of the clips at tol 0.01 (synthetic weights - the shape of the read-out, not a finding): "
                 f"{eval_utils.settling_depth(out['lens_score'], 0.01).tolist()}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
