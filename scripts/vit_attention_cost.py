"""What ``model.vit_attention`` (csrc/vitmap.hip) costs at the benched shape: 32 frames of 448 x 448 through the InternViT-300M of the 8B sizes
(24 layers, 16 heads of 64, S = 1025; synthetic weights; the LLM cut to one layer - it plays no part), in one process on one box.

* ``vit_tokens``: the unarmed pass - the code path of the tree before the map existed.  ``--root DIR`` imports the package from another checkout
  (its library already built), so the same command times the parent commit's ``vit_tokens``; alternate the two trees call by call;
* ``--maps`` (this tree only): ``vit_attention`` over all layers, head mean (3.2 GB of maps); per head over a 4-layer window (8.6 GB); one layer,
  head mean; and ``vit_tokens`` once more behind them.  Device events around every call, medians, minima and maxima; the output tensors are
  allocated inside the timed call (the caching allocator hands the same block back after the warm-up).

Usage: python scripts/vit_attention_cost.py [--root DIR] [--maps] [--frames 32]      (prints one ``COST {json}`` line; needs an MI355X)."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--maps", action="store_true")
ap.add_argument("--frames", type=int, default=32)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch                                   # noqa: E402
import aigv_assessor_amd as pkg               # noqa: E402
from aigv_assessor_amd import synth           # noqa: E402
from aigv_assessor_amd.modeling import InternVLChatModel   # noqa: E402

assert torch.cuda.is_available(), "needs an MI355X"
cfg = pkg.internvl2_8b()
cfg.llm_config.num_hidden_layers = 1
model = InternVLChatModel(cfg, stage=2)
model.load_state_dict(synth.make_state_dict(cfg, seed=0, device=torch.device("cuda"), rich=True))
model = model.eval().cuda()
pv = synth.synthetic_frames(args.frames, 448, seed=1).cuda().to(torch.bfloat16)


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3), reps=reps)


L = cfg.vision_config.num_hidden_layers
out = dict(root=args.root, frames=args.frames, layers=L, vit_tokens_ms=timed(lambda: model.vit_tokens(pv)))
if args.maps:
    out["vit_attention_all_layers_head_mean_ms"] = timed(lambda: model.vit_attention(pv), reps=5, warm=2)
    out["vit_attention_4_layers_per_head_ms"] = timed(lambda: model.vit_attention(pv, layers=(L - 4, L), per_head=True), reps=5, warm=2)
    out["vit_attention_1_layer_head_mean_ms"] = timed(lambda: model.vit_attention(pv, layers=(L - 1, L)), reps=5, warm=2)
    out["vit_tokens_after_ms"] = timed(lambda: model.vit_tokens(pv))
    a = model.vit_attention(pv, layers=(0, 1))
    assert torch.equal(a["tokens"], model.vit_tokens(pv))
    out["worst_row_sum_error"] = float((a["vit_attention"].double().sum(-1) - 1).abs().max())
print("COST " + json.dumps(out), flush=True)
