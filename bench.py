#!/usr/bin/env python
"""Headline benchmark: scored clips/s of the stage-2 scoring pass (InternVL2-8B, 8 frames x 448x448 per clip).

    python bench.py --gpus N --steps K --warmup W
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...
     - or plainly `python bench.py --gpus N ...`: the process then starts its N rank processes itself, before anything touches a GPU)

One "step" = one pass of the hot path over one batch of synthetic clips: frames -> InternViT -> pixel-shuffle ->
[all-gather] -> projector (+ motion token) -> InternLM2 pass -> answer-row argmax + score head.  Inputs are resident
in HBM before the timed region.  Workload at N = 1: BASELINE.json configs[1] (batch 4 x 8 frames, 1 MI355X, bf16);
at N > 1 every rank adds its own 4 clips (weak scaling, BASELINE.json configs[2] at N = 8) with the frame-DP
all-gather of visual tokens over RCCL.  Prints ONE JSON line on rank 0.

Inputs of the timed step are bf16 NCHW frames RESIDENT in HBM: no host-to-device copy and no resize / normalise inside the step
(the reference loop copies per clip, stage2_eval.py:919-921); `--ingest` puts both inside (pinned uint8 720p frames -> H2D ->
aigv_op_frame_resize_ingest -> the same step) as a separately reported variant, never the headline `value`.
`--dry-run-cpu` executes the multi-process control flow of this file (process group, barriers, all_reduce(MAX), the lock-step
second pass, the result gather of score_clips_dp) on gloo with a trivial stand-in model: a rehearsal of the N > 1 path on a
machine without GPUs, not a measurement.

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`): nothing else.  `--full` adds
everything else this file measures or checks, all outside the timed region: the presettle steps and the settling batches in front
of it, the host enqueue time and the eager step behind it, then `roofline` (the bf16 MFMA GEMM kernel, 95 % of the FLOPs, timed with
HIP events on the launch stream in a second pass of K steps), `device_calibration`, the greedy-decode and reference-loop figures,
the parity check against the reference's recorded outputs and `cpu_baseline` (the CPU oracle, a torch CPU restatement of the
reference path, timed on this box's host cores on a bounded sample: full-width layers, reduced depth, scaled by layer counts).
`--dump-outputs DIR` writes what the last timed step returned (score1, logit, label) as DIR/<name>.npy; the inputs are seeded, so
two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak, MI355X (MI355X_MICROARCH.md)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(outs, path):
    """--dump-outputs: one DIR/<name>.npy per tensor the step returned (host copies), floating outputs as float32 and integer ones (token ids,
    labels) as float64 - exact either way.  An output larger than its share of DUMP_LIMIT_BYTES is cut to a fixed, seeded sample of its elements."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(1, len(outs))
    for name, t in outs.items():
        a = (t.float() if t.is_floating_point() else t.double()).numpy()
        if a.nbytes > share:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))]
        np.save(os.path.join(path, f"{name}.npy"), a)


def flops_per_clip(cfg, T, N, answer_rows):
    """Algorithmic FLOPs of one scored clip, logits on the answer rows only (SURVEY.md §8d formulas)."""
    v, l = cfg.vision_config, cfg.llm_config
    S = cfg.grid ** 2 + 1
    Hv, Iv, Lv = v.hidden_size, v.intermediate_size, v.num_hidden_layers
    vit = T * (Lv * (8 * S * Hv * Hv + 4 * S * Hv * Iv + 4 * S * S * Hv) + 2 * (S - 1) * (3 * v.patch_size ** 2) * Hv)
    H, I, L = l.hidden_size, l.intermediate_size, l.num_hidden_layers
    ntok = cfg.num_image_token
    proj = ntok * T * (2 * cfg.proj_in * H + 2 * H * H) + 2 * cfg.motion_dim * H + 2 * H * H
    d = l.head_dim
    llm = N * L * (2 * H * (l.num_attention_heads + 2 * l.num_key_value_heads) * d + 2 * H * H + 6 * H * I) \
        + L * 4 * H * N * (N + 1) / 2
    logits = answer_rows * 2 * H * l.vocab_size
    # what the last decoder layer must still do for the consumed rows only (answer rows + the score row): the rows are
    # independent after attention, so the rest of that layer is as dead as the unused logits rows.  `executed` is the work
    # this build runs (row trimming on); `total` stays SURVEY.md's figure, the one `achieved` rates are quoted on.
    rows = answer_rows + 1
    # the closing <|im_end|> of every clip is dead in every layer (nothing consumed attends to it; the reference drops its logits
    # with shift_logits): the build runs N - 1 rows per clip
    Ne = N - 1
    llm_e = Ne * L * (2 * H * (l.num_attention_heads + 2 * l.num_key_value_heads) * d + 2 * H * H + 6 * H * I) + L * 4 * H * Ne * (Ne + 1) / 2
    dead = (Ne - rows) * (2 * H * H + 6 * H * I) + 4 * H * (Ne * (Ne + 1) / 2 - rows * Ne)
    return dict(vit=vit, projector=proj, llm=llm, logits=logits, total=vit + proj + llm + logits,
                executed=vit + proj + llm_e + logits - dead)


def cpu_baseline(cfg, T, N, budget_s=30.0, slowfast=False):
    """Time the CPU oracle on this host: one full-width ViT layer over T frames, one full-width LLM layer over N
    tokens, the lm-head over all N rows (as the reference computes it) and the projector; scale by layer counts."""
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import synth
    from oracle import oracle as O   # the checker, timed as the CPU baseline (never on the product path)
    v, l = cfg.vision_config, cfg.llm_config
    small = pkg.InternVLChatConfig.from_dict(cfg.to_dict())
    small.vision_config.num_hidden_layers = 1
    small.llm_config.num_hidden_layers = 1
    t0 = time.time()
    sd = synth.make_state_dict(small, seed=1, dtype=torch.bfloat16)
    gen_s = time.time() - t0
    g = torch.Generator().manual_seed(0)
    S = cfg.grid ** 2 + 1
    xv = (torch.randn(T, S, v.hidden_size, generator=g) * 0.5).to(torch.bfloat16)
    xl = torch.randn(1, N, l.hidden_size, generator=g).to(torch.bfloat16)
    mask = O.additive_mask(torch.ones(1, N, dtype=torch.bool), N, 0, torch.bfloat16)
    pos = torch.arange(N).unsqueeze(0)
    frames = synth.synthetic_frames(T, cfg.image_size, seed=0)

    def timed(fn, reps=2):
        fn()  # warm
        best = 1e30
        for _ in range(reps):
            t = time.time()
            fn()
            best = min(best, time.time() - t)
        return best

    with torch.no_grad():
        t_vit_layer = timed(lambda: O.vit_layer(sd, small, 0, xv))
        t_llm_layer = timed(lambda: O.llm_layer(sd, small, 0, xl, mask, pos))
        t_embed = timed(lambda: O.vit_embeddings(sd, small, frames), reps=1)
        tok = O.shuffled_tokens(xv, cfg.downsample_ratio)
        t_proj = timed(lambda: O.projector(sd, "mlp1", tok), reps=1)
        t_logits = timed(lambda: O.lm_logits(sd, xl).argmax(-1), reps=1)
    t_sf = 0.0
    if slowfast:   # the motion branch of the same clip (oracle/slowfast.py, bf16 modules as in the reference)
        from oracle import slowfast as OSF
        sf_sd = synth.slowfast_state_dict(seed=1)
        clip = frames.view(1, T, 3, cfg.image_size, cfg.image_size).permute(0, 2, 1, 3, 4)
        with torch.no_grad():
            t_sf = timed(lambda: OSF.slowfast_features(sf_sd, clip), reps=1)
    per_clip = t_vit_layer * v.num_hidden_layers + t_llm_layer * l.num_hidden_layers + t_embed + t_proj + t_logits + t_sf
    # the same two layers in fp32 (the reference's other CPU dtype; on hosts without a bf16 matrix unit it is the FASTER of the two)
    with torch.no_grad():
        sd32 = {k: (t.float() if t.is_floating_point() else t) for k, t in sd.items()}
        mask32 = O.additive_mask(torch.ones(1, N, dtype=torch.bool), N, 0, torch.float32)
        t_vit32 = timed(lambda: O.vit_layer(sd32, small, 0, xv.float()), reps=1)
        t_llm32 = timed(lambda: O.llm_layer(sd32, small, 0, xl.float(), mask32, pos), reps=1)
    per_clip32 = t_vit32 * v.num_hidden_layers + t_llm32 * l.num_hidden_layers + t_embed + t_proj + t_logits + t_sf
    info = host_cpu_info()
    return {
        "value": 1.0 / per_clip, "unit": "clips/s", "cores": torch.get_num_threads(), "kind": "port",
        "cores_note": (f"torch intra-op threads used = {torch.get_num_threads()}; host: {info['model']}, {info['physical_cores']} physical cores / "
                       f"{info['logical_cpus']} logical CPUs visible to this process"),
        "cpu_model": info["model"], "physical_cores": info["physical_cores"], "logical_cpus": info["logical_cpus"],
        "sample": (f"oracle (torch CPU bf16 eager restatement of the reference path), 1 clip: 1 full-width ViT layer x{v.num_hidden_layers} "
                   f"({t_vit_layer:.2f}s each) + 1 full-width LLM layer x{l.num_hidden_layers} ({t_llm_layer:.2f}s each, N={N}) + patch-embed "
                   f"{t_embed:.2f}s + projector {t_proj:.2f}s + lm-head on all rows {t_logits:.2f}s + SlowFast-R50 branch {t_sf:.2f}s; weight gen {gen_s:.0f}s untimed"),
        "s_per_clip": per_clip,
        "fp32": {"value": 1.0 / per_clip32, "s_per_clip": per_clip32,
                 "sample": f"the same layers in fp32: ViT layer {t_vit32:.2f}s, LLM layer {t_llm32:.2f}s (other terms as above)"},
        "oracle_vs_reference": ("wall time of this oracle against the imported reference on one host: profiles/r2_oracle_vs_reference_walltime.txt "
                                "(0.84x bf16 / 0.93x fp32 of the reference's time); the imported reference itself, full depth, in the 8-vCPU AMX build "
                                "container: 34-38 s per bf16 clip, 70 s fp32 (BASELINE.md)"),
    }


def host_cpu_info():
    """CPU model string, physical cores (unique (package, core) pairs of /proc/cpuinfo) and the logical CPUs this process may run on."""
    model, pairs, phys, core = "unknown", set(), None, None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "model name" and model == "unknown":
                    model = v
                elif k == "physical id":
                    phys = v
                elif k == "core id":
                    core = v
                elif not k and phys is not None and core is not None:
                    pairs.add((phys, core)); phys = core = None
        if phys is not None and core is not None:
            pairs.add((phys, core))
    except OSError:
        pass
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return {"model": model, "physical_cores": len(pairs) or logical, "logical_cpus": logical}


def parity_vs_reference(model, cfg, dev):
    """The benched configuration against the REFERENCE itself: tests/golden/e2e_8b_r3.pt holds the outputs of the imported reference
    (CPU eager path, bf16 and fp32) on exactly this batch - 4 clips x 8 frames x 448 px, the seed-0 tokens / frames / motion feature of
    this file - with the golden's seeded weights (make_golden_8b_r3.py); e2e_8b_r3b.pt the same for a second batch of that shape (seed-1
    inputs).  The model takes those weights (generated on the CPU generator, ~1.5 min, outside every timed region), scores each batch
    once and the differences go into the JSON line: the `score D vs ref` half of BASELINE.json's metric.  The top-level keys are the
    BENCHED batch (seed 0); `score_delta_vs_ref_batches` carries both.  Returns None when the fixtures are not there."""
    paths = [os.path.join(ROOT, "tests", "golden", f) for f in ("e2e_8b_r3.pt", "e2e_8b_r3b.pt")]
    if not os.path.exists(paths[0]):
        return None
    from aigv_assessor_amd import synth
    g = torch.load(paths[0], weights_only=True)
    t0 = time.time()
    sd = synth.make_state_dict(cfg, seed=g["w_seed"], rich=True)
    for k, v in g["overrides"].items():
        sd[k] = torch.full_like(sd[k], v)
    model.load_state_dict(sd)
    del sd
    gen_s = time.time() - t0

    # the near-tie bar for level tokens: 1.3 x the largest gap (bf16 ulps of the reference's own logits) by which the REFERENCE's level tokens flip
    # against itself when only the host thread count changes (tests/golden/e2e_8b_r5.pt: 22 of 390 rows flip, largest gap 5.0 -> 6.5); 4 without it
    tie_bar, ref_flips = 4.0, None
    r5_path = os.path.join(ROOT, "tests", "golden", "e2e_8b_r5.pt")
    if os.path.exists(r5_path) and os.path.exists(paths[1]):
        c5 = torch.load(r5_path, weights_only=True)["cases"]
        base = {"batch4/seed0": g["cases"]["batch4/bf16"], "batch4/seed1": torch.load(paths[1], weights_only=True)["cases"]["batch4/bf16"]}
        rows_n, flips, worst = 0, 0, 0.0
        for key, c in c5.items():
            name, tag = key.rsplit("/", 1)
            if tag in ("t1", "t2", "t4") and name in base:
                b = base[name]
                rows_n += int(b["logit"].numel())
                for i in (c["logit"] != b["logit"]).nonzero().flatten().tolist():
                    flips += 1
                    ids_, vals_ = b["top_ids"][i].tolist(), b["top_values"][i].tolist()
                    if int(c["logit"][i]) in ids_:
                        u = 2.0 ** (torch.tensor(abs(vals_[0])).clamp_min(1e-30).log2().floor().item() - 7)
                        worst = max(worst, (vals_[0] - vals_[ids_.index(int(c["logit"][i]))]) / u)
        if flips:
            tie_bar, ref_flips = 1.3 * worst, {"rows": rows_n, "flips": flips, "largest_gap_ulps": worst}

    def one(gold):
        r16, r32 = gold["cases"]["batch4/bf16"], gold["cases"]["batch4/fp32"]
        B, T, seed = r16["B"], r16["T"], r16["seed"]
        toks = synth.canonical_tokens(cfg, B, T, seed=seed)
        model.img_context_token_id = toks["img_context_token_id"]
        out = model(mos=None, pixel_values=synth.synthetic_frames(B * T, cfg.image_size, seed=seed).to(dev), input_ids=toks["input_ids"],
                    attention_mask=toks["attention_mask"], image_flags=torch.ones(B * T, 1, dtype=torch.long), labels=toks["labels"],
                    motion_feature=synth.synthetic_motion(B, cfg.motion_dim, seed=seed).to(dev))
        torch.cuda.synchronize()
        hip = out["score1"].float().cpu()
        b16, f32 = r16["score1"].float(), r32["score1"].float()
        # the 4096-wide hidden state the score head reads (hidden[:, -4]): relative L2 distance - a vector norm, far less noisy than the scalar score
        hid = None
        if "hidden_m4" in r16 and "hidden_m4" in r32:
            rel = lambda a, b: float(((a.float() - b.float()).norm(dim=-1) / b.float().norm(dim=-1)).mean())
            h = model.last_hidden_rows(B).cpu()
            hid = {"hip_vs_ref_bf16": rel(h, r16["hidden_m4"]), "hip_vs_ref_fp32": rel(h, r32["hidden_m4"]), "ref_bf16_vs_ref_fp32": rel(r16["hidden_m4"], r32["hidden_m4"])}
        got = out["logit"].cpu()[r16["answer_rows"]]
        diff = (got != r16["logit"]).nonzero().flatten().tolist()
        outside = 0
        for i in diff:   # a mismatch is a near-tie when the reference's own logits put the HIP token within `tie_bar` bf16 ulps of its maximum
            ids, vals = r16["top_ids"][i].tolist(), r16["top_values"][i].tolist()
            ulp = 2.0 ** (torch.tensor(abs(vals[0])).clamp_min(1e-30).log2().floor().item() - 7)
            if int(got[i]) not in ids or (vals[0] - vals[ids.index(int(got[i]))]) / ulp > tie_bar:
                outside += 1
        return {"seed": seed, "score_delta_vs_ref": float((hip - b16).abs().max()), "score_delta_vs_ref_mean": float((hip - b16).abs().mean()),
                "score_delta_vs_ref_fp32_mean": float((hip - f32).abs().mean()), "ref_bf16_vs_ref_fp32_mean": float((b16 - f32).abs().mean()),
                "level_mismatches": len(diff), "level_mismatches_outside_near_ties": outside, "level_rows": int(got.numel()),
                "level_agreement_with_ref_fp32": {"hip": int((got == r32["logit"]).sum()), "ref_bf16": int((r16["logit"] == r32["logit"]).sum())},
                "hidden_state_rel_l2": hid}
    first = one(g)
    res = dict(first)
    res.pop("seed")
    res["level_near_tie_bar_ulps"] = tie_bar
    if ref_flips:
        res["reference_level_flips_vs_itself"] = ref_flips
    res["score_delta_vs_ref_batches"] = {"seed0_benched": first}
    if os.path.exists(paths[1]):
        res["score_delta_vs_ref_batches"]["seed1"] = one(torch.load(paths[1], weights_only=True))
    self_path = os.path.join(ROOT, "tests", "golden", "e2e_8b_r4_self.pt")
    if os.path.exists(self_path):   # how far the REFERENCE's bf16 pass moves against itself (threads 1 / 4 / 8, alone / in batch): the attainable bar
        res["reference_vs_itself"] = reference_self_spread(torch.load(self_path, weights_only=True))
    r5_path = os.path.join(ROOT, "tests", "golden", "e2e_8b_r5.pt")
    if os.path.exists(r5_path):     # round 5: the same two batches under 1 / 2 / 4 host threads against the recorded 8-thread pass, in bf16 ulps of the score
        c5 = torch.load(r5_path, weights_only=True)["cases"]
        d = []
        for seed, gold in ((0, g), (1, torch.load(paths[1], weights_only=True) if os.path.exists(paths[1]) else None)):
            if gold is None:
                continue
            base = gold["cases"]["batch4/bf16"]["score1"].float()
            for t in (1, 2, 4):
                if f"batch4/seed{seed}/t{t}" in c5:
                    s = c5[f"batch4/seed{seed}/t{t}"]["score1"].float()
                    d += [abs(float(s[i] - base[i])) / 2.0 ** (torch.tensor(abs(float(base[i]))).clamp_min(1e-30).log2().floor().item() - 7) for i in range(len(s))]
        if d:
            res.setdefault("reference_vs_itself", {})
            res["reference_vs_itself"]["benched_shape_threads_1_2_4_vs_8_ulps"] = {"n": len(d), "mean": sum(d) / len(d), "max": max(d)}
            res["reference_vs_itself"]["all_37_clip_sample"] = "profiles/r5_parity_stats.txt: reference against itself 2.56 mean / 8.0 max bf16 ulps over 44 pairs; this path 2.80 mean / 9.0 max over 37 clips"
    res["hidden_state_note"] = ("hidden_state_rel_l2: mean relative L2 distance of hidden[:, -4] (the score head's 4096-wide input) per clip; the reference against ITSELF under other "
                                "host thread counts: 0.0356 (24 clips), this path 0.0390 vs its bf16 pass / 0.0331 vs its fp32 pass over 32 clips (profiles/r6_hidden_distance.txt)")
    res["parity_note"] = ("one pass per recorded batch (4 clips x 8 frames; seed-0 inputs = the benched batch, seed-1 = a second batch of the shape; motion_feature "
                          "input) with the golden's seeded weights against the imported reference's recorded bf16 / fp32 outputs (tests/golden/e2e_8b_r3.pt, "
                          f"e2e_8b_r3b.pt); score1 is a bf16 number (ulp 0.0039 in [0.5, 1)), the reference's own bf16 pass sits {first['ref_bf16_vs_ref_fp32_mean']:.4f} "
                          f"(mean) from its fp32 pass on the benched clips; weight generation {gen_s:.0f} s, untimed")
    return res


def reference_self_spread(g):
    """tests/golden/e2e_8b_r4_self.pt (make_golden_8b_r4.py): the reference's bf16 scores of the SAME clips under 8 / 4 / 1 host threads
    and alone / in a batch of four -> the spread of the reference against itself, in score units and bf16 ulps of [0.5, 1)."""
    c = g["cases"]
    out = {}

    def dmax(a, b):
        return float((a.float() - b.float()).abs().max())
    for seed in (0, 1):
        if f"batch4/seed{seed}/t8" in c and all(f"alone/seed{seed}/clip{i}/t8" in c for i in range(4)):
            alone = torch.cat([c[f"alone/seed{seed}/clip{i}/t8"]["score1"] for i in range(4)])
            out[f"alone_vs_batch_seed{seed}"] = dmax(alone, c[f"batch4/seed{seed}/t8"]["score1"])
    if "alone/seed0/clip0/t1" in c:
        out["threads_1_vs_8_clip0"] = dmax(c["alone/seed0/clip0/t1"]["score1"], c["alone/seed0/clip0/t8"]["score1"])
    if "batch4/seed0/t4" in c:
        out["threads_4_vs_8_batch"] = dmax(c["batch4/seed0/t4"]["score1"], c["batch4/seed0/t8"]["score1"])
        out["threads_4_vs_8_level_changes"] = int((c["batch4/seed0/t4"]["logit"] != c["batch4/seed0/t8"]["logit"]).sum())
    out["bf16_ulp"] = 2.0 ** -8
    return out


def device_calibration(dev):
    """One fixed launch (8192^3 bf16 GEMM, this library's 256x256 kernel, plain store) timed after the run: MI355X devices
    of this pool differ by up to ~12 % on identical MFMA-bound binaries (MI355X_MICROARCH.md, DVFS give-back item 5), so
    numbers from different boxes are only comparable next to this figure.  Not part of `value`."""
    from aigv_assessor_amd import native
    from aigv_assessor_amd.native import ptr
    lib = native.load()
    n = 8192
    A = (torch.randn(n, n, device=dev) * 0.5).to(torch.bfloat16)
    W = (torch.randn(n, n, device=dev) / 90.0).to(torch.bfloat16)
    C = torch.empty(n, n, dtype=torch.bfloat16, device=dev)
    call = lambda: native.check(lib.aigv_op_gemm(ptr(A), n, ptr(W), n, ptr(C), n, None, None, None, 0, None, 0, n, n, n, 0, None))
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        call()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    return {"gemm_8192_cubed_tflops": 2.0 * n ** 3 / (ms * 1e-3) / 1e12, "ms": ms,
            "note": "measured right after the timed steps (chip warm: 1.28-1.35 PFLOP/s seen); the same launch from a cold start reads 1.46-1.68 PFLOP/s depending on the box"}


class _DryRunModel:
    """--dry-run-cpu stand-in: the members score_clips_dp and the timed loop touch, as cheap deterministic functions of the
    inputs (no kernels, no oracle).  Exists to execute THIS FILE's multi-process control flow on a machine without GPUs."""
    stage = 2
    slowfast_model = None

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")

    def vit_tokens(self, pv):
        m = pv.float().mean(dim=(1, 2, 3))
        return m.view(-1, 1, 1).expand(pv.shape[0], self.cfg.num_image_token, self.cfg.proj_in).to(torch.bfloat16).contiguous()

    def motion_feature(self, pv, clips):
        return pv.float().reshape(clips, -1).mean(1, keepdim=True).expand(clips, self.cfg.motion_dim).contiguous()

    def __call__(self, mos=None, pixel_values=None, input_ids=None, attention_mask=None, image_flags=None, labels=None,
                 motion_feature=None, visual_tokens=None):
        B = input_ids.shape[0]
        vt = visual_tokens if visual_tokens is not None else self.vit_tokens(pixel_values)
        mf = motion_feature if motion_feature is not None else self.motion_feature(pixel_values, B)
        score = (vt.float().reshape(B, -1).mean(1) + mf.float().reshape(B, -1).mean(1)).to(torch.bfloat16)
        logit = torch.where(labels[:, 1:] != -100, (input_ids[:, 1:] + 1) % 7, torch.full_like(input_ids[:, 1:], -1)).reshape(-1)
        return {"score1": score, "logit": logit, "label": labels[:, 1:].reshape(-1)}

    def prof_enable(self, on):
        pass


def decode_metric(model, cfg, toks, pv, T, n_short=9, n_long=41, fp8=False):
    """Greedy decode at batch 1 behind clip 0's prompt (generate(): modeling_internvl_chat.py:769-811): ms per new token from the
    difference of two runs (same prefill, 32 more tokens), and the fraction of the 8 TB/s HBM roof the weight stream reaches -
    a decode step reads every decoder weight and the lm-head once."""
    l = cfg.llm_config
    n_prompt = int((toks["labels"][0] == -100).sum())
    ids = toks["input_ids"][:1, :n_prompt].clone()
    ctx_id = toks["img_context_token_id"]
    ids[0, (ids[0] == ctx_id).nonzero()[-1]] = 7          # generate() prompts carry no motion slot: turn it into a text token
    am = torch.ones_like(ids)
    # End-of-sequence checking ON, as in every chat() call of the reference (modeling_internvl_chat.py:612): the id is one that never
    # wins on these weights (the last added special token), so all n tokens are decoded with the device-side EOS bookkeeping and the
    # host's periodic check inside the measurement.
    eos_id = l.vocab_size - 1

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(pixel_values=pv[:T], input_ids=ids, attention_mask=am, max_new_tokens=n, do_sample=False, eos_token_id=eos_id)
        torch.cuda.synchronize()
        assert out.shape[1] == n, f"the end token {eos_id} was generated: pick another id"
        return time.perf_counter() - t0
    run(n_long)                                            # sizes the KV cache (re-creates the context once) and warms up
    t_s = min(run(n_short) for _ in range(3))
    t_l = min(run(n_long) for _ in range(3))
    ms = 1e3 * (t_l - t_s) / (n_long - n_short)
    d = l.head_dim
    per_layer = (l.num_attention_heads + 2 * l.num_key_value_heads) * d * l.hidden_size + l.hidden_size * l.hidden_size + 3 * l.hidden_size * l.intermediate_size
    weight_bytes = 2.0 * (l.num_hidden_layers * per_layer + l.vocab_size * l.hidden_size)
    if fp8:   # fp8 mode: one byte per weight except the post-attention half of the last layer and the lm-head (they stay bf16)
        post = l.hidden_size * l.hidden_size + 3 * l.hidden_size * l.intermediate_size
        weight_bytes = 1.0 * (l.num_hidden_layers * per_layer - post) + 2.0 * (post + l.vocab_size * l.hidden_size)
    kv_bytes = 2.0 * 2 * l.num_hidden_layers * l.num_key_value_heads * d * (n_prompt + (n_short + n_long) / 2)
    return {"decode_ms_per_token": ms, "decode_batch": 1, "decode_prompt_tokens": n_prompt, "decode_eos_checking": True,
            "decode_bytes_per_token": weight_bytes + kv_bytes, "decode_hbm_tb_per_s": (weight_bytes + kv_bytes) / (ms * 1e-3) / 1e12,
            "decode_hbm_frac_of_8tbps": (weight_bytes + kv_bytes) / (ms * 1e-3) / 8.0e12}


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher (N > 1): start the N rank processes - fresh interpreters of this same file with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set, as torch.distributed.run would - and wait for them.  This
    parent never touches a GPU (no HIP call, no torch.cuda.is_available()) and never replaces itself: the ranks are CHILD processes.
    Rank 0's JSON line goes straight to this process's stdout.  Returns the exit code: 0 only if every rank exited 0; the first
    failure ends the others."""
    import socket
    import subprocess
    # the rendezvous port: a free one picked by the kernel.  The socket is closed before the ranks bind it (torch's TCPStore has no way to
    # adopt an open socket): a small window in which another process could take it - rank 0 then fails to listen, exits non-zero, and the
    # loop below ends the others instead of hanging.
    so = socket.socket()
    so.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    deadline = time.time() + float(os.environ.get("AIGV_BENCH_DEADLINE_S", "3000"))   # the whole job; a hung collective must not hang the launcher
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    live = set(range(n))
    kill_at = None          # after a failure: SIGTERM at once, SIGKILL ten seconds later (a rank inside an RCCL collective whose peer died ignores SIGTERM)
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"bench.py: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr)
                for o in live:
                    procs[o].terminate()
                kill_at = time.time() + 10.0
        if rc == 0 and live and time.time() > deadline:
            rc = 124
            print(f"bench.py: ranks {sorted(live)} still running at the deadline; stopping them", file=sys.stderr)
            for o in live:
                procs[o].terminate()
            kill_at = time.time() + 10.0
        if kill_at is not None and live and time.time() > kill_at:
            for o in live:
                procs[o].kill()      # the exact child PIDs this function started
            kill_at = None
        time.sleep(0.2)
    return rc


def reference_loop_metric(model, cfg, toks, dev, T, n_clips=6):
    """The reference's OWN eval-loop shape (stage2_eval.py:908-941: DataLoader batch_size = 1, `.to(device)` per clip, one
    `score1.item()` host synchronisation and the answer-token slice per clip): for every clip, T decoded uint8 720p frames in pinned host
    memory -> H2D -> Pillow-exact resize + normalise on the GPU -> one forward at batch 1 (SlowFast branch inside when the model carries it)
    -> score to the host.  A second, separately labelled number: never the headline `value`."""
    from aigv_assessor_amd import eval_utils
    g8 = torch.Generator().manual_seed(6)
    clips = [torch.randint(0, 256, (T, 720, 1280, 3), dtype=torch.uint8, generator=g8).pin_memory() for _ in range(2)]
    ids, labels, am = toks["input_ids"][:1], toks["labels"][:1], toks["attention_mask"][:1]
    flags = torch.ones(T, 1, dtype=torch.long)
    motion = None if model.slowfast_model is not None else torch.zeros(1, cfg.motion_dim, dtype=torch.bfloat16, device=dev)
    times, scores = [], []
    for i in range(n_clips + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pv = model.ingest_frames(clips[i % 2].to(dev, non_blocking=True))
        out = model(mos=None, pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=flags, labels=labels, motion_feature=motion)
        score = out["score1"].item()
        pred = eval_utils.answer_ids(labels[0], out["logit"].cpu())
        times.append((time.perf_counter() - t0) * 1e3)
        scores.append((score, int(pred.numel())))
    times = sorted(times[2:])
    ms = times[len(times) // 2]
    # the same loop with the NEXT clip's visual front (H2D, resize, InternViT, SlowFast) started one clip ahead on a stream of its own
    # (aigv_assessor_amd.eval_utils.lookahead: a two-line change of the driver; same kernels, same bits) - clip-to-clip wall time
    marks, ahead_scores = [], []
    torch.cuda.synchronize()
    for c, ahead in eval_utils.lookahead([clips[i % 2] for i in range(n_clips + 3)], model, frames=lambda c: c):
        out = model(mos=None, pixel_values=ahead, input_ids=ids, attention_mask=am, image_flags=flags, labels=labels, motion_feature=motion)
        ahead_scores.append(out["score1"].item())
        eval_utils.answer_ids(labels[0], out["logit"].cpu())
        marks.append(time.perf_counter())
    gaps = sorted((b - a) * 1e3 for a, b in zip(marks[2:-1], marks[3:]))
    ahead_ms = gaps[len(gaps) // 2]
    same = all(a == scores[i][0] for i, a in enumerate(ahead_scores[: len(scores)]))
    # the same loop through eval_utils.batched: k = 4 consecutive dataloader items (batch-1 ids / labels / flags, each clip's uint8 720p frames in its
    # own pinned host buffer) scored by ONE forward, the next group's visual front one group ahead, ONE host synchronisation per group
    k, n_groups = 4, 5
    item = lambda i: {"input_ids": ids, "attention_mask": am, "labels": labels, "image_flags": flags[None], "frames": clips[i % 2],
                      **({} if motion is None else {"motion_feature": motion})}
    marks, group_scores = [], []
    torch.cuda.synchronize()
    for j, (_, o) in enumerate(eval_utils.batched((item(i) for i in range(k * (n_groups + 3))), model, k=k, frames=lambda it: it["frames"])):
        group_scores.append(o["score1"].item())
        eval_utils.answer_ids(labels[0], o["logit"])
        if j % k == k - 1:
            marks.append(time.perf_counter())
    bgaps = sorted((b - a) * 1e3 / k for a, b in zip(marks[2:-2], marks[3:-1]))      # (the last two groups come out together: the loop is pipelined two deep)
    batched_ms = bgaps[len(bgaps) // 2]
    bsame = all(a == scores[i % 2][0] for i, a in enumerate(group_scores))
    return {"latency_ms_per_clip": ms, "clips_per_s": 1e3 / ms, "clips_timed": n_clips, "ms_min_max": [times[0], times[-1]],
            "lookahead": {"ms_per_clip": ahead_ms, "clips_per_s": 1e3 / ahead_ms, "ms_min_max": [gaps[0], gaps[-1]], "scores_equal_the_plain_loop": same,
                          "what": "the same loop through eval_utils.lookahead (a two-line change of the driver): the next clip's H2D + resize + InternViT + SlowFast run on their own "
                                  "stream beside the current clip's InternLM2 pass; median clip-to-clip wall time"},
            "batched": {"ms_per_clip": batched_ms, "clips_per_s": 1e3 / batched_ms, "k": k, "ms_min_max": [bgaps[0], bgaps[-1]], "scores_equal_the_plain_loop": bsame,
                        "what": f"the same loop through eval_utils.batched(k = {k}) (a two-line change of the driver): {k} consecutive batch-1 dataloader items - each clip's uint8 720p "
                                "frames in its own pinned host buffer - scored by ONE forward, the next group's H2D + resize + InternViT + SlowFast one group ahead on their own "
                                f"stream, ONE host synchronisation per group; median group-to-group wall time / {k}"},
            "shape": (f"the reference's eval loop (stage2_eval.py:908-941): batch 1, per clip {T} uint8 720p frames from pinned host memory -> H2D -> BICUBIC "
                      "resize + normalise -> forward -> score1.item() + answer-token slice on the host; median of the timed clips after two warm-up clips")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips-per-gpu", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["8b", "26b", "tiny"],
                    help="8b = the headline config; 26b = BASELINE config 4 widths (InternViT-6B + InternLM2-20B; use --frames 16 --clips-per-gpu 1)")
    ap.add_argument("--motion", default="slowfast", choices=["slowfast", "input"],
                    help="slowfast: the SlowFast-R50 branch runs on the frames inside the step, as in the reference's forward; "
                         "input: motion_feature is a resident synthetic [B, 2304] tensor (SURVEY.md 8d)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: the InternLM2 prefill linears on the e4m3 MFMA (BASELINE config 5; NOT the headline - the reference path is bf16)")
    ap.add_argument("--full", action="store_true",
                    help="also run every figure and check outside the headline: presettle + settling, host enqueue, eager step, roofline pass, device "
                         "calibration, decode, reference loop shape, parity with the reference's recorded outputs, CPU baseline (the --no-* options below "
                         "leave single ones out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write what the last timed step returned as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prof", action="store_true", help="skip the per-launch HIP-event roofline measurement")
    ap.add_argument("--all-rows", action="store_true", help="A/B: run every row through the last decoder layer (no row trimming)")
    ap.add_argument("--force-dp", action="store_true", help="variant: route a 1-GPU run through the frame/clip-DP scorer with its RCCL collectives executed on a one-rank group")
    ap.add_argument("--ingest", action="store_true", help="variant: pinned uint8 720p frames -> H2D -> resize + normalise on the GPU inside every step")
    ap.add_argument("--attn-kernel", type=int, default=0, choices=[0, 4, 8],
                    help="A/B: force one form of the prefill-attention kernel (aigv_tune_attention): 4 / 8 waves per workgroup; 0 = default")
    ap.add_argument("--tune-gemm", type=int, default=0, help="A/B: aigv_tune_gemm mode word (kernel choice + 16 * (1 + 256-kernel schedule variant))")
    ap.add_argument("--co-kmax", type=int, default=-1, help="A/B: largest K the co-resident 256x128 GEMM kernel takes (aigv_tune_co_gemm); 0 = never, -1 = the library default")
    ap.add_argument("--serial-motion", action="store_true", help="A/B: run the SlowFast branch on the launch stream in front of the ViT instead of on a side stream beside it")
    ap.add_argument("--attn-numerics", default="fp32", choices=["reference", "fp32"],
                    help="prefill attention: 'fp32' keeps the score matrix in fp32 (default since round 5); 'reference' rounds it to bf16 where the reference's eager path does (A/B)")
    ap.add_argument("--no-graph", action="store_true", help="A/B: launch every kernel of a step from the host (eager) instead of replaying the step's captured HIP graph(s)")
    ap.add_argument("--no-settle", action="store_true", help="skip the untimed settling batches in front of the timed region")
    ap.add_argument("--no-decode", action="store_true", help="skip the greedy-decode measurement appended after the timed region")
    ap.add_argument("--no-parity", action="store_true", help="skip the score / level comparison with the reference's recorded outputs (tests/golden/e2e_8b_r3.pt; ~1.5 min of CPU weight generation)")
    ap.add_argument("--dry-run-cpu", action="store_true", help="rehearse the multi-process control flow on gloo / CPU with a stand-in model (no measurement)")
    ap.add_argument("--dry-run-fault", default="", choices=["", "stuck-peer"],
                    help="with --dry-run-cpu only (tests): 'stuck-peer' = rank 1 exits with code 3 and rank 0 ignores SIGTERM and sleeps, the state of a rank inside a collective whose peer died")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))      # plain `python bench.py --gpus N`: this process only starts and reaps the N ranks
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE {world}")
    dry = args.dry_run_cpu
    if args.dry_run_fault == "stuck-peer" and dry and world > 1:
        if rank == 1:
            raise SystemExit(3)
        import signal
        signal.signal(signal.SIGTERM, signal.SIG_IGN)
        time.sleep(300)
        raise SystemExit(0)
    if args.ingest and world > 1:
        raise SystemExit("--ingest is a single-GPU variant (the per-rank ingest of a frame shard is not wired into score_clips_dp)")
    if dry:
        if world > 1:
            dist.init_process_group("gloo")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback (--dry-run-cpu rehearses the control flow only)")
        if os.environ.get("AIGV_BENCH_SHARE_DEVICE"):   # rehearsal only: every rank on ONE card (a builder's box has a single MI355X); not a measurement
            local_rank = int(os.environ["AIGV_BENCH_SHARE_DEVICE"])
        torch.cuda.set_device(local_rank)
        if args.force_dp and world == 1 and "RANK" not in os.environ:
            # `python bench.py --gpus 1 --force-dp`: a one-rank RCCL group of its own, and the collectives of score_clips_dp run although one
            # rank needs none - the N > 1 code path (all_gather_into_tensor with async work handles, result gathers) on a single MI355X
            import socket
            so = socket.socket(); so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]; so.close()
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        if world > 1 and os.environ.get("AIGV_BENCH_SHARE_DEVICE"):
            # rehearsal only (every rank on ONE card; RCCL refuses duplicate devices): the real model, the real control flow, collectives over gloo
            dist.init_process_group("gloo")
        elif world > 1 or (args.force_dp and "RANK" in os.environ):
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
            if args.force_dp and world == 1:
                from aigv_assessor_amd import dist_utils as _du
                _du.force_single_rank_collectives = True

    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import synth
    from aigv_assessor_amd.dist_utils import score_clips_dp
    from aigv_assessor_amd.modeling import InternVLChatModel

    if dry:
        cfg = pkg.tiny(image_size=56)
    else:
        cfg = pkg.internvl2_8b() if args.model == "8b" else pkg.internvl2_26b() if args.model == "26b" else pkg.tiny(image_size=448)
    T, Bl = args.frames, args.clips_per_gpu
    B = Bl * world
    N = synth.canonical_len(cfg, T)
    dev = torch.device("cpu") if dry else torch.device("cuda", local_rank)

    toks = synth.canonical_tokens(cfg, B, T, seed=0)
    if dry:
        model = _DryRunModel(cfg)
    else:
        model = InternVLChatModel(cfg, device=dev, max_clips=Bl, max_frames=max(Bl * T, (B * T + world - 1) // world),
                                  max_tokens=Bl * N)
        sd = synth.make_state_dict(cfg, seed=0, device=dev, rich=True)
        model.load_state_dict(sd)
        del sd
        model.img_context_token_id = toks["img_context_token_id"]
        model.eval()
        if args.all_rows:
            model.set_row_trimming(False)
        if args.precision == "fp8":
            model.set_precision("fp8")
        if args.attn_numerics != "fp32":
            model.set_attention_numerics(args.attn_numerics)
        if args.attn_kernel:
            from aigv_assessor_amd import native
            native.check(native.load().aigv_tune_attention(args.attn_kernel))
        if args.tune_gemm:
            from aigv_assessor_amd import native
            native.check(native.load().aigv_tune_gemm(args.tune_gemm, 0.0))
        if args.co_kmax >= 0:
            from aigv_assessor_amd import native
            native.check(native.load().aigv_tune_co_gemm(args.co_kmax))
    # inputs resident in HBM before the timed region (token ids are host data in the reference loop; tiny either way)
    # (CPU generator: at N = 1 these are the values tests/golden/e2e_8b_r3.pt was recorded on by the imported reference)
    pv = synth.synthetic_frames(B * T, cfg.image_size, seed=0).to(dev)
    motion = synth.synthetic_motion(B, cfg.motion_dim, seed=0).to(dev) if args.motion == "input" else None
    if args.motion == "slowfast" and not dry:
        from aigv_assessor_amd.slowfast import SlowFastR50
        model.slowfast_model = SlowFastR50(synth.slowfast_state_dict(seed=0))
        if args.serial_motion:
            model.overlap_motion_branch = False
    flags = torch.ones(B * T, 1, dtype=torch.long)
    ids, labels, am = toks["input_ids"], toks["labels"], toks["attention_mask"]
    frames_u8 = None
    if args.ingest and not dry:
        # the variant with the data path inside the step: decoded 720p frames in pinned host memory (what a video decoder hands
        # over) -> one H2D copy -> Pillow-exact BICUBIC resize to the model size + normalise on the GPU (aigv_op_frame_resize_ingest)
        g8 = torch.Generator().manual_seed(5)
        frames_u8 = torch.randint(0, 256, (B * T, 720, 1280, 3), dtype=torch.uint8, generator=g8).pin_memory()

    def step():
        x = pv
        if frames_u8 is not None:
            x = model.ingest_frames(frames_u8.to(dev, non_blocking=True))
        if world == 1 and not args.force_dp:
            return model(mos=None, pixel_values=x, input_ids=ids, attention_mask=am, image_flags=flags, labels=labels,
                         motion_feature=motion)
        return score_clips_dp(model, x, ids, am, flags, labels, motion)

    # scalars that cross ranks (settling decisions, rank times): device tensors over RCCL; host tensors over gloo (the dry run and the
    # one-card rehearsal - gloo has no device all-gather, and its device all-reduce is not relied on)
    cdev = torch.device("cpu") if (dry or (dist.is_initialized() and dist.get_backend() == "gloo")) else dev

    def fence():
        if world > 1:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    # first contact (the driver's 8-GPU run is the only N > 1 run on hardware there is): which device every rank really sits on (UUID + PCI address),
    # gathered through the process group itself and put into the line: N ranks must show N distinct devices
    pg_devices = None
    if dist.is_initialized():
        if dry:
            me = {"rank": rank, "local_rank": local_rank, "device": f"cpu:{os.getpid()}"}
        else:
            pr = torch.cuda.get_device_properties(dev)
            pci = ":".join(str(getattr(pr, a, "?")) for a in ("pci_domain_id", "pci_bus_id", "pci_device_id"))
            me = {"rank": rank, "local_rank": local_rank, "device_index": dev.index, "device": f"{getattr(pr, 'uuid', '')} pci {pci}", "name": pr.name}
        pg_devices = [None] * world
        dist.all_gather_object(pg_devices, me)
        shared = bool(os.environ.get("AIGV_BENCH_SHARE_DEVICE"))
        if len({d["device"] for d in pg_devices}) != world and not shared and rank == 0:
            # recorded and shouted, not fatal: this may be the only N > 1 run there is, and an identity string that does not tell two devices apart (a virtualised
            # UUID) must not cost it - `process_group.distinct_devices` in the line is what the reader checks
            print(f"bench.py: WARNING - {world} ranks report {len({d['device'] for d in pg_devices})} distinct device identities: {pg_devices}", file=sys.stderr)

    # N = 1: the step is captured into a HIP graph (InternVLChatModel.enable_graph_replay: first call eager, second captured, then replayed -
    # one host call per step instead of ~1000 launches; same kernels, same bits).  Three untimed priming steps make sure that the W warm-up
    # steps and everything behind them are replays whatever W is.  The per-launch roofline pass below runs eager (its HIP events are per launch).
    # N > 1 (and --force-dp): the same per rank in two graphs - the front half (ViT shard + SlowFast of the rank's clips) and the projector +
    # InternLM2 half - with the RCCL token all-gather between them launched from the host (score_clips_dp / InternVLChatModel.dp_front).
    graph_mode = (not dry) and not args.no_graph
    if graph_mode:
        model.enable_graph_replay(True)
        for _ in range(3):
            out = step()
    for _ in range(args.warmup):
        out = step()
    import gc
    gc.collect()
    gc.freeze()   # no generation-2 sweep over the (large, static) module graph inside the timed region

    # ---- settling (--full; untimed, reported): some boxes of the pool run their first 10-20 s of GPU work at less than half speed with every kernel at its
    # usual duration (three of ~50 calls of round 3; it decays by itself and the next process is normal).  Batches of 5 more untimed
    # steps until two consecutive batches agree within 3 %, at most 30 s; on a healthy box this is two batches.  The timed region below is untouched:
    # exactly K steps, fenced on both sides; `settle_ms_per_step` lists what the batches read so that nothing is hidden.
    #  a short timed run BEFORE any settling: what `--steps 5 --warmup W` read in rounds 1-2, reported beside the headline
    presettle_ms, settle = None, []
    if args.full:
        fence()
        tp = time.perf_counter()
        for _ in range(min(5, args.steps)):
            out = step()
        fence()
        presettle_ms = (time.perf_counter() - tp) / min(5, args.steps) * 1e3
    if args.full and not args.no_settle:
        t_settle = time.perf_counter()
        while True:
            fence()
            tb = time.perf_counter()
            for _ in range(5):
                out = step()
            fence()
            bt = torch.tensor([(time.perf_counter() - tb) / 5 * 1e3], dtype=torch.float64, device=cdev)
            if world > 1:
                dist.all_reduce(bt, op=dist.ReduceOp.MAX)      # every rank takes the same decision
            settle.append(float(bt.item()))
            stop = torch.tensor([1.0 if (len(settle) >= 2 and abs(settle[-1] - settle[-2]) <= 0.03 * settle[-1]) or time.perf_counter() - t_settle > 30.0 else 0.0],
                                dtype=torch.float64, device=cdev)
            if world > 1:
                dist.all_reduce(stop, op=dist.ReduceOp.MAX)
            if stop.item() > 0:
                break

    # ---- the timed region: exactly K steps, barrier + synchronize on both sides, no instrumentation ----
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    fence()
    dt = time.perf_counter() - t0
    # host copies now: in graph mode the next step overwrites the device buffers behind `out`
    last = {k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v)} if args.dump_outputs and rank == 0 else None
    # host side of a step (--full): how long the launching thread needs to ENQUEUE one step on an idle GPU (no synchronisation inside; the GPU
    # then works through it).  The step is GPU-bound as long as this stays well under ms_per_step; on a contended host it is the first
    # thing to look at (a box of the pool once returned 282 ms/step with every kernel class at its usual duration).
    host_enqueue_ms = None
    if args.full and not dry:
        hs = []
        for _ in range(3):
            fence()
            th = time.perf_counter()
            out = step()
            hs.append((time.perf_counter() - th) * 1e3)
        fence()
        host_enqueue_ms = sorted(hs)[1]
    eager_ms = None
    if args.full and graph_mode:   # the same step launched kernel by kernel from the host, 5 steps, for the record (NOT the headline: `launch` in the line)
        model.enable_graph_replay(False)
        for _ in range(2):
            out = step()
        fence()
        te = time.perf_counter()
        for _ in range(5):
            out = step()
        fence()
        eager_ms = (time.perf_counter() - te) / 5 * 1e3
        model.enable_graph_replay(True)
        for _ in range(3):
            out = step()
        fence()
    # ---- roofline pass: the same K steps again with one HIP-event pair around every GEMM / attention launch on the
    # launch stream.  Kept out of the timed region above because ~900 event records per step cost ~10 % of wall time;
    # the per-launch durations themselves are unaffected (they agree with the rocprofv3 kernel trace in profiles/).
    prof = args.full and rank == 0 and not args.no_prof and not dry
    dt_prof = None
    from aigv_assessor_amd import dist_utils as _dist_utils
    if dist.is_initialized() and args.full and not dry and not args.no_prof and dist.get_backend() == "nccl":
        _dist_utils.collective_timing = []      # this pass only (every rank alike: same schedule): each all-gather completed at once, between two events
    if prof:
        model.prof_enable(True)
        fence()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        fence()
        dt_prof = time.perf_counter() - t1
    elif world > 1 and args.full and not args.no_prof and not dry:
        # keep the ranks in lock-step with rank 0's roofline pass: the SAME sequence of collectives on every rank - fence, K steps, fence.
        # (Until round 4 the other ranks skipped the first fence: rank 0's extra barrier then paired with their first token all-gather and
        # the run hung at N > 1 - found by the one-card two-rank rehearsal, AIGV_BENCH_SHARE_DEVICE; no multi-GPU run had ever executed.)
        fence()
        for _ in range(args.steps):
            out = step()
        fence()
    coll = _dist_utils.read_collective_timing() if _dist_utils.collective_timing is not None else []
    _dist_utils.collective_timing = None
    rank_ms = [1e3 * dt / args.steps]
    if world > 1:
        mine = torch.tensor([dt], dtype=torch.float64, device=cdev)
        every = torch.zeros(world, dtype=torch.float64, device=cdev)
        dist.all_gather_into_tensor(every, mine)
        rank_ms = [1e3 * float(t) / args.steps for t in every.tolist()]
        tmax = mine.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    assert torch.isfinite(out["score1"].float()).all()
    if dry:
        # what the rehearsal can check: every rank ends with the full result, equal to the stand-in applied to all clips at once
        whole = model(mos=None, pixel_values=pv, input_ids=ids, attention_mask=am, image_flags=flags, labels=labels, motion_feature=motion)
        assert torch.equal(out["score1"], whole["score1"]) and torch.equal(out["logit"], whole["logit"]), "data-parallel result differs"

    if rank == 0:
        fl = flops_per_clip(cfg, T, N, answer_rows=10)
        clips_per_s = B * args.steps / dt
        line = {
            "metric": f"scored clips/sec ({T}-frame {cfg.image_size}x{cfg.image_size}, InternVL2-{args.model.upper()} stage-2 score eval)" if not dry else
                      "DRY RUN on CPU / gloo with a stand-in model: control-flow rehearsal, not a measurement", "value": clips_per_s,
            "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16" if args.precision == "bf16" else "fp8 (e4m3 InternLM2 prefill linears, fp32 accumulate; everything else bf16)", "data": "synthetic",
            "config": {"workload": f"InternVL2-{args.model.upper()} stage-2 score eval, {Bl} clips/GPU x {T} frames x {cfg.image_size}px, "
                                   f"N={N} tokens/clip, canonical token layout (SURVEY.md 8d); random-init weights",
                       "motion_branch": "SlowFast-R50 on the frames, inside the step" if args.motion == "slowfast" else "synthetic motion_feature input",
                       "inputs": ("bf16 NCHW frames resident in HBM before the timed region: no H2D copy, no resize / normalise inside the step"
                                  if frames_u8 is None else "pinned uint8 720p frames: H2D copy + BICUBIC resize + normalise INSIDE the step (--ingest variant)"),
                       "attention_numerics": args.attn_numerics,
                       "global_batch_clips": B, "frames_per_clip": T, "tokens_per_clip": N,
                       "parallelism": f"frame/clip-dp{world}" + ((" + RCCL" if not dist.is_initialized() or dist.get_backend() == "nccl" else " + " + dist.get_backend() + " (rehearsal)")
                                                                   + " all-gather of visual tokens" if world > 1 or args.force_dp else "")},
            "slowfast_tflop_per_clip": (model.slowfast_model.flops_per_clip() / 1e12 if args.motion == "slowfast" and not dry else 0.0),   # not in the figures below
            "algorithmic_tflop_per_clip": fl["total"] / 1e12,
            "executed_tflop_per_clip": (fl["total"] if args.all_rows else fl["executed"]) / 1e12,
            "host_enqueue_ms_per_step": host_enqueue_ms,
            "launch": ({"mode": ("HIP graph replay: the step (InternViT, projector, SlowFast side stream, InternLM2, heads: ~1000 launches) captured once, one hipGraphLaunch "
                                 "per step" if world == 1 and not args.force_dp else
                                 "HIP graph replay: per rank two captured graphs per step (InternViT shard + SlowFast | projector + InternLM2 + heads) around the RCCL token "
                                 "all-gather, which the host launches between them") + "; same kernels and bits as the eager step (InternVLChatModel.enable_graph_replay; --no-graph = eager)",
                        "eager_ms_per_step": eager_ms,
                        "eager_note": "--full: the same step with every kernel launched from the host, 5 steps after the timed region; equal on a quiet host, up to 3x slower "
                                      "where the container's CPU quota throttles the launching thread (profiles/r5_graph_replay.txt)"} if graph_mode else
                       {"mode": "eager: every kernel launched from the host"}),
            "ms_per_step_by_rank": rank_ms,
            "process_group": ({"backend": dist.get_backend(), "world_size": dist.get_world_size(), "devices": pg_devices,
                               "distinct_devices": len({d["device"] for d in pg_devices})} if dist.is_initialized() else None),
            "ranks_share_one_device": bool(os.environ.get("AIGV_BENCH_SHARE_DEVICE")),
            "protocol": (f"{args.warmup} warmup steps; "
                         + ((f"{min(5, args.steps)} untimed-but-reported steps (presettle_ms_per_step); "
                             + ("no settling; " if args.no_settle else "untimed settling batches of 5 steps until two agree within 3 %, at most 30 s (settle_ms_per_step); "))
                            if args.full else "")
                         + f"then EXACTLY {args.steps} timed steps between barrier + synchronize fences"),
            "presettle_ms_per_step": presettle_ms,
            "settle_ms_per_step": settle,
            "achieved_tflops_whole_step_per_gpu": (fl["total"] if args.all_rows else fl["executed"]) * B / dt / 1e12 / world * args.steps,
        }
        if prof:
            p = model.prof_read()
            model.prof_enable(False)     # the decode measurement below must not carry the per-launch events
            gm = p["gemm"]
            if gm["launches"]:
                ach = gm["flops"] / (gm["ms"] * 1e-3) / 1e12
                traffic, tnote = None, None
                # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command (scripts/pmc_summary.py); newest round's file first
                tf = next((f for f in (os.path.join(ROOT, "profiles", f"r{r}_gemm_traffic.json") for r in (6, 5, 4, 3, 2, 1)) if os.path.exists(f)), None)
                if tf:
                    tj = json.load(open(tf))
                    traffic = tj["all_gemm"]["traffic_bytes_per_launch"]
                    tnote = (f"NOT measured in this run: a committed constant - L2<->fabric bytes per GEMM launch from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                             f"passes of this command (profiles/{os.path.basename(tf)}, scripts/pmc_summary.py); a PMC pass cannot run inside the timed process")
                # the ceiling this chip SUSTAINS on a bare LDS-fed MFMA loop of the kernel's wave tile (it lowers its clock under MFMA load: 2.5 PF assumes
                # 2.4 GHz): scripts/mfma_lds_probe.hip, re-measured per round on this pool's MI355X class (a committed constant, not measured in this run)
                sp = next((f for f in (os.path.join(ROOT, "profiles", f"r{r}_mfma_lds_probe.json") for r in (6,)) if os.path.exists(f)), None)
                sustained = None
                if sp:
                    sj = json.load(open(sp))
                    sustained = {"value": sj["sustained_peak_tflops"], "unit": "TFLOP/s", "frac": ach / sj["sustained_peak_tflops"], "in_kernel_clock_mhz": sj["in_kernel_clock_mhz"],
                                 "note": f"NOT measured in this run: the bare ds_read_b128 + v_mfma_f32_16x16x32_bf16 loop of the shipped 128x64 wave tile on an MI355X of this pool "
                                         f"(profiles/{os.path.basename(sp)}, scripts/mfma_lds_probe.hip); `frac` above stays achieved / the 2500 TFLOP/s spec peak"}
                line["roofline"] = {
                    "bound": "mfma", "achieved": ach, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_BF16_TFLOPS, "sustained_peak": sustained,
                    "traffic": traffic, "traffic_note": tnote, "algorithmic_bytes_per_launch": gm["bytes"] / gm["launches"],
                    "kernel": "bf16 MFMA GEMM (gemm256_kernel 256x256x64 phase-interleaved + gemm_bf16_kernel 128x128x64 / skinny tails, all epilogues)",
                    "measured": f"HIP events on the launch stream around every launch, second pass of {args.steps} steps ({1e3 * dt_prof / args.steps:.1f} ms/step with the events)",
                    "launches": gm["launches"], "avg_launch_ms": gm["ms"] / gm["launches"],
                    "flops_per_launch": gm["flops"] / gm["launches"], "gemm_ms_per_step": gm["ms"] / args.steps,
                    "other_kernels_ms_per_step": {k: p[k]["ms"] / args.steps for k in ("attn_vit", "attn_llm", "skinny")},
                    "attn_tflops": {k: (p[k]["flops"] / (p[k]["ms"] * 1e-3) / 1e12 if p[k]["ms"] else None) for k in ("attn_vit", "attn_llm")},
                }
                # the same measurement per kernel class, so that the weakest class is visible in the line itself
                def cls(name, label):
                    c = p[name]
                    if not c["launches"] or not c["ms"]:
                        return None
                    a_ = c["flops"] / (c["ms"] * 1e-3) / 1e12
                    return {"kernels": label, "bound": "mfma", "achieved": a_, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": a_ / PEAK_BF16_TFLOPS,
                            "ms_per_step": c["ms"] / args.steps, "launches_per_step": c["launches"] / args.steps}
                line["roofline_by_class"] = {
                    "gemm_llm": cls("gemm_llm", "InternLM2 linears (wqkv, wo, w1|w3 + SwiGLU, w2; K = 4096 / 14336)"),
                    "gemm_vit": cls("gemm_vit", "InternViT linears + mlp1 projector (qkv, proj, fc1 + GELU, fc2; K = 1024 / 4096)"),
                    "attn_vit": cls("attn_vit", "InternViT attention (non-causal, d = 64, 1025 rows per frame)"),
                    "attn_llm": cls("attn_llm", "InternLM2 prefill attention (causal GQA, d = 128)"),
                }
        if coll:   # the RCCL token all-gather as rank 0 saw it in the roofline pass (completed at once there; overlapped in the timed steps)
            big = max(n for n, _ in coll)
            ms_ = sorted(t for n, t in coll if n == big)
            med = ms_[len(ms_) // 2]
            line["token_all_gather"] = {"gathered_bytes": big, "launches": len(ms_), "ms_median": med, "ms_min_max": [ms_[0], ms_[-1]],
                                        "GB_per_s_received_per_rank": big * (world - 1) / max(world, 1) / (med * 1e-3) / 1e9 if world > 1 else None,
                                        "note": "all_gather_into_tensor of the pre-projector visual tokens, issue -> completion between two events on the compute stream, "
                                                "roofline pass only (there it is waited for at once; in the timed steps it overlaps the InternLM2 pass where the clip split allows)"}
        if prof and args.precision == "fp8":
            g8 = p["gemm_fp8"]   # (prof_read consumes the records: `p` is the one read of this run)
            if g8["launches"]:
                a8 = g8["flops"] / (g8["ms"] * 1e-3) / 1e12
                line["roofline_fp8"] = {"bound": "mfma", "achieved": a8, "peak": 5000.0, "unit": "TFLOP/s", "frac": a8 / 5000.0, "launches": g8["launches"],
                                        "gemm_ms_per_step": g8["ms"] / args.steps,
                                        "kernel": "gemm256_kernel<EPI, 7, FP8> (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales); activation quantisation passes not included"}
        if prof:
            line["device_calibration"] = device_calibration(dev)
        if dry:
            line["dry_run"] = True
        if args.full and world == 1 and not dry and not args.no_decode and args.model == "8b":
            dm = decode_metric(model, cfg, toks, pv, T, fp8=args.precision == "fp8")
            line.update(dm)
            if "roofline_by_class" in line:
                line["roofline_by_class"]["decode"] = {"kernels": "generate(): q_len = 1 GEMVs + split-KV attention, batch 1", "bound": "hbm",
                                                       "achieved": dm["decode_hbm_tb_per_s"] * 1e3, "peak": 8000.0, "unit": "GB/s",
                                                       "frac": dm["decode_hbm_frac_of_8tbps"], "ms_per_token": dm["decode_ms_per_token"]}
        if args.full and world == 1 and not dry and not args.no_decode and not args.ingest:
            line["reference_loop_shape"] = reference_loop_metric(model, cfg, toks, dev, T)
        if (args.full and world == 1 and not dry and not args.no_parity and args.model == "8b" and args.precision == "bf16" and T == 8 and Bl == 4
                and not args.all_rows and not args.tune_gemm and not args.attn_kernel and args.attn_numerics == "fp32"):
            par = parity_vs_reference(model, cfg, dev)      # (replaces the model's weights: after every measurement)
            if par:
                line.update(par)
        if args.full and world == 1 and not dry and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(cfg, T, N, slowfast=args.motion == "slowfast")
            line["gpu_over_cpu"] = clips_per_s / line["cpu_baseline"]["value"]
        if last is not None:
            dump_outputs(last, args.dump_outputs)
        print(json.dumps(line))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
