"""Child process of tests/test_gpu_topk_logprob.py (not a test module): ``score_clips_dp(top_logprobs=k)`` over RCCL on ONE MI355X,
as tests/rccl_single_rank_child.py runs the plain scorer - a fresh process with WORLD_SIZE = 1 and the collectives forced - against
``forward(top_logprobs=k)`` of the same model, eager and under graph replay.  Prints TOPK_DP_OK on success."""
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch
    import torch.distributed as dist
    import aigv_assessor_amd as pkg
    from aigv_assessor_amd import dist_utils, synth
    from aigv_assessor_amd.modeling import InternVLChatModel

    dist_utils.init_dist("pytorch", backend="nccl")
    dev = torch.device("cuda", torch.cuda.current_device())
    dist_utils.force_single_rank_collectives = True
    cfg = pkg.tiny(image_size=224, vit_layers=1, llm_layers=2)
    model = InternVLChatModel(cfg)
    model.load_state_dict(synth.make_state_dict(cfg, seed=71, rich=True))
    model.eval().cuda()
    B, T = 3, 2
    toks = synth.canonical_tokens(cfg, B, T, seed=71)
    model.img_context_token_id = toks["img_context_token_id"]
    pv = synth.synthetic_frames(B * T, 224, seed=71).to(dev)
    motion = synth.synthetic_motion(B, cfg.motion_dim, seed=71).to(dev)
    flags = torch.ones(B * T, 1, dtype=torch.long)
    K = 5
    bits = lambda t: t.detach().float().cpu().contiguous().view(torch.int32)
    want = model(pixel_values=pv, input_ids=toks["input_ids"], attention_mask=toks["attention_mask"], image_flags=flags, labels=toks["labels"],
                 motion_feature=motion, top_logprobs=K, return_logprobs=True)
    args = (model, pv, toks["input_ids"], toks["attention_mask"], flags, toks["labels"], motion)
    assert "top_ids" not in dist_utils.score_clips_dp(*args)
    runs = [dist_utils.score_clips_dp(*args, top_logprobs=K), dist_utils.score_clips_dp(*args, top_logprobs=K, return_logprobs=True, prefer_gathered=True)]
    model.enable_graph_replay(True)
    runs += [dist_utils.score_clips_dp(*args, top_logprobs=K) for _ in range(3)]
    model.enable_graph_replay(False)
    torch.cuda.synchronize()
    for got in runs:
        assert got["top_ids"].shape == want["top_ids"].shape == (B * (toks["input_ids"].shape[1] - 1), K) and got["top_ids"].dtype == torch.long
        assert torch.equal(got["top_ids"], want["top_ids"]) and torch.equal(bits(got["top_logprob"]), bits(want["top_logprob"]))
        assert torch.equal(got["logit"], want["logit"]) and torch.equal(got["score1"], want["score1"])
    assert torch.equal(bits(runs[1]["logprob"]), bits(want["logprob"]))
    dist.barrier()
    dist.destroy_process_group()
    print("TOPK_DP_OK")


if __name__ == "__main__":
    main()
