"""Checkpoint loading of ``InternVLChatModel`` and the parameter containers that give its weights the reference's module paths."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .config import InternVLChatConfig
from .context import resized_pos_table


# ------------------------------------------------------------------------------------------------------
# parameter containers with the reference's module paths (so state_dict keys match §8a row W)
# ------------------------------------------------------------------------------------------------------
class _Node(nn.Module):
    """Parameter holder; children are added under their reference names."""

    def __len__(self):
        return len(self._modules)

    def __iter__(self):
        return iter(self._modules.values())

    def __getitem__(self, i):
        return self._modules[str(i)]


class _VisionModel(_Node):
    """``model.vision_model`` surface used by the drivers (modeling_intern_vit.py:297-323)."""

    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)

    def resize_pos_embeddings(self, old_size, new_size, patch_size):
        # modeling_intern_vit.py:309-319 (weight surgery, host side)
        emb = self.embeddings
        pos = emb.position_embedding.data
        new = resized_pos_table(pos, old_size // patch_size, new_size // patch_size).to(pos.device)
        emb.position_embedding = nn.Parameter(new, requires_grad=False)
        self._owner.config.vision_config.image_size = new_size
        self._owner._invalidate()

    def get_input_embeddings(self):
        return self.embeddings


class _LanguageModel(_Node):
    """``model.language_model`` surface (modeling_internlm2.py:1016-1032 + HF resize_token_embeddings)."""

    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)

    @property
    def config(self):
        return self._owner.config.llm_config

    def get_input_embeddings(self):
        return self.model.tok_embeddings

    def get_output_embeddings(self):
        return self.output

    def resize_token_embeddings(self, n: int):
        for node in (self.model.tok_embeddings, self.output):
            old = node.weight.data
            new = torch.zeros((n, old.shape[1]), dtype=old.dtype, device=old.device)
            new[: min(n, old.shape[0])] = old[: min(n, old.shape[0])]
            if n > old.shape[0]:
                new[old.shape[0]:].normal_(0.0, self.config.initializer_range)
            node.weight = nn.Parameter(new, requires_grad=False)
        self.config.vocab_size = n
        self._owner._invalidate()
        return self.model.tok_embeddings


def _attach(root: nn.Module, dotted: str, tensor: torch.Tensor):
    parts = dotted.split(".")
    node = root
    for p in parts[:-1]:
        if p not in node._modules:
            node.add_module(p, _Node())
        node = node._modules[p]
    node.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


class Loading:
    # ---- construction / (de)serialisation ----------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, torch_dtype=torch.bfloat16, config: Optional[InternVLChatConfig] = None, **kw):
        """Load ``config.json`` + the MODEL shards of a checkpoint directory with the reference's state-dict names
        (stage2_eval.py:779-780); ``slowfast_model.*`` tensors build the native motion branch.

        A directory written by the reference trainer (HF Trainer) also holds ``training_args.bin``, ``optimizer.pt``,
        ``scheduler.pt``, ``rng_state*.pth`` and possibly ``lora_weights.pth`` (stage2_train.py:223-235): only
        ``model*.safetensors`` / ``pytorch_model*.bin`` are read (through the ``*.index.json`` weight map when there is one),
        ``lora_weights.pth`` is folded in by ``weights.merge_lora_state_dict``, everything else is ignored."""
        if config is None:
            config = InternVLChatConfig.from_pretrained(path)
        model = cls(config, dtype=torch_dtype, **kw)
        model.load_state_dict(cls._read_checkpoint(path))
        return model

    @staticmethod
    def _checkpoint_files(path) -> List[str]:
        """The weight shards of a checkpoint directory, in load order (host logic; no tensor is read)."""
        import json
        names = sorted(os.listdir(path))
        for index in ("model.safetensors.index.json", "pytorch_model.bin.index.json"):
            if index in names:
                with open(os.path.join(path, index)) as f:
                    shards = sorted(set(json.load(f)["weight_map"].values()))
                missing = [x for x in shards if x not in names]
                if missing:
                    raise FileNotFoundError(f"{index} names shards that are not under {path}: {missing}")
                return shards
        st = [f for f in names if f.endswith(".safetensors") and (f.startswith("model") or f.startswith("pytorch_model"))]
        if st:
            return st
        return [f for f in names if f.startswith("pytorch_model") and f.endswith(".bin")]

    @classmethod
    def _read_checkpoint(cls, path) -> Dict[str, torch.Tensor]:
        files = cls._checkpoint_files(path)
        if not files:
            raise FileNotFoundError(f"no model shards (model*.safetensors / pytorch_model*.bin) found under {path}")
        sd: Dict[str, torch.Tensor] = {}
        for f in files:
            fp = os.path.join(path, f)
            if f.endswith(".safetensors"):
                from safetensors.torch import load_file
                sd.update(load_file(fp))
            else:
                sd.update(torch.load(fp, map_location="cpu", weights_only=True))
        lora = os.path.join(path, "lora_weights.pth")
        has_adapters = any(".lora_A." in k for k in sd)
        if os.path.exists(lora) or has_adapters:
            from .weights import merge_lora_state_dict
            extra = torch.load(lora, map_location="cpu", weights_only=True) if os.path.exists(lora) else None
            sd = merge_lora_state_dict(sd, extra)
        return sd

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sf = {k: v for k, v in state_dict.items() if k.startswith("slowfast_model.")}
        if sf:   # the motion branch's backbone travels in the reference's checkpoints (modeling_internvl_chat.py:253)
            from .slowfast import SlowFastR50
            self.slowfast_model = SlowFastR50(sf)
        sd = {k: v for k, v in state_dict.items() if not k.startswith("slowfast_model.")}
        sd = self._family_names(sd)
        if self.stage == 1:
            sd = {k: v for k, v in sd.items() if not k.startswith("mlpscore.")}
        own = dict(self.named_parameters())
        missing = [k for k in own if k not in sd]
        unexpected = [k for k in sd if k not in own]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]}{'...' if len(missing) > 5 else ''}, "
                               f"unexpected {unexpected[:5]}{'...' if len(unexpected) > 5 else ''}")
        with torch.no_grad():
            for k, p in own.items():
                if k in sd:
                    if tuple(sd[k].shape) != tuple(p.shape):
                        raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(p.shape)}")
                    p.copy_(sd[k].to(p.dtype))
        self._invalidate()
        return missing, unexpected

    def _family_names(self, sd):
        """A transformers-Llama state dict (the reference's second LLM family) -> this module's InternLM2-layout names and packing."""
        from . import weights
        if not weights.is_llama_state_dict(sd):
            return sd
        if self.llm_arch_name != "LlamaForCausalLM":
            raise RuntimeError("load_state_dict: Llama tensor names in a checkpoint for an InternLM2 configuration")
        return weights.llama_to_internlm2(sd, self.config.llm_config)

    def load_state_dict_stream(self, named_tensors, strict: bool = True):
        """load_state_dict from an iterable of (name, tensor) without ever holding the whole state dict on the host (InternVL2-26B: 51 GB):
        every tensor is copied into its parameter as it arrives.  The same contract as load_state_dict: InternLM2-layout names always load,
        transformers-Llama names are re-packed on the fly (Llama configurations only), ``slowfast_model.*`` tensors build the motion branch,
        names the model does not own raise, and so do missing tensors unless ``strict=False`` (then their names are returned).  Whatever
        happens, the native copy of the weights is invalidated - a failed stream never leaves it silently out of step with the module."""
        from .weights import llama_stream_to_internlm2
        own = dict(self.named_parameters())
        seen = set()
        slowfast = {}

        def routed():
            for k, v in named_tensors:
                if k.startswith("slowfast_model."):
                    slowfast[k] = v
                    continue
                yield k, v

        stream = routed()
        if self.llm_arch_name == "LlamaForCausalLM":
            stream = llama_stream_to_internlm2(stream, self.config.llm_config)     # (InternLM2-layout names pass through unchanged)
        try:
            with torch.no_grad():
                for k, v in stream:
                    if self.stage == 1 and k.startswith("mlpscore."):
                        continue
                    if k not in own:
                        raise RuntimeError(f"load_state_dict_stream: unexpected tensor {k}")
                    if tuple(v.shape) != tuple(own[k].shape):
                        raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(own[k].shape)}")
                    own[k].copy_(v.to(own[k].dtype))
                    seen.add(k)
            if slowfast:
                from .slowfast import SlowFastR50
                self.slowfast_model = SlowFastR50(slowfast)
        finally:
            self._invalidate()
        missing = [k for k in own if k not in seen]
        if strict and missing:
            raise RuntimeError(f"load_state_dict_stream: missing {missing[:5]}{'...' if len(missing) > 5 else ''}")
        return missing
