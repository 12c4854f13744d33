"""Host-side mirror of the reference's ``InternVLChatModel`` over the gfx950 C-ABI library.

Same class name, constructor, attributes and method signatures as
internvl/model/internvl_chat_eval2/modeling_internvl_chat.py:195-853 (stage-2 flavour; ``stage=1`` gives
internvl_chat_eval1's return dict), so ``stage{1,2}_eval.py`` call sites run unchanged:

    model = InternVLChatModel.from_pretrained(path, torch_dtype=torch.bfloat16, config=cfg)
    model.img_context_token_id = ...; model.eval(); model.cuda()
    out = model(mos=..., pixel_values=..., input_ids=..., attention_mask=..., image_flags=..., labels=...)
    out['score1'], out['logit'], out['label']

PyTorch is used for tensor containers, weight (de)serialisation and index bookkeeping only; every FLOP of
the hot path runs in ``libaigv_amd.so``.  There is no CPU / eager fallback: without the library or a GPU the
hot-path methods raise.

Documented deviations from the reference (all outside what its eval scripts exercise):
  * ``logit`` holds argmax ids only at positions whose shifted label is not -100 (the answer rows the eval
    slices, stage2_eval.py:940-941); other positions are -1 unless ``full_logits=True``.
  * the score row ``hidden[:, -4]`` is taken relative to each clip's true (un-padded) end.
  * a visual-token count mismatch raises instead of overwriting a prefix (modeling_internvl_chat.py:381-386).
  * the SlowFast motion branch (``slowfast_model``) is the native ``SlowFastR50`` when the state dict carries
    ``slowfast_model.*`` tensors (the reference downloads them from pytorchvideo's hub at construction time,
    which cannot happen offline); otherwise pass ``motion_feature=[B, 2304]`` or set ``slowfast_model`` to a
    callable with the reference's interface.
  * ``generate`` implements greedy decoding and multinomial sampling (temperature / top-k / top-p, HF's warper order) with HF's
    repetition_penalty / no_repeat_ngram_size processors; the reference defers to HF ``generate`` - its eval configs use
    do_sample=False.  num_beams > 1 runs HF's beam search (beam.py: best hypothesis only; beam sampling / beam groups raise).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import generation, readouts, synth
from .config import InternVLChatConfig
from .context import NativeContext, resized_pos_table, rope_tables      # noqa: F401  (the two table builders are part of this module's surface)
from .conversation import get_conv_template
from .decoding import Generation
from .graphs import _PARKED_GRAPHS, GraphReplay                         # noqa: F401  (the very list the graph code appends to)
from .loading import Loading, _attach, _LanguageModel, _Node, _VisionModel
from .scoring import ScoringPass, VisualAhead                           # noqa: F401


class InternVLChatModel(Loading, NativeContext, GraphReplay, ScoringPass, Generation, nn.Module):
    """The model is assembled here from its concerns, one module each: checkpoint loading (loading.py), the native context and its modes
    (context.py), HIP-graph replay (graphs.py), the scoring pass (scoring.py; which read-outs a pass carries: readouts.py) and generation
    (decoding.py).  The pieces are plain base classes that share this object's state; none imports this module."""
    main_input_name = "pixel_values"
    # thin aliases, under the names they have always had here, of what lives in readouts.py and generation.py
    MAX_CANDIDATES, MAX_TOPK = readouts.MAX_CANDIDATES, readouts.MAX_TOPK
    _candidates = staticmethod(readouts.candidates)
    _top_logprobs_k = staticmethod(readouts.top_logprobs_k)
    _gen_args = staticmethod(generation.gen_args)
    _gen_flags = staticmethod(generation.gen_flags)
    _repetition_penalty = staticmethod(generation.repetition_penalty)
    _no_repeat_ngram = staticmethod(generation.no_repeat_ngram)
    _sample = staticmethod(generation.sample)
    _warp = staticmethod(generation.warp)

    def __init__(self, config: InternVLChatConfig, vision_model=None, language_model=None, use_flash_attn=True,
                 device=None, dtype=torch.bfloat16, stage: int = 2, max_clips: int = 4, max_frames: Optional[int] = None,
                 max_tokens: int = 0):
        super().__init__()
        if vision_model is not None or language_model is not None:
            raise NotImplementedError("pass weights through load_state_dict / from_pretrained")
        if config.llm_config.architectures[0] not in ("InternLM2ForCausalLM", "LlamaForCausalLM"):
            # the two families the reference constructor accepts (modeling_internvl_chat.py:228-233).  A Llama checkpoint is re-packed
            # into the InternLM2 weight layout when it is loaded (weights.llama_to_internlm2): the kernels and this module's parameter
            # names are the same for both families
            raise NotImplementedError(f"{config.llm_config.architectures[0]} is not implemented.")
        if dtype != torch.bfloat16:
            raise NotImplementedError("the gfx950 path computes in bf16 (the reference eval dtype, stage2_eval.py:780)")
        self.config = config
        self.stage = stage
        self.patch_size = config.vision_config.patch_size
        self.select_layer = config.select_layer
        self.template = config.template
        self.num_image_token = config.num_image_token
        self.downsample_ratio = config.downsample_ratio
        self.ps_version = config.ps_version
        if self.ps_version != "v2":
            raise NotImplementedError("only ps_version 'v2' (the shipped config) is on the hot path")
        self.llm_arch_name = config.llm_config.architectures[0]
        self.img_context_token_id = None
        self.conv_template = get_conv_template(self.template)
        self.system_message = self.conv_template.system_message
        self.slowfast_model = None          # optional callable([slow, fast]) -> [B, 2304, 1, 1, 1]
        self._max_clips, self._max_frames, self._max_tokens = max_clips, max_frames, max_tokens
        self._ctx = None
        self._ctx_key = None
        self._dirty = True
        self._rope_ntk = 0                  # sequence length the dynamic-NTK rotary base is currently built for (0: plain tables)

        dev = torch.device(device) if device is not None else torch.device("cpu")
        self.vision_model = _VisionModel(self)
        self.language_model = _LanguageModel(self)
        for name, shape, _kind in synth.weight_shapes(config):
            if stage == 1 and name.startswith("mlpscore."):
                continue
            root, rest = name.split(".", 1)
            if root not in self._modules:
                self.add_module(root, _Node())
            _attach(self._modules[root], rest, torch.empty(shape, dtype=dtype, device=dev))

