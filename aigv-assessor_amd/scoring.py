"""The scoring pass of ``InternVLChatModel``: the visual front, pass planning, prefill, the score-attention probe, ``forward`` and the shared-prefix pass."""
from __future__ import annotations

import ctypes as C
from itertools import accumulate
from typing import List, Optional

import torch
import torch.nn.functional as F

from . import native, readouts


# ------------------------------------------------------------------------------------------------------
class VisualAhead:
    """The visual front of a LATER ``forward`` call, started ahead of time by ``InternVLChatModel.prefetch``: pre-projector tokens
    [F, ntok, 4 Hv], the SlowFast feature of the clips (or None) and the event the consuming stream waits for.  Pass it as ``pixel_values``."""
    __slots__ = ("tokens", "motion", "event", "n_clips")

    def __init__(self, tokens, motion, event, n_clips):
        self.tokens, self.motion, self.event, self.n_clips = tokens, motion, event, n_clips


class ScoringPass:
    # ---- hot path -----------------------------------------------------------------------------------------
    def ingest_frames(self, frames_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                      size: Optional[int] = None) -> torch.Tensor:
        """uint8 [F, H, W, 3] RGB frames (one tensor, or a list of per-clip tensors) -> normalised bf16 NCHW ``pixel_values`` on the GPU: the reference's per-frame
        ``image.resize((448, 448))`` (PIL BICUBIC; dataset.py:702-738 with max_num = 1, stage2_eval.py:453-456) when the
        frames are not at the model resolution yet, then ToTensor + Normalize + the bf16 cast of its eval transform
        (dataset.py:267-274, stage2_eval.py:932).  The resize is bit-exact with Pillow (include/aigv_amd.h)."""
        parts = list(frames_u8) if isinstance(frames_u8, (list, tuple)) else [frames_u8]
        for t in parts:
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or t.shape[1:] != parts[0].shape[1:]:
                raise ValueError("frames must be uint8 [F, H, W, 3] (or a list of such tensors of one frame size)")
        lib = native.load()
        if self.device.type != "cuda":
            raise native.NativeError("the scorer hot path runs on an MI355X only (no CPU fallback)")
        S = int(size or self.config.image_size)
        # (pinned host frames go up without blocking the host: the copy is ordered on the current stream like the kernels that read it.  A list -
        # the clips of one group, each in its own host buffer - is copied clip by clip and joined on the device: no host-side concatenation)
        parts = [t.to(self.device, non_blocking=not t.is_cuda and t.is_pinned()) for t in parts]
        f = (torch.cat(parts) if len(parts) > 1 else parts[0]).contiguous()
        n, h, w, _ = f.shape
        out = torch.empty((n, 3, S, S), dtype=torch.bfloat16, device=self.device)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        if (h, w) == (S, S):
            native.check(lib.aigv_op_frame_ingest(f.data_ptr(), n, h, w, m3, s3, out.data_ptr(), native.stream_ptr()))
        else:
            tmp = torch.empty(n * h * S * 3, dtype=torch.uint8, device=self.device)
            native.check(lib.aigv_op_frame_resize_ingest(f.data_ptr(), n, h, w, S, S, m3, s3, tmp.data_ptr(), None, out.data_ptr(),
                                                         native.stream_ptr()))
        return out

    def vit_tokens(self, pixel_values: torch.Tensor, patch_drop: Optional[torch.Tensor] = None, patch_drop_layers=None) -> torch.Tensor:
        """InternViT -> drop cls -> pixel-shuffle: [F,3,S,S] -> [F, ntok, 4*Hv] pre-projector tokens (the
        frame-DP all-gather payload; modeling_internvl_chat.py:509-527).

        ``patch_drop`` (None: exactly the call without it): PATCH OCCLUSION inside the tower - bool [F, G, G], G = image_size // patch_size, True =
        patch (y, x) of that frame is hidden, AS A KEY, from every row of its frame in the tower's attention (the non-causal key-drop form of the
        attention kernel; ``aigv_vit_key_drop_arm``).  Pixels, positions, the cls token and every other patch stay as they are; cls is not
        addressable, so no row is ever without a key.  The hidden patches' own rows still run and still carry their own content to their cell's
        token - ``eval_utils.patch_occlusion`` hides those tokens from the LLM.  ``patch_drop_layers = (lo, hi)``: the mask applies in layers
        lo <= l < hi only, 0 <= lo < hi <= ``vit_layers_run()``; None: every layer the pass runs.  The masked call runs eagerly on the current
        stream (never inside a graph capture) after waiting for a prefetch in flight; ValueError for a wrong shape, dtype or window."""
        if patch_drop is not None:
            return self._vit_tokens_masked(pixel_values, patch_drop, patch_drop_layers)
        if patch_drop_layers is not None:
            raise ValueError("vit_tokens: patch_drop_layers qualifies a patch_drop mask and needs one")
        if pixel_values.dim() != 4:
            raise ValueError(f"wrong pixel_values size: {pixel_values.shape}")  # modeling_intern_vit.py:345
        nf = pixel_values.shape[0]
        S = self.config.image_size
        if tuple(pixel_values.shape[1:]) != (self.config.vision_config.num_channels, S, S):
            raise ValueError(f"pixel_values must be [F,{self.config.vision_config.num_channels},{S},{S}], got {tuple(pixel_values.shape)}")
        lib, ctx = self._native(n_frames=nf)
        self._wait_for_prefetch()
        pv = pixel_values.to(device=self.device, dtype=torch.bfloat16).contiguous()
        out = torch.empty((nf, self.num_image_token, self.config.proj_in), dtype=torch.bfloat16, device=self.device)
        native.check(lib.aigv_vit_forward(ctx, pv.data_ptr(), nf, out.data_ptr(), native.stream_ptr()), ctx)
        return out

    def _vit_tokens_masked(self, pixel_values, patch_drop, patch_drop_layers) -> torch.Tensor:
        """``vit_tokens(patch_drop=...)``: the checks, the host-built words, the armed pass."""
        from . import prompts
        if pixel_values.dim() != 4:
            raise ValueError(f"wrong pixel_values size: {pixel_values.shape}")
        v = self.config.vision_config
        nf, size = pixel_values.shape[0], self.config.image_size
        if nf < 1 or tuple(pixel_values.shape[1:]) != (v.num_channels, size, size):
            raise ValueError(f"pixel_values must be [F,{v.num_channels},{size},{size}] with F >= 1, got {tuple(pixel_values.shape)}")
        G = size // v.patch_size
        if not torch.is_tensor(patch_drop) or patch_drop.dtype != torch.bool or tuple(patch_drop.shape) != (nf, G, G):
            raise ValueError(f"vit_tokens: patch_drop must be a bool tensor [{nf}, {G}, {G}] (frames, patch rows, patch columns), got "
                             f"{getattr(patch_drop, 'dtype', type(patch_drop).__name__)} {tuple(getattr(patch_drop, 'shape', ()))}")
        n_run = self.vit_layers_run()
        try:
            lo, hi = (0, n_run) if patch_drop_layers is None else (int(x) for x in patch_drop_layers)
        except (TypeError, ValueError):
            lo, hi = 0, 0
        if not 0 <= lo < hi <= n_run:
            raise ValueError(f"vit_tokens: patch_drop_layers = {patch_drop_layers!r} is no window (lo, hi) with 0 <= lo < hi <= {n_run}, the layers the pass runs")
        if self._capture_keep is not None or native._captures_underway > 0 or (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("vit_tokens(patch_drop=...) runs eagerly: it cannot be part of a graph capture")
        if self.device.type != "cuda":
            raise native.NativeError("the scorer hot path runs on an MI355X only (no CPU fallback)")
        words = prompts.patch_drop_words(patch_drop).to(self.device)      # int64 [F, W]: the 64 bits the kernel reads
        lib, ctx = self._native(n_frames=nf)
        self._wait_for_prefetch()
        pv = pixel_values.to(device=self.device, dtype=torch.bfloat16).contiguous()
        out = torch.empty((nf, self.num_image_token, self.config.proj_in), dtype=torch.bfloat16, device=self.device)
        native.check(lib.aigv_vit_key_drop_arm(ctx, words.data_ptr(), int(words.shape[1]), lo, hi), ctx)
        native.check(lib.aigv_vit_forward(ctx, pv.data_ptr(), nf, out.data_ptr(), native.stream_ptr()), ctx)
        return out      # (`words` stays referenced until the launches are queued; the caching allocator keeps freed memory stream-ordered)

    def vit_layers_run(self) -> int:
        """The number of InternViT layers a pass runs: ``select_layer``'s count (-1: all of them), not ``num_hidden_layers``."""
        n = self.config.vision_config.num_hidden_layers
        sel = self.select_layer
        return n if sel == -1 else n + 1 + sel if sel < 0 else sel

    def vit_attention(self, pixel_values: torch.Tensor, layers=None, per_head: bool = False) -> dict:
        """INSIDE the vision tower: the full, non-causal softmax matrix of every row of every frame, per layer - what the flash kernel never forms
        (csrc/vitmap.hip; ``aigv_vit_attention_arm`` in include/aigv_amd.h defines the quantity: fp32 scores and weights whatever the attention
        numerics, the unscaled bf16 Q - the flash kernel's bf16 ``q_prescale`` rounding is not reproduced).  Returns ``{"vit_attention": fp32
        [F, hi - lo, S, S] - the head mean - or [F, hi - lo, n_heads, S, S] with ``per_head``, "tokens": the pass's pre-projector tokens, bit
        for bit ``vit_tokens(pixel_values)``}``; S = patches + 1, row / column 0 the cls token, patch (y, x) at 1 + grid * y + x.
        ``layers = (lo, hi)``: the window 0 <= lo < hi <= ``vit_layers_run()``; None: every layer the pass runs.  Runs eagerly on the current
        stream (never inside a graph capture) after waiting for a prefetch in flight.  ValueError for a bad window and - with the byte count -
        for a result that does not fit the device's free memory: F (hi - lo) S^2 4 bytes, times n_heads per head (3.2 GB for 32 frames x 24
        layers at S = 1025, head mean).  ``eval_utils.vit_rollout`` / ``pixel_heatmaps`` carry a heat map through it to the pixels."""
        if pixel_values.dim() != 4:
            raise ValueError(f"wrong pixel_values size: {pixel_values.shape}")
        v = self.config.vision_config
        nf, size = pixel_values.shape[0], self.config.image_size
        if nf < 1 or tuple(pixel_values.shape[1:]) != (v.num_channels, size, size):
            raise ValueError(f"pixel_values must be [F,{v.num_channels},{size},{size}] with F >= 1, got {tuple(pixel_values.shape)}")
        n_run = self.vit_layers_run()
        try:
            lo, hi = (0, n_run) if layers is None else (int(x) for x in layers)
        except (TypeError, ValueError):
            lo, hi = 0, 0
        if not 0 <= lo < hi <= n_run:
            raise ValueError(f"vit_attention: layers = {layers!r} is no window (lo, hi) with 0 <= lo < hi <= {n_run}, the layers the pass runs")
        if self._capture_keep is not None or native._captures_underway > 0 or (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("vit_attention runs eagerly: it cannot be part of a graph capture")
        if self.device.type != "cuda":
            raise native.NativeError("the scorer hot path runs on an MI355X only (no CPU fallback)")
        S = (size // v.patch_size) ** 2 + 1
        shape = (nf, hi - lo) + ((v.num_attention_heads,) if per_head else ()) + (S, S)
        need = 4 * nf * (hi - lo) * (v.num_attention_heads if per_head else 1) * S * S
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:      # (before the context grows for the frames: nothing is allocated for a refused call)
            raise ValueError(f"vit_attention: the result {list(shape)} takes {need} bytes, the device has {free} free: narrow `layers` or pass fewer frames")
        lib, ctx = self._native(n_frames=nf)
        self._wait_for_prefetch()
        pv = pixel_values.to(device=self.device, dtype=torch.bfloat16).contiguous()
        tokens = torch.empty((nf, self.num_image_token, self.config.proj_in), dtype=torch.bfloat16, device=self.device)
        att = torch.empty(shape, dtype=torch.float32, device=self.device)
        native.check(lib.aigv_vit_attention_arm(ctx, att.data_ptr(), lo, hi, int(bool(per_head))), ctx)
        native.check(lib.aigv_vit_forward(ctx, pv.data_ptr(), nf, tokens.data_ptr(), native.stream_ptr()), ctx)
        return {"vit_attention": att, "tokens": tokens}

    def _take_ahead(self, pixel_values, visual_tokens, motion_feature):
        """``pixel_values`` may be the handle of a visual front started ahead of time (``prefetch``): wait for it on the caller's stream and continue
        from its tokens / SlowFast feature; a plain ``pixel_values`` first waits for any prefetch in flight (one visual front at a time)."""
        if isinstance(pixel_values, VisualAhead):
            torch.cuda.current_stream(self.device).wait_event(pixel_values.event)
            return None, pixel_values.tokens, pixel_values.motion if motion_feature is None else motion_feature
        if pixel_values is not None:
            self._wait_for_prefetch()
        return pixel_values, visual_tokens, motion_feature

    def _wait_for_prefetch(self):
        """The InternViT workspaces of the context serve ONE visual front at a time: a pass that runs the ViT on the caller's stream (eager or
        as a replayed graph) first waits for whatever ``prefetch`` still has in flight on its own stream."""
        if self._capture_keep is not None:
            return      # inside a graph capture: the caller (forward / dp_front) already waited before _graph_call; an event recorded on a
                        # non-capturing stream must not be waited on from the capture stream
        look = getattr(self, "_look_stream", None)
        cur = torch.cuda.current_stream(self.device)
        if look is not None and cur != look:
            cur.wait_stream(look)

    def project(self, tokens: torch.Tensor) -> torch.Tensor:
        """mlp1 on pre-projector tokens [..., 4*Hv] -> [..., H] (modeling_internvl_chat.py:529)."""
        lib, ctx = self._native()
        t = tokens.to(device=self.device, dtype=torch.bfloat16).contiguous()
        rows = t.numel() // t.shape[-1]
        out = torch.empty(t.shape[:-1] + (self.config.llm_config.hidden_size,), dtype=torch.bfloat16, device=self.device)
        native.check(lib.aigv_project(ctx, t.data_ptr(), rows, out.data_ptr(), native.stream_ptr()), ctx)
        return out

    def extract_feature(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """modeling_internvl_chat.py:508-531: [F,3,S,S] -> [F, num_image_token, llm_hidden]."""
        return self.project(self.vit_tokens(pixel_values))

    def motion_embed(self, motion_feature: torch.Tensor) -> torch.Tensor:
        """motion_mlp on the SlowFast feature [B, motion_dim] -> [B, H] (modeling_internvl_chat.py:344-345)."""
        b = motion_feature.shape[0]
        self._join_side_stream()
        lib, ctx = self._native(n_clips=b)
        m = motion_feature.reshape(b, -1).to(device=self.device, dtype=torch.bfloat16).contiguous()
        if m.shape[1] != self.config.motion_dim:
            raise ValueError(f"motion_feature must be [B,{self.config.motion_dim}]")
        out = torch.empty((b, self.config.llm_config.hidden_size), dtype=torch.bfloat16, device=self.device)
        native.check(lib.aigv_motion_project(ctx, m.data_ptr(), b, out.data_ptr(), native.stream_ptr()), ctx)
        return out

    def motion_feature(self, pixel_values: torch.Tensor, batch: int) -> torch.Tensor:
        """SlowFast feature [batch, motion_dim] of the clips in ``pixel_values`` [batch * T, 3, S, S] (modeling_internvl_chat.py:336-343)."""
        out = self._motion_feature(pixel_values, batch, None)
        self._join_side_stream()
        return out

    def motion_feature_async(self, pixel_values: torch.Tensor, batch: int) -> torch.Tensor:
        """The same, without joining the side stream: the tensor is only safe to consume through ``forward(motion_feature=...)`` /
        ``motion_embed``, which join it (used by the data-parallel scorer to start the branch before its ViT shard)."""
        return self._motion_feature(pixel_values, batch, None)

    def _join_side_stream(self):
        if getattr(self, "_side_pending", False):
            torch.cuda.current_stream().wait_stream(self._side_stream)
            self._side_pending = False

    def _motion_feature(self, pixel_values, batch, motion_feature):
        if motion_feature is not None:
            return motion_feature
        if self.slowfast_model is None:
            raise RuntimeError("the SlowFast motion branch is an input of this path: pass motion_feature=[B, "
                               f"{self.config.motion_dim}] or set model.slowfast_model (SURVEY.md §2 row 6)")
        if hasattr(self.slowfast_model, "features"):     # the native branch reads pixel_values as they are and samples the slow pathway itself
            pv = pixel_values.to(self.device)
            if not getattr(self, "overlap_motion_branch", True):
                return self.slowfast_model.features(pv, batch)
            # The branch depends on the frames only and its result is needed after ViT + projector: enqueue it on a side stream so that its
            # low-occupancy kernels (the slow pathway's deep layers run ~100 workgroups) fill in around the ViT's; motion_embed() joins.
            cur = torch.cuda.current_stream()
            side = getattr(self, "_side_stream", None)
            if side is None:
                side = self._side_stream = torch.cuda.Stream(device=self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                feat = self.slowfast_model.features(pv, batch)
            feat.record_stream(cur)
            pv.record_stream(side)
            self._side_pending = True
            return feat
        # a user-supplied callable: reference data flow (modeling_internvl_chat.py:337-344, pack_pathway_output :97-133)
        S = self.config.image_size
        frames = pixel_values.view(batch, pixel_values.shape[0] // batch, 3, S, S).permute(0, 2, 1, 3, 4)
        idx = torch.linspace(0, frames.shape[2] - 1, frames.shape[2] // 4).long().to(frames.device)
        with torch.no_grad():
            return self.slowfast_model([frames.index_select(2, idx), frames]).view(batch, -1)

    @staticmethod
    def _pack(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor]):
        """Strip padding: returns (packed ids [T], cu_seqlens list, packed-row index of every [b, p] or -1)."""
        b, n = input_ids.shape
        mask = torch.ones_like(input_ids, dtype=torch.bool) if attention_mask is None else attention_mask.bool()
        lens = mask.sum(1).tolist()
        cu = list(accumulate((int(x) for x in lens), initial=0))
        row_of = torch.full((b, n), -1, dtype=torch.long, device=input_ids.device)
        row_of[mask] = torch.arange(cu[-1], device=input_ids.device)
        return input_ids[mask].contiguous(), cu, row_of

    def _h2d(self, t):
        """Host tensor -> device through pinned memory without blocking the host.  While a HIP graph is being captured (``capture_forward``)
        the pinned staging buffer is kept alive with the graph: its replays copy from that very address."""
        if t.is_cuda:
            return t
        pinned = t.contiguous().pin_memory()
        keep = getattr(self, "_capture_keep", None)
        if keep is not None:
            keep.append(pinned)
        return pinned.to(self.device, non_blocking=True)

    def _prefill(self, ids_packed, slot, cu, vis, n_vis, motion, score_rows, logit_rows, keep_kv=False, kv_cap=0, probe=None, ld_tok=0, values=False, drop_words=None,
                 drop_row_words=None, drop_layers=None, lens=None, stream_capture=None, stream_patch=None, head_capture=None, head_patch=None,
                 head_scale=None, neuron_capture=None, neuron_patch=None, neuron_scale=None, attention_map=None):
        b = len(cu) - 1
        T = cu[-1]
        lib, ctx = self._native(n_tokens=T, n_clips=b, out_rows=len(logit_rows), kv_cap=kv_cap)
        dev = self.device
        def up(t, dt):   # host index arrays go up through pinned memory without blocking the host
            return self._h2d(t.to(dt).contiguous())
        ids_d = up(ids_packed, torch.long)
        slot_d = up(slot, torch.int32)
        score = torch.empty(b, dtype=torch.float32, device=dev) if score_rows is not None else None
        amax = torch.empty(max(len(logit_rows), 1), dtype=torch.long, device=dev)
        cu_a = native.i32_array(cu)
        sr_a = native.i32_array(score_rows) if score_rows is not None else None
        lr_a = native.i32_array(logit_rows) if len(logit_rows) else None
        att, tok, *val = self._arm_score_attention(probe, ld_tok, values) if probe is not None else (None, None)   # (armed for exactly the pass below)
        if drop_words is not None:      # key_drop: host int64 [B, W] (prompts.key_drop_words) -> armed for exactly the pass below, which disarms
            words_d = up(drop_words, torch.int64)
            if drop_row_words is None and drop_layers is None:
                native.check(lib.aigv_key_drop_arm(ctx, words_d.data_ptr(), int(drop_words.shape[1])), ctx)
            else:       # key_drop_rows / key_drop_layers: the mask by query row (same layout, same width) and layer window
                rows_d = up(drop_row_words, torch.int64) if drop_row_words is not None else None
                lo, hi = drop_layers if drop_layers is not None else (0, self.config.llm_config.num_hidden_layers)
                native.check(lib.aigv_key_drop_arm_ex(ctx, words_d.data_ptr(), native.ptr(rows_d), int(drop_words.shape[1]), int(lo), int(hi)), ctx)
        if attention_map is not None:   # return_segment_attention / return_row_attention: (device int32 [T] table, S, scratch, seg_out, rows_out, lo, hi) - armed likewise
            m_seg, m_S, m_scratch, m_fold, m_rows, m_lo, m_hi = attention_map
            native.check(lib.aigv_attention_map_arm(ctx, m_seg.data_ptr(), int(m_S), native.ptr(m_scratch), native.ptr(m_fold), native.ptr(m_rows), int(m_lo), int(m_hi)), ctx)
        if lens is not None:            # return_depth_lens: (score rows, token rows, hidden, normed, score) - armed for exactly the pass below, which disarms
            l_score, l_token, l_hidden, l_normed, l_out = lens
            native.check(lib.aigv_depth_lens_arm(ctx, native.i32_array(l_score) if l_score else None, len(l_score), native.i32_array(l_token) if l_token else None,
                                                 len(l_token), l_hidden.data_ptr(), l_normed.data_ptr(), native.ptr(l_out)), ctx)
        # the row options - stream_patch / return_stream, head_scale / head_patch / return_heads, neuron_scale / neuron_patch / return_neurons: armed for exactly the
        # pass below, which disarms (host arrays are read in place: the library copies them on arming)
        i32p = lambda t: C.cast(t.data_ptr(), native._I32P) if t is not None and t.numel() else None
        f32p = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float)) if t is not None and t.numel() else None

        def arm_window(arm, opt, extra=lambda opt: ()):     # a patch or a capture: (packed rows, lo, hi, [what ``extra`` passes on,] device bf16 buffer)
            if opt is not None:
                rows, lo, hi, buf = *opt[:3], opt[-1]
                native.check(arm(ctx, i32p(rows), int(rows.numel()), int(lo), int(hi), *extra(opt), native.ptr(buf) if buf.numel() else None), ctx)
        arm_window(lib.aigv_stream_patch_arm, stream_patch)     # buffers: [n, hi - lo, H]
        arm_window(lib.aigv_stream_capture_arm, stream_capture)
        if head_scale is not None:      # (packed rows or None: every row, host fp32 [L, n_heads])
            h_rows, table = head_scale
            native.check(lib.aigv_head_scale_arm(ctx, i32p(h_rows), 0 if h_rows is None else int(h_rows.numel()), C.cast(table.data_ptr(), C.POINTER(C.c_float))), ctx)
        # buffers: [n, hi - lo, n_heads, D]; the patch: one mask word per layer or None - every head
        arm_window(lib.aigv_head_patch_arm, head_patch, lambda opt: (None if opt[3] is None else (C.c_uint64 * len(opt[3]))(*opt[3]),))
        arm_window(lib.aigv_head_capture_arm, head_capture)
        if neuron_scale is not None:    # (packed rows or None: every row, host fp32 [L] or None, host int32 [m] layers / columns and fp32 [m] factors or None)
            n_rows, table, sel_l, sel_c, sel_f = neuron_scale
            native.check(lib.aigv_neuron_scale_arm(ctx, i32p(n_rows), 0 if n_rows is None else int(n_rows.numel()), f32p(table), i32p(sel_l), i32p(sel_c), f32p(sel_f),
                                                   0 if sel_l is None else int(sel_l.numel())), ctx)
        # buffers: [n, hi - lo, I or m]; cols: host int32 [m] or None - every neuron (an empty list is a list)
        cols = lambda opt: (None, 0) if opt[3] is None else (C.cast(opt[3].data_ptr(), native._I32P), int(opt[3].numel()))
        arm_window(lib.aigv_neuron_patch_arm, neuron_patch, cols)
        arm_window(lib.aigv_neuron_capture_arm, neuron_capture, cols)
        native.check(lib.aigv_llm_prefill(
            ctx, ids_d.data_ptr(), slot_d.data_ptr(), cu_a, b, native.ptr(vis), n_vis, native.ptr(motion),
            sr_a, native.ptr(score), lr_a, len(logit_rows), amax.data_ptr(), int(keep_kv), native.stream_ptr()), ctx)
        if probe is not None:
            return (score, amax[: len(logit_rows)], att, tok) + tuple(val)      # (the value vectors only when asked for: the four-element form is the one callers know)
        return score, amax[: len(logit_rows)]

    # ---- score-row attention by segment (return_score_attention) -------------------------------------------------------------------------
    MAX_ATTN_SEGMENTS = 64   # = AIGV_MAX_ATTN_SEGMENTS
    MAX_PROBE_ROWS = 64      # = AIGV_MAX_PROBE_ROWS

    def _probe_rows(self, plan) -> List[int]:
        """The packed row of every clip whose attention is reported: the score row (stage 2), else the row that predicts the clip's first
        answer token."""
        if plan["score_rows"] is not None:
            return [int(r) for r in plan["score_rows"]]
        rows = []
        answer = (plan["labels_h"][:, 1:] != -100) & (plan["row_of"][:, :-1] >= 0)
        for b in range(answer.shape[0]):
            at = answer[b].nonzero().flatten()
            if not at.numel():
                raise ValueError(f"return_score_attention: clip {b} has no answer token (a stage-1 model reports the row that predicts the first one: pass labels)")
            rows.append(int(plan["row_of"][b, int(at[0])]))
        return rows

    def _frames_per_clip(self, plan) -> List[int]:
        """The frames every clip of the plan carries: its visual-token slots over the tokens per frame."""
        slot, cu = plan["slot"], plan["cu"]
        return [int(((slot[cu[b]:cu[b + 1]] >= 0) & (slot[cu[b]:cu[b + 1]] < plan["n_vis"])).sum()) // self.num_image_token for b in range(len(cu) - 1)]

    def _default_segments(self, plan):
        """(``prompts.attention_segments`` of the plan's packed tokens, host int32 [T]; the number of bins F + 4)."""
        from . import prompts
        frames = self._frames_per_clip(plan)
        return prompts.attention_segments(plan["slot"], plan["cu"], frames, self.num_image_token), max(frames) + prompts.N_TEXT_SEGMENTS

    def _score_attention_probe(self, plan, input_ids, ro):
        """What ``_prefill`` arms the pass with: (probe rows, device int32 segment id per packed token, S).  ``ro.segments``: None -
        ``prompts.attention_segments`` - or the user's own table, an integer tensor laid out like ``input_ids`` [B, N] (on any device; padded
        positions are ignored, ids outside [0, S) drop their key from the bins), S = its largest id + 1."""
        rows = self._probe_rows(plan)
        if len(rows) > self.MAX_PROBE_ROWS:
            raise ValueError(f"return_score_attention: at most {self.MAX_PROBE_ROWS} clips per pass, got {len(rows)}")
        if ro.segments is None:
            seg, S = self._default_segments(plan)
            seg_d = self._h2d(seg)
        else:
            t = ro.segments
            S = getattr(self, "_probe_n_segments", None) or ro.n_segments(input_ids.shape)     # (a replayed graph carries S in its key: no sync in there)
            kept = (plan["row_of"] >= 0).flatten().nonzero().flatten()          # [b, p] of every packed row, in packed order (host)
            seg_d = t.to(self.device).flatten().index_select(0, self._h2d(kept)).to(torch.int32).contiguous()
        if not 1 <= S <= self.MAX_ATTN_SEGMENTS:
            raise ValueError(f"return_score_attention: {S} segments, outside 1..{self.MAX_ATTN_SEGMENTS}")
        return rows, seg_d, None, 0, S

    def _attention_map_table(self, plan, input_ids, ro):
        """The attention map's table for this plan, on the HOST: (int32 [T] segment id per packed token, S).  ``ro.segments``: None -
        ``prompts.attention_segments`` - or the user's table [B, N] (on any device), the probe's rules.  ValueError for more than 64 bins."""
        if ro.segments is None:
            seg, S = self._default_segments(plan)
            return seg.to(torch.int32).contiguous(), ro.map_segments(input_ids.shape, S)
        S = ro.map_segments(input_ids.shape, 0)
        kept = (plan["row_of"] >= 0).flatten().nonzero().flatten()              # [b, p] of every packed row, in packed order (host)
        return ro.segments.detach().to("cpu").flatten().index_select(0, kept).to(torch.int32).contiguous(), S

    def _attention_map_buffers(self, plan, seg, S, amap):
        """What ``_prefill`` arms the map with: (device table, S, scratch [T, n_heads, S] or None, seg_out [B, L, n_heads, S, S] or None, rows_out
        [hi - lo, T, n_heads, S] or None, lo, hi), fp32 on the device."""
        llm = self.config.llm_config
        T, B, L, nh = plan["cu"][-1], len(plan["cu"]) - 1, llm.num_hidden_layers, llm.num_attention_heads
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        lo, hi = amap.rows if amap.rows is not None and amap.rows[0] < amap.rows[1] else (0, 0)
        fold = new(B, L, nh, S, S) if amap.segments else None
        return (self._h2d(seg), S, new(T, nh, S) if fold is not None and hi - lo < L else None, fold, new(hi - lo, T, nh, S) if hi > lo else None, lo, hi)

    def _attention_map_outputs(self, plan, N, seg, armed, amap) -> dict:
        """The map's entries of the result dict: ``segment_attention`` / ``segment_rows`` and ``row_attention`` (``forward``'s docstring)."""
        _, S, _, fold, rows, lo, hi = armed
        cu, out = plan["cu"], {}
        B = len(cu) - 1
        if amap.segments:
            count = torch.zeros(B, S, dtype=torch.long)
            for b in range(B):
                mine = seg[cu[b]:cu[b + 1]].long()
                count[b] = torch.bincount(mine[(mine >= 0) & (mine < S)], minlength=S)
            out["segment_attention"], out["segment_rows"] = fold, self._h2d(count)
        if amap.rows is not None:
            nh = self.config.llm_config.num_attention_heads
            full = torch.full((B, amap.rows[1] - amap.rows[0], nh, N, S), float("nan"), dtype=torch.float32, device=self.device)
            if rows is not None:
                for b in range(B):
                    full[b, :, :, :cu[b + 1] - cu[b]] = rows[:, cu[b]:cu[b + 1]].permute(0, 2, 1, 3)
            out["row_attention"] = full
        return out

    def visual_token_positions(self, input_ids, attention_mask=None, image_flags=None, n_frames: Optional[int] = None) -> torch.Tensor:
        """``prompts.visual_token_positions`` of a batch as ``forward`` would pack it (host only, no GPU work): long [B, F, tokens_per_frame], the
        column of ``score_attention_tokens[b]`` that holds every visual token of every frame, -1 where a clip has fewer frames than the
        longest.  ``n_frames``: the frames handed to ``forward`` (``pixel_values.shape[0]``; default: ``image_flags.shape[0]``)."""
        from . import prompts
        if n_frames is None:
            if image_flags is None:
                raise ValueError("visual_token_positions: pass n_frames or image_flags")
            n_frames = int(image_flags.shape[0])
        plan = self._plan(input_ids, attention_mask, None, image_flags, int(n_frames))
        return prompts.visual_token_positions(plan["slot"], plan["cu"], self._frames_per_clip(plan), self.num_image_token)

    def unit_masks(self, input_ids, attention_mask=None, image_flags=None, n_frames: Optional[int] = None) -> torch.Tensor:
        """The ablation units of a batch as ``forward(key_drop=...)`` masks (host only, no GPU work): bool [B, F + 1, N] laid out like
        ``input_ids``; unit u < F marks the visual tokens of the clip's frame u, unit F its motion token.  A clip with fewer frames than the
        longest has all-False rows for the frames it lacks.  Built from ``prompts.attention_segments`` of the batch as ``forward`` would pack
        it, the way ``visual_token_positions`` is.  ``n_frames``: the frames handed to ``forward`` (default: ``image_flags.shape[0]``)."""
        if n_frames is None:
            if image_flags is None:
                raise ValueError("unit_masks: pass n_frames or image_flags")
            n_frames = int(image_flags.shape[0])
        from . import prompts
        plan = self._plan(input_ids, attention_mask, None, image_flags, int(n_frames))
        seg, S = self._default_segments(plan)
        F = S - prompts.N_TEXT_SEGMENTS
        row_of = plan["row_of"]
        seg_of = torch.where(row_of >= 0, seg.long()[row_of.clamp_min(0)], torch.full_like(row_of, -1))      # [B, N]: segment id, -1 where not run
        return torch.stack([seg_of == u for u in range(F + 1)], 1)

    def segment_masks(self, input_ids, attention_mask=None, image_flags=None, n_frames: Optional[int] = None) -> dict:
        """The token groups of a batch as ``key_drop`` / ``key_drop_rows`` masks (host only, no GPU work): a dict of bool [B, N] laid out like
        ``input_ids`` - ``frames`` (every visual token: the union of ``unit_masks[:, :F]``), ``motion`` (the motion token), ``first`` (the
        clip's first token, the sink), ``text_before`` (the other text up to the last visual token), ``text_after`` (the text behind it:
        question and answer) and ``score_row`` (the row the score head reads, inside ``text_after``; all False in a stage-1 model).  The first
        five partition every clip's tokens.  Built from ``prompts.attention_segments``, the table the attention bins use.  ``n_frames``: the
        frames handed to ``forward`` (default: ``image_flags.shape[0]``)."""
        if n_frames is None:
            if image_flags is None:
                raise ValueError("segment_masks: pass n_frames or image_flags")
            n_frames = int(image_flags.shape[0])
        from . import prompts
        plan = self._plan(input_ids, attention_mask, None, image_flags, int(n_frames), drop_dead_tail=False)      # (every un-padded token, also those behind the score row)
        seg, S = self._default_segments(plan)
        F = S - prompts.N_TEXT_SEGMENTS
        row_of = plan["row_of"]
        seg_of = torch.where(row_of >= 0, seg.long()[row_of.clamp_min(0)], torch.full_like(row_of, -1))      # [B, N]: segment id, -1 for padding
        score = torch.zeros_like(row_of, dtype=torch.bool)
        for r in plan["score_rows"] or []:
            score |= row_of == int(r)
        return {"frames": (seg_of >= 0) & (seg_of < F), "motion": seg_of == F, "first": seg_of == F + 1, "text_before": seg_of == F + 2,
                "text_after": seg_of == F + 3, "score_row": score}

    def _key_drop_words(self, plan, key_drop: torch.Tensor, key_drop_rows: Optional[torch.Tensor] = None):
        """``forward(key_drop=...)``: the host bool mask [B, N] checked against the plan -> ``prompts.key_drop_words`` (host int64 [B, W]).
        Positions the pass does not run (padding, a dropped dead tail) are ignored.  Refused before anything is launched: dropping a clip's
        first token (the sink: it guarantees that every row keeps a visible key) and dropping a row whose output is consumed.
        With ``key_drop_rows`` (host bool [B, N]) -> (key words, row words), both [B, W]: no row may be cut from itself (``key_drop_rows &
        key_drop`` is empty - with the first token that guarantees every row a visible key), and a consumed row may then be a key."""
        from . import prompts
        row_of, cu = plan["row_of"], plan["cu"]
        if tuple(key_drop.shape) != tuple(row_of.shape):
            raise ValueError(f"key_drop: shape {tuple(key_drop.shape)} differs from input_ids {tuple(row_of.shape)}")
        rows = row_of[key_drop & (row_of >= 0)]                    # the packed rows that are dropped
        dropped = torch.zeros(cu[-1], dtype=torch.bool)
        dropped[rows] = True
        for b in range(len(cu) - 1):
            if bool(dropped[cu[b]]):
                raise ValueError(f"key_drop: clip {b}: the first token cannot be dropped (it guarantees every row a visible key)")
        if key_drop_rows is not None:
            if tuple(key_drop_rows.shape) != tuple(row_of.shape):
                raise ValueError(f"key_drop_rows: shape {tuple(key_drop_rows.shape)} differs from input_ids {tuple(row_of.shape)}")
            both = (key_drop_rows & key_drop & (row_of >= 0)).any(1)
            if bool(both.any()):
                raise ValueError(f"key_drop_rows: clip {int(both.nonzero()[0])}: a token is both a dropped key and a selected row (a row is never cut from itself)")
            return prompts.key_drop_words(key_drop, cu, row_of), prompts.key_drop_words(key_drop_rows, cu, row_of)
        for r in list(plan["logit_rows"]) + list(plan["score_rows"] or []):
            if bool(dropped[r]):
                b = max(i for i in range(len(cu) - 1) if cu[i] <= r)
                raise ValueError(f"key_drop: clip {b}: token {r - cu[b]} is a consumed row (an answer row or the score row) and cannot be dropped")
        return prompts.key_drop_words(key_drop, cu, row_of)

    def _arm_score_attention(self, probe, ld_tok: int = 0, values: bool = False):
        """Arm the context's NEXT prefill / continuation pass; returns (att, tok): the fp32 tensor [rows, L, n_heads, S] the pass fills
        (aigv_score_attention_arm) and - ``ld_tok`` > 0, ``return_token_attention``: aigv_score_attention_arm_tokens - the dense rows [rows, L,
        n_heads, ld_tok] the same pass fills, else None.  ``values`` (``return_score_values``: aigv_score_attention_arm_values) -> (att, tok, val),
        val the fp32 value vectors [rows, L, n_heads, S + 1, D] the same pass fills."""
        rows, seg_new, seg_cached, ld_cached, S = probe
        llm = self.config.llm_config
        att = torch.empty((len(rows), llm.num_hidden_layers, llm.num_attention_heads, S), dtype=torch.float32, device=self.device)
        lib, tok = native.load(), None
        args = (self._ctx, native.i32_array(rows), len(rows), seg_new.data_ptr(), native.ptr(seg_cached), int(ld_cached), int(S), att.data_ptr())
        if ld_tok:
            tok = torch.empty((len(rows), llm.num_hidden_layers, llm.num_attention_heads, int(ld_tok)), dtype=torch.float32, device=self.device)
        if values:
            val = torch.empty((len(rows), llm.num_hidden_layers, llm.num_attention_heads, S + 1, llm.head_dim), dtype=torch.float32, device=self.device)
            native.check(lib.aigv_score_attention_arm_values(*args, native.ptr(tok), int(ld_tok), val.data_ptr()), self._ctx)
            return att, tok, val
        if ld_tok:
            native.check(lib.aigv_score_attention_arm_tokens(*args, tok.data_ptr(), int(ld_tok)), self._ctx)
        else:
            native.check(lib.aigv_score_attention_arm(*args), self._ctx)
        return att, tok

    # ---- the depth lens (return_depth_lens) ---------------------------------------------------------------------------------------------
    def _depth_lens_rows(self, plan, with_tokens: bool):
        """(the packed score row of every clip - stage 2, else none; the clips that have an answer token; the packed row that predicts each one's
        first answer token: ``_probe_rows``' stage-1 rule, applied in both stages)."""
        score_rows = [int(r) for r in plan["score_rows"]] if plan["score_rows"] is not None else []
        clips, token_rows = [], []
        if with_tokens:
            answer = (plan["labels_h"][:, 1:] != -100) & (plan["row_of"][:, :-1] >= 0)
            for b in range(answer.shape[0]):
                at = answer[b].nonzero().flatten()
                if at.numel():
                    clips.append(b)
                    token_rows.append(int(plan["row_of"][b, int(at[0])]))
        if not score_rows and not token_rows:
            raise ValueError("return_depth_lens: nothing to read - a stage-1 model needs labels with an answer token (the lens reads the row that predicts the first one)")
        return score_rows, clips, token_rows

    def _depth_lens_buffers(self, score_rows, token_rows):
        """What ``_prefill`` arms the pass with (aigv_depth_lens_arm): the row lists and the three tensors the pass fills."""
        llm = self.config.llm_config
        D, n = llm.num_hidden_layers + 1, len(score_rows) + len(token_rows)
        hidden = torch.empty((D, n, llm.hidden_size), dtype=torch.bfloat16, device=self.device)
        normed = torch.empty_like(hidden)
        score = torch.empty((D, len(score_rows)), dtype=torch.float32, device=self.device) if score_rows else None
        return score_rows, token_rows, hidden, normed, score

    def _depth_lens_outputs(self, B, lens, clips, ro, with_tokens: bool) -> dict:
        """The ``lens_*`` entries of the result dict from the armed pass's buffers; the token read-outs through aigv_depth_lens_token_readout (one pass
        over the lm-head per 64 rows, top-1 and candidates from the same logits)."""
        score_rows, token_rows, hidden, normed, score = lens
        D, n, H = hidden.shape
        nS, nT = len(score_rows), len(token_rows)
        dev, out = self.device, {}
        if nS:
            out["lens_score"] = score.t().contiguous()                              # [B, L + 1]
            out["lens_score_hidden"] = hidden[:, :nS].transpose(0, 1).contiguous()    # [B, L + 1, H]
        if not with_tokens:                 # (without labels the token outputs are absent)
            return out
        C = 0 if ro.cand is None else int(ro.cand.numel())
        tok = torch.full((B, D), -1, dtype=torch.long, device=dev)
        lp = torch.full((B, D), float("nan"), dtype=torch.float32, device=dev)
        th = torch.zeros((B, D, H), dtype=torch.bfloat16, device=dev)
        cl = torch.full((B, D, C), float("nan"), dtype=torch.float32, device=dev) if C else None
        if nT:
            lib, ctx = native.load(), self._ctx
            rows = normed[:, nS:].contiguous()                                      # [L + 1, nT, H]: the token rows of every depth, dense
            top_id = torch.empty(D * nT, dtype=torch.long, device=dev)
            top_lp = torch.empty(D * nT, dtype=torch.float32, device=dev)
            cand_lp = torch.empty((D * nT, C), dtype=torch.float32, device=dev) if C else None
            native.check(lib.aigv_depth_lens_token_readout(ctx, rows.data_ptr(), H, D * nT, self._h2d(ro.cand).data_ptr() if C else None, C, top_id.data_ptr(),
                                                           top_lp.data_ptr(), native.ptr(cand_lp), native.stream_ptr()), ctx)
            at = self._h2d(torch.tensor(clips, dtype=torch.long))
            tok.index_copy_(0, at, top_id.view(D, nT).t().contiguous())
            lp.index_copy_(0, at, top_lp.view(D, nT).t().contiguous())
            th.index_copy_(0, at, hidden[:, nS:].transpose(0, 1).contiguous())
            if C:
                cl.index_copy_(0, at, cand_lp.view(D, nT, C).transpose(0, 1).contiguous())
        out.update(lens_token=tok, lens_token_logprob=lp, lens_token_hidden=th)
        if C:
            out["lens_cand_logprob"] = cl
        return out

    # ---- activation patching (return_stream / stream_patch) -------------------------------------------------------------------------------
    @staticmethod
    def _stream_rows(plan, mask: torch.Tensor):
        """A host bool mask [B, N] -> (host int32 [n]: the packed rows of the selected tokens the pass runs, ascending; host int64 [n, 2]: their
        (clip, position), clip-major and position-ascending - the same order).  Padded positions and a dropped dead tail are skipped through the
        plan's ``row_of``."""
        sel = mask & (plan["row_of"] >= 0)
        return plan["row_of"][sel].to(torch.int32).contiguous(), sel.nonzero().to(torch.long)

    @staticmethod
    def _patch_rows_check(name: str, n: int, patch, index) -> None:
        """What the three patch planners check alike - ``name`` is the option's: the values hold one row per token the mask selects in the pass (``n``), and a
        donor's ``index``, when given, lists exactly the pass's (clip, position) pairs (``index``).  ValueError: a count mismatch (both counts), the first
        differing pair."""
        if int(patch.values.shape[0]) != n:
            raise ValueError(f"{name}: values hold {int(patch.values.shape[0])} rows, the mask selects {n} tokens the pass runs")
        if patch.index is not None:
            if int(patch.index.shape[0]) != n:
                raise ValueError(f"{name}: index holds {int(patch.index.shape[0])} pairs, the mask selects {n} tokens the pass runs")
            differ = (patch.index != index).any(1).nonzero().flatten()
            if differ.numel():
                i = int(differ[0])
                raise ValueError(f"{name}: pair {i} of index is (clip, position) = {tuple(patch.index[i].tolist())}, the pass's is {tuple(index[i].tolist())}")

    def _model_sizes(self) -> dict:
        """The model's sizes under the names ``readouts.FAMILIES`` reads them by."""
        llm = self.config.llm_config
        return dict(n_layers=llm.num_hidden_layers, n_heads=llm.num_attention_heads, head_dim=llm.head_dim, n_inter=llm.intermediate_size, hidden=llm.hidden_size)

    # ---- the patches of the three families (stream_patch; head_patch: head patching; neuron_patch: neuron patching) -------------------------------
    def _patch_plan(self, fam, plan, patch):
        """A checked patch record of the family ``fam`` (a line of ``readouts.FAMILIES``) against the plan, host work only -> None (an empty window,
        an empty selection or an extra that selects nothing: the plain pass) or (packed rows, lo, hi, [the family's extra as the C ABI takes it or
        None,] the values as given).  ValueError: the values' width (where the family checks it here), a count mismatch (both counts), the first
        differing (clip, position)."""
        rows, index = self._stream_rows(plan, patch.rows)
        (lo, hi), v = getattr(patch, fam.word), patch.values
        want = tuple(size for _, size in fam.dims(self._model_sizes(), None))
        if fam.misfit is not None and tuple(v.shape[2:]) != want:
            raise ValueError(f"{fam.patch}: {fam.misfit(tuple(v.shape[2:]), want)}")
        n = int(rows.numel())
        self._patch_rows_check(fam.patch, n, patch, index)
        packed, any_selected = fam.pack(getattr(patch, fam.extra)) if fam.extra else (None, True)
        return (rows, lo, hi, *((packed,) if fam.extra else ()), v) if n and hi > lo and any_selected else None

    def _stream_patch_plan(self, plan, patch):
        return self._patch_plan(readouts.STREAM, plan, patch)

    def _head_patch_plan(self, plan, patch):
        return self._patch_plan(readouts.HEAD, plan, patch)

    def _neuron_patch_plan(self, plan, patch):
        return self._patch_plan(readouts.NEURON, plan, patch)

    def forward(self, mos: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
                input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                position_ids=None, image_flags: Optional[torch.Tensor] = None, past_key_values=None,
                labels: Optional[torch.Tensor] = None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, motion_feature: Optional[torch.Tensor] = None,
                visual_tokens: Optional[torch.Tensor] = None, full_logits: bool = False, return_logprobs: bool = False,
                candidate_ids=None, top_logprobs: Optional[int] = None, return_score_attention: bool = False, attention_segments=None,
                return_token_attention: bool = False, key_drop: Optional[torch.Tensor] = None, key_drop_rows: Optional[torch.Tensor] = None,
                key_drop_layers: Optional[tuple] = None, return_depth_lens: bool = False, return_stream: Optional[torch.Tensor] = None,
                stream_depths: Optional[tuple] = None, stream_patch: Optional[readouts.StreamPatch] = None, return_heads: Optional[torch.Tensor] = None,
                head_layers: Optional[tuple] = None, head_patch: Optional[readouts.HeadPatch] = None, head_scale: Optional[readouts.HeadScale] = None,
                return_neurons: Optional[torch.Tensor] = None, neuron_layers: Optional[tuple] = None, neuron_ids: Optional[torch.Tensor] = None,
                neuron_patch: Optional[readouts.NeuronPatch] = None, neuron_scale: Optional[readouts.NeuronScale] = None, return_score_values: bool = False,
                return_segment_attention: bool = False, return_row_attention: Optional[tuple] = None):
        """Stage-2 eval pass (modeling_internvl_chat.py:306-488) or, with ``stage=1``, the stage-1 pass
        (internvl_chat_eval1/modeling_internvl_chat.py:250-366).  ``visual_tokens`` optionally supplies
        already all-gathered pre-projector tokens (frame-DP) instead of ``pixel_values``.

        ``return_logprobs=True`` adds ``logprob`` (fp32 [B (N - 1)], laid out like ``label`` / ``logit``: log_softmax of the fp32-upcast
        bf16 logits at the shifted label, NaN wherever the label is -100) and ``ce_loss`` (fp32 0-dim: the reference's
        ``CrossEntropyLoss()(shift_logits, shift_labels)``, modeling_internvl_chat.py:452-463 - the mean over the non-ignored labels of the
        batch, NaN when there are none).  Labels must then be -100 or lie in [0, vocab), and no such label may follow a padded position
        (the reference would score the padded row itself): ValueError otherwise.  ``loss`` (stage 2: L1 against ``mos``) is unchanged.

        ``candidate_ids`` (LongTensor [C] or list, 1 <= C <= 64 token ids - ``prompts.level_token_ids``) adds ``cand_logprob`` (fp32
        [B (N - 1), C], rows laid out like ``logit`` / ``logprob``, NaN rows wherever the label is -100): column c is the FULL-vocabulary
        ``log_softmax(logits.float())[candidate_ids[c]]`` - bit for bit the ``logprob`` the pass gives with ``candidate_ids[c]`` as that
        row's label - so ``softmax(cand_logprob, -1)`` is the closed-set distribution over the candidates and
        ``eval_utils.expected_level`` its mean level, from ONE pass.  An id outside [0, vocab) gives a NaN column.  Needs ``labels`` (they
        say which rows are answer rows) under ``return_logprobs``' label rules, with or without ``return_logprobs``.  The ids are a device
        input of a replayed graph: other VALUES replay the same graph, another C is another graph.  fp8 mode: the lm-head stays bf16
        there, so the same kernels serve.

        ``top_logprobs=k`` (int, 1 <= k <= 16) adds what the model preferred at every answer row: ``top_ids`` (int64 [B (N - 1), k], -1
        rows wherever the label is -100) - the ids of the k largest bf16 logits, equal logits by ascending id, i.e. the first k of
        ``torch.sort(logits.float(), descending=True, stable=True)``; column 0 is ``logit`` - and ``top_logprob`` (fp32, same shape, NaN
        rows there): their full-vocabulary log-probabilities, bit for bit what ``candidate_ids=top_ids[row]`` gives.  Needs ``labels``
        under ``return_logprobs``' label rules.  The three options combine freely and none changes another's bits; under graph replay k
        is part of the graph's key (it is an output shape).

        ``return_score_attention=True`` adds ``score_attention`` (fp32 [B, L, n_heads, S]): where the clip's score row - ``hidden[:, -4]``;
        in a stage-1 model, which has no score head, the row that predicts the first answer token - looks in every layer and head, as the
        softmax mass it puts on each of S key segments.  Default segments (``prompts.attention_segments``, S = F + 4): frame 0 .. F - 1 |
        motion token | first token (the sink) | text up to the last visual token | text after it; a row's S values sum to 1.  Or pass
        ``attention_segments=`` (integer tensor like ``input_ids``; S = largest id + 1 <= 64; an id outside [0, S) drops its key from the
        bins but not from the softmax).  What the reference reads from ``output_attentions=True`` on its eager attention, here from a
        small stand-alone kernel per layer that recomputes that one row's softmax in fp32 from the layer's Q and K (the flash kernels
        never form a probability matrix): no other output of the pass changes a bit, and the option combines freely with the
        log-probability options.  ``eval_utils.frame_saliency`` folds it to [B, F].  Under graph replay the flag (and S) is part of the
        graph's key, a user table is a graph input, the tensor a graph output.

        ``return_token_attention=True`` (implies ``return_score_attention``) also adds ``score_attention_tokens`` (fp32 [B, L, n_heads, N], N =
        ``input_ids.shape[1]``): the same row's softmax per KEY, from the same launch per layer - column j is the clip's j-th un-masked token
        (``input_ids[b, j]`` for the collator's right-padded inputs), the columns behind the score row and the padding are 0.  The values
        share the bins' scores, total and division (a bin of one key holds that key's bits); ``score_attention`` and every other output
        keep their bits.  ``prompts.visual_token_positions`` + ``eval_utils.frame_heatmaps`` fold it to a 16 x 16 map per frame.  Under
        graph replay the flag and N are part of the graph's key; the tensor is handed back as a copy.

        ``return_score_values=True`` (implies ``return_score_attention``) - WHAT the row takes from each source: adds ``score_values`` (fp32 [B, L,
        n_heads, S, D]: ``sum over the keys j of segment s of softmax_j * v_j``, the head's attention output at the score row split by where it
        was read from, from the same launch per layer) and ``score_values_rest`` (fp32 [B, L, n_heads, D]: the keys outside every segment - all
        zeros with the default table); the two are views of one buffer, and ``score_values.sum(3) + score_values_rest`` is the head output the
        layer's ``wo`` consumes (``return_heads``) up to the flash kernel's bf16 roundings.  Attention mass is a poor proxy for contribution (a
        sink key holds mass and writes almost nothing); ``eval_utils.source_writes`` puts the vectors through ``wo`` - the norm of what every
        source writes into the score row's stream, or its projection on a direction - and ``eval_utils.frame_write_saliency`` folds the norms to
        [B, F] beside ``frame_saliency``.  ``score_attention``, ``score_attention_tokens`` and every other output keep their bits; combines
        with everything the probe combines with.  0 x Inf is NaN as in the attention itself: a non-finite V row makes its segment NaN.  At most
        64 clips; with graph replay enabled a call with the flag runs eagerly.

        ``return_segment_attention`` / ``return_row_attention`` - WHO READS WHOM (the attention flow map): the same bins for EVERY query row of the
        pass, not the score row alone, from a stand-alone MFMA kernel per layer that recomputes the causal softmax of all rows in fp32 from the
        layer's Q and K.  One table per call, shared with the probe: ``attention_segments=`` or the default; ``eval_utils.flow_segments`` is the
        default with the score row as a bin of its own (S = F + 5).  ``return_segment_attention=True`` adds ``segment_attention`` (fp32 [B, L,
        n_heads, S, S]: entry [a, c] is the mean, over the clip's query rows of segment a, of the mass a row puts on the keys of segment c - the
        rows added in ascending order in fp32, one division; a row of the matrix sums to 1 minus the mass on keys outside every bin; NaN where
        the clip has no token of segment a) and ``segment_rows`` (int64 [B, S]: the clip's query rows per segment).
        ``return_row_attention=(lo, hi)``, 0 <= lo <= hi <= L, adds ``row_attention`` (fp32 [B, hi - lo, n_heads, N, S]: the bins of every
        token at the layers lo <= l < hi; column n is the clip's n-th un-masked token, as in ``score_attention_tokens``; NaN at padding
        positions and at tokens the pass does not run) - B (hi - lo) n_heads N S 4 bytes, 14.5 MB per layer at the benched shape (4 clips of 8
        frames, 32 heads, N = 2177, S = 13 with ``flow_segments``), 0.46 GB for all 32 layers: size the window accordingly.  At the score row ``row_attention`` is ``score_attention`` up to summation
        order.  Under teacher forcing the rows of the answer tokens say which frames each answer token reads.  ``score_attention`` and every
        other output keep their bits with the map armed.  ValueError, before anything is launched: together with ``key_drop`` (the map does not
        know the mask), a window outside 0 <= lo <= hi <= L, more than 64 segments, more than 127 clips.  With graph replay enabled a call with either option runs
        eagerly and captures nothing.  ``forward_shared_prefix``, ``generate*``, ``eval_utils.batched`` and ``score_clips_dp`` do not take the
        options.  ``eval_utils.segment_flow`` folds the matrix over layers and heads, ``eval_utils.attention_rollout`` multiplies it through the
        depth (Abnar & Zuidema 2020).

        ``key_drop`` (bool or integer tensor [B, N] laid out like ``input_ids``, on any device): WHAT IF these tokens were not there.  True
        hides that token, as a key, from every row of its clip in every layer; padded positions are ignored.  Every output - ``score1``,
        ``logit``, the log-probability read-outs - is that of the masked pass; positions, packing and the dead-tail trimming are untouched.
        This is what the reference computes for ``attention_mask & ~key_drop``: zeros in the middle of its mask keep every token's position
        and hide those keys through the additive mask.  This path does NOT do that for interior zeros of ``attention_mask`` itself: it
        treats every zero as padding and strips the token, which moves the later tokens' positions - that behaviour stays.  The V rows of
        dropped keys must be finite: they are multiplied by an exact 0, and 0 x NaN is NaN here as it is in torch.  ValueError, before
        anything is launched, for a wrong shape, for dropping a clip's first token (the sink guarantees every row a visible key) or a
        consumed row (an answer row, the score row), and in combination with ``return_score_attention`` / ``return_token_attention`` / ``return_score_values`` (the
        probe does not know the mask).  With graph replay enabled a call with ``key_drop`` runs eagerly - the same bits as with replay
        off - and captures nothing; unmasked calls keep replaying.  ``unit_masks`` builds the per-frame masks,
        ``eval_utils.frame_ablation`` the per-frame score deltas.

        ``key_drop_rows`` / ``key_drop_layers`` qualify ``key_drop`` - WHICH WAY, AT WHICH DEPTH a token's content travels (the attention
        knock-out): with ``key_drop_rows`` (bool or integer tensor [B, N] like ``input_ids``) only those query rows are cut from the dropped
        keys, with ``key_drop_layers=(lo, hi)``, 0 <= lo <= hi <= L, only in the layers lo <= l < hi; every other edge and every other layer
        is untouched.  What the reference computes when the additive mask of those layers also holds ``finfo.min`` at every (row r, key j) with
        ``key_drop_rows[b, r] and key_drop[b, j]``.  Left at None they change nothing: every row, every layer.  ValueError, before anything
        is launched: either one without ``key_drop``; a wrong shape or window; a token that is both a dropped key and a selected row (a row is
        never cut from itself) - under ``key_drop_rows`` a consumed row MAY then be a dropped key; the first token never.  Empty rows, empty
        keys or an empty window give the plain pass's bits.  ``segment_masks`` builds the usual groups (frames, text after them, the score
        row), ``eval_utils.flow_knockout`` the score deltas per path and layer window.

        ``return_depth_lens=True`` - AT WHICH DEPTH the score exists (the logit lens): the residual stream of two rows per clip after every
        layer, through the model's own final norm and its own heads.  With L layers, depth d = 0 is the embedding, depth d the stream after d
        layers, depth L what the final norm consumes.  Stage 2 adds ``lens_score`` (fp32 [B, L + 1]: the score head on the final norm of the
        score row at depth d, its NaN guard taken over the batch's B score rows of that depth; column L is ``score1``, bit for bit) and
        ``lens_score_hidden`` (bf16 [B, L + 1, H]: that row's raw, un-normed residual).  With ``labels`` either stage adds, for the row that
        predicts the clip's first answer token: ``lens_token`` (int64 [B, L + 1]: the most likely token under final norm + lm-head at depth d,
        equal logits by the lower id, -1 for a clip without an answer token; column L is ``logit`` at that row), ``lens_token_logprob`` (fp32
        [B, L + 1]: its full-vocabulary log-probability, NaN where the token is -1; column L is ``top_logprob[row, 0]``),
        ``lens_token_hidden`` (bf16 [B, L + 1, H], zeros for such a clip) and - with ``candidate_ids`` - ``lens_cand_logprob`` (fp32 [B, L + 1,
        C]: the candidates' columns of the same log-softmax; depth L is ``cand_logprob[row]``).  ``top_logprobs`` does not extend to the lens.
        The lens reads the stream, not the attention: no other output changes a bit, and it combines with every other option, ``key_drop``
        and its qualifiers (the lens of the masked pass) and the probe included.  At most 64 clips per pass.  Under graph replay the flag is
        part of the graph's key; with ``key_drop`` the call runs eagerly as it does without the lens.  ``eval_utils.settling_depth`` folds
        ``lens_score`` to the depth from which the score stays put.

        ``return_stream`` / ``stream_patch`` - WHERE THE QUALITY LIVES (activation patching, causal tracing): rows of the residual stream copied out
        of the pass, or overwritten in it, by depth.  Depth d, 0 <= d < L, is the stream layer d CONSUMES: d = 0 the embedding with the visual and
        motion tokens in place, depth d the stream after d layers (the lens' numbering; depth L is not offered - the lens reads it).
        ``return_stream`` (bool or integer tensor [B, N] laid out like ``input_ids``, on any device) with ``stream_depths=(lo, hi)`` (default (0,
        L)) adds ``stream`` (bf16 [n, hi - lo, H]: the selected tokens' rows at the depths lo <= d < hi) and ``stream_index`` (int64 [n, 2]: each
        one's (clip, position), clip-major and position-ascending).  Padded positions and tokens the pass does not run (the dead tail behind a
        clip's last consumed row) are skipped: ``stream_index`` says what was captured; an empty selection gives n = 0.
        ``stream_patch=readouts.StreamPatch(rows, values, depths, index=None)``: immediately before each layer d of ``depths`` = (lo, hi) runs, the
        rows of the tokens ``rows`` selects are overwritten with ``values`` (bf16 [n, hi - lo, H], on the device or the host, laid out exactly like
        the ``stream`` a capture with that mask and those depths returns) - a bit copy: NaN and Inf payloads travel unchanged.  What the reference
        computes when a forward pre-hook on ``language_model.model.layers[d]`` assigns ``hidden_states[b, pos] = value``.  Every output -
        ``score1``, ``logit``, the log-probability read-outs, the lens, a capture (which reads the stream as the layer consumes it, after the
        patch) - is that of the patched pass.  ValueError, before anything is launched: a wrong shape or window, ``stream_depths`` without
        ``return_stream``, n other than the number of selected tokens the pass runs (both counts are named), and - with ``index``, a donor's
        ``stream_index`` - the first (clip, position) pair that differs from the recipient's.  An empty window or selection gives the plain
        pass's bits.  Steering: capture a row, add a direction in torch, patch it back.  The two options combine with each other and with every
        other option, fp8 mode included.  With graph replay enabled a call carrying either runs eagerly and captures nothing, as a masked call
        does.  ``eval_utils.causal_trace`` runs the donor / recipient sweep over token groups and depth windows.

        ``return_heads`` / ``head_patch`` / ``head_scale`` - WHICH HEADS (head knock-out, Michel et al. 2019; head patching / path patching, Wang et
        al. 2022): the per-head attention outputs of layer l, 0 <= l < L - the row that layer's ``wo`` consumes, bf16 [n_heads, D] per token, what a
        forward pre-hook on ``layers[l].attention.wo`` sees - copied out, overwritten, or multiplied by a factor per head.  Inside a layer the
        order is: attention, scale, patch, capture, ``wo``; a capture armed beside the other two returns what ``wo`` consumes, and every later
        layer, the lens, a stream capture and all heads see the modified pass.  ``return_heads`` (bool or integer tensor [B, N] laid out like
        ``input_ids``) with ``head_layers=(lo, hi)`` (default (0, L)) adds ``heads`` (bf16 [n, hi - lo, n_heads, D]) and ``heads_index`` (int64
        [n, 2]); rows are selected exactly as ``return_stream`` selects them.  ``head_patch=readouts.HeadPatch(rows, values, layers, index=None,
        heads=None)``: ``values`` laid out like a capture; only the columns of the heads ``heads`` selects (bool [n_heads] or [hi - lo, n_heads];
        None: all) are overwritten - a bit copy, NaN payloads travel unchanged; an unselected head is neither read nor written.
        ``head_scale=readouts.HeadScale(scale, rows=None)``: ``scale`` a float tensor [L, n_heads]; over the query rows ``rows`` selects (None:
        every row the pass runs) head h of layer l becomes ``bf16(fp32(x) * scale[l, h])``, round to nearest even - what ``(x.float() *
        s).to(torch.bfloat16)`` gives.  An entry that is exactly 1.0 leaves its head untouched; scale 0 is the head knock-out.  0 x Inf is NaN, as
        in torch: a head whose output holds an Inf (or a NaN) is not silenced by a zero - as ``key_drop`` does not silence a NaN in a V row it
        still reads.  A NaN in ``scale`` is a ValueError, as are a wrong shape or window, ``head_layers`` without ``return_heads``, a count
        mismatch (both counts named), the first differing (clip, position) pair, and a model of more than 64 query heads - all before anything is
        launched.  In the row-trimmed last layer a capture makes the attention launch cover every row (the consumed rows keep their bits), so a
        capture never returns unwritten memory; a patch or scale of a row the last layer does not consume has no effect.  The options combine with
        each other and with every other option, fp8 mode included; under graph replay a call carrying one runs eagerly.
        ``eval_utils.head_knockout`` and ``eval_utils.head_trace`` run the sweeps over (layer, head).

        ``return_neurons`` / ``neuron_patch`` / ``neuron_scale`` - WHICH MLP, WHICH NEURONS (causal tracing, Meng et al. 2022; neuron ablation, Geva
        et al. 2021, Dai et al. 2022): the neurons of layer l, 0 <= l < L - the row that layer's ``w2`` consumes, the output of the fused SwiGLU,
        bf16 [I] per token, what a forward pre-hook on ``layers[l].feed_forward.w2`` sees - copied out, overwritten, or multiplied by a factor.
        Inside a layer the order is: ``w1|w3`` + SwiGLU, scale, patch, capture, ``w2``; a capture armed beside the other two returns what ``w2``
        consumes, and every later layer, the lens, a stream capture and a head capture see the modified pass.  ``return_neurons`` (a mask like
        ``return_heads``) with ``neuron_layers=(lo, hi)`` (default (0, L)) adds ``neurons`` (bf16 [n, hi - lo, I]) and ``neurons_index`` (int64
        [n, 2]); ``neuron_ids`` (integer tensor [m], strictly ascending, m <= 4096) narrows it to those neurons: bf16 [n, hi - lo, m] - the sparse
        form, which is what makes a capture of every frame row at every layer affordable (a dense one is 2 I bytes per row and layer: sized by the
        caller).  ``neuron_patch=readouts.NeuronPatch(rows, values, layers, index=None, neurons=None)``: ``values`` laid out like a capture; a bit
        copy, NaN payloads travel unchanged; a neuron not listed is neither read nor written.  ``neuron_scale=readouts.NeuronScale(scale,
        neurons=None, rows=None)``: ``scale`` float [L] - every neuron of layer l becomes ``bf16(fp32(x) * scale[l])``, 0 the MLP-block knock-out -
        or, with ``neurons`` long [m, 2] of unique (layer, neuron) pairs, float [m]; over ``rows`` (None: every row the pass runs).  A factor of
        exactly 1.0 touches nothing; 0 x Inf is NaN, as in torch.  A NaN factor, a wrong shape or window, a list that is not strictly ascending or
        longer than 4096, a qualifier without ``return_neurons``, a count mismatch (both counts named) and the first differing (clip, position)
        pair are ValueErrors before anything is launched.  THE ROW-TRIMMED LAST LAYER is not un-trimmed: the value captured, patched or scaled for
        a row is the input of the ``w2`` launch whose output the pass keeps for it; when layer L - 1 runs for the consumed rows only (the score
        row and the answer rows), any other selected row has no MLP activation there - a patch or scale of it does nothing and its captured
        (row, L - 1) slice is NaN, as ``logprob`` is where there is no label.  The options combine with each other and with every other option,
        fp8 mode included; under graph replay a call carrying one runs eagerly.  ``eval_utils.mlp_knockout``, ``eval_utils.neuron_knockout`` and
        ``eval_utils.neuron_trace`` run the sweeps.

        Of several faults in one call the first in this order is raised: every check that needs no plan (``readouts.ReadOuts.parse``: the clip count
        of ``return_score_values``, the key-drop options, the stream, head and neuron options, ``candidate_ids``, ``top_logprobs``, the clip count of
        ``return_depth_lens``), then the token plan's own checks and those against it (key-drop, the stream, head and neuron patches, the lens' rows)."""
        if position_ids is not None or past_key_values is not None:
            raise NotImplementedError("the eval pass takes default positions and no cache, like the reference drivers")
        if self.img_context_token_id is None:
            raise AssertionError("img_context_token_id must be set by the caller (stage2_eval.py:810)")
        llm, sizes = self.config.llm_config, self._model_sizes()
        # every option, checked once, before anything needs a plan or touches the device; every later step reads the record
        ro = readouts.ReadOuts.parse(
            llm.vocab_size, labels, return_logprobs=return_logprobs, candidate_ids=candidate_ids, top_logprobs=top_logprobs,
            return_score_attention=return_score_attention, attention_segments=attention_segments, return_token_attention=return_token_attention,
            return_score_values=return_score_values, key_drop=key_drop, key_drop_rows=key_drop_rows, key_drop_layers=key_drop_layers,
            return_depth_lens=return_depth_lens, return_stream=return_stream, stream_depths=stream_depths, stream_patch=stream_patch,
            return_heads=return_heads, head_layers=head_layers, head_patch=head_patch, head_scale=head_scale, return_neurons=return_neurons,
            neuron_layers=neuron_layers, neuron_ids=neuron_ids, neuron_patch=neuron_patch, neuron_scale=neuron_scale,
            return_segment_attention=return_segment_attention, return_row_attention=return_row_attention,
            ids_shape=None if input_ids is None else input_ids.shape, n_layers=sizes["n_layers"], n_heads=sizes["n_heads"], head_dim=sizes["head_dim"],
            n_inter=sizes["n_inter"])
        drop_words = drop_row_words = None
        built = []

        def host_plan():    # the host plan of this call, built on first use: by the first option below that is checked against it, else by the eager pass
            if not built:
                src = visual_tokens if visual_tokens is not None else pixel_values
                built.append(self._plan(input_ids, attention_mask, labels, image_flags, (src.tokens if isinstance(src, VisualAhead) else src).shape[0], full_logits))
            return built[0]
        # the checks against the plan, host work only (the eager pass below, which such a call takes, reuses the plan): key_drop in full, ...
        if ro.key_drop is not None:
            drop_words = self._key_drop_words(host_plan(), ro.key_drop, ro.key_drop_rows)
            if ro.key_drop_rows is not None:
                drop_words, drop_row_words = drop_words
        # ... a patch's counts and pairs, ...
        patched = {fam.patch: self._patch_plan(fam, host_plan(), getattr(ro, fam.patch)) for fam in readouts.FAMILIES if getattr(ro, fam.patch) is not None}
        map_table = self._attention_map_table(host_plan(), input_ids, ro) if ro.attention_map is not None else None     # ... the map's bin count, ...
        if ro.depth_lens and self._capture_keep is None:      # ... and the lens: is there a row to read?  (inside a capture the call that led here has checked)
            self._depth_lens_rows(host_plan(), labels is not None)
        pixel_values, visual_tokens, motion_feature = self._take_ahead(pixel_values, visual_tokens, motion_feature)
        if self._graph_replay_enabled and self._capture_keep is None:
            # (a masked call stays eager and leaves the graph cache as it is: capturing masked passes is out of scope)
            # (so does a call that captures or patches the residual stream, or captures, patches or scales head outputs or MLP neurons, or returns score values)
            out = None if ro.runs_eagerly else self._forward_through_graph(mos, pixel_values, input_ids, attention_mask, image_flags, labels,
                                                                                  motion_feature, visual_tokens, full_logits, ro)
            if out is not None:
                return out
        B, N = input_ids.shape
        n_frames = visual_tokens.shape[0] if visual_tokens is not None else pixel_values.shape[0]
        # ---- index bookkeeping first, on the host (one small D2H copy if the ids live on the device), so that
        # every kernel of the step can then be enqueued back to back without a host sync in between ----
        plan = host_plan()
        lp_labels = self._logprob_labels(plan) if ro.wants_labels else None
        lens_rows = self._depth_lens_rows(plan, labels is not None) if ro.depth_lens else None
        motion_feature = self._motion_feature(pixel_values, B, motion_feature)

        # ---- device work: ViT -> projector -> motion projector -> LLM pass + heads ----
        self._native(n_frames=n_frames, n_tokens=plan["cu"][-1], n_clips=B, out_rows=len(plan["logit_rows"]), seq_len=N)   # size workspaces once
        vit_embeds, motion = self._visual_inputs(pixel_values, visual_tokens, motion_feature, plan)
        probe = self._score_attention_probe(plan, input_ids, ro) if ro.score_attention else None
        lens = None if lens_rows is None else self._depth_lens_buffers(lens_rows[0], lens_rows[2])
        amap = None if map_table is None else self._attention_map_buffers(plan, *map_table, ro.attention_map)
        armed, captured = {}, []    # what ``_prefill`` arms the pass with, by its keyword; (result name, buffer, (clip, position) index) of every capture
        for fam in readouts.FAMILIES:
            mask, p, q = getattr(ro, fam.rows), patched.get(fam.patch), getattr(ro, fam.scale) if fam.scale else None
            if mask is not None:    # a capture: (packed rows, lo, hi, [the further qualifier as the C ABI takes it,] the bf16 buffer the pass fills [n, hi - lo, *dims])
                ids = getattr(ro, fam.ids) if fam.ids else None
                rows, index = self._stream_rows(plan, mask)
                lo, hi = getattr(ro, fam.window)
                buf = torch.empty((int(rows.numel()), hi - lo, *(size for _, size in fam.dims(sizes, ids))), dtype=torch.bfloat16, device=self.device)
                if fam.trimmed_last and lo < hi == llm.num_hidden_layers and buf.numel():
                    buf[:, -1].fill_(float("nan"))      # a selected row the row-trimmed last layer does not consume has no activation there: no launch writes its slice
                captured.append((fam.result, buf, index))
                if buf.numel():     # (an empty capture arms nothing: its empty buffer is the result)
                    armed[fam.name + "_capture"] = (rows, lo, hi, *((fam.pack(ids)[0],) if fam.ids else ()), buf)
            if p is not None:       # a patch, checked against this very plan on the way in: its values go up (or stay) on the device
                armed[fam.patch] = p[:-1] + (self._h2d(p[-1].detach().contiguous()),)
            if q is not None and bool((q.scale != 1).any()):      # (factors of one: the plain pass)
                rows = None if q.rows is None else self._stream_rows(plan, q.rows)[0]
                if rows is None or rows.numel():
                    armed[fam.scale] = (rows, *fam.scale_args(q))
        score, amax, *probed = self._prefill(plan["ids_packed"], plan["slot"], plan["cu"], vit_embeds, plan["n_vis"], motion,
                                             plan["score_rows"], plan["logit_rows"], probe=probe, ld_tok=N if ro.token_attention else 0, values=ro.score_values,
                                             drop_words=drop_words, drop_row_words=drop_row_words, drop_layers=ro.key_drop_layers, lens=lens,
                                             attention_map=amap if amap is not None and (amap[3] is not None or amap[4] is not None) else None, **armed)   # (an empty window alone arms nothing)
        att, tok, *val = probed or (None, None)  # (_prefill hands the probe's tensors back only when it armed one)
        reads = self._read_rows(B if score is not None else 0, len(plan["logit_rows"]), ro, lp_labels)
        out = self._outputs(plan, B, N, score, amax, mos, reads, att, tok, *val)
        if lens is not None:
            out.update(self._depth_lens_outputs(B, lens, lens_rows[1], ro, labels is not None))
        for name, buf, index in captured:
            out.update({name: buf, name + "_index": self._h2d(index)})
        if amap is not None:
            out.update(self._attention_map_outputs(plan, N, map_table[0], amap, ro.attention_map))
        return out

    def dp_front(self, frames_local: torch.Tensor, frames_clips: Optional[torch.Tensor], n_clips: int):
        """The data-parallel scorer's front half on this rank (dist_utils.score_clips_dp): the SlowFast feature of its own clips (side
        stream) beside the InternViT tokens of its frame shard -> (tokens [F_local, ntok, 4 Hv], motion feature [n_clips, motion_dim] or
        None).  With graph replay enabled the two run as ONE captured graph (joined at its end); the token all-gather and the projector +
        InternLM2 half (``forward(visual_tokens=...)``, a graph of its own) follow on the host's side of the collective."""
        self._wait_for_prefetch()

        def fn(fl, fc):
            mf = self._motion_feature(fc, n_clips, None) if fc is not None else None
            tok = self.vit_tokens(fl)
            self._join_side_stream()
            return tok, mf
        if (self._graph_replay_enabled and self._capture_keep is None and frames_local.is_cuda and not self._dirty and self._ctx is not None
                and not getattr(self, "_prof_on", False) and (frames_clips is None or (frames_clips.is_cuda and hasattr(self.slowfast_model, "features")))):
            self._prepare_motion_branch(frames_clips, int(n_clips))
            out = self._graph_call(("dp_front", int(n_clips), self._branch_uid(), bool(getattr(self, "overlap_motion_branch", True))),
                                   [frames_local, frames_clips], fn, clone_outputs=False)
            if out is not None:
                return out
        if frames_clips is None:
            return self.vit_tokens(frames_local), None
        mf = self.motion_feature_async(frames_clips, n_clips)       # eager: joined where forward() consumes it
        return self.vit_tokens(frames_local), mf

    def prefetch(self, pixel_values: Optional[torch.Tensor] = None, frames_u8: Optional[torch.Tensor] = None, n_clips: int = 1) -> VisualAhead:
        """Start the visual front of a LATER ``forward`` call NOW, on a stream of its own: frame ingest (when ``frames_u8`` [F, H, W, 3] is
        given: H2D copy + Pillow-exact resize + normalise), InternViT + pixel-shuffle, and the SlowFast branch of the ``n_clips`` clips -
        everything that depends on the frames only.  The returned handle is passed to ``forward`` as ``pixel_values``; that call waits for
        the handle's event and runs projector + InternLM2 + heads.  In an eval loop that scores one clip per call (stage2_eval.py:908-941)
        the next clip's visual front then runs BESIDE the current clip's InternLM2 pass, whose wo / w2 launches leave half the CUs idle at
        one clip (``eval_utils.lookahead`` wraps a loop that way).  Same kernels, same bits as the plain call; the InternViT workspaces of
        the context serve one visual front at a time, so a prefetch waits for the previous one.  (HIP deals a process's streams round-robin onto a
        few hardware queues: should the prefetch stream land on the queue of the caller's stream, the two serialise and the loop runs at the plain
        loop's speed - with the same results.)"""
        if (pixel_values is None) == (frames_u8 is None):
            raise ValueError("prefetch takes pixel_values or frames_u8")
        cur = torch.cuda.current_stream(self.device)
        look = getattr(self, "_look_stream", None)
        if look is None:
            look = self._look_stream = torch.cuda.Stream(device=self.device)
        look.wait_stream(cur)                       # inputs produced on the caller's stream; the previous prefetch is ordered by the stream itself
        with torch.cuda.stream(look):
            pv = self.ingest_frames(frames_u8) if frames_u8 is not None else pixel_values.to(device=self.device, dtype=torch.bfloat16)
            need_motion = self.slowfast_model is not None and hasattr(self.slowfast_model, "features")
            tok, mf = self.dp_front(pv, pv if need_motion else None, n_clips)
            self._join_side_stream()                # (the eager SlowFast branch forks from and joins back into this stream)
            tok = tok.clone()                       # (a replayed graph hands out its own output buffers: the next prefetch overwrites them)
            mf = None if mf is None else mf.clone()
            ev = torch.cuda.Event()
            ev.record(look)
        for t in ([pixel_values] + (list(frames_u8) if isinstance(frames_u8, (list, tuple)) else [frames_u8])):
            if t is not None and t.is_cuda:
                t.record_stream(look)
        tok.record_stream(cur)
        if mf is not None:
            mf.record_stream(cur)
        return VisualAhead(tok, mf, ev, n_clips)

    def _plan(self, input_ids, attention_mask, labels, image_flags, n_frames, full_logits=False, drop_dead_tail=None):
        """Host-side token bookkeeping of one pass: packed ids, which packed row takes which visual / motion token
        (modeling_internvl_chat.py:351-378), and the rows whose outputs are consumed."""
        B, N = input_ids.shape
        ids_h = input_ids.detach().to("cpu")
        mask_h = attention_mask.detach().to("cpu") if attention_mask is not None else None
        labels_h = labels.detach().to("cpu") if labels is not None else torch.full_like(ids_h, -100)
        flags_h = image_flags.detach().to("cpu").squeeze(-1) if image_flags is not None else None
        ids_packed, cu, row_of = self._pack(ids_h, mask_h)
        lens = [cu[i + 1] - cu[i] for i in range(B)]
        sel = ids_packed == self.img_context_token_id
        seq_of = torch.repeat_interleave(torch.arange(B), torch.tensor(lens))
        # last <IMG_CONTEXT> of each clip <- motion token; the others, in order <- visual tokens (:351-378)
        pos_idx = torch.arange(ids_packed.numel())
        last_pos = torch.full((B,), -1, dtype=torch.long)
        last_pos.scatter_reduce_(0, seq_of[sel], pos_idx[sel], reduce="amax")
        if bool((last_pos < 0).any()):
            raise ValueError("every clip needs at least one <IMG_CONTEXT> token")
        is_motion = torch.zeros_like(sel)
        is_motion[last_pos] = True
        vis_sel = sel & ~is_motion
        keep = torch.arange(n_frames) if flags_h is None else (flags_h == 1).nonzero().flatten()
        n_vis = int(keep.numel()) * self.num_image_token
        if int(vis_sel.sum()) != n_vis:
            raise ValueError(f"visual token count mismatch: {int(vis_sel.sum())} <IMG_CONTEXT> slots vs {n_vis} visual tokens")
        slot = torch.full_like(ids_packed, -1, dtype=torch.int32)
        slot[vis_sel] = torch.arange(n_vis, dtype=torch.int32)
        slot[is_motion] = n_vis + seq_of[is_motion].to(torch.int32)
        # rows whose next-token argmax is consumed: shifted positions p with labels[p+1] != -100
        if full_logits:
            want = row_of[:, :-1] >= 0
        else:
            want = (labels_h[:, 1:] != -100) & (row_of[:, :-1] >= 0)
        logit_rows = row_of[:, :-1][want].tolist()
        score_rows = [cu[i + 1] - 4 for i in range(B)] if self.stage == 2 else None
        if score_rows is not None and min(lens) < 4:
            raise ValueError("clips need at least 4 tokens for the score row hidden[:, -4]")
        # Dead trailing tokens: with causal attention a token influences only later rows, so whatever follows a clip's last
        # consumed row (the closing <|im_end|>, whose own logits the reference drops with shift_logits = logits[:, :-1],
        # modeling_internvl_chat.py:451-455) changes no returned value.  Such text tokens are not run at all - for the
        # canonical clip 2177 -> 2176 = 17 x 128 rows, which also removes the ragged row tile / query block of every kernel.
        if drop_dead_tail is None:
            drop_dead_tail = getattr(self, "drop_dead_tail", True)
        if drop_dead_tail and not full_logits:
            last_needed = [cu[b] for b in range(B)]
            for r in logit_rows + (score_rows or []):
                b = int(seq_of[r])
                last_needed[b] = max(last_needed[b], r + 1)
            keep_row = torch.zeros(ids_packed.numel(), dtype=torch.bool)
            for b in range(B):
                end = max(last_needed[b], cu[b] + 1)
                if bool((slot[end:cu[b + 1]] >= 0).any()):      # never drop a visual / motion slot
                    end = cu[b + 1]
                keep_row[cu[b]:end] = True
            if not bool(keep_row.all()):
                new_index = torch.cumsum(keep_row.long(), 0) - 1
                remap = lambda rows: [int(new_index[r]) for r in rows]
                logit_rows = remap(logit_rows)
                score_rows = remap(score_rows) if score_rows is not None else None
                last_pos = new_index[last_pos]
                kept = keep_row.nonzero().flatten()
                row_of = torch.where(row_of >= 0, torch.where(keep_row[row_of.clamp_min(0)], new_index[row_of.clamp_min(0)], torch.full_like(row_of, -1)), row_of)
                ids_packed, slot, seq_of = ids_packed[kept], slot[kept], seq_of[kept]
                lens = [int((seq_of == b).sum()) for b in range(B)]
                cu = list(accumulate(lens, initial=0))
        return dict(ids_h=ids_h, mask_h=mask_h, labels_h=labels_h, flags_h=flags_h, ids_packed=ids_packed, cu=cu, row_of=row_of,
                    lens=lens, slot=slot, n_vis=n_vis, keep=keep, n_frames=n_frames, want=want, logit_rows=logit_rows,
                    score_rows=score_rows, last_ctx=(last_pos - torch.tensor(cu[:-1])).tolist())

    def _visual_inputs(self, pixel_values, visual_tokens, motion_feature, plan):
        H = self.config.llm_config.hidden_size
        if visual_tokens is None:
            visual_tokens = self.vit_tokens(pixel_values)
        vit_embeds = self.project(visual_tokens)                       # [F, ntok, H]
        if plan["flags_h"] is not None and int(plan["keep"].numel()) != plan["n_frames"]:
            vit_embeds = vit_embeds[self._h2d(plan["keep"])]
        return vit_embeds.reshape(-1, H), self.motion_embed(motion_feature)

    def _outputs(self, plan, B, N, score, amax, mos, reads, att=None, tok=None, val=None):
        """The result dict of one pass: ``reads`` (``_read_rows``) and the argmax ids, each scattered to its place among the label positions
        under its ``readouts.ROW_FIELDS`` fill, the score head's outputs and the probe's tensors."""
        dev = self.device
        up = self._h2d   # host -> device through pinned memory, never blocking the host (keeps the CPU ahead of the GPU)
        idx = up(plan["want"].reshape(-1).nonzero().flatten()) if len(plan["logit_rows"]) else None   # index list built on the host: no sync

        def scatter(rows, fill):
            """Per-consumed-row values -> their places among the B (N - 1) label positions, ``fill`` everywhere else."""
            full = torch.full((B * (N - 1),) + tuple(rows.shape[1:]), fill, dtype=rows.dtype, device=dev)
            return full if idx is None else full.index_copy_(0, idx, rows)

        rows = dict(reads, logit=amax)
        answer = None
        if "top_ids" in rows:                       # top_logprobs: -1 / NaN rows wherever the label is -100, also under full_logits
            is_answer = plan["labels_h"][..., 1:][plan["want"]] != -100      # (host: no sync)
            if not bool(is_answer.all()):
                answer = up(is_answer).view(-1, 1)
        out = {"label": up(plan["labels_h"][..., 1:].contiguous().view(-1))}
        for name, member, _, fill in readouts.ROW_FIELDS:
            if name in rows:
                r = rows[name]
                if member == "topk" and answer is not None:
                    r = torch.where(answer, r, torch.full_like(r, fill))
                out[name] = scatter(r, fill)
        if self.stage == 2:
            score1 = score.to(torch.bfloat16)       # the head computes in bf16; the value is exact in fp32
            out["score1"] = score1
            out["loss"] = F.l1_loss(score1, mos.to(dev).to(score1.dtype)) if mos is not None else None
        if "logprob" in out:                        # return_logprobs
            out["ce_loss"] = readouts.ce_loss(out["logprob"], plan["labels_h"][..., 1:], up)
        if att is not None:                         # return_score_attention: [B, L, n_heads, S]
            out["score_attention"] = att
        if tok is not None:                         # return_token_attention: [B, L, n_heads, N]
            out["score_attention_tokens"] = tok
        if val is not None:                         # return_score_values: [B, L, n_heads, S + 1, D], slot S = the keys outside every segment
            out["score_values"], out["score_values_rest"] = val[..., :-1, :], val[..., -1, :]
        return out

    def _logprob_labels(self, plan) -> torch.Tensor:
        """Host int64 labels of the pass's consumed rows (in ``logit_rows`` order), checked first as torch's cross entropy would."""
        lab = plan["labels_h"][:, 1:].to(torch.long)
        V = self.config.llm_config.vocab_size
        scored = lab != -100
        bad = scored & ((lab < 0) | (lab >= V))
        if bool(bad.any()):
            raise ValueError(f"return_logprobs: label {int(lab[bad][0])} is outside [0, {V}) and not the ignore index -100")
        if bool((scored & ~plan["want"]).any()):
            raise ValueError("return_logprobs: a label that is not -100 follows a padded (masked) position; the reference would score the "
                             "padded row itself, which this path does not run - set such labels to -100")
        return lab[plan["want"]].contiguous()

    def _read_rows(self, first_row: int, R: int, ro, labels: Optional[torch.Tensor] = None) -> dict:
        """Every per-row read-out ``ro`` asks for, of consumed rows first_row .. first_row + R - 1 of the last native pass, keyed by its
        ``readouts.ROW_FIELDS`` name: ``logprob`` fp32 [R], the log-probabilities of ``labels`` (int64 [R], aigv_out_row_logprob); ``cand_logprob``
        fp32 [R, C] of the candidates ``ro.cand`` (int64 [C], aigv_out_row_cand_logprob); ``top_ids`` int64 [R, k] / ``top_logprob`` fp32 [R, k]
        (aigv_out_row_topk_logprob): the k largest bf16 logits of every row, equal logits by ascending id, under the same log-sum-exp.
        Host tensors go up through pinned memory, device tensors are read where they are - no host sync, and no allocation inside the library
        (the pass may be captured)."""
        lib, ctx, first_row = native.load(), self._ctx, int(first_row)
        out = {name: torch.empty((max(R, 1),) + width, dtype=dt, device=self.device)[:R] for name, width, dt, _ in ro.row_fields() if name != "logit"}
        if R and ro.logprobs:
            native.check(lib.aigv_out_row_logprob(ctx, first_row, R, self._h2d(labels).data_ptr(), out["logprob"].data_ptr(), native.stream_ptr()), ctx)
        if R and ro.cand is not None:
            native.check(lib.aigv_out_row_cand_logprob(ctx, first_row, R, self._h2d(ro.cand).data_ptr(), int(ro.cand.numel()), out["cand_logprob"].data_ptr(),
                                                       native.stream_ptr()), ctx)
        if R and ro.topk:
            native.check(lib.aigv_out_row_topk_logprob(ctx, first_row, R, int(ro.topk), out["top_ids"].data_ptr(), out["top_logprob"].data_ptr(),
                                                       native.stream_ptr()), ctx)
        return out

    @staticmethod
    def _shared_prefix_lengths(plans, B: int) -> List[int]:
        """Per clip: the number of leading tokens every prompt shares, capped so that every consumed row (answer rows, score
        row) stays in the continuation; raises if the prompts diverge before the last <IMG_CONTEXT> token (host logic only)."""
        pre = []
        for b in range(B):
            seqs = [pl["ids_packed"][pl["cu"][b]:pl["cu"][b + 1]] for pl in plans]
            n = min(len(x) for x in seqs)
            eq = torch.ones(n, dtype=torch.bool)
            for x in seqs[1:]:
                eq &= x[:n] == seqs[0][:n]
            lcp = int(n if bool(eq.all()) else eq.long().argmin())
            first_needed = []
            for pl in plans:
                rows = [r - pl["cu"][b] for r in pl["logit_rows"] if pl["cu"][b] <= r < pl["cu"][b + 1]]
                if pl["score_rows"] is not None:
                    rows.append(pl["score_rows"][b] - pl["cu"][b])
                first_needed.append(min(rows) if rows else pl["lens"][b] - 1)
            p_b = min([lcp] + first_needed + [pl["lens"][b] - 1 for pl in plans])
            if p_b <= max(pl["last_ctx"][b] for pl in plans):
                raise ValueError(f"clip {b}: the prompts diverge before the last <IMG_CONTEXT> token - no shared video prefix")
            pre.append(p_b)
        return pre

    def forward_shared_prefix(self, prompts, pixel_values: Optional[torch.Tensor] = None, image_flags: Optional[torch.Tensor] = None,
                              motion_feature: Optional[torch.Tensor] = None, visual_tokens: Optional[torch.Tensor] = None, mos=None,
                              return_logprobs: bool = False, candidate_ids=None, top_logprobs: Optional[int] = None,
                              return_score_attention: bool = False, return_token_attention: bool = False, key_drop_rows=None, key_drop_layers=None,
                              return_score_values: bool = False):
        """Score the same clips under several prompts that share their beginning - the reference's four quality
        perspectives ask four questions BEHIND the same system + frame + motion tokens (8f-3) and
        run four full passes (stage2_eval.py evaluates one jsonl per perspective).  Here the common prefix runs once
        (ViT, projector, LLM prefill into the KV cache); every prompt then only continues its own few question / answer
        tokens over the cached keys (``aigv_llm_extend``).  ``prompts``: list of ``(input_ids[B, N_p], attention_mask,
        labels)``; returns the list of ``forward`` result dicts, one per prompt.  Causal attention makes the prefix rows
        independent of what follows, so each result is that of a separate ``forward`` call up to kernel summation order.
        ``return_logprobs``: every prompt's dict carries ``logprob`` and ``ce_loss`` as ``forward`` defines them - with candidate answers
        as the prompts, their log-likelihoods behind one video prefix (README).  ``candidate_ids``: every prompt's dict carries
        ``cand_logprob`` as ``forward`` defines it (the same candidates for every prompt).  ``top_logprobs``: every prompt's dict carries
        ``top_ids`` / ``top_logprob`` as ``forward`` defines them.  ``return_score_attention``: every prompt's dict carries its own
        ``score_attention`` [B, L, n_heads, F + 4] as ``forward`` defines it (default segments), read by the continuation pass over the cached
        prefix keys and the prompt's own tokens; at most 64 (clip, prompt) pairs.  ``return_token_attention`` (implies it): every prompt's dict
        also carries ``score_attention_tokens`` [B, L, n_heads, N] as ``forward`` defines it, N = the longest prefix + prompt length over the
        prompts; the columns cover the prefix and then the prompt's own tokens, in order.  ``key_drop_rows`` / ``key_drop_layers`` are refused with
        a ValueError: the prefix lives in the KV cache, ``forward`` takes them."""
        readouts.refuse_key_drop_qualifiers("forward_shared_prefix", key_drop_rows, key_drop_layers)
        if self.img_context_token_id is None:
            raise AssertionError("img_context_token_id must be set by the caller (stage2_eval.py:810)")
        if not prompts:
            return []
        pixel_values, visual_tokens, motion_feature = self._take_ahead(pixel_values, visual_tokens, motion_feature)
        n_frames = visual_tokens.shape[0] if visual_tokens is not None else pixel_values.shape[0]
        plans = [self._plan(ids, am, lab, image_flags, n_frames) for (ids, am, lab) in prompts]
        ro = readouts.ReadOuts.parse(self.config.llm_config.vocab_size, "given", return_logprobs=return_logprobs, candidate_ids=candidate_ids, top_logprobs=top_logprobs,
                                     return_score_attention=return_score_attention, return_token_attention=return_token_attention, return_score_values=return_score_values)
        lp_labels = [self._logprob_labels(pl) for pl in plans] if ro.wants_labels else None
        B = prompts[0][0].shape[0]
        pre = self._shared_prefix_lengths(plans, B)
        p0 = plans[0]
        ids_prefix = torch.cat([p0["ids_packed"][p0["cu"][b]:p0["cu"][b] + pre[b]] for b in range(B)])
        slot_prefix = torch.cat([p0["slot"][p0["cu"][b]:p0["cu"][b] + pre[b]] for b in range(B)])
        cu_prefix = list(accumulate(pre, initial=0))
        motion_feature = self._motion_feature(pixel_values, B, motion_feature)
        longest = max(max(pl["lens"]) for pl in plans)
        P = len(plans)
        n_suffix = sum(pl["cu"][-1] for pl in plans) - P * cu_prefix[-1]
        self._native(n_frames=n_frames, n_tokens=max(cu_prefix[-1], n_suffix), n_clips=B * P,
                     out_rows=sum(len(pl["logit_rows"]) for pl in plans), kv_cap=longest + 1,
                     seq_len=max(ids.shape[1] for (ids, _, _) in prompts))
        vit_embeds, motion = self._visual_inputs(pixel_values, visual_tokens, motion_feature, p0)
        self._prefill(ids_prefix, slot_prefix, cu_prefix, vit_embeds, p0["n_vis"], motion, None, [], keep_kv=True, kv_cap=longest + 1)
        lib, ctx = native.load(), self._ctx
        dev = self.device
        # one cache copy per prompt, then ONE continuation pass over B * P sequences (sequence p * B + b = clip b under prompt p):
        # the decoder weights are streamed once for all prompts
        native.check(lib.aigv_kv_fork(ctx, P, native.stream_ptr()), ctx)
        parts, cu_s, lrows, srows, n_l = [], [0], [], [], []
        for pl in plans:
            starts = []
            for b in range(B):
                parts.append(pl["ids_packed"][pl["cu"][b] + pre[b]:pl["cu"][b + 1]])
                starts.append(cu_s[-1])
                cu_s.append(cu_s[-1] + pl["lens"][b] - pre[b])
            def local(r, pl=pl, starts=starts):   # packed row of the full prompt -> packed row of the suffix batch
                b = max(i for i in range(B) if pl["cu"][i] <= r)
                return starts[b] + (r - pl["cu"][b] - pre[b])
            rows = [local(r) for r in pl["logit_rows"]]
            lrows += rows
            n_l.append(len(rows))
            if pl["score_rows"] is not None:
                srows += [local(r) for r in pl["score_rows"]]
        ids_d = torch.cat(parts).to(torch.long).contiguous().pin_memory().to(dev, non_blocking=True)
        score = torch.empty(B * P, dtype=torch.float32, device=dev) if self.stage == 2 else None
        amax = torch.empty(max(len(lrows), 1), dtype=torch.long, device=dev)
        att = tok = val = None
        if ro.score_attention:
            # rows: sequence p * B + b of the continuation batch; segments of its new tokens: the prompt's own table behind the prefix; of the
            # cached keys: the clip's prefix table, tiled over the P prompts (row p * B + b, padded with -1 to the longest prefix)
            if B * P > self.MAX_PROBE_ROWS:
                raise ValueError(f"return_score_attention: at most {self.MAX_PROBE_ROWS} (clip, prompt) pairs per call, got {B * P}")
            prows, seg_parts, S = [], [], 0
            for p, pl in enumerate(plans):
                seg_p, S = self._default_segments(pl)
                for b, r in enumerate(self._probe_rows(pl)):
                    prows.append(cu_s[p * B + b] + (r - pl["cu"][b] - pre[b]))
                    seg_parts.append(seg_p[pl["cu"][b] + pre[b]:pl["cu"][b + 1]])
            seg0, _ = self._default_segments(p0)
            ld = max(pre)
            seg_cached = torch.full((P * B, ld), -1, dtype=torch.int32)
            for b in range(B):
                seg_cached[b::B, :pre[b]] = seg0[p0["cu"][b]:p0["cu"][b] + pre[b]]
            probe = (prows, self._h2d(torch.cat(seg_parts).contiguous()), self._h2d(seg_cached), ld, S)
            # (without the dense rows: the one-argument call, the form wrappers of this method have always been written against)
            if ro.score_values:
                att, tok, val = self._arm_score_attention(probe, longest if ro.token_attention else 0, True)
            else:
                att, tok = self._arm_score_attention(probe, longest) if ro.token_attention else self._arm_score_attention(probe)
        native.check(lib.aigv_llm_extend(ctx, ids_d.data_ptr(), native.i32_array(cu_s), B * P,
                                         native.i32_array(srows) if score is not None else None, native.ptr(score),
                                         native.i32_array(lrows) if lrows else None, len(lrows), amax.data_ptr(), 0,
                                         native.stream_ptr()), ctx)
        reads = self._read_rows(len(srows), len(lrows), ro, torch.cat(lp_labels) if ro.logprobs else None)   # rows [score rows | logit rows]
        outs, off = [], 0
        clips_of = lambda t, p: None if t is None else t[p * B:(p + 1) * B]
        for p, (pl, (ids, _, _)) in enumerate(zip(plans, prompts)):
            outs.append(self._outputs(pl, B, ids.shape[1], clips_of(score, p), amax[off:off + n_l[p]], mos,
                                      {k: v[off:off + n_l[p]] for k, v in reads.items()}, clips_of(att, p), clips_of(tok, p), clips_of(val, p)))
            off += n_l[p]
        return outs

