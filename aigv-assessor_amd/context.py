"""The native context of ``InternVLChatModel``: its capacities, weight and rotary-table upload, the per-context mode setters and the profiler read-out."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from . import native
from .graphs import _PARKED_GRAPHS


# ------------------------------------------------------------------------------------------------------
# host-side weight preparation (not on the hot path: runs once per weight upload)
# ------------------------------------------------------------------------------------------------------
def rope_tables(head_dim: int, theta: float, n_pos: int, max_pos: int = 32768, scaling: Optional[dict] = None,
                seq_len: Optional[int] = None):
    """cos/sin [n_pos, head_dim/2] bf16, computed as the reference does (modeling_internlm2.py:161-243):
    fp32 inv_freq and angles, cos/sin in fp32, then cast to the activation dtype.  The reference table is
    cat(freqs, freqs) so only the first half is stored.

    ``n_pos`` is only the number of table rows (a capacity: packed tokens of a batch, KV capacity).  Dynamic-NTK
    rescaling is decided by ``seq_len``, the length of the longest SINGLE sequence of the call - the reference keys it
    on the per-sequence ``kv_seq_len`` (:218-243, :387-391), so a batch of many short clips is never rescaled however
    many tokens it packs.  ``seq_len=None`` means "no sequence is longer than max_pos" (no rescale)."""
    base = float(theta)
    if scaling is not None and scaling.get("type") == "dynamic" and seq_len is not None and seq_len > max_pos:
        f = float(scaling["factor"])
        base = base * ((f * seq_len / max_pos) - (f - 1)) ** (head_dim / (head_dim - 2))
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2).float() / head_dim))
    t = torch.arange(n_pos).to(inv_freq.dtype)
    if scaling is not None and scaling.get("type") == "linear":
        t = t / float(scaling["factor"])
    freqs = torch.outer(t, inv_freq)
    return freqs.cos().to(torch.bfloat16).contiguous(), freqs.sin().to(torch.bfloat16).contiguous()


def resized_pos_table(pos: torch.Tensor, base_grid: int, grid: int) -> torch.Tensor:
    """Position table for a ``grid x grid`` patch grid (modeling_intern_vit.py:87-93,102-105): class row
    as-is, patch rows bicubic-resized in fp32 (align_corners=False) and cast back.  Precomputed once per
    upload instead of on every forward; at the native grid it is the identity."""
    pos = pos.detach().to("cpu")
    dt = pos.dtype
    patch = pos[:, 1:, :].float().reshape(1, base_grid, base_grid, -1).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(grid, grid), mode="bicubic", align_corners=False)
    patch = patch.reshape(1, -1, grid * grid).permute(0, 2, 1).to(dt)
    return torch.cat([pos[:, :1, :], patch], dim=1).contiguous()


class NativeContext:
    def _apply(self, fn, *a, **k):  # .cuda() / .to(): weights move, the native copy must follow
        out = super()._apply(fn, *a, **k)
        self._invalidate()
        return out

    def _invalidate(self):
        self._dirty = True
        self._drop_graphs()

    @property
    def device(self):
        return self.mlp1._modules["1"].weight.device

    @property
    def dtype(self):
        return torch.bfloat16

    # ---- native context ---------------------------------------------------------------------------------
    def _rope_seq_len(self, seq_len: int) -> int:
        """The sequence length the dynamic-NTK base is computed for, 0 = plain tables.  The reference rescales the rotary
        base when the per-sequence ``kv_seq_len`` (the padded N of the call, plus any cache) exceeds
        ``max_position_embeddings`` (modeling_internlm2.py:218-243); the packed token count of a batch plays no part."""
        l = self.config.llm_config
        sc = l.rope_scaling
        if sc and sc.get("type") == "dynamic" and seq_len > l.max_position_embeddings:
            return int(seq_len)
        return 0

    def _native(self, n_frames: int = 0, n_tokens: int = 0, n_clips: int = 0, out_rows: int = 0, kv_cap: int = 0,
                seq_len: int = 0):
        """Create (or grow) the native context and upload weights if they changed.  ``seq_len`` = the longest single
        sequence of the call about to run (0: leave the rotary tables as they are)."""
        if self.device.type != "cuda":
            raise native.NativeError("the scorer hot path runs on an MI355X only: move the model with .cuda() "
                                     "(there is no CPU fallback)")
        lib = native.load()
        cfg, v, l = self.config, self.config.vision_config, self.config.llm_config
        key = getattr(self, "_cap", None) or dict(frames=0, tokens=0, clips=0, rows=0, kv=0)
        # capacities only grow, in coarse steps (tokens by 512, KV by 256, output rows by 64).  A request above one re-allocates the
        # workspaces of the context (aigv_ctx_resize: a device sync and a few hipMallocs); the weights are uploaded once per load
        up = lambda x, m: (int(x) + m - 1) // m * m
        want = dict(frames=max(key["frames"], n_frames, self._max_frames or 0, 1),
                    tokens=max(key["tokens"], up(max(n_tokens, self._max_tokens, 1), 512)), clips=max(key["clips"], n_clips, self._max_clips, 1),
                    rows=max(key["rows"], up(max(out_rows, 64), 64)), kv=max(key["kv"], up(kv_cap, 256)))
        geom = (v.image_size if cfg.force_image_size is None else cfg.force_image_size, v.hidden_size, l.vocab_size,
                self.select_layer)
        if self._ctx is None or want != key or geom != self._ctx_key:
            self._drop_graphs()                  # captured graphs hold the old workspaces' addresses
            # same model, larger capacities: only the workspaces are re-allocated (aigv_ctx_resize), the weights stay on the device
            grow = self._ctx is not None and geom == self._ctx_key and not self._dirty
            if self._ctx is not None and not grow:
                lib.aigv_ctx_destroy(self._ctx)
                self._ctx = None
            c = native.AigvConfig()
            c.vit_hidden, c.vit_inter, c.vit_heads, c.vit_layers = v.hidden_size, v.intermediate_size, v.num_attention_heads, v.num_hidden_layers
            c.image_size, c.patch_size, c.num_channels = cfg.image_size, v.patch_size, v.num_channels
            c.vit_norm_rms = 1 if v.norm_type == "rms_norm" else 0
            c.vit_qk_norm, c.vit_qkv_bias, c.vit_eps = int(v.qk_normalization), int(v.qkv_bias), v.layer_norm_eps
            c.select_layer, c.shuffle = self.select_layer, int(round(1 / cfg.downsample_ratio))
            c.llm_hidden, c.llm_inter, c.llm_heads, c.llm_kv_heads = l.hidden_size, l.intermediate_size, l.num_attention_heads, l.num_key_value_heads
            c.llm_layers, c.vocab, c.rms_eps = l.num_hidden_layers, l.vocab_size, l.rms_norm_eps
            c.max_positions = max(want["tokens"], want["kv"], 64)
            c.motion_dim = cfg.motion_dim
            dims = list(cfg.score_dims) if self.stage == 2 else [1]
            c.n_score_layers = len(dims)
            for i, d in enumerate(dims):
                c.score_dims[i] = d
            c.max_frames = want["frames"]
            c.vit_chunk = min(want["frames"], 64)
            c.max_tokens, c.max_seqs, c.max_out_rows, c.kv_capacity = want["tokens"], want["clips"], want["rows"], want["kv"]
            if grow:
                rc = lib.aigv_ctx_resize(self._ctx, C.byref(c))
                if rc != 0:                      # e.g. out of memory: the context is unusable now
                    msg = lib.aigv_last_error(self._ctx)
                    lib.aigv_ctx_destroy(self._ctx)
                    self._ctx, self._dirty = None, True
                    raise native.NativeError(f"libaigv_amd error {rc}: {msg.decode() if msg else '?'}")
                self._cap = want
                if c.max_positions != self._n_pos:   # longer rotary tables: reload them (aigv_finalize_weights inside; it keeps the precision mode)
                    self._n_pos = c.max_positions
                    self._upload_rope()
            else:
                h = C.c_void_p()
                native.check(lib.aigv_ctx_create(self.device.index or 0, C.byref(c), C.byref(h)))
                self._ctx, self._cap, self._ctx_key, self._dirty = h, want, geom, True
                self._n_pos = c.max_positions
        if seq_len:
            ntk = self._rope_seq_len(seq_len)
            if ntk != getattr(self, "_rope_ntk", 0):
                self._rope_ntk = ntk
                self._drop_graphs()              # (the rotary tables a captured pass reads are replaced)
                if not self._dirty:
                    self._upload_rope()
        if self._dirty:
            self._upload()
        return lib, self._ctx

    def _rope_for_decode(self, kv_seq_len: int):
        """Dynamic-NTK rope scaling during decode: the reference's rotary module rebuilds its tables, with the base of the CURRENT
        ``kv_seq_len`` (cached keys + the new token, the padded width of the batch), whenever that exceeds what it has cached - i.e.
        at every decode step past ``max_position_embeddings`` - and rotates only the new token's q / k with them; cached keys keep the
        base they were rotated with (modeling_internlm2.py:187-194,227-243).  Here: the tables are rebuilt and swapped before such a step
        (a host computation and two H2D copies per token - this far out, decode is not a throughput path)."""
        ntk = self._rope_seq_len(kv_seq_len)
        if ntk != getattr(self, "_rope_ntk", 0):
            self._rope_ntk = ntk
            self._drop_graphs()
            torch.cuda.current_stream(self.device).synchronize()     # the previous step still reads the tables being replaced
            self._upload_rope()

    def _upload_rope(self):
        """(Re)build the rotary tables: rows = the context's position capacity, base = the dynamic-NTK base of the current call."""
        lib, ctx = native.load(), self._ctx
        l = self.config.llm_config
        ntk = getattr(self, "_rope_ntk", 0)
        cos, sin = rope_tables(l.head_dim, l.rope_theta, self._n_pos, l.max_position_embeddings, l.rope_scaling, seq_len=ntk or None)
        for name, t in (("rope.cos", cos), ("rope.sin", sin)):
            shape = (C.c_int64 * t.dim())(*t.shape)
            native.check(lib.aigv_load_weight(ctx, name.encode(), t.data_ptr(), shape, t.dim(), 0, 0), ctx)
        if not self._dirty:     # tables swapped under finalized weights: re-derive the pointers.  The library keeps the precision mode
            native.check(lib.aigv_finalize_weights(ctx), ctx)     # and the e4m3 copies: no InternLM2 linear was reloaded (aigv_amd.h)

    def _upload(self):
        lib, ctx = native.load(), self._ctx
        cfg, v, l = self.config, self.config.vision_config, self.config.llm_config

        def put(name, t):
            t = t.detach()
            if t.dtype != torch.bfloat16:
                t = t.to(torch.bfloat16)
            t = t.contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            native.check(lib.aigv_load_weight(ctx, name.encode(), t.data_ptr(), shape, t.dim(), 0, int(t.is_cuda)), ctx)

        for name, p in self.named_parameters():
            if name.startswith("mlpscore.ln1"):
                continue  # present in the reference state-dict, unused by its forward (:55,85)
            if name == "vision_model.embeddings.position_embedding":
                put(name, resized_pos_table(p.data, v.image_size // v.patch_size, cfg.image_size // v.patch_size))
            else:
                put(name, p.data)
        if self.stage == 1:  # stage-1 flavour has no score head: a 1-wide dummy keeps the ABI uniform
            put("mlpscore.fc1.weight", torch.zeros(1, l.hidden_size, dtype=torch.bfloat16))
            put("mlpscore.fc1.bias", torch.zeros(1, dtype=torch.bfloat16))
        self._upload_rope()
        native.check(lib.aigv_finalize_weights(ctx), ctx)
        # finalize resets the context to bf16 and drops stale e4m3 weight copies: a re-created context or reloaded weights keep the mode
        native.check(lib.aigv_set_precision(ctx, 1 if getattr(self, "_precision", "bf16") == "fp8" else 0), ctx)
        # per-context switches survive a re-created context
        native.check(lib.aigv_set_gemm_mode(ctx, int(getattr(self, "_gemm_mode", -1))), ctx)
        native.check(lib.aigv_set_row_trimming(ctx, int(getattr(self, "_row_trim", True))), ctx)
        native.check(lib.aigv_set_attention_numerics(ctx, int(getattr(self, "_attn_numerics", 0))), ctx)
        self._dirty = False

    def __del__(self):
        try:
            _PARKED_GRAPHS.extend(v for v in getattr(self, "_graphs", {}).values() if isinstance(v, tuple))      # (see _drop_graphs)
        except Exception:
            pass
        try:
            if getattr(self, "_ctx", None) is not None:
                native.release("aigv_ctx_destroy", self._ctx)      # (parked while a stream capture is underway: native.release)
        except Exception:
            pass

    def _ctx_set(self, entry: str, *args):
        """One per-context switch of the library, on this model's context (created first if there is none yet)."""
        lib, ctx = self._native()
        native.check(getattr(lib, entry)(ctx, *args), ctx)

    def set_precision(self, mode: str = "bf16"):
        """"bf16" (default: the reference's dtype flow) or "fp8": the InternLM2 prefill linears of ``forward`` on the e4m3 MFMA with
        per-channel weight scales and per-token activation scales (BASELINE config 5; aigv_set_precision in include/aigv_amd.h).
        The reference has no fp8 path; scores move by the quantisation noise documented in DESIGN.md."""
        self._drop_graphs()
        if mode not in ("bf16", "fp8"):
            raise ValueError("precision must be 'bf16' or 'fp8'")
        self._precision = mode
        if self._ctx is not None and not self._dirty:
            native.check(native.load().aigv_set_precision(self._ctx, 1 if mode == "fp8" else 0), self._ctx)

    def set_attention_numerics(self, mode: str = "fp32"):
        """Prefill attention: "fp32" (default since round 5) keeps the score matrix in fp32 up to the softmax; "reference" rounds it to bf16
        exactly where the reference's eager path does (modeling_internlm2.py:417, modeling_intern_vit.py:153).  Over the 37 clips the
        imported reference was recorded on the two are equally far from its bf16 scores (2.80 / 3.09 bf16 ulps mean; the reference against
        itself under other host thread counts: 2.56), "fp32" is closer to its fp32 scores (2.01 / 3.59) and ~1.6 % faster
        (profiles/r5_parity_stats.txt)."""
        self._drop_graphs()
        if mode not in ("reference", "fp32"):
            raise ValueError("attention numerics must be 'reference' or 'fp32'")
        self._attn_numerics = 1 if mode == "reference" else 0
        self._ctx_set("aigv_set_attention_numerics", self._attn_numerics)

    def set_gemm_mode(self, mode: int = -1):
        """GEMM tile choice of this model's context (aigv_set_gemm_mode): -1 process default, 0 per-clip / per-frame row plans (the
        default: batch-invariant bits), 1 every row on the 128x128 kernel, 2 the 256x256 kernel wherever it applies (both full K: test
        aliases), 3 the batch-level cost-model dispatch of rounds 1-3 (A/B only)."""
        self._drop_graphs()
        self._gemm_mode = int(mode)
        self._ctx_set("aigv_set_gemm_mode", int(mode))

    TUNE_KNOBS = {"gemm_mode": 0, "gemm256_order": 1, "gemm256_variant": 2, "attn_waves": 3, "skinny_p": 4, "body_tile": 5, "co_kmax": 6,
                  "tail_slices": 7, "attn_lead_key": 8, "decode_fused": 9, "decode_fp8": 10, "skinny_p8": 11, "fuse_tails": 12, "lone_body": 13}

    def tune(self, knob: str, value: int = -1):
        """Experiment knobs of THIS model's context (aigv_ctx_tune; -1 = follow the process default): tests and A/B runs only."""
        self._drop_graphs()
        self._ctx_set("aigv_ctx_tune", self.TUNE_KNOBS[knob], int(value))

    def set_row_trimming(self, on: bool = True):
        """Last-layer row trimming (default on): the last decoder layer finishes only the rows whose hidden state is
        consumed (score row + answer rows; stage2_eval.py:940-941, modeling_internvl_chat.py:469-481).  Off = every row
        through every layer, as the reference computes it; the returned values are the same."""
        self._drop_graphs()
        self._row_trim = bool(on)
        self._ctx_set("aigv_set_row_trimming", int(on))
        self.drop_dead_tail = bool(on)      # the host-side half: tokens behind a clip's last consumed row are not run

    # ---- measurement ---------------------------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        self._drop_graphs()
        self._prof_on = bool(on)        # (per-launch HIP events: such passes are not replayed from a graph)
        self._ctx_set("aigv_prof_enable", int(on))

    def prof_read(self) -> Dict[str, Dict[str, float]]:
        lib, ctx = self._native()
        out = {}
        for cls, name in enumerate(("gemm_llm", "attn_vit", "attn_llm", "skinny", "gemm_fp8", "gemm_vit")):
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            native.check(lib.aigv_prof_read(ctx, cls, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), ctx)
            out[name] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)
        out["gemm"] = {k: out["gemm_llm"][k] + out["gemm_vit"][k] for k in out["gemm_llm"]}     # every bf16 tile-kernel GEMM launch
        return out
