"""HIP-graph replay of whole scoring passes for ``InternVLChatModel``: the graph cache, capture, and everything this stack taught about parked graphs."""
from __future__ import annotations

import os

import torch

from . import native, readouts

_PARKED_GRAPHS: list = []      # captured passes that were dropped: kept alive until the interpreter exits (InternVLChatModel._drop_graphs)


class GraphReplay:
    # ---- HIP-graph replay of whole scoring passes (opt-in: enable_graph_replay) ---------------------------------------------------------
    _graph_replay_enabled = False
    _capture_keep = None
    GRAPH_CACHE_SIZE = 8
    PARKED_GRAPHS_LIMIT = 384     # dropped graphs kept alive before capturing stops for good (~95 MB each for a 4-clip pass at 8B sizes: ~36 GB)

    def enable_graph_replay(self, on: bool = True):
        """``forward`` calls whose HOST-side arguments (token ids, masks, labels, frame flags, options) and tensor shapes repeat - the
        reference's eval loop scores every clip behind the same prompt (stage2_eval.py:908-941) - are captured into a HIP graph on their
        second occurrence and replayed from the third on: ONE host call launches the ~1000 kernels of the pass (InternViT, projector,
        SlowFast side stream, InternLM2, heads), the frames are copied into the graph's input buffer first.  Same kernels, same bits
        (tests/test_gpu_api.py); what changes is the host time per pass (5-6 ms -> ~0.1 ms) - decisive where the host is slower than the
        GPU's launch stream (a CPU-throttled container: 314 -> 115 ms per step measured, profiles/r5_graph_replay.txt).  Off by default;
        any weight / mode / knob change drops the captured graphs (after a device synchronisation).  At most GRAPH_CACHE_SIZE call shapes are
        tracked; a captured graph is never evicted while the model runs - once every entry holds a graph, further call shapes stay eager (round 6:
        a 1200-clip soak with ragged groups showed that destroying a graph to make room, possibly with its replay still in flight, poisons a later
        capture: tests/manual/soak_loop.py)."""
        self._graph_replay_enabled = bool(on)
        self._drop_graphs()
        self._graphs = {}

    def _drop_graphs(self):
        """Forget every captured pass (a weight / mode / knob / capacity change made them stale).  The graph OBJECTS are not destroyed: they are parked in a
        process-wide list until the interpreter exits.  On this stack (ROCm 7.2, torch 2.10) destroying a graph object - like any device-memory release - INSIDE a
        stream capture kills that capture (the process aborts or can launch nothing any more: scripts/capture_hipfree_probe.py), an object that is merely dropped
        may be destroyed at any later moment by Python's cyclic collector, also in the middle of another capture, and destroying them at a quiet moment (device
        idle, no capture underway, followed by empty_cache) was tried and is not safe either: with several models alive, a later replay of ANOTHER model's live
        graph then crashed inside hipGraphLaunch (tests/manual/fuzz_api.py seed 3; profiles/r6_soak.txt).  Parking costs the graph's private pool and static copies
        (~95 MB per captured 4-clip pass at 8B sizes) plus ~1.5 MiB of runtime memory, at most GRAPH_CACHE_SIZE graphs per drop; drops happen on weight / mode / capacity changes and when the
        motion branch retires a native handle, i.e. rarely."""
        if getattr(self, "_graphs", None):
            held = [v for v in self._graphs.values() if isinstance(v, tuple)]
            if held and self.device.type == "cuda":
                torch.cuda.synchronize(self.device)      # (no replay in flight while the entries change hands)
            _PARKED_GRAPHS.extend(held)
            self._graphs = {}

    def _branch_uid(self):
        sf = self.slowfast_model
        return None if sf is None else getattr(sf, "uid", None) or ("id", id(sf))

    def _prepare_motion_branch(self, frames, n_clips: int):
        """In front of every pass that may be captured or replayed with the native SlowFast branch inside: make the branch's native handle for
        this geometry exist NOW (creating one allocates and uploads weights - illegal inside a capture), and drop this model's graphs when any
        handle of the branch has been destroyed since they were captured (a graph holds the addresses of a handle's buffers; SlowFastR50.epoch)."""
        sf = self.slowfast_model
        if sf is None or not hasattr(sf, "prepare"):
            return
        if frames is not None and n_clips > 0 and frames.dim() == 4 and frames.shape[0] % n_clips == 0:
            sf.prepare(self.device, int(n_clips), int(frames.shape[0]) // int(n_clips), int(frames.shape[2]), int(frames.shape[3]))
        seen = (self._branch_uid(), sf.epoch)
        if getattr(self, "_sf_epoch", None) != seen:
            if getattr(self, "_sf_epoch", None) is not None and any(isinstance(v, tuple) for v in self.__dict__.get("_graphs", {}).values()):
                self._drop_graphs()
            self._sf_epoch = seen

    def _capture(self, fn):
        """``fn()`` captured into a new HIP graph (device idle first) -> (graph, what ``fn`` returned, the pinned staging buffers ``_h2d`` made
        inside it: the graph's replays copy from those very addresses, so they live as long as the graph)."""
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        self._capture_keep = []
        try:
            with native.capturing(), torch.cuda.graph(graph, capture_error_mode="relaxed"):
                outputs = fn()
            return graph, outputs, self._capture_keep
        finally:
            self._capture_keep = None

    def _graph_call(self, host_key, dev_inputs, fn, clone_outputs=True):
        """Graph-cached call of ``fn(*dev_inputs)`` (launches on torch's current stream only; device tensors in, a tensor / tuple / dict of
        device tensors out): first occurrence of (host_key, input shapes) -> None (the caller runs eager); second -> capture on static copies
        of the inputs; afterwards copy the inputs in, replay, hand the outputs back (cloned unless the caller consumes them at once)."""
        key = (host_key, tuple(None if t is None else (tuple(t.shape), t.dtype) for t in dev_inputs))
        graphs = self.__dict__.setdefault("_graphs", {})
        ent = graphs.get(key)
        if os.environ.get("AIGV_GRAPH_DEBUG"):
            import sys as _s
            print(f"[graph] {host_key[0]} key#{hash(key) & 0xffff:04x} state={'new' if ent is None else ent if isinstance(ent, str) else 'captured'} cache={len(graphs)} "
                  f"stream={torch.cuda.current_stream(self.device).cuda_stream:#x}", file=_s.stderr, flush=True)
        if ent is None:                      # first occurrence: eager (sizes the context, warms every kernel); remember the key
            if len(graphs) >= self.GRAPH_CACHE_SIZE:
                # make room by forgetting a key that holds no graph; a CAPTURED graph is never destroyed while the model runs (only by _drop_graphs:
                # a weight / mode / capacity change) - when all entries hold graphs, further call shapes simply stay eager
                victim = next((k for k, v in graphs.items() if isinstance(v, str)), None)
                if victim is None:
                    return None
                graphs.pop(victim)
            graphs[key] = "seen"
            return None
        if ent == "eager":
            return None
        if ent == "seen" and len(_PARKED_GRAPHS) >= self.PARKED_GRAPHS_LIMIT:
            # dropped graphs cannot be destroyed safely on this stack (_drop_graphs): they are parked, with their memory.  A process that has dropped this many
            # (hundreds of mode / weight / capacity changes under graph replay) stops capturing instead of running out of device memory: same kernels, same bits, eager
            if not getattr(type(self), "_park_limit_warned", False):
                type(self)._park_limit_warned = True
                import warnings
                warnings.warn(f"graph replay: {len(_PARKED_GRAPHS)} dropped graphs are parked (they cannot be destroyed safely on this ROCm build); no further pass is "
                              "captured in this process - the eager path runs the same kernels")
            graphs[key] = "eager"
            return None
        if ent == "seen":                    # second occurrence: capture, on static copies of the device inputs
            statics = [None if t is None else t.clone() for t in dev_inputs]
            try:
                graph, outputs, keep = self._capture(lambda: fn(*statics))
            except Exception as e:           # a pass that does not capture (an allocation or a synchronisation inside it) stays eager for good - and
                import warnings              # says so; the eager run that follows raises whatever was a real error rather than a capture-illegal call
                import traceback
                where = "".join(traceback.format_tb(e.__traceback__)[-3:])
                warnings.warn(f"graph replay: capture of {host_key[0]!r} failed ({type(e).__name__}: {str(e).splitlines()[0]}); this call shape stays eager\n{where}")
                graphs[key] = "eager"
                native.load().aigv_clear_hip_error()
                try:                             # can this process still launch?  (scripts/capture_error_probe.py: on ROCm 7.2 a capture that an illegal call INVALIDATED
                    torch.zeros(1, device=self.device).add_(1)      # is never ended - hipStreamEndCapture on it crashes - and every later launch on any stream
                    torch.cuda.synchronize(self.device)             # fails with hipErrorStreamCaptureInvalidated: there is nothing to fall back to)
                except Exception as dead:
                    raise native.NativeError(
                        f"HIP-graph capture of {host_key[0]!r} was invalidated ({type(e).__name__}: {str(e).splitlines()[0]}) and this ROCm build cannot recover from that: every "
                        "further kernel launch of the process fails.  Restart without enable_graph_replay() - the eager path runs the same kernels - and report the call "
                        "sequence that led here") from dead
                return None
            ent = graphs[key] = (graph, outputs, statics, keep)
        graph, outputs, statics, _keep = ent
        for st, t in zip(statics, dev_inputs):
            if st is not None:
                st.copy_(t)
        graph.replay()
        if not clone_outputs:
            return outputs
        cl = lambda v: v.clone() if torch.is_tensor(v) else v      # (the graph's own output tensors are overwritten by the next replay)
        if isinstance(outputs, dict):
            return {k: cl(v) for k, v in outputs.items()}
        if isinstance(outputs, (tuple, list)):
            return tuple(cl(v) for v in outputs)
        return cl(outputs)

    def _forward_through_graph(self, mos, pixel_values, input_ids, attention_mask, image_flags, labels, motion_feature, visual_tokens, full_logits, ro):
        """The replay path of ``forward`` (``ro``: the call's ``readouts.ReadOuts``); returns None when the call does not qualify (the eager path then runs)."""
        src = visual_tokens if visual_tokens is not None else pixel_values
        if self._rope_seq_len(int(input_ids.shape[1])) != getattr(self, "_rope_ntk", 0):
            return None      # this pass re-derives the rotary tables (dynamic NTK: another sequence length than the last pass) - synchronous uploads, never inside a capture
        if (mos is not None or src is None or not src.is_cuda or self._dirty or self._ctx is None or getattr(self, "_prof_on", False)
                or (motion_feature is not None and not motion_feature.is_cuda) or (visual_tokens is not None and motion_feature is None)):
            return None
        host = lambda t: None if t is None else t.detach().to("cpu").contiguous()
        parts = [host(input_ids), host(attention_mask), host(labels), host(image_flags)]
        host_key = ("forward", visual_tokens is not None, bool(full_logits), int(self.img_context_token_id), self._branch_uid(),
                    bool(getattr(self, "overlap_motion_branch", True)), bool(getattr(self, "drop_dead_tail", True)),
                    tuple(None if t is None else (tuple(t.shape), t.dtype, t.numpy().tobytes()) for t in parts))
        n_seg = ro.n_segments(input_ids.shape)       # (read back from a user table HERE, outside the capture)
        host_key += ro.key_tail(input_ids.shape, n_seg)
        cand = None if ro.cand is None else self._h2d(ro.cand)
        seg = None if ro.segments is None else self._h2d(ro.segments.contiguous())
        self._join_side_stream()             # (a motion feature started by motion_feature_async: joined BEFORE the graph copies it in)
        self._prepare_motion_branch(pixel_values if (motion_feature is None and visual_tokens is None) else None, int(input_ids.shape[0]))

        def fn(src_static, mf_static, cand_static, seg_static=None):
            self._probe_n_segments = n_seg or None      # (S is in the key: the pass inside the capture does not read it back from the device)
            try:        # forward itself, with the static candidate and segment tensors substituted into the record
                return self.forward(mos=None, pixel_values=None if visual_tokens is not None else src_static, input_ids=input_ids, attention_mask=attention_mask,
                                    image_flags=image_flags, labels=labels, motion_feature=mf_static, full_logits=full_logits,
                                    visual_tokens=src_static if visual_tokens is not None else None,
                                    **readouts.forward_kwargs(ro.with_(cand=cand_static, segments=seg_static)))      # (with_, not dataclasses.replace: it keeps ro.attention_map, which is no field)
            finally:
                self._probe_n_segments = None
        return self._graph_call(host_key, [src, motion_feature, cand] + ([seg] if seg is not None else []), fn)   # (a user table only: the other keys stay what they were)

    def capture_forward(self, **forward_kwargs):
        """One scoring pass captured into a HIP graph (torch.cuda.CUDAGraph: every launch ``forward`` makes through the C ABI on torch's
        current stream, the SlowFast branch on its side stream, the small index uploads) -> ``(replay, outputs)``: ``replay()`` re-runs the
        ~1000 launches of the pass with ONE host call and refreshes ``outputs`` (the dict ``forward`` returned, static tensors) from the
        CURRENT contents of the input tensors' device memory; host-side arguments (token ids, labels, masks) are frozen at capture time.
        For callers whose host cannot keep up with the launch stream (a CPU-throttled container): same kernels, same bits.  The context
        must be warm (one eager ``forward`` of the same shapes first); profiling brackets must be off.  The replay stays valid until the model's
        weights, modes or capacities change or the motion branch retires the native handle of this geometry (SlowFastR50 keeps MAX_HANDLES
        geometries alive): capture again after any of those (``enable_graph_replay`` tracks all of that by itself)."""
        pv = forward_kwargs.get("pixel_values")
        if torch.is_tensor(pv) and forward_kwargs.get("motion_feature") is None and forward_kwargs.get("input_ids") is not None:
            self._prepare_motion_branch(pv, int(forward_kwargs["input_ids"].shape[0]))
        graph, outputs, keep = self._capture(lambda: self.forward(**forward_kwargs))

        def replay(_graph=graph, _keep=keep):
            _graph.replay()
            return outputs
        return replay, outputs

