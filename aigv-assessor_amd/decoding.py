"""Generation with ``InternVLChatModel``: the decode loop, beam search, ``generate*`` and the chat wrappers."""
from __future__ import annotations

import ctypes as C
from itertools import accumulate
from typing import List, Optional

import torch

from . import generation, native, prompts, readouts
from .conversation import get_conv_template


class Generation:
    # ---- generation (API surface; greedy) -------------------------------------------------------------------
    def _decode_step(self, tok: torch.Tensor, logprobs: bool = False, cand: Optional[torch.Tensor] = None, topk: int = 0):
        """One native decode step for the current tokens ``tok`` [b] -> (next tokens, lp, clp, top): with ``logprobs`` or candidates ``cand`` (device
        int64 [C]) the lm-head pass that picks the token also gives its fp32 log-probability [b] and the candidates' [b, C]; with ``topk`` also
        top = (ids int64 [b, k], log-probabilities fp32 [b, k]) of the k largest logits; None for what the step did not compute."""
        lib, ctx, b = native.load(), self._ctx, tok.numel()
        new = torch.empty_like(tok)
        lp = torch.empty(b, dtype=torch.float32, device=self.device) if logprobs or cand is not None or topk else None
        clp = None if cand is None else torch.empty((b, cand.numel()), dtype=torch.float32, device=self.device)
        top = None
        if topk:                    # one lm-head pass: token, its log-probability, the k most likely tokens and (optionally) the candidates
            top = (torch.empty((b, topk), dtype=torch.long, device=self.device), torch.empty((b, topk), dtype=torch.float32, device=self.device))
            native.check(lib.aigv_decode_step_topk_logprob(ctx, tok.data_ptr(), new.data_ptr(), lp.data_ptr(), int(topk), top[0].data_ptr(),
                                                           top[1].data_ptr(), native.ptr(cand), 0 if cand is None else cand.numel(),
                                                           native.ptr(clp), native.stream_ptr()), ctx)
        elif cand is not None:    # one lm-head pass: token, its log-probability and the candidates'
            native.check(lib.aigv_decode_step_cand_logprob(ctx, tok.data_ptr(), new.data_ptr(), lp.data_ptr(), cand.data_ptr(), cand.numel(),
                                                           clp.data_ptr(), native.stream_ptr()), ctx)
        elif logprobs:
            native.check(lib.aigv_decode_step_logprob(ctx, tok.data_ptr(), new.data_ptr(), lp.data_ptr(), native.stream_ptr()), ctx)
        else:
            native.check(lib.aigv_decode_step(ctx, tok.data_ptr(), new.data_ptr(), native.stream_ptr()), ctx)
        return new, lp, clp, top

    EOS_CHECK_EVERY = 8     # tokens between two host reads of the device-side "finished" flags

    def _greedy(self, ids_packed, slot, cu, vis, n_vis, max_new_tokens: int, eos_ids: List[int], pad_id: int, motion=None, sampler=None,
                processors=None, beams=None, flags=None, cand=None, topk: int = 0, drop_words=None):
        """The token loop of generate(): HF's greedy search / multinomial sampling loop (the reference calls ``language_model.generate``,
        modeling_internvl_chat.py:798-809).  The end-of-sequence bookkeeping runs on the device (aigv_decode_eos): a finished sequence
        emits ``pad_id``, the loop stops once every sequence has emitted an end token - checked by the host only every EOS_CHECK_EVERY
        tokens, so no per-token host synchronisation; the columns past HF's stopping point are cut off afterwards.

        ``flags`` (generation.output_flags): with return_dict_in_generate / return_logprobs the result is a generation.GenerateOutput.  Greedy
        decoding without processors takes its log-probabilities from the decode step's fused lm-head (aigv_decode_step_logprob; the first
        token's from aigv_out_row_logprob) and never builds a [B, V] tensor; wherever the step's logits are materialised (processors,
        sampling, output_scores / output_logits) they come from the scores the token was chosen from.

        ``cand`` (int64 [C], ``candidate_ids``): ``cand_logprobs`` [B, T, C], the full-vocabulary log-probabilities of the candidates at every
        step - from the fused decode step (aigv_decode_step_cand_logprob; the first token's from aigv_out_row_cand_logprob) on the greedy
        path without processors, else the log-softmax of the step's RAW logits (before processors and warpers) at the candidates.

        ``topk`` (``top_logprobs=k``): ``top_ids`` / ``top_logprobs`` [B, T, k], the k most likely tokens of every step under the RAW logits -
        from the fused decode step (aigv_decode_step_topk_logprob; the first token's from aigv_out_row_topk_logprob) on the greedy path
        without processors, else generation.top_logprobs of the step's raw logits.

        ``drop_words`` (``key_drop``: host int64 [B, W], ``_gen_drop_words``): the prompt pass runs masked and keeps the mask with its KV cache
        (aigv_key_drop_arm in front of aigv_llm_prefill(keep_kv)); every decode step, the beams' fork and reorder included, then runs under the
        cache's mask.  Nothing here is captured into a graph: a masked generation runs eagerly like every other."""
        flags = flags or {k: False for k in generation.FLAGS}
        dict_out = generation.wants_output(flags) or cand is not None or bool(topk)
        b = len(cu) - 1
        longest = max(cu[i + 1] - cu[i] for i in range(b))
        last_rows = [cu[i + 1] - 1 for i in range(b)]
        nb = beams["num_beams"] if beams else 1
        self._native(seq_len=longest, n_clips=b * nb, out_rows=b * nb)       # (beam search: room for every beam before the prompt pass)
        _, nxt = self._prefill(ids_packed, slot, cu, vis, n_vis, motion, None, last_rows, keep_kv=True,
                               kv_cap=longest + max_new_tokens + 1, drop_words=drop_words)
        lib, ctx = native.load(), self._ctx
        if beams:
            seq, seq_scores = self._beam_decode(b, [cu[i + 1] - cu[i] for i in range(b)], max_new_tokens, eos_ids, pad_id, processors or [], **beams)
            return generation.build(seq, flags, sequences_scores=seq_scores) if dict_out else seq
        ntk_decode = self._rope_seq_len(longest + max_new_tokens) != 0
        eos_a = (C.c_int64 * max(len(eos_ids), 1))(*[int(e) for e in eos_ids]) if eos_ids else None
        state = torch.zeros(b + 1, dtype=torch.int32, device=self.device)     # finished flags + live-column count (aigv_amd.h)
        # aigv_decode_eos takes at most 8 end ids (kernel-argument array): longer lists keep HF's bookkeeping in torch ops on the device -
        # the same rule (next = next * unfinished + pad * (1 - unfinished); unfinished &= next not in eos), still without a per-token sync
        host_eos = len(eos_ids) > 8
        eos_t = torch.tensor([int(e) for e in eos_ids], dtype=torch.long, device=self.device) if host_eos else None
        outs: List[torch.Tensor] = []
        want_scores = dict_out and flags["output_scores"]
        want_logits = dict_out and flags["output_logits"]
        logprobs = flags["return_logprobs"]
        materialise = sampler is not None or bool(processors) or want_scores or want_logits
        step_scores: List[torch.Tensor] = []
        step_logits: List[torch.Tensor] = []
        step_lp: List[torch.Tensor] = []
        cur_lp: Optional[torch.Tensor] = None      # log-probability of the current raw token (before the end-of-sequence rule)
        step_clp: List[torch.Tensor] = []
        cur_clp: Optional[torch.Tensor] = None     # [b, C] candidate log-probabilities of the current step
        cand = None if cand is None else self._h2d(cand)
        step_top: List[tuple] = []
        cur_top = None                             # ([b, k] ids, [b, k] log-probabilities) of the current step

        def eos_step(tok):
            live = state[:b] == 0
            tok = torch.where(live, tok, torch.full_like(tok, int(pad_id)))
            state[b] += live.any().to(torch.int32)
            state[:b] |= (live & torch.isin(tok, eos_t)).to(torch.int32)
            return tok

        def pick(greedy_tok):
            """The step's raw token: the fused argmax, or - with logits processors / sampling - a choice over the rows' lm-head logits."""
            nonlocal cur_lp, cur_clp, cur_top
            if not materialise:
                return greedy_tok
            raw = self._row_logits(b)
            logits = raw
            if processors:
                hist = torch.stack(outs, dim=1) if outs else torch.zeros((b, 0), dtype=torch.long, device=self.device)
                for proc in processors:
                    logits = proc(hist, logits)
            if sampler is not None:     # = _sample, with the warped scores kept (HF's `scores` of a sampling run)
                logits = self._warp(logits, sampler["temperature"], sampler["top_k"], sampler["top_p"])
                tok = torch.multinomial(logits.softmax(-1), 1, generator=sampler["generator"]).squeeze(1)
            else:
                tok = greedy_tok if not processors else logits.argmax(-1)
            if want_logits:
                step_logits.append(raw)
            if want_scores:
                step_scores.append(logits)
            if logprobs:
                cur_lp = generation.token_logprobs(logits, tok)
            if cand is not None:
                cur_clp = generation.candidate_logprobs(raw, cand)
            if topk:
                cur_top = generation.top_logprobs(raw, topk)
            return tok

        tok = pick(nxt).contiguous()
        if not materialise:     # the first token: the prompt pass's rows, once per call
            first = self._read_rows(0, b, readouts.ReadOuts(logprobs, cand, topk or None), tok)
            cur_lp, cur_clp = first.get("logprob"), first.get("cand_logprob")
            cur_top = (first["top_ids"], first["top_logprob"]) if topk else None
        for step in range(max_new_tokens):
            if logprobs or cand is not None or topk:
                live = None if not eos_ids else (state[:b] == 0)
            if host_eos:
                tok = eos_step(tok).contiguous()
            elif eos_ids:     # tok: raw -> emitted (pad for finished sequences); flags / live-column count advance on the device
                native.check(lib.aigv_decode_eos(ctx, tok.data_ptr(), state.data_ptr(), eos_a, len(eos_ids), int(pad_id), native.stream_ptr()), ctx)
            outs.append(tok)
            if logprobs:
                step_lp.append(generation.mask_after_end(cur_lp, live))
            if cand is not None:
                step_clp.append(generation.mask_after_end(cur_clp, live))
            if topk:
                step_top.append((generation.mask_ids_after_end(cur_top[0], live), generation.mask_after_end(cur_top[1], live)))
            if step + 1 == max_new_tokens:
                break
            if eos_ids and (step + 1) % self.EOS_CHECK_EVERY == 0 and bool(state[:b].all()):
                break
            if ntk_decode:
                self._rope_for_decode(longest + step + 1)
            fused = not materialise     # else pick() reads the step's log-probabilities off the materialised logits
            new, cur_lp, cur_clp, top = self._decode_step(tok, logprobs and fused, cand if fused else None, topk if fused else 0)
            if fused:
                cur_top = top
            tok = pick(new).contiguous()
        out = torch.stack(outs, dim=1)
        if eos_ids:
            out = out[:, : max(1, int(state[b].item()))]     # HF stops after the column in which the last live sequence ended
        if dict_out:
            return generation.build(out, flags, scores=step_scores, logits=step_logits, logprobs=step_lp,
                                    cand_logprobs=step_clp if cand is not None else None,
                                    top_ids=[t[0] for t in step_top] if topk else None, top_logprobs=[t[1] for t in step_top] if topk else None)
        return out

    def _beam_decode(self, b: int, prompt_lens: List[int], max_new_tokens: int, eos_ids: List[int], pad_id, processors, num_beams: int,
                     length_penalty: float = 1.0, early_stopping=False):
        """HF beam search (beam.beam_search) behind a prompt pass that kept its KV: the prompts' caches are replicated once per beam
        (aigv_kv_fork: sequence k * b + i is beam k of prompt i), every step decodes all b * num_beams sequences in one aigv_decode_step
        (the decoder weights stream once for all beams) and the chosen parents are gathered in the cache (aigv_kv_reorder).
        Returns (tokens, sequences_scores)."""
        from . import beam
        lib, ctx = native.load(), self._ctx
        V = self.config.llm_config.vocab_size
        n = b * num_beams
        first = self._row_logits(b)
        native.check(lib.aigv_kv_fork(ctx, num_beams, native.stream_ptr()), ctx)
        fed = [0]                                  # tokens every beam has been fed so far = cached positions behind its prompt
        slot_of = lambda i, k: k * b + i

        def reorder(parent: torch.Tensor):
            if fed[0] == 0:
                return                             # the copies are still identical
            src = beam.parents_to_slots(parent.cpu(), slot_of)
            if src == list(range(n)):
                return
            lens = [prompt_lens[s % b] + fed[0] for s in range(n)]
            native.check(lib.aigv_kv_reorder(ctx, native.i32_array(src), native.i32_array(lens), n, native.stream_ptr()), ctx)

        ntk_decode = self._rope_seq_len(max(prompt_lens) + max_new_tokens) != 0

        def step(tok: torch.Tensor) -> torch.Tensor:
            t = tok.t().contiguous().view(-1)      # [b, nb] -> cache order
            new = torch.empty_like(t)
            if ntk_decode:
                self._rope_for_decode(max(prompt_lens) + fed[0] + 1)
            native.check(lib.aigv_decode_step(ctx, t.data_ptr(), new.data_ptr(), native.stream_ptr()), ctx)
            fed[0] += 1
            return self._row_logits(n).view(num_beams, b, V).transpose(0, 1)

        return beam.beam_search(first, step, reorder, num_beams, max_new_tokens, eos_ids=eos_ids, pad_id=pad_id, length_penalty=length_penalty,
                                early_stopping=early_stopping, processors=processors, return_scores=True)

    def _row_logits(self, n_rows: int) -> torch.Tensor:
        """fp32 [n_rows, vocab]: lm-head logits of the rows the last native pass consumed (aigv_out_row_logits) - the reference's
        ``logits = output(h).float()`` (modeling_internlm2.py:1095-1096)."""
        lib, ctx = native.load(), self._ctx
        V = self.config.llm_config.vocab_size
        ldo = (V + 3) // 4 * 4
        buf = torch.empty((n_rows, ldo), dtype=torch.bfloat16, device=self.device)
        native.check(lib.aigv_out_row_logits(ctx, 0, n_rows, buf.data_ptr(), ldo, native.stream_ptr()), ctx)
        return buf[:, :V].float()

    def last_hidden_rows(self, n_rows: int, first_row: int = 0) -> torch.Tensor:
        """bf16 [n_rows, H]: final hidden states (after the last RMSNorm) of the rows the last native pass consumed, in the order
        [score rows | logit rows] (aigv_out_row_hidden).  After ``forward`` rows 0..B-1 are the reference's
        ``hidden_states[-1][:, -4, :]`` - the score head's input (modeling_internvl_chat.py:469-481)."""
        lib, ctx = native.load(), self._ctx
        if ctx is None:
            raise native.NativeError("no native pass has run yet")
        H = self.config.llm_config.hidden_size
        buf = torch.empty((n_rows, H), dtype=torch.bfloat16, device=self.device)
        native.check(lib.aigv_out_row_hidden(ctx, first_row, n_rows, buf.data_ptr(), H, native.stream_ptr()), ctx)
        return buf

    @staticmethod
    def _gen_drop_words(key_drop, ids_shape, cu, row_of):
        """``generate*(key_drop=...)``: None, or the mask [B, N] (laid out like the call's ``input_ids`` / embeddings) checked on the host - before anything
        is launched - and turned into ``prompts.key_drop_words`` (host int64 [B, W]).  ``cu`` / ``row_of``: the packed prompt (``_pack``).  Padded
        positions are ignored.  Refused: a wrong shape or dtype (``readouts.key_drop_mask``), a clip's first token (it guarantees every row a
        visible key) and a clip's last prompt token (its row predicts the first new token: the consumed row of ``forward``'s rule)."""
        kd = readouts.key_drop_mask(key_drop, ids_shape)
        if kd is None:
            return None
        row_of = row_of.detach().to("cpu")
        dropped = torch.zeros(cu[-1], dtype=torch.bool)
        dropped[row_of[kd & (row_of >= 0)]] = True
        for b in range(len(cu) - 1):
            if bool(dropped[cu[b]]):
                raise ValueError(f"key_drop: clip {b}: the first token cannot be dropped (it guarantees every row a visible key)")
            if bool(dropped[cu[b + 1] - 1]):
                raise ValueError(f"key_drop: clip {b}: the last prompt token is a consumed row (it predicts the first new token) and cannot be dropped")
        return prompts.key_drop_words(kd, cu, row_of)

    def _gen_setup(self, generation_config, generate_kwargs):
        """What the three generate entry points read from their generation config / kwargs (``candidate_ids`` and ``top_logprobs`` are taken out of
        the kwargs): (max_new_tokens, eos ids, pad id, ``_greedy``'s keyword arguments)."""
        # (the knock-out qualifiers of forward(key_drop=...): refused here, before they could pass for sampling settings)
        readouts.refuse_key_drop_qualifiers("generate*", generate_kwargs.pop("key_drop_rows", None), generate_kwargs.pop("key_drop_layers", None))
        ro = readouts.ReadOuts.parse(self.config.llm_config.vocab_size, candidate_ids=generate_kwargs.pop("candidate_ids", None),
                                     top_logprobs=generate_kwargs.pop("top_logprobs", None))
        max_new, eos, pad, sampler, procs, beams = self._gen_args(generation_config, generate_kwargs)
        flags = self._gen_flags(generation_config, generate_kwargs, beams, ro.cand, ro.topk or 0)
        pad = self.config.llm_config.pad_token_id if pad is None else pad
        return max_new, eos, pad, dict(sampler=sampler, processors=procs, beams=beams, flags=flags, cand=ro.cand, topk=ro.topk or 0)

    @torch.no_grad()
    def generate(self, pixel_values: Optional[torch.Tensor] = None, input_ids: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, visual_features: Optional[torch.Tensor] = None,
                 generation_config=None, output_hidden_states=None, return_dict=None, key_drop=None, **generate_kwargs) -> torch.Tensor:
        """modeling_internvl_chat.py:769-811: every <IMG_CONTEXT> slot takes a visual token (no motion
        token), then greedy decode with a KV cache.  Returns the NEW tokens [B, <=max_new_tokens] - or, with HF's
        ``return_dict_in_generate`` (``output_scores`` / ``output_logits``) or ``return_logprobs``, a generation.GenerateOutput
        (``sequences``, ``scores``, ``logits``, ``logprobs``; beam search: ``sequences_scores``).

        ``candidate_ids`` (LongTensor [C] or list, 1 <= C <= 64): the output object also carries ``cand_logprobs`` fp32 [B, T, C], the
        full-vocabulary log-probability of every candidate token at every step under the RAW lm-head logits (before logits processors and
        sampling warpers), NaN after a sequence's end token like ``logprobs``; ``softmax(cand_logprobs[:, t], -1)`` is the closed-set
        distribution at step t.  Greedy decoding without processors reads them in the decode step's own lm-head pass
        (aigv_decode_step_cand_logprob); beam search refuses them.  fp8 mode: the lm-head stays bf16, the same kernels serve.

        ``top_logprobs=k`` (int, 1 <= k <= 16): the output object also carries ``top_ids`` long [B, T, k] and ``top_logprobs`` fp32 [B, T, k] -
        what the model preferred at every step: the k largest RAW lm-head logits (equal logits by ascending id, so entry 0 is the greedy
        token) and their full-vocabulary log-probabilities; -1 / NaN after a sequence's end token.  Greedy decoding without processors
        selects them in the decode step's own lm-head pass (aigv_decode_step_topk_logprob: ``top_logprobs[:, :, 0]`` is ``logprobs``, bit
        for bit); otherwise they are ``generation.top_logprobs`` of the step's raw logits.  Beam search refuses them.

        ``key_drop`` (bool or integer tensor [B, N] laid out like ``input_ids``, on any device): WHAT IF these prompt tokens were not there - what
        the model SAYS without them.  True = the token is hidden, as a key, from every later row of its clip: the prompt pass runs masked as
        ``forward(key_drop=...)`` does, the mask stays with the KV cache, and every generated token attends under it (the generated tokens see
        each other).  Positions stay as they are.  Composes with ``candidate_ids``, ``top_logprobs``, ``return_logprobs``, sampling, processors
        and beam search.  ValueError before anything is launched: a wrong shape or dtype, a clip's first token, a clip's last prompt token (its
        row predicts the first new token)."""
        assert self.img_context_token_id is not None
        max_new, eos, pad, how = self._gen_setup(generation_config, generate_kwargs)
        if key_drop is not None:        # checked in full on the host first
            _, cu_h, row_of = self._pack(input_ids.detach().to("cpu"), attention_mask.detach().to("cpu") if attention_mask is not None else None)
            how["drop_words"] = self._gen_drop_words(key_drop, input_ids.shape, cu_h, row_of)
        dev = self.device
        input_ids = input_ids.to(dev)
        ids_packed, cu, _ = self._pack(input_ids, attention_mask.to(dev) if attention_mask is not None else None)
        slot = torch.full_like(ids_packed, -1, dtype=torch.int32)
        vis, n_vis = None, 0
        if pixel_values is not None or visual_features is not None:
            vit = visual_features if visual_features is not None else self.extract_feature(pixel_values)
            vis = vit.reshape(-1, vit.shape[-1]).to(dev).contiguous()
            n_vis = vis.shape[0]
            sel = ids_packed == self.img_context_token_id
            assert int(sel.sum()) != 0
            if int(sel.sum()) != n_vis:
                raise ValueError(f"visual token count mismatch: {int(sel.sum())} slots vs {n_vis} tokens")
            slot[sel] = torch.arange(n_vis, device=dev, dtype=torch.int32)
        return self._greedy(ids_packed, slot, cu, vis, n_vis, max_new, eos, pad, **how)

    @torch.no_grad()
    def generate2(self, input_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, visual_features=None,
                  generation_config=None, output_hidden_states=None, return_dict=None, key_drop=None, **generate_kwargs) -> torch.Tensor:
        """modeling_internvl_chat.py:812-853: decode from precomputed input embeddings [B, N, C].  Output flags, ``candidate_ids``, ``top_logprobs`` and
        ``key_drop`` (laid out like the embeddings' [B, N]) as ``generate``."""
        max_new, eos, pad, how = self._gen_setup(generation_config, generate_kwargs)
        dev = self.device
        b, n, _ = input_embeds.shape
        if key_drop is not None:        # checked in full on the host first
            mask_h = torch.ones((b, n), dtype=torch.bool) if attention_mask is None else attention_mask.detach().to("cpu").bool()
            _, cu_h, row_of = self._pack(torch.zeros((b, n), dtype=torch.long), mask_h)
            how["drop_words"] = self._gen_drop_words(key_drop, (b, n), cu_h, row_of)
        mask = torch.ones((b, n), dtype=torch.bool, device=dev) if attention_mask is None else attention_mask.to(dev).bool()
        emb = input_embeds.to(dev)[mask].to(torch.bfloat16).contiguous()
        cu = list(accumulate((int(x) for x in mask.sum(1).tolist()), initial=0))
        T = emb.shape[0]
        ids = torch.zeros(T, dtype=torch.long, device=dev)
        slot = torch.arange(T, dtype=torch.int32, device=dev)          # every row comes from `emb`
        return self._greedy(ids, slot, cu, emb, T, max_new, eos, pad, **how)

    @torch.no_grad()
    def generate_stage2(self, pixel_values, input_ids, attention_mask=None, image_flags=None, motion_feature=None,
                        generation_config=None, visual_tokens=None, key_drop=None, **generate_kwargs) -> torch.LongTensor:
        """Greedy decode behind a stage-2 prompt: the embedding assembly of the reference's ``chat2``
        (modeling_internvl_chat.py:642-707: all <IMG_CONTEXT> slots but the last of each clip take visual tokens, the last one the
        motion token) followed by its ``generate2``.  Ids and slot map go to the native prefill, whose embed kernel gathers
        token / visual / motion rows - no embedding tensor is assembled on the host side.

        ``visual_tokens`` (``vit_tokens(pixel_values)``, with ``motion_feature``): the visual front computed once and handed to several calls, as
        ``forward`` takes them; ``pixel_values`` may then be None.  ``key_drop`` [B, N] as ``generate``: ``unit_masks`` builds the per-frame masks,
        ``eval_utils.frame_ablation_generate`` the per-frame replies."""
        if self.img_context_token_id is None:
            raise AssertionError("img_context_token_id must be set (stage2_eval.py:810)")
        max_new, eos, pad, how = self._gen_setup(generation_config, generate_kwargs)
        B = input_ids.shape[0]
        n_frames = visual_tokens.shape[0] if visual_tokens is not None else pixel_values.shape[0]
        plan = self._plan(input_ids, attention_mask, None, image_flags, n_frames, drop_dead_tail=False)
        how["drop_words"] = self._gen_drop_words(key_drop, input_ids.shape, plan["cu"], plan["row_of"])      # (host only: before anything is launched)
        motion_feature = self._motion_feature(pixel_values, B, motion_feature)
        self._native(n_frames=n_frames, n_tokens=plan["cu"][-1], n_clips=B)
        vit_embeds, motion = self._visual_inputs(pixel_values, visual_tokens, motion_feature, plan)
        return self._greedy(plan["ids_packed"], plan["slot"], plan["cu"], vit_embeds, plan["n_vis"], max_new, eos, pad, motion=motion, **how)

    def chat2(self, tokenizer, pixel_values, input_ids, generation_config, attention_mask, history=None,
              return_history=False, image_flags=None, IMG_START_TOKEN="<img>", IMG_END_TOKEN="</img>",
              IMG_CONTEXT_TOKEN="<IMG_CONTEXT>", verbose=False, motion_feature=None, key_drop=None):
        """modeling_internvl_chat.py:638-767: pre-tokenised stage-2 prompt (with the motion slot) -> decoded response.  ``key_drop`` as
        ``generate_stage2``: the response with those prompt tokens hidden."""
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        template = get_conv_template(self.template)
        generation_config["eos_token_id"] = tokenizer.convert_tokens_to_ids(template.sep)
        out = self.generate_stage2(pixel_values, input_ids, attention_mask, image_flags, motion_feature, key_drop=key_drop, **generation_config)
        response = tokenizer.batch_decode(out, skip_special_tokens=True)[0].split(template.sep)[0].strip()
        return (response, history) if return_history else response

    def chat(self, tokenizer, pixel_values, question, generation_config, history=None, return_history=False,
             num_patches_list=None, IMG_START_TOKEN="<img>", IMG_END_TOKEN="</img>", IMG_CONTEXT_TOKEN="<IMG_CONTEXT>",
             verbose=False):
        """modeling_internvl_chat.py:582-636 (mutates generation_config['eos_token_id'] like the reference)."""
        if history is None and pixel_values is not None and "<image>" not in question:
            question = "<image>\n" + question
        if num_patches_list is None:
            num_patches_list = [pixel_values.shape[0]] if pixel_values is not None else []
        assert pixel_values is None or len(pixel_values) == sum(num_patches_list)
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        template = get_conv_template(self.template)
        template.system_message = self.system_message
        eos_token_id = tokenizer.convert_tokens_to_ids(template.sep)
        history = [] if history is None else history
        for old_q, old_a in history:
            template.append_message(template.roles[0], old_q)
            template.append_message(template.roles[1], old_a)
        template.append_message(template.roles[0], question)
        template.append_message(template.roles[1], None)
        query = template.get_prompt()
        for num_patches in num_patches_list:
            image_tokens = IMG_START_TOKEN + IMG_CONTEXT_TOKEN * self.num_image_token * num_patches + IMG_END_TOKEN
            query = query.replace("<image>", image_tokens, 1)
        model_inputs = tokenizer(query, return_tensors="pt")
        generation_config["eos_token_id"] = eos_token_id
        out = self.generate(pixel_values=pixel_values, input_ids=model_inputs["input_ids"],
                            attention_mask=model_inputs["attention_mask"], **generation_config)
        response = tokenizer.batch_decode(out, skip_special_tokens=True)[0].split(template.sep)[0].strip()
        history.append((question, response))
        if return_history:
            return response, history
        if verbose:
            print(query.replace(IMG_CONTEXT_TOKEN, "").replace(f"{IMG_START_TOKEN}{IMG_END_TOKEN}", "<image>"), response)
        return response

    def batch_chat(self, tokenizer, pixel_values, questions, generation_config, num_patches_list=None, history=None,
                   return_history=False, IMG_START_TOKEN="<img>", IMG_END_TOKEN="</img>",
                   IMG_CONTEXT_TOKEN="<IMG_CONTEXT>", verbose=False, image_counts=None):
        """modeling_internvl_chat.py:533-580 (left padding is stripped by the packed layout)."""
        if history is not None or return_history:
            raise NotImplementedError("Now multi-turn chat is not supported in batch_chat.")
        if image_counts is not None:
            num_patches_list = image_counts
        self.img_context_token_id = tokenizer.convert_tokens_to_ids(IMG_CONTEXT_TOKEN)
        queries = []
        template = None
        for idx, num_patches in enumerate(num_patches_list):
            question = questions[idx]
            if pixel_values is not None and "<image>" not in question:
                question = "<image>\n" + question
            template = get_conv_template(self.template)
            template.system_message = self.system_message
            template.append_message(template.roles[0], question)
            template.append_message(template.roles[1], None)
            query = template.get_prompt()
            image_tokens = IMG_START_TOKEN + IMG_CONTEXT_TOKEN * self.num_image_token * num_patches + IMG_END_TOKEN
            queries.append(query.replace("<image>", image_tokens, 1))
        tokenizer.padding_side = "left"
        model_inputs = tokenizer(queries, return_tensors="pt", padding=True)
        generation_config["eos_token_id"] = tokenizer.convert_tokens_to_ids(template.sep)
        out = self.generate(pixel_values=pixel_values, input_ids=model_inputs["input_ids"],
                            attention_mask=model_inputs["attention_mask"], **generation_config)
        responses = tokenizer.batch_decode(out, skip_special_tokens=True)
        return [r.split(template.sep)[0].strip() for r in responses]

