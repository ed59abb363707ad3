"""Greedy decoding with a static KV cache under hipGraph replay.

Replaces the reference's cache-free sampling loop (models/vision_encoder_decoder.py:136-182 with ``top_k=1``,
``temperature=1``): there every new token re-runs the whole decoder over all t tokens and synchronises with the host
for the n-gram ban (``.tolist()``).  Here
  * the encoder runs once, the cross-attention K/V of every cross layer are projected once per image;
  * one decode step = one token per caption through single-row kernels: LayerNorm -> QKV GEMM -> append K/V to the
    cache -> attention of the new query against keys 0..pos -> projections / MLP with fused residuals -> ln_f ->
    tied lm_head (fp32 logits) -> on-device no-repeat-n-gram ban + argmax that appends the token to the id buffer;
  * every position-dependent kernel reads ``pos`` / ``len`` from device memory, so the step is captured ONCE into a
    hipGraph and replayed per token: no host sync, no per-step launch overhead, token ids never leave the GPU until
    the end.
Because text rows never attend to the soft-prompt columns (see engine.py) the cache holds text positions only; the
prompt shifts the position embedding by n_cls.

The sampling modes of ``generate`` (temperature / top-k / nucleus, reference :152-180; ``eval_model``'s call shape
trainer.py:41-56) run on the same cached step: only its last kernel differs -- ``i2t_sample_token`` (csrc/sample.hip)
instead of the ban + argmax -- so a sampled token also costs one hipGraph replay and no host sync.  The draw is a
counter-based function of (seed, step, row): ``Sampling.seed`` comes from torch's CPU generator once per call, so
``torch.manual_seed`` reproduces a run.

This module holds the device drivers and re-exports its device-free siblings: caption_plan.py says what a call means (argument
tuples, window and cache planners, every refusal, ``plan_captions``), phrase_trie.py builds the phrase tries and their level tables,
decoding_host.py holds the numpy statements the kernels are tested against.
"""
import os
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import ops
from .caption_plan import (BEAM_DEAD, DECODE_LONG_MAX_KEYS, DECODE_MAX_KEYS, LONG_CHUNK_KEYS, LONG_HEAD_DIMS, MAX_CAPTION_BEAMS, MAX_TOP_LOGPROBS,
                           PROMPT_PREFILL_MODES, BeamSpec, CaptionFacts, CaptionPlan, ClosedSet, GeneratedCaptions, PhraseBeams, PhraseScores,
                           Processors, Sampling, PhraseSets, PhraseSetScores, cache_plan, caption_graph_key, caption_processors,
                           check_beam_caption_args, check_caption_args, check_phrase_caption_args, check_phrase_score_args,
                           check_phrase_search_args, check_phrase_set_caption_args, check_phrase_set_score_args, check_phrase_sets,
                           check_ragged_caption_args, check_top_logprobs, closed_set, decode_window, held_phrase_trie, one_closed_set, per_image_closed_set,
                           phrase_beam_sets_graph_key, plan_captions, plan_phrase_scores, plan_phrase_search, prefill_plan, row_images, takes_long_cache,
                           text_window, trie_widest_level)
from .decoding_host import (_finish_rows, apply_finish_rule, apply_finish_rule_ragged, banned_log_softmax_host, beam_advance_host,
                            beam_pool_select_host, beam_search_host, constrained_decode_host, kv_prefill_host, phrase_beam_search_host,
                            phrase_scores_host, phrase_set_scores_host, process_logits_host, slot_positions, split_attention_host, trie_advance_host,
                            trie_advance_ragged_host, trie_beam_candidates_host, trie_beam_select_host, trie_beam_select_sets_host,
                            top_logprobs_host, trie_mask_host, trie_mask_ragged_host)
from .engine import BF16, F32, HotPath
from .phrase_trie import (PhraseForest, PhraseTrie, SetLevelTables, TrieLevel, TrieLevels, level_expand_tables, phrase_forest, phrase_node_csr,
                          phrase_trie, set_level_tables, set_step_state, trie_levels)

assert LONG_CHUNK_KEYS == ops.LONG_CHUNK_KEYS       # caption_plan.py loads no library: it keeps the figure, ops.py the kernels' copy


ENC_CHUNK = int(os.environ.get('I2T_DECODE_ENC_CHUNK', '4096'))      # images per encoder pass inside generate()
TOP2_HEAD = os.environ.get('I2T_DECODE_TOP2', '1') not in ('', '0')    # greedy steps: lm_head + argmax through segment maxima (ops.gemm_top2)


PREFILL_ROWS = int(os.environ.get('I2T_PREFILL_ROWS', '8192'))       # token rows per forward pass of prompt_prefill='pass' 


class GreedyDecoder:
    """KV-cache decoder; greedy by default, ``generate(..., sampling=Sampling(...))`` draws tokens on the device instead."""

    def __init__(self, model):
        self.model = model
        self.eng: HotPath = model._engine
        self._state = None
        self._long_state = None             # the state of calls past text_window (cache_plan): classic calls never run on it
        self._state_mem = self._long_state_mem = None       # the two under ``image_index``: a call without it never runs on them

    # ------------------------------------------------------------------------------------------------ buffers
    def _cache_args(self):
        """(block, off, prefix, llama) of this model, as decode_window and cache_plan take them"""
        eng, dc = self.eng, self.eng.dec
        ncls = eng.enc.ncls
        return (dc.block, ncls if self.model.config.use_soft_prompting else 0, min(ncls, dc.block) if dc.prefixed else 0,
                takes_long_cache(dc.llama))

    def _state_for(self, rows: int, total: int, build, extra=None, mem=None):
        """The cached state that serves a call over ``rows`` rows and ``total`` id columns, (re)built by ``build(clen)`` -- clen None: the
        classic window's -- when the cached one does not (_reusable).  A call that fits text_window runs on self._state, whatever ran
        before; one past it (takes_long_cache) on self._long_state, rebuilt when it holds fewer cache slots than the call needs.  A call
        past decode_window is cache_plan's ValueError.  ``mem`` = (memory rows, indexed) of a caller that knows them: an
        ``image_index`` call runs on states of its own (self._state_mem / self._long_state_mem) -- its steps launch other cross-attention
        kernels and its graphs bake st.mem_index --, rebuilt when the number of images differs; a call without it never sees them."""
        block, off, prefix, llama = self._cache_args()
        clen, long = cache_plan(block, off, prefix, total, llama)
        slot = ('_long_state' if long else '_state') + ('_mem' if mem is not None and mem[1] else '')
        st = getattr(self, slot)
        if not self._reusable(st, rows, total, lambda st: (not long or st.clen >= clen) and (extra is None or extra(st)) and
                              (mem is None or (st.mem_rows == mem[0] and (st.mem_index is not None) == mem[1]))):
            setattr(self, slot, None)                           # the old buffers go before the new ones are made
            st = build(clen if long else None)
            setattr(self, slot, st)
        assert total <= st.tmax
        return st

    def _build(self, B: int, ids_ld: int, mem_rows: Optional[int] = None, clen: Optional[int] = None, indexed: bool = False):
        """Buffers of a step over B rows; the cross-attention memory holds ``mem_rows`` (default B) rows -- the images, when the B
        rows are beams of them (BeamDecoder).  ``clen``: the cache slots per row of a long state (cache_plan), whose self-attention
        runs the split-key kernels over st.attn_ws; None: the classic window.  ``indexed`` (``image_index``): the rows
        reach the ``mem_rows`` memory rows through the table st.mem_index, int32 [B], persistent because captured graphs bake its
        pointer; its contents are written per call (_set_mem_index)."""
        eng, a = self.eng, self.eng.arena
        dc = eng.dec
        dev = a.device
        cfg = self.model.config
        ncls = eng.enc.ncls
        off = ncls if cfg.use_soft_prompting else 0
        d, ff = dc.d, dc.ff
        # Hugging Face decoder + soft prompt (engine.decode_prefixed): the encoder outputs are the first cache positions of every caption
        prefix = min(ncls, dc.block) if dc.prefixed else 0
        tmax = text_window(dc.block, off, prefix) if clen is None else clen - prefix
        st = SimpleNamespace(B=B, ids_ld=ids_ld, off=off, tmax=tmax, arena=a, sparse_epoch=eng.sparse_epoch, prefix=prefix,
                             clen=tmax + prefix)
        e = lambda *s, dtype=BF16: torch.zeros(*s, dtype=dtype, device=dev)
        st.ids = torch.zeros(B, ids_ld, dtype=torch.long, device=dev)
        st.counters = torch.zeros(2, dtype=torch.int32, device=dev)        # [pos, len]
        st.counters_init = torch.tensor([prefix, 1], dtype=torch.int32, device=dev)
        st.x = e(B, d, dtype=F32)
        st.ln = e(B, d)
        st.qkv = e(B, 3 * d)
        st.ao = e(B, d)
        st.q = e(B, d)
        st.h = e(B, ff)
        st.hid = e(B, d)
        st.logits = e(B, dc.Vp, dtype=F32)                      # rows padded to 8 columns: 16-byte aligned rows for the GEMM epilogue
        st.margin = e(B, dtype=F32)
        st.top2 = st.seg_se = None          # the segment-maxima head's buffers, made at the first step that takes it (_greedy_head)
        # fp32 planes of the deterministic split-K GEMM form (ops.gemm(workspace=...)): the step's GEMMs with few output tiles and a
        # long K (attention / MLP output projections at anything but the largest caption batches) spread over K slices
        st.ws = torch.empty(16 << 20, dtype=F32, device=dev)
        st.attn_ws = None                   # a long state's chunk partials (below)
        if dc.llama is not None:
            ls = dc.llama
            st.qkv, st.ao, st.gu = e(B, (ls.H + 2 * ls.Hkv) * ls.hd), e(B, ls.H * ls.hd), e(B, 2 * ff)
            st.kc = [e(B, st.clen, ls.Hkv * ls.hd) for _ in range(dc.L)]
            st.vc = [e(B, st.clen, ls.Hkv * ls.hd) for _ in range(dc.L)]
            if st.clen > DECODE_MAX_KEYS:                       # one layer's chunk partials at a time: every layer overwrites them
                st.attn_ws = torch.empty(ops.gq_decode_long_workspace_floats(B, ls.H, st.clen, ls.hd), dtype=F32, device=dev)
        elif dc.fam is None:
            st.kc = [e(B, st.clen, d) for _ in range(dc.L)]
            st.vc = [e(B, st.clen, d) for _ in range(dc.L)]
        S = ncls
        st.cross_kv = {l: (e(mem_rows or B, S, 2 * d), S) for l in self._cross_layers()}
        st.hist = st.hist_init = None       # beam search: int32 [B][clen] history table (BeamDecoder), None: row b's keys are row b's
        st.ctrl = None                      # int32 [done, unfinished]: the modes that stop early (_reset clears it, _replay polls it)
        st.mem_div = 1                      # rows per cross-attention memory row
        st.mem_rows = mem_rows or B         # the cross-attention memory's rows
        st.mem_index = torch.zeros(B, dtype=torch.int32, device=dev) if indexed else None      # row -> memory row; None: row // st.mem_div
        if dc.fam is not None:
            self._build_family(st, e)
        if dc.advpos:
            st.pos_h = [e(B, g) for g in (self.eng.dcfg.advanced_pos_emb_gate_sizes or ())]
        st.ngrams = torch.tensor(list(cfg.no_repeat_n_grams), dtype=torch.int32, device=dev)
        st.graphs = {}                      # None -> prefill step, 'greedy' / Sampling.key() -> full step
        st.seed = torch.zeros(2, dtype=torch.int32, device=dev)
        st.dist = None                      # optional [B, V] f32: the distribution of the last sampled step (tests)
        return st

    def _build_family(self, st, e):
        """Buffers of the nano-mini family's decode step (engine_family.py): a K/V cache of Hkv heads per layer that, in a sparse
        layer, holds the kept positions only (slot = number of kept positions before the token), the per-layer slot / membership
        tables, and the MoE routing workspaces."""
        eng, dc = self.eng, self.eng.dec
        sp, dev = dc.fam, st.arena.device
        B, d, hd, tmax, off = st.B, dc.d, sp.hd, st.tmax, st.off
        st.Hkv = 1 if sp.mqa else dc.H
        st.slots = tmax
        st.sparse = sp.sparse
        if sp.sparse:
            rank, member = np.zeros((dc.L, tmax), dtype=np.int32), np.zeros((dc.L, tmax), dtype=np.int32)
            for l, (idx, _not) in enumerate(eng._sparse_idx['dec']):
                if int((idx < off + 1).sum()) < 2:
                    # layers.py:572-573 sends the WHOLE sequence through the null connector while <= 1 position is kept; a token's
                    # state would then depend on the current length and could not be cached
                    raise NotImplementedError('KV-cache generation with sparse decoder blocks needs >= 2 kept positions before the '
                                              'first text token (a soft prompt of >= 2 encoder outputs)')
                if off + tmax > idx.size + _not.size:
                    raise AssertionError('block_size + prompt exceeds max_block_size of the sparse decoder blocks')
                text = np.zeros(off + tmax, dtype=np.int32)
                text[idx[idx < off + tmax]] = 1
                member[l] = text[off:]
                rank[l] = np.cumsum(member[l]) - member[l]
            kpos = slot_positions(member)
            st.slots = kpos.shape[1]
            # beam search reads key s of a sparse layer from row hist[r][kpos[l][s]] (i2t_beam_gq_decode_attention's slot_pos)
            assert int(kpos.max()) < st.clen, 'a kept position lies beyond the beam history table'
            st.rank, st.member = torch.from_numpy(rank).to(dev), torch.from_numpy(member).to(dev)
            st.kpos = torch.from_numpy(kpos).to(dev)
            st.lpos = torch.zeros(dc.L, dtype=torch.int32, device=dev)
            st.lmem = torch.zeros(dc.L, dtype=torch.int32, device=dev)
            st.xb, st.xn, st.xnb = e(B, d, dtype=F32), e(B, d, dtype=F32), e(B, d)
        w = st.Hkv * hd
        st.kc = [e(B, st.slots, w) for _ in range(dc.L)]
        st.vc = [e(B, st.slots, w) for _ in range(dc.L)]
        st.kvn = e(B, 2 * w)
        if sp.moe is not None:
            m = sp.moe
            st.U = e(B, m.E * m.P + (m.G if m.G else m.E), dtype=F32)
            st.A = e(B, m.Kp)
            st.gates, st.wsel = e(B, m.E, dtype=F32), e(B, m.E, dtype=F32)

    def _moe_step(self, st, pfx: str, x_bf, y, act: int, residual):
        eng, m = self.eng, self.eng.dec.fam.moe
        mv = eng._moe_views(pfx, m)
        ops.gemm(x_bf, mv.W1, st.U, st.B, mv.N1, mv.in_f, bias=mv.b1)
        ops.moe_gate_fwd(st.U, mv.wg2, mv.bg2, st.A, st.gates, st.wsel, st.B, m.E, m.P, m.G, m.top_k, mv.in_f ** -0.5)
        ops.gemm(st.A, mv.W2aug, y, st.B, mv.out_f, m.Kp, act=act, residual=residual)

    def _layers_family(self, st):
        """The decoder blocks of one decode step for the nano-mini family.  A sparse layer computes both of its paths for the new
        token -- the block (whose K/V land in the layer's next free cache slot: a skipped token's entry is overwritten by the next
        kept one before anything reads it) and x + null_connector(x) -- and keeps the one its position table selects; which
        one is a device-side flag, so the captured graph is the same for every position."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        sp = dc.fam
        B, d, ff, H, hd, Hkv = st.B, dc.d, dc.ff, dc.H, sp.hd, st.Hkv
        w = Hkv * hd
        dp = eng.dp
        if st.sparse:
            ops.sparse_step_setup(st.counters[0:1], st.rank, st.member, st.lpos, st.lmem, dc.L, st.tmax)
        for l in range(dc.L):
            p = f'{dp}transformer.h.{l}'
            xo = st.xb if st.sparse else st.x
            pos_ptr = st.lpos[l:l + 1] if st.sparse else st.counters[0:1]
            ops.layernorm_fwd(st.x, a.P(f'{p}.ln_1.weight'), a.P(f'{p}.ln_1.bias'), st.ln, None, None, B, d)
            if sp.mqa:
                ops.gemm(st.ln, a.W(f'{p}.attn.q_proj.weight'), st.q, B, d, d, bias=a.P(f'{p}.attn.q_proj.bias'), workspace=st.ws)
                ops.gemm(st.ln, a.W(f'{p}.attn.kv_proj.weight'), st.kvn, B, 2 * hd, d, bias=a.P(f'{p}.attn.kv_proj.bias'), workspace=st.ws)
                qv, kn, vn, out_name = st.q, st.kvn[:, :hd], st.kvn[:, hd:], 'attn.out_proj'
            else:
                ops.gemm(st.ln, a.W(f'{p}.attn.c_attn.weight'), st.qkv, B, 3 * d, d, bias=a.P(f'{p}.attn.c_attn.bias'), workspace=st.ws)
                qv, kn, vn, out_name = st.qkv[:, :d], st.qkv[:, d:2 * d], st.qkv[:, 2 * d:], 'attn.c_proj'
            self._self_attention(st, l, pos_ptr, (qv, kn, vn, H, Hkv, hd, st.slots), slot_pos=st.kpos[l] if st.sparse else None)
            ops.gemm(st.ao, a.W(f'{p}.{out_name}.weight'), xo, B, d, d, bias=a.P(f'{p}.{out_name}.bias'), residual=st.x, workspace=st.ws)
            if l in st.cross_kv:
                win, bin_ = a.W(f'{p}.cross_attn.in_proj_weight'), a.P(f'{p}.cross_attn.in_proj_bias')
                ops.layernorm_fwd(xo, a.P(f'{p}.ln_3.weight'), a.P(f'{p}.ln_3.bias'), st.ln, None, None, B, d)
                ops.gemm(st.ln, win[:d], st.q, B, d, d, bias=bin_[:d], workspace=st.ws)
                self._cross_attention(st, l, hd)
                ops.gemm(st.ao, a.W(f'{p}.cross_attn.out_proj.weight'), xo, B, d, d, bias=a.P(f'{p}.cross_attn.out_proj.bias'), residual=xo, workspace=st.ws)
            ops.layernorm_fwd(xo, a.P(f'{p}.ln_2.weight'), a.P(f'{p}.ln_2.bias'), st.ln, None, None, B, d)
            if sp.moe is not None:
                self._moe_step(st, f'{p}.mlp.c_fc', st.ln, st.h, 1, None)
                self._moe_step(st, f'{p}.mlp.c_proj', st.h, xo, 0, xo)
            else:
                ops.gemm(st.ln, a.W(f'{p}.mlp.c_fc.weight'), st.h, B, ff, d, bias=a.P(f'{p}.mlp.c_fc.bias'), act=1, workspace=st.ws)
                ops.gemm(st.h, a.W(f'{p}.mlp.c_proj.weight'), xo, B, d, ff, bias=a.P(f'{p}.mlp.c_proj.bias'), residual=xo, workspace=st.ws)
            if st.sparse:
                ops.cast_f32_bf16(st.x, st.xnb)
                ops.gemm(st.xnb, a.W(f'{p}.null_connector.weight'), st.xn, B, d, d, bias=a.P(f'{p}.null_connector.bias'), residual=st.x, workspace=st.ws)
                ops.select_rows(st.lmem[l:l + 1], st.xb, st.xn, st.x, B * d)

    def _cross_layers(self):
        cfg = self.model.config
        return [l for l in range(self.eng.dec.L)
                if self.eng.cross_inputs and (self.eng.dec_cross[l] or not self.eng.dcfg.skip_alternate_cross_attn)]

    # ------------------------------------------------------------------------------------------------ one token
    def _step(self, st, with_head: bool, sampling: Optional[Sampling] = None, top2: bool = False):
        """Consume the token at ids[:, pos]; when with_head also choose ids[:, len] (argmax after the n-gram ban, or a draw from
        the filtered distribution when ``sampling`` is given); then advance pos and len."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        B, d = st.B, dc.d
        len_ptr = st.counters[1:2]
        if not with_head:
            self._body(st)
        elif top2 and sampling is None:
            # greedy, nobody asked for margins: the lm_head leaves the two largest logits of every 64-column segment of a row
            # instead of the row (51 MB instead of 823 MB written and read back at 4096 captions), the ban + argmax merges them
            self._body(st)
            self._final_norm(st)
            ops.gemm_top2(st.hid, a.W(eng.n_head), st.top2, B, dc.V, d)
            ops.top2_ngram_argmax(st.top2, st.hid, a.W(eng.n_head), st.ids, st.ids_ld, len_ptr, st.ngrams, st.ngrams.numel(), B, dc.V, d)
        else:
            self._logits_head(st)
            if sampling is None:
                ops.ngram_ban_argmax(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, st.ngrams.numel(), B, dc.V, st.margin)
            else:
                ops.sample_token(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, st.ngrams.numel(), B, dc.V,
                                 sampling.temperature, sampling.top_k, sampling.nucleus_p, st.seed, dist_out=st.dist)
        ops.advance(st.counters, 1)                            # pos and len together

    def _logits_head(self, st):
        """The step up to its raw logits, for every mode that reads the whole row: _body, _final_norm, the fp32 lm_head into st.logits."""
        self._body(st)
        self._final_norm(st)
        dc = self.eng.dec
        ops.gemm(st.hid, self.eng.arena.W(self.eng.n_head), st.logits, st.B, dc.V, dc.d, workspace=st.ws)

    def _body(self, st):
        """Embedding of the token at ids[:, len - 1] and the decoder blocks at position pos: st.x holds the new hidden rows."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        B, d = st.B, dc.d
        pos_ptr, len_ptr = st.counters[0:1], st.counters[1:2]
        dp = eng.dp
        ops.embed_step(st.ids, st.ids_ld, len_ptr, a.P(eng.n_wte),
                       None if (dc.advpos or dc.llama is not None) else a.P(f'{dp}transformer.wpe.weight'), st.x, B, d, st.off, dc.V)
        if dc.advpos:           # x = MLP_p(e) + e with p = off + pos read on the device: the same captured launches serve every position
            pv = eng._pos_views()
            ops.cast_f32_bf16(st.x, st.ln)
            h = st.ln
            for i, L in enumerate(pv.layers):
                last = i == len(pv.layers) - 1
                out = st.x if last else st.pos_h[i]
                ops.grouped_gemm(0, h, L.W[:L.N * L.K].view(L.N, L.K), out, L.N, L.K, b_group_stride=pv.stride, bias=L.b,
                                 bias_group_stride=pv.stride, act=0 if last else 1, residual=st.x if last else None, n_groups=1, max_rows=B,
                                 group_ptr=pos_ptr, group0=st.off)
                h = out
        if dc.llama is not None:
            self._layers_llama(st)
        elif dc.fam is not None:
            self._layers_family(st)
        else:
            self._layers_dense(st)

    def _final_norm(self, st):
        """st.hid = the final norm of st.x (the lm_head's input)."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        B, d, dp = st.B, dc.d, eng.dp
        if dc.llama is not None and dc.llama.arch == 'falcon':
            wn = dp + dc.llama.norm_f
            ops.layernorm_fwd(st.x, a.P(wn + '.weight'), a.P(wn + '.bias'), st.hid, None, None, B, d, eps=dc.llama.eps)
        elif dc.llama is not None:
            ops.rmsnorm_fwd(st.x, a.P(dp + dc.llama.norm_f + '.weight'), st.hid, None, B, d, dc.llama.eps)
        else:
            ops.layernorm_fwd(st.x, a.P(f'{dp}transformer.ln_f.weight'), a.P(f'{dp}transformer.ln_f.bias'), st.hid, None, None, B, d)

    def _w(self, l: int, site: str, name: str, rows=None):
        """bf16 weight of a decoder linear for the decode step: the arena's shadow, or -- under a LoRA adapter -- the merged
        W + s B A in its persistent buffer (engine_lora.py; generation has no dropout, so merging is exact)"""
        eng = self.eng
        if eng._lora_site(l, site) is not None:
            return eng.lora_merged(l, site, name, rows)
        w = eng.arena.W(name)
        return w if rows is None else w[rows]

    def _layers_dense(self, st):
        """The decoder blocks of one decode step for the dense multi-head model (64-wide heads, GELU-MLP)."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        B, d, ff, H = st.B, dc.d, dc.ff, dc.H
        pos_ptr = st.counters[0:1]
        dp = eng.dp
        for l in range(dc.L):
            p = f'{dp}transformer.h.{l}'
            ops.layernorm_fwd(st.x, a.P(f'{p}.ln_1.weight'), a.P(f'{p}.ln_1.bias'), st.ln, None, None, B, d)
            ops.gemm(st.ln, self._w(l, 'attn_c_attn', f'{p}.attn.c_attn.weight'), st.qkv, B, 3 * d, d, bias=a.P(f'{p}.attn.c_attn.bias'),
                     workspace=st.ws)
            self._self_attention(st, l, pos_ptr)
            ops.gemm(st.ao, a.W(f'{p}.attn.c_proj.weight'), st.x, B, d, d, bias=a.P(f'{p}.attn.c_proj.bias'), residual=st.x, workspace=st.ws)
            if l in st.cross_kv:
                win, bin_ = a.W(f'{p}.cross_attn.in_proj_weight'), a.P(f'{p}.cross_attn.in_proj_bias')
                ops.layernorm_fwd(st.x, a.P(f'{p}.ln_3.weight'), a.P(f'{p}.ln_3.bias'), st.ln, None, None, B, d)
                ops.gemm(st.ln, win[:d], st.q, B, d, d, bias=bin_[:d], workspace=st.ws)
                self._cross_attention(st, l)
                ops.gemm(st.ao, a.W(f'{p}.cross_attn.out_proj.weight'), st.x, B, d, d,
                         bias=a.P(f'{p}.cross_attn.out_proj.bias'), residual=st.x, workspace=st.ws)
            ops.layernorm_fwd(st.x, a.P(f'{p}.ln_2.weight'), a.P(f'{p}.ln_2.bias'), st.ln, None, None, B, d)
            ops.gemm(st.ln, self._w(l, 'mlp_c_fc', f'{p}.mlp.c_fc.weight'), st.h, B, ff, d, bias=a.P(f'{p}.mlp.c_fc.bias'), act=1, workspace=st.ws)
            ops.gemm(st.h, self._w(l, 'mlp_c_proj', f'{p}.mlp.c_proj.weight'), st.x, B, d, ff, bias=a.P(f'{p}.mlp.c_proj.bias'), residual=st.x,
                     workspace=st.ws)

    def _layers_llama(self, st):
        """The Llama-2 / Qwen2 blocks of one decode step (engine_llama.py): the rotary angle is looked up at the position counter on
        the device (absolute position = cache slot: prompt rows first), so one captured graph serves every step."""
        eng, dc, ls = self.eng, self.eng.dec, self.eng.dec.llama
        B, d, ff, H, G, hd = st.B, dc.d, dc.ff, ls.H, ls.Hkv, ls.hd
        pos_ptr = st.counters[0:1]
        cs = eng.rope_table()
        for l in range(dc.L):
            v = eng._llama_views(l)
            if getattr(dc, 'lora', None) is not None:          # merged W + s B A per adapted projection (engine_lora.lora_merged)
                nm = v.names
                Wqkv, Wo, Wgu, Wdn = (eng.lora_merged(l, site, names) if eng._llama_lora(l, site) is not None else W for site, names, W in
                                      (('qkv', nm.qkv, v.Wqkv), ('o', nm.o, v.Wo), ('gu', nm.gu, v.Wgu), ('dn', nm.dn, v.Wdn)))
                v = SimpleNamespace(**{**vars(v), 'Wqkv': Wqkv, 'Wo': Wo, 'Wgu': Wgu, 'Wdn': Wdn})
            if ls.arch == 'falcon':        # n = LN(x);  x += dense(attn(rope(qkv(n)))) + W2 gelu(W1 n)   (engine_llama.falcon_block_fwd)
                ops.layernorm_fwd(st.x, v.n1, v.b1, st.ln, None, None, B, d, eps=ls.eps)
                ops.gemm(st.ln, v.Wqkv, st.qkv, B, v.nq, d, workspace=st.ws)
                ops.rope(st.qkv, v.nq, 0, H + G, hd, cs, B, pos_ptr=pos_ptr)
                self._gq_self_attention(st, l, H, G, hd)
                ops.gemm(st.ao, v.Wo, st.x, B, d, H * hd, residual=st.x, workspace=st.ws)
                ops.gemm(st.ln, v.Wgu, st.h, B, ff, d, act=ops.ACT_GELU_ERF)
                ops.gemm(st.h, v.Wdn, st.x, B, d, ff, residual=st.x, workspace=st.ws)
                continue
            ops.rmsnorm_fwd(st.x, v.n1, st.ln, None, B, d, ls.eps)
            ops.gemm(st.ln, v.Wqkv, st.qkv, B, v.nq, d, bias=v.bqkv, workspace=st.ws)
            ops.rope(st.qkv, v.nq, 0, H + G, hd, cs, B, pos_ptr=pos_ptr)
            self._gq_self_attention(st, l, H, G, hd)
            ops.gemm(st.ao, v.Wo, st.x, B, d, H * hd, residual=st.x, workspace=st.ws)
            ops.rmsnorm_fwd(st.x, v.n2, st.ln, None, B, d, ls.eps)
            ops.gemm(st.ln, v.Wgu, st.gu, B, 2 * ff, d, workspace=st.ws)
            ops.swiglu_fwd(st.gu, st.h, B, ff)
            ops.gemm(st.h, v.Wdn, st.x, B, d, ff, residual=st.x, workspace=st.ws)

    def _gq_self_attention(self, st, l: int, H: int, G: int, hd: int):
        """Self-attention of a Llama-2 / Qwen2 / Falcon decode step over the row-major cache [B][slot][G hd] (packed q | k | v rows)."""
        q, k, v = st.qkv[:, :H * hd], st.qkv[:, H * hd:(H + G) * hd], st.qkv[:, (H + G) * hd:]
        self._self_attention(st, l, st.counters[0:1], (q, k, v, H, G, hd, st.clen))

    def _self_attention(self, st, l: int, pos_ptr, gq=None, slot_pos=None):
        """st.ao = layer l's new query over its self-attention cache, the token's K/V appended at *pos_ptr.  gq = (q, k, v, H, Hkv, hd,
        slots): the row-major cache [B][slots][Hkv hd]; None: the dense model's packed st.qkv row and head-major cache
        [B][H][prefix + tmax][64].  Beam search (st.hist) reads the keys through its history table, a sparse layer's through slot_pos."""
        B, d = st.B, self.eng.dec.d
        if gq is None:
            args = (st.qkv, 3 * d, st.kc[l], st.vc[l], st.clen * d, 64, st.ao, d, pos_ptr, 0, B, self.eng.dec.H)
            kw = dict(append_dm=d, cache_hs=st.clen * 64)
            ops.decode_attention(*args, **kw) if st.hist is None else ops.beam_decode_attention(*args, hist=st.hist, **kw)
        else:
            q, k, v, H, Hkv, hd, slots = gq
            w = Hkv * hd
            args = (q, k, v, st.kc[l], st.vc[l], slots * w, w, st.ao, pos_ptr, 0, slots, B, H, Hkv, hd)
            if st.clen > DECODE_MAX_KEYS:       # a long state (Llama family: slots = st.clen, no slot_pos): the keys split across workgroups
                ops.gq_decode_attention_long(*args, st.attn_ws) if st.hist is None else \
                    ops.beam_gq_decode_attention_long(*args, st.attn_ws, hist=st.hist)
                return
            ops.gq_decode_attention(*args) if st.hist is None else ops.beam_gq_decode_attention(*args, hist=st.hist, slot_pos=slot_pos)

    def _cross_attention(self, st, l: int, gq_hd: Optional[int] = None):
        """st.ao = st.q over layer l's cross-attention memory (every head its own K/V; gq_hd: head width, through the grouped-query
        kernel; None: 64, the dense model's).  Under beam search the st.mem_div rows of an image share its memory row."""
        B, d, H = st.B, self.eng.dec.d, self.eng.dec.H
        kv, S = st.cross_kv[l]
        if st.mem_index is not None:        # ``image_index``: row r over memory row st.mem_index[r], checked on the host
            if gq_hd is None:
                ops.mem_decode_attention(st.q, d, kv, kv.view(-1)[d:], S * 2 * d, 2 * d, st.ao, d, S, st.mem_index, st.mem_rows, B, H)
            else:
                ops.mem_gq_decode_attention(st.q, kv, kv.view(-1)[d:], S * 2 * d, 2 * d, st.ao, S, st.mem_index, st.mem_rows, B, H, H, gq_hd)
            return
        kw = {} if st.mem_div == 1 else dict(rows_per_mem=st.mem_div)
        if gq_hd is None:
            args = (st.q, d, kv, kv.view(-1)[d:], S * 2 * d, 2 * d, st.ao, d, None, S, B, H)
            ops.beam_decode_attention(*args, **kw) if kw else ops.decode_attention(*args)
        else:
            args = (st.q, None, None, kv, kv.view(-1)[d:], S * 2 * d, 2 * d, st.ao, None, S, S, B, H, H, gq_hd)
            ops.beam_gq_decode_attention(*args, **kw) if kw else ops.gq_decode_attention(*args)

    def _reusable(self, st, rows: int, total: int, extra=None) -> bool:
        """Whether the cached state ``st`` serves a call over ``rows`` rows and ``total`` id columns on the current arena and sparse
        tables; ``extra(st)``: what else the mode needs of it."""
        eng = self.eng
        return (st is not None and st.B == rows and st.arena is eng.arena and st.ids_ld >= total and st.sparse_epoch == eng.sparse_epoch
                and (extra is None or extra(st)))

    def _greedy_head(self, st, sampling: Optional[Sampling], logits: bool = False, lse: bool = False):
        """-> (top2, the first element of the full step's graph key).  top2: a greedy step whose head takes the segment-maxima form
        (nobody needs the ``logits``; d % 128 == 0: the persistent GEMM kernel's K rule; I2T_DECODE_TOP2=0: the logits form); its
        buffers are made at the first such call, with the segment sums beside them when the step takes the token's log-prob (``lse``)."""
        dc = self.eng.dec
        top2 = sampling is None and not logits and TOP2_HEAD and dc.d % 128 == 0
        if top2 and st.top2 is None:
            nseg = (dc.V + 63) // 64
            st.top2 = torch.zeros(st.B, nseg, 4, dtype=F32, device=st.arena.device)
            if lse:
                st.seg_se = torch.zeros(st.B, nseg, dtype=F32, device=st.arena.device)
        return top2, ('greedy_top2' if top2 else 'greedy') if sampling is None else sampling.key()

    @staticmethod
    def _drop_graphs(st, tag):
        """Forget the captured steps that hold a buffer about to be replaced: those whose key is a tuple that starts with ``tag`` (or with
        one of a tuple of tags) or -- tag 'top_logprobs' alone -- ends with ``caption_graph_key``'s ('top_logprobs', K), or -- tag None --
        ``generate``'s sampling steps, every key but None / 'greedy' / 'greedy_top2'."""
        tags = tag if isinstance(tag, tuple) else (tag,)
        ends = 'top_logprobs' in tags                       # the one tag that stands at a key's end, and only when it is asked for
        tagged = lambda k: isinstance(k, tuple) and k[:1] and (k[0] in tags or (ends and k[-2:-1] == ('top_logprobs',)))
        stale = (lambda k: k not in (None, 'greedy', 'greedy_top2')) if tag is None else tagged
        st.graphs = {k: g for k, g in st.graphs.items() if not stale(k)}

    def _upload_trie(self, st, trie, tag, fanout: bool = False):
        """The trie -- a ``PhraseTrie``, or a ``PhraseForest``, which the kernels walk as they walk a trie -- into st.trie =
        (child_off, child_tok, child_next, term): persistent because captured steps bake their pointers, and regrown -- together with
        the graphs tagged ``tag`` (a tag or a tuple of them: every kind of step that points at it) -- only when the trie does not fit.
        The kernels take the arrays' CAPACITIES as nodes / edges, so a captured step serves any trie that fits; the trie's contents
        are copied in per call, the spare nodes childless and ending no phrase.  ``fanout``: st.kept, f32 [B, widest fan-out + 1 in
        whole 4s], is kept and regrown with them."""
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        if st.trie is None or st.trie[3].numel() < trie.nodes or st.trie[1].numel() < trie.edges \
                or (fanout and st.kept.shape[1] < trie.max_fanout + 1):
            nodes, edges = max(64, trie.nodes), max(64, trie.edges)
            st.trie = (torch.zeros(nodes + 1, **i32), torch.zeros(edges, **i32), torch.zeros(edges, **i32), torch.full((nodes,), -1, **i32))
            if fanout:
                st.kept = torch.zeros(st.B, (max(64, trie.max_fanout + 1) + 3) // 4 * 4, dtype=F32, device=dev)
            self._drop_graphs(st, tag)
        nodes, edges = st.trie[3].numel(), st.trie[1].numel()
        off = np.full(nodes + 1, trie.edges, dtype=np.int32)
        off[:trie.nodes + 1] = trie.child_off
        tok, nxt, term = np.zeros(edges, dtype=np.int32), np.zeros(edges, dtype=np.int32), np.full(nodes, -1, dtype=np.int32)
        tok[:trie.edges], nxt[:trie.edges], term[:trie.nodes] = trie.child_tok, trie.child_next, trie.term
        for buf, host in zip(st.trie, (off, tok, nxt, term)):
            buf.copy_(torch.from_numpy(host))

    @staticmethod
    def _reset(st, prompt_rows, P: int, start=None):
        """What every mode's loop starts from: the prompt in the id buffer, the counters at ``start`` (default st.counters_init) and, in
        the states that have them, the identity history table and a cleared control word."""
        st.ids.zero_()
        st.ids[:, :P] = prompt_rows
        st.counters.copy_(st.counters_init if start is None else start)      # device-to-device: no host sync in the loop
        if st.hist is not None:
            st.hist.copy_(st.hist_init)
        if st.ctrl is not None:
            st.ctrl.zero_()

    def _replay(self, st, full_key, full_step, reset, n_prefill: int, n_full: int, use_graph: bool, each=None, poll_every: int = 0,
                prefill_first: bool = False) -> int:
        """The decode loop of every mode: ``reset()``, then ``n_prefill`` prefill steps (a prompt token into the cache, no head; graph
        key None) and up to ``n_full`` full steps (``full_step()`` issues their launches; graph key ``full_key``), each one hipGraph
        replay under ``use_graph``.  A step kind without a graph is captured first: both kinds run eagerly once (code objects must be
        loaded before capture; ``prefill_first``: in which order), the missing ones are captured, and ``reset()`` undoes it.
        ``each(i)`` runs after full step i.  ``poll_every`` > 0: every so many full steps the host reads st.ctrl[0:1] -- one 4-byte copy
        -- and stops once it is raised.  -> the full steps launched."""
        prefill = lambda: self._step(st, False)
        reset()
        if use_graph and (full_key not in st.graphs or None not in st.graphs):
            kinds = ((None, prefill), (full_key, full_step)) if prefill_first else ((full_key, full_step), (None, prefill))
            for _, fn in kinds:
                fn()
            for key, fn in kinds:
                if key not in st.graphs:
                    st.graphs[key] = _capture_launches(st.arena.device, fn)
            reset()
        for _ in range(n_prefill):                              # prompt tokens before the last: fill the cache only
            st.graphs[None].launch() if use_graph else prefill()
        replays = 0
        while replays < n_full:
            st.graphs[full_key].launch() if use_graph else full_step()
            replays += 1
            if each is not None:
                each(replays - 1)
            if poll_every and replays % poll_every == 0 and replays < n_full and int(st.ctrl[0:1].item()):
                break
        return replays

    def _set_mem_index(self, st, rows, per: int):
        """The row -> image table of a call (``CaptionPlan.row_images`` / ``caption_plan.row_images``: int32 [R] on the host, its values
        checked by ``check_image_index``; None: nothing to do) into st.mem_index, its one upload -> (the table as int64 on the device,
        for _prepare_inputs' gather; ``image_index`` int32 [Q] as the results carry it, every ``per``-th word of the table)"""
        if rows is None:
            return None, None
        assert rows.shape == (st.B,) and rows.min() >= 0 and rows.max() < st.mem_rows      # no out-of-range row ever reaches the device
        st.mem_index.copy_(torch.from_numpy(rows))
        return st.mem_index.long(), st.mem_index[::per].clone()

    def _prepare_inputs(self, st, images, B: int, W: int = 1, prefill=None, index=None):
        """Everything a step reads besides the ids: the encoder output of the B images, the per-layer cross K/V (B rows), the
        soft-prompt rows' K/V at the head of the cache (copied to the W rows b * W .. b * W + W - 1 of every image) and the packed
        expert weights.  ``prefill`` = (prompt [B, >= m], m >= 1) under prompt_prefill='pass': the first m prompt columns' K/V go into
        the cache too, from one pass that also covers the soft-prompt rows (_prefill_pass).  ``index`` (``image_index``, DESIGN.md 4ac:
        int64 [R] on the device, row -> image): the encoder, the cross K/V and the soft-prompt pass still run over the B images, once;
        the soft-prompt K/V then reach the R rows through a gather, row r taking image index[r]'s (W is not read)."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        # encoder + per-layer cross K/V (once per image)
        # (in slices of ENC_CHUNK images -- 4096: +1.4 % captions/s over 1024 -- every image is independent in the encoder, and its activations -- ~20 MB per
        # image in eval mode -- would otherwise set the memory footprint of a large caption batch)
        if B <= ENC_CHUNK:
            enc_out, _ = eng.encode(images, False)
        else:
            enc_out = None
            for i in range(0, B, ENC_CHUNK):
                part, _ = eng.encode(images[i:i + ENC_CHUNK], False)
                if enc_out is None:
                    enc_out = torch.empty(B, *part.shape[1:], dtype=part.dtype, device=part.device)
                enc_out[i:i + ENC_CHUNK].copy_(part)
                del part
        S = enc_out.shape[1]
        eng.prepare_lora_merged()                               # merged adapter weights follow the current parameters
        if st.cross_kv:
            assert S == next(iter(st.cross_kv.values()))[1]
            mem = eng._mem_bf16(enc_out)
            for l, (kv, _) in st.cross_kv.items():              # persistent buffers: captured graphs bake their pointers
                p = f'{eng.dp}transformer.h.{l}.cross_attn'
                ops.gemm(mem, self._w(l, 'xattn_c_attn', f'{p}.in_proj_weight', slice(dc.d, 3 * dc.d)), kv.view(B * S, 2 * dc.d), B * S,
                         2 * dc.d, dc.d, bias=a.P(f'{p}.in_proj_bias')[dc.d:])
        if prefill is not None:
            self._prefill_pass(st, enc_out, prefill[0], prefill[1], W)
        elif st.prefix:     # the prompt rows' keys and values (one causal pass over the encoder outputs) open every caption's cache
                            # (every one of its W rows)
            n_p = st.prefix
            if dc.llama is not None:          # row-major cache [B][slot][Hkv hd]; the saved keys already carry their rotation.  Each layer's
                ls = dc.llama                 # K / V go into the cache as the layer finishes (a 7-B model's 32 saves would not fit beside it)

                def take_kv(l, sv):
                    qkv = sv.qkv.view(B, n_p, -1)
                    kq, vq = qkv[..., ls.H * ls.hd:(ls.H + ls.Hkv) * ls.hd], qkv[..., (ls.H + ls.Hkv) * ls.hd:]
                    if index is not None:
                        st.kc[l][:, :n_p].copy_(kq.index_select(0, index))
                        st.vc[l][:, :n_p].copy_(vq.index_select(0, index))
                        return
                    st.kc[l].view(B, W, st.clen, -1)[:, :, :n_p].copy_(kq.unsqueeze(1))
                    st.vc[l].view(B, W, st.clen, -1)[:, :, :n_p].copy_(vq.unsqueeze(1))
                eng._layer_sink = take_kv
            try:
                _, _, pctx = eng.decode_segment(B, n_p, eng._mem_bf16(enc_out) if eng.cross_inputs else None, S, True,
                                                embeds=enc_out[:, :n_p].reshape(B * n_p, dc.d), pos_offset=0)
            finally:
                eng._layer_sink = None
            for l in range(dc.L if dc.llama is None else 0):
                qkv = pctx.saves[l].qkv.view(B, n_p, 3, dc.H, 64)
                if index is not None:
                    st.kc[l].view(-1, dc.H, st.clen, 64)[:, :, :n_p].copy_(qkv[:, :, 1].transpose(1, 2).index_select(0, index))
                    st.vc[l].view(-1, dc.H, st.clen, 64)[:, :, :n_p].copy_(qkv[:, :, 2].transpose(1, 2).index_select(0, index))
                    continue
                st.kc[l].view(B, W, dc.H, st.clen, 64)[:, :, :, :n_p].copy_(qkv[:, :, 1].transpose(1, 2).unsqueeze(1))
                st.vc[l].view(B, W, dc.H, st.clen, 64)[:, :, :, :n_p].copy_(qkv[:, :, 2].transpose(1, 2).unsqueeze(1))
            del pctx
        if dc.fam is not None and dc.fam.moe is not None:       # the packed expert output weights follow the current parameters
            for l in range(dc.L):
                for part in ('c_fc', 'c_proj'):
                    mv = eng._moe_views(f'{eng.dp}transformer.h.{l}.mlp.{part}', dc.fam.moe)
                    ops.moe_pack_w2(mv.l2w, mv.l2b, mv.W2aug, mv.out_f, dc.fam.moe.E, dc.fam.moe.P)

    def _prefill_pass(self, st, enc_out, prompt, m: int, W: int):
        """prompt_prefill='pass' (DESIGN.md 4q): prompt columns 0 .. m - 1 of the B images through the decoder's forward as ONE causal
        sequence per image -- behind the n_p = st.prefix encoder outputs when the decoder is prefixed, the same sequence
        decode_prefixed runs -- and every layer's K / V rows into cache slots 0 .. n_p + m - 1 of the W rows of each image, one
        i2t_kv_prefill launch per layer.  The images go through in slices of PREFILL_ROWS token rows.  A Llama-family layer hands its
        K / V over as it finishes (eng._layer_sink): its saves never coexist."""
        eng, dc = self.eng, self.eng.dec
        B, S, n_p = enc_out.shape[0], enc_out.shape[1], st.prefix
        T = n_p + m
        ids = prompt[:, :m].contiguous()
        if dc.llama is not None:            # row-major cache [R][clen][Hkv hd]; packed q | k | v rows, the keys already rotated
            ls = dc.llama
            hd, w = ls.hd, ls.Hkv * ls.hd
            k_off, v_off = ls.H * ls.hd, (ls.H + ls.Hkv) * ls.hd
            strides = (st.clen * w, w, hd)
        else:                               # head-major cache [R][H][clen][64]; packed q | k | v rows of width 3 d
            hd, w = 64, dc.d
            k_off, v_off = dc.d, 2 * dc.d
            strides = (st.clen * dc.d, 64, st.clen * 64)
        per = max(1, PREFILL_ROWS // T)
        for i in range(0, B, per):
            c = min(per, B - i)

            def put(l, sv):
                ops.kv_prefill(sv.qkv, sv.qkv.stride(0), k_off, v_off, T, 0, T, st.kc[l][i * W:], st.vc[l][i * W:], *strides, hd, w, 0, c, W)
            part = enc_out[i:i + c]
            mem = eng._mem_bf16(part) if eng.cross_inputs else None
            if dc.llama is not None:
                eng._layer_sink = put
            try:
                if n_p:
                    _, _, pctx = eng.decode_prefixed(c, m, part, mem, True, ids[i:i + c])
                else:
                    _, _, pctx = eng.decode_segment(c, m, mem, S, True, ids=ids[i:i + c], pos_offset=st.off)
            finally:
                eng._layer_sink = None
            for l in range(dc.L if dc.llama is None else 0):
                put(l, pctx.saves[l])
            del pctx

    # ------------------------------------------------------------------------------------------------ public
    @torch.no_grad()
    def generate(self, images, prompt_ids: torch.Tensor, max_new_tokens: int, return_margins: bool = False,
                 use_graph: bool = True, sampling: Optional[Sampling] = None, return_dists: bool = False):
        """-> ids (B, P + max_new_tokens) [, margins (B, N) greedy only] [, dists (B, N, V) sampling only: the filtered,
        renormalised distribution every token was drawn from]."""
        eng = self.eng
        if not eng.dec.causal:      # nothing to cache under bidirectional attention: the reference's re-evaluation loop
            assert not return_margins and not return_dists, 'margins / distributions are recorded on the KV-cache path only'
            return generate_by_recompute(self.model, images, prompt_ids, max_new_tokens, sampling)
        a = eng.prepare(False)
        dc = eng.dec
        B, P = prompt_ids.shape
        total = P + max_new_tokens
        window = decode_window(*self._cache_args())
        assert total <= window, f'prompt + new tokens ({total}) exceed the text window ({window})'
        st = self._state_for(B, total, lambda clen: self._build(B, max(total, dc.block), clen=clen))
        assert not (return_margins and sampling is not None) and not (return_dists and sampling is None)
        self._prepare_inputs(st, images, B)
        if sampling is not None:
            _draw_seed(st.seed, sampling.seed)
            if return_dists != (st.dist is not None):         # captured sampling steps bake the dist pointer (or its absence)
                st.dist = torch.zeros(B, dc.V, dtype=F32, device=a.device) if return_dists else None
                self._drop_graphs(st, None)
        top2, full_key = self._greedy_head(st, sampling, logits=return_margins)
        reset = lambda: self._reset(st, prompt_ids, P)
        margins = torch.zeros(max_new_tokens, B, dtype=F32, device=a.device) if return_margins else None
        dists = torch.zeros(max_new_tokens, B, dc.V, dtype=F32, device=a.device) if return_dists else None
        keep = (lambda i: margins[i].copy_(st.margin)) if return_margins else (lambda i: dists[i].copy_(st.dist)) if return_dists else None
        self._replay(st, full_key, lambda: self._step(st, True, sampling, top2), reset, P - 1, max_new_tokens, use_graph, each=keep)
        out = st.ids[:, :total].clone()
        if return_margins:
            return out, margins.t().contiguous()
        if return_dists:
            return out, dists.transpose(0, 1).contiguous()
        return out


class BeamDecoder(GreedyDecoder):
    """Beam search on the static KV cache: R = B * W rows (batch-major, r = b * W + w) through GreedyDecoder's buffers and layer
    sequence, under GreedyDecoder._replay (no poll).  The step's head is the fp32 lm_head, then on the device (csrc/beam.hip):
    i2t_beam_candidates (ban, crop, E candidates, EOS rule) -> i2t_beam_consolidate (W survivors per caption, ids and history rows
    moved to the children) -> i2t_beam_advance.  Survivors copy no K/V: the history table st.hist[r][t] names the cache row that
    holds key t of beam r, and the attention kernels read through it (a sparse layer's slot s through hist[r][st.kpos[l][s]], the
    text position the slot holds).  The encoder and the cross K/V run once per image
    (rows_per_mem = W); the prompt is prefilled for all R rows under the identity table.  Once every beam of every caption holds
    EOS the remaining replays do nothing, so the host launches them all and reads the final length once."""

    def _build_beam(self, B: int, spec: BeamSpec, ids_ld: int, record: bool, clen: Optional[int] = None, mem=None):
        """``mem`` = (images, True) under ``image_index``: B is then the queries"""
        W, E = spec.beam_width, spec.expansion
        R = B * W
        st = self._build(R, ids_ld, mem_rows=B if mem is None else mem[0], clen=clen, indexed=mem is not None and mem[1])
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        st.W, st.images = W, B
        st.mem_div = W
        st.hist = torch.zeros(R, st.clen, **i32)
        st.hist_init = torch.arange(R, **i32).unsqueeze(1).expand(R, st.clen).contiguous()
        st.cand_tok, st.cand_lp = torch.zeros(R, E, **i32), torch.zeros(R, E, dtype=F32, device=dev)
        st.scores = torch.zeros(R, dtype=F32, device=dev)
        st.has_eos, st.parent = torch.zeros(R, **i32), torch.zeros(R, **i32)
        st.ctrl = torch.zeros(2, **i32)                         # [done, unfinished captions]
        st.raw_tok = torch.zeros(R, E, **i32) if record else None
        st.raw_pick = torch.zeros(R, **i32) if record else None
        st.spec = spec
        st.beam_ngrams = torch.tensor(list(spec.ngram_sizes), **i32)
        return st

    @staticmethod
    def _build_pool(st, B: int, W: int, ids_ld: Optional[int] = None):
        """The finished pool of a mode that keeps one (CaptionBeamDecoder, PhraseBeamDecoder), W entries per image: the score they are
        sorted by, the raw sum, the length, the count, and the image's closed flag.  ``ids_ld``: also the entries' id and token
        log-prob rows (captions)."""
        dev = st.arena.device
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=F32, device=dev)
        st.pool_score, st.pool_sum = torch.zeros(B, W, **f32), torch.zeros(B, W, **f32)
        st.pool_len, st.pool_n, st.closed = torch.zeros(B, W, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
        if ids_ld is not None:
            st.pool_ids, st.pool_lp = torch.zeros(B, W, ids_ld, dtype=torch.long, device=dev), torch.zeros(B, W, ids_ld, **f32)

    @staticmethod
    def _reset_pool(st):
        """an empty pool and every image open (the mode's own pool rows -- ids, phrases -- are its reset's)"""
        st.pool_score.fill_(BEAM_DEAD)
        for buf in (st.pool_sum, st.pool_len, st.pool_n, st.closed):
            buf.zero_()

    def _beam_step(self, st):
        dc, sp = self.eng.dec, st.spec
        pos_ptr, len_ptr = st.counters[0:1], st.counters[1:2]
        self._logits_head(st)
        ops.beam_candidates(st.logits, st.ids, len_ptr, st.ctrl, st.beam_ngrams, st.B, dc.V, sp.expansion, sp.temperature, sp.top_k,
                            sp.eos, sp.log_boost, st.seed, st.cand_tok, st.cand_lp, st.raw_tok)
        ops.beam_consolidate(st.cand_tok, st.cand_lp, st.scores, st.ids, st.hist, st.has_eos, st.parent, pos_ptr, len_ptr, st.ctrl,
                             st.images, st.W, sp.expansion, sp.consolidation_temperature, sp.eos, st.seed, st.raw_pick)
        ops.beam_advance(st.counters, st.ctrl)

    @torch.no_grad()
    def search(self, images, prompt_ids: torch.Tensor, max_len: int, spec: BeamSpec, seed: Optional[int] = None, use_graph: bool = True,
               record: bool = False):
        """-> ids (B, W, L), cumulative log scores (B, W) [, draws: per step the raw candidate draws (B * W, E) before the EOS rule
        and the flat picks (B, W) of consolidation, when ``record``].  Steps run while the length is below ``max_len`` and some
        caption still has a beam without EOS (BeamSearchTokenGenerator's loop test); ``seed`` (64-bit) keys the draws."""
        eng = self.eng
        dc = eng.dec
        if not dc.causal:
            raise ValueError('BeamDecoder needs a causal decoder')
        W, E = spec.beam_width, spec.expansion
        if spec.temperature > 0 and spec.top_k is not None and 0 < spec.top_k < E:
            raise ValueError(f'top_k = {spec.top_k} leaves fewer than beam_expansion_factor = {E} tokens to draw without replacement')
        a = eng.prepare(False)
        prompt_ids = prompt_ids.to(a.device)
        B, P = prompt_ids.shape
        R = B * W
        total = max(P, max_len)
        n_steps = total - P
        window = decode_window(*self._cache_args())
        assert total <= window, f'prompt + new tokens ({total}) exceed the text window ({window})'
        st = self._state_for(R, total, lambda clen: self._build_beam(B, spec, max(total, dc.block), record, clen),
                             lambda st: st.W == W and st.spec.key() == spec.key() and (st.raw_tok is not None) == record)
        prompt_rows = prompt_ids.repeat_interleave(W, dim=0)
        if spec.eos is not None and bool((prompt_ids == spec.eos).any(dim=-1).all()):
            ids = prompt_rows.view(B, W, P).clone()          # every beam already holds EOS: nothing to do
            return (ids, torch.zeros(B, W, device=a.device)) + (([],) if record else ())
        self._prepare_inputs(st, images, B, W)
        _draw_seed(st.seed, seed)

        def reset():
            self._reset(st, prompt_rows, P)
            st.scores.zero_()
            if spec.eos is None:
                st.has_eos.zero_()
            else:
                st.has_eos.copy_((prompt_rows == spec.eos).any(dim=-1))
        draws = []
        self._replay(st, 'beam', lambda: self._beam_step(st), reset, P - 1, n_steps, use_graph, prefill_first=True,
                     each=(lambda i: draws.append((st.raw_tok.clone(), st.raw_pick.view(B, W).clone()))) if record else None)
        L = int(st.counters[1].item())                        # the one host sync of the search
        ids = st.ids[:, :L].reshape(B, W, L).clone()
        scores = st.scores.view(B, W).clone()
        return (ids, scores, draws[:L - P]) if record else (ids, scores)


class CaptionDecoder(GreedyDecoder):
    """``generate_captions`` on the static KV cache: R = B * N rows (batch-major, r = b * N + n) through GreedyDecoder's buffers and layer
    sequence, under GreedyDecoder._replay.  The encoder and the cross K/V run once per image (rows_per_mem = N); the
    self-attention cache is the identity one (no history table).  A step is _body -> _final_norm -> head and choice with the token's
    log-prob (i2t_gemm_bf16_top2_lse + i2t_top2_ngram_argmax_lp; or fp32 logits + i2t_ngram_ban_argmax_lp / i2t_sample_token_lp) ->
    i2t_caption_finish -> i2t_beam_advance.  Once every row has emitted EOS the device raises ctrl[0]; from then on no kernel of a
    replay writes ids, tok_lp, finished or lengths, and the driver, which polls that word every ``poll_every`` steps,
    stops launching.  The decoder keeps its own state and graphs: nothing here touches what ``generate`` uses.
    With ``prompt_lengths`` the rows' prompts differ in length: the same state and buffers, Pmin - 1 prefill replays,
    then full steps that end in i2t_caption_finish_ragged, which puts a row's next prompt token over the chooser's while the column
    is below the row's prompt length and counts max_new_tokens per row; those steps have graph keys of their own."""

    last_replays = 0                    # full-step replays the last call launched (tests, tools)
    last_prefill_steps = 0              # prefill replays the last call launched: Pmin - 1, or 0 under prompt_prefill='pass'

    def _build_captions(self, B: int, N: int, ids_ld: int, clen: Optional[int] = None, mem=None):
        """``mem`` = (images, True) under ``image_index``: B is then the queries"""
        R = B * N
        st = self._build(R, ids_ld, mem_rows=B if mem is None else mem[0], clen=clen, indexed=mem is not None and mem[1])
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        st.N, st.images = N, B
        st.mem_div = N
        st.ctrl = torch.zeros(2, **i32)                         # [done, unfinished rows]
        st.finished, st.lengths = torch.zeros(R, **i32), torch.zeros(R, **i32)
        st.tok_lp = torch.zeros(R, ids_ld, dtype=F32, device=dev)
        st.rag_prompt = st.rag_plen = None                      # prompt_lengths: int64 [B, ids_ld] / int32 [B], made at the first such call
        st.raw_lse = st.saved = st.suppress = None              # logits processors: f32 [R] / f32 [R, ids_ld] / int32 list, made at the first active call
        st.node = st.phrase_index = st.kept = st.trie = None    # phrases: int32 [R] / int32 [R] / f32 [R, fan-out + 1] / the four trie arrays (and raw_lse)
        st.node_init = None                                     # phrase_sets: int32 [R], every row's start node, made at the first such call
        st.top_tok = st.top_lp = st.entropy = None              # top_logprobs: int32 / f32 [R, ids_ld, K] and f32 [R, ids_ld], made at the first such call
        return st

    def _top_logprobs_state(self, st, K: int):
        """The result buffers of a ``top_logprobs`` step, persistent because captured steps bake their pointers: st.top_tok
        and st.top_lp (R * ids_ld * K * 4 bytes each) and st.entropy (R * ids_ld * 4 bytes), regrown -- together with the graphs tagged
        'top_logprobs' -- only when a call asks for a larger K than they were made for.  -> (top_tok, top_lp) as this call's [R, ids_ld,
        K]: the kernel takes K as the cells' width, so a smaller K is a view of the head of the same storage, and a step captured for
        it points at the same base.  reset() fills the views with the values of a cell no step writes."""
        if st.top_tok is None or st.top_tok.shape[2] < K:
            dev = st.arena.device
            st.top_tok = st.top_lp = None                       # the old buffers go before the new ones are made
            st.top_tok = torch.full((st.B, st.ids_ld, K), -1, dtype=torch.int32, device=dev)
            st.top_lp = torch.zeros(st.B, st.ids_ld, K, dtype=F32, device=dev)
            if st.entropy is None:
                st.entropy = torch.zeros(st.B, st.ids_ld, dtype=F32, device=dev)
            self._drop_graphs(st, 'top_logprobs')        # (the tag stands at the END of a key: caption_graph_key)
        n = st.B * st.ids_ld * K
        return st.top_tok.view(-1)[:n].view(st.B, st.ids_ld, K), st.top_lp.view(-1)[:n].view(st.B, st.ids_ld, K)

    def _processor_state(self, st, proc: Processors):
        """The buffers of an active-processor step, persistent because captured steps bake their pointers: st.raw_lse,
        st.saved (R * ids_ld * 4 bytes) and the suppress list's buffer, which is regrown only together with the graphs that hold it; the
        list's contents are copied in per call."""
        dev = st.arena.device
        if st.raw_lse is None:                                  # (a phrases call may have made it: _trie_state)
            st.raw_lse = torch.zeros(st.B, dtype=F32, device=dev)
        if st.saved is None:
            st.saved = torch.zeros(st.B, st.ids_ld, dtype=F32, device=dev)
        n = len(proc.suppress)
        if st.suppress is None or st.suppress.numel() < n:
            st.suppress = torch.zeros(max(64, n), dtype=torch.int32, device=dev)
            self._drop_graphs(st, 'proc')
        if n:
            st.suppress[:n].copy_(torch.tensor(proc.suppress, dtype=torch.int32))

    def _trie_state(self, st, trie, roots=None):
        """The buffers of a phrase-constrained step, persistent because captured steps bake their pointers: st.node,
        st.phrase_index, st.raw_lse, and the trie with st.kept beside it (_upload_trie), under the graph tags 'trie' and 'trie_sets' --
        both kinds of step point at the same buffers.  ``roots`` (a ``phrase_sets`` call, DESIGN.md 4x: int32 [B], the root of every
        image's set in the forest ``trie``): st.node_init, which reset() copies into st.node; no step reads it."""
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        if st.node is None:
            st.node, st.phrase_index = torch.zeros(st.B, **i32), torch.full((st.B,), -1, **i32)
        if st.raw_lse is None:                                  # (shared with the logits processors: _processor_state)
            st.raw_lse = torch.zeros(st.B, dtype=F32, device=dev)
        self._upload_trie(st, trie, ('trie', 'trie_sets'), fanout=True)
        if roots is not None:
            if st.node_init is None:
                st.node_init = torch.zeros(st.B, **i32)
            st.node_init.copy_(torch.from_numpy(np.repeat(np.asarray(roots, dtype=np.int32), st.N)))

    def _caption_step(self, st, sampling: Optional[Sampling], top2: bool, eos: Optional[int], pad: int, forced=None, proc=None,
                      trie: bool = False, top=None):
        """The launches of a full step.  ``forced``: None, or (prompt, plen, max_new) of a ``prompt_lengths`` call -- the finish rule is
        then i2t_caption_finish_ragged; the choosers run as they are, on every row, and what they wrote at a forced column is replaced
        after them.  ``proc``: None, or (Processors, P) of a call with active logits processors (never with ``top2``):
        i2t_caption_logits_process between the GEMM and the chooser, i2t_caption_raw_logprob between the chooser and the finish rule.
        ``trie`` (a ``phrases`` or ``phrase_sets`` call; never with ``top2`` or ``proc``): i2t_caption_trie_mask before
        the chooser, which then runs without n-gram sizes -- the phrase set says what may be emitted --, i2t_caption_trie_advance after it.
        Together with ``forced`` (``phrase_sets`` under ``prompt_lengths``) the pair is i2t_caption_trie_mask_ragged /
        i2t_caption_trie_advance_ragged, which hold a row's trie state still while its column is forced.  ``top``: None, or (top_tok,
        top_lp, K) of a ``top_logprobs`` call (never with ``top2``): i2t_caption_top_logprobs right behind the GEMM, where
        the row is still raw -- before the processors and the trie mask, which write it."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        R, d = st.B, dc.d
        len_ptr, done = st.counters[1:2], st.ctrl[0:1]
        nn = 0 if trie else st.ngrams.numel()
        if top2:
            self._body(st)
            self._final_norm(st)
            ops.gemm_top2_lse(st.hid, a.W(eng.n_head), st.top2, st.seg_se, R, dc.V, d)
            ops.top2_ngram_argmax_lp(st.top2, st.seg_se, st.hid, a.W(eng.n_head), st.ids, st.ids_ld, len_ptr, st.ngrams, nn, R, dc.V, d, done,
                                     st.tok_lp)
        else:
            self._logits_head(st)
            if top is not None:
                ops.caption_top_logprobs(st.logits, dc.Vp, len_ptr, None if forced is None else forced[1], st.N, st.finished, done, top[0], top[1],
                                         st.entropy, top[2], R, dc.V)
            if proc is not None:
                pr, P = proc
                ops.caption_logits_process(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, None if forced is None else forced[1], P, st.N,
                                           st.suppress, len(pr.suppress), eos, pr.min_new, pr.theta, pr.inv_theta, done, st.raw_lse, st.saved,
                                           R, dc.V)
            if trie:
                off, tok, nxt, term = st.trie
                if forced is None:
                    ops.caption_trie_mask(st.logits, dc.Vp, st.node, off, tok, term, eos, done, st.raw_lse, st.kept, R, dc.V)
                else:
                    ops.caption_trie_mask_ragged(st.logits, dc.Vp, st.node, off, tok, term, eos, done, st.raw_lse, st.kept, len_ptr, forced[1],
                                                 st.N, R, dc.V)
            if sampling is None:
                ops.ngram_ban_argmax_lp(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, nn, R, dc.V, done, st.tok_lp)
            else:
                ops.sample_token_lp(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, nn, R, dc.V, sampling.temperature,
                                    sampling.top_k, sampling.nucleus_p, st.seed, done, st.tok_lp)
            if proc is not None:                                # the chooser's log-prob was taken on the processed row: the raw one over it
                ops.caption_raw_logprob(st.ids, st.ids_ld, len_ptr, st.raw_lse, st.saved, st.logits, dc.Vp, done, st.tok_lp, R, dc.V)
            if trie and forced is None:                         # the row moves along the chosen edge; the raw log-prob over the chooser's
                ops.caption_trie_advance(st.ids, st.ids_ld, len_ptr, st.finished, st.logits, dc.Vp, st.raw_lse, off, tok, nxt, term, eos, done,
                                         st.node, st.phrase_index, st.tok_lp, R, dc.V)
            elif trie:
                ops.caption_trie_advance_ragged(st.ids, st.ids_ld, len_ptr, st.finished, st.logits, dc.Vp, st.raw_lse, off, tok, nxt, term, eos,
                                                done, st.node, st.phrase_index, st.tok_lp, forced[1], st.N, R, dc.V)
        if forced is None:
            ops.caption_finish(st.ids, st.ids_ld, len_ptr, eos, pad, st.finished, st.lengths, st.tok_lp, st.ctrl, R)
        else:
            prompt, plen, max_new = forced
            ops.caption_finish_ragged(st.ids, st.ids_ld, len_ptr, prompt, plen, st.N, max_new, eos, pad, st.finished, st.lengths, st.tok_lp,
                                      st.ctrl, R)
        ops.beam_advance(st.counters, st.ctrl)

    @torch.no_grad()
    def generate_captions(self, images, prompt_ids: torch.Tensor, max_new_tokens: int, eos: Optional[int] = None, pad: Optional[int] = None,
                          num_return_sequences: int = 1, sampling: Optional[Sampling] = None, poll_every: int = 8,
                          use_graph: bool = True, prompt_lengths=None, prompt_prefill: str = 'steps', repetition_penalty: float = 1.0,
                          min_new_tokens: int = 0, suppress_tokens=None, phrases=None, each=None, phrase_sets=None,
                          phrase_set_index=None, top_logprobs: int = 0, image_index=None) -> GeneratedCaptions:
        """Row (b, n) is prompt_ids[b] and up to max_new_tokens emitted tokens.  With ``prompt_lengths`` it is prompt_ids[b, :p_b]: all
        rows share the step's column counter, and a row whose prompt reaches past the column is forced on the device;
        None is the case Pmin = Pmax = P, which needs no forcing table.  ``prompt_prefill`` (``prefill_plan``): 'steps'
        feeds prompt columns 0 .. Pmin - 2 one prefill replay each; 'pass' takes them through one forward pass per IMAGE
        (_prefill_pass) and starts the counters behind them -- the full steps, their graphs and everything after are the same.
        ``repetition_penalty`` / ``min_new_tokens`` / ``suppress_tokens`` (``caption_processors``): with any of them active
        the step takes the fp32-logits head whatever the decoder's width -- the segment-maxima head cannot see a penalised token's
        neighbours, so a d % 128 == 0 decoder gives up that head's saving -- with i2t_caption_logits_process before the
        chooser and i2t_caption_raw_logprob after it, under graph keys of their own; inactive, the call is the one without them.
        ``phrases`` (a sequence of token-id sequences, or the ``PhraseTrie`` the model built of one; ``check_phrase_caption_args``,
        DESIGN.md 4u): every row emits
        one of the phrases, then EOS.  The step takes the fp32-logits head with i2t_caption_trie_mask before the chooser -- which runs
        over the allowed tokens only, without the n-gram ban -- and i2t_caption_trie_advance after it, under graph keys of their own;
        the result carries ``phrase_index``.  None: the call is the one without the argument.  ``phrase_sets`` / ``phrase_set_index``
        (``check_phrase_set_caption_args``): a phrase set per image -- the sets as one forest in the trie's buffers, every
        row starting at its set's root --, with or without ``prompt_lengths``; graph keys ('trie_sets', ...).  ``top_logprobs`` = K
        (``check_top_logprobs``): the K best tokens of every step's RAW row with their log-probs, and the row's entropy --
        i2t_caption_top_logprobs between the GEMM and whatever writes the row, on the fp32-logits head whatever the decoder's width, under
        graph keys (..., 'top_logprobs', K); the result carries ``top_tokens`` / ``top_logprobs`` / ``token_entropy``.  0: the call without
        the argument.  ``each(i)`` runs after full step i (tests read the step's buffers there)."""
        plan = plan_captions(caption_facts(self.model), *prompt_ids.shape, max_new_tokens, eos, pad, num_return_sequences,
                             poll_every=poll_every, prompt_lengths=prompt_lengths, prompt_prefill=prompt_prefill,
                             repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens,
                             phrases=phrases, phrase_sets=phrase_sets, phrase_set_index=phrase_set_index, sampling=sampling,
                             image_index=image_index, images=len(images), top_logprobs=top_logprobs)
        return self.run(images, prompt_ids, plan, use_graph, each)

    @torch.no_grad()
    def run(self, images, prompt_ids: torch.Tensor, plan: CaptionPlan, use_graph: bool = True, each=None) -> GeneratedCaptions:
        """A 'cache' plan (``plan_captions``) on ``prompt_ids`` [B, P]: nothing is checked or derived again here.  Under
        ``plan.image_index`` B is Q, the queries -- rows are (query, n), and everything below is per query -- except in
        what runs once per IMAGE: the encoder, the cross K/V and the soft-prompt pass (_prepare_inputs over ``mem[0]`` images)."""
        if plan.mode != 'cache':
            raise ValueError('CaptionDecoder needs a causal decoder')
        eng = self.eng
        dc = eng.dec
        B = prompt_ids.shape[0]
        mem = (B, False) if plan.image_index is None else (len(images), True)
        N, sampling, eos, pad, poll_every, max_new_tokens = plan.N, plan.sampling, plan.eos, plan.pad, plan.poll_every, plan.max_new
        plen, pmin, pmax, proc, trie, m, start = plan.plen, plan.pmin, plan.pmax, plan.proc, plan.trie, plan.m, plan.start
        sets, K = plan.sets, plan.top_logprobs
        if sets is not None:                # the forest stands where the trie stands: the step's launches differ only under prompt_lengths
            trie = sets.forest
        ragged = plen is not None
        n_prefill = pmin - 1 - m
        if not max_new_tokens:              # nothing to emit: no step reads the cache, so 'pass' fills nothing -- no pass, no replay
            m = 0
        a = eng.prepare(False)
        R, total = B * N, pmax + max_new_tokens
        st = self._state_for(R, total, lambda clen: self._build_captions(B, N, max(total, dc.block), clen, mem), lambda st: st.N == N, mem)
        row_index, index_dev = self._set_mem_index(st, plan.row_images, N)
        prompt = prompt_ids[:, :pmax].to(a.device)
        plen_dev = forced = None
        if ragged:
            if st.rag_prompt is None:                           # persistent: the captured steps bake their pointers
                st.rag_prompt = torch.zeros(B, st.ids_ld, dtype=torch.long, device=a.device)
                st.rag_plen = torch.ones(B, dtype=torch.int32, device=a.device)
            plen_dev = torch.from_numpy(plen).to(a.device)
            # columns at or past p_b are dropped here: nothing downstream sees what the caller left in them
            keep = torch.arange(pmax, device=a.device)[None, :] < plen_dev[:, None]
            prompt = torch.where(keep, prompt, torch.zeros((), dtype=torch.long, device=a.device))
            st.rag_prompt.zero_()
            st.rag_prompt[:, :pmax] = prompt
            st.rag_plen.copy_(plen_dev)
            len_rows = (plen_dev.repeat_interleave(N) if N > 1 else plen_dev) + max_new_tokens
            if max_new_tokens == 0:                           # nothing to emit: the prompts, padded
                ids = torch.where(keep, prompt, torch.full((), pad, dtype=torch.long, device=a.device)).repeat_interleave(N, dim=0)
                self.last_replays = self.last_prefill_steps = 0
                zero = torch.zeros(B, N, pmax - pmin, dtype=F32, device=a.device)
                none = {} if not K else dict(top_tokens=torch.full((B, N, pmax - pmin, K), -1, dtype=torch.int32, device=a.device),
                                             top_logprobs=torch.zeros(B, N, pmax - pmin, K, dtype=F32, device=a.device), token_entropy=zero.clone())
                return GeneratedCaptions(ids.view(B, N, pmax), len_rows.view(B, N).clone(), zero, zero.sum(dim=-1), plen_dev, image_index=index_dev,
                                         **none)
            forced = (st.rag_prompt, st.rag_plen, max_new_tokens)
        self._prepare_inputs(st, images, mem[0], N, prefill=(prompt, m) if m else None, index=row_index)
        # 'pass': the first step is at slot prefix + m, column 1 + m; st.counters_init stays what 'steps' calls on this state start from
        start = torch.tensor(start, dtype=torch.int32, device=a.device) if m else st.counters_init
        if sampling is not None:
            _draw_seed(st.seed, sampling.seed)
        if proc is not None:
            self._processor_state(st, proc)
        if trie is not None:
            self._trie_state(st, trie, None if sets is None else sets.roots)
        top = None if not K else self._top_logprobs_state(st, K) + (K,)
        top2, head = self._greedy_head(st, sampling, logits=proc is not None or trie is not None or top is not None, lse=True)
        # eos, pad and max_new_tokens are kernel arguments: a captured step holds them ('ragged': never an equal-length step's key), and
        # so are the processors' scalars ('proc': never an inactive call's key); 'trie': never a key of a call without phrases
        # 'trie_sets': never a key of a call without phrase_sets; 'top_logprobs': never a key of a call without K
        full_key = caption_graph_key(head, eos, pad, max_new_tokens if ragged else None, proc, pmax, trie is not None, sets is not None, K)
        prompt_rows = prompt.repeat_interleave(N, dim=0) if N > 1 else prompt

        def reset():
            self._reset(st, prompt_rows, pmax, start)
            st.finished.zero_()
            # what a row without an EOS ends with: p_b + max_new_tokens
            st.lengths.copy_(len_rows) if ragged else st.lengths.fill_(total)
            st.tok_lp.zero_()
            if trie is not None:                                # every row at the root (of its set), no phrase named yet
                st.node.zero_() if sets is None else st.node.copy_(st.node_init)
                st.phrase_index.fill_(-1)
            if top is not None:                                 # what a cell no step writes holds
                top[0].fill_(-1)
                top[1].zero_()
                st.entropy.zero_()
        # Pmin - 1 columns every row holds a prompt token in, then the longest prompt's row emits its last token in the last full step
        # ('pass': those columns' K/V are in the cache already, n_prefill = 0)
        self.last_prefill_steps = n_prefill
        self.last_replays = self._replay(st, full_key, lambda: self._caption_step(st, sampling, top2, eos, pad, forced, None if proc is None else (proc, pmax),
                                                                                  trie is not None, top),
                                         reset, n_prefill,
                                         pmax - pmin + max_new_tokens, use_graph, each=each, poll_every=poll_every if eos is not None else 0)
        lengths = st.lengths.clone()
        L = int(lengths.max().item()) if max_new_tokens else pmax       # the final host sync
        ids = st.ids[:, :L].reshape(B, N, L).clone()
        tok_lp = st.tok_lp[:, pmin:L].reshape(B, N, L - pmin).clone()
        cut = lambda t: t[:, pmin:L].reshape((B, N, L - pmin) + tuple(t.shape[2:])).clone()
        return GeneratedCaptions(ids, lengths.view(B, N), tok_lp, tok_lp.sum(dim=-1), plen_dev,
                                 phrase_index=None if trie is None else st.phrase_index.view(B, N).clone(), image_index=index_dev,
                                 top_tokens=None if top is None else cut(top[0]), top_logprobs=None if top is None else cut(top[1]),
                                 token_entropy=None if top is None else cut(st.entropy))


class CaptionBeamDecoder(BeamDecoder):
    """``generate_captions(num_beams=W)`` on the static KV cache: BeamDecoder's R = B * W rows, history table and
    attention kernels, under GreedyDecoder._replay with ``poll_every``.  A step is _body -> _final_norm -> fp32 lm_head ->
    i2t_beam_candidates (temperature 0, E = 2 W, no EOS rule, no crop) -> i2t_beam_pool_select -> i2t_beam_advance; the finished pool and
    the per-image closed flags live in device memory, and the result is the first N pool rows of every image.  The decoder keeps its own
    state; its graph key is ('caption_beam', ...), never 'beam'."""

    last_replays = 0                    # full-step replays the last call launched (tests, tools)

    def _build_caption_beam(self, B: int, W: int, ids_ld: int, clen: Optional[int] = None, mem=None):
        spec = BeamSpec(W, 2 * W, 0.0, None, 0.0, None, 0.0, tuple(int(n) for n in self.model.config.no_repeat_n_grams))
        st = self._build_beam(B, spec, ids_ld, False, clen, mem)
        dev = st.arena.device
        st.tok_lp = torch.zeros(B * W, ids_ld, dtype=F32, device=dev)
        self._build_pool(st, B, W, ids_ld)
        st.scores_init = torch.full((B, W), BEAM_DEAD, dtype=F32, device=dev)
        st.scores_init[:, 0] = 0.0
        return st

    def _caption_beam_step(self, st, P: int, max_new: int, eos, pad: int, length_penalty: float, early_stopping: bool):
        dc, sp = self.eng.dec, st.spec
        pos_ptr, len_ptr = st.counters[0:1], st.counters[1:2]
        self._logits_head(st)
        ops.beam_candidates(st.logits, st.ids, len_ptr, st.ctrl, st.beam_ngrams, st.B, dc.V, sp.expansion, 0.0, None, None, 0.0, st.seed,
                            st.cand_tok, st.cand_lp, None)
        ops.beam_pool_select(st.cand_tok, st.cand_lp, st.scores, st.ids, st.hist, st.tok_lp, st.pool_ids, st.pool_lp, st.pool_score,
                             st.pool_sum, st.pool_len, st.pool_n, st.closed, pos_ptr, len_ptr, st.ctrl, st.images, st.W, P, max_new, eos, pad,
                             length_penalty, early_stopping)
        ops.beam_advance(st.counters, st.ctrl)

    @torch.no_grad()
    def generate_captions(self, images, prompt_ids: torch.Tensor, max_new_tokens: int, num_beams: int, eos: Optional[int] = None,
                          pad: Optional[int] = None, num_return_sequences: int = 1, length_penalty: float = 1.0,
                          early_stopping: bool = False, poll_every: int = 8, use_graph: bool = True, each=None,
                          image_index=None) -> GeneratedCaptions:
        """``beam_search_host`` for every image of the batch, on the device -> GeneratedCaptions with ``beam_scores``.  ``each(i)`` runs
        after full step i (tests read the step's buffers there)."""
        plan = plan_captions(caption_facts(self.model), *prompt_ids.shape, max_new_tokens, eos, pad, num_return_sequences,
                             poll_every=poll_every, num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping,
                             image_index=image_index, images=len(images))
        return self.run(images, prompt_ids, plan, use_graph, each)

    @torch.no_grad()
    def run(self, images, prompt_ids: torch.Tensor, plan: CaptionPlan, use_graph: bool = True, each=None) -> GeneratedCaptions:
        """A 'beam' plan (``plan_captions``) on ``prompt_ids`` [B, P]: nothing is checked or derived again here.  Under
        ``plan.image_index`` B is Q, the queries: rows are (query, w), the pools are the queries'."""
        assert plan.mode == 'beam', plan.mode
        eng = self.eng
        dc = eng.dec
        N, W, eos, pad, poll_every, max_new_tokens = plan.N, plan.W, plan.eos, plan.pad, plan.poll_every, plan.max_new
        length_penalty, early_stopping = plan.length_penalty, plan.early_stopping
        a = eng.prepare(False)
        prompt_ids = prompt_ids.to(a.device)
        B, P = prompt_ids.shape
        R, total = B * W, P + max_new_tokens
        mem = (B, False) if plan.image_index is None else (len(images), True)
        if max_new_tokens == 0:             # nothing to emit: the prompts, N times, at score 0
            self.last_replays = 0
            zero = torch.zeros(B, N, 0, dtype=F32, device=a.device)
            return GeneratedCaptions(prompt_ids[:, None].expand(B, N, P).clone(), torch.full((B, N), P, dtype=torch.int32, device=a.device),
                                     zero, zero.sum(dim=-1), None, torch.zeros(B, N, dtype=F32, device=a.device),
                                     image_index=None if plan.image_index is None else torch.from_numpy(plan.image_index).to(a.device))
        st = self._state_for(R, total, lambda clen: self._build_caption_beam(B, W, max(total, dc.block), clen, mem),
                             lambda st: st.W == W, mem)
        row_index, index_dev = self._set_mem_index(st, plan.row_images, W)
        self._prepare_inputs(st, images, mem[0], W, index=row_index)
        prompt_rows = prompt_ids.repeat_interleave(W, dim=0)

        def reset():
            self._reset(st, prompt_rows, P)
            st.scores.copy_(st.scores_init.view(-1))
            st.tok_lp.zero_()
            st.pool_ids.fill_(pad)
            st.pool_lp.zero_()
            self._reset_pool(st)
        # P, max_new_tokens, eos, pad and the two beam arguments are kernel arguments: a captured step holds them
        key = ('caption_beam', P, max_new_tokens, -1 if eos is None else int(eos), pad, length_penalty, early_stopping)
        self.last_replays = self._replay(st, key, lambda: self._caption_beam_step(st, P, max_new_tokens, eos, pad, length_penalty,
                                                                                  early_stopping),
                                         reset, P - 1, max_new_tokens, use_graph, each=each, poll_every=poll_every, prefill_first=True)
        lengths = st.pool_len[:, :N].contiguous()
        L = int(lengths.max().item())                           # the final host sync
        tok_lp = st.pool_lp[:, :N, P:L].contiguous()
        return GeneratedCaptions(st.pool_ids[:, :N, :L].contiguous(), lengths, tok_lp, tok_lp.sum(dim=-1), None,
                                 st.pool_score[:, :N].contiguous(), image_index=index_dev)


TRIE_SCORE_BYTES = int(os.environ.get('I2T_TRIE_SCORE_BYTES', str(8 << 30)))      # the per-pass state budget images_per_pass is derived from


class TrieScoreDecoder(BeamDecoder):
    """``score_phrases`` on the static KV cache: the phrase trie walked level by level, every node of a level a row,
    nothing pruned -- BeamDecoder's R = images * W rows (W = the widest level), history table, shared cross K/V (rows_per_mem = W) and
    attention kernels, but none of its candidates / consolidate / pool kernels, so their W <= 8 does not apply: the state is
    GreedyDecoder._build's plus the few buffers below.  The prompt goes through P - 1 ordinary prefill steps on all rows under the
    identity table.  Level t = 0 .. longest is then: the level's history columns into st.hist -> _body -> _final_norm -> the rows' LSE
    (d % 128 == 0: i2t_gemm_bf16_lse + i2t_lse_token_logprob with every label ignored, no logits; else the fp32 lm_head + i2t_rows_lse)
    -> i2t_trie_level_expand -> i2t_advance.  Rows beyond a level's width keep token 0 and the identity history; they run and their
    results are never read.  Eager launches: a level is one step and its tables differ from the last one's."""

    last_passes = 0                     # the image groups the last call ran (tests, tools)
    _score_state = None                 # this decoder's own state: neither GreedyDecoder._state nor ._long_state

    def row_bytes(self, clen: int, ids_ld: int) -> int:
        """what one row of the state costs, for the images_per_pass default: its K/V cache over every layer, its fp32 logits row (the
        shared allocation makes it whatever the head), the two history tables, ids, segment statistics and the step's activations"""
        dc = self.eng.dec
        if dc.llama is not None:
            kvw = dc.llama.Hkv * dc.llama.hd
        elif dc.fam is not None:
            kvw = (1 if dc.fam.mqa else dc.H) * dc.fam.hd
        else:
            kvw = dc.d
        return 2 * dc.L * clen * kvw * 2 + dc.Vp * 4 + 2 * clen * 4 + ids_ld * 8 + (dc.V + 63) // 64 * 8 + (16 * dc.d + 3 * dc.ff) * 4

    def _build_score(self, B: int, W: int, ids_ld: int, clen: int):
        R = B * W
        st = self._build(R, ids_ld, mem_rows=B, clen=clen)
        dev, dc = st.arena.device, self.eng.dec
        st.W, st.images, st.mem_div = W, B, W
        st.hist_init = torch.arange(R, dtype=torch.int32, device=dev).unsqueeze(1).expand(R, st.clen).contiguous()
        st.hist = st.hist_init.clone()
        st.row_base = (torch.arange(B, dtype=torch.int32, device=dev) * W).view(B, 1, 1)
        st.path = (torch.zeros(R, dtype=F32, device=dev), torch.zeros(R, dtype=F32, device=dev))      # swapped every level
        st.lse = torch.zeros(R, dtype=F32, device=dev)
        st.lse_route = dc.d % 128 == 0                           # the persistent GEMM kernel's K rule, as HotPath.token_logprobs
        if st.lse_route:
            st.stats = torch.zeros(R, (dc.V + 63) // 64, 2, dtype=F32, device=dev)
            st.no_label = torch.full((R,), -100, dtype=torch.long, device=dev)
            st.no_lp = torch.zeros(R, dtype=F32, device=dev)
        return st

    def _encode_all(self, st, images, B: int):
        """The encoder, the cross K/V and the soft-prompt rows' K/V of ALL B images, once, through _prepare_inputs on a one-row-per-image
        stand-in for the state: what a group of images starts from does not depend on how the images are grouped (the forward's GEMMs
        choose their kernels by the number of rows)."""
        dev = st.arena.device
        e = lambda *s: torch.zeros(*s, dtype=BF16, device=dev)
        pre = SimpleNamespace(prefix=st.prefix, clen=max(st.prefix, 1), cross_kv={l: (e(B, *kv.shape[1:]), S) for l, (kv, S) in st.cross_kv.items()})
        if st.prefix:
            pre.kc = [e(B, st.prefix, k.shape[-1]) for k in st.kc]
            pre.vc = [e(B, st.prefix, v.shape[-1]) for v in st.vc]
        self._prepare_inputs(pre, images, B, 1)
        return pre

    def _load_group(self, st, pre, take):
        """the cross K/V of images ``take`` [st.images] and their soft-prompt K/V into the head of every row's cache.  Under
        ``image_index`` ``take`` names the images of the group's QUERIES: an image asked twice in a pass has its K/V
        there twice -- the pass keeps rows_per_mem = W and its kernels"""
        dc = self.eng.dec
        Bp, W, n_p = st.images, st.W, st.prefix
        for l, (kv, _) in st.cross_kv.items():
            kv.copy_(pre.cross_kv[l][0][take])
        for l in range(dc.L if n_p else 0):
            for dst, src in ((st.kc[l], pre.kc[l]), (st.vc[l], pre.vc[l])):
                if dc.llama is not None:                        # row-major [R][slot][Hkv hd]
                    dst.view(Bp, W, st.clen, -1)[:, :, :n_p].copy_(src[take].unsqueeze(1))
                else:                                           # head-major [R][H][slot][64]
                    dst.view(Bp, W, dc.H, st.clen, 64)[:, :, :, :n_p].copy_(src.view(-1, dc.H, n_p, 64)[take].unsqueeze(1))

    def _level_lse(self, st):
        """the level's step on all rows and the rows' LSE into st.lse -> the z operands of the expand kernel"""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        R, V, d = st.B, dc.V, dc.d
        head = a.W(eng.n_head)
        if st.lse_route:
            self._body(st)
            self._final_norm(st)
            ops.gemm_lse(st.hid, head, st.stats, R, V, d)
            ops.lse_token_logprob(st.stats, st.hid, head, st.no_label, st.lse, st.no_lp, R, V, d, ignore_index=-100)
            return dict(hidden=st.hid, w_head=head, d=d)
        self._logits_head(st)
        ops.rows_lse(st.logits, dc.Vp, st.lse, R, V)
        return dict(logits=st.logits, ld=dc.Vp)

    def _score_state_for(self, B: int, W: int, total: int, images_per_pass: Optional[int]):
        """-> (the decoder's own state for groups of Bp images of W rows and ``total`` id columns, Bp).  The walk reads ``total`` cache
        slots however long the text window is, and W rows per image multiply every slot: a cache of that many slots (in whole 16s) --
        or, past text_window on a decoder that takes the long cache, cache_plan's whole chunks."""
        block, off, prefix, llama = self._cache_args()
        clen, long = cache_plan(block, off, prefix, total, llama)
        clen = clen if long else min(clen, prefix + -(-total // 16) * 16)
        ids_ld = -(-total // 8) * 8
        if images_per_pass is None:
            images_per_pass = max(1, TRIE_SCORE_BYTES // (W * self.row_bytes(clen, ids_ld)))
        Bp = min(int(images_per_pass), B)
        st = self._score_state
        if not self._reusable(st, Bp * W, total, lambda st: st.W == W and st.images == Bp and st.clen >= clen):
            self._score_state = st = None                       # the old buffers go before the new ones are made
            self._score_state = st = self._build_score(Bp, W, ids_ld, clen)
        assert total <= st.tmax
        return st, Bp

    def _level_walk(self, st, trie: PhraseTrie, levels, P: int, eos: int):
        """-> walk(i, part) of a call on one set for all images: levels t = 0 .. longest on every image of the group at once, the
        columns in which level t's history table is not the identity written on the device"""
        dev, dc, Bp, W = st.arena.device, self.eng.dec, st.images, st.W
        # every level's tables, checked on the host and uploaded once per call
        tables = [ops.trie_level_tables(*level_expand_tables(trie, levels, t), W, dc.V, int(trie.phrase_node.shape[0]), dev)
                  for t in range(trie.longest + 1)]
        anc = [torch.from_numpy(lv.anc).to(dev) for lv in levels.levels]
        first = st.prefix + P - 1                               # the cache slot of the level-0 step (TrieLevels.history)

        def walk(i, part):
            for t in range(trie.longest + 1):
                if t >= 2:
                    st.hist.view(Bp, W, st.clen)[:, :, first + 1:first + t] = st.row_base + anc[t][None, :, 1:t]
                z = self._level_lse(st)
                ops.trie_level_expand(tables[t], st.lse, st.path[t & 1], st.path[(t + 1) & 1], st.ids, st.ids_ld, st.counters[1:2], part, eos,
                                      Bp, W, dc.V, **z)
                ops.advance(st.counters, 1)
        return walk

    def _sets_walk(self, st, one: ClosedSet, tabs, plen, prompt_host, eos: int):
        """-> walk(i, part) of a call with a set and a prompt length per image: one step per id column from the shortest
        prompt up to the group's largest p_b + longest phrase; in each the host says where every image stands (``set_step_state``) and
        uploads that and the images' history tables -- ``TrieLevels.history`` of the image's own level and prompt length, the identity
        for a forced or finished image"""
        dev, dc, Bp, W = st.arena.device, self.eng.dec, st.images, st.W
        tables = ops.trie_set_tables(tabs, W, dc.V, dev)        # checked on the host and uploaded once per call
        identity = np.arange(Bp * W, dtype=np.int32).reshape(Bp, W, 1).repeat(st.clen, axis=2)
        histories = {}

        def history(s, t, first):
            if (s, t, first) not in histories:
                histories[s, t, first] = tabs.levels[s].history(t, first, st.clen)
            return histories[s, t, first]

        def walk(i, part):
            take = np.minimum(np.arange(i, i + Bp), len(plen) - 1)              # the group's images, as the caller fills a short last one
            g_index, g_plen, g_prompt = one.index[take], plen[take], prompt_host[take]
            for k, col in enumerate(range(int(plen.min()), int((g_plen + one.longest[take]).max()) + 1)):
                state = set_step_state(tabs, g_index, g_plen, g_prompt, col)
                hist = identity.copy()
                for b in np.flatnonzero(state[:, 0] >= 2).tolist():              # below level 2 a table is the identity
                    h = history(int(g_index[b]), int(state[b, 0]), st.prefix + int(g_plen[b]) - 1)
                    hist[b, :h.shape[0]] = b * W + h
                st.hist.copy_(torch.from_numpy(hist).view(Bp * W, st.clen))
                z = self._level_lse(st)
                ops.trie_level_expand_sets(tables, ops.trie_set_state(tables, state, W, dc.V, st.ids_ld, dev), st.lse, st.path[k & 1],
                                           st.path[(k + 1) & 1], st.ids, st.ids_ld, part, eos, W, dc.V, **z)
                ops.advance(st.counters, 1)
        return walk

    @torch.no_grad()
    def run(self, images, prompt_ids: torch.Tensor, one: ClosedSet, eos: int, images_per_pass: Optional[int] = None):
        """``phrase_scores_host`` -- ``one.per_image``: ``phrase_set_scores_host`` -- for every image of the batch, on the
        device -> ``PhraseScores`` / ``PhraseSetScores``.  ``one``: what ``plan_phrase_scores`` returned; under ``one.image_index``
         B below is Q, the queries, the groups are groups of queries, and only _encode_all runs over the images.  The encoder once, then groups
        of ``images_per_pass`` images; all rows share the step counter: min p_b - 1 prefill steps, then the form's walk.  What the two
        forms do not share is the walk, what a column no phrase writes holds (0 / -inf) and the prompt columns at or past p_b, which
        only the per-image form has and drops here: nothing downstream sees what the caller left in them."""
        dev = self.eng.prepare(False).device
        prompt = prompt_ids.to(dev)
        B, P = prompt.shape
        per = one.per_image
        plen = np.full(B, P, dtype=np.int32) if one.plen is None else np.asarray(one.plen, dtype=np.int32)
        if per:
            tabs = set_level_tables(one.tries)
            W, K, lengths, fill = tabs.wmax, tabs.kmax, tabs.lengths, float('-inf')
        else:
            trie, = one.tries
            levels = trie_levels(trie)
            depth = np.zeros(trie.nodes, dtype=np.int32)
            for t, lv in enumerate(levels.levels):
                depth[lv.nodes] = t
            W, K, lengths, fill = levels.wmax, int(trie.phrase_node.shape[0]), (depth[trie.phrase_node] + 1).astype(np.int32), 0.0
        pmin, pmax = int(plen.min()), int(plen.max())
        st, Bp = self._score_state_for(B, W, int((plen + one.longest + 1).max()), images_per_pass)
        if per:
            keep = torch.arange(pmax, device=dev)[None, :] < torch.from_numpy(plen).to(dev)[:, None]
            prompt = torch.where(keep, prompt[:, :pmax], torch.zeros((), dtype=torch.long, device=dev))
            walk = self._sets_walk(st, one, tabs, plen, prompt.cpu().numpy(), eos)
        else:
            walk = self._level_walk(st, trie, levels, P, eos)
        out = torch.full((B, K), fill, dtype=F32, device=dev)
        part = torch.zeros(Bp, (K + 3) // 4 * 4, dtype=F32, device=dev)
        self.last_passes = 0
        index_dev = None if one.image_index is None else torch.from_numpy(one.image_index).to(dev)
        pre = self._encode_all(st, images, B if index_dev is None else len(images))
        for i in range(0, B, Bp):
            n = min(Bp, B - i)
            take = torch.arange(i, i + Bp, device=dev).clamp(max=B - 1)         # a short last group is filled with its last image
            self._load_group(st, pre, take if index_dev is None else index_dev.long()[take])
            self._reset(st, prompt[take].repeat_interleave(W, dim=0), pmax)
            st.path[0].zero_()
            part.fill_(fill)
            for _ in range(pmin - 1):                           # prompt tokens every image has before its last: fill the cache only
                self._step(st, False)
            walk(i, part)
            out[i:i + n] = part[:n, :K]
            self.last_passes += 1
        top = out.max(dim=1, keepdim=True).values
        best = torch.where(out == top, torch.arange(K, device=dev)[None, :], torch.full((), K, device=dev)).min(dim=1).values
        return (PhraseSetScores if per else PhraseScores)(out, best, torch.from_numpy(lengths).to(dev), image_index=index_dev)

    def score(self, images, prompt_ids: torch.Tensor, trie: PhraseTrie, eos: int, images_per_pass: Optional[int] = None) -> PhraseScores:
        """``run`` on one checked trie for all images"""
        return self.run(images, prompt_ids, one_closed_set(trie, prompt_ids.shape[0]), eos, images_per_pass)


class PhraseBeamDecoder(BeamDecoder):
    """``search_phrases`` on the static KV cache: a beam over the phrase trie -- BeamDecoder's R = B * W rows, history
    table, shared cross K/V and attention kernels, under GreedyDecoder._replay with ``poll_every``; W rows per image however large the
    set.  A step is _body -> _final_norm -> fp32 lm_head -> i2t_trie_beam_candidates (every live row's W best children and the total of
    ending at its node) -> i2t_trie_beam_select (the pool of finished phrases, the image's next rows, the close test) ->
    i2t_beam_advance.  Every row carries its trie node and path sum in device memory; the trie lives in device buffers the step only
    points at, sized by capacity (_upload_trie), so a captured step serves any set that fits.  The decoder keeps its
    own state; its graph key is ('phrase_beam', ...)."""

    last_replays = 0                    # full-step replays the last call launched (tests, tools)

    def _build_phrase_beam(self, B: int, W: int, ids_ld: int, clen: Optional[int] = None, mem=None):
        st = self._build_beam(B, BeamSpec(W, W, 0.0, None, 0.0, None, 0.0, ()), ids_ld, False, clen, mem)  # cand_tok / cand_lp: [R, W]
        dev = st.arena.device
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=F32, device=dev)
        R = B * W
        st.node, st.path, st.fin_total = torch.zeros(R, **i32), torch.zeros(R, **f32), torch.zeros(R, **f32)
        st.node_init = torch.full((B, W), -1, **i32)
        st.node_init[:, 0] = 0
        self._build_pool(st, B, W)
        st.pool_phrase = torch.zeros(B, W, **i32)
        st.trie = None                      # (child_off, child_tok, child_next, term), made at the first call (_upload_trie)
        st.set_node_init = st.set_plen = st.set_longest = None      # phrase_sets: int32 [B, W] / [B] / [B], made at the first such call
        return st

    def _phrase_beam_step(self, st, P: int, eos: int, longest: int, length_penalty: float, per_image: bool):
        """``per_image``: P is the longest prompt, and every image's prompt length and longest phrase are read from
        st.set_plen / st.set_longest in place of P and ``longest``"""
        dc = self.eng.dec
        off, tok, nxt, term = st.trie
        self._logits_head(st)
        ops.trie_beam_candidates(st.logits, dc.Vp, st.node, st.path, off, tok, term, eos, st.ctrl, st.cand_tok, st.cand_lp, st.fin_total,
                                 st.B, st.W, dc.V)
        shared = (st.cand_tok, st.cand_lp, st.fin_total, st.node, st.path, tok, nxt, term, eos, st.ids, st.hist, st.pool_phrase, st.pool_sum,
                  st.pool_score, st.pool_len, st.pool_n, st.closed, st.counters[0:1], st.counters[1:2], st.ctrl, st.images, st.W, P)
        if per_image:
            ops.trie_beam_select_sets(*shared, st.set_plen, st.set_longest, length_penalty)
        else:
            ops.trie_beam_select(*shared, longest, length_penalty)
        ops.beam_advance(st.counters, st.ctrl)

    @torch.no_grad()
    def run(self, images, prompt_ids: torch.Tensor, one: ClosedSet, eos: int, W: int, N: int, length_penalty: float = 0.0,
            poll_every: int = 8, use_graph: bool = True, each=None) -> PhraseBeams:
        """``phrase_beam_search_host`` for every image of the batch, on the device.  ``one``, ``W``, ``N``: what ``plan_phrase_search``
        returned -- nothing is checked again here.  ``each(i)`` runs after full step i.  One set for all images: row 0 of every image
        starts at the root, P - 1 prefill steps, longest + 1 full steps; P, eos, the longest phrase and the penalty are kernel
        arguments, so a captured step holds them (W is the state's).  ``one.per_image``: row 0 of image b starts at its
        set's root; Pmin - 1 prefill steps, then Pmax - Pmin + max(longest) + 1 full steps in which an image whose prompt reaches past
        the column is held still by i2t_trie_beam_select_sets.  The start nodes, prompt lengths and longest phrases are then device
        tables filled per call: the graph key is ('phrase_beam_sets', Pmax, W, eos, penalty).  Under ``one.image_index`` B
        is Q, the queries: rows are (query, w), the pools are the queries'."""
        eng = self.eng
        dc = eng.dec
        a = eng.prepare(False)
        dev = a.device
        prompt = prompt_ids = prompt_ids.to(dev)
        B, P = prompt_ids.shape
        per = one.per_image
        plen = np.full(B, P, dtype=np.int32) if one.plen is None else np.asarray(one.plen, dtype=np.int32)
        pmin, pmax = (int(plen.min()), int(plen.max())) if per else (P, P)
        longest, length_penalty = int(one.longest.max()), float(length_penalty)
        R, total = B * W, pmax + longest + 1
        mem = (B, False) if one.image_index is None else (len(images), True)
        st = self._state_for(R, total, lambda clen: self._build_phrase_beam(B, W, max(total, dc.block), clen, mem),
                             lambda st: st.W == W, mem)
        self._upload_trie(st, one.trie, ('phrase_beam', 'phrase_beam_sets'))
        node_init = st.node_init
        if per:
            if st.set_node_init is None:    # persistent: the captured steps bake the two tables' pointers
                i32 = dict(dtype=torch.int32, device=dev)
                st.set_node_init, st.set_plen, st.set_longest = torch.full((B, W), -1, **i32), torch.ones(B, **i32), torch.ones(B, **i32)
            node_init = st.set_node_init
            node_init[:, 0] = torch.from_numpy(one.roots).to(dev)
            st.set_plen.copy_(torch.from_numpy(plen))
            st.set_longest.copy_(torch.from_numpy(one.longest))
        row_index, index_dev = self._set_mem_index(st, row_images(one.image_index, W), W)
        self._prepare_inputs(st, images, mem[0], W, index=row_index)
        if per:                             # columns at or past p_b are dropped here: nothing downstream sees what the caller left in them
            keep = torch.arange(pmax, device=dev)[None, :] < st.set_plen[:, None]
            prompt = torch.where(keep, prompt_ids[:, :pmax], torch.zeros((), dtype=torch.long, device=dev))
        prompt_rows = prompt.repeat_interleave(W, dim=0)

        def reset():
            self._reset(st, prompt_rows, pmax)
            st.node.copy_(node_init.view(-1))
            st.path.zero_()
            st.pool_phrase.fill_(-1)
            self._reset_pool(st)
        key = phrase_beam_sets_graph_key(pmax, W, eos, length_penalty) if per else ('phrase_beam', P, W, int(eos), longest, length_penalty)
        self.last_replays = self._replay(st, key, lambda: self._phrase_beam_step(st, pmax, int(eos), longest, length_penalty, per), reset,
                                         pmin - 1, pmax - pmin + longest + 1, use_graph, each=each, poll_every=poll_every, prefill_first=True)
        return PhraseBeams(st.pool_phrase[:, :N].long(), st.pool_sum[:, :N].clone(), st.pool_score[:, :N].clone(), st.pool_len[:, :N].clone(),
                           W >= one.widest_level(), image_index=index_dev)

    def search(self, images, prompt_ids: torch.Tensor, trie: PhraseTrie, eos: int, W: int, N: int, length_penalty: float = 0.0,
               poll_every: int = 8, use_graph: bool = True, each=None) -> PhraseBeams:
        """``run`` on one checked trie for all images"""
        return self.run(images, prompt_ids, one_closed_set(trie, prompt_ids.shape[0]), eos, W, N, length_penalty, poll_every, use_graph, each)

    def search_sets(self, images, prompt_ids: torch.Tensor, sets: PhraseSets, eos: int, W: int, N: int, length_penalty: float = 0.0,
                    poll_every: int = 8, use_graph: bool = True, each=None, plen=None) -> PhraseBeams:
        """``run`` on checked ``PhraseSets`` and (``plen`` int32 [B], or None) a prompt length per image"""
        return self.run(images, prompt_ids, per_image_closed_set(sets, plen), eos, W, N, length_penalty, poll_every, use_graph, each)


def caption_facts(model) -> CaptionFacts:
    """what ``plan_captions`` and the phrase calls' checks need to know of ``model``"""
    dc = model._engine.dec
    block, off, prefix, llama = GreedyDecoder(model)._cache_args()
    window = model.decoder.block_size - model.space_for_prompt
    return CaptionFacts(dc.V, dc.causal, dc.fam, window, prefix, min(window, decode_window(block, off, prefix, llama)) if dc.causal else window,
                        dc.fam is not None and bool(dc.fam.sparse))


def _draw_seed(buf: torch.Tensor, seed: Optional[int]):
    """``seed`` into ``buf``; None: one draw from torch's CPU generator, so ``torch.manual_seed`` reproduces the call"""
    _set_seed(buf, seed if seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item()))


def _set_seed(buf: torch.Tensor, seed: int):
    """the two 32-bit words of a 64-bit seed into an int32 device buffer"""
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    buf.copy_(torch.tensor([lo - (1 << 32) if lo >= (1 << 31) else lo, hi - (1 << 32) if hi >= (1 << 31) else hi], dtype=torch.int32))


def _capture_launches(device, fn):
    """hipGraph of the launches ``fn`` issues, captured on a side stream."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    g = ops.Graph()
    with torch.cuda.stream(side):
        g.begin()
        fn()
        g.end()
    torch.cuda.current_stream().wait_stream(side)
    return g


@torch.no_grad()
def generate_by_recompute(model, images, prompt_ids: torch.Tensor, max_new_tokens: int, sampling: Optional[Sampling] = None):
    """generate() for a NON-causal decoder, as the reference runs it (vision_encoder_decoder.py:143-180): the whole text segment is
    re-evaluated for every new token (with bidirectional attention a new token changes the state of all earlier ones, so there is
    nothing to cache); the encoder runs once, and the token choice -- n-gram ban + argmax or the sampling step -- stays on the device."""
    eng: HotPath = model._engine
    a = eng.prepare(False)
    dc, cfg = eng.dec, model.config
    dev = a.device
    B, P = prompt_ids.shape
    total = P + max_new_tokens
    enc_out, _ = eng.encode(images, False)
    ncls = enc_out.shape[1]
    mem = eng._mem_bf16(enc_out) if eng.cross_inputs else None
    off = ncls if cfg.use_soft_prompting else 0
    blk = dc.block - off
    ids = torch.zeros(B, total, dtype=torch.long, device=dev)
    ids[:, :P] = prompt_ids.to(dev)
    counters = torch.tensor([P - 1, P], dtype=torch.int32, device=dev)
    ngrams = torch.tensor(list(cfg.no_repeat_n_grams), dtype=torch.int32, device=dev)
    logits = torch.zeros(B, dc.Vp, dtype=F32, device=dev)
    margin = torch.zeros(B, dtype=F32, device=dev)
    seed = torch.zeros(2, dtype=torch.int32, device=dev)
    if sampling is not None:
        _draw_seed(seed, sampling.seed)
    for t in range(P, total):
        cond = ids[:, :t] if t <= blk else ids[:, t - blk:t]                     # the reference crops the conditioning to the block
        Tc = cond.shape[1]
        _, hb, _ = eng.decode_segment(B, Tc, mem, ncls, False, ids=cond.contiguous(), pos_offset=off)
        last = hb.view(B, Tc, dc.d)[:, -1].contiguous()
        ops.gemm(last, a.W(eng.n_head), logits, B, dc.V, dc.d)
        if sampling is None:
            ops.ngram_ban_argmax(logits, dc.Vp, ids, total, counters[1:2], ngrams, ngrams.numel(), B, dc.V, margin)
        else:
            ops.sample_token(logits, dc.Vp, ids, total, counters[1:2], ngrams, ngrams.numel(), B, dc.V, sampling.temperature,
                             sampling.top_k, sampling.nucleus_p, seed)
        ops.advance(counters, 1)
    return ids


class ConcurrentGreedyDecoder:
    """Several independent caption batches decoded at the same time, one HIP stream + one captured graph each.

    A single decode stream is latency-bound (one token per caption per step: ~120 short dependent kernels, most of
    them on far fewer than 256 workgroups), so the chip is mostly idle; batches are independent (decode shards
    trivially), so their graphs are replayed on separate streams and overlap on the GPU."""

    def __init__(self, model, n_streams: int):
        self.model = model
        self.lanes = [(GreedyDecoder(model), torch.cuda.Stream()) for _ in range(n_streams)]

    @torch.no_grad()
    def generate(self, image_batches, prompt_batches, max_new_tokens: int):
        assert len(image_batches) == len(prompt_batches) <= len(self.lanes)
        cur = torch.cuda.current_stream()
        # shared state is brought up to date on the parent stream BEFORE fanning out: the bf16 weight shadow's re-cast (if a
        # torch-side optimizer touched the parameters) must not land on one lane's stream while the other lanes read it; the
        # lanes' own prepare() calls then find nothing to do.  Per-lane state (KV caches, graphs, the encoder's conv weight
        # workspace -- keyed by stream in the engine) is private.
        self.model._engine.prepare(False)
        self.model._engine.prepare_lora_merged()
        outs = []
        for (dec, stream), images, prompt in zip(self.lanes, image_batches, prompt_batches):
            stream.wait_stream(cur)
            with torch.cuda.stream(stream):
                outs.append(dec.generate(images, prompt, max_new_tokens))
        for _, stream in self.lanes:
            cur.wait_stream(stream)
        return outs
