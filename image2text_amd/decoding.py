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
"""
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .engine import BF16, F32, HotPath


ENC_CHUNK = int(os.environ.get('I2T_DECODE_ENC_CHUNK', '4096'))      # images per encoder pass inside generate()
TOP2_HEAD = os.environ.get('I2T_DECODE_TOP2', '1') not in ('', '0')    # greedy steps: lm_head + argmax through segment maxima (ops.gemm_top2)


PREFILL_ROWS = int(os.environ.get('I2T_PREFILL_ROWS', '8192'))       # token rows per forward pass of prompt_prefill='pass' 


class Sampling(NamedTuple):
    """How the next token is chosen when it is not the argmax (arguments of the reference's generate, :136-137)."""
    temperature: float = 1.0
    top_k: Optional[int] = None
    nucleus_p: Optional[float] = None
    seed: Optional[int] = None          # 64-bit; None: drawn from torch's CPU generator at the start of the call

    def key(self):
        return (float(self.temperature), int(self.top_k or 0), None if self.nucleus_p is None else float(self.nucleus_p))


# i2t_decode_attention and i2t_gq_decode_attention (csrc/common.h::DECODE_MAX_KEYS) keep the scores of at most this many keys per caption
# in LDS; neither reads a key count from the device against it, so the cache THEY attend over is never allocated longer (a longer
# one is the long state's, below, and runs other kernels)
DECODE_MAX_KEYS = 1024


def text_window(block: int, off: int, prefix: int) -> int:
    """Text positions of the decode step's self-attention cache: the decoder's block less the soft-prompt offset ``off``, capped so
    that ``prefix`` cached prompt rows + the text fit in DECODE_MAX_KEYS keys."""
    tmax = min(block - off, DECODE_MAX_KEYS - prefix)
    if tmax < 1:
        raise ValueError(f'the KV-cache decode step attends over at most {DECODE_MAX_KEYS} keys per caption: {prefix} prompt rows leave '
                         f'no room for text (block {block}, soft-prompt offset {off})')
    return tmax


# The Llama-family decoders with heads of 64 or 128 (row-major cache) have a second attention form, i2t_gq_decode_attention_long,
# which splits a row's keys into chunks of LONG_CHUNK_KEYS across workgroups and bounds a row by its workspace alone
# (csrc/common.h::LONG_CHUNK_KEYS / DECODE_LONG_MAX_KEYS, both pinned by tests/test_long_decode_host_cpu.py).  A call
# that fits text_window never sees it.
LONG_CHUNK_KEYS = ops.LONG_CHUNK_KEYS
DECODE_LONG_MAX_KEYS = 32768
LONG_HEAD_DIMS = (64, 128)          # the head widths the split-key kernels are built for


def takes_long_cache(llama_spec) -> bool:
    """Whether a decoder may decode past text_window: ``llama_spec`` is its Llama-family spec (engine.dec.llama; None for the dense and
    nano-mini decoders).  The plugins also accept heads of 16 and 32, which the split-key kernels are not built for: those decoders
    keep the classic window and its refusal."""
    return llama_spec is not None and llama_spec.hd in LONG_HEAD_DIMS


def decode_window(block: int, off: int, prefix: int, llama: bool) -> int:
    """The text positions a KV-cache call may span: text_window, or -- ``llama``: a decoder that takes the long cache -- the model's
    own block less the soft-prompt offset, with at most DECODE_LONG_MAX_KEYS keys per row, the ``prefix`` prompt rows included."""
    return min(block - off, DECODE_LONG_MAX_KEYS - prefix) if llama else text_window(block, off, prefix)


def cache_plan(block: int, off: int, prefix: int, total: int, llama: bool):
    """-> (clen, long): the slots per row of the self-attention cache that a call over ``total`` id columns runs on, and whether it is
    the long cache of the split-key attention.  A call that fits ``text_window(block, off, prefix)`` gets that window's cache -- what
    every call got before the long form existed -- and long = False.  One that does not, on a decoder that takes the long cache
    (``llama``: takes_long_cache), gets prefix + total slots rounded up to whole chunks, at most prefix + decode_window, and
    long = True.  A total past ``decode_window`` is a ValueError naming that window, the same text for every decoder."""
    try:
        tmax = text_window(block, off, prefix)
    except ValueError:
        if not llama:
            raise
        tmax = 0
    if total <= tmax:
        return tmax + prefix, False
    window = decode_window(block, off, prefix, llama)
    if total > window:
        raise ValueError(f'prompt + new tokens ({total}) exceed the text window ({window})')
    return min(prefix + window, -(-(prefix + total) // LONG_CHUNK_KEYS) * LONG_CHUNK_KEYS), True


def split_attention_host(q: np.ndarray, k: np.ndarray, v: np.ndarray, scale: float, chunk: int = LONG_CHUNK_KEYS) -> np.ndarray:
    """What the split-key decode attention computes, on the host in fp64 (numpy): q [hd] against k / v [n][hd].  Every chunk of
    ``chunk`` keys yields its maximum m_c, s_c = sum exp(score - m_c) and the unnormalised a_c = sum exp(score - m_c) v
    (gq_decode_attention_split_kernel); the combine takes M = max m_c and returns sum_c a_c exp(m_c - M) / sum_c s_c exp(m_c - M), the
    chunks in order."""
    q, k, v = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = k.shape[0]
    assert n >= 1 and chunk >= 1 and k.shape == v.shape and q.shape == k.shape[1:]
    parts = []
    for lo in range(0, n, chunk):
        s = (k[lo:lo + chunk] @ q) * scale
        m = s.max()
        p = np.exp(s - m)
        parts.append((m, p.sum(), p @ v[lo:lo + chunk]))
    M = max(m for m, _, _ in parts)
    num, den = np.zeros_like(q), 0.0
    for m, s, a in parts:
        f = np.exp(m - M)
        num, den = num + a * f, den + s * f
    return num / den


PROMPT_PREFILL_MODES = ('steps', 'pass')


def prefill_plan(mode: str, pmin: int, prefix: int, fam, causal: bool):
    """How ``generate_captions`` fills the cache with the prompt columns every row shares -> (m, (pos, len)): the first m
    prompt columns go through ONE forward pass, the counters start at (pos, len) -- the cache slot and the id column of the first
    step -- and pmin - 1 - m prefill replays follow.  'steps': m = 0, the counters (prefix, 1), pmin - 1 replays: every prompt token a
    decode step.  'pass': m = pmin - 1 and the counters (prefix + m, 1 + m): no prefill replay; pmin = 1 leaves m = 0, which IS
    'steps'.  ``prefix``: the soft-prompt rows at the head of the cache; ``fam``: the nano-mini family's spec (None: a dense or
    Llama-family decoder), refused under 'pass'; a non-causal decoder has no cache and nothing to plan: the mode is checked and ignored."""
    if mode not in PROMPT_PREFILL_MODES:
        raise ValueError(f'prompt_prefill = {mode!r}: one of {PROMPT_PREFILL_MODES}')
    if pmin < 1 or prefix < 0:
        raise ValueError(f'pmin = {pmin}, prefix = {prefix}: every row needs a prompt token, and a prefix cannot be negative')
    if mode == 'steps' or not causal:
        return 0, (prefix, 1)
    if fam is not None:
        raise NotImplementedError("prompt_prefill='pass' is not available for the nano-mini decoder family: a sparse layer caches the "
                                  "positions it keeps by slot, not by position, which the one-pass scatter does not map; use 'steps'")
    m = pmin - 1
    return m, (prefix + m, 1 + m)


def kv_prefill_host(src: np.ndarray, k_off: int, v_off: int, src_T: int, src_t0: int, m: int, kcache: np.ndarray, vcache: np.ndarray,
                    cache_bs: int, cache_rs: int, cache_hs: int, hd: int, w: int, slot0: int, B: int, N: int):
    """What i2t_kv_prefill does, on the host (numpy): ``src`` [rows, src_ld] holds K at columns k_off .. k_off + w - 1 and V at v_off ..;
    token t < m of image b is source row b * src_T + src_t0 + t and goes to slot slot0 + t of cache rows b * N .. b * N + N - 1.
    ``kcache`` / ``vcache`` are FLAT arrays, element (row, head, slot, column) at row * cache_bs + head * cache_hs + slot * cache_rs +
    column (head-major [R][H][clen][64]: cache_rs = 64, cache_hs = clen * 64; row-major [R][clen][w]: cache_rs = w, cache_hs = hd).
    Written in place; nothing else is touched."""
    assert kcache.ndim == 1 and vcache.ndim == 1 and w % hd == 0 and src_t0 + m <= src_T
    for b in range(B):
        for t in range(m):
            row = src[b * src_T + src_t0 + t]
            for n in range(N):
                for h in range(w // hd):
                    at = (b * N + n) * cache_bs + h * cache_hs + (slot0 + t) * cache_rs
                    kcache[at:at + hd] = row[k_off + h * hd:k_off + (h + 1) * hd]
                    vcache[at:at + hd] = row[v_off + h * hd:v_off + (h + 1) * hd]


def slot_positions(member: np.ndarray) -> np.ndarray:
    """int32 [L][slots] from a sparse decoder's membership table (int [L][tmax], 1 where layer l keeps text position p): row l lists
    the text positions layer l keeps, in order, zero-padded -- the position whose K/V sit at each cache slot (slot = rank of the
    position among the kept ones); slots = the largest count, at least 1."""
    member = np.asarray(member) != 0
    kpos = np.zeros((member.shape[0], max(int(member.sum(axis=1).max(initial=0)), 1)), dtype=np.int32)
    for l, row in enumerate(member):
        kept = np.flatnonzero(row)
        kpos[l, :kept.size] = kept
    return kpos


class GreedyDecoder:
    """KV-cache decoder; greedy by default, ``generate(..., sampling=Sampling(...))`` draws tokens on the device instead."""

    def __init__(self, model):
        self.model = model
        self.eng: HotPath = model._engine
        self._state = None
        self._long_state = None             # the state of calls past text_window (cache_plan): classic calls never run on it

    # ------------------------------------------------------------------------------------------------ buffers
    def _cache_args(self):
        """(block, off, prefix, llama) of this model, as decode_window and cache_plan take them"""
        eng, dc = self.eng, self.eng.dec
        ncls = eng.enc.ncls
        return (dc.block, ncls if self.model.config.use_soft_prompting else 0, min(ncls, dc.block) if dc.prefixed else 0,
                takes_long_cache(dc.llama))

    def _state_for(self, rows: int, total: int, build, extra=None):
        """The cached state that serves a call over ``rows`` rows and ``total`` id columns, (re)built by ``build(clen)`` -- clen None: the
        classic window's -- when the cached one does not (_reusable).  A call that fits text_window runs on self._state, whatever ran
        before; one past it (takes_long_cache) on self._long_state, rebuilt when it holds fewer cache slots than the call needs.  A call
        past decode_window is cache_plan's ValueError."""
        block, off, prefix, llama = self._cache_args()
        clen, long = cache_plan(block, off, prefix, total, llama)
        slot = '_long_state' if long else '_state'
        st = getattr(self, slot)
        if not self._reusable(st, rows, total, lambda st: (not long or st.clen >= clen) and (extra is None or extra(st))):
            setattr(self, slot, None)                           # the old buffers go before the new ones are made
            st = build(clen if long else None)
            setattr(self, slot, st)
        assert total <= st.tmax
        return st

    def _build(self, B: int, ids_ld: int, mem_rows: Optional[int] = None, clen: Optional[int] = None):
        """Buffers of a step over B rows; the cross-attention memory holds ``mem_rows`` (default B) rows -- the images, when the B
        rows are beams of them (BeamDecoder).  ``clen``: the cache slots per row of a long state (cache_plan), whose self-attention
        runs the split-key kernels over st.attn_ws; None: the classic window."""
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
        # fp32 planes of the deterministic split-K GEMM form (ops.gemm(workspace=...)): the step's GEMMs with few output tiles and a
        # long K (attention / MLP output projections at anything but the largest caption batches) spread over K slices
        st.ws = torch.empty(16 << 20, dtype=F32, device=dev)
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
        st.hist = None                      # beam search: int32 [B][clen] history table (BeamDecoder), None: row b's keys are row b's
        st.mem_div = 1                      # rows per cross-attention memory row
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
        self._body(st)
        if with_head:
            self._final_norm(st)
            if top2 and sampling is None:
                # greedy, nobody asked for margins: the lm_head leaves the two largest logits of every 64-column segment of a row
                # instead of the row (51 MB instead of 823 MB written and read back at 4096 captions), the ban + argmax merges them
                ops.gemm_top2(st.hid, a.W(eng.n_head), st.top2, B, dc.V, d)
                ops.top2_ngram_argmax(st.top2, st.hid, a.W(eng.n_head), st.ids, st.ids_ld, len_ptr, st.ngrams, st.ngrams.numel(), B, dc.V, d)
                ops.advance(st.counters, 1)
                return
            ops.gemm(st.hid, a.W(eng.n_head), st.logits, B, dc.V, d, workspace=st.ws)
            if sampling is None:
                ops.ngram_ban_argmax(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, st.ngrams.numel(), B, dc.V, st.margin)
            else:
                ops.sample_token(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, st.ngrams.numel(), B, dc.V,
                                 sampling.temperature, sampling.top_k, sampling.nucleus_p, st.seed, dist_out=st.dist)
        ops.advance(st.counters, 1)                            # pos and len together

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
        if top2 and getattr(st, 'top2', None) is None:
            nseg = (dc.V + 63) // 64
            st.top2 = torch.zeros(st.B, nseg, 4, dtype=F32, device=st.arena.device)
            if lse:
                st.seg_se = torch.zeros(st.B, nseg, dtype=F32, device=st.arena.device)
        return top2, ('greedy_top2' if top2 else 'greedy') if sampling is None else sampling.key()

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

    def _prepare_inputs(self, st, images, B: int, W: int = 1, prefill=None):
        """Everything a step reads besides the ids: the encoder output of the B images, the per-layer cross K/V (B rows), the
        soft-prompt rows' K/V at the head of the cache (copied to the W rows b * W .. b * W + W - 1 of every image) and the packed
        expert weights.  ``prefill`` = (prompt [B, >= m], m >= 1) under prompt_prefill='pass': the first m prompt columns' K/V go into
        the cache too, from one pass that also covers the soft-prompt rows (_prefill_pass)."""
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
                    st.kc[l].view(B, W, st.clen, -1)[:, :, :n_p].copy_(qkv[..., ls.H * ls.hd:(ls.H + ls.Hkv) * ls.hd].unsqueeze(1))
                    st.vc[l].view(B, W, st.clen, -1)[:, :, :n_p].copy_(qkv[..., (ls.H + ls.Hkv) * ls.hd:].unsqueeze(1))
                eng._layer_sink = take_kv
            try:
                _, _, pctx = eng.decode_segment(B, n_p, eng._mem_bf16(enc_out) if eng.cross_inputs else None, S, True,
                                                embeds=enc_out[:, :n_p].reshape(B * n_p, dc.d), pos_offset=0)
            finally:
                eng._layer_sink = None
            for l in range(dc.L if dc.llama is None else 0):
                qkv = pctx.saves[l].qkv.view(B, n_p, 3, dc.H, 64)
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
                st.graphs = {k: g for k, g in st.graphs.items() if k in (None, 'greedy', 'greedy_top2')}
        top2, full_key = self._greedy_head(st, sampling, logits=return_margins)

        def reset():
            st.ids.zero_()
            st.ids[:, :P] = prompt_ids
            st.counters.copy_(st.counters_init)                 # device-to-device: no host sync in the loop
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


class BeamSpec(NamedTuple):
    """Arguments of a beam search (BeamSearchTokenGenerator's, models/generation_utils.py); eos None: no EOS rule."""
    beam_width: int = 3
    expansion: int = 4
    temperature: float = 1.0
    top_k: Optional[int] = None
    consolidation_temperature: float = 1.0
    eos: Optional[int] = None
    log_boost: float = 0.0
    ngram_sizes: tuple = (2, 3, 4)

    def key(self):
        return (int(self.beam_width), int(self.expansion), float(self.temperature), int(self.top_k or 0),
                float(self.consolidation_temperature), -1 if self.eos is None else int(self.eos), float(self.log_boost),
                tuple(int(n) for n in self.ngram_sizes))


class BeamDecoder(GreedyDecoder):
    """Beam search on the static KV cache: R = B * W rows (batch-major, r = b * W + w) through GreedyDecoder's buffers and layer
    sequence, under GreedyDecoder._replay (no poll).  The step's head is the fp32 lm_head, then on the device (csrc/beam.hip):
    i2t_beam_candidates (ban, crop, E candidates, EOS rule) -> i2t_beam_consolidate (W survivors per caption, ids and history rows
    moved to the children) -> i2t_beam_advance.  Survivors copy no K/V: the history table st.hist[r][t] names the cache row that
    holds key t of beam r, and the attention kernels read through it (a sparse layer's slot s through hist[r][st.kpos[l][s]], the
    text position the slot holds).  The encoder and the cross K/V run once per image
    (rows_per_mem = W); the prompt is prefilled for all R rows under the identity table.  Once every beam of every caption holds
    EOS the remaining replays do nothing, so the host launches them all and reads the final length once."""

    def _build_beam(self, B: int, spec: BeamSpec, ids_ld: int, record: bool, clen: Optional[int] = None):
        W, E = spec.beam_width, spec.expansion
        R = B * W
        st = self._build(R, ids_ld, mem_rows=B, clen=clen)
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

    def _beam_step(self, st):
        eng, a, dc, sp = self.eng, self.eng.arena, self.eng.dec, st.spec
        pos_ptr, len_ptr = st.counters[0:1], st.counters[1:2]
        self._body(st)
        self._final_norm(st)
        ops.gemm(st.hid, a.W(eng.n_head), st.logits, st.B, dc.V, dc.d, workspace=st.ws)
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
                             lambda st: (getattr(st, 'W', None) == W and st.spec.key() == spec.key() and (st.raw_tok is not None) == record))
        prompt_rows = prompt_ids.repeat_interleave(W, dim=0)
        if spec.eos is not None and bool((prompt_ids == spec.eos).any(dim=-1).all()):
            ids = prompt_rows.view(B, W, P).clone()          # every beam already holds EOS: nothing to do
            return (ids, torch.zeros(B, W, device=a.device)) + (([],) if record else ())
        self._prepare_inputs(st, images, B, W)
        _draw_seed(st.seed, seed)

        def reset():
            st.ids.zero_()
            st.ids[:, :P] = prompt_rows
            st.counters.copy_(st.counters_init)
            st.hist.copy_(st.hist_init)
            st.scores.zero_()
            st.ctrl.zero_()
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


class _CaptionFields(NamedTuple):
    ids: torch.Tensor                   # int64 [B, N, L]: prompt, new tokens up to and including the first emitted EOS, then the pad id
    lengths: torch.Tensor               # int32 [B, N]: prompt + new tokens up to and including that EOS (P + max_new_tokens without one)
    token_logprobs: torch.Tensor        # fp32 [B, N, L - P]: log_softmax of the step's raw logits at the chosen token; 0.0 past the EOS
    logprob: torch.Tensor               # fp32 [B, N]: the row sums


class GeneratedCaptions(_CaptionFields):
    """What ``generate_captions`` returns; rows are batch-major (caption n of image b).  The four fields above are the tuple: it
    unpacks into four and ``_fields`` names four, as before ``prompt_lengths`` existed.  ``prompt_lengths`` (int32 [B], or None when
    every row's prompt fills all P columns) is the optional fifth argument and an attribute beside them; with it ``lengths`` counts
    from p_b and ``token_logprobs`` is [B, N, L - Pmin], entry t belonging to column Pmin + t.  ``_replace`` and
    ``_make`` build the four fields only."""
    prompt_lengths: Optional[torch.Tensor] = None
    beam_scores: Optional[torch.Tensor] = None      # fp32 [B, N] under num_beams > 1: the length-penalised score the N
                                                    # captions of an image are sorted by, best first; None in every other mode
    phrase_index: Optional[torch.Tensor] = None     # int32 [B, N] under ``phrases``: the index into ``phrases`` of the
                                                    # phrase the row emitted; None in every other mode

    def __new__(cls, ids, lengths, token_logprobs, logprob, prompt_lengths=None, beam_scores=None, phrase_index=None):
        self = super().__new__(cls, ids, lengths, token_logprobs, logprob)
        self.prompt_lengths = prompt_lengths
        self.beam_scores = beam_scores
        self.phrase_index = phrase_index
        return self


def apply_finish_rule(ids: np.ndarray, P: int, eos: Optional[int], pad: Optional[int] = None, token_logprobs: Optional[np.ndarray] = None):
    """The finish rule of ``generate_captions`` on the host (numpy): what i2t_caption_finish does step by step on the device, applied to
    whole rows.  ``ids`` [R, P + T]: the prompt and the T tokens a chooser emitted for every row (it goes on emitting after an EOS).  A row
    is finished once it has EMITTED ``eos`` -- an EOS inside the prompt does not count --, that EOS is kept, later columns hold ``pad``
    (default: the EOS id) and log-prob 0.0, a row without one has length P + T; ``eos`` None: no rule.  The steps end once every row has
    finished, so L = lengths.max().  This is ``apply_finish_rule_ragged`` with every prompt P long, less its refusals (no rows, or an
    empty prompt, pass).  -> (ids [R, L], lengths int32 [R], token_logprobs [R, L - P] or None)"""
    ids = np.array(ids)
    return _finish_rows(ids, np.full(ids.shape[0], P, dtype=np.int64), P, ids.shape[1] - P, eos, pad, token_logprobs)


def apply_finish_rule_ragged(ids: np.ndarray, plen, max_new: int, eos: Optional[int], pad: Optional[int] = None,
                             token_logprobs: Optional[np.ndarray] = None):
    """``apply_finish_rule`` for rows whose prompts differ in length: what i2t_caption_finish_ragged does step by step on the device.
    ``ids`` [R, Pmax + max_new]: row r holds its prompt in columns < plen[r] and the tokens a chooser emitted from column plen[r] on
    (columns at or past plen[r] + max_new are not read); ``token_logprobs`` [R, Pmax + max_new - Pmin] is aligned by COLUMN, entry t
    belonging to column Pmin + t.  A row is finished once it has EMITTED ``eos`` (an EOS inside its prompt does not count; ``eos``
    None: never) or ``max_new`` tokens; ``lengths[r]`` = plen[r] + the emitted tokens up to and including that EOS; later columns hold
    ``pad`` (default: the EOS id, 0 without one) and log-prob 0.0, and so do a row's prompt columns (nothing was chosen there).
    L = lengths.max().  With every plen[r] = P this is ``apply_finish_rule(ids, P, eos, pad, token_logprobs)``.
    -> (ids [R, L], lengths int32 [R], token_logprobs [R, L - Pmin] or None)"""
    ids = np.array(ids)
    plen = np.asarray(plen, dtype=np.int64).reshape(-1)
    R, total = ids.shape
    assert plen.shape == (R,) and R >= 1 and max_new >= 0 and int(plen.min()) >= 1 and int(plen.max()) + max_new == total
    return _finish_rows(ids, plen, int(plen.min()), max_new, eos, pad, token_logprobs)


def _finish_rows(ids: np.ndarray, plen: np.ndarray, pmin: int, max_new: int, eos, pad, token_logprobs):
    """the rule both ``apply_finish_rule`` forms state; ``ids`` is the caller's copy and is written"""
    R, total = ids.shape
    pad = (0 if eos is None else eos) if pad is None else pad
    lengths = (plen + max_new).astype(np.int32)
    for r in range(R if eos is not None else 0):
        hit = np.flatnonzero(ids[r, plen[r]:plen[r] + max_new] == eos)
        if hit.size:
            lengths[r] = plen[r] + int(hit[0]) + 1
    L = int(lengths.max()) if R else total
    ids = ids[:, :L]
    lp = None if token_logprobs is None else np.array(token_logprobs)[:, :L - pmin]
    for r in range(R):
        ids[r, lengths[r]:] = pad
        if lp is not None:
            lp[r, :plen[r] - pmin] = 0.0
            lp[r, lengths[r] - pmin:] = 0.0
    return ids, lengths, lp


class Processors(NamedTuple):
    """The active logits processors of a ``generate_captions`` call, as ``caption_processors`` leaves them."""
    theta: float                        # repetition penalty; the kernel and the host statement round it to fp32
    inv_theta: float                    # fp32(1) / fp32(theta), formed once here: the device multiplies
    min_new: int                        # EOS is banned while a row has emitted fewer tokens (0 without an EOS id: no rule)
    suppress: tuple                     # distinct ids in [0, V) that are never emitted

    def key(self):
        """what a captured step bakes of them; the list's contents are copied into st.suppress per call"""
        return (float(self.theta), int(self.min_new), len(self.suppress))


def caption_processors(repetition_penalty: float, min_new_tokens: int, suppress_tokens, max_new_tokens: int, eos, vocab: Optional[int]):
    """The refusals of ``repetition_penalty`` / ``min_new_tokens`` / ``suppress_tokens`` (host only) -> Processors, or None when none of
    them is active: penalty 1, no suppressed id, and min_new_tokens 0 or no EOS id to ban (then the call is the one without them).
    ``vocab`` None: ids are not checked against a vocabulary.  Duplicates in the list are dropped; an EOS id in the list together with
    min_new_tokens > 0 is allowed (the same -inf twice)."""
    theta = float(repetition_penalty)
    if not np.isfinite(theta) or theta <= 0:
        raise ValueError(f'repetition_penalty = {repetition_penalty}: a finite value above 0 is needed (1.0: none)')
    with np.errstate(all='ignore'):
        inv = np.float32(1.0) / np.float32(theta)
    if not (np.isfinite(inv) and inv > 0 and np.isfinite(np.float32(theta)) and np.float32(theta) > 0):
        raise ValueError(f'repetition_penalty = {repetition_penalty}: neither it nor its reciprocal is a positive finite fp32 number')
    min_new = int(min_new_tokens)
    if min_new != min_new_tokens or min_new < 0:
        raise ValueError(f'min_new_tokens = {min_new_tokens}: a whole number of tokens, 0 or more')
    if min_new > max_new_tokens:
        raise ValueError(f'min_new_tokens = {min_new} exceeds max_new_tokens = {max_new_tokens}')
    if isinstance(suppress_tokens, torch.Tensor):
        suppress_tokens = suppress_tokens.detach().cpu().reshape(-1).tolist()
    suppress = []
    for t in (suppress_tokens if suppress_tokens is not None else ()):
        if int(t) != t:
            raise ValueError(f'suppress_tokens holds {t!r}: token ids are integers')
        if int(t) < 0 or (vocab is not None and int(t) >= vocab):
            raise ValueError(f'suppress_tokens holds {int(t)}: outside the vocabulary [0, {vocab if vocab is not None else "V"})')
        if int(t) not in suppress:
            suppress.append(int(t))
    if vocab is not None and len(suppress) >= vocab:
        raise ValueError(f'suppress_tokens covers the whole vocabulary of {vocab} tokens: nothing is left to emit')
    if eos is None:
        min_new = 0
    if theta == 1.0 and not suppress and min_new == 0:
        return None
    return Processors(theta, float(inv), min_new, tuple(suppress))


def process_logits_host(z, ids_row, length: int, emitted: int, theta: float, suppress, eos: Optional[int], min_new: int) -> np.ndarray:
    """What i2t_caption_logits_process leaves of one raw fp32 logits row ``z`` [V], on the host (numpy fp32, a copy): it is to the
    pre-pass what ``apply_finish_rule`` is to the finish kernel.  In the order of transformers' RepetitionPenaltyLogitsProcessor ->
    SuppressTokensLogitsProcessor -> MinNewTokensLengthLogitsProcessor: every DISTINCT token t of ``ids_row[:length]`` (the prompt
    included) gets z[t] * fp32(1 / theta) if z[t] > 0, else z[t] * fp32(theta) -- one fp32 multiply, as on the device; z[t] = -inf
    for t in ``suppress``; z[eos] = -inf while ``emitted`` < ``min_new`` (``eos`` None: no rule).  Ids outside [0, V) take no part."""
    z = np.array(z, dtype=np.float32)
    assert z.ndim == 1
    V = z.shape[0]
    th = np.float32(theta)
    inv = np.float32(1.0) / th
    seen = np.unique(np.asarray(ids_row).reshape(-1)[:length].astype(np.int64))
    seen = seen[(seen >= 0) & (seen < V)]
    v = z[seen]
    z[seen] = np.where(v > 0, v * inv, v * th).astype(np.float32)
    sup = [int(t) for t in (suppress if suppress is not None else ()) if 0 <= int(t) < V]
    z[sup] = -np.inf
    if eos is not None and 0 <= eos < V and emitted < min_new:
        z[eos] = -np.inf
    return z


def caption_graph_key(head, eos, pad, ragged_max_new: Optional[int] = None, proc: Optional[Processors] = None, P: int = 0, trie: bool = False):
    """The graph key of a ``generate_captions`` full step: everything a captured step holds as a kernel argument.  (head, eos, pad), or
    ('ragged', head, eos, pad, max_new) under ``prompt_lengths`` -- and with active processors ('proc', theta, min_new, n_suppress, P,
    ...that key): an inactive call never sees a 'proc' key.  ``P``: the prompt length the min-length count starts from (0 when ragged:
    the count then reads the device's table).  ``trie`` (a ``phrases`` call): ('trie', eos, ...that key) -- the trie's
    contents live in device buffers the step only points at, so they are no part of it; a call without phrases never sees a 'trie' key."""
    key = (head, eos, pad) if ragged_max_new is None else ('ragged', head, eos, pad, ragged_max_new)
    key = key if proc is None else ('proc',) + proc.key() + (0 if ragged_max_new is not None else int(P),) + key
    return ('trie', eos) + key if trie else key


# ------------------------------------------------------------------------------------------------ phrase sets
class PhraseTrie(NamedTuple):
    """A phrase set as a flat CSR trie (``phrase_trie``); node 0 is the root.  All arrays numpy int32."""
    child_off: np.ndarray               # [nodes + 1]: the children of node n are edges child_off[n] .. child_off[n + 1)
    child_tok: np.ndarray               # [edges]: an edge's token, ascending within a node
    child_next: np.ndarray              # [edges]: the node the edge leads to
    term: np.ndarray                    # [nodes]: the index of the phrase that ends at the node (the lowest among duplicates), or -1
    max_fanout: int                     # the largest number of children of a node
    longest: int                        # the tokens of the longest phrase
    phrase_node: Optional[np.ndarray] = None    # [K]: the node at which phrase k ends, duplicates included (``phrase_trie`` fills it;
                                                # ``score_phrases`` needs it: ``term`` keeps the lowest index of a node only)

    @property
    def nodes(self) -> int:
        return int(self.term.shape[0])

    @property
    def edges(self) -> int:
        return int(self.child_tok.shape[0])

    def children(self, node: int):
        """-> (tokens, next nodes) of ``node``"""
        lo, hi = int(self.child_off[node]), int(self.child_off[node + 1])
        return self.child_tok[lo:hi], self.child_next[lo:hi]


def phrase_trie(phrases, eos, vocab: int, max_new_tokens: int) -> PhraseTrie:
    """The refusals of ``generate_captions(phrases=...)`` that concern the set itself (host only, ValueError) and the set as a
    ``PhraseTrie``.  ``phrases``: K >= 1 sequences (or 1-D tensors) of token ids in [0, ``vocab``), none empty, none holding ``eos``;
    ``eos`` is needed (a row ends its phrase by emitting it) and ``max_new_tokens`` must reach the longest phrase + 1, so that every
    row can end with EOS and the finish rule never cuts a phrase.  Duplicate phrases keep the lowest index."""
    if eos is None:
        raise ValueError('phrases need eos_token_id: a row ends its phrase by emitting it')
    eos = int(eos)
    if not 0 <= eos < vocab:
        raise ValueError(f'eos_token_id = {eos} outside the vocabulary [0, {vocab})')
    if isinstance(phrases, torch.Tensor):
        phrases = phrases.detach().cpu().tolist()
    rows = []
    for k, ph in enumerate(phrases):
        if isinstance(ph, torch.Tensor):
            ph = ph.detach().cpu().reshape(-1).tolist()
        row = []
        for t in ph:
            if int(t) != t:
                raise ValueError(f'phrases[{k}] holds {t!r}: token ids are integers')
            t = int(t)
            if not 0 <= t < vocab:
                raise ValueError(f'phrases[{k}] holds {t}: outside the vocabulary [0, {vocab})')
            if t == eos:
                raise ValueError(f'phrases[{k}] holds eos_token_id = {eos}: the EOS ends a phrase, it cannot be inside one')
            row.append(t)
        if not row:
            raise ValueError(f'phrases[{k}] is empty: a phrase holds at least one token')
        rows.append(row)
    if not rows:
        raise ValueError('phrases is empty: at least one phrase is needed')
    longest = max(len(r) for r in rows)
    if max_new_tokens < longest + 1:
        raise ValueError(f'max_new_tokens = {max_new_tokens} is below the longest phrase + 1 = {longest + 1}: every row ends with EOS')
    kids, term, ends = [{}], [-1], []                           # insertion: node -> {token: next node}
    for k, row in enumerate(rows):
        n = 0
        for t in row:
            if t not in kids[n]:
                kids[n][t] = len(kids)
                kids.append({})
                term.append(-1)
            n = kids[n][t]
        if term[n] < 0:
            term[n] = k
        ends.append(n)
    off, tok, nxt = [0], [], []
    for d in kids:
        for t in sorted(d):
            tok.append(t)
            nxt.append(d[t])
        off.append(len(tok))
    i32 = np.int32
    return PhraseTrie(np.array(off, dtype=i32), np.array(tok, dtype=i32), np.array(nxt, dtype=i32), np.array(term, dtype=i32),
                      max(len(d) for d in kids), longest, np.array(ends, dtype=i32))


def check_phrase_caption_args(phrases, eos, vocab: int, max_new_tokens: int, prompt_lengths=None, processors_active: bool = False,
                              num_beams=1, causal: bool = True) -> PhraseTrie:
    """``phrase_trie`` and then what ``phrases`` does not combine with, all before anything runs -> the trie.  NotImplementedError,
    naming the reason: ``prompt_lengths``, an active logits processor, ``num_beams`` > 1, a non-causal decoder.  ``phrases`` may be a
    ``PhraseTrie`` that an earlier call of this function built (the model hands its own to the decoder): it is not built again, only
    held against this call's ``eos``, ``vocab`` and ``max_new_tokens``."""
    if isinstance(phrases, PhraseTrie):
        trie = phrases
        if eos is None or not 0 <= int(eos) < vocab or trie.edges < 1 or int(trie.child_tok.min()) < 0 or int(trie.child_tok.max()) >= vocab \
                or bool((trie.child_tok == int(eos)).any()) or max_new_tokens < trie.longest + 1:
            raise ValueError(f'a PhraseTrie built for another call: eos_token_id = {eos}, vocabulary {vocab}, max_new_tokens = '
                             f'{max_new_tokens} against a longest phrase of {trie.longest} tokens')
    else:
        trie = phrase_trie(phrases, eos, vocab, max_new_tokens)
    if prompt_lengths is not None:
        raise NotImplementedError('phrases with prompt_lengths: a forced prompt column would have to hold the trie still, and the ragged '
                                  'finish rule has no such case')
    if processors_active:
        raise NotImplementedError('phrases with repetition_penalty / min_new_tokens / suppress_tokens: the phrase set says what may be '
                                  'emitted, and a processor could leave a node without an allowed token')
    if isinstance(num_beams, (int, np.integer)) and not isinstance(num_beams, bool) and num_beams > 1:
        raise NotImplementedError('phrases under num_beams > 1: the beam step has no trie state per hypothesis')
    if not causal:
        raise NotImplementedError('phrases run inside the KV-cache caption step; a non-causal decoder generates by re-evaluation '
                                  '(generate_by_recompute), which has no constrained step')
    return trie


def trie_mask_host(z, node: int, trie: PhraseTrie, eos: int) -> np.ndarray:
    """What i2t_caption_trie_mask leaves of one raw fp32 logits row ``z`` [V], on the host (numpy fp32, a copy): -inf everywhere except
    the columns of ``node``'s children and, when a phrase ends at ``node``, the EOS column; those keep their raw values."""
    z = np.array(z, dtype=np.float32)
    assert z.ndim == 1
    out = np.full_like(z, -np.inf)
    toks, _ = trie.children(node)
    out[toks] = z[toks]
    if trie.term[node] >= 0:
        out[eos] = z[eos]
    return out


def trie_advance_host(node: int, token: int, trie: PhraseTrie, eos: int):
    """What i2t_caption_trie_advance does with a row at ``node`` whose chooser wrote ``token`` -> (node, phrase index or -1, whether
    the token was one the node allows).  EOS at a node that ends a phrase names that phrase and the node stays; a child moves the row;
    anything else (never from a chooser) changes nothing, and the kernel then leaves the step's log-prob as it was."""
    token = int(token)
    if token == eos:
        p = int(trie.term[node])
        return node, p, p >= 0
    toks, nxt = trie.children(node)
    at = int(np.searchsorted(toks, token))
    if at < toks.shape[0] and int(toks[at]) == token:
        return int(nxt[at]), -1, True
    return node, -1, False


def constrained_decode_host(step_logits, prompt, trie: PhraseTrie, eos: int, pad, max_new: int):
    """The whole greedy search of ``generate_captions(phrases=...)`` for ONE image on the host: ``step_logits(sequence)`` gives the fp32
    logits row [V] that follows a token sequence (a list of ints, the prompt included).  Every step takes ``trie_mask_host`` of the
    row, its argmax (the lower id on ties), the fp32 log_softmax of the RAW row there, and ``trie_advance_host``; the search ends with
    the EOS.  -> SimpleNamespace(ids int64 [L], length, token_logprobs f32 [L - P], logprob f32, phrase_index, steps, gaps): ``gaps``
    holds per step the best allowed logit minus the second-best allowed one (inf where a node allows one token).  A search whose gaps
    all exceed a perturbation of the logits keeps its result under it.  (``pad`` takes no part for one image -- nothing follows the EOS;
    the signature is ``beam_search_host``'s.)"""
    seq = [int(t) for t in np.asarray(prompt).reshape(-1)]
    P = len(seq)
    assert P >= 1 and max_new >= 1
    f32 = np.float32
    node, phrase, lps, gaps = 0, -1, [], []
    while phrase < 0 and len(seq) - P < max_new:
        z = np.asarray(step_logits(list(seq)), dtype=f32).reshape(-1)
        masked = trie_mask_host(z, node, trie, eos)
        order = sorted(np.flatnonzero(masked > -np.inf).tolist(), key=lambda t: (-masked[t], t))
        assert order, 'no allowed token has a finite logit'
        c = order[0]
        gaps.append(float(masked[c]) - float(masked[order[1]]) if len(order) > 1 else float('inf'))
        m = z.max()
        lps.append(f32(z[c] - (m + np.log(np.exp(z - m, dtype=f32).sum(dtype=f32), dtype=f32))))
        node, phrase, ok = trie_advance_host(node, c, trie, eos)
        assert ok
        seq.append(c)
    lp = np.array(lps, dtype=f32)
    return SimpleNamespace(ids=np.array(seq, dtype=np.int64), length=len(seq), token_logprobs=lp, logprob=lp.sum(dtype=f32),
                           phrase_index=phrase, steps=len(lps), gaps=gaps)


# ------------------------------------------------------------------------------------------------ exact phrase scores
class PhraseScores(NamedTuple):
    """What ``score_phrases`` returns."""
    logprob: torch.Tensor               # fp32 [B, K]: the raw log-likelihood of phrase k + EOS after image b's prompt (``score``'s quantity)
    best: torch.Tensor                  # int64 [B]: the argmax over k, the lowest index on ties (duplicate phrases tie exactly)
    lengths: torch.Tensor               # int32 [K]: the tokens of each phrase + 1 (the EOS)


class TrieLevel(NamedTuple):
    """The nodes of one depth of a phrase trie (``trie_levels``); all arrays numpy int32."""
    nodes: np.ndarray                   # [n_t]: the nodes at depth t, ascending (node order)
    rows: np.ndarray                    # [n_t]: the row w each of them holds during the level's step -- its rank in ``nodes``
    parent_rows: np.ndarray             # [n_t]: the row its parent held at depth t - 1 (-1 at the root)
    tokens: np.ndarray                  # [n_t]: the token of the edge that leads to it (-1 at the root)
    term: np.ndarray                    # [n_t]: trie.term of the node
    anc: np.ndarray                     # [wmax, t + 1]: anc[w][j] = the row the depth-j ancestor of row w's node held (j = t: w itself);
                                        # rows w >= n_t hold no node: w in every column


class TrieLevels(NamedTuple):
    levels: tuple                       # TrieLevel for t = 0 (the root alone) .. longest
    wmax: int                           # the widest level: the rows per image of the walk

    def history(self, t: int, first: int, clen: int) -> np.ndarray:
        """int32 [wmax, clen]: the static history table of level t's step.  ``first`` is the cache slot the level-0 step writes (the
        last prompt token's: soft-prompt rows + P - 1), so the level-j step writes slot first + j, in the row the depth-j node holds.
        Key slot s of row w is read from cache row history[w][s]: slots up to ``first`` -- soft prompt and prompt, which every row ran
        itself -- and slot first + t, which the row writes in this very step, from row w; slot first + j, 0 < j < t, from anc[w][j];
        later slots are not read (w)."""
        lv = self.levels[t]
        assert first >= 0 and first + t < clen
        h = np.repeat(np.arange(self.wmax, dtype=np.int32)[:, None], clen, axis=1)
        h[:, first + 1:first + t] = lv.anc[:, 1:t]
        return h


def trie_levels(trie: PhraseTrie) -> TrieLevels:
    """The CSR trie as per-depth tables, t = 0 .. trie.longest, built once on the host: ``score_phrases`` walks them level by level, a
    "beam search" that prunes nothing and whose parents come from the trie instead of a top-k, so every table is static."""
    n = trie.nodes
    depth, parent, token = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    depth[0] = 0
    order = [0]
    for nd in order:                                            # breadth first from the root: a parent is placed before its children
        toks, nxt = trie.children(nd)
        for tk, c in zip(toks.tolist(), nxt.tolist()):
            assert depth[c] < 0, 'not a tree'
            depth[c], parent[c], token[c] = depth[nd] + 1, nd, tk
            order.append(c)
    assert len(order) == n and int(depth.max()) == trie.longest, 'the trie holds nodes its root does not reach, or a wrong longest'
    per = [np.flatnonzero(depth == t).astype(np.int32) for t in range(trie.longest + 1)]
    wmax = max(p.shape[0] for p in per)
    row_of = np.zeros(n, dtype=np.int32)
    for p in per:
        row_of[p] = np.arange(p.shape[0], dtype=np.int32)
    levels = []
    for t, nodes in enumerate(per):
        anc = np.repeat(np.arange(wmax, dtype=np.int32)[:, None], t + 1, axis=1)
        at = nodes.copy()
        for j in range(t, -1, -1):                              # up the tree: the depth-j ancestor of every node of the level
            anc[:nodes.shape[0], j] = row_of[at]
            at = parent[at] if j else at
        levels.append(TrieLevel(nodes, np.arange(nodes.shape[0], dtype=np.int32),
                                row_of[parent[nodes]] if t else np.full(1, -1, dtype=np.int32), token[nodes], trie.term[nodes], anc))
    return TrieLevels(tuple(levels), int(wmax))


def phrase_node_csr(trie: PhraseTrie):
    """-> (off int32 [nodes + 1], idx int32 [K]): the phrases that end at node n are idx[off[n] .. off[n + 1]), ascending -- the
    duplicates of a phrase share its node, which ``trie.term`` names by the lowest index only"""
    if trie.phrase_node is None:
        raise ValueError('a PhraseTrie without phrase_node (not built by phrase_trie): the phrases that share a node are unknown')
    ends = np.asarray(trie.phrase_node, dtype=np.int64)
    idx = np.argsort(ends, kind='stable').astype(np.int32)
    off = np.zeros(trie.nodes + 1, dtype=np.int32)
    np.cumsum(np.bincount(ends, minlength=trie.nodes), out=off[1:])
    return off, idx


def level_expand_tables(trie: PhraseTrie, levels: TrieLevels, t: int):
    """The five tables i2t_trie_level_expand takes at level t (numpy int32) -> (child_parent, child_tok, term_row, term_off,
    term_phrase): the nodes of level t + 1 in row order with their parents' rows at level t (empty at the last level), and the rows of
    level t whose node ends a phrase with the CSR of the phrase indices that end there."""
    i32 = np.int32
    lv = levels.levels[t]
    nxt = levels.levels[t + 1] if t + 1 < len(levels.levels) else None
    child_parent = nxt.parent_rows if nxt is not None else np.zeros(0, dtype=i32)
    child_tok = nxt.tokens if nxt is not None else np.zeros(0, dtype=i32)
    off, idx = phrase_node_csr(trie)
    rows = [w for w, nd in enumerate(lv.nodes.tolist()) if off[nd + 1] > off[nd]]
    term_off, term_phrase = [0], []
    for w in rows:
        nd = int(lv.nodes[w])
        term_phrase += idx[off[nd]:off[nd + 1]].tolist()
        term_off.append(len(term_phrase))
    return child_parent.astype(i32), child_tok.astype(i32), np.array(rows, dtype=i32), np.array(term_off, dtype=i32), np.array(term_phrase, dtype=i32)


def phrase_scores_host(step_logits_fn, trie: PhraseTrie, eos: int, prompt=()):
    """The normative replica of ``score_phrases`` for ONE image on the host: ``step_logits_fn(sequence)`` gives the raw fp32 logits row
    [V] that follows a token sequence (a list of ints: ``prompt``, then the path from the root).  The levels are walked in order; every
    node's row gives lse = m + log(sum exp(z - m)) in fp32, a child's path sum is path[parent] + (z[token] - lse) and a phrase that ends
    at the node gets path[node] + (z[eos] - lse), in exactly this order in fp32 -- the device's (i2t_trie_level_expand).
    -> SimpleNamespace(logprob f32 [K], best: the argmax, the lowest index on ties, lengths int32 [K])."""
    f32 = np.float32
    levels = trie_levels(trie)
    off, idx = phrase_node_csr(trie)
    K = idx.shape[0]
    logprob = np.zeros(K, dtype=f32)
    prompt = [int(t) for t in np.asarray(prompt).reshape(-1)]
    path, seq = {0: f32(0.0)}, {0: []}
    for lv in levels.levels:
        for nd in lv.nodes.tolist():
            z = np.asarray(step_logits_fn(prompt + seq[nd]), dtype=f32).reshape(-1)
            m = z.max()
            lse = f32(m + np.log(np.exp(z - m, dtype=f32).sum(dtype=f32), dtype=f32))
            toks, kids = trie.children(nd)
            for tk, c in zip(toks.tolist(), kids.tolist()):
                path[c], seq[c] = f32(path[nd] + f32(z[tk] - lse)), seq[nd] + [tk]
            for k in idx[off[nd]:off[nd + 1]].tolist():
                logprob[k] = f32(path[nd] + f32(z[eos] - lse))
    depth_of = {int(nd): t for t, lv in enumerate(levels.levels) for nd in lv.nodes.tolist()}
    lengths = np.array([depth_of[int(nd)] + 1 for nd in trie.phrase_node], dtype=np.int32)
    return SimpleNamespace(logprob=logprob, best=int(np.flatnonzero(logprob == logprob.max())[0]), lengths=lengths)


def check_phrase_score_args(phrases, eos, vocab: int, P: int, window: int, causal: bool = True, sparse: bool = False,
                            images_per_pass=None) -> PhraseTrie:
    """The refusals of ``score_phrases``, all before anything runs -> the trie.  ValueError: everything ``phrase_trie`` refuses about the
    set (or a ``PhraseTrie`` built for another EOS / vocabulary, or one without ``phrase_node``), prompt + longest phrase + 1 past
    the decode ``window`` (the text of every other call), ``images_per_pass`` < 1.  NotImplementedError, naming the reason: a
    non-causal decoder, sparse nano-mini blocks."""
    if isinstance(phrases, PhraseTrie):
        trie = phrases
        if eos is None or not 0 <= int(eos) < vocab or trie.edges < 1 or int(trie.child_tok.min()) < 0 or int(trie.child_tok.max()) >= vocab \
                or bool((trie.child_tok == int(eos)).any()):
            raise ValueError(f'a PhraseTrie built for another call: eos_token_id = {eos}, vocabulary {vocab}')
        phrase_node_csr(trie)
    else:
        trie = phrase_trie(phrases, eos, vocab, 1 << 30)
    if not causal:
        raise NotImplementedError('score_phrases walks the trie on the KV cache; a non-causal decoder has none -- every new token changes the '
                                  'state of the earlier ones --, so use rerank')
    if sparse:
        raise NotImplementedError('score_phrases on sparse nano-mini decoder blocks: a sparse layer caches the positions it keeps by slot, and '
                                  'the static per-level history tables have not been run through its slot table (slot_pos); use rerank')
    total = int(P) + trie.longest + 1
    if total > window:
        raise ValueError(f'prompt + new tokens ({total}) exceed the text window ({window})')
    if images_per_pass is not None and (isinstance(images_per_pass, bool) or int(images_per_pass) != images_per_pass or int(images_per_pass) < 1):
        raise ValueError(f'images_per_pass = {images_per_pass!r}: a whole number of images, at least 1')
    return trie


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

    def _build_captions(self, B: int, N: int, ids_ld: int, clen: Optional[int] = None):
        R = B * N
        st = self._build(R, ids_ld, mem_rows=B, clen=clen)
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        st.N, st.images = N, B
        st.mem_div = N
        st.ctrl = torch.zeros(2, **i32)                         # [done, unfinished rows]
        st.finished, st.lengths = torch.zeros(R, **i32), torch.zeros(R, **i32)
        st.tok_lp = torch.zeros(R, ids_ld, dtype=F32, device=dev)
        st.top2 = st.seg_se = None
        st.rag_prompt = st.rag_plen = None                      # prompt_lengths: int64 [B, ids_ld] / int32 [B], made at the first such call
        st.raw_lse = st.saved = st.suppress = None              # logits processors: f32 [R] / f32 [R, ids_ld] / int32 list, made at the first active call
        st.node = st.phrase_index = st.kept = st.trie = None    # phrases: int32 [R] / int32 [R] / f32 [R, fan-out + 1] / the four trie arrays (and raw_lse)
        return st

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
            st.graphs = {k: g for k, g in st.graphs.items() if not (isinstance(k, tuple) and k and k[0] == 'proc')}
        if n:
            st.suppress[:n].copy_(torch.tensor(proc.suppress, dtype=torch.int32))

    def _trie_state(self, st, trie: PhraseTrie):
        """The buffers of a phrase-constrained step, persistent because captured steps bake their pointers: st.node,
        st.phrase_index, st.raw_lse, and -- regrown only together with the graphs that hold them -- st.kept and the four trie arrays
        st.trie = (child_off, child_tok, child_next, term).  The kernels take the arrays' CAPACITIES as nodes / edges, so a captured step
        serves any trie that fits; the trie's contents are copied in per call, the spare nodes childless and ending no phrase."""
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        if st.node is None:
            st.node, st.phrase_index = torch.zeros(st.B, **i32), torch.full((st.B,), -1, **i32)
        if st.raw_lse is None:                                  # (shared with the logits processors: _processor_state)
            st.raw_lse = torch.zeros(st.B, dtype=F32, device=dev)
        if st.trie is None or st.trie[3].numel() < trie.nodes or st.trie[1].numel() < trie.edges or st.kept.shape[1] < trie.max_fanout + 1:
            nodes, edges = max(64, trie.nodes), max(64, trie.edges)
            st.trie = (torch.zeros(nodes + 1, **i32), torch.zeros(edges, **i32), torch.zeros(edges, **i32), torch.full((nodes,), -1, **i32))
            st.kept = torch.zeros(st.B, (max(64, trie.max_fanout + 1) + 3) // 4 * 4, dtype=F32, device=dev)
            st.graphs = {k: g for k, g in st.graphs.items() if not (isinstance(k, tuple) and k and k[0] == 'trie')}
        nodes, edges = st.trie[3].numel(), st.trie[1].numel()
        off = np.full(nodes + 1, trie.edges, dtype=np.int32)
        off[:trie.nodes + 1] = trie.child_off
        tok, nxt, term = np.zeros(edges, dtype=np.int32), np.zeros(edges, dtype=np.int32), np.full(nodes, -1, dtype=np.int32)
        tok[:trie.edges], nxt[:trie.edges], term[:trie.nodes] = trie.child_tok, trie.child_next, trie.term
        for buf, host in zip(st.trie, (off, tok, nxt, term)):
            buf.copy_(torch.from_numpy(host))

    def _caption_step(self, st, sampling: Optional[Sampling], top2: bool, eos: Optional[int], pad: int, forced=None, proc=None,
                      trie: bool = False):
        """The launches of a full step.  ``forced``: None, or (prompt, plen, max_new) of a ``prompt_lengths`` call -- the finish rule is
        then i2t_caption_finish_ragged; the choosers run as they are, on every row, and what they wrote at a forced column is replaced
        after them.  ``proc``: None, or (Processors, P) of a call with active logits processors (never with ``top2``):
        i2t_caption_logits_process between the GEMM and the chooser, i2t_caption_raw_logprob between the chooser and the finish rule.
        ``trie`` (a ``phrases`` call; never with ``top2``, ``forced`` or ``proc``): i2t_caption_trie_mask before the
        chooser, which then runs without n-gram sizes -- the phrase set says what may be emitted --, i2t_caption_trie_advance after it."""
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        R, d = st.B, dc.d
        len_ptr, done = st.counters[1:2], st.ctrl[0:1]
        nn = 0 if trie else st.ngrams.numel()
        self._body(st)
        self._final_norm(st)
        if top2:
            ops.gemm_top2_lse(st.hid, a.W(eng.n_head), st.top2, st.seg_se, R, dc.V, d)
            ops.top2_ngram_argmax_lp(st.top2, st.seg_se, st.hid, a.W(eng.n_head), st.ids, st.ids_ld, len_ptr, st.ngrams, nn, R, dc.V, d, done,
                                     st.tok_lp)
        else:
            ops.gemm(st.hid, a.W(eng.n_head), st.logits, R, dc.V, d, workspace=st.ws)
            if proc is not None:
                pr, P = proc
                ops.caption_logits_process(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, None if forced is None else forced[1], P, st.N,
                                           st.suppress, len(pr.suppress), eos, pr.min_new, pr.theta, pr.inv_theta, done, st.raw_lse, st.saved,
                                           R, dc.V)
            if trie:
                off, tok, nxt, term = st.trie
                ops.caption_trie_mask(st.logits, dc.Vp, st.node, off, tok, term, eos, done, st.raw_lse, st.kept, R, dc.V)
            if sampling is None:
                ops.ngram_ban_argmax_lp(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, nn, R, dc.V, done, st.tok_lp)
            else:
                ops.sample_token_lp(st.logits, dc.Vp, st.ids, st.ids_ld, len_ptr, st.ngrams, nn, R, dc.V, sampling.temperature,
                                    sampling.top_k, sampling.nucleus_p, st.seed, done, st.tok_lp)
            if proc is not None:                                # the chooser's log-prob was taken on the processed row: the raw one over it
                ops.caption_raw_logprob(st.ids, st.ids_ld, len_ptr, st.raw_lse, st.saved, st.logits, dc.Vp, done, st.tok_lp, R, dc.V)
            if trie:                                            # the row moves along the chosen edge; the raw log-prob over the chooser's
                ops.caption_trie_advance(st.ids, st.ids_ld, len_ptr, st.finished, st.logits, dc.Vp, st.raw_lse, off, tok, nxt, term, eos, done,
                                         st.node, st.phrase_index, st.tok_lp, R, dc.V)
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
                          min_new_tokens: int = 0, suppress_tokens=None, phrases=None, each=None) -> GeneratedCaptions:
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
        the result carries ``phrase_index``.  None: the call is the one without the argument.  ``each(i)`` runs after full step i (tests
        read the step's buffers there)."""
        eng = self.eng
        dc = eng.dec
        N = int(num_return_sequences)
        B, P = prompt_ids.shape
        ragged = prompt_lengths is not None
        procs = dict(repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens, vocab=dc.V)
        if ragged:
            plen = check_ragged_caption_args(prompt_lengths, B, P, N, sampling, eos, pad, poll_every, max_new_tokens, **procs)
            pmin, pmax = int(plen.min()), int(plen.max())
        else:
            check_caption_args(N, sampling, eos, pad, poll_every, max_new_tokens, **procs)
            pmin = pmax = P
        proc = caption_processors(repetition_penalty, min_new_tokens, suppress_tokens, max_new_tokens, eos, dc.V)
        trie = None
        if phrases is not None:
            trie = check_phrase_caption_args(phrases, eos, dc.V, max_new_tokens, prompt_lengths, proc is not None, 1, dc.causal)
        if not dc.causal:
            raise ValueError('CaptionDecoder needs a causal decoder')
        m, start = prefill_plan(prompt_prefill, pmin, min(eng.enc.ncls, dc.block) if dc.prefixed else 0, dc.fam, True)
        n_prefill = pmin - 1 - m
        if not max_new_tokens:              # nothing to emit: no step reads the cache, so 'pass' fills nothing -- no pass, no replay
            m = 0
        a = eng.prepare(False)
        R, total = B * N, pmax + max_new_tokens
        pad = (0 if eos is None else eos) if pad is None else pad
        st = self._state_for(R, total, lambda clen: self._build_captions(B, N, max(total, dc.block), clen), lambda st: st.N == N)
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
                return GeneratedCaptions(ids.view(B, N, pmax), len_rows.view(B, N).clone(), zero, zero.sum(dim=-1), plen_dev)
            forced = (st.rag_prompt, st.rag_plen, max_new_tokens)
        self._prepare_inputs(st, images, B, N, prefill=(prompt, m) if m else None)
        # 'pass': the first step is at slot prefix + m, column 1 + m; st.counters_init stays what 'steps' calls on this state start from
        start = torch.tensor(start, dtype=torch.int32, device=a.device) if m else st.counters_init
        if sampling is not None:
            _draw_seed(st.seed, sampling.seed)
        if proc is not None:
            self._processor_state(st, proc)
        if trie is not None:
            self._trie_state(st, trie)
        top2, head = self._greedy_head(st, sampling, logits=proc is not None or trie is not None, lse=True)
        # eos, pad and max_new_tokens are kernel arguments: a captured step holds them ('ragged': never an equal-length step's key), and
        # so are the processors' scalars ('proc': never an inactive call's key); 'trie': never a key of a call without phrases
        full_key = caption_graph_key(head, eos, pad, max_new_tokens if ragged else None, proc, pmax, trie is not None)
        prompt_rows = prompt.repeat_interleave(N, dim=0) if N > 1 else prompt

        def reset():
            st.ids.zero_()
            st.ids[:, :pmax] = prompt_rows
            st.counters.copy_(start)                            # device-to-device: no host sync in the loop
            st.ctrl.zero_()
            st.finished.zero_()
            # what a row without an EOS ends with: p_b + max_new_tokens
            st.lengths.copy_(len_rows) if ragged else st.lengths.fill_(total)
            st.tok_lp.zero_()
            if trie is not None:                                # every row at the root, no phrase named yet
                st.node.zero_()
                st.phrase_index.fill_(-1)
        # Pmin - 1 columns every row holds a prompt token in, then the longest prompt's row emits its last token in the last full step
        # ('pass': those columns' K/V are in the cache already, n_prefill = 0)
        self.last_prefill_steps = n_prefill
        self.last_replays = self._replay(st, full_key, lambda: self._caption_step(st, sampling, top2, eos, pad, forced, None if proc is None else (proc, pmax),
                                                                                  trie is not None),
                                         reset, n_prefill,
                                         pmax - pmin + max_new_tokens, use_graph, each=each, poll_every=poll_every if eos is not None else 0)
        lengths = st.lengths.clone()
        L = int(lengths.max().item()) if max_new_tokens else pmax       # the final host sync
        ids = st.ids[:, :L].reshape(B, N, L).clone()
        tok_lp = st.tok_lp[:, pmin:L].reshape(B, N, L - pmin).clone()
        return GeneratedCaptions(ids, lengths.view(B, N), tok_lp, tok_lp.sum(dim=-1), plen_dev,
                                 phrase_index=None if trie is None else st.phrase_index.view(B, N).clone())


def check_caption_args(N: int, sampling: Optional[Sampling], eos, pad, poll_every: int, max_new_tokens: int, repetition_penalty: float = 1.0,
                       min_new_tokens: int = 0, suppress_tokens=None, vocab: Optional[int] = None):
    """the refusals of generate_captions that need no device; those of the logits processors are ``caption_processors``'"""
    if N < 1:
        raise ValueError(f'num_return_sequences = {N}: at least one caption per image')
    if sampling is None and N > 1:
        raise ValueError(f'greedy decoding with num_return_sequences = {N}: the {N} rows of an image would be identical; sample instead')
    if sampling is not None and not sampling.temperature > 0:
        raise ValueError('sampling needs a positive temperature')
    if eos is not None and eos < 0:
        raise ValueError(f'eos_token_id = {eos}')
    if pad is not None and pad < 0:
        raise ValueError(f'pad_token_id = {pad}')
    if poll_every < 0 or max_new_tokens < 0:
        raise ValueError(f'poll_every = {poll_every}, max_new_tokens = {max_new_tokens}: neither may be negative')
    caption_processors(repetition_penalty, min_new_tokens, suppress_tokens, max_new_tokens, eos, vocab)


def check_ragged_caption_args(prompt_lengths, B: int, P: int, N: int, sampling: Optional[Sampling], eos, pad, poll_every: int,
                              max_new_tokens: int, **processors) -> np.ndarray:
    """check_caption_args, and the refusals of ``prompt_lengths`` (read on the host, before anything moves to the device): one integer
    per image, 1 <= p_b <= P  -> the lengths, int32 [B]"""
    check_caption_args(N, sampling, eos, pad, poll_every, max_new_tokens, **processors)
    if isinstance(prompt_lengths, torch.Tensor):
        if prompt_lengths.is_floating_point() or prompt_lengths.is_complex() or prompt_lengths.dtype == torch.bool:
            raise ValueError(f'prompt_lengths of dtype {prompt_lengths.dtype}: integers are needed')
        plen = prompt_lengths.detach().cpu().numpy()
    else:
        plen = np.asarray(prompt_lengths)
        if plen.size and not np.issubdtype(plen.dtype, np.integer):
            raise ValueError(f'prompt_lengths of type {plen.dtype}: integers are needed')
    if plen.shape != (B,):
        raise ValueError(f'prompt_lengths of shape {tuple(plen.shape)} for prompt_ids of {B} rows: one length per image, shape ({B},)')
    if B and int(plen.min()) < 1:
        raise ValueError(f'prompt_lengths[{int(plen.argmin())}] = {int(plen.min())}: every row needs at least one prompt token')
    if B and int(plen.max()) > P:
        raise ValueError(f'prompt_lengths[{int(plen.argmax())}] = {int(plen.max())} exceeds the {P} columns of prompt_ids')
    return plen.astype(np.int32)


# ------------------------------------------------------------------------------------------------ caption beams
MAX_CAPTION_BEAMS = 8               # i2t_beam_candidates takes E = 2 W <= 16
BEAM_DEAD = -1.0e9                  # the running score of beams 1 .. W - 1 before the first step (transformers' constant)


def check_beam_caption_args(num_beams, num_return_sequences, length_penalty, early_stopping, temperature=1.0, top_k=None, nucleus_p=None,
                            seed=None, prompt_lengths=None, prompt_prefill='steps', repetition_penalty=1.0, min_new_tokens=0,
                            suppress_tokens=None, max_new_tokens=1, eos=None, pad=None, poll_every=8, causal=True, vocab=None) -> int:
    """The refusals of ``generate_captions(num_beams=W, ...)`` that need no device, all before anything runs -> W.  W = 1 is the call
    without the beam arguments: only W itself, ``length_penalty`` and ``early_stopping`` are looked at.  ValueError: W outside
    1 .. MAX_CAPTION_BEAMS (the candidates kernel takes E = 2 W <= 16), N outside 1 .. W, a non-finite ``length_penalty``,
    ``early_stopping`` not False / True ("never" is out of scope), any sampling argument (beam sampling is out of scope), a negative
    id or count.  NotImplementedError, naming the reason: ``prompt_lengths``, ``prompt_prefill='pass'``, an active
    ``repetition_penalty`` / ``min_new_tokens`` / ``suppress_tokens``, a non-causal decoder."""
    if isinstance(num_beams, bool) or int(num_beams) != num_beams or not 1 <= int(num_beams) <= MAX_CAPTION_BEAMS:
        raise ValueError(f'num_beams = {num_beams!r}: a whole number from 1 to {MAX_CAPTION_BEAMS} (the candidates kernel takes 2 * num_beams '
                         f'<= 16 candidates per row)')
    W = int(num_beams)
    try:
        finite = bool(np.isfinite(float(length_penalty)))
    except (TypeError, ValueError):
        finite = False
    if not finite:
        raise ValueError(f'length_penalty = {length_penalty!r}: a finite number is needed')
    if not isinstance(early_stopping, (bool, np.bool_)):
        raise ValueError(f'early_stopping = {early_stopping!r}: False or True ("never" is not supported)')
    if W == 1:
        return W
    N = int(num_return_sequences)
    if not 1 <= N <= W:
        raise ValueError(f'num_return_sequences = {N} with num_beams = {W}: from 1 to num_beams captions per image')
    if temperature != 1 or top_k is not None or nucleus_p is not None or seed is not None:
        raise ValueError('num_beams > 1 is deterministic beam search: temperature, top_k, nucleus_p and seed must stay at their defaults '
                         '(beam sampling is not supported)')
    if (eos is not None and eos < 0) or (pad is not None and pad < 0):
        raise ValueError(f'eos_token_id = {eos}, pad_token_id = {pad}: neither may be negative')
    if poll_every < 0 or max_new_tokens < 0:
        raise ValueError(f'poll_every = {poll_every}, max_new_tokens = {max_new_tokens}: neither may be negative')
    if caption_processors(repetition_penalty, min_new_tokens, suppress_tokens, max_new_tokens, eos, vocab) is not None:
        raise NotImplementedError('repetition_penalty / min_new_tokens / suppress_tokens under num_beams > 1: the beam step has no '
                                  'logits-processor pass')
    if prompt_lengths is not None:
        raise NotImplementedError('prompt_lengths under num_beams > 1: the beam step has no forcing table for ragged prompts')
    if prompt_prefill not in PROMPT_PREFILL_MODES:
        raise ValueError(f'prompt_prefill = {prompt_prefill!r}: one of {PROMPT_PREFILL_MODES}')
    if prompt_prefill != 'steps':
        raise NotImplementedError("prompt_prefill='pass' under num_beams > 1: the beam rows are prefilled step by step under the identity "
                                  "history table")
    if not causal:
        raise NotImplementedError('num_beams > 1 needs a causal decoder: a non-causal one has no KV cache to run the beams on')
    return W


def beam_pool_select_host(cand_tok, cand_lp, scores, ids, hist, tok_lp, pool_ids, pool_lp, pool_score, pool_sum, pool_len, pool_n, closed,
                          counters, ctrl, W: int, P: int, max_new: int, eos, pad: int, length_penalty: float, early_stopping: bool,
                          gaps: Optional[list] = None, pool_gaps: Optional[list] = None):
    """One i2t_beam_pool_select call on the host (numpy, in place on the arrays given; fp32 arithmetic in the kernel's order): the
    normative statement of the selection step of ``generate_captions(num_beams=W)``, pinned to transformers 5.x
    ``GenerationMixin._beam_search`` (do_sample=False, one EOS id).  ``cand_tok`` / ``cand_lp`` [R, 2 W]: every row's 2 W best tokens and
    their log-probs; ``scores`` f32 [R]; ``ids`` int64 [R, ids_ld]; ``hist`` int32 [R, hist_ld]; ``tok_lp`` f32 [R, lp_ld]; the pool
    ``pool_ids`` [B, W, ids_ld], ``pool_lp`` [B, W, lp_ld], ``pool_score`` / ``pool_sum`` f32 [B, W], ``pool_len`` int32 [B, W], ``pool_n``
    / ``closed`` int32 [B]; ``counters`` = [pos, len], ``ctrl`` = [done, open] (``i2t_beam_advance`` moves both; ``beam_advance_host``).
    Per image that is not closed (nothing happens once ctrl[0] is set):
      * totals = scores[row] + cand_lp (fp32); the top 2 W of the W * 2 W, descending, the lower flat index w * 2 W + e first on ties;
      * emitted = len + 1 - P counts the token being added; a candidate HITS if its token is ``eos`` or emitted == max_new;
      * hits ranked below W are offered at total / fp32(emitted) ** fp32(length_penalty) (one fp32 power, one fp32 division); the pool
        keeps the W best of (pool, offers), sorted descending, an entry it holds before a new one of equal score, an earlier offer
        before a later one; a pool row is the parent's ids and log-probs, the token and its log-prob, then ``pad`` and 0.0;
      * the first W candidates that do not hit, in rank order, become the image's rows: ids, history and log-prob rows move from
        parent to child;
      * the image closes at the bound (its rows then stay as they are); with ``early_stopping`` once the pool holds W; without it
        once the pool holds W and not (best running total / fp32(emitted) ** fp32(length_penalty) > the pool's worst score) --
        ``_check_early_stop_heuristic`` with early_stopping=False: the length is cur_len - prompt length AFTER the step's increment;
      * an image left open sets ctrl[1] = 1.
    ``gaps`` (a list, optional) receives the differences between neighbours among the top 2 W totals; ``pool_gaps`` those between an
    offer and the pool entries beside it and between the close test's two sides."""
    if ctrl[0]:
        return
    pos, ln = int(counters[0]), int(counters[1])
    R = scores.shape[0]
    B, E = R // W, 2 * W
    if ln < P or ln >= P + max_new or pos < 0 or pos >= hist.shape[1]:
        return
    f32 = np.float32
    emitted = ln + 1 - P
    bound = emitted >= max_new
    with np.errstate(all='ignore'):
        denom = np.power(f32(emitted), f32(length_penalty)).astype(f32)
    for b in range(B):
        if closed[b]:
            continue
        r0 = b * W
        tot = (scores[r0:r0 + W].astype(f32)[:, None] + cand_lp[r0:r0 + W].astype(f32)).astype(f32).reshape(-1)
        order = sorted(range(W * E), key=lambda j: (-tot[j], j))[:E]
        if gaps is not None:
            gaps.extend(float(tot[order[k]]) - float(tot[order[k + 1]]) for k in range(E - 1) if np.isfinite(tot[order[k + 1]]))
        m = int(pool_n[b])
        entries = [(f32(pool_score[b, i]), i, None) for i in range(m)]          # (score, the slot it held or -1, the candidate)
        children = []
        for k, j in enumerate(order):
            w, e = divmod(j, E)
            tk, lpv = int(cand_tok[r0 + w, e]), f32(cand_lp[r0 + w, e])
            if bound or (eos is not None and eos >= 0 and tk == eos):
                if k >= W:
                    continue
                s = f32(tot[j] / denom)
                at = 0
                while at < len(entries) and entries[at][0] >= s:
                    at += 1
                if pool_gaps is not None:
                    pool_gaps.extend(abs(float(entries[i][0]) - float(s)) for i in (at - 1, at) if 0 <= i < len(entries))
                if at >= W:
                    continue
                entries.insert(at, (s, -1, (r0 + w, tk, f32(tot[j]), lpv)))
                del entries[W:]
            elif len(children) < W:
                children.append((r0 + w, tk, f32(tot[j]), lpv))
        while len(children) < W:
            children.append((r0 + len(children), int(pad), f32(-np.inf), f32(0.0)))
        if any(src < 0 for _, src, _ in entries):
            old_ids, old_lp = pool_ids[b].copy(), pool_lp[b].copy()
            old_sum, old_len = pool_sum[b].copy(), pool_len[b].copy()
            total = P + max_new
            for d, (s, src, c) in enumerate(entries):
                pool_score[b, d] = s
                if src >= 0:
                    pool_ids[b, d, :total], pool_lp[b, d, :total] = old_ids[src, :total], old_lp[src, :total]
                    pool_sum[b, d], pool_len[b, d] = old_sum[src], old_len[src]
                else:
                    par, tk, t, lpv = c
                    pool_ids[b, d, :ln], pool_lp[b, d, :ln] = ids[par, :ln], tok_lp[par, :ln]
                    pool_ids[b, d, ln], pool_lp[b, d, ln] = tk, lpv
                    pool_ids[b, d, ln + 1:total], pool_lp[b, d, ln + 1:total] = pad, 0.0
                    pool_sum[b, d], pool_len[b, d] = t, ln + 1
        m = len(entries)
        pool_n[b] = m
        cl = bool(bound)
        if not cl and m == W:
            if early_stopping:
                cl = True
            else:
                with np.errstate(all='ignore'):
                    best = f32(children[0][2] / denom)
                cl = not (best > entries[W - 1][0])
                if pool_gaps is not None and np.isfinite(best):
                    pool_gaps.append(abs(float(best) - float(entries[W - 1][0])))
        closed[b] = 1 if cl else 0
        if not cl:
            ctrl[1] = 1
        if bound:
            continue
        pars = [c[0] for c in children]
        ids[r0:r0 + W, :ln] = ids[pars, :ln]
        tok_lp[r0:r0 + W, :ln] = tok_lp[pars, :ln]
        hist[r0:r0 + W, :pos] = hist[pars, :pos]
        for w, (par, tk, t, lpv) in enumerate(children):
            ids[r0 + w, ln], tok_lp[r0 + w, ln], hist[r0 + w, pos], scores[r0 + w] = tk, lpv, par, t


def beam_advance_host(counters, ctrl):
    """i2t_beam_advance on the host: while ctrl[0] is clear pos and len advance and ctrl[0] = (ctrl[1] == 0); then ctrl[1] = 0"""
    if not ctrl[0]:
        counters[0] += 1
        counters[1] += 1
        if ctrl[1] == 0:
            ctrl[0] = 1
    ctrl[1] = 0


def banned_log_softmax_host(z, ids_row, ngram_sizes) -> np.ndarray:
    """fp32 log_softmax of one logits row after the no-repeat-n-gram ban over ``ids_row`` (-inf at a token that would complete an
    n-gram the row already holds): the quantity ``i2t_beam_candidates`` returns at temperature <= 0"""
    z = np.array(z, dtype=np.float32).reshape(-1)
    row = [int(t) for t in ids_row]
    for n in ngram_sizes:
        if n < 1 or len(row) < n:
            continue
        tail = tuple(row[len(row) - n + 1:]) if n > 1 else ()
        for i in range(len(row) - n + 1):
            if tuple(row[i:i + n - 1]) == tail and 0 <= row[i + n - 1] < z.shape[0]:
                z[row[i + n - 1]] = -np.inf
    m = z.max()
    return (z - (m + np.log(np.exp(z - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32))).astype(np.float32)


def beam_search_host(step_logits, prompt, W: int, N: int, max_new: int, eos, pad, length_penalty: float, early_stopping: bool,
                     ngram_sizes=()):
    """The whole search of ``generate_captions(num_beams=W)`` for ONE image on the host: ``step_logits(sequence)`` gives the fp32 logits
    row [V] that follows a token sequence (a list of ints, the prompt included); ``prompt`` is the image's prompt (P >= 1 ids).  Every
    step takes each running row's ``banned_log_softmax_host``, its 2 W best tokens (descending, the lower id first on ties), one
    ``beam_pool_select_host`` call and ``beam_advance_host``; running scores start at [0, BEAM_DEAD, ...].  -> SimpleNamespace(ids
    int64 [N, L], lengths int32 [N], token_logprobs f32 [N, L - P], logprob f32 [N], beam_scores f32 [N], steps, gaps, pool_gaps): the
    first N pool entries, L = lengths.max(), the pad id and 0.0 past each length; ``gaps``: per step the differences between
    neighbours among the top 2 W totals and between the 2 W-th and the next one; ``pool_gaps``: those the pool merges and the close
    tests hung on (``beam_pool_select_host``); ``decision_gaps``: per step the gap between the last total that runs on and the next one
    that does not, and -- when a hit ranks among the top 2 W -- between ranks W - 1 and W.  A search whose ``decision_gaps`` and
    ``pool_gaps`` all exceed a perturbation of the totals keeps its result under it."""
    prompt = [int(t) for t in np.asarray(prompt).reshape(-1)]
    P, E = len(prompt), 2 * W
    assert P >= 1 and 1 <= N <= W and max_new >= 1
    pad = int((0 if eos is None else eos) if pad is None else pad)
    total = P + max_new
    f32, i32 = np.float32, np.int32
    ids = np.zeros((W, total), dtype=np.int64)
    ids[:, :P] = prompt
    hist = np.repeat(np.arange(W, dtype=i32)[:, None], total, axis=1)
    tok_lp = np.zeros((W, total), dtype=f32)
    scores = np.full(W, BEAM_DEAD, dtype=f32)
    scores[0] = 0.0
    pool_ids, pool_lp = np.full((1, W, total), pad, dtype=np.int64), np.zeros((1, W, total), dtype=f32)
    pool_score, pool_sum = np.full((1, W), BEAM_DEAD, dtype=f32), np.zeros((1, W), dtype=f32)
    pool_len, pool_n, closed = np.zeros((1, W), dtype=i32), np.zeros(1, dtype=i32), np.zeros(1, dtype=i32)
    counters, ctrl = np.array([P - 1, P], dtype=i32), np.zeros(2, dtype=i32)
    gaps, pool_gaps, decision_gaps, steps = [], [], [], 0
    while steps < max_new and not ctrl[0]:
        ln = int(counters[1])
        cand_tok, cand_lp = np.zeros((W, E), dtype=i32), np.zeros((W, E), dtype=f32)
        spare, seen, tops, lps = [], {}, [], []
        for w in range(W):
            key = tuple(int(t) for t in ids[w, :ln])
            if key not in seen:
                seen[key] = banned_log_softmax_host(step_logits(list(key)), key, ngram_sizes)
            lp = seen[key]
            order = sorted(range(lp.shape[0]), key=lambda t: (-lp[t], t))[:E + 1]
            assert len(order) >= E, 'the vocabulary holds fewer than 2 W tokens'
            cand_tok[w], cand_lp[w] = order[:E], lp[order[:E]]
            tops.append(order)
            lps.append(lp)
            spare.extend(f32(scores[w] + lp[t]) for t in order[E:])
        if not closed[0]:
            # what the step's outcome hangs on: the last candidate that runs on against the next one that does not, and -- with a hit
            # in sight, or at the bound -- rank W - 1 against rank W, the line below which a hit is dropped
            every = sorted(((float(f32(scores[w] + lps[w][t])), w * (E + 1) + e, t) for w in range(W) for e, t in enumerate(tops[w])),
                           key=lambda c: (-c[0], c[1]))
            at_bound = ln + 1 - P >= max_new
            hit = [at_bound or (eos is not None and c[2] == eos) for c in every]
            live = [c[0] for c, h in zip(every, hit) if not h]
            if len(live) > W and np.isfinite(live[W]):
                decision_gaps.append(live[W - 1] - live[W])
            if any(hit[:E]) and len(every) > W and np.isfinite(every[W][0]):
                decision_gaps.append(every[W - 1][0] - every[W][0])
            tot = np.sort((scores[:, None] + cand_lp).astype(f32).reshape(-1))[::-1]
            nxt = max([float(tot[E])] + [float(v) for v in spare]) if W > 1 else max([float(v) for v in spare], default=-np.inf)
            if np.isfinite(nxt):
                gaps.append(float(tot[E - 1]) - nxt)
        beam_pool_select_host(cand_tok, cand_lp, scores, ids, hist, tok_lp, pool_ids, pool_lp, pool_score, pool_sum, pool_len, pool_n, closed,
                              counters, ctrl, W, P, max_new, eos, pad, length_penalty, early_stopping, gaps, pool_gaps)
        beam_advance_host(counters, ctrl)
        steps += 1
    assert int(pool_n[0]) >= N
    lengths = pool_len[0, :N].copy()
    L = int(lengths.max())
    lp = pool_lp[0, :N, P:L].copy()
    return SimpleNamespace(ids=pool_ids[0, :N, :L].copy(), lengths=lengths, token_logprobs=lp, logprob=lp.sum(axis=-1, dtype=f32),
                           beam_scores=pool_score[0, :N].copy(), steps=steps, gaps=gaps, pool_gaps=pool_gaps, decision_gaps=decision_gaps)


class CaptionBeamDecoder(BeamDecoder):
    """``generate_captions(num_beams=W)`` on the static KV cache: BeamDecoder's R = B * W rows, history table and
    attention kernels, under GreedyDecoder._replay with ``poll_every``.  A step is _body -> _final_norm -> fp32 lm_head ->
    i2t_beam_candidates (temperature 0, E = 2 W, no EOS rule, no crop) -> i2t_beam_pool_select -> i2t_beam_advance; the finished pool and
    the per-image closed flags live in device memory, and the result is the first N pool rows of every image.  The decoder keeps its own
    state; its graph key is ('caption_beam', ...), never 'beam'."""

    last_replays = 0                    # full-step replays the last call launched (tests, tools)

    def _build_caption_beam(self, B: int, W: int, ids_ld: int, clen: Optional[int] = None):
        spec = BeamSpec(W, 2 * W, 0.0, None, 0.0, None, 0.0, tuple(int(n) for n in self.model.config.no_repeat_n_grams))
        st = self._build_beam(B, spec, ids_ld, False, clen)
        dev = st.arena.device
        i32 = dict(dtype=torch.int32, device=dev)
        st.tok_lp = torch.zeros(B * W, ids_ld, dtype=F32, device=dev)
        st.pool_ids = torch.zeros(B, W, ids_ld, dtype=torch.long, device=dev)
        st.pool_lp = torch.zeros(B, W, ids_ld, dtype=F32, device=dev)
        st.pool_score, st.pool_sum = torch.zeros(B, W, dtype=F32, device=dev), torch.zeros(B, W, dtype=F32, device=dev)
        st.pool_len, st.pool_n, st.closed = torch.zeros(B, W, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
        st.scores_init = torch.full((B, W), BEAM_DEAD, dtype=F32, device=dev)
        st.scores_init[:, 0] = 0.0
        st.caption_beam = True
        return st

    def _caption_beam_step(self, st, P: int, max_new: int, eos, pad: int, length_penalty: float, early_stopping: bool):
        eng, a, dc, sp = self.eng, self.eng.arena, self.eng.dec, st.spec
        pos_ptr, len_ptr = st.counters[0:1], st.counters[1:2]
        self._body(st)
        self._final_norm(st)
        ops.gemm(st.hid, a.W(eng.n_head), st.logits, st.B, dc.V, dc.d, workspace=st.ws)
        ops.beam_candidates(st.logits, st.ids, len_ptr, st.ctrl, st.beam_ngrams, st.B, dc.V, sp.expansion, 0.0, None, None, 0.0, st.seed,
                            st.cand_tok, st.cand_lp, None)
        ops.beam_pool_select(st.cand_tok, st.cand_lp, st.scores, st.ids, st.hist, st.tok_lp, st.pool_ids, st.pool_lp, st.pool_score,
                             st.pool_sum, st.pool_len, st.pool_n, st.closed, pos_ptr, len_ptr, st.ctrl, st.images, st.W, P, max_new, eos, pad,
                             length_penalty, early_stopping)
        ops.beam_advance(st.counters, st.ctrl)

    @torch.no_grad()
    def generate_captions(self, images, prompt_ids: torch.Tensor, max_new_tokens: int, num_beams: int, eos: Optional[int] = None,
                          pad: Optional[int] = None, num_return_sequences: int = 1, length_penalty: float = 1.0,
                          early_stopping: bool = False, poll_every: int = 8, use_graph: bool = True, each=None) -> GeneratedCaptions:
        """``beam_search_host`` for every image of the batch, on the device -> GeneratedCaptions with ``beam_scores``.  ``each(i)`` runs
        after full step i (tests read the step's buffers there)."""
        eng = self.eng
        dc = eng.dec
        N = int(num_return_sequences)
        W = check_beam_caption_args(num_beams, N, length_penalty, early_stopping, max_new_tokens=max_new_tokens, eos=eos, pad=pad,
                                    poll_every=poll_every, causal=dc.causal)
        if W * 2 > dc.V:
            raise ValueError(f'num_beams = {W} needs 2 * num_beams candidates per row: the vocabulary holds {dc.V} tokens')
        a = eng.prepare(False)
        prompt_ids = prompt_ids.to(a.device)
        B, P = prompt_ids.shape
        R, total = B * W, P + max_new_tokens
        pad = int((0 if eos is None else eos) if pad is None else pad)
        if max_new_tokens == 0:             # nothing to emit: the prompts, N times, at score 0
            self.last_replays = 0
            zero = torch.zeros(B, N, 0, dtype=F32, device=a.device)
            return GeneratedCaptions(prompt_ids[:, None].expand(B, N, P).clone(), torch.full((B, N), P, dtype=torch.int32, device=a.device),
                                     zero, zero.sum(dim=-1), None, torch.zeros(B, N, dtype=F32, device=a.device))
        st = self._state_for(R, total, lambda clen: self._build_caption_beam(B, W, max(total, dc.block), clen),
                             lambda st: getattr(st, 'caption_beam', False) and st.W == W)
        self._prepare_inputs(st, images, B, W)
        prompt_rows = prompt_ids.repeat_interleave(W, dim=0)
        length_penalty, early_stopping = float(length_penalty), bool(early_stopping)

        def reset():
            st.ids.zero_()
            st.ids[:, :P] = prompt_rows
            st.counters.copy_(st.counters_init)
            st.hist.copy_(st.hist_init)
            st.scores.copy_(st.scores_init.view(-1))
            st.ctrl.zero_()
            st.tok_lp.zero_()
            st.pool_ids.fill_(pad)
            st.pool_lp.zero_()
            st.pool_score.fill_(BEAM_DEAD)
            st.pool_sum.zero_()
            st.pool_len.zero_()
            st.pool_n.zero_()
            st.closed.zero_()
        # P, max_new_tokens, eos, pad and the two beam arguments are kernel arguments: a captured step holds them
        key = ('caption_beam', P, max_new_tokens, -1 if eos is None else int(eos), pad, length_penalty, early_stopping)
        self.last_replays = self._replay(st, key, lambda: self._caption_beam_step(st, P, max_new_tokens, eos, pad, length_penalty,
                                                                                  early_stopping),
                                         reset, P - 1, max_new_tokens, use_graph, each=each, poll_every=poll_every, prefill_first=True)
        lengths = st.pool_len[:, :N].contiguous()
        L = int(lengths.max().item())                           # the final host sync
        tok_lp = st.pool_lp[:, :N, P:L].contiguous()
        return GeneratedCaptions(st.pool_ids[:, :N, :L].contiguous(), lengths, tok_lp, tok_lp.sum(dim=-1), None,
                                 st.pool_score[:, :N].contiguous())


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

    def _build_trie_score(self, B: int, W: int, ids_ld: int, clen: int):
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
        st.trie_score = True
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
        """the cross K/V of images ``take`` [st.images] and their soft-prompt K/V into the head of every row's cache"""
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

    def _level_step(self, st, tables, t: int, eos: int, logprob):
        eng, a, dc = self.eng, self.eng.arena, self.eng.dec
        R, V, d = st.B, dc.V, dc.d
        self._body(st)
        self._final_norm(st)
        head = a.W(eng.n_head)
        if st.lse_route:
            ops.gemm_lse(st.hid, head, st.stats, R, V, d)
            ops.lse_token_logprob(st.stats, st.hid, head, st.no_label, st.lse, st.no_lp, R, V, d, ignore_index=-100)
            z = dict(hidden=st.hid, w_head=head, d=d)
        else:
            ops.gemm(st.hid, head, st.logits, R, V, d, workspace=st.ws)
            ops.rows_lse(st.logits, dc.Vp, st.lse, R, V)
            z = dict(logits=st.logits, ld=dc.Vp)
        ops.trie_level_expand(tables, st.lse, st.path[t & 1], st.path[(t + 1) & 1], st.ids, st.ids_ld, st.counters[1:2], logprob, eos,
                              st.images, st.W, V, **z)
        ops.advance(st.counters, 1)

    @torch.no_grad()
    def score(self, images, prompt_ids: torch.Tensor, trie: PhraseTrie, eos: int, images_per_pass: Optional[int] = None) -> PhraseScores:
        """``phrase_scores_host`` for every image of the batch, on the device.  ``trie``: what ``check_phrase_score_args`` returned."""
        eng = self.eng
        dc = eng.dec
        a = eng.prepare(False)
        dev = a.device
        prompt_ids = prompt_ids.to(dev)
        B, P = prompt_ids.shape
        K = int(trie.phrase_node.shape[0])
        levels = trie_levels(trie)
        W = levels.wmax
        total = P + trie.longest + 1
        block, off, prefix, llama = self._cache_args()
        # The walk reads prompt + longest phrase + 1 cache slots however long the text window is, and W rows per image multiply every
        # slot: the state is this decoder's own, with a cache of that many slots (in whole 16s) -- or, past text_window on a decoder that
        # takes the long cache, cache_plan's whole chunks
        clen, long = cache_plan(block, off, prefix, total, llama)
        clen = clen if long else min(clen, prefix + -(-total // 16) * 16)
        ids_ld = -(-total // 8) * 8
        if images_per_pass is None:
            images_per_pass = max(1, TRIE_SCORE_BYTES // (W * self.row_bytes(clen, ids_ld)))
        Bp = min(int(images_per_pass), B)
        st = self._score_state
        if not self._reusable(st, Bp * W, total, lambda st: st.W == W and st.images == Bp and st.clen >= clen):
            self._score_state = st = None                       # the old buffers go before the new ones are made
            self._score_state = st = self._build_trie_score(Bp, W, ids_ld, clen)
        assert total <= st.tmax
        # every level's tables, checked on the host and uploaded once per call
        tables = [ops.trie_level_tables(*level_expand_tables(trie, levels, t), W, dc.V, K, dev) for t in range(trie.longest + 1)]
        anc = [torch.from_numpy(lv.anc).to(dev) for lv in levels.levels]
        first = st.prefix + P - 1                               # the cache slot of the level-0 step (TrieLevels.history)
        out = torch.zeros(B, K, dtype=F32, device=dev)
        part = torch.zeros(Bp, (K + 3) // 4 * 4, dtype=F32, device=dev)
        self.last_passes = 0
        pre = self._encode_all(st, images, B)
        for i in range(0, B, Bp):
            n = min(Bp, B - i)
            take = torch.arange(i, i + Bp, device=dev).clamp(max=B - 1)         # a short last group is filled with its last image
            self._load_group(st, pre, take)
            st.ids.zero_()
            st.ids[:, :P] = prompt_ids[take].repeat_interleave(W, dim=0)
            st.counters.copy_(st.counters_init)
            st.hist.copy_(st.hist_init)
            st.path[0].zero_()
            part.zero_()
            for _ in range(P - 1):                              # prompt tokens before the last: fill the cache only
                self._step(st, False)
            for t in range(trie.longest + 1):
                if t >= 2:                                      # the columns in which level t's table is not the identity
                    st.hist.view(Bp, W, st.clen)[:, :, first + 1:first + t] = st.row_base + anc[t][None, :, 1:t]
                self._level_step(st, tables[t], t, eos, part)
            out[i:i + n] = part[:n, :K]
            self.last_passes += 1
        top = out.max(dim=1, keepdim=True).values
        best = torch.where(out == top, torch.arange(K, device=dev)[None, :], torch.full((), K, device=dev)).min(dim=1).values
        depth = np.zeros(trie.nodes, dtype=np.int32)
        for t, lv in enumerate(levels.levels):
            depth[lv.nodes] = t
        lengths = torch.from_numpy((depth[trie.phrase_node] + 1).astype(np.int32)).to(dev)
        return PhraseScores(out, best, lengths)


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
