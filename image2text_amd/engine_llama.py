"""Llama-2 / Qwen2 decoder blocks on the HIP hot path (reference models/decoder.py:404-440 wraps transformers'
LlamaForCausalLM / Qwen2ForCausalLM -- the arithmetic followed here is transformers' modeling_llama.py / modeling_qwen2.py):

    h   = x + o_proj(attention(rope(q_proj(n1)), rope(k_proj(n1)), v_proj(n1))),     n1 = RMSNorm(x)       H query heads on Hkv K/V heads
    out = h + down_proj(silu(gate_proj(n2)) * up_proj(n2)),                           n2 = RMSNorm(h)

How it maps to the MI355X:
  * q | k | v and gate | up are ONE GEMM each: the arena lays the three (two) weight matrices next to each other (engine._arena_order),
    so the fused [N, K] operand is a view -- the persistent 256^2 MFMA kernel sees N = (H + 2 Hkv) hd and N = 2 ff;
  * the rotary embedding runs in place on the q and k columns of that GEMM's bf16 output (i2t_rope: table lookup of transformers' own
    cos / sin values, 16-byte accesses); its backward is the same kernel with the angle negated, in place on dq | dk;
  * attention = the grouped-query kernels of the nano-mini family (attention_g.hip) with Hkv > 1;
  * the residual stream stays fp32 ([M, d]); o_proj and down_proj add it in their GEMM epilogue; RMSNorm backward accumulates
    the branch gradient onto the fp32 stream gradient and emits the bf16 copy the next GEMM reads (as LayerNorm backward does);
  * no dropout (transformers' attention_dropout is 0 for these checkpoints), no gradient normaliser, no learned positions.
"""
from types import SimpleNamespace

import torch

from . import ops
from .engine_lora import LPAD, fuse_guard

BF16, F32 = torch.bfloat16, torch.float32


class LlamaBlocks:
    """Mixin of engine.HotPath (uses its arena, ``_empty``, ``dec`` namespace and parameter prefix ``dp``)."""

    def _llama_views(self, l: int):
        """One block's parameter views: the four linear sites qkv / o / gu / dn (engine_lora._site: weight, gradient and bias views,
        the LoRA adapter when one is configured -- fixed per arena, as dec.lora is -- and the decoder's fp8 switch), the norm parameters, and
        what the decode step reads"""
        key = ('llama', l, id(self.arena))
        v = self._sub_cache.get(key)
        if v is not None:
            return v
        a, ls = self.arena, self.dec.llama
        nq = ls.H * ls.hd + 2 * ls.Hkv * ls.hd
        if ls.arch == 'falcon':          # ONE fused query_key_value [q heads | k | v], ONE LayerNorm (weight + bias), a two-matrix GELU MLP
            p = f'{self.dp}backbone.transformer.h.{l}'
            nm = SimpleNamespace(qkv=[f'{p}.self_attention.query_key_value.weight'], qkv_b=[], o=f'{p}.self_attention.dense.weight',
                                 gu=[f'{p}.mlp.dense_h_to_4h.weight'], dn=f'{p}.mlp.dense_4h_to_h.weight',
                                 n1=f'{p}.input_layernorm.weight', b1=f'{p}.input_layernorm.bias', n2=None)
            n_gu = ls.ff
        else:
            p = f'{self.dp}backbone.model.layers.{l}'
            nm = SimpleNamespace(qkv=[f'{p}.self_attn.{x}_proj.weight' for x in 'qkv'],
                                 qkv_b=[f'{p}.self_attn.{x}_proj.bias' for x in 'qkv'] if ls.qkv_bias else [], o=f'{p}.self_attn.o_proj.weight',
                                 gu=[f'{p}.mlp.gate_proj.weight', f'{p}.mlp.up_proj.weight'], dn=f'{p}.mlp.down_proj.weight',
                                 n1=f'{p}.input_layernorm.weight', b1=None, n2=f'{p}.post_attention_layernorm.weight')
            n_gu = 2 * ls.ff
        site = (lambda name, N, K, bias=None: self._site(getattr(nm, name), N, K, bias, lora=self._llama_lora(l, name), switch='fp8'))
        qkv, o, gu, dn = site('qkv', nq, ls.d, nm.qkv_b), site('o', ls.d, ls.H * ls.hd), site('gu', n_gu, ls.d), site('dn', ls.d, ls.ff)
        v = self._sub_cache[key] = SimpleNamespace(
            nq=nq, qkv=qkv, o=o, gu=gu, dn=dn, Wqkv=qkv.W, bqkv=qkv.b, Wo=o.W, Wgu=gu.W, Wdn=dn.W, names=nm,
            n1=a.P(nm.n1), gn1=a.G(nm.n1), b1=a.P(nm.b1) if nm.b1 else None, gb1=a.G(nm.b1) if nm.b1 else None,
            n2=a.P(nm.n2) if nm.n2 else None, gn2=a.G(nm.n2) if nm.n2 else None)
        return v

    # ---- LoRA adapters on these blocks (reference models/utils.py:46-65 -> peft LoraModel over the transformers module; the targets of
    # training_configs/gpu/llama2-13b.yaml: q_proj, k_proj, v_proj, o_proj, up_proj, down_proj).  The fused projections keep ONE GEMM:
    # the adapters of q | k | v (gate | up) share a stacked lora_A -- u = dropout(x) [A_q; A_k; A_v]^T -- and their B matrices sit
    # block-diagonally in the K panel (engine_lora._lora_panel); everything else is engine_lora's machinery.
    _LLAMA_SITES = {'qkv': ('q', 'k', 'v'), 'o': ('o',), 'gu': ('gate', 'up'), 'dn': ('down',)}
    _FALCON_SITES = {'qkv': ('qkv',), 'o': ('o',), 'gu': ('fc',), 'dn': ('proj',)}      # query_key_value, dense, dense_h_to_4h, dense_4h_to_h

    def _llama_lora(self, l: int, site: str):
        lo = getattr(self.dec, 'lora', None)
        if lo is None or site not in lo.sites:
            return None
        key = ('llama_lora', l, site, id(self.arena))
        v = self._sub_cache.get(key)
        if v is None:
            a, ls = self.arena, self.dec.llama
            nA = f'{self.dp}lora_params.h{l}_{site}_A'
            K = a.entries[nA][2][1]
            rows = {'q': ls.H * ls.hd, 'k': ls.Hkv * ls.hd, 'v': ls.Hkv * ls.hd, 'o': ls.d, 'gate': ls.ff, 'up': ls.ff, 'down': ls.d,
                    'qkv': (ls.H + 2 * ls.Hkv) * ls.hd, 'fc': ls.ff, 'proj': ls.d}
            parts, row0, col0 = [], 0, 0
            for t in (self._FALCON_SITES if ls.arch == 'falcon' else self._LLAMA_SITES)[site]:
                nB = f'{self.dp}lora_params.h{l}_{t}_B'
                if nB in a.entries:
                    parts.append((row0, rows[t], col0, a.P(nB), a.G(nB)))
                    col0 += lo.r
                row0 += rows[t]
            names = [nA] + ([nA + '.<pad>'] if a.entries[nA][2][0] < LPAD else [])
            v = self._sub_cache[key] = SimpleNamespace(K=K, N=row0, r=lo.r, scale=lo.scale, kind=f'lora_{site}', A=a.span('W', names, (LPAD, K)),
                                                       GA=a.span('G', names, (LPAD, K)), parts=parts, nA=nA)
        return v

    # ---- the fused producers of a site's input row (csrc/fp8.hip): a frozen projection on fp8 operands takes the e4m3 row straight from
    # the row kernel -- no bf16 copy is written and no quantisation pass reads it, unless an adapter wants the bf16 row beside it
    # (engine_lora._operand_rows / linear_path).  -> (bf16 row or None, (e4m3 row, scale) or None)
    def _rmsnorm_rows(self, s, x, w, rstd, M: int, d: int, ff: int):
        y, yq = self._operand_rows(s, M, d, fuse_guard(self.fp8_fuse, d, ff))
        if yq is None:
            ops.rmsnorm_fwd(x, w, y, rstd, M, d, self.dec.llama.eps)
        else:
            ops.rmsnorm_fwd_fp8(x, w, yq[0], yq[1], rstd, M, d, self.dec.llama.eps, y_bf16=y)
        return y, yq

    def _swiglu_rows(self, s, gu, M: int, d: int, ff: int):
        h, hq = self._operand_rows(s, M, ff, fuse_guard(self.fp8_fuse, d, ff))
        if hq is None:
            ops.swiglu_fwd(gu, h, M, ff)
        else:
            ops.swiglu_fwd_fp8(gu, hq[0], hq[1], M, ff, h_bf16=h)
        return h, hq

    def _swiglu_bwd_rows(self, s, dh, gu, M: int, ff: int):
        dgu, dguq = self._operand_rows(s, M, 2 * ff, fuse_guard(self.fp8_fuse, ff=ff))
        if dguq is None:
            ops.swiglu_bwd(dh, gu, dgu, M, ff)
        else:
            ops.swiglu_bwd_fp8(dh, gu, dguq[0], dguq[1], M, ff, dgu_bf16=dgu)      # [d gate | d up] straight to the e4m3 operand of dx = d(gu) . W
        return dgu, dguq

    def rope_table(self):
        """fp32 [block, hd] = [cos | sin] per position, taken from the checkpoint's own rotary module (models/decoder.py)"""
        key = ('rope', str(self.arena.device))
        t = self._sub_cache.get(key)
        if t is None:
            t = self._sub_cache[key] = self.model.decoder.rope_table(self.dec.block).to(device=self.arena.device, dtype=F32).contiguous()
        return t

    # ------------------------------------------------------------------------------------------------ one block
    def llama_block_fwd(self, l: int, x, B: int, T: int, pos_offset: int, save: bool, vl=None):
        """vl: packed variable-length rows (cu, pos, total) -- x is [total, d], T the longest sequence"""
        ls, v = self.dec.llama, self._llama_views(l)
        M, d, H, G, hd, ff = (vl.total if vl is not None else B * T), ls.d, ls.H, ls.Hkv, ls.hd, ls.ff
        cu, rpos = (vl.cu, vl.pos) if vl is not None else (None, None)
        v3 = (lambda t, w: t) if vl is not None else (lambda t, w: t.view(B, T, w))
        cs = self.rope_table()
        plan = self.dec_drop if save else None
        drop = {site: plan.get(l, f'lora_{site}') if plan is not None else None for site in ('qkv', 'o', 'gu', 'dn')}
        svlo = {}
        r1 = self._empty(M)
        qkv = self._empty(M, v.nq, dtype=BF16)
        n1, n1q = self._rmsnorm_rows(v.qkv, x, v.n1, r1, M, d, ff)
        svlo['qkv'] = self._site_fwd(v.qkv, n1, qkv, M, drop['qkv'], save, xq=n1q)
        ops.rope(qkv, v.nq, 0, H + G, hd, cs, M, pos=rpos, pos_offset=pos_offset, T=T)      # q heads and k heads are adjacent columns
        q3 = v3(qkv, v.nq)
        ao, lse = self._empty(M, H * hd, dtype=BF16), self._empty(H * M)
        ops.gq_attention_fwd(q3[..., :H * hd], q3[..., H * hd:(H + G) * hd], q3[..., (H + G) * hd:], v3(ao, H * hd), lse,
                             B, H, G, hd, T, T, True, cu_q=cu, cu_k=cu, total_q=M)
        x1 = self._empty(M, d)
        svlo['o'] = self._site_fwd(v.o, ao, x1, M, drop['o'], save, residual=x)
        r2 = self._empty(M)
        gu = self._empty(M, 2 * ff, dtype=BF16)
        n2, n2q = self._rmsnorm_rows(v.gu, x1, v.n2, r2, M, d, ff)
        svlo['gu'] = self._site_fwd(v.gu, n2, gu, M, drop['gu'], save, xq=n2q)
        x2 = self._empty(M, d)
        h, hq = self._swiglu_rows(v.dn, gu, M, d, ff)
        svlo['dn'] = self._site_fwd(v.dn, h, x2, M, drop['dn'], save, residual=x1, xq=hq)
        return x2, (SimpleNamespace(x=x, n1=n1, r1=r1, qkv=qkv, ao=ao, lse=lse, x1=x1, n2=n2, r2=r2, gu=gu, h=h,
                                    lo={k: r for k, r in svlo.items() if r is not None}, lo_drop=drop) if save else None)

    def llama_block_bwd(self, l: int, sv, dx, dxb, B: int, T: int, pos_offset: int, vl=None):
        """dx fp32 / dxb bf16: gradient w.r.t. the block output; on return both hold the gradient w.r.t. the block input"""
        ls, v = self.dec.llama, self._llama_views(l)
        M, d, H, G, hd, ff = (vl.total if vl is not None else B * T), ls.d, ls.H, ls.Hkv, ls.hd, ls.ff
        cu, rpos = (vl.cu, vl.pos) if vl is not None else (None, None)
        v3 = (lambda t, w: t) if vl is not None else (lambda t, w: t.view(B, T, w))
        # (frozen parameters -- prepare_for_kbit_training, models/decoder.py: their gradient GEMMs are skipped, the input gradient is not;
        # an adapted site returns its fp32 dx -- engine_lora._site_bwd -- which rmsnorm_bwd takes as it is)
        tr, nm, svlo, drop = self.arena.trainable, v.names, sv.lo, sv.lo_drop
        # ---- MLP
        dh = self._empty(M, ff, dtype=BF16)
        dh32 = self._site_bwd(v.dn, svlo.get('dn'), dxb, sv.h, M, drop['dn'], dx_out=dh)
        if dh32 is not dh:
            ops.cast_f32_bf16(dh32, dh)
        dn = self._empty(M, d, dtype=BF16)
        dgu, dguq = self._swiglu_bwd_rows(v.gu, dh, sv.gu, M, ff)
        dn2 = self._site_bwd(v.gu, svlo.get('gu'), dgu, sv.n2, M, drop['gu'], dq=dguq, dx_out=dn)
        ops.rmsnorm_bwd(dn2, sv.x1, v.n2, sv.r2, dx, v.gn2 if tr(nm.n2) else None, M, d, dx_accumulate=True, dx_bf16=dxb)
        # ---- attention
        dao = self._empty(M, H * hd, dtype=BF16)
        dao32 = self._site_bwd(v.o, svlo.get('o'), dxb, sv.ao, M, drop['o'], dx_out=dao)
        if dao32 is not dao:
            ops.cast_f32_bf16(dao32, dao)
        dqkv = self._empty(M, v.nq, dtype=BF16)
        q3, g3 = v3(sv.qkv, v.nq), v3(dqkv, v.nq)
        sl = (slice(0, H * hd), slice(H * hd, (H + G) * hd), slice((H + G) * hd, v.nq))
        ops.gq_attention_bwd(q3[..., sl[0]], q3[..., sl[1]], q3[..., sl[2]], v3(sv.ao, H * hd), v3(dao, H * hd), sv.lse,
                             self._empty(H * M), g3[..., sl[0]], g3[..., sl[1]], g3[..., sl[2]], B, H, G, hd, T, T, True,
                             cu_q=cu, cu_k=cu, total_q=M)
        ops.rope(dqkv, v.nq, 0, H + G, hd, self.rope_table(), M, pos=rpos, pos_offset=pos_offset, T=T, inverse=True)
        dn1 = self._site_bwd(v.qkv, svlo.get('qkv'), dqkv, sv.n1, M, drop['qkv'], dx_out=dn)
        ops.rmsnorm_bwd(dn1, sv.x, v.n1, sv.r1, dx, v.gn1 if tr(nm.n1) else None, M, d, dx_accumulate=True, dx_bf16=dxb)

    # ------------------------------------------------------------------------------------------------ one Falcon block
    # transformers' FalconDecoderLayer with parallel_attn (falcon-7b):  n = LN(x);  y = x + dense(attn(rope(qkv(n)))) + W2 gelu(W1 n)
    def falcon_block_fwd(self, l: int, x, B: int, T: int, pos_offset: int, save: bool, vl=None):
        ls, v = self.dec.llama, self._llama_views(l)
        M, d, H, G, hd, ff = (vl.total if vl is not None else B * T), ls.d, ls.H, ls.Hkv, ls.hd, ls.ff
        cu, rpos = (vl.cu, vl.pos) if vl is not None else (None, None)
        v3 = (lambda t, w: t) if vl is not None else (lambda t, w: t.view(B, T, w))
        n1, m1, r1 = self._empty(M, d, dtype=BF16), self._empty(M), self._empty(M)
        ops.layernorm_fwd(x, v.n1, v.b1, n1, m1, r1, M, d, eps=ls.eps)
        plan = self.dec_drop if save else None
        drop = {site: plan.get(l, f'lora_{site}') if plan is not None else None for site in ('qkv', 'o', 'gu', 'dn')}
        svlo = {}
        qkv = self._empty(M, v.nq, dtype=BF16)
        svlo['qkv'] = self._site_fwd(v.qkv, n1, qkv, M, drop['qkv'], save)
        ops.rope(qkv, v.nq, 0, H + G, hd, self.rope_table(), M, pos=rpos, pos_offset=pos_offset, T=T)
        q3 = v3(qkv, v.nq)
        ao, lse = self._empty(M, H * hd, dtype=BF16), self._empty(H * M)
        ops.gq_attention_fwd(q3[..., :H * hd], q3[..., H * hd:(H + G) * hd], q3[..., (H + G) * hd:], v3(ao, H * hd), lse,
                             B, H, G, hd, T, T, True, cu_q=cu, cu_k=cu, total_q=M)
        x1 = self._empty(M, d)
        svlo['o'] = self._site_fwd(v.o, ao, x1, M, drop['o'], save, residual=x)
        h, pre = self._empty(M, ff, dtype=BF16), (self._empty(M, ff, dtype=BF16) if save else None)
        svlo['gu'] = self._site_fwd(v.gu, n1, h, M, drop['gu'], save, act=ops.ACT_GELU_ERF, aux_out=pre)
        x2 = self._empty(M, d)
        svlo['dn'] = self._site_fwd(v.dn, h, x2, M, drop['dn'], save, residual=x1)
        return x2, (SimpleNamespace(x=x, n1=n1, m1=m1, r1=r1, qkv=qkv, ao=ao, lse=lse, h=h, pre=pre,
                                    lo={k: r for k, r in svlo.items() if r is not None}, lo_drop=drop) if save else None)

    def falcon_block_bwd(self, l: int, sv, dx, dxb, B: int, T: int, pos_offset: int, vl=None):
        """dx fp32 / dxb bf16: gradient w.r.t. the block output; on return both hold the gradient w.r.t. the block input"""
        ls, v = self.dec.llama, self._llama_views(l)
        M, d, H, G, hd, ff = (vl.total if vl is not None else B * T), ls.d, ls.H, ls.Hkv, ls.hd, ls.ff
        cu, rpos = (vl.cu, vl.pos) if vl is not None else (None, None)
        v3 = (lambda t, w: t) if vl is not None else (lambda t, w: t.view(B, T, w))
        tr, nm, svlo, drop = self.arena.trainable, v.names, sv.lo, sv.lo_drop
        # ---- MLP branch: dn1 (fp32) = (dy W2 * gelu'(pre)) W1
        dpre = self._empty(M, ff, dtype=BF16)
        self._site_bwd(v.dn, svlo.get('dn'), dxb, sv.h, M, drop['dn'], dx_out=dpre, act=ops.ACT_DGELU_ERF, aux_in=sv.pre)
        dn1 = self._site_bwd(v.gu, svlo.get('gu'), dpre, sv.n1, M, drop['gu'], dx_out=self._empty(M, d) if v.gu.lora is None else None)
        # ---- attention branch: both branches read the same LayerNorm output, their input gradients add up in dn1
        dao = self._empty(M, H * hd, dtype=BF16)
        dao32 = self._site_bwd(v.o, svlo.get('o'), dxb, sv.ao, M, drop['o'], dx_out=dao)
        if dao32 is not dao:
            ops.cast_f32_bf16(dao32, dao)
        dqkv = self._empty(M, v.nq, dtype=BF16)
        q3, g3 = v3(sv.qkv, v.nq), v3(dqkv, v.nq)
        sl = (slice(0, H * hd), slice(H * hd, (H + G) * hd), slice((H + G) * hd, v.nq))
        ops.gq_attention_bwd(q3[..., sl[0]], q3[..., sl[1]], q3[..., sl[2]], v3(sv.ao, H * hd), v3(dao, H * hd), sv.lse,
                             self._empty(H * M), g3[..., sl[0]], g3[..., sl[1]], g3[..., sl[2]], B, H, G, hd, T, T, True,
                             cu_q=cu, cu_k=cu, total_q=M)
        ops.rope(dqkv, v.nq, 0, H + G, hd, self.rope_table(), M, pos=rpos, pos_offset=pos_offset, T=T, inverse=True)
        dq32 = self._site_bwd(v.qkv, svlo.get('qkv'), dqkv, sv.n1, M, drop['qkv'], dx_out=dn1, residual=dn1)
        if dq32 is not dn1:
            dn1.add_(dq32)
        ops.layernorm_bwd(dn1, sv.x, v.n1, sv.m1, sv.r1, dx, v.gn1 if tr(nm.n1) else None, v.gb1 if tr(nm.b1) else None, M, d,
                          dx_accumulate=True, dx_bf16=dxb)

    # ------------------------------------------------------------------------------------------------ the decoder stack
    def llama_decode_fwd(self, B: int, T: int, save: bool, ids, embeds, pos_offset: int, vl):
        """decode_segment for these decoders: (hidden fp32 [M, d] after the final norm, its bf16 copy, ctx)"""
        a, dc, ls = self.arena, self.dec, self.dec.llama
        d, M = dc.d, (vl.total if vl is not None else B * T)
        if ids is not None:
            ids = ids.to(device=a.device, dtype=torch.long).contiguous()
            x = self._empty(M, d)
            if vl is not None:
                ops.embed_fwd(ids, a.P(self.n_wte), None, x, M, 1, d, 0, dc.V)
            else:
                ops.embed_fwd(ids, a.P(self.n_wte), None, x, B, T, d, 0, dc.V)
        else:
            x = embeds.to(device=a.device, dtype=F32).contiguous().view(M, d)
        saves, cur = [], x
        block = self.falcon_block_fwd if ls.arch == 'falcon' else self.llama_block_fwd
        sink = getattr(self, '_layer_sink', None)         # generation's prompt prefill: takes a layer's K / V and lets the rest go
        for l in range(dc.L):
            cur, sv = block(l, cur, B, T, pos_offset, save, vl)
            if sink is not None and sv is not None:
                sink(l, sv)
                sv = None
            saves.append(sv)
        wn = self.dp + ls.norm_f
        hid, hb, rf, mf = self._empty(M, d), self._empty(M, d, dtype=BF16), self._empty(M), None
        if ls.arch == 'falcon':          # ln_f: a LayerNorm; the fp32 output is what forward() returns, the bf16 copy feeds the head
            mf = self._empty(M)
            ops.layernorm_fwd(cur, a.P(wn + '.weight'), a.P(wn + '.bias'), hid, mf, rf, M, d, eps=ls.eps)
            ops.cast_f32_bf16(hid, hb)
        else:
            ops.rmsnorm_fwd(cur, a.P(wn + '.weight'), hb, rf, M, d, ls.eps, y_f32=hid)
        ctx = SimpleNamespace(ids=ids, saves=saves, xl=cur, rf=rf, mf=mf, hb=hb, B=B, T=T, S=0, pos_offset=pos_offset, vl=vl, M=M,
                              emb_drop=None, pos_ctx=None) if save else None
        return hid, hb, ctx

    def llama_decode_bwd(self, ctx, dh):
        """dh fp32 [M, d]: gradient w.r.t. the final norm's output.  Returns the gradient w.r.t. the block stack's input."""
        a, dc = self.arena, self.dec
        M, d = ctx.M, dc.d
        dx, dxb = self._empty(M, d), self._empty(M, d, dtype=BF16)
        ls = dc.llama
        wn = self.dp + ls.norm_f
        if ls.arch == 'falcon':
            ops.layernorm_bwd(dh, ctx.xl, a.P(wn + '.weight'), ctx.mf, ctx.rf, dx, a.Gt(wn + '.weight'), a.Gt(wn + '.bias'), M, d, dx_bf16=dxb)
        else:
            ops.rmsnorm_bwd(dh, ctx.xl, a.P(wn + '.weight'), ctx.rf, dx, a.Gt(wn + '.weight'), M, d, dx_bf16=dxb)
        block = self.falcon_block_bwd if ls.arch == 'falcon' else self.llama_block_bwd
        for l in reversed(range(dc.L)):
            block(l, ctx.saves[l], dx, dxb, ctx.B, ctx.T, ctx.pos_offset, ctx.vl)
        return dx
