"""LoRA adapters on the HIP hot path (reference models/utils.py:46-65 wraps the decoder in peft's LoraModel:
every targeted linear computes ``y = base(x) + lora_B(lora_A(dropout(x))) * lora_alpha / r``, the base parameters are frozen).

How it maps to the MI355X (dense GPT-2 blocks, engine.block_fwd / block_bwd):
  * forward: the adapter rides in the K panel of the layer's own GEMM --  ``[x | u] . [W | s B | 0]^T`` with ``u = dropout(x) . A^T`` --
    so the layer's fused epilogue (bias, GELU + saved pre-activation, residual + dropout) sees base + adapter as ONE accumulator and
    nothing is added afterwards.  The rank is padded to LPAD = 128 columns (zero rows behind lora_A in the arena, zero columns behind
    s B): K + 128 keeps the 256^2 persistent kernel's K % 128 rule, and u = x . A_pad^T is itself a plain GEMM (N = 128);
  * backward: the frozen base weight's dW GEMM -- a third of a layer's GEMM flops -- is skipped (ParamArena.trainable); the adapter
    costs four thin GEMMs: dB = s . dY^T u (N = 128), du = dY . (s B) (N = 128), dA = du^T dropout(x) (M = 128), and
    dx = dY . W + dropout(du . A) (K = 128, the adapter's input dropout applied by the GEMM's residual + dropout epilogue);
  * generation (no dropout): merged weights W + s B A in persistent bf16 buffers, refreshed per generate() call -- the decode graph
    runs the un-adapted step.
"""
from types import SimpleNamespace

import torch

from . import ops

BF16, F32 = torch.bfloat16, torch.float32
LPAD = 128


def _f8pad(k: int) -> int:
    return (k + 255) // 256 * 256


def fuse_guard(fp8_fuse: bool, d: int = 0, ff: int = 0) -> bool:
    """May a row producer emit the e4m3 operand itself?  The fused row kernels (csrc/fp8.hip) keep a whole row in registers: model width
    up to 8192, MLP width up to 12288 (pass the widths the producer at hand works on)."""
    return bool(fp8_fuse) and d <= 8192 and ff <= 12288


def linear_path(adapter: bool, trainable: bool, switch, fp8: bool, fp8_vit: bool, fuse: bool = False):
    """How one linear runs -- THE place where that is decided (no tensors: tests/test_host_cpu.py enumerates it).
    adapter: a LoRA adapter rides on the site; trainable: any of its base weights takes gradient steps; switch: which engine switch
    governs the site ('fp8': decoder, 'fp8_vit': ViT backbone, None: never e4m3) and the switches' values; fuse: the producer of the
    input row may emit the e4m3 operand itself (``fuse_guard``).
    -> (path: 'bf16' | 'fp8' | 'lora' | 'lora_fp8',  producer form: 'bf16' | 'e4m3' | 'both' rows)"""
    e4m3 = not trainable and {'fp8': fp8, 'fp8_vit': fp8_vit, None: False}[switch]      # a frozen matrix has no dW: both its GEMMs can take e4m3
    path = ('lora_fp8' if e4m3 else 'lora') if adapter else ('fp8' if e4m3 else 'bf16')
    return path, ('bf16' if not (e4m3 and fuse) else 'both' if adapter else 'e4m3')      # (the adapter's u = dropout(x) A^T reads the bf16 row)


class LoraAdapters:
    """Mixin of engine.HotPath: the linear sites (plain / frozen-on-e4m3 / LoRA-adapted: ``_site`` + ``_site_fwd`` / ``_site_bwd``
    own the choice between the three) and the adapters' machinery."""

    def _site(self, names, N: int, K: int, bias=None, lora=None, switch=None, rows=None):
        """The cached record of one linear y = x W^T (+ b), W [N, K]: names = its arena entry (several ADJACENT entries: a fused
        projection); bias likewise or None; rows = (r0, r1): a row block of the entry; lora: the adapter's spec or None; switch: see
        ``linear_path``.  The policy (switch, adapter) is part of the record's identity: a caller never gets a record another caller
        made with another policy for the same weight (``engine._linear_bwd``'s plain sites beside the ViT backbone's fp8_vit ones).  The
        adapter spec is fixed per arena (``dec.lora`` is set once, in HotPath.__init__)."""
        key = ('site', names if isinstance(names, str) else tuple(names), rows, switch, None if lora is None else lora.nA, id(self.arena))
        s = self._sub_cache.get(key)          # (the hit is on the host path of every step: nothing is normalised before it)
        if s is not None:
            assert s.N == N and s.K == K and s.lora is lora, (names, (s.N, s.K), (N, K))
        else:
            a = self.arena
            names, bias = ((names,) if isinstance(names, str) else tuple(names)), ((bias,) if isinstance(bias, str) else tuple(bias or ()))
            bias = bias if bias and bias[0] in a.entries else ()
            view = (lambda kind, nn, shape: None if not nn else getattr(a, kind)(nn[0]) if len(nn) == 1 else a.span(kind, list(nn), shape))
            W, G, b, gb = view('W', names, (N, K)), view('G', names, (N, K)), view('P', bias, (N,)), view('G', bias, (N,))
            if rows is not None:
                W, G, b, gb = (t if t is None else t[rows[0]:rows[1]] for t in (W, G, b, gb))
            s = self._sub_cache[key] = SimpleNamespace(names=names, bnames=bias, W=W, G=G, b=b, gb=gb, N=N, K=K, lora=lora, switch=switch)
        return s

    def _site_path(self, s, fuse: bool = False):
        return linear_path(s.lora is not None, any(self.arena.trainable(n) for n in s.names), s.switch, self.fp8, self.fp8_vit, fuse)

    def _site_e4m3(self, s) -> bool:
        """Does this call run the site's base product on e4m3 operands?  (once per forward / backward helper call)"""
        if s.switch is None:
            return False
        on = 'fp8' in self._site_path(s)[0]
        if not on and getattr(self, s.switch):
            # a weight that trains (again): the optimizer writes it through the arena without moving its version counter, so an e4m3 image
            # kept from an earlier frozen phase would be stale if the weight is frozen once more
            self._sub_cache.pop(('fp8w', s.names, id(self.arena)), None)
        return on

    # ---- fp8 operands for FROZEN weights (I2T_FP8=1 / I2T_FP8_VIT=1; csrc/fp8.hip, BASELINE.json configs[4]): a frozen matrix has no dW,
    # so both GEMMs that touch it -- y = x W^T and dx = dy W -- run on the block-scaled e4m3 MFMA; W is quantised once per parameter
    # version in both orientations (per-output-row scales for the forward, per-input-row scales for the backward), activations per call
    def _fp8_weight(self, s):
        key = ('fp8w', s.names, id(self.arena))
        ent = self._sub_cache.get(key)
        # a frozen parameter is skipped by the fused optimizers (arena.generation moves every step, these values do not): the image
        # is rebuilt only when torch-side code wrote the parameter (load_state_dict, a manual edit -> its version counter moves)
        version = tuple(self.arena.params[n]._version for n in s.names)
        if ent is None or ent.generation != version:
            self.arena.refresh_shadow()
            N, K, dev = s.N, s.K, s.W.device
            # rows zero-padded to a multiple of 256 bytes: the GEMM then runs K' = the padded length (zeros contribute nothing) and every
            # projection is eligible for the persistent fp8 kernel (K % 256 == 0; Falcon-7B: 4544 -> 4608)
            ent = SimpleNamespace(generation=version,
                                  w8=torch.empty(N, _f8pad(K), dtype=torch.uint8, device=dev), sw=torch.empty(N, dtype=F32, device=dev),
                                  wt8=torch.empty(K, _f8pad(N), dtype=torch.uint8, device=dev), swt=torch.empty(K, dtype=F32, device=dev))
            ops.quant_rows_fp8(s.W, ent.w8, ent.sw, N, K)
            ops.quant_cols_fp8(s.W, ent.wt8, ent.swt, N, K)
            self._sub_cache[key] = ent
        return ent

    def _fp8_rows(self, x_bf, M: int, K: int):
        x8 = torch.empty(M, _f8pad(K), dtype=torch.uint8, device=x_bf.device)
        sx = self._empty(M)
        ops.quant_rows_fp8(x_bf, x8, sx, M, K)
        return x8, sx

    def _operand_rows(self, s, M: int, n: int, fuse: bool):
        """Buffers for the row a fused producer (RMSNorm, SwiGLU forward / backward: engine_llama) hands to site ``s``: (bf16 [M, n] or
        None, (e4m3 [M, pad n], scale [M]) or None) -- the e4m3 row when the site takes fp8 operands, the bf16 one unless nothing reads it"""
        form = self._site_path(s, fuse)[1]
        row = self._empty(M, n, dtype=BF16) if form != 'e4m3' else None
        return row, ((torch.empty(M, _f8pad(n), dtype=torch.uint8, device=self.arena.device), self._empty(M)) if form != 'bf16' else None)

    def _site_fwd(self, s, x_bf, out, M: int, drop_l=None, save: bool = False, xq=None, **ep):
        """out = epilogue(x W^T (+ b)) on the site's path.  xq = (x8, scale): the producer already emitted the e4m3 operand (x_bf may
        then be None on the plain fp8 path); drop_l: the adapter's input-dropout entry; ep: ops.gemm's epilogue keywords -- ``aux_out``
        (even None) asks for the pre-activation beside ``act``, which the fp8 classes cannot write: product -> pre-activation, one more
        pass applies the GELU.  Returns the adapter's save record (``_lora_bwd`` takes it) or None."""
        e4m3 = self._site_e4m3(s)
        if s.lora is not None:
            return (self._lora_gemm_fp8 if e4m3 else self._lora_gemm)(s, x_bf, out, M, drop_l, save, xq=xq, bias=s.b, **ep)
        if not e4m3:
            ops.gemm(x_bf, s.W, out, M, s.N, s.K, bias=s.b, **ep)
            return None
        e = self._fp8_weight(s)
        x8, sx = xq if xq is not None else self._fp8_rows(x_bf, M, s.K)
        if 'aux_out' in ep:
            act, pre = ep.pop('act'), ep.pop('aux_out')
            tgt = pre if pre is not None else out
            ops.gemm_fp8(x8, sx, e.w8, e.sw, tgt, M, s.N, _f8pad(s.K), bias=s.b, **ep)
            ops.gelu_fwd(tgt, out, erf=(act == ops.ACT_GELU_ERF))
        else:
            ops.gemm_fp8(x8, sx, e.w8, e.sw, out, M, s.N, _f8pad(s.K), bias=s.b, **ep)
        return None

    def _site_bwd(self, s, sv_l, dY, x_bf, M: int, drop_l=None, dq=None, dx_out=None, dy_sumsq=None, act=0, aux_in=None, **dx_kw):
        """Backward of ``_site_fwd``: dY bf16 [M, N] (dq = (dy8, scale): its e4m3 image from a fused producer), x_bf the saved input,
        sv_l the adapter's save record.  Accumulates db / dW (trainable ones only) and the adapter's gradients, then dx [M, K] = dY . W:
        the plain and fp8 paths fill ``dx_out`` (dx_kw: the dx GEMM's keywords, e.g. residual / accumulate) and return it, the LoRA path
        returns its own fp32 tensor.  act / aux_in: the activation derivative behind dx (the bf16 GEMM's epilogue; one more pass over the
        fp32 dx on the other paths) -- dx_out then holds the result on every path.
        dy_sumsq (1-float device tensor): dY is an UN-normalised gradient whose normaliser 1 / (sqrt(dy_sumsq) + 1e-6) the three
        consumers apply themselves (ops.gemm alpha_sumsq): no pass over dY exists just to rescale it."""
        a, N, K = self.arena, s.N, s.K
        gW = s.G if all(a.trainable(n) for n in s.names) else None
        gb = s.gb if s.gb is not None and all(a.trainable(n) for n in s.bnames) else None
        e4m3 = self._site_e4m3(s)
        if s.lora is not None:
            assert act in (0, ops.ACT_DGELU, ops.ACT_DGELU_ERF), act
            dx32 = self._lora_bwd(s, sv_l, dY, x_bf, gW, gb, M, drop_l, e4m3, dq)
        else:
            if gW is not None:          # (db rides on the dW launch: dY is not read a third time just to sum its columns)
                ops.gemm(dY, x_bf, gW, N, K, M, a_kmajor=True, b_kmajor=True, accumulate=True, alpha_sumsq=dy_sumsq, colsum_out=gb)
            elif gb is not None:
                ops.colsum(dY, gb, M, N, accumulate=True, alpha_sumsq=dy_sumsq)
            if dx_out is None:
                return None
            if not e4m3:
                return ops.gemm(dY, s.W, dx_out, M, K, N, b_kmajor=True, alpha_sumsq=dy_sumsq, act=act, aux_in=aux_in, **dx_kw)
            assert act in (0, ops.ACT_DGELU, ops.ACT_DGELU_ERF), act          # (a GELU derivative is the only epilogue restated below)
            dx32 = self._empty(M, K) if act else dx_out
            e = self._fp8_weight(s)
            d8, sd = dq if dq is not None else self._fp8_rows(dY, M, N)
            ops.gemm_fp8(d8, sd, e.wt8, e.swt, dx32, M, K, _f8pad(N), **dx_kw)
        return ops.dgelu_mul(dx32, aux_in, dx_out, erf=(act == ops.ACT_DGELU_ERF)) if act else dx32

    def _lora_site(self, l: int, site: str):
        lo = getattr(self.dec, 'lora', None)
        if lo is None or site not in lo.sites:
            return None
        key = ('lora', l, site, id(self.arena))
        v = self._sub_cache.get(key)
        if v is None:
            a = self.arena
            nA, nB = f'{self.dp}lora_params.h{l}_{site}_A', f'{self.dp}lora_params.h{l}_{site}_B'
            K, N = a.entries[nA][2][1], a.entries[nB][2][0]
            names = [nA] + ([nA + '.<pad>'] if lo.r < LPAD else [])
            v = self._sub_cache[key] = SimpleNamespace(
                K=K, N=N, r=lo.r, scale=lo.scale, kind=f'lora_{site}', A=a.span('W', names, (LPAD, K)), GA=a.span('G', names, (LPAD, K)),
                B=a.P(nB), GB=a.G(nB), parts=[(0, N, 0, a.P(nB), a.G(nB))], nA=nA)
        return v

    def _rank_gemm(self, a, b, out, M: int, K: int, b_kmajor: bool = False):
        """out bf16 [M, LPAD] = a [M, K] . b (b: [LPAD, K], or [K, LPAD] when b_kmajor) -- the adapters' u = dropout(x) A^T and
        du = dY (s B).  128 output columns are M / 256 half-empty tiles of the persistent kernel (12 820 rows: 51 workgroups, 1.4 TB/s);
        for a long K the fp32 split-K form (atomics into a zeroed plane, ~4 slices) + one cast runs 2.2x faster (tools/ab_thin_gemm.py)."""
        if K < 2048 or M < 2048:
            return ops.gemm(a, b, out, M, LPAD, K, b_kmajor=b_kmajor)
        plane = torch.zeros(M, LPAD, dtype=F32, device=out.device)
        ops.gemm(a, b, plane, M, LPAD, K, b_kmajor=b_kmajor, accumulate=True)
        return ops.cast_f32_bf16(plane, out)

    def _lora_panel(self, ls, dtype=BF16):
        """[N, LPAD] = the adapter's B matrices at their (row block, rank column block) -- ONE block for a plain linear, block-diagonal for
        a fused projection (q | k | v, gate | up: engine_llama) -- times the LoRA scale, zero elsewhere."""
        dev = ls.A.device
        panel = torch.zeros(ls.N, LPAD, dtype=dtype, device=dev)
        for row0, nrows, col0, B, _ in ls.parts:
            panel[row0:row0 + nrows, col0:col0 + B.shape[1]].copy_(B * ls.scale)
        return panel

    def _lora_gemm(self, st, x, out, M: int, drop_l, save: bool, xq=None, **epilogue):
        """out = epilogue([x | u] . [W | s B | 0]^T), u = dropout(x) . A^T.  st: the adapted site (``_site``), x bf16 [M, K] contiguous.
        Returns what the backward needs (u and s B, both [*, LPAD] bf16) when save.  xq (an e4m3 image of x from a fused producer) is
        accepted for ``_site_fwd``'s uniform call and ignored on purpose: this form reads bf16 operands only."""
        ls, W, K, N = st.lora, st.W, st.K, st.N
        xcat = torch.empty(M, K + LPAD, dtype=BF16, device=x.device)
        xd = torch.empty(M, K, dtype=BF16, device=x.device) if drop_l is not None else None
        ops.lora_stage(x, xcat, xd, M, K, drop_l)                    # one pass: x into the concatenated operand + its masked copy
        u = torch.empty(M, LPAD, dtype=BF16, device=x.device)
        self._rank_gemm(xd if xd is not None else x, ls.A, u, M, K)
        xcat[:, K:].copy_(u)
        wcat = torch.empty(N, K + LPAD, dtype=BF16, device=x.device)
        wcat[:, :K].copy_(W)
        wcat[:, K:].copy_(self._lora_panel(ls))
        ops.gemm(xcat, wcat, out, M, N, K + LPAD, **epilogue)
        # (the masked copy of x is kept for dA = du^T dropout(x): re-making it in backward cost two more passes over [M, K])
        return SimpleNamespace(u=u, sB=wcat[:, K:].contiguous(), xd=xd) if save else None

    def _lora_gemm_fp8(self, st, x, out, M: int, drop_l, save: bool, bias=None, residual=None, act=0, aux_out=None, xq=None):
        """The same layer with its FROZEN base weight on fp8 operands (I2T_FP8=1; ``_fp8_weight``): the base product runs
        at the fp8 MFMA rate, so the adapter leaves the K panel -- out = fp8(x) . fp8(W)^T (+ bias) (+ residual) + u . (s B)^T, the
        rank-128 product added by a second, thin GEMM (in place on an fp32 output; ahead of the base GEMM, as its fp32 residual, when
        the output is bf16).  No K-concatenated copies of x and W; one quantisation pass over x instead."""
        ls, K, N = st.lora, st.K, st.N
        if act:          # GELU behind the layer (Falcon's dense_h_to_4h): the product goes to the pre-activation buffer, one more pass applies it
            pre = aux_out if aux_out is not None else torch.empty(M, N, dtype=BF16, device=x.device)
            sv = self._lora_gemm_fp8(st, x, pre, M, drop_l, save, bias=bias, residual=residual, xq=xq)
            ops.gelu_fwd(pre, out, erf=(act == ops.ACT_GELU_ERF))
            return sv
        xd = None
        if drop_l is not None:
            xd = x.clone()
            ops.dropout_apply(xd, M, K, drop_l)                      # (the index space of lora_stage and of the backward's epilogue mask)
        u = torch.empty(M, LPAD, dtype=BF16, device=x.device)
        self._rank_gemm(xd if xd is not None else x, ls.A, u, M, K)
        panel = self._lora_panel(ls)
        e = self._fp8_weight(st)
        x8, sx = xq if xq is not None else self._fp8_rows(x, M, K)          # (xq: the producer of x emitted the e4m3 row beside the bf16 one)
        if out.dtype == F32:
            ops.gemm_fp8(x8, sx, e.w8, e.sw, out, M, N, x8.shape[1], bias=bias, residual=residual)      # (K' = the zero-padded row length)
            ops.gemm(u, panel, out, M, N, LPAD, residual=out)
        else:
            tmp = torch.empty(M, N, dtype=F32, device=x.device)
            ops.gemm(u, panel, tmp, M, N, LPAD, residual=residual)
            ops.gemm_fp8(x8, sx, e.w8, e.sw, out, M, N, x8.shape[1], bias=bias, residual=tmp)
        return SimpleNamespace(u=u, sB=panel, xd=xd) if save else None

    def _lora_bwd(self, st, sv_l, dY, x, gW, gb, M: int, drop_l, e4m3: bool = False, dq=None):
        """dY bf16 [M, N]: gradient w.r.t. the adapted linear's pre-epilogue output.  gW / gb: gradient views of the base weight /
        bias or None (frozen).  Accumulates every parameter gradient; returns dx fp32 [M, K] = dY . W + dropout(du . A)."""
        ls, W, K, N = st.lora, st.W, st.K, st.N
        if gW is not None:
            ops.gemm(dY, x, gW, N, K, M, a_kmajor=True, b_kmajor=True, accumulate=True, colsum_out=gb)
        elif gb is not None:
            ops.colsum(dY, gb, M, N, accumulate=True)
        tmp = torch.zeros(N, LPAD, dtype=F32, device=dY.device)
        ops.gemm(dY, sv_l.u, tmp, N, LPAD, M, a_kmajor=True, b_kmajor=True, accumulate=True)
        for row0, nrows, col0, B, GB in ls.parts:             # (a fused projection: only the diagonal blocks are parameters)
            GB.add_(tmp[row0:row0 + nrows, col0:col0 + B.shape[1]], alpha=ls.scale)
        du = torch.empty(M, LPAD, dtype=BF16, device=dY.device)
        self._rank_gemm(dY, sv_l.sB, du, M, N, b_kmajor=True)
        xd = sv_l.xd if sv_l.xd is not None else x
        ops.gemm(du, xd, ls.GA, LPAD, K, M, a_kmajor=True, b_kmajor=True, accumulate=True)
        dx = torch.empty(M, K, dtype=F32, device=dY.device)
        if e4m3:      # frozen base weight: dx on fp8 operands too
            e = self._fp8_weight(st)
            d8, sd = dq if dq is not None else self._fp8_rows(dY, M, N)
            ops.gemm_fp8(d8, sd, e.wt8, e.swt, dx, M, K, d8.shape[1])
        else:
            ops.gemm(dY, W, dx, M, K, N, b_kmajor=True)
        ops.gemm(du, ls.A, dx, M, K, LPAD, b_kmajor=True, residual=dx, drop=drop_l)
        return dx

    # ------------------------------------------------------------------------------------------------ generation: merged weights
    def lora_merged(self, l: int, site: str, W_name: str, rows=None):
        """bf16 W + s B A of one adapted linear in a persistent buffer (same address on every call: captured decode graphs read it);
        ``prepare_lora_merged`` recomputes the contents from the current parameters."""
        key = ('lora_merged', l, site, id(self.arena))
        buf = self._sub_cache.get(key)
        if buf is None:
            ls = self._lora_site(l, site) if self.dec.llama is None else self._llama_lora(l, site)
            buf = self._sub_cache[key] = torch.empty(ls.N, ls.K, dtype=BF16, device=self.arena.device)
            self._lora_merge_list.append((buf, l, site, W_name, rows))
        return buf

    def prepare_lora_merged(self):
        """Create every adapted linear's merged-weight buffer and bring the contents up to date with the parameters (skipped when
        nothing changed since the last call).  Called before a decode -- by ConcurrentGreedyDecoder on the parent stream, before it
        fans out: the buffers are shared by its lanes."""
        lo = getattr(self.dec, 'lora', None)
        if lo is None:
            return
        a, d = self.arena, self.dec.d
        for l in range(self.dec.L if self.dec.llama is not None else 0):          # Llama / Qwen2 blocks (engine_llama._llama_lora)
            v = self._llama_views(l)
            for site, names in (('qkv', v.names.qkv), ('o', v.names.o), ('gu', v.names.gu), ('dn', v.names.dn)):
                if self._llama_lora(l, site) is not None:
                    self.lora_merged(l, site, names, None)
        for l in range(self.dec.L if self.dec.llama is None else 0):
            p = f'{self.dp}transformer.h.{l}'
            for site, name, rows in (('attn_c_attn', f'{p}.attn.c_attn.weight', None), ('mlp_c_fc', f'{p}.mlp.c_fc.weight', None),
                                     ('mlp_c_proj', f'{p}.mlp.c_proj.weight', None),
                                     ('xattn_c_attn', f'{p}.cross_attn.in_proj_weight', slice(d, 3 * d))):
                if site in lo.sites and name in a.entries:
                    self.lora_merged(l, site, name, rows)
        ver = (id(a), len(self._lora_merge_list), a.generation)       # (prepare() has run refresh_shadow: torch-side writes are counted)
        if ver == getattr(self, '_lora_merged_ver', None):
            return
        self._lora_merged_ver = ver
        for buf, l, site, W_name, rows in self._lora_merge_list:
            ls = self._lora_site(l, site) if self.dec.llama is None else self._llama_lora(l, site)
            W = a.P(W_name) if isinstance(W_name, str) else a.span('P', W_name, (ls.N, ls.K))
            W = W if rows is None else W[rows]
            # buf = bf16(W + s B A): one GEMM on the padded rank (the [N, LPAD] panel of _lora_panel; A's pad rows are zero in the arena),
            # the fp32 base weight as the epilogue's residual
            ops.gemm(self._lora_panel(ls), ls.A, buf, ls.N, ls.K, LPAD, b_kmajor=True, residual=W.contiguous())
