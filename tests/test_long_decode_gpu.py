"""Decoding past 1024 cached keys on the Llama-family decoders: the split-key decode attention
(i2t_gq_decode_attention_long, i2t_beam_gq_decode_attention_long) against the fp64 statement test_decode_kernels_gpu.py holds the classic
kernel to, under the same bound; its history table, one captured launch over many positions, its refusals; and generate /
generate_captions / beam search over 1030-token prompts on the fixture Llama, which the classic window refuses.

The kernel bound is test_gq_decode_attention's check(1e-4, 1/200): the output is the same single bf16 rounding (2^-9) of an fp32 sum, and
the combine adds at most NC fp32 rescales of ~1e-7 relative each."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import DECODE_LONG_MAX_KEYS, LONG_CHUNK_KEYS
from test_decode_kernels_gpu import check, i32, ref_attn, rnd

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
CH = LONG_CHUNK_KEYS
ATOL, RTOL = 1e-4, 1 / 200


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def over_bound(got, ref):
    """worst |got - ref| / (ATOL + RTOL |ref|)"""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def workspace(ops, R, H, max_keys, hd):
    return torch.empty(ops.gq_decode_long_workspace_floats(R, H, max_keys, hd), dtype=F32, device=dev())


# ------------------------------------------------------------------------------------------------------ a. the kernel against fp64
@pytest.mark.parametrize('H,Hkv,hd', [(4, 2, 64), (12, 2, 128), (71, 1, 64), (32, 32, 128)])
def test_split_kernel_against_fp64(ops, H, Hkv, hd):
    R, T = 2, 9 * CH
    G, w, scale = H // Hkv, Hkv * hd, hd ** -0.5
    kt, vt = rnd(R, T, Hkv, hd, dtype=BF16, seed=hd + H), rnd(R, T, Hkv, hd, dtype=BF16, seed=2 * hd + H)
    out = torch.empty(R, H * hd, dtype=BF16, device=dev())
    ws = workspace(ops, R, H, T, hd)
    worst = 0.0
    for n in sorted({1, CH - 1, CH, CH + 1, 1024, 1025, 9 * CH - 1, 9 * CH}):
        last_chunk = (n - 1) // CH * CH                     # first slot of the last live chunk
        cases = [(0.0, 'flat', None), (1.0, 'mixed', None)]
        cases += [(8.0, f'one-hot@{t}', t) for t in sorted({min(CH // 2, n - 1), last_chunk, n - 1})]
        for qscale, tag, win in cases:
            q = (rnd(R, H * hd, dtype=BF16, seed=7 * n + H).float() * qscale).to(BF16)
            kvn = rnd(R, 2 * w, dtype=BF16, seed=n + 1)
            k0, v0 = kt, vt
            if win is not None:     # the key along the query of its group's first head: that head's softmax is one-hot at slot `win`
                qd = q.view(R, Hkv, G, hd)[:, :, 0].float()
                plant = (qd / qd.norm(dim=-1, keepdim=True) * 8.0).to(BF16)
                k0 = kt.clone()
                k0[:, win] = plant
                if win == n - 1:
                    kvn[:, :w] = plant.reshape(R, w)
            qv = q.view(R, H, hd)
            # the append form: slot n - 1 is written by the launch and attended to from the new rows
            kc, vc = k0.clone(), vt.clone()
            ops.gq_decode_attention_long(q, kvn[:, :w], kvn[:, w:], kc, vc, T * w, w, out, i32([n - 1]), 0, T, R, H, Hkv, hd, ws)
            ke, ve = k0.clone(), v0.clone()
            ke[:, n - 1], ve[:, n - 1] = kvn[:, :w].view(R, Hkv, hd), kvn[:, w:].view(R, Hkv, hd)
            assert torch.equal(kc, ke) and torch.equal(vc, ve), f'append n={n} {tag}: the cache differs outside slot n - 1'
            want = ref_attn(qv, ke[:, :n], ve[:, :n], scale, G)
            if win is not None:
                p = torch.softmax(torch.einsum('bhe,bnhe->bhn', qv.double(), ke[:, :n].double().repeat_interleave(G, 2)) * scale, -1)
                assert bool((p[:, ::G, win] > 0.99).all()), f'n={n} {tag}: the planted key does not win'
            worst = max(worst, over_bound(out.view(R, H, hd), want))
            check(f'long append hd={hd} H={H}/{Hkv} n={n} {tag}', out.view(R, H, hd), want, ATOL, RTOL)
            # the cached form, through pos_ptr and through a fixed key count
            want = ref_attn(qv, k0[:, :n], v0[:, :n], scale, G)
            kc, vc = k0.clone(), vt.clone()
            ops.gq_decode_attention_long(q, None, None, kc, vc, T * w, w, out, i32([n - 1]), 0, T, R, H, Hkv, hd, ws)
            worst = max(worst, over_bound(out.view(R, H, hd), want))
            check(f'long cached hd={hd} H={H}/{Hkv} n={n} {tag}', out.view(R, H, hd), want, ATOL, RTOL)
            o2 = torch.empty_like(out)
            ops.gq_decode_attention_long(q, None, None, kc, vc, T * w, w, o2, None, n, T, R, H, Hkv, hd, ws)
            assert torch.equal(o2, out), f'fixed n={n} {tag}'
            assert torch.equal(kc, k0) and torch.equal(vc, vt), 'the cached form writes no cache'
    print(f'split kernel hd={hd} H={H}/{Hkv}: worst error over the bound {worst:.3g}')


# ------------------------------------------------------------------------------------------------------ b. the history table
@pytest.mark.parametrize('H,Hkv,hd', [(4, 2, 64), (12, 2, 128)])
def test_history_table(ops, H, Hkv, hd):
    R, T = 4, 5 * CH
    G, w, scale = H // Hkv, Hkv * hd, hd ** -0.5
    kt, vt = rnd(R, T, Hkv, hd, dtype=BF16, seed=3 + H), rnd(R, T, Hkv, hd, dtype=BF16, seed=4 + H)
    ws = workspace(ops, R, H, T, hd)
    ident = torch.arange(R, dtype=torch.int32, device=dev()).unsqueeze(1).expand(R, T).contiguous()
    g = torch.Generator().manual_seed(H)
    perm = torch.randint(0, R, (R, T), generator=g, dtype=torch.int32).to(dev())
    o0, o1 = (torch.empty(R, H * hd, dtype=BF16, device=dev()) for _ in range(2))
    for n in (CH + 1, 3 * CH + 5, 5 * CH):
        q = rnd(R, H * hd, dtype=BF16, seed=n, scale=2.0)
        kvn = rnd(R, 2 * w, dtype=BF16, seed=n + 1)
        pos = i32([n - 1])
        for new in ((kvn[:, :w], kvn[:, w:]), (None, None)):
            k1, v1, k2, v2 = kt.clone(), vt.clone(), kt.clone(), vt.clone()
            ops.gq_decode_attention_long(q, *new, k1, v1, T * w, w, o0, pos, 0, T, R, H, Hkv, hd, ws)
            ops.beam_gq_decode_attention_long(q, *new, k2, v2, T * w, w, o1, pos, 0, T, R, H, Hkv, hd, ws, hist=ident)
            assert torch.equal(o0, o1) and torch.equal(k1, k2) and torch.equal(v1, v2), f'identity table n={n}'
        # rows drawn per key: key t of row r comes from row perm[r][t]; the new token goes to the row's own slot n - 1
        k2, v2 = kt.clone(), vt.clone()
        ops.beam_gq_decode_attention_long(q, kvn[:, :w], kvn[:, w:], k2, v2, T * w, w, o1, pos, 0, T, R, H, Hkv, hd, ws, hist=perm)
        kn, vn = kvn[:, :w].view(R, Hkv, hd), kvn[:, w:].view(R, Hkv, hd)
        rest = torch.arange(T, device=dev()) != n - 1
        assert torch.equal(k2[:, n - 1], kn) and torch.equal(v2[:, n - 1], vn), 'the new key goes to (r, n - 1)'
        assert torch.equal(k2[:, rest], kt[:, rest]) and torch.equal(v2[:, rest], vt[:, rest]), 'nothing else is written'
        ar = torch.arange(n - 1, device=dev())
        rows = perm[:, :n - 1].long()
        kk, vv = torch.cat([kt[rows, ar], kn.unsqueeze(1)], 1), torch.cat([vt[rows, ar], vn.unsqueeze(1)], 1)
        want = ref_attn(q.view(R, H, hd), kk, vv, scale, G)
        print(f'history table hd={hd} n={n} append: worst error over the bound {over_bound(o1.view(R, H, hd), want):.3g}')
        check(f'permuted table append n={n}', o1.view(R, H, hd), want, ATOL, RTOL)
        ar = torch.arange(n, device=dev())
        rows = perm[:, :n].long()
        ops.beam_gq_decode_attention_long(q, None, None, k2, v2, T * w, w, o1, pos, 0, T, R, H, Hkv, hd, ws, hist=perm)
        check(f'permuted table cached n={n}', o1.view(R, H, hd), ref_attn(q.view(R, H, hd), k2[rows, ar], v2[rows, ar], scale, G), ATOL, RTOL)


# ------------------------------------------------------------------------------------------------------ c. one graph, many positions
def test_one_graph_serves_every_position(ops):
    from image2text_amd.decoding import _capture_launches
    R, H, Hkv, hd, T = 2, 12, 2, 128, 9 * CH
    w = Hkv * hd
    kt, vt = rnd(R, T, Hkv, hd, dtype=BF16, seed=1), rnd(R, T, Hkv, hd, dtype=BF16, seed=2)
    q, kvn = rnd(R, H * hd, dtype=BF16, seed=3, scale=2.0), rnd(R, 2 * w, dtype=BF16, seed=4)
    ws = workspace(ops, R, H, T, hd)
    first, last = 4 * CH - 3, 4 * CH + 3
    # eager: one launch per position on its own caches (every launch appends, so the caches evolve as under the replays)
    ke, ve, eager = kt.clone(), vt.clone(), []
    for p in range(first, last + 1):
        o = torch.empty(R, H * hd, dtype=BF16, device=dev())
        ops.gq_decode_attention_long(q, kvn[:, :w], kvn[:, w:], ke, ve, T * w, w, o, i32([p]), 0, T, R, H, Hkv, hd, ws)
        eager.append(o)
    kc, vc = kt.clone(), vt.clone()
    out = torch.empty(R, H * hd, dtype=BF16, device=dev())
    pos = i32([first])
    launch = lambda: ops.gq_decode_attention_long(q, kvn[:, :w], kvn[:, w:], kc, vc, T * w, w, out, pos, 0, T, R, H, Hkv, hd, ws)
    graph = _capture_launches(dev(), launch)                # capture runs nothing: the caches are still the inputs
    assert torch.equal(kc, kt)
    for i, p in enumerate(range(first, last + 1)):
        graph.launch()
        assert int(pos.item()) == p and torch.equal(out, eager[i]), f'replay at position {p}'
        ops.advance(pos, 1)
    assert torch.equal(kc, ke) and torch.equal(vc, ve)


# ------------------------------------------------------------------------------------------------------ d. refusals
def test_refusals(ops):
    from image2text_amd import lib as i2tlib
    lib = i2tlib.load()
    R, H, Hkv, hd, T = 2, 4, 2, 64, 2 * CH
    w = Hkv * hd
    q = torch.zeros(R, H * hd, dtype=BF16, device=dev())
    out = torch.full((R, H * hd + 8), 3.0, dtype=BF16, device=dev())
    kc, vc = torch.zeros(R, T + 1, w, dtype=BF16, device=dev()), torch.zeros(R, T + 1, w, dtype=BF16, device=dev())
    ws = workspace(ops, R, H, T, hd)
    hist = torch.zeros(R, T, dtype=torch.int32, device=dev())
    pos = i32([0])
    base = dict(q=q.data_ptr(), q_rs=H * hd, kc=kc.data_ptr(), vc=vc.data_ptr(), cache_bs=(T + 1) * w, cache_rs=w, out=out.data_ptr(),
                out_rs=H * hd + 8, pos=pos.data_ptr(), n_fixed=0, max_keys=T, hd=hd, ws=ws.data_ptr(), ws_floats=ws.numel(),
                hist=hist.data_ptr(), hist_ld=T)

    def call(beam, **kw):
        a = {**base, **kw}
        head = (None, a['q'], a['q_rs'], None, None, 0, a['kc'], a['vc'], a['cache_bs'], a['cache_rs'], a['out'], a['out_rs'], a['pos'],
                a['n_fixed'], a['max_keys'])
        tail = (R, H, Hkv, a['hd'], a['ws'], a['ws_floats'])
        if beam:
            return lib.i2t_beam_gq_decode_attention_long(*head, a['hist'], a['hist_ld'], *tail)
        return lib.i2t_gq_decode_attention_long(*head, *tail)

    cases = [(dict(max_keys=0), 'max_keys'), (dict(max_keys=-4), 'max_keys'), (dict(max_keys=DECODE_LONG_MAX_KEYS + 1), 'max_keys'),
             (dict(pos=None, n_fixed=T + 1), 'n_keys_fixed'), (dict(ws=None), 'ws'), (dict(ws_floats=ws.numel() - 1), 'ws'),
             (dict(ws=ws.data_ptr() + 4), 'ws'), (dict(hd=16), 'head_dim'), (dict(hd=32), 'head_dim'),
             (dict(kc=kc.data_ptr() + 2), 'aligned'), (dict(vc=vc.data_ptr() + 2), 'aligned'), (dict(out=out.data_ptr() + 2), 'aligned'),
             (dict(cache_rs=w + 4), 'aligned'), (dict(out_rs=H * hd + 4), 'aligned')]
    for beam in (False, True):
        name = 'i2t_beam_gq_decode_attention_long' if beam else 'i2t_gq_decode_attention_long'
        for kw, word in cases + ([(dict(hist_ld=T - 1), 'hist_ld'), (dict(hist=None), 'hist')] if beam else []):
            rc = call(beam, **kw)
            msg = i2tlib.last_error()
            assert rc == -1 and name in msg and word in msg, (beam, kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), 'a refused call wrote the output'
    assert call(False) == 0 and call(True) == 0              # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((out[:, :H * hd] == 0).all()) and bool((out[:, H * hd:] == 3.0).all())


# ------------------------------------------------------------------------------------------------------ e / f. end to end
P_LONG, NEW = 1030, 6


def _llama(tmp_path, monkeypatch):
    from test_hf_decoder_gpu import _llama_model
    cfg, m, _, V = _llama_model(tmp_path, monkeypatch, 'llama')
    m = m.to(dev()).eval()
    dc = m._engine.dec
    assert dc.llama is not None and dc.prefixed and dc.block == 4096 and (dc.llama.H, dc.llama.Hkv, dc.llama.hd) == (4, 2, 64)
    g = torch.Generator().manual_seed(5)
    images = torch.randn(2, 3, 32, 32, generator=g).to(dev())
    prompt = torch.randint(0, V, (2, P_LONG), generator=g).to(dev())
    return cfg, m, images, prompt


def check_row_logprobs(m, images, out, tag):
    """check_logprobs for rows whose prompts differ in length: every row against the forward over ITS ids, 4 . logits_tol"""
    from test_model_gpu import logits_tol
    B, N, L = out.ids.shape
    assert N == 1
    pmin = int(out.prompt_lengths.min())
    worst = 0.0
    for b in range(B):
        p, n = int(out.prompt_lengths[b]), int(out.lengths[b, 0])
        ids = out.ids[b, :, :n]
        with torch.no_grad():
            logits = m(images=images[b:b + 1], ids=ids).logits
        bar = 4 * logits_tol(logits.float().cpu().numpy())
        ref = torch.log_softmax(logits.double(), dim=-1)[0, p - 1:n - 1].gather(-1, ids[0, p:, None])[:, 0]
        got = out.token_logprobs[b, 0]
        assert bool((got[:p - pmin] == 0).all()) and bool((got[n - pmin:] == 0).all())
        err = float((got[p - pmin:n - pmin].double() - ref).abs().max())
        worst = max(worst, err / bar)
        assert torch.isfinite(got).all() and err <= bar, (tag, b, err, bar)
    print(f'{tag}: token_logprobs worst error / bar vs forward {worst:.3g}')


def test_generate_captions_past_the_classic_window(tmp_path, monkeypatch):
    from test_generate_captions_gpu import check_logprobs, check_shapes
    cfg, m, images, prompt = _llama(tmp_path, monkeypatch)
    short = prompt[:, :4].contiguous()
    before = m.generate_captions(images, short, max_new_tokens=NEW, top_k=1)
    cap = m._captioner
    assert cap._state is not None and cap._long_state is None and cap._state.clen <= 1024
    outs = {}
    for mode, prefill, replays in (('pass', 0, NEW), ('steps', P_LONG - 1, NEW)):
        out = outs[mode] = m.generate_captions(images, prompt, max_new_tokens=NEW, top_k=1, prompt_prefill=mode)
        check_shapes(out, 2, 1, P_LONG)
        assert bool((out.lengths == P_LONG + NEW).all()) and torch.equal(out.ids[:, 0, :P_LONG], prompt)
        assert (cap.last_prefill_steps, cap.last_replays) == (prefill, replays), mode
        check_logprobs(m, images, out, P_LONG, f'llama P={P_LONG} prompt_prefill={mode}')
    st = cap._long_state
    assert st is not None and st.clen > 1024 and st.clen % CH == 0 and st.clen >= 8 + P_LONG + NEW and st.attn_ws is not None
    # generate(): the same ids as the step-by-step captions
    ids = m.generate(images, prompt, max_new_tokens=NEW, top_k=1)
    assert torch.equal(ids, outs['steps'].ids[:, 0])
    assert m._greedy._long_state is not None and m._greedy._state is None
    # prompts of different lengths in one long batch
    rag = m.generate_captions(images, prompt, max_new_tokens=NEW, top_k=1, prompt_lengths=[P_LONG, 700])
    assert rag.lengths.flatten().tolist() == [P_LONG + NEW, 700 + NEW] and cap._long_state is st
    assert (cap.last_prefill_steps, cap.last_replays) == (699, P_LONG - 700 + NEW)
    check_row_logprobs(m, images, rag, f'llama prompt_lengths=[{P_LONG}, 700]')
    # f. a short call is what it was before the long ones: its state and graphs were never touched
    after = m.generate_captions(images, short, max_new_tokens=NEW, top_k=1)
    assert torch.equal(after.ids, before.ids) and torch.equal(after.token_logprobs, before.token_logprobs)
    assert cap._long_state is st


def test_beam_search_past_the_classic_window(tmp_path, monkeypatch):
    from image2text_amd.decoding import BeamDecoder, BeamSpec
    from test_beam_cache_gpu import rescore
    cfg, m, images, prompt = _llama(tmp_path, monkeypatch)
    ngrams = tuple(cfg.no_repeat_n_grams)
    spec = BeamSpec(2, 2, 0.0, None, 0.0, None, 0.0, ngrams)
    dec = BeamDecoder(m)
    ids, scores = dec.search(images, prompt, P_LONG + 4, spec)
    assert dec._long_state is not None and dec._state is None and dec._long_state.hist.shape[1] == dec._long_state.clen > 1024
    assert tuple(ids.shape) == (2, 2, P_LONG + 4) and bool((ids[:, :, :P_LONG] == prompt[:, None]).all())
    assert torch.isfinite(scores).all() and bool((scores[:, :-1] >= scores[:, 1:]).all())
    with torch.no_grad():
        want = rescore(m, images, ids, P_LONG, ngrams, 2)
    err = (scores.double().cpu() - want).abs().max().item()
    print(f'long beam search: worst |score - teacher-forced sum| {err:.3g} (bound {2e-2 * 4:.3g})')
    assert err <= 2e-2 * 4, err
    # through the public generator
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    gen = BeamSearchTokenGenerator(m, beam_width=2, temperature=0.0, max_new_tokens=5, no_repeat_n_grams=ngrams,     # max_len = P + 5 - 1
                                   beam_expansion_factor=2, consolidation_temperature=0.0, kv_cache=True)
    gids, gscores = gen(images, prompt)
    assert torch.equal(gids, ids) and torch.equal(gscores, scores)
