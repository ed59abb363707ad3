"""tests/train_ref.py against torch float64 autograd (1e-12 relative), and its extras against compositions of the plain reference.
No GPU, no library."""
import numpy as np
import torch
import torch.nn.functional as F

import train_ref as R

F64 = torch.float64
REL = 1e-12


def close(name, got, ref):
    got, ref = got.to(F64), ref.to(F64)
    scale = ref.abs().max().clamp_min(1e-300)
    err = (got - ref).abs().max() / scale
    assert got.shape == ref.shape and float(err) <= REL, f'{name}: {float(err):.3g} relative'


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=F64) * scale


def _ln_case(M, d, seed):
    x = (rand(M, d, seed=seed) + 100.0) * torch.logspace(-3, 3, M, dtype=F64).unsqueeze(1)
    return x, 1 + 0.5 * rand(d, seed=seed + 1), rand(d, seed=seed + 2), rand(M, d, seed=seed + 3)


def test_row_layernorm_matches_autograd():
    for M, d, eps in ((5, 64, 1e-5), (3, 260, 1e-6), (1, 4, 1e-5)):
        x, g, b, dy = _ln_case(M, d, M + d)
        e = R.f32(eps)
        xa, ga, ba = (t.clone().requires_grad_() for t in (x, g, b))
        y = F.layer_norm(xa, (d,), ga, ba, e)
        y.backward(dy)
        r = R.ln_fwd(x, g, b, eps)
        close('y', r['y'], y.detach())
        close('mean', r['mean'], x.mean(-1))
        close('rstd', r['rstd'], (x.var(-1, unbiased=False) + e).rsqrt())
        close('y no beta', R.ln_fwd(x, g, None, eps)['y'], F.layer_norm(x, (d,), g, None, e))
        bw = R.ln_bwd(dy, x, g, r['mean'], r['rstd'])
        close('dx', bw['dx'], xa.grad)
        close('dgamma', bw['dgamma'], ga.grad)
        close('dbeta', bw['dbeta'], ba.grad)
        assert (bw['dx_terms'] >= bw['dx'].abs() * (1 - 1e-12)).all() and (bw['dgamma_terms'] >= bw['dgamma'].abs() * (1 - 1e-12)).all()


def test_row_layernorm_extras_are_compositions():
    M, d = 11, 64
    x, g, b, dy = rand(M, d, seed=5), 1 + 0.5 * rand(d, seed=6), None, rand(M, d, seed=7)
    r = R.ln_fwd(x, g, b, 1e-5)
    plain = R.ln_bwd(dy, x, g, r['mean'], r['rstd'])
    dx0 = rand(M, d, seed=8)
    acc = R.ln_bwd(dy, x, g, r['mean'], r['rstd'], dx0=dx0)
    close('accumulate', acc['dx'], plain['dx'] + dx0)
    # acc_period: "zero-fill the other rows, then accumulate"
    for period, rows in ((5, 1), (5, 0), (5, 5), (4, 2)):
        filled = dx0.clone()
        filled[torch.arange(M) % period >= rows] = 0.0
        close(f'acc_period {period} {rows}', R.ln_bwd(dy, x, g, r['mean'], r['rstd'], dx0=dx0, acc_period=period, acc_rows=rows)['dx'],
              R.ln_bwd(dy, x, g, r['mean'], r['rstd'], dx0=filled)['dx'])
    # dx_pre_sumsq: "normalise dx0 first, then accumulate"
    ss = torch.tensor([float(dx0.pow(2).sum())], dtype=F64)
    close('pre_sumsq', R.ln_bwd(dy, x, g, r['mean'], r['rstd'], dx0=dx0, pre_sumsq=ss)['dx'],
          R.ln_bwd(dy, x, g, r['mean'], r['rstd'], dx0=R.grad_normalize(dx0)['g'])['dx'])
    # masks: the f32 dx is masked, sumsq and the bf16 copy see the unmasked value; the bf16 drop touches the copy only
    mask, drop = torch.rand(M, d, generator=torch.Generator().manual_seed(1)) > 0.3, torch.rand(M, d, generator=torch.Generator().manual_seed(2)) > 0.3
    both = R.ln_bwd(dy, x, g, r['mean'], r['rstd'], dx0=dx0, mask=mask, mask_scale=1.25, drop=drop, drop_scale=1.5)
    close('dx masked', both['dx'], acc['dx'] * mask * 1.25)
    close('bf16 dropped', both['dx_bf16'], acc['dx'] * drop * 1.5)
    close('sumsq unmasked', both['sumsq'], acc['dx'].pow(2).sum())
    close('unmasked', both['dx_unmasked'], acc['dx'])


def test_layernorm_nd_matches_autograd():
    for B, rows, d in ((3, 3, 20), (2, 17, 964), (1, 1, 4)):
        n = rows * d
        x, add, g, b, dy = rand(B, n, seed=B), rand(n, seed=1), 1 + 0.5 * rand(n, seed=2), rand(n, seed=3), rand(B, n, seed=4)
        xa, aa, ga, ba = (t.clone().requires_grad_() for t in (x, add, g, b))
        e = R.f32(1e-5)
        y = F.layer_norm((xa + aa).view(B, rows, d), (rows, d), ga.view(rows, d), ba.view(rows, d), e).view(B, n)
        y.backward(dy)
        r = R.lnnd_fwd(x, add, g, b)
        close('y', r['y'], y.detach())
        bw = R.lnnd_bwd(dy, x, add, g, r['mean'], r['rstd'])
        for name, ref in (('dx', xa.grad), ('dgamma', ga.grad), ('dbeta', ba.grad), ('dadd', aa.grad)):
            close(name, bw[name], ref)
        close('y no add', R.lnnd_fwd(x, None, g, None)['y'], F.layer_norm(x, (n,), g, None, e))
        keep = torch.rand(B, n, generator=torch.Generator().manual_seed(3)) > 0.2
        close('drop', R.lnnd_fwd(x, add, g, b, keep=keep, keep_scale=1.25)['y'], r['y'] * keep * 1.25)


def test_embedding_matches_index_add():
    vocab, npos, d, B, T, off = 11, 9, 8, 3, 4, 2
    ids = torch.tensor([[0, 10, -3, 11], [16, 5, 5, 5], [1, 2, 3, 4]])
    wte, wpe, dx = rand(vocab, d, seed=1), rand(npos, d, seed=2), rand(B * T, d, seed=3)
    tok = ids.reshape(-1).clamp(0, vocab - 1)
    for pos in (None, torch.tensor([0, 1, 2, 0, 1, 0, 1, 2, 3, 0, 0, 0], dtype=torch.int32)):
        p = (pos.long() if pos is not None else torch.arange(B * T) % T) + off
        close('fwd', R.embed_fwd(ids, wte, wpe, T, off, vocab, pos), wte[tok] + wpe[p])
        close('fwd no wpe', R.embed_fwd(ids, wte, None, T, off, vocab, pos), wte[tok])
        r = R.embed_bwd(ids, dx, vocab, npos, T, off, vocab, pos)
        close('dwte', r['dwte'], torch.zeros(vocab, d, dtype=F64).index_add_(0, tok, dx))
        close('dwpe', r['dwpe'], torch.zeros(npos, d, dtype=F64).index_add_(0, p, dx))
        assert int(r['dwte_count'].sum()) == B * T and int(r['dwte_count'][5]) == 3 and int(r['dwte_count'][10]) == 3


def test_cross_entropy_matches_autograd():
    M, V, ld, ignore = 9, 13, 16, -100
    z = torch.full((M, ld), 7.0, dtype=torch.bfloat16)
    z[:, :V] = rand(M, V, seed=1, scale=2.0).to(torch.bfloat16)
    labels = torch.tensor([0, V - 1, 9, ignore, -5, V, V + 3, 4, 2])
    w = torch.rand(M, generator=torch.Generator().manual_seed(2), dtype=F64).float()
    w[7] = 0.0
    for temp in (1.0, 0.7, 2.0):
        it = R.f32(1.0 / temp)
        r = R.ce(z, V, labels, w, 1.0 / temp, ignore, gscale=3.1)
        live = r['live']
        assert live.tolist() == [True, True, True, False, False, False, False, True, True]
        za = z[:, :V].double().clone().requires_grad_()
        rows = F.cross_entropy(za[live] * it, labels[live], reduction='none') * w[live].double()
        (rows.sum() * R.f32(3.1)).backward()
        close('rows', r['rows'][live], rows.detach())
        close('loss', r['loss'], rows.detach().sum())
        close('grad', r['grad'][live], za.grad[live])
        close('lse', r['lse'][live], torch.logsumexp(z[:, :V].double()[live] * it, -1))
        assert (r['grad'][~live] == 0).all() and (r['lse'][~live] == 0).all() and (r['rows'][~live] == 0).all() and (r['grad'][7] == 0).all()
        one = R.ce(z, V, labels, w, 1.0 / temp, ignore)
        close('two-pass = gscale x one-pass', r['grad'], one['grad'] * R.f32(3.1))
    close('scale_bf16', R.scale_bf16(z, 0.5), z.double() * 0.5)


def test_grad_normalize_matches_the_definition():
    g = rand(1023, seed=1, scale=30.0)
    n = R.grad_normalize(g)
    close('g', n['g'], g / (g.norm() + 1e-6))
    close('sumsq', R.sumsq(g, start=2.5), g.pow(2).sum() + 2.5)
    ws = torch.tensor([float(g.pow(2).sum())], dtype=F64)
    close('presummed', R.grad_normalize(g, ws=ws)['g'], n['g'])
    keep = torch.rand(1023, generator=torch.Generator().manual_seed(1)) > 0.1
    k = R.grad_normalize(g, keep=keep, keep_scale=256 / 230, keep_f32=True)
    assert torch.equal(k['g'], g)
    close('bf16 copy', k['g_bf16'], n['g'] * keep * R.f32(256 / 230))
    z = R.grad_normalize(torch.zeros(5, dtype=F64))
    assert (z['g'] == 0).all() and torch.isfinite(z['g']).all()


def test_adamw_matches_torch_optim():
    """5 steps of torch.optim.AdamW on float64 parameters, one parameter per live segment; a frozen and an lr == 0 segment beside them"""
    sizes, lrs, wds = [8, 40, 16, 24], [3e-3, -1.0, 0.0, 1e-2], [0.1, 0.3, 0.2, 0.0]
    ends = np.cumsum(sizes).tolist()
    n, b1, b2, eps, gs = ends[-1], 0.9, 0.999, 1e-8, 1.0 / 64
    p = rand(n, seed=1)
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    segs = [slice(e - s, e) for s, e in zip(sizes, ends)]
    params = [p[s].clone().requires_grad_() for s in segs]
    opt = torch.optim.AdamW([dict(params=[params[i]], lr=R.f32(lrs[i]), weight_decay=R.f32(wds[i])) for i in (0, 2, 3)],
                            betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps))
    p0 = p.clone()
    for step in range(1, 6):
        g = rand(n, seed=10 + step, scale=4.0)
        for i in (0, 2, 3):
            params[i].grad = g[segs[i]] * R.f32(gs)
        opt.step()
        r = R.adamw(p, g, m, v, ends, lrs, wds, b1, b2, eps, step, grad_scale=gs)
        p, m, v = r['p'], r['m'], r['v']
        for i in (0, 2, 3):
            close(f'step {step} segment {i} p', p[segs[i]], params[i].detach())
            st = opt.state[params[i]]
            close(f'step {step} segment {i} m', m[segs[i]], st['exp_avg'])
            close(f'step {step} segment {i} v', v[segs[i]], st['exp_avg_sq'])
        assert torch.equal(p[segs[1]], p0[segs[1]]) and (m[segs[1]] == 0).all() and (v[segs[1]] == 0).all() and r['frozen'][segs[1]].all()
        assert torch.equal(p[segs[2]], p0[segs[2]]) and float(v[segs[2]].min()) > 0
    z = R.adamw(torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(8, dtype=F64), [8], [1e-3], [0.0],
                b1, b2, eps, 1)
    assert torch.isfinite(z['p']).all() and torch.equal(z['p'], torch.ones(8, dtype=F64))


def test_strided_helpers():
    x = rand(5, 3, 8, seed=1)
    s, t = R.sum_over_batch(x, start=torch.ones(3, 8, dtype=F64))
    close('sum_over_batch', s, x.sum(0) + 1)
    assert (t >= s.abs() * (1 - 1e-12)).all()
    xb = rand(100, 16, seed=2).to(torch.bfloat16)
    ss = torch.tensor([4.0])
    s, _ = R.colsum(xb, 12, start=torch.full((12,), 2.0, dtype=F64), alpha_sumsq=ss)
    close('colsum', s, xb.double()[:, :12].sum(0) / (2.0 + 1e-6) + 2)
    keep = torch.tensor([True, False, True, False])
    d = R.dropout(torch.tensor([1.0, -2.0, 3.0, 4.0]), keep, 2.0)
    assert d.tolist() == [2.0, -0.0, 6.0, 0.0] and bool(torch.signbit(d[1]))
