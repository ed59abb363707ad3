"""The numpy statements the decode kernels and drivers are held to: what a kernel, or a whole search, computes, written out on the host
(``*_host``, the finish rules).  Two serve production code as well: ``slot_positions`` (GreedyDecoder._build_family) and
``apply_finish_rule_ragged`` (the non-causal path of ``generate_captions``).  No device, engine or library; ``decoding`` re-exports
every name."""
from types import SimpleNamespace
from typing import Optional

import numpy as np

from .caption_plan import BEAM_DEAD, LONG_CHUNK_KEYS
from .phrase_trie import PhraseTrie, phrase_node_csr, phrase_trie, set_level_tables, set_step_state, trie_levels


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


def top_logprobs_host(logits: np.ndarray, K: int):
    """What i2t_caption_top_logprobs computes for every row of ``logits`` [R, V] (the raw rows, any float dtype; read as given and
    evaluated in fp64) -> (tokens int32 [R, K], logprobs fp64 [R, K], entropy fp64 [R]); DESIGN.md 4ad.  The normative statement of two
    rules.  The TIE rule: column j of ``tokens`` is the j-th column of the row under the order (z descending, id ascending) -- equal
    logits, the -inf ones among them, go by ascending id.  The -INF rule: a column that holds -inf has probability 0; it adds 0 to the
    entropy, and if the list reaches it (fewer than K finite columns) its log-prob is -inf.  logprobs = z - lse(z) with lse over the
    finite columns; entropy = sum over the finite columns of p (lse - z), p = exp(z - lse).  A row without a finite column has no
    distribution: it is refused."""
    z = np.asarray(logits).astype(np.float64)
    assert z.ndim == 2 and 1 <= int(K) <= z.shape[1] and not np.isnan(z).any() and not (z == np.inf).any()
    R, V = z.shape
    tok, lp, ent = np.zeros((R, K), dtype=np.int32), np.zeros((R, K), dtype=np.float64), np.zeros(R, dtype=np.float64)
    for r in range(R):
        row = z[r]
        order = np.lexsort((np.arange(V), -row))             # the last key is the primary one: -z ascending, then the id
        fin = row[np.isfinite(row)]
        assert fin.size, f'row {r} holds no finite logit'
        m = fin.max()
        lse = m + np.log(np.exp(fin - m).sum())
        tok[r] = order[:K]
        lp[r] = row[order[:K]] - lse
        ent[r] = (np.exp(fin - lse) * (lse - fin)).sum()
    return tok, lp, ent


def score_top_logprobs_host(logits: np.ndarray, labels, K: int, scale: float = 1.0, ignore_index: int = -100):
    """What i2t_score_top_logprobs computes for every row of ``logits`` [R, V] with ``labels`` [R] -> (tokens int32 [R, K],
    logprobs fp64 [R, K], entropy fp64 [R], rank int32 [R], lse fp64 [R], label_logprob fp64 [R]).  The row the kernel works on is
    v = np.float32(z) * np.float32(scale), formed in fp32: the kernel's one rounding per column, so the order and the ties are the
    kernel's; everything after that is evaluated in fp64 by ``top_logprobs_host``'s TIE rule and -INF rule.  rank[r] = the number of
    columns c with v[c] > v[y] or (v[c] == v[y] and c < y), y = labels[r]: the label's place in the order the tokens are listed in (0:
    the arg-max), so rank < K puts y at tokens[r, rank]; a label on a -inf column has log-prob -inf and stands behind every finite
    column and the -inf columns of lower id.  A label equal to ``ignore_index`` or outside [0, V): rank -1, label_logprob 0.0."""
    z = np.asarray(logits)
    assert z.ndim == 2 and np.isfinite(np.float32(scale)) and np.float32(scale) > 0
    v = z.astype(np.float32) * np.float32(scale)
    assert v.dtype == np.float32
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    R, V = v.shape
    assert labels.shape == (R,)
    tok, lp, ent = top_logprobs_host(v, K)
    v64 = v.astype(np.float64)
    rank, lse, lab_lp = np.full(R, -1, dtype=np.int32), np.zeros(R, dtype=np.float64), np.zeros(R, dtype=np.float64)
    ids = np.arange(V)
    for r in range(R):
        fin = v64[r][np.isfinite(v64[r])]
        m = fin.max()
        lse[r] = m + np.log(np.exp(fin - m).sum())
        y = int(labels[r])
        if y == ignore_index or not 0 <= y < V:
            continue
        rank[r] = int(((v[r] > v[r, y]) | ((v[r] == v[r, y]) & (ids < y))).sum())
        lab_lp[r] = v64[r, y] - lse[r]
    return tok, lp, ent, rank, lse, lab_lp


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


def trie_mask_ragged_host(z, node: int, trie, eos: int, length: int, plen: int) -> np.ndarray:
    """What i2t_caption_trie_mask_ragged leaves of one raw fp32 logits row at column ``length`` of a row whose prompt is ``plen`` long
    (DESIGN.md 4x): the raw row while length < plen -- a forced column, where the kernel also leaves raw_lse and kept alone --, else
    ``trie_mask_host``'s.  ``trie``: a ``PhraseTrie`` or a ``PhraseForest``."""
    if int(length) < int(plen):
        return np.array(z, dtype=np.float32)
    return trie_mask_host(z, node, trie, eos)


def trie_advance_ragged_host(node: int, token: int, trie, eos: int, length: int, plen: int):
    """What i2t_caption_trie_advance_ragged does with a row at column ``length`` whose prompt is ``plen`` long -> ``trie_advance_host``'s
    triple; in a forced column (length < plen) the row keeps its node, names no phrase and its log-prob is not written (False)."""
    if int(length) < int(plen):
        return int(node), -1, False
    return trie_advance_host(node, token, trie, eos)


def constrained_decode_host(step_logits, prompt, trie: PhraseTrie, eos: int, pad, max_new: int, start: int = 0):
    """The whole greedy search of ``generate_captions(phrases=...)`` for ONE image on the host: ``step_logits(sequence)`` gives the fp32
    logits row [V] that follows a token sequence (a list of ints, the prompt included).  Every step takes ``trie_mask_host`` of the
    row, its argmax (the lower id on ties), the fp32 log_softmax of the RAW row there, and ``trie_advance_host``; the search ends with
    the EOS.  -> SimpleNamespace(ids int64 [L], length, token_logprobs f32 [L - P], logprob f32, phrase_index, steps, gaps): ``gaps``
    holds per step the best allowed logit minus the second-best allowed one (inf where a node allows one token).  A search whose gaps
    all exceed a perturbation of the logits keeps its result under it.  (``pad`` takes no part for one image -- nothing follows the EOS;
    the signature is ``beam_search_host``'s.)  ``start``: the node the walk begins at -- the root of the image's set in a
    ``PhraseForest``, whose ``term`` then names the phrase within that set; 0: a trie's root."""
    seq = [int(t) for t in np.asarray(prompt).reshape(-1)]
    P = len(seq)
    assert P >= 1 and max_new >= 1
    f32 = np.float32
    node, phrase, lps, gaps = int(start), -1, [], []
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


def phrase_set_scores_host(step_logits_fn, sets, set_index, eos: int, prompts, prompt_lengths=None):
    """The normative replica of ``score_phrases(phrase_sets=...)`` on the host: ``step_logits_fn(b, sequence)`` gives the
    raw fp32 logits row [V] that follows a token sequence for image b (a list of ints: the image's prompt, then the path from its set's
    root).  ``sets``: S phrase sets (token-id sequences, or the ``PhraseTrie`` of each); ``set_index`` [B]; ``prompts`` [B][>= p_b] with
    ``prompt_lengths`` [B] (None: every row's whole length).  It walks as the device does: one global column counter from min p_b on,
    every image forced, at its own level of its own set's tables (``set_level_tables`` / ``set_step_state``, the tables the kernel
    reads) or finished; a child's path sum is path_in[parent] + (z[token] - lse) and a phrase that ends at a node gets path_in[node] +
    (z[eos] - lse), in exactly this order in fp32 -- i2t_trie_level_expand_sets', which is i2t_trie_level_expand's: for S = 1 and equal
    lengths the values are ``phrase_scores_host``'s bit for bit.
    -> SimpleNamespace(logprob f32 [B, Kmax], -inf behind an image's own set; best int64 [B], the lowest index on ties; lengths int32
    [S, Kmax], 0 in the padding; steps: the walk steps; states: every step's int32 [B, 8])."""
    f32 = np.float32
    tries = [s if isinstance(s, PhraseTrie) else phrase_trie(s, eos, 1 << 31, 1 << 30) for s in sets]
    tabs = set_level_tables(tries)
    set_index = [int(s) for s in np.asarray(set_index).reshape(-1)]
    B, W = len(set_index), tabs.wmax
    prompts = [[int(t) for t in np.asarray(p).reshape(-1)] for p in prompts]
    plen = [len(p) for p in prompts] if prompt_lengths is None else [int(p) for p in np.asarray(prompt_lengths).reshape(-1)]
    assert len(prompts) == B and len(plen) == B and all(1 <= plen[b] <= len(prompts[b]) for b in range(B))
    logprob = np.full((B, tabs.kmax), -np.inf, dtype=f32)
    path_in, path_out = np.zeros((B, W), dtype=f32), np.zeros((B, W), dtype=f32)
    seqs = [[[]] + [None] * (W - 1) for _ in range(B)]
    states = []
    for col in range(min(plen), max(plen[b] + int(tries[set_index[b]].longest) for b in range(B)) + 1):
        st = set_step_state(tabs, set_index, plen, prompts, col)
        states.append(st)
        for b in range(B):
            level, forced, c_at, n_c, t_at, n_t, o_at, _ = (int(v) for v in st[b])
            if level < 0:
                if forced >= 0:
                    path_out[b] = path_in[b]
                continue
            rows = {}

            def row(p):
                if p not in rows:
                    z = np.asarray(step_logits_fn(b, prompts[b][:plen[b]] + seqs[b][p]), dtype=f32).reshape(-1)
                    rows[p] = (z, _row_lse_host(z))
                return rows[p]
            nxt = [None] * W
            for j in range(n_c):
                p, tk = int(tabs.child_parent[c_at + j]), int(tabs.child_tok[c_at + j])
                z, lse = row(p)
                path_out[b, j], nxt[j] = f32(path_in[b, p] + f32(z[tk] - lse)), seqs[b][p] + [tk]
            for j in range(n_t):
                p = int(tabs.term_row[t_at + j])
                z, lse = row(p)
                for i in tabs.term_phrase[tabs.term_off[o_at + j]:tabs.term_off[o_at + j + 1]].tolist():
                    logprob[b, i] = f32(path_in[b, p] + f32(z[eos] - lse))
            seqs[b] = nxt
        path_in, path_out = path_out, path_in
    best = np.array([int(np.flatnonzero(r == r.max())[0]) for r in logprob], dtype=np.int64)
    return SimpleNamespace(logprob=logprob, best=best, lengths=tabs.lengths, steps=len(states), states=states)


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


# ------------------------------------------------------------------------------------------------ search_phrases
def _row_lse_host(z) -> np.float32:
    """m + log(sum exp(z - m)) of one fp32 row in fp32, as ``phrase_scores_host`` forms it"""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    m = z.max()
    return np.float32(m + np.log(np.exp(z - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32))


def trie_beam_candidates_host(logits, node, path, trie: PhraseTrie, eos: int, W: int, V: Optional[int] = None, lse=None):
    """One i2t_trie_beam_candidates call on the host (numpy, fp32 arithmetic in the kernel's order).  ``logits`` [R, >= V]: the raw rows;
    ``node`` int [R]: every row's trie node, -1 a dead row; ``path`` f32 [R]: the row's path sum.  Per live row, with z its raw row and
    lse its log-sum-exp over [0, V) -- the mask does not enter the normaliser --: fin_total = path + (z[eos] - lse) when a phrase ends
    at the node, else -inf; every edge e of the node (a global index into child_tok / child_next) has total = path + (z[child_tok[e]] -
    lse), in exactly this order in fp32, and the row keeps its W largest, descending, the lower edge first on ties: cand_edge (-1 where
    the node has fewer than W children) and cand_total (-inf there).  A dead row gives -1 / -inf and reads no logits.  ``lse`` f32 [R]
    (optional): the rows' log-sum-exp as given -- on the device it is i2t_rows_lse's value on the same row, bit for bit, which a test
    hands in here; None: ``_row_lse_host``, the form ``phrase_scores_host`` takes.
    -> (cand_edge int32 [R, W], cand_total f32 [R, W], fin_total f32 [R], lse f32 [R], 0 at a dead row)"""
    f32 = np.float32
    logits = np.asarray(logits, dtype=f32)
    R = logits.shape[0]
    V = logits.shape[1] if V is None else V
    cand_edge, cand_total = np.full((R, W), -1, dtype=np.int32), np.full((R, W), -np.inf, dtype=f32)
    fin_total, out_lse = np.full(R, -np.inf, dtype=f32), np.zeros(R, dtype=f32)
    for r in range(R):
        nd = int(node[r])
        if nd < 0 or nd >= trie.nodes:
            continue
        z = logits[r, :V]
        ls = _row_lse_host(z) if lse is None else f32(lse[r])
        out_lse[r] = ls
        p = f32(path[r])
        if trie.term[nd] >= 0:
            fin_total[r] = f32(p + f32(z[eos] - ls))
        lo, hi = int(trie.child_off[nd]), int(trie.child_off[nd + 1])
        tot = {e: f32(p + f32(z[int(trie.child_tok[e])] - ls)) for e in range(lo, hi)}
        for i, e in enumerate(sorted(tot, key=lambda e: (-tot[e], e))[:W]):
            cand_edge[r, i], cand_total[r, i] = e, tot[e]
    return cand_edge, cand_total, fin_total, out_lse


def trie_beam_select_host(cand_edge, cand_total, fin_total, node, path, trie: PhraseTrie, eos: int, ids, hist, pool_phrase, pool_sum,
                          pool_score, pool_len, pool_n, closed, counters, ctrl, W: int, P: int, longest: int, length_penalty: float,
                          close_rule: bool = True, gaps: Optional[list] = None, pool_gaps: Optional[list] = None, plen=None, longest_of=None):
    """One i2t_trie_beam_select call on the host (numpy, in place on the arrays given; fp32 arithmetic in the kernel's order): the
    normative statement of the selection step of ``search_phrases``.  ``cand_edge`` / ``cand_total`` [R, W] and ``fin_total`` [R]:
    ``trie_beam_candidates_host``'s; ``node`` int32 [R], ``path`` f32 [R]; ``ids`` int64 [R, ids_ld]; ``hist`` int32 [R, hist_ld]; the
    pool ``pool_phrase`` int32 / ``pool_sum`` f32 / ``pool_score`` f32 / ``pool_len`` int32 [B, W], ``pool_n`` / ``closed`` int32 [B];
    ``counters`` = [pos, len], ``ctrl`` = [done, open] (``beam_advance_host`` moves both).  The depth is t = len - P; nothing happens
    once ctrl[0] is set, for a closed image, or with t outside 0 .. longest or pos outside the history rows.  Per open image:
      * FINISH: the rows in order; a live row at a node where a phrase ends (term >= 0) offers (term, f = fin_total, s = f /
        fp32(t + 1) ** fp32(length_penalty), t + 1) -- one fp32 power, one fp32 division; the pool keeps the W best of (pool, offers),
        descending by s, an entry it holds before a new one of equal score, an earlier offer before a later one;
      * NEXT ROWS: the W largest child totals of the image's rows, descending, the lower row first and then the lower edge on ties
        (an absent candidate, edge -1, never ranks); child k takes node child_next[e], path = its total, the token child_tok[e] at
        ids[row k][len] and hist[row k][pos] = the parent's row behind the parent's history columns [0, pos); rows without a child
        are dead: node -1, path -inf, the token ``eos`` (a valid id for the next embedding lookup), their own history row;
      * CLOSE: when no row is live; or (``close_rule``) when the pool holds W and not (best / fp32(Lopt) ** fp32(length_penalty) >
        pool_score[W - 1]) with best the largest next total and Lopt = longest + 1 for a penalty >= 0, else t + 2.  Log-probs are
        <= 0 (lse >= max z in fp32 as well, and fp32 addition is monotone), so no continuation of a running row -- its sum at most
        best, its length between t + 2 and longest + 1 -- can score above that bound: every later offer would be refused by the
        full pool.  Closing there never changes the pool; it only saves steps (``close_rule`` False shows it);
      * an image left open sets ctrl[1] = 1.
    ``gaps`` (a list, optional) receives, per image and step, the W-th next total minus the best child total that was left out by
    this merge; ``pool_gaps`` the differences between an offer's score and the pool entries beside it.
    ``plen`` / ``longest_of`` (int [B], optional: ``trie_beam_select_sets_host`` hands them in) replace ``P`` / ``longest`` per image."""
    if ctrl[0]:
        return
    pos, ln = int(counters[0]), int(counters[1])
    R = node.shape[0]
    B = R // W
    sets = plen is not None or longest_of is not None
    f32 = np.float32
    P_all, longest_all = P, longest
    for b in range(B):
        if closed[b]:
            continue
        r0 = b * W
        P = P_all if plen is None else int(plen[b])
        longest = longest_all if longest_of is None else int(longest_of[b])
        t = ln - P
        if sets and t < 0:                                      # a forced column: the identity history column, the search stays open
            if ln < 0 or pos < 0 or pos >= hist.shape[1]:
                continue
            hist[r0:r0 + W, pos] = np.arange(r0, r0 + W)
            ctrl[1] = 1
            continue
        if t < 0 or t > longest or ln >= ids.shape[1] or pos < 0 or pos >= hist.shape[1]:
            continue
        with np.errstate(all='ignore'):
            denom = np.power(f32(t + 1), f32(length_penalty)).astype(f32)
            lopt = np.power(f32(longest + 1 if length_penalty >= 0 else t + 2), f32(length_penalty)).astype(f32)
        m = int(pool_n[b])
        entries = [(f32(pool_score[b, i]), int(pool_phrase[b, i]), f32(pool_sum[b, i]), int(pool_len[b, i])) for i in range(m)]
        for w in range(W):
            nd = int(node[r0 + w])
            if nd < 0 or nd >= trie.nodes or trie.term[nd] < 0:
                continue
            f = f32(fin_total[r0 + w])
            s = f32(f / denom)
            at = 0
            while at < len(entries) and entries[at][0] >= s:
                at += 1
            if pool_gaps is not None:
                pool_gaps.extend(abs(float(entries[i][0]) - float(s)) for i in (at - 1, at) if 0 <= i < len(entries))
            if at >= W:
                continue
            entries.insert(at, (s, int(trie.term[nd]), f, t + 1))
            del entries[W:]
        m = len(entries)
        for i, (s, ph, f, length) in enumerate(entries):
            pool_score[b, i], pool_phrase[b, i], pool_sum[b, i], pool_len[b, i] = s, ph, f, length
        pool_n[b] = m
        flat = [(f32(cand_total[r0 + w, i]), w * W + i, int(cand_edge[r0 + w, i])) for w in range(W) for i in range(W)
                if int(node[r0 + w]) >= 0 and cand_edge[r0 + w, i] >= 0]
        flat.sort(key=lambda c: (-c[0], c[1]))
        children = flat[:W]
        if gaps is not None and len(flat) > W and np.isfinite(flat[W][0]):
            gaps.append(float(children[W - 1][0]) - float(flat[W][0]))
        cl = not children
        if not cl and close_rule and m == W:
            with np.errstate(all='ignore'):
                cl = not (f32(children[0][0] / lopt) > entries[W - 1][0])
        closed[b] = 1 if cl else 0
        if not cl:
            ctrl[1] = 1
        pars = [r0 + c[1] // W for c in children] + [r0 + k for k in range(len(children), W)]
        hist[r0:r0 + W, :pos] = hist[pars, :pos]
        for k in range(W):
            if k < len(children):
                tot, _, e = children[k]
                node[r0 + k], path[r0 + k], ids[r0 + k, ln] = int(trie.child_next[e]), tot, int(trie.child_tok[e])
            else:
                node[r0 + k], path[r0 + k], ids[r0 + k, ln] = -1, -np.inf, eos
            hist[r0 + k, pos] = pars[k]


def trie_beam_select_sets_host(cand_edge, cand_total, fin_total, node, path, trie, eos: int, ids, hist, pool_phrase, pool_sum, pool_score,
                               pool_len, pool_n, closed, counters, ctrl, W: int, P: int, plen, longest_of, length_penalty: float,
                               close_rule: bool = True, gaps: Optional[list] = None, pool_gaps: Optional[list] = None):
    """One i2t_trie_beam_select_sets call on the host: ``trie_beam_select_host`` with image b's depth t = len -
    ``plen[b]`` (``plen`` None: ``P`` for every image) and its own ``longest_of[b]`` in the guard, the close test's optimistic length
    and the column bound.  An image with t < 0 sits in a forced prompt column: nothing of its pool, node, path, closed or ids is
    touched, every row records itself as its parent, hist[r][pos] = r, and ctrl[1] = 1.  ``trie``: a ``PhraseTrie`` or a
    ``PhraseForest`` -- ``term`` then names a phrase within its set."""
    assert longest_of is not None
    trie_beam_select_host(cand_edge, cand_total, fin_total, node, path, trie, eos, ids, hist, pool_phrase, pool_sum, pool_score, pool_len,
                          pool_n, closed, counters, ctrl, W, P, 0, length_penalty, close_rule, gaps, pool_gaps, plen=plen,
                          longest_of=np.asarray(longest_of))


def phrase_beam_search_host(step_logits, prompt, trie: PhraseTrie, eos: int, W: int, N: int, length_penalty: float,
                            close_rule: bool = True, start: int = 0, longest: Optional[int] = None):
    """The whole search of ``search_phrases`` for ONE image on the host: ``step_logits(sequence)`` gives the raw fp32 logits row [V] that
    follows a token sequence (a list of ints, the prompt included).  W rows, each a trie node and an fp32 path sum: row 0 starts at the
    root with path 0, the others dead.  Depth t = 0, 1, ...: ``trie_beam_candidates_host`` over the live rows, one
    ``trie_beam_select_host`` call and ``beam_advance_host``; at most longest + 1 steps.  -> SimpleNamespace(phrase_index int64 [N],
    logprob f32 [N], scores f32 [N], lengths int32 [N]: the first N pool entries; steps; pool_n; gaps, pool_gaps:
    ``trie_beam_select_host``'s, and in ``gaps`` also, per row, the W-th kept child total minus the best one the row dropped).  A
    search whose gaps all exceed a perturbation of the totals keeps its phrases and their order under it.  ``start`` / ``longest``: the
    node row 0 starts at and the longest phrase below it -- the root and the longest phrase of the image's set in a ``PhraseForest``
    (DESIGN.md 4x); 0 / None: a trie's root and its own ``longest``."""
    prompt = [int(t) for t in np.asarray(prompt).reshape(-1)]
    P, longest = len(prompt), int(trie.longest if longest is None else longest)
    assert P >= 1 and 1 <= N <= W
    total = P + longest + 1
    f32, i32 = np.float32, np.int32
    ids = np.zeros((W, total), dtype=np.int64)
    ids[:, :P] = prompt
    hist = np.repeat(np.arange(W, dtype=i32)[:, None], total, axis=1)
    node, path = np.full(W, -1, dtype=i32), np.zeros(W, dtype=f32)
    node[0] = int(start)
    seqs = [list(prompt)] + [None] * (W - 1)
    pool_phrase, pool_sum = np.full((1, W), -1, dtype=i32), np.zeros((1, W), dtype=f32)
    pool_score, pool_len = np.full((1, W), BEAM_DEAD, dtype=f32), np.zeros((1, W), dtype=i32)
    pool_n, closed = np.zeros(1, dtype=i32), np.zeros(1, dtype=i32)
    counters, ctrl = np.array([P - 1, P], dtype=i32), np.zeros(2, dtype=i32)
    gaps, pool_gaps, steps = [], [], 0
    V = None
    while steps < longest + 1 and not ctrl[0]:
        rows = [np.asarray(step_logits(list(seqs[w])), dtype=f32).reshape(-1) if node[w] >= 0 else None for w in range(W)]
        V = next(z.shape[0] for z in rows if z is not None)
        logits = np.stack([z if z is not None else np.zeros(V, dtype=f32) for z in rows])
        cand_edge, cand_total, fin_total, lse = trie_beam_candidates_host(logits, node, path, trie, eos, W)
        for w in range(W):                                      # what a row's own top W hung on
            nd = int(node[w])
            if nd >= 0 and trie.child_off[nd + 1] - trie.child_off[nd] > W:
                rest = [f32(path[w] + f32(logits[w, int(trie.child_tok[e])] - lse[w])) for e in range(int(trie.child_off[nd]), int(trie.child_off[nd + 1]))
                        if e not in cand_edge[w].tolist()]
                gaps.append(float(cand_total[w, W - 1]) - float(max(rest)))
        before = [(int(node[w]), seqs[w]) for w in range(W)]
        ln = int(counters[1])
        trie_beam_select_host(cand_edge, cand_total, fin_total, node, path, trie, eos, ids, hist, pool_phrase, pool_sum, pool_score,
                              pool_len, pool_n, closed, counters, ctrl, W, P, longest, length_penalty, close_rule, gaps, pool_gaps)
        for w in range(W):                                      # the sequence a child row continues: its parent's and its token
            seqs[w] = before[int(hist[w, counters[0]])][1] + [int(ids[w, ln])] if node[w] >= 0 else None
        beam_advance_host(counters, ctrl)
        steps += 1
    assert int(pool_n[0]) >= N
    return SimpleNamespace(phrase_index=pool_phrase[0, :N].astype(np.int64), logprob=pool_sum[0, :N].copy(), scores=pool_score[0, :N].copy(),
                           lengths=pool_len[0, :N].copy(), steps=steps, pool_n=int(pool_n[0]), gaps=gaps, pool_gaps=pool_gaps)
