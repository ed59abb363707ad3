"""Phrase sets as token tries: the CSR trie ``generate_captions(phrases=...)`` walks on the device and the per-depth
tables ``score_phrases`` walks level by level, for one set or for a set per image.  Host only (numpy; torch only to accept tensors of ids); ``decoding`` re-exports every name."""
from typing import NamedTuple, Optional

import numpy as np
import torch


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


class PhraseForest(NamedTuple):
    """S phrase sets as ONE flat CSR (``phrase_forest``): the sets' tries laid end to end, so the device kernels -- which
    index nodes blindly -- walk it as they walk a trie; a row that starts at ``roots[s]`` never leaves set s.  All arrays numpy int32.
    It has what the drivers and the host statements read of a ``PhraseTrie``: ``nodes``, ``edges``, ``children``, ``max_fanout``."""
    child_off: np.ndarray               # [nodes + 1]
    child_tok: np.ndarray               # [edges]: ascending within a node
    child_next: np.ndarray              # [edges]: a node of the same set
    term: np.ndarray                    # [nodes]: the index WITHIN ITS SET of the phrase that ends at the node (the lowest among duplicates), or -1
    roots: np.ndarray                   # [S]: the root of set s; roots[0] == 0
    longest: np.ndarray                 # [S]: the tokens of set s's longest phrase
    widest: np.ndarray                  # [S]: the nodes of set s's widest level (the root's level counts)
    max_fanout: int                     # the largest number of children of a node, over all sets
    distinct: np.ndarray                # [S]: the distinct phrases of set s

    @property
    def nodes(self) -> int:
        return int(self.term.shape[0])

    @property
    def edges(self) -> int:
        return int(self.child_tok.shape[0])

    @property
    def sets(self) -> int:
        return int(self.roots.shape[0])

    def children(self, node: int):
        """-> (tokens, next nodes) of ``node``"""
        lo, hi = int(self.child_off[node]), int(self.child_off[node + 1])
        return self.child_tok[lo:hi], self.child_next[lo:hi]


def widest_level(trie, root: int = 0) -> int:
    """the largest number of nodes at one depth below ``root`` (the root's level counts: at least 1)"""
    widest, level = 1, [int(root)]
    while level:
        widest = max(widest, len(level))
        level = [int(c) for nd in level for c in trie.children(nd)[1]]
    return widest


def phrase_forest(sets, eos, vocab: int, max_new_tokens: int = 1 << 30) -> PhraseForest:
    """``sets``: S >= 1 phrase sets, each what ``phrase_trie`` takes -> their tries laid end to end (set 0 first, so its root is node 0
    and a one-set forest has ``phrase_trie``'s arrays element for element).  ValueError: no set; whatever ``phrase_trie`` refuses about
    set s, in its words behind 'phrase_sets[s]: '.  ``max_new_tokens`` is held against EVERY set here; a caller that knows which sets
    are in use (``caption_plan``) leaves the default and checks those alone."""
    if isinstance(sets, torch.Tensor):
        sets = sets.detach().cpu().tolist()
    sets = list(sets)
    if not sets:
        raise ValueError('phrase_sets is empty: at least one set is needed')
    tries = []
    for s, one in enumerate(sets):
        try:
            tries.append(phrase_trie(one, eos, vocab, max_new_tokens))
        except ValueError as e:
            raise ValueError(f'phrase_sets[{s}]: {e}') from None
    i32 = np.int32
    node0 = np.cumsum([0] + [t.nodes for t in tries])
    edge0 = np.cumsum([0] + [t.edges for t in tries])
    off = np.concatenate([t.child_off[:-1].astype(np.int64) + edge0[s] for s, t in enumerate(tries)] + [edge0[-1:]]).astype(i32)
    tok = np.concatenate([t.child_tok for t in tries]).astype(i32)
    nxt = np.concatenate([t.child_next.astype(np.int64) + node0[s] for s, t in enumerate(tries)]).astype(i32)
    term = np.concatenate([t.term for t in tries]).astype(i32)
    return PhraseForest(off, tok, nxt, term, node0[:-1].astype(i32), np.array([t.longest for t in tries], dtype=i32),
                        np.array([widest_level(t) for t in tries], dtype=i32), max(t.max_fanout for t in tries),
                        np.array([int((t.term >= 0).sum()) for t in tries], dtype=i32))


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


class SetLevelTables(NamedTuple):
    """The ``level_expand_tables`` of S phrase sets laid end to end (``set_level_tables``): segment g = level_at[s] + t
    holds level t of set s.  All arrays numpy int32."""
    child_parent: np.ndarray            # [n_child_all]
    child_tok: np.ndarray               # [n_child_all]
    term_row: np.ndarray                # [n_term_all]
    term_off: np.ndarray                # [n_term_all + segments]: a segment's n_term + 1 offsets, absolute into term_phrase
    term_phrase: np.ndarray             # [the phrases of all sets]: a phrase's index WITHIN ITS SET
    child_at: np.ndarray                # [segments]: where the segment's children start in child_parent / child_tok
    n_child: np.ndarray                 # [segments]
    term_at: np.ndarray                 # [segments]: where its terminal rows start in term_row
    n_term: np.ndarray                  # [segments]
    off_at: np.ndarray                  # [segments]: where its offsets start in term_off
    level_at: np.ndarray                # [S + 1]: set s's levels are segments level_at[s] .. level_at[s + 1]
    levels: tuple                       # S ``TrieLevels``
    wmax: int                           # the widest level over all sets: the rows per image of the walk
    kmax: int                           # the phrases of the largest set
    lengths: np.ndarray                 # [S, kmax]: the tokens of phrase k of set s + 1, 0 in the padding


def set_level_tables(tries) -> SetLevelTables:
    """``tries``: S >= 1 ``PhraseTrie`` (with ``phrase_node``) -> every set's per-level tables end to end"""
    i32 = np.int32
    cp, ct, tr, to, tp = [], [], [], [], []
    seg = {k: [] for k in ('child_at', 'n_child', 'term_at', 'n_term', 'off_at')}
    level_at, all_levels = [0], []
    n_c = n_t = n_o = n_p = 0
    kmax = max(int(t.phrase_node.shape[0]) for t in tries)
    lengths = np.zeros((len(tries), kmax), dtype=i32)
    for s, trie in enumerate(tries):
        levels = trie_levels(trie)
        all_levels.append(levels)
        depth = np.zeros(trie.nodes, dtype=i32)
        for t, lv in enumerate(levels.levels):
            depth[lv.nodes] = t
            a, b, c, d, e = level_expand_tables(trie, levels, t)
            for k, v in zip(seg, (n_c, a.shape[0], n_t, c.shape[0], n_o)):
                seg[k].append(v)
            cp.append(a), ct.append(b), tr.append(c), to.append(d.astype(np.int64) + n_p), tp.append(e)
            n_c, n_t, n_o, n_p = n_c + a.shape[0], n_t + c.shape[0], n_o + d.shape[0], n_p + e.shape[0]
        lengths[s, :trie.phrase_node.shape[0]] = depth[trie.phrase_node] + 1
        level_at.append(level_at[-1] + len(levels.levels))
    cat = lambda parts: np.concatenate(parts).astype(i32)
    return SetLevelTables(cat(cp), cat(ct), cat(tr), cat(to), cat(tp), *(np.array(seg[k], dtype=i32) for k in seg), np.array(level_at, dtype=i32),
                          tuple(all_levels), max(lv.wmax for lv in all_levels), kmax, lengths)


def set_step_state(tabs: SetLevelTables, set_index, plen, prompts, col: int) -> np.ndarray:
    """int32 [B, 8]: every image's state at the walk step that writes id column ``col`` (i2t_trie_level_expand_sets
    reads it).  Image b, whose prompt is ``prompts[b, :plen[b]]`` and whose set is ``set_index[b]``, is FORCED while col < plen[b] (level
    -1, the token prompts[b, col]), at level t = col - plen[b] of its set while t <= the set's longest phrase (the segment's ranges),
    else FINISHED (level -1, token -1).  Columns: level, forced token, child start, children, terminal start, terminal rows, offset
    start, ``col``."""
    B = len(set_index)
    st = np.zeros((B, 8), dtype=np.int32)
    st[:, 0], st[:, 1], st[:, 7] = -1, -1, col
    for b in range(B):
        s, t = int(set_index[b]), col - int(plen[b])
        if t < 0:
            st[b, 1] = int(prompts[b][col])
        elif t < len(tabs.levels[s].levels):
            g = int(tabs.level_at[s]) + t
            st[b, :7] = (t, -1, tabs.child_at[g], tabs.n_child[g], tabs.term_at[g], tabs.n_term[g], tabs.off_at[g])
    return st
