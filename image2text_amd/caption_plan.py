"""What a decoding call means, decided on the host before anything runs: the argument tuples (``Sampling``, ``Processors``, ``BeamSpec``),
the window and cache planners, the refusals of ``generate_captions`` / ``score_phrases`` / ``search_phrases`` and -- composing them -- ``plan_captions``, the
one function that resolves a ``generate_captions`` call into a ``CaptionPlan``; the result tuples and the graph key beside them.  numpy,
and torch only to accept tensors; no device, engine or library.  ``decoding`` re-exports every name."""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .phrase_trie import PhraseForest, PhraseTrie, phrase_forest, phrase_node_csr, phrase_trie, widest_level


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
LONG_CHUNK_KEYS = 256               # = ops.LONG_CHUNK_KEYS, which this module does not import (decoding.py holds the two equal)
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

    image_index: Optional[torch.Tensor] = None      # int32 [Q] under ``image_index``: the image query q was asked of -- every
                                                    # "B" above is then Q, the queries; None without the argument

    # under ``top_logprobs`` = K > 0, all three aligned by column as ``token_logprobs`` is; None without the argument.  A cell
    # no step wrote -- a row's prompt columns under ``prompt_lengths``, columns past its end -- holds -1 / 0.0 / 0.0.
    top_tokens: Optional[torch.Tensor] = None       # int32 [B, N, L - Pmin, K]: the K best tokens of the step's raw row, (z descending, id ascending)
    top_logprobs: Optional[torch.Tensor] = None     # fp32 [B, N, L - Pmin, K]: their log-probs, ``token_logprobs``' quantity at those tokens
    token_entropy: Optional[torch.Tensor] = None    # fp32 [B, N, L - Pmin]: the entropy of the step's raw distribution, in nats

    def __new__(cls, ids, lengths, token_logprobs, logprob, prompt_lengths=None, beam_scores=None, phrase_index=None, image_index=None,
                top_tokens=None, top_logprobs=None, token_entropy=None):
        self = super().__new__(cls, ids, lengths, token_logprobs, logprob)
        self.prompt_lengths = prompt_lengths
        self.beam_scores = beam_scores
        self.phrase_index = phrase_index
        self.image_index = image_index
        self.top_tokens, self.top_logprobs, self.token_entropy = top_tokens, top_logprobs, token_entropy
        return self


def check_image_index(image_index, Q: int, images: Optional[int] = None) -> Optional[np.ndarray]:
    """What ``image_index`` refuses about itself (host only, ValueError, read before anything moves to the device) -> the
    table, int32 [Q], or None without the argument: query q is ``prompt_ids[q]`` asked of image ``image_index[q]``.  ``Q``: the rows of
    ``prompt_ids``; ``images``: the images of the call (None: a caller that does not know them checks no range and no count).  In this
    order: a non-integer dtype; a shape other than (Q,); a value outside [0, images).  Without the argument, Q != images: row b of
    ``prompt_ids`` is then asked of image b.  Before this check the drivers sized everything by Q and never compared it with the
    images (DESIGN.md 4ac says what each call then did): with fewer prompts than images the cross K/V GEMM took the first Q images'
    encoder rows and the others were dropped without a word; with more it ran over Q * S rows of an operand that holds images * S."""
    if image_index is None:
        if images is not None and int(images) != Q:
            raise ValueError(f'{Q} prompts for {int(images)} images: without image_index row b of prompt_ids is asked of image b, so there is one '
                             f'prompt per image; image_index (one image per prompt, shape ({Q},), values in [0, {int(images)})) asks several '
                             f'prompts of one image')
        return None
    if isinstance(image_index, torch.Tensor):
        if image_index.is_floating_point() or image_index.is_complex() or image_index.dtype == torch.bool:
            raise ValueError(f'image_index of dtype {image_index.dtype}: integers are needed')
        index = image_index.detach().cpu().numpy()
    else:
        index = np.asarray(image_index)
        if index.dtype == np.bool_ or (index.size and not np.issubdtype(index.dtype, np.integer)):
            raise ValueError(f'image_index of type {index.dtype}: integers are needed')
    if index.shape != (Q,):
        raise ValueError(f'image_index of shape {tuple(index.shape)} for prompt_ids of {Q} rows: one image per prompt, shape ({Q},)')
    if images is not None and Q and (int(index.min()) < 0 or int(index.max()) >= int(images)):
        bad = int(np.flatnonzero((index < 0) | (index >= int(images)))[0])
        raise ValueError(f'image_index[{bad}] = {int(index[bad])} is outside the {int(images)} images: [0, {int(images)})')
    if images is None and Q and int(index.min()) < 0:
        raise ValueError(f'image_index[{int(index.argmin())}] = {int(index.min())}: an image index cannot be negative')
    return index.astype(np.int32)


def row_images(image_index: Optional[np.ndarray], per: int) -> Optional[np.ndarray]:
    """The row -> image table of a call whose R = Q * ``per`` rows are query-major -- (query, n) or (query, w) --, int32 [R]: what the
    drivers upload into st.mem_index; None without ``image_index``"""
    return None if image_index is None else np.repeat(np.asarray(image_index, dtype=np.int32), int(per))


def refuse_image_index_prefill(image_index, prompt_prefill: str, causal: bool = True):
    """``image_index`` with ``prompt_prefill='pass'`` (NotImplementedError; a non-causal decoder has no cache and ignores the mode)"""
    if image_index is not None and prompt_prefill == 'pass' and causal:
        raise NotImplementedError("image_index with prompt_prefill='pass': the prefill pass is one causal sequence per IMAGE, and a prompt per "
                                  "query needs that pass per query over gathered encoder outputs, which is not built; use 'steps'")


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


MAX_TOP_LOGPROBS = 8                # i2t_caption_top_logprobs keeps a thread's K best in 8 register pairs (csrc/decode.hip::TOPLP_MAXK)


def check_top_logprobs(top_logprobs, vocab: int) -> int:
    """The refusals of ``top_logprobs`` about itself (host only, ValueError) -> K, 0 for the call without the argument.
    In this order: not a whole number (a bool is not one); outside 0 .. MAX_TOP_LOGPROBS; more alternatives than the vocabulary holds."""
    K = top_logprobs
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)):
        raise ValueError(f'top_logprobs = {K!r}: a whole number of alternatives per step, from 0 (none) to {MAX_TOP_LOGPROBS}')
    if not 0 <= int(K) <= MAX_TOP_LOGPROBS:
        raise ValueError(f'top_logprobs = {int(K)}: from 0 (none) to {MAX_TOP_LOGPROBS} alternatives per step (the kernel keeps a thread\'s best in '
                         f'{MAX_TOP_LOGPROBS} register pairs)')
    if int(K) > vocab:
        raise ValueError(f'top_logprobs = {int(K)} alternatives of a vocabulary of {vocab} tokens')
    return int(K)


def check_score_top_logprobs(top_logprobs, temperature, vocab: int) -> int:
    """The refusals of ``score(..., top_logprobs=K)`` (host only, ValueError) -> K, 0 for the call without the argument:
    ``check_top_logprobs``' about K itself, then -- with K > 0 only, the call without the argument keeps taking what it took -- a
    temperature that is not a finite positive number: the kernel scales the row by fp32(1 / temperature) and refuses anything else."""
    K = check_top_logprobs(top_logprobs, vocab)
    if K:
        try:
            t = float(temperature)
        except (TypeError, ValueError):
            t = float('nan')
        # (fp32's range: the smallest subnormal and the largest finite number)
        if not (math.isfinite(t) and t > 0 and 2.0 ** -149 <= 1.0 / t <= (2.0 - 2.0 ** -23) * 2.0 ** 127):
            raise ValueError(f'temperature = {temperature!r} with top_logprobs = {K}: a finite positive number whose reciprocal is one in fp32 '
                             f'(the rows are scaled by fp32(1 / temperature))')
    return K


def caption_graph_key(head, eos, pad, ragged_max_new: Optional[int] = None, proc: Optional[Processors] = None, P: int = 0, trie: bool = False,
                      sets: bool = False, top_logprobs: int = 0):
    """The graph key of a ``generate_captions`` full step: everything a captured step holds as a kernel argument.  (head, eos, pad), or
    ('ragged', head, eos, pad, max_new) under ``prompt_lengths`` -- and with active processors ('proc', theta, min_new, n_suppress, P,
    ...that key): an inactive call never sees a 'proc' key.  ``P``: the prompt length the min-length count starts from (0 when ragged:
    the count then reads the device's table).  ``trie`` (a ``phrases`` call): ('trie', eos, ...that key) -- the trie's
    contents live in device buffers the step only points at, so they are no part of it; a call without phrases never sees a 'trie' key.
    ``sets`` (a ``phrase_sets`` call): ('trie_sets', eos, ...the ragged or plain key) -- the forest, the start nodes and the
    prompt lengths are device tables; a call without ``phrase_sets`` never sees a 'trie_sets' key.  ``top_logprobs`` = K > 0 (DESIGN.md
    4ad): (...that key, whichever of the above it is, 'top_logprobs', K) -- K is a kernel argument and the step points at the three result
    buffers; the pair stands at the END, so the key still starts with the tag of every other buffer the step points at (_drop_graphs);
    K = 0 leaves every key above as it is."""
    key = (head, eos, pad) if ragged_max_new is None else ('ragged', head, eos, pad, ragged_max_new)
    key = key if proc is None else ('proc',) + proc.key() + (0 if ragged_max_new is not None else int(P),) + key
    if sets:
        key = ('trie_sets', eos) + key
    elif trie:
        key = ('trie', eos) + key
    return tuple(key) + ('top_logprobs', int(top_logprobs)) if top_logprobs else key


def phrase_beam_sets_graph_key(pmax: int, W: int, eos: int, length_penalty: float):
    """The graph key of a ``search_phrases(phrase_sets=...)`` full step: the longest prompt, W, eos and the penalty are
    kernel arguments; every image's prompt length and longest phrase are device tables, so they are no part of it."""
    return ('phrase_beam_sets', int(pmax), int(W), int(eos), float(length_penalty))


class PhraseSets(NamedTuple):
    """``phrase_sets`` / ``phrase_set_index`` of a call, checked (``check_phrase_sets``)."""
    forest: PhraseForest
    index: np.ndarray                   # int32 [B]: image b answers from set index[b]
    roots: np.ndarray                   # int32 [B]: forest.roots[index]
    longest: np.ndarray                 # int32 [B]: forest.longest[index]
    widest: int                         # the widest level over the sets in use
    smallest: int                       # the fewest distinct phrases of a set in use


def check_phrase_sets(phrases, phrase_sets, phrase_set_index, B: int, eos, vocab: int) -> PhraseSets:
    """What ``phrase_sets`` / ``phrase_set_index`` refuse about themselves (host only, ValueError), in this order: ``phrase_set_index``
    without ``phrase_sets``; ``phrases`` given too; no set, or what ``phrase_trie`` refuses about set s in its own words behind
    'phrase_sets[s]: ' (``phrase_forest``); an index that is not one whole number per image; ``phrase_set_index`` None with S != B; an
    index outside [0, S)."""
    if phrase_sets is None:
        raise ValueError('phrase_set_index without phrase_sets: it names a set of phrase_sets per image')
    if phrases is not None:
        raise ValueError('phrases and phrase_sets are both given: one set for all images, or phrase_sets with a set per image')
    forest = phrase_forest(phrase_sets, eos, vocab)
    S = forest.sets
    if phrase_set_index is None:
        if S != B:
            raise ValueError(f'phrase_set_index = None needs one set per image: {S} sets for {B} images')
        index = np.arange(B, dtype=np.int64)
    else:
        if isinstance(phrase_set_index, torch.Tensor):
            if phrase_set_index.is_floating_point() or phrase_set_index.is_complex() or phrase_set_index.dtype == torch.bool:
                raise ValueError(f'phrase_set_index of dtype {phrase_set_index.dtype}: integers are needed')
            index = phrase_set_index.detach().cpu().numpy()
        else:
            index = np.asarray(phrase_set_index)
            if index.size and not np.issubdtype(index.dtype, np.integer):
                raise ValueError(f'phrase_set_index of type {index.dtype}: integers are needed')
        if index.shape != (B,):
            raise ValueError(f'phrase_set_index of shape {tuple(index.shape)} for {B} images: one set index per image, shape ({B},)')
        if B and (int(index.min()) < 0 or int(index.max()) >= S):
            bad = int(np.flatnonzero((index < 0) | (index >= S))[0])
            raise ValueError(f'phrase_set_index[{bad}] = {int(index[bad])} is outside the {S} sets of phrase_sets: [0, {S})')
    index = index.astype(np.int32)
    used = np.unique(index)
    return PhraseSets(forest, index, forest.roots[index].astype(np.int32), forest.longest[index].astype(np.int32),
                      int(forest.widest[used].max()) if used.size else 1, int(forest.distinct[used].min()) if used.size else 0)


class ClosedSet(NamedTuple):
    """The phrases of a closed-set call, whichever way the caller named them (``closed_set``): ``phrases``, one set for all images -- a
    forest of one whose root is node 0 --, or ``phrase_sets`` / ``phrase_set_index``, a set per image.  The drivers
    take this record; only ``per_image`` decides which entry points, graph key and result type they use."""
    trie: object                        # the ``PhraseTrie`` / ``PhraseForest`` whose arrays go to the device
    roots: np.ndarray                   # int32 [B]: the node image b starts at
    longest: np.ndarray                 # int32 [B]: the tokens of the longest phrase image b may answer
    plen: Optional[np.ndarray]          # int32 [B] under ``prompt_lengths``, else None: every prompt fills all P columns
    widest: Optional[int]               # the widest level over the sets in use; None for one set, which ``widest_level`` counts when asked
    distinct: int                       # the distinct phrases of the set -- of the smallest set in use
    tries: Optional[tuple]              # every set's own ``PhraseTrie``, which ``score_phrases`` walks; None where no one asked for them
    index: np.ndarray                   # int32 [B]: image b answers from set index[b]
    per_image: bool                     # the call came through ``phrase_sets``
    image_index: Optional[np.ndarray] = None    # int32 [Q] under ``image_index``: every "B" above is then Q, the queries

    @property
    def sets(self) -> PhraseSets:
        return PhraseSets(self.trie, self.index, self.roots, self.longest, self.widest, self.distinct)

    def widest_level(self) -> int:
        return widest_level(self.trie) if self.widest is None else self.widest


def one_closed_set(trie: PhraseTrie, B: int) -> ClosedSet:
    """a checked ``PhraseTrie`` as the record of a call on B images"""
    none = np.zeros(B, dtype=np.int32)
    return ClosedSet(trie, none, np.full(B, trie.longest, dtype=np.int32), None, None, int((trie.term >= 0).sum()), (trie,), none, False)


def per_image_closed_set(sets: PhraseSets, plen=None, tries=None) -> ClosedSet:
    """checked ``PhraseSets`` (and prompt lengths int32 [B], and the sets' own tries) as the record of a call"""
    return ClosedSet(sets.forest, sets.roots, sets.longest, plen, sets.widest, sets.smallest, tries, sets.index, True)


def held_phrase_trie(trie: PhraseTrie, eos, vocab: int, max_new_tokens: Optional[int] = None) -> PhraseTrie:
    """A ``PhraseTrie`` that an earlier call built (the model hands its own to the decoder) is not built again, only held against this
    call's ``eos`` and ``vocab`` -- and, in ``generate_captions`` alone, ``max_new_tokens`` -> the trie, or ValueError."""
    if eos is None or not 0 <= int(eos) < vocab or trie.edges < 1 or int(trie.child_tok.min()) < 0 or int(trie.child_tok.max()) >= vocab \
            or bool((trie.child_tok == int(eos)).any()) or (max_new_tokens is not None and max_new_tokens < trie.longest + 1):
        raise ValueError(f'a PhraseTrie built for another call: eos_token_id = {eos}, vocabulary {vocab}' + (
            '' if max_new_tokens is None else f', max_new_tokens = {max_new_tokens} against a longest phrase of {trie.longest} tokens'))
    return trie


def closed_set(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab: int, B: int, P: int, max_new_tokens: Optional[int] = None,
               tries: bool = False, per_image: Optional[bool] = None) -> ClosedSet:
    """The phrase arguments of a call on ``prompt_ids`` [B, P], resolved (host only, ValueError).  With any of ``phrase_sets`` /
    ``phrase_set_index`` / ``prompt_lengths`` (or ``per_image``, which overrides that test): ``check_phrase_sets``' refusals, then
    ``prompt_lengths``' own (``check_ragged_caption_args``' texts); ``tries`` asks for every set's own trie.  Else ``phrases``, one set
    for all images: ``phrase_trie``'s refusals, or ``held_phrase_trie``'s; ``max_new_tokens`` (``generate_captions``) is held against
    this one set alone -- a caller with sets knows which are in use and checks those."""
    if (phrase_sets is not None or phrase_set_index is not None or prompt_lengths is not None) if per_image is None else per_image:
        sets = check_phrase_sets(phrases, phrase_sets, phrase_set_index, B, eos, vocab)
        if tries:
            each = phrase_sets.detach().cpu().tolist() if isinstance(phrase_sets, torch.Tensor) else phrase_sets
            tries = tuple(phrase_trie(one, eos, vocab, 1 << 30) for one in each)
        return per_image_closed_set(sets, None if prompt_lengths is None else _prompt_lengths(prompt_lengths, B, P), tries or None)
    if isinstance(phrases, PhraseTrie):
        return one_closed_set(held_phrase_trie(phrases, eos, vocab, max_new_tokens), B)
    return one_closed_set(phrase_trie(phrases, eos, vocab, 1 << 30 if max_new_tokens is None else max_new_tokens), B)


def _refuse_caption_combinations(name: str, processors_active, num_beams, causal: bool):
    """what ``phrases`` / ``phrase_sets`` (``name``) do not combine with in ``generate_captions`` (NotImplementedError): an active logits
    processor -- ``processors_active`` may be a callable, asked only here --, ``num_beams`` > 1, a non-causal decoder"""
    if processors_active() if callable(processors_active) else processors_active:
        raise NotImplementedError(f'{name} with repetition_penalty / min_new_tokens / suppress_tokens: the phrase set says what may be '
                                  'emitted, and a processor could leave a node without an allowed token')
    if isinstance(num_beams, (int, np.integer)) and not isinstance(num_beams, bool) and num_beams > 1:
        raise NotImplementedError(f'{name} under num_beams > 1: the beam step has no trie state per hypothesis')
    if not causal:
        raise NotImplementedError(f'{name} run inside the KV-cache caption step; a non-causal decoder generates by re-evaluation '
                                  '(generate_by_recompute), which has no constrained step')


def check_phrase_set_caption_args(phrases, phrase_sets, phrase_set_index, B: int, eos, vocab: int, max_new_tokens: int,
                                  processors_active=False, num_beams=1, causal: bool = True) -> PhraseSets:
    """``check_phrase_sets``, then ``max_new_tokens`` below the longest phrase of a set in use + 1 (ValueError), then what
    ``phrase_sets`` does not combine with in ``generate_captions`` (NotImplementedError, naming the reason): an active logits
    processor, ``num_beams`` > 1, a non-causal decoder.  ``prompt_lengths`` is NOT among them.  ``processors_active``
    may be a callable: it is asked only once the ValueErrors above have passed."""
    one = closed_set(phrases, phrase_sets, phrase_set_index, None, eos, vocab, B, 0, per_image=True)
    longest = int(one.longest.max()) if B else 1
    if max_new_tokens < longest + 1:
        raise ValueError(f'max_new_tokens = {max_new_tokens} is below the longest phrase + 1 = {longest + 1} of the sets in use: every row '
                         f'ends with EOS')
    _refuse_caption_combinations('phrase_sets', processors_active, num_beams, causal)
    return one.sets


def check_phrase_caption_args(phrases, eos, vocab: int, max_new_tokens: int, prompt_lengths=None, processors_active: bool = False,
                              num_beams=1, causal: bool = True) -> PhraseTrie:
    """``phrase_trie`` and then what ``phrases`` does not combine with, all before anything runs -> the trie.  NotImplementedError,
    naming the reason: ``prompt_lengths``, an active logits processor, ``num_beams`` > 1, a non-causal decoder.  ``phrases`` may be a
    ``PhraseTrie`` that an earlier call of this function built (the model hands its own to the decoder): it is not built again, only
    held against this call's ``eos``, ``vocab`` and ``max_new_tokens``."""
    one = closed_set(phrases, None, None, None, eos, vocab, 1, 0, max_new_tokens, per_image=False)
    if prompt_lengths is not None:
        raise NotImplementedError('phrases with prompt_lengths: a forced prompt column would have to hold the trie still, and the ragged '
                                  'finish rule has no such case')
    _refuse_caption_combinations('phrases', processors_active, num_beams, causal)
    return one.trie


class _PhraseScoreFields(NamedTuple):
    logprob: torch.Tensor               # fp32 [B, K]: the raw log-likelihood of phrase k + EOS after image b's prompt (``score``'s quantity)
    best: torch.Tensor                  # int64 [B]: the argmax over k, the lowest index on ties (duplicate phrases tie exactly)
    lengths: torch.Tensor               # int32 [K]: the tokens of each phrase + 1 (the EOS)


class _ImageIndexed:
    """``image_index`` (int32 [Q], or None without the argument) as an attribute BESIDE a result tuple, the optional last
    argument of its constructor -- ``GeneratedCaptions.prompt_lengths``' way: the tuple unpacks as before and ``_fields`` names what it named."""
    image_index: Optional[torch.Tensor] = None

    def __new__(cls, *fields, image_index=None):
        self = super().__new__(cls, *fields)
        self.image_index = image_index
        return self


class PhraseScores(_ImageIndexed, _PhraseScoreFields):
    """What ``score_phrases`` returns; with ``image_index`` every B is Q, the queries, and the attribute ``image_index`` holds the table."""


class _PhraseSetScoreFields(NamedTuple):
    logprob: torch.Tensor               # fp32 [B, Kmax], Kmax the phrases of the largest set: column k < K_s the raw log-likelihood of phrase k of
                                        # the image's own set + EOS after its own prompt (``score``'s quantity), -inf in columns k >= K_s
    best: torch.Tensor                  # int64 [B]: the argmax within the image's own set, the lowest index on ties (duplicates tie exactly)
    lengths: torch.Tensor               # int32 [S, Kmax]: the tokens of phrase k of set s + 1 (the EOS), 0 in the padding


class PhraseSetScores(_ImageIndexed, _PhraseSetScoreFields):
    """What ``score_phrases(phrase_sets=...)`` returns; ``image_index`` as in ``PhraseScores``."""


def plan_phrase_scores(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab: int, B: int, P: int, window: int, causal: bool = True,
                       sparse: bool = False, images_per_pass=None, per_image: Optional[bool] = None, image_index=None,
                       images: Optional[int] = None) -> ClosedSet:
    """The refusals of ``score_phrases`` on ``prompt_ids`` [B, P], all before anything runs (host only) -> the call's ``ClosedSet``, with
    every set's own trie.  ValueError, in this order: ``prompt_lengths`` without ``phrase_sets``, or no phrases at all; ``closed_set``'s
    (the set or sets, the index, then ``prompt_lengths``' own); a held ``PhraseTrie`` without ``phrase_node``.  Then NotImplementedError,
    naming the reason, for a non-causal decoder and for sparse nano-mini blocks; then ValueError for the largest p_b + longest phrase of
    b's set + 1 past the decode ``window`` (the text of every other call) and for ``images_per_pass`` < 1.  ``image_index`` / ``images``
    (DESIGN.md 4ac): ``check_image_index``' refusals come first; B is then Q, the queries, and the record carries the table."""
    index = check_image_index(image_index, B, images)
    if phrase_sets is None and phrase_set_index is None and prompt_lengths is not None:
        raise ValueError('score_phrases(prompt_lengths=...) needs phrase_sets: one phrase list for all images is '
                         'phrase_sets=[phrases], phrase_set_index=[0] * B')
    if phrases is None and phrase_sets is None and phrase_set_index is None and not per_image:
        raise ValueError('score_phrases needs phrases or phrase_sets')
    one = closed_set(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab, B, P, tries=True, per_image=per_image)
    if not one.per_image:
        phrase_node_csr(one.trie)
    rows = np.full(B, int(P), dtype=np.int64) if one.plen is None else one.plen.astype(np.int64)
    total = int((rows + one.longest + 1).max()) if B else int(P)
    if not causal:
        raise NotImplementedError('score_phrases walks the trie on the KV cache; a non-causal decoder has none -- every new token changes the '
                                  'state of the earlier ones --, so use rerank')
    if sparse:
        raise NotImplementedError('score_phrases on sparse nano-mini decoder blocks: a sparse layer caches the positions it keeps by slot, and '
                                  'the static per-level history tables have not been run through its slot table (slot_pos); use rerank')
    if total > window:
        raise ValueError(f'prompt + new tokens ({total}) exceed the text window ({window})')
    if images_per_pass is not None and (isinstance(images_per_pass, bool) or int(images_per_pass) != images_per_pass or int(images_per_pass) < 1):
        raise ValueError(f'images_per_pass = {images_per_pass!r}: a whole number of images, at least 1')
    return one if index is None else one._replace(image_index=index)


def check_phrase_score_args(phrases, eos, vocab: int, P: int, window: int, causal: bool = True, sparse: bool = False,
                            images_per_pass=None) -> PhraseTrie:
    """``plan_phrase_scores`` of ``phrases``, one set for all images, with its refusals in its order -> the trie"""
    return plan_phrase_scores(phrases, None, None, None, eos, vocab, 1, P, window, causal, sparse, images_per_pass).trie


def check_phrase_set_score_args(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab: int, B: int, P: int, window: int,
                                causal: bool = True, sparse: bool = False, images_per_pass=None):
    """``plan_phrase_scores`` of ``phrase_sets`` / ``phrase_set_index`` / ``prompt_lengths``, with its refusals in its
    order -> (the S sets' ``PhraseTrie``, index int32 [B], plen int32 [B] or None)"""
    one = plan_phrase_scores(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab, B, P, window, causal, sparse, images_per_pass,
                             per_image=True)
    return one.tries, one.index, one.plen


class _PhraseBeamFields(NamedTuple):
    phrase_index: torch.Tensor          # int64 [B, N]: the index into ``phrases``; among duplicates the one the trie's ``term`` holds (the lowest)
    logprob: torch.Tensor               # fp32 [B, N]: the raw log-likelihood of phrase + EOS after image b's prompt (``score``'s quantity)
    scores: torch.Tensor                # fp32 [B, N]: logprob / (tokens + 1) ** length_penalty, the sort key; at penalty 0.0 it equals logprob
    lengths: torch.Tensor               # int32 [B, N]: the tokens of the phrase + 1 (the EOS)
    exhaustive: bool                    # num_beams >= the widest trie level: nothing was pruned, the result is the exact top N of the set


class PhraseBeams(_ImageIndexed, _PhraseBeamFields):
    """What ``search_phrases`` returns: the N best phrases of the set per image, best first; ``image_index`` as in
    ``PhraseScores``."""


trie_widest_level = widest_level        # the largest number of nodes at one depth of a trie (the root's level counts: at least 1)


def plan_phrase_search(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab: int, B: int, P: int, window: int, num_beams=4,
                       num_return_sequences=1, length_penalty=0.0, poll_every=8, causal: bool = True, sparse: bool = False, image_index=None,
                       images: Optional[int] = None):
    """The refusals of ``search_phrases`` on ``prompt_ids`` [B, P], all before anything runs (host only) -> (the call's ``ClosedSet``, W,
    N).  ValueError, in this order: ``prompt_lengths`` without ``phrase_sets`` (the forced column is ``phrase_sets``' rule), or no phrases
    at all; ``closed_set``'s about the set or sets and the index; ``num_beams`` outside 1 .. MAX_CAPTION_BEAMS; ``num_return_sequences``
    outside 1 .. min(num_beams, distinct phrases -- of the smallest set in use); a non-finite ``length_penalty``; ``prompt_lengths``' own
    refusals (``check_ragged_caption_args``' texts), which stand behind those of N and the penalty; the longest prompt + the longest phrase in
    use + 1 past the decode ``window`` (the text of every other call); a negative ``poll_every``.  NotImplementedError, naming the
    reason: a non-causal decoder, sparse nano-mini blocks.  ``image_index`` / ``images``: ``check_image_index``' refusals
    come first; B is then Q, the queries, and the record carries the table."""
    index = check_image_index(image_index, B, images)
    if phrase_sets is None and phrase_set_index is None:
        if prompt_lengths is not None:
            raise ValueError('search_phrases(prompt_lengths=...) needs phrase_sets: one answer list for all images is '
                             'phrase_sets=[answers], phrase_set_index=[0] * B')
        if phrases is None:
            raise ValueError('search_phrases needs phrases or phrase_sets')
    one = closed_set(phrases, phrase_sets, phrase_set_index, None, eos, vocab, B, P)
    if isinstance(num_beams, bool) or int(num_beams) != num_beams or not 1 <= int(num_beams) <= MAX_CAPTION_BEAMS:
        raise ValueError(f'num_beams = {num_beams!r}: a whole number from 1 to {MAX_CAPTION_BEAMS} (the trie beam kernels keep at most '
                         f'{MAX_CAPTION_BEAMS} rows per image)')
    W = int(num_beams)
    N = num_return_sequences
    if isinstance(N, bool) or int(N) != N or not 1 <= int(N) <= min(W, one.distinct):
        raise ValueError(f'num_return_sequences = {N!r} with num_beams = {W} and {one.distinct} distinct phrases: from 1 to '
                         f'{min(W, one.distinct)} phrases per image')
    try:
        finite = bool(np.isfinite(float(length_penalty)))
    except (TypeError, ValueError):
        finite = False
    if not finite:
        raise ValueError(f'length_penalty = {length_penalty!r}: a finite number is needed')
    if prompt_lengths is not None:
        one = one._replace(plen=_prompt_lengths(prompt_lengths, B, P))
    total = (int(P) if one.plen is None else int(one.plen.max())) + int(one.longest.max()) + 1
    if total > window:
        raise ValueError(f'prompt + new tokens ({total}) exceed the text window ({window})')
    if isinstance(poll_every, bool) or int(poll_every) != poll_every or int(poll_every) < 0:
        raise ValueError(f'poll_every = {poll_every!r}: it may not be negative')
    if not causal:
        raise NotImplementedError('search_phrases runs its beam over the trie on the KV cache; a non-causal decoder has none -- every new '
                                  'token changes the state of the earlier ones --, so use rerank')
    if sparse:
        raise NotImplementedError('search_phrases on sparse nano-mini decoder blocks: a sparse layer caches the positions it keeps by slot, '
                                  'and the trie beam step has not been run through its slot table (slot_pos); use rerank')
    return (one if index is None else one._replace(image_index=index)), W, int(N)


def check_phrase_search_args(phrases, eos, vocab: int, P: int, window: int, num_beams=4, num_return_sequences=1, length_penalty=0.0,
                             poll_every=8, causal: bool = True, sparse: bool = False, phrase_sets=None, phrase_set_index=None,
                             prompt_lengths=None, B: Optional[int] = None):
    """``plan_phrase_search`` under the name and with the results it had before ``ClosedSet``: (trie, W, N) of a call with ``phrases``,
    (``PhraseSets``, W, N, plen int32 [B] or None) of one with ``phrase_sets`` / ``phrase_set_index`` / ``prompt_lengths`` (``B``: the
    images).  New code calls ``plan_phrase_search``, which returns one shape."""
    one, W, N = plan_phrase_search(phrases, phrase_sets, phrase_set_index, prompt_lengths, eos, vocab, 1 if B is None else B, P, window,
                                   num_beams, num_return_sequences, length_penalty, poll_every, causal, sparse)
    return (one.sets, W, N, one.plen) if one.per_image else (one.trie, W, N)


def check_caption_args(N: int, sampling: Optional[Sampling], eos, pad, poll_every: int, max_new_tokens: int, repetition_penalty: float = 1.0,
                       min_new_tokens: int = 0, suppress_tokens=None, vocab: Optional[int] = None, formed=None):
    """the refusals of generate_captions that need no device; those of the logits processors are ``caption_processors``' (``formed``:
    what ``plan_captions`` hands every check in its place -- it enters ``caption_processors`` once per call and yields the result)"""
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
    formed() if formed is not None else caption_processors(repetition_penalty, min_new_tokens, suppress_tokens, max_new_tokens, eos, vocab)


def check_ragged_caption_args(prompt_lengths, B: int, P: int, N: int, sampling: Optional[Sampling], eos, pad, poll_every: int,
                              max_new_tokens: int, **processors) -> np.ndarray:
    """check_caption_args, and the refusals of ``prompt_lengths`` (read on the host, before anything moves to the device): one integer
    per image, 1 <= p_b <= P  -> the lengths, int32 [B]"""
    check_caption_args(N, sampling, eos, pad, poll_every, max_new_tokens, **processors)
    return _prompt_lengths(prompt_lengths, B, P)


def _prompt_lengths(prompt_lengths, B: int, P: int) -> np.ndarray:
    """the refusals of ``prompt_lengths`` itself -> int32 [B]"""
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
                            suppress_tokens=None, max_new_tokens=1, eos=None, pad=None, poll_every=8, causal=True, vocab=None, formed=None) -> int:
    """The refusals of ``generate_captions(num_beams=W, ...)`` that need no device, all before anything runs -> W.  W = 1 is the call
    without the beam arguments: only W itself, ``length_penalty`` and ``early_stopping`` are looked at.  ValueError: W outside
    1 .. MAX_CAPTION_BEAMS (the candidates kernel takes E = 2 W <= 16), N outside 1 .. W, a non-finite ``length_penalty``,
    ``early_stopping`` not False / True ("never" is out of scope), any sampling argument (beam sampling is out of scope), a negative
    id or count.  NotImplementedError, naming the reason: ``prompt_lengths``, ``prompt_prefill='pass'``, an active
    ``repetition_penalty`` / ``min_new_tokens`` / ``suppress_tokens``, a non-causal decoder.  ``formed``: as in ``check_caption_args``."""
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
    if (formed() if formed is not None else caption_processors(repetition_penalty, min_new_tokens, suppress_tokens, max_new_tokens, eos, vocab)) is not None:
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


# ------------------------------------------------------------------------------------------------ one plan per call
class CaptionFacts(NamedTuple):
    """What ``plan_captions`` and the checks of the phrase calls need to know of the model."""
    V: int                              # the vocabulary
    causal: bool                        # False: no cache, the call runs by re-evaluation
    fam: object                         # the nano-mini family's spec, as ``prefill_plan`` takes it (None: a dense or Llama-family decoder)
    window: int                         # the text window: decoder.block_size - space_for_prompt
    prefix: int                         # the soft-prompt rows at the head of the cache: min(ncls, block) when the decoder is prefixed, else 0
    # what ``check_phrase_score_args`` / ``check_phrase_search_args`` take (``plan_captions`` reads neither; the defaults are a hand-made record's)
    cache_window: Optional[int] = None  # min(window, decode_window) on a causal decoder, else window
    sparse: bool = False                # sparse nano-mini decoder blocks


class CaptionPlan(NamedTuple):
    """What a ``generate_captions`` call is, every argument checked and resolved (``plan_captions``): the drivers run it as it stands."""
    mode: str                           # 'cache' (CaptionDecoder), 'beam' (CaptionBeamDecoder), 'recompute' (a non-causal decoder)
    N: int                              # captions per image
    W: int                              # beams per image (1: no beam search)
    sampling: Optional[Sampling]        # None: greedy
    eos: Optional[int]
    pad: int                            # resolved: the EOS id by default, 0 without one
    poll_every: int
    max_new: int
    plen: Optional[np.ndarray]          # int32 [B] under ``prompt_lengths``, else None
    pmin: int                           # the shortest and the longest prompt (both P without ``prompt_lengths``)
    pmax: int
    prompt_prefill: str
    m: int                              # ``prefill_plan``'s: the prompt columns one forward pass takes ...
    start: tuple                        # ... and the (pos, len) the counters start at
    proc: Optional[Processors]          # None: no logits processor is active
    trie: Optional[PhraseTrie]          # None: no ``phrases``
    length_penalty: float
    early_stopping: bool
    sets: Optional[PhraseSets] = None   # ``phrase_sets``: the forest, every image's set, root and longest phrase; None: no sets
    image_index: Optional[np.ndarray] = None    # int32 [Q] under ``image_index``: every "per image" above is then per query
    top_logprobs: int = 0               # K alternatives and the entropy per step; 0: the call without the argument

    @property
    def rows_per_query(self) -> int:
        return self.W if self.mode == 'beam' else self.N

    @property
    def row_images(self) -> Optional[np.ndarray]:
        """the row -> image table of the call's R = Q * rows_per_query rows (query-major), int32 [R]; None without ``image_index``"""
        return row_images(self.image_index, self.rows_per_query)


def plan_captions(facts: CaptionFacts, B: int, P: int, max_new_tokens=128, eos_token_id=None, pad_token_id=None, num_return_sequences=1,
                  temperature=1.0, top_k=None, nucleus_p=None, seed=None, poll_every=8, prompt_lengths=None, prompt_prefill='steps',
                  repetition_penalty=1.0, min_new_tokens=0, suppress_tokens=None, num_beams=1, length_penalty=1.0, early_stopping=False,
                  phrases=None, phrase_sets=None, phrase_set_index=None, *, sampling=..., image_index=None,
                  images: Optional[int] = None, top_logprobs=0) -> CaptionPlan:
    """The one place that says what ``generate_captions(...)`` on ``prompt_ids`` [B, P] means, or refuses it: the arguments are the model
    method's (``sampling``: the decoders' keyword methods hand their ``Sampling`` or None in place of the four sampling arguments).
    Refusals come in this order, the first that applies wins: ``phrase_sets`` / ``phrase_set_index``
    (``check_phrase_set_caption_args``: its ValueErrors, then the logits processors' own, then its NotImplementedErrors); ``phrases``
    (``check_phrase_caption_args``, behind the logits processors' own ValueErrors); the beam arguments (``check_beam_caption_args``); under num_beams = W > 1 the text window, then 2 W > V; else
    ``check_caption_args`` / ``check_ragged_caption_args``; an active processor on a non-causal decoder; ``prefill_plan``'s; the text
    window.  At W = 1 only ``num_beams``, ``length_penalty`` and ``early_stopping`` are looked at among the beam arguments.
    ``image_index`` / ``images`` (``images``: the images of the call, None: unknown): ``check_image_index``' ValueErrors
    come before everything above -- B is then Q, the queries, in all of it --, and its one NotImplementedError,
    ``prompt_prefill='pass'``, after everything above; the plan carries the table.
    ``top_logprobs`` = K: ``check_top_logprobs``' ValueErrors come right behind ``check_image_index``' and before everything
    else; with K > 0 a NotImplementedError under num_beams > 1 right behind the beam arguments' own refusals (before the beam window), and
    one on a non-causal decoder behind the processors' refusal there (before ``prefill_plan``'s).  Every K > 0 plan is a 'cache' plan; K = 0
    is the call without the argument."""
    eos, pad, formed = eos_token_id, pad_token_id, []
    index = check_image_index(image_index, B, images)
    K = check_top_logprobs(top_logprobs, facts.V)

    def processors():                   # caption_processors, entered once, by the first check that reaches it: its refusals keep their place
        if not formed:
            formed.append(caption_processors(repetition_penalty, min_new_tokens, suppress_tokens, max_new_tokens, eos, facts.V))
        return formed[0]
    procs = dict(repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens, vocab=facts.V,
                 formed=processors)
    trie = sets = None
    if phrase_sets is not None or phrase_set_index is not None:
        sets = check_phrase_set_caption_args(phrases, phrase_sets, phrase_set_index, B, eos, facts.V, max_new_tokens,
                                             lambda: processors() is not None, num_beams, facts.causal)
    elif phrases is not None:           # before the beam checks: those keep their own texts
        trie = check_phrase_caption_args(phrases, eos, facts.V, max_new_tokens, prompt_lengths, processors() is not None, num_beams,
                                         facts.causal)
    W = check_beam_caption_args(num_beams, num_return_sequences, length_penalty, early_stopping, temperature=temperature, top_k=top_k,
                                nucleus_p=nucleus_p, seed=seed, prompt_lengths=prompt_lengths, prompt_prefill=prompt_prefill,
                                max_new_tokens=max_new_tokens, eos=eos, pad=pad, poll_every=poll_every, causal=facts.causal, **procs)
    N = int(num_return_sequences)
    if W > 1 and K:
        raise NotImplementedError('top_logprobs under num_beams > 1: the beam step\'s quantity is the row AFTER the n-gram ban, and its rows are '
                                  'reordered between steps, so no column of the result would belong to one hypothesis')
    if W > 1:
        if P + max_new_tokens > facts.window:
            raise ValueError(f'prompt + new tokens ({P + max_new_tokens}) exceed the text window ({facts.window})')
        if W * 2 > facts.V:
            raise ValueError(f'num_beams = {W} needs 2 * num_beams candidates per row: the vocabulary holds {facts.V} tokens')
        return CaptionPlan('beam', N, W, None, eos, int((0 if eos is None else eos) if pad is None else pad), poll_every, max_new_tokens, None,
                           P, P, prompt_prefill, 0, (facts.prefix, 1), None, None, float(length_penalty), bool(early_stopping), None, index)
    if sampling is ...:
        sampling = None if (top_k == 1 and nucleus_p is None) else Sampling(temperature, top_k, nucleus_p, seed)
    if prompt_lengths is None:
        check_caption_args(N, sampling, eos, pad, poll_every, max_new_tokens, **procs)
        plen, pmin, pmax = None, P, P
    else:
        plen = check_ragged_caption_args(prompt_lengths, B, P, N, sampling, eos, pad, poll_every, max_new_tokens, **procs)
        pmin, pmax = int(plen.min()), int(plen.max())
    proc = processors()
    if not facts.causal and proc is not None:
        raise NotImplementedError('repetition_penalty / min_new_tokens / suppress_tokens run inside the KV-cache caption step; a non-causal '
                                  'decoder generates by re-evaluation (generate_by_recompute), which has no processed step')
    if not facts.causal and K:
        raise NotImplementedError('top_logprobs runs inside the KV-cache caption step; a non-causal decoder generates by re-evaluation '
                                  '(generate_by_recompute), whose loop has no such step')
    m, start = prefill_plan(prompt_prefill, pmin, facts.prefix, facts.fam, facts.causal)
    if pmax + max_new_tokens > facts.window:
        raise ValueError(f'prompt + new tokens ({pmax + max_new_tokens}) exceed the text window ({facts.window})')
    refuse_image_index_prefill(index, prompt_prefill, facts.causal)
    return CaptionPlan('cache' if facts.causal else 'recompute', N, 1, sampling, eos, (0 if eos is None else eos) if pad is None else pad,
                       poll_every, max_new_tokens, plen, pmin, pmax, prompt_prefill, m, start, proc, trie, float(length_penalty),
                       bool(early_stopping), sets, index, K)

