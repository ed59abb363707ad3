"""The host side of generate_captions(prompt_prefill=...), written out: ``prefill_plan`` -- how many prompt columns go
through one forward pass, where the counters start, and what is refused -- and ``kv_prefill_host``, the numpy statement of what
i2t_kv_prefill scatters, on a hand-written table of two images in both cache layouts.  No device."""
import numpy as np
import pytest

from image2text_amd.decoding import PROMPT_PREFILL_MODES, kv_prefill_host, prefill_plan

FAM = object()          # any nano-mini family spec: prefill_plan only asks whether there is one


def test_the_plan_written_out():
    assert PROMPT_PREFILL_MODES == ('steps', 'pass')
    # (mode, pmin, prefix, fam, causal) -> (m, (pos, len))
    table = [
        # dense decoder, no prefix: 'steps' starts at slot 0, column 1 and replays pmin - 1 prefill steps; 'pass' starts behind them
        (('steps', 6, 0, None, True), (0, (0, 1))),
        (('pass', 6, 0, None, True), (5, (5, 6))),
        (('pass', 2, 0, None, True), (1, (1, 2))),
        # prefixed (Hugging Face decoder + soft prompt of 4 rows): the text follows the prefix in the cache
        (('steps', 6, 4, None, True), (0, (4, 1))),
        (('pass', 6, 4, None, True), (5, (9, 6))),
        # Pmin = 1: nothing to prefill, 'pass' IS 'steps'
        (('steps', 1, 0, None, True), (0, (0, 1))),
        (('pass', 1, 0, None, True), (0, (0, 1))),
        (('pass', 1, 4, None, True), (0, (4, 1))),
        # the family under 'steps' is untouched
        (('steps', 6, 0, FAM, True), (0, (0, 1))),
        # a non-causal decoder has no cache: the mode is checked and ignored, family or not
        (('steps', 6, 0, None, False), (0, (0, 1))),
        (('pass', 6, 0, None, False), (0, (0, 1))),
        (('pass', 6, 4, FAM, False), (0, (4, 1))),
    ]
    for args, want in table:
        assert prefill_plan(*args) == want, args
    for pmin in range(1, 9):
        for prefix in (0, 3):
            m, (pos, ln) = prefill_plan('pass', pmin, prefix, None, True)
            assert m == pmin - 1 and pos == prefix + m and ln == 1 + m
            assert pmin - 1 - m == 0                                         # prefill replays left
            assert prefill_plan('steps', pmin, prefix, None, True) == (0, (prefix, 1))


def test_refusals():
    for causal in (True, False):
        with pytest.raises(ValueError, match="prompt_prefill = 'graph'"):
            prefill_plan('graph', 6, 0, None, causal)
    with pytest.raises(ValueError, match='prompt_prefill = None'):
        prefill_plan(None, 6, 0, None, True)
    with pytest.raises(NotImplementedError, match='nano-mini decoder family: a sparse layer caches the positions it keeps by slot'):
        prefill_plan('pass', 6, 0, FAM, True)
    with pytest.raises(NotImplementedError, match="use 'steps'"):
        prefill_plan('pass', 1, 0, FAM, True)                                # refused whatever the prompt length
    with pytest.raises(ValueError, match='pmin = 0'):
        prefill_plan('pass', 0, 0, None, True)


def _source():
    """2 images x 3 source tokens (src_T = 3), rows of 8 columns: q | k | v with w = 2, heads of width 1 -- element = 100 row + column"""
    return (100 * np.arange(6)[:, None] + np.arange(8)[None, :]).astype(np.int64)


def test_scatter_head_major_by_hand():
    """B = 2, N = 2, Hkv = 2, hd = 1, clen = 3: tokens 1, 2 of every image (src_t0 = 1, m = 2) into slots 1, 2.  Cache [R][H][clen][hd]."""
    src = _source()
    R, H, clen, hd = 4, 2, 3, 1
    kc, vc = np.full(R * H * clen * hd, -1, dtype=np.int64), np.full(R * H * clen * hd, -1, dtype=np.int64)
    kv_prefill_host(src, 2, 4, 3, 1, 2, kc, vc, H * clen * hd, hd, clen * hd, hd, 2, 1, 2, 2)
    # image 0: source rows 1, 2 -> K columns 2 | 3 = (102, 103), (202, 203); image 1: rows 4, 5 -> (402, 403), (502, 503)
    img0_k = [[-1, 102, 202], [-1, 103, 203]]           # [head][slot]
    img1_k = [[-1, 402, 502], [-1, 403, 503]]
    assert kc.reshape(R, H, clen).tolist() == [img0_k, img0_k, img1_k, img1_k]
    img0_v = [[-1, 104, 204], [-1, 105, 205]]
    img1_v = [[-1, 404, 504], [-1, 405, 505]]
    assert vc.reshape(R, H, clen).tolist() == [img0_v, img0_v, img1_v, img1_v]


def test_scatter_row_major_by_hand():
    """the same table into the row-major cache [R][clen][w]: cache_rs = w, cache_hs = hd; all three tokens into slots 0 .. 2 of 4"""
    src = _source()
    R, clen, w, hd = 4, 4, 2, 1
    kc, vc = np.full(R * clen * w, -1, dtype=np.int64), np.full(R * clen * w, -1, dtype=np.int64)
    kv_prefill_host(src, 2, 4, 3, 0, 3, kc, vc, clen * w, w, hd, hd, w, 0, 2, 2)
    img0_k = [[2, 3], [102, 103], [202, 203], [-1, -1]]             # [slot][column]
    img1_k = [[302, 303], [402, 403], [502, 503], [-1, -1]]
    assert kc.reshape(R, clen, w).tolist() == [img0_k, img0_k, img1_k, img1_k]
    img0_v = [[4, 5], [104, 105], [204, 205], [-1, -1]]
    img1_v = [[304, 305], [404, 405], [504, 505], [-1, -1]]
    assert vc.reshape(R, clen, w).tolist() == [img0_v, img0_v, img1_v, img1_v]
    # N = 1, one image, a later slot: nothing but that slot of row 0 is written
    kc[:] = -1
    vc[:] = -1
    kv_prefill_host(src, 2, 4, 3, 2, 1, kc, vc, clen * w, w, hd, hd, w, 3, 1, 1)
    want = np.full((R, clen, w), -1)
    want[0, 3] = (202, 203)
    assert np.array_equal(kc.reshape(R, clen, w), want)
