"""The host side of generate_captions(prompt_lengths=...) that needs no GPU: decoding.apply_finish_rule_ragged -- the
numpy statement of what i2t_caption_finish_ragged does step by step on the device, which the GPU tests use as their expectation -- on
hand-made id tables, and the argument refusals that are raised before any device call."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import (GeneratedCaptions, Sampling, apply_finish_rule, apply_finish_rule_ragged, check_caption_args,
                                     check_ragged_caption_args)

EOS, PAD = 9, 0


@pytest.mark.parametrize('eos,pad', [(EOS, PAD), (EOS, None), (None, None), (None, 7)])
@pytest.mark.parametrize('P', [1, 3])
def test_equal_lengths_are_the_old_rule(P, eos, pad):
    rng = np.random.default_rng(P)
    T, R = 6, 7
    ids = rng.integers(0, 12, size=(R, P + T))
    ids[0, P:] = [1, 2, 3, 4, 5, 6]                              # one row without an EOS: L = P + T
    ids[1, :P] = EOS                                             # an EOS in the prompt
    lp = -rng.random((R, T)).astype(np.float32) - 0.5
    for table in (ids, ids[1:]):                                 # with and without the row that keeps L at P + T
        tlp = lp[-table.shape[0]:]
        want = apply_finish_rule(table, P, eos, pad, tlp)
        got = apply_finish_rule_ragged(table, [P] * table.shape[0], T, eos, pad, tlp)
        for w, g in zip(want, got):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        assert apply_finish_rule_ragged(table, [P] * table.shape[0], T, eos, pad)[2] is None
    assert (ids[1, :P] == EOS).all()                             # the input is left alone


def test_an_eos_inside_the_longer_prompt_does_not_finish_the_row():
    # max_new = 3, lengths (1, 4): row 1 holds EOS at columns 1 and 3 of its PROMPT, where row 0 is already emitting
    ids = np.array([[5, 1, EOS, 8, 8, 8, 8],                     # emits 1, EOS: length 3 (columns past 1 + 3 are not read)
                    [5, EOS, 2, EOS, 4, 6, EOS]])                # emits 4, 6, EOS: length 7
    lp = -np.arange(1, 13, dtype=np.float32).reshape(2, 6)       # column-aligned: entry t belongs to column 1 + t
    out, lengths, olp = apply_finish_rule_ragged(ids, [1, 4], 3, EOS, PAD, lp)
    assert lengths.dtype == np.int32 and lengths.tolist() == [3, 7]
    assert out.tolist() == [[5, 1, EOS, PAD, PAD, PAD, PAD], [5, EOS, 2, EOS, 4, 6, EOS]]
    assert olp.tolist() == [[-1, -2, 0, 0, 0, 0], [0, 0, 0, -10, -11, -12]]          # 0.0 at forced columns and past a row's end


def test_a_row_that_hits_its_budget_early_is_padded_from_there():
    # lengths (1, 3), max_new = 2, no EOS anywhere: row 0 ends at column 3 and is padded to L = 5
    ids = np.array([[5, 1, 2, 77, 78], [5, 6, 7, 3, 4]])
    lp = -np.ones((2, 4), dtype=np.float32)
    out, lengths, olp = apply_finish_rule_ragged(ids, [1, 3], 2, EOS, PAD, lp)
    assert lengths.tolist() == [3, 5]
    assert out.tolist() == [[5, 1, 2, PAD, PAD], [5, 6, 7, 3, 4]]
    assert olp.tolist() == [[-1, -1, 0, 0], [0, 0, -1, -1]]
    # the longest row ends early: L shrinks to the other row's budget
    ids2 = np.array([[5, 1, 2, 77, 78], [5, 6, 7, EOS, 4]])
    out, lengths, olp = apply_finish_rule_ragged(ids2, [1, 3], 2, EOS, None, lp)
    assert lengths.tolist() == [3, 4] and out.tolist() == [[5, 1, 2, EOS], [5, 6, 7, EOS]]          # the default pad is the EOS id
    assert olp.tolist() == [[-1, -1, 0], [0, 0, -1]]
    assert ids2[0, 3] == 77


def test_without_an_eos_id_rows_end_on_their_budget():
    ids = np.array([[5, 1, 2, 77, 78], [5, 6, 7, 3, 4], [5, 6, 1, 2, 79]])
    lp = -np.ones((3, 4), dtype=np.float32)
    out, lengths, olp = apply_finish_rule_ragged(ids, [1, 3, 2], 2, None, None, lp)
    assert lengths.tolist() == [3, 5, 4]
    assert out.tolist() == [[5, 1, 2, 0, 0], [5, 6, 7, 3, 4], [5, 6, 1, 2, 0]]          # no EOS id, no pad id: pad 0
    assert olp.tolist() == [[-1, -1, 0, 0], [0, 0, -1, -1], [0, -1, -1, 0]]
    out, _, _ = apply_finish_rule_ragged(ids, [1, 3, 2], 2, None, 11)
    assert out[0].tolist() == [5, 1, 2, 11, 11]


def test_one_row():
    ids = np.array([[5, 6, 1, EOS, 3]])
    out, lengths, olp = apply_finish_rule_ragged(ids, [2], 3, EOS, PAD, np.array([[-1.0, -2.0, -3.0]]))
    assert lengths.tolist() == [4] and out.tolist() == [[5, 6, 1, EOS]] and olp.tolist() == [[-1.0, -2.0]]
    out, lengths, olp = apply_finish_rule_ragged(ids, np.array([2]), 3, None, PAD, np.array([[-1.0, -2.0, -3.0]]))
    assert lengths.tolist() == [5] and out.tolist() == ids.tolist() and olp.tolist() == [[-1.0, -2.0, -3.0]]


def test_refusals_that_need_no_gpu():
    ok = dict(B=3, P=5, N=1, sampling=None, eos=EOS, pad=None, poll_every=8, max_new_tokens=4)
    for good in ([1, 5, 3], (1, 5, 3), np.array([1, 5, 3]), torch.tensor([1, 5, 3]), torch.tensor([1, 5, 3], dtype=torch.int32)):
        plen = check_ragged_caption_args(good, **ok)
        assert plen.dtype == np.int32 and plen.tolist() == [1, 5, 3]
    with pytest.raises(ValueError, match=r'shape \(2,\)'):
        check_ragged_caption_args([1, 5], **ok)
    with pytest.raises(ValueError, match=r'shape \(3, 1\)'):
        check_ragged_caption_args(torch.tensor([[1], [5], [3]]), **ok)
    with pytest.raises(ValueError, match=r'shape \(\)'):
        check_ragged_caption_args(3, **ok)
    with pytest.raises(ValueError, match=r'prompt_lengths\[1\] = 0'):
        check_ragged_caption_args([1, 0, 3], **ok)
    with pytest.raises(ValueError, match=r'prompt_lengths\[2\] = -4'):
        check_ragged_caption_args([1, 2, -4], **ok)
    with pytest.raises(ValueError, match=r'prompt_lengths\[0\] = 6 exceeds the 5 columns'):
        check_ragged_caption_args([6, 5, 3], **ok)
    with pytest.raises(ValueError, match='integers'):
        check_ragged_caption_args([1.0, 5.0, 3.0], **ok)
    with pytest.raises(ValueError, match='identical'):
        check_ragged_caption_args([1, 5, 3], **dict(ok, N=2))    # greedy with N > 1, as without lengths
    check_ragged_caption_args([1, 5, 3], **dict(ok, N=2, sampling=Sampling(0.7, None, 0.6)))
    for bad in (dict(N=0), dict(eos=-2), dict(pad=-1), dict(poll_every=-1), dict(max_new_tokens=-1), dict(sampling=Sampling(0.0, 5))):
        with pytest.raises(ValueError):
            check_ragged_caption_args([1, 5, 3], **dict(ok, **bad))
    check_caption_args(1, None, None, None, 0, 0)                # the old function takes what it took


def test_the_result_type_keeps_its_four_fields():
    """prompt_lengths rides beside the tuple: four fields unpack and construct positionally as before, a fifth argument is taken"""
    a, b, c, d = (torch.zeros(1) for _ in range(4))
    out = GeneratedCaptions(a, b, c, d)
    assert out.prompt_lengths is None and len(out) == 4 and out.ids is a and out.logprob is d
    ids, lengths, lp, total = out
    assert ids is a and total is d
    plen = torch.ones(1, dtype=torch.int32)
    out = GeneratedCaptions(a, b, c, d, plen)
    assert out.prompt_lengths is plen and len(out) == 4 and GeneratedCaptions(a, b, c, d, prompt_lengths=plen).prompt_lengths is plen
    assert GeneratedCaptions(ids=a, lengths=b, token_logprobs=c, logprob=d).lengths is b


def test_model_refuses_before_touching_the_device():
    """bad lengths, greedy with N > 1 and a request past the text window are refused on a CPU model: no kernel has run by then; the
    window is measured from the LONGEST prompt in use, not from the columns of prompt_ids"""
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import tiny_config
    m = VisionEncoderDecoder(tiny_config())
    images, prompt = torch.zeros(2, 3, 32, 32), torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match=r'prompt_lengths\[1\] = 5 exceeds the 4 columns'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, prompt_lengths=[1, 5])
    with pytest.raises(ValueError, match=r'prompt_lengths\[0\] = 0'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, prompt_lengths=torch.tensor([0, 2]))
    with pytest.raises(ValueError, match='shape'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, prompt_lengths=[1, 2, 3])
    with pytest.raises(ValueError, match='identical'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, num_return_sequences=2, prompt_lengths=[1, 2])
    window = m.decoder.block_size - m.space_for_prompt
    with pytest.raises(ValueError, match=rf'prompt \+ new tokens \({window + 1}\) exceed the text window \({window}\)'):
        m.generate_captions(images, prompt, max_new_tokens=window - 2, top_k=1, prompt_lengths=[1, 3])
