"""The host side of VisionEncoderDecoder.generate_captions that needs no GPU: decoding.apply_finish_rule -- the numpy statement of the
finish rule i2t_caption_finish applies step by step on the device, which the GPU tests use as their expectation -- on hand-made id
streams, and the argument refusals that are raised before any device call."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import GeneratedCaptions, Sampling, apply_finish_rule, check_caption_args

EOS, PAD = 9, 0


def test_eos_at_the_first_step():
    ids = np.array([[5, 6, EOS, 3, 4, 7]])                       # P = 2: the first emitted token is EOS
    lp = np.array([[-1.0, -2.0, -3.0, -4.0]])
    out, lengths, olp = apply_finish_rule(ids, 2, EOS, PAD, lp)
    assert lengths.dtype == np.int32 and lengths.tolist() == [3]
    assert out.tolist() == [[5, 6, EOS]]                         # L = lengths.max(): the EOS is kept, nothing follows
    assert olp.tolist() == [[-1.0]]                              # the EOS keeps its log-prob


def test_eos_never():
    ids = np.array([[5, 1, 2, 3, 4], [6, 4, 3, 2, 1]])
    lp = -np.arange(8, dtype=np.float32).reshape(2, 4) - 1
    out, lengths, olp = apply_finish_rule(ids, 1, EOS, PAD, lp)
    assert lengths.tolist() == [5, 5] and np.array_equal(out, ids) and np.array_equal(olp, lp)
    out, lengths, olp = apply_finish_rule(ids, 1, None, None, lp)             # no rule at all
    assert lengths.tolist() == [5, 5] and np.array_equal(out, ids) and np.array_equal(olp, lp)


def test_eos_in_the_prompt_only_does_not_finish_the_row():
    ids = np.array([[EOS, 1, 2, 3], [EOS, EOS, 4, 5]])           # P = 2 (BOS = EOS, as GPT-2 has it): only emitted tokens count
    out, lengths, _ = apply_finish_rule(ids, 2, EOS, PAD)
    assert lengths.tolist() == [4, 4] and np.array_equal(out, ids)
    out, lengths, _ = apply_finish_rule(np.array([[EOS, 1, EOS, 3]]), 1, EOS, PAD)
    assert lengths.tolist() == [3] and out.tolist() == [[EOS, 1, EOS]]


def test_rows_finish_at_different_steps():
    ids = np.array([[5, 1, EOS, 3, 4, 2, 2],
                    [5, EOS, 1, EOS, 4, 2, 2],                   # the FIRST emitted EOS ends the row
                    [5, 1, 2, 3, EOS, 2, 2],
                    [5, 1, 2, EOS, EOS, 2, 2]])
    lp = -np.ones((4, 6), dtype=np.float32)
    out, lengths, olp = apply_finish_rule(ids, 1, EOS, PAD, lp)
    assert lengths.tolist() == [3, 2, 5, 4]
    assert out.tolist() == [[5, 1, EOS, PAD, PAD], [5, EOS, PAD, PAD, PAD], [5, 1, 2, 3, EOS], [5, 1, 2, EOS, PAD]]      # L = 5
    assert olp.tolist() == [[-1, -1, 0, 0], [-1, 0, 0, 0], [-1, -1, -1, -1], [-1, -1, -1, 0]]
    assert (olp.sum(-1) == -(lengths - 1)).all()
    # the default pad is the EOS id; one unfinished row keeps L at P + T
    out, lengths, _ = apply_finish_rule(np.vstack([ids, [[5, 1, 2, 3, 4, 6, 7]]]), 1, EOS)
    assert lengths.tolist() == [3, 2, 5, 4, 7] and out.shape == (5, 7)
    assert out[0].tolist() == [5, 1, EOS, EOS, EOS, EOS, EOS] and out[4].tolist() == [5, 1, 2, 3, 4, 6, 7]
    assert ids[0, 3] == 3                                         # the input is left alone


def test_refusals_that_need_no_gpu():
    with pytest.raises(ValueError, match='identical'):
        check_caption_args(3, None, EOS, None, 8, 16)            # greedy with N > 1
    check_caption_args(3, Sampling(0.7, None, 0.6), EOS, None, 8, 16)
    check_caption_args(1, None, None, None, 0, 0)
    for bad in (dict(N=0), dict(eos=-2), dict(pad=-1), dict(poll_every=-1), dict(max_new_tokens=-1), dict(sampling=Sampling(0.0, 5))):
        kw = dict(N=1, sampling=None, eos=EOS, pad=None, poll_every=8, max_new_tokens=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_caption_args(**kw)


def test_model_refuses_before_touching_the_device():
    """greedy with N > 1 and a request past the text window are refused on a CPU model: no kernel has run by then"""
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import tiny_config
    m = VisionEncoderDecoder(tiny_config())
    images, prompt = torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, dtype=torch.long)
    with pytest.raises(ValueError, match='identical'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, num_return_sequences=2)
    window = m.decoder.block_size - m.space_for_prompt
    with pytest.raises(ValueError, match='text window'):
        m.generate_captions(images, prompt, max_new_tokens=window, top_k=1)
    assert GeneratedCaptions._fields == ('ids', 'lengths', 'token_logprobs', 'logprob')
