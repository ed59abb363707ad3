"""Host-side pieces of caption scoring: the label shift of VisionEncoderDecoder.score, the EOS masking of generation_utils.rerank
and the output record."""
import torch

from image2text_amd.models.generation_utils import post_eos_positions, rerank_labels
from image2text_amd.models.vision_encoder_decoder import next_token_labels
from image2text_amd.object_models import CaptionScores


def test_next_token_labels():
    ids = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])
    lab = next_token_labels(ids, -100)
    assert lab.tolist() == [[6, 7, 8, -100], [2, 3, 4, -100]]
    assert lab.dtype == ids.dtype and ids.tolist() == [[5, 6, 7, 8], [1, 2, 3, 4]]          # the input is left alone
    assert next_token_labels(ids, -1)[:, -1].tolist() == [-1, -1]


def test_next_token_labels_single_column():
    ids = torch.tensor([[9], [3]])
    assert next_token_labels(ids, -100).tolist() == [[-100], [-100]]


def test_post_eos_positions():
    eos = 9
    ids = torch.tensor([[9, 1, 2, 9, 4, 9],      # BOS = EOS in column 0 is the prompt: the first EOS is column 3
                        [9, 1, 2, 3, 4, 5],      # no EOS
                        [9, 9, 2, 3, 4, 5],      # EOS straight after the prompt
                        [9, 1, 2, 3, 4, 9]])     # EOS in the last column
    got = post_eos_positions(ids, eos)
    assert got.tolist() == [[False, False, False, False, True, True],
                            [False] * 6,
                            [False, False, True, True, True, True],
                            [False] * 6]
    assert not post_eos_positions(ids, None).any()
    assert post_eos_positions(ids, eos, prompt_len=0)[1].tolist() == [False, True, True, True, True, True]
    assert ids[0].tolist() == [9, 1, 2, 9, 4, 9]


def test_rerank_labels():
    eos, ig = 9, -100
    ids = torch.tensor([[9, 1, 2, 9, 4, 9],
                        [9, 1, 2, 3, 4, 5]])
    assert rerank_labels(ids, eos).tolist() == [[1, 2, 9, ig, ig, ig], [1, 2, 3, 4, 5, ig]]       # the first EOS itself is scored
    assert rerank_labels(ids, None).tolist() == [[1, 2, 9, 4, 9, ig], [1, 2, 3, 4, 5, ig]]
    assert rerank_labels(ids, eos, prompt_len=2).tolist() == [[ig, 2, 9, ig, ig, ig], [ig, 2, 3, 4, 5, ig]]      # prompt tokens are not scored


def test_caption_scores_record():
    assert CaptionScores._fields == ('token_logprobs', 'lse', 'logprob')
    r = CaptionScores(torch.zeros(2, 3), torch.ones(2, 3), torch.zeros(2))
    assert r.lse is r[1] and r.logprob.shape == (2,)
