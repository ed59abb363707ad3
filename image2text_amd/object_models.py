"""Output records: VisionEncoderDecoder.forward's (same field names as the reference's object_models.py:4-5) and
VisionEncoderDecoder.score's (an addition: the reference has no scoring call)."""
from typing import NamedTuple

import torch


class VisionEncoderDecoderModelOutput(NamedTuple):
    encoder_output: torch.Tensor
    logits: torch.Tensor
    hidden_state: torch.Tensor


class CaptionScores(NamedTuple):
    token_logprobs: torch.Tensor      # [B, T] f32: log p(labels[b, t] | image b, ids[b, :t + 1]); 0 where the label is ignored
    lse: torch.Tensor                 # [B, T] f32: logsumexp of the position's logits / temperature
    logprob: torch.Tensor             # [B] f32: the row sums of token_logprobs
