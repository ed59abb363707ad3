"""Output records: VisionEncoderDecoder.forward's (same field names as the reference's object_models.py:4-5) and
VisionEncoderDecoder.score's (an addition: the reference has no scoring call)."""
from typing import NamedTuple, Optional

import torch


class VisionEncoderDecoderModelOutput(NamedTuple):
    encoder_output: torch.Tensor
    logits: torch.Tensor
    hidden_state: torch.Tensor


class _CaptionScoreFields(NamedTuple):
    token_logprobs: torch.Tensor      # [B, T] f32: log p(labels[b, t] | image b, ids[b, :t + 1]); 0 where the label is ignored
    lse: torch.Tensor                 # [B, T] f32: logsumexp of the position's logits / temperature
    logprob: torch.Tensor             # [B] f32: the row sums of token_logprobs


class CaptionScores(_CaptionScoreFields):
    """What ``score`` returns.  The three fields above are the tuple: it unpacks into three and ``_fields`` names three, as before
    ``top_logprobs`` existed.  Under ``top_logprobs`` = K > 0 the four attributes below stand beside them, as
    ``caption_plan.GeneratedCaptions`` carries its additions; all four are None without the argument.  ``_replace`` and ``_make`` build
    the three fields only."""
    top_tokens: Optional[torch.Tensor] = None       # int32 [B, T, K]: the K best tokens of v = logits / temperature, (v descending, id ascending)
    top_logprobs: Optional[torch.Tensor] = None     # fp32 [B, T, K]: their log-probs v[token] - lse
    token_entropy: Optional[torch.Tensor] = None    # fp32 [B, T]: the entropy of softmax(v), in nats
    label_rank: Optional[torch.Tensor] = None       # int32 [B, T]: the columns strictly ahead of the label (0: the arg-max); -1 where ignored

    def __new__(cls, token_logprobs, lse, logprob, top_tokens=None, top_logprobs=None, token_entropy=None, label_rank=None):
        self = super().__new__(cls, token_logprobs, lse, logprob)
        self.top_tokens, self.top_logprobs, self.token_entropy, self.label_rank = top_tokens, top_logprobs, token_entropy, label_rank
        return self
