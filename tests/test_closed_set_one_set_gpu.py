"""One phrase set named two ways: ``phrases=X`` against ``phrase_sets=[X], phrase_set_index=[0] * B``, bit for bit.

The three closed-set calls -- ``generate_captions`` (greedy), ``search_phrases`` and ``score_phrases`` -- reach the same device
arithmetic whichever way the caller names the set: a one-set forest has ``phrase_trie``'s arrays element for element, the walk kernels
share ``expand_value`` and the candidate / select bodies, and every image's prompt fills all P columns.  So the two forms promise equal
bits, not close values: integer fields are held with ``torch.equal``, float fields as their int32 bit patterns.  The models are the tiny
dense one and the tiny Llama of tests/test_decode_launches_gpu.py, B = 3 images behind a prompt of 3 tokens; X holds four phrases of 1
to 3 tokens, three of which share their first token and one of which is a prefix of another (widest trie level: 3 nodes).
``search_phrases`` runs at W = 2, which prunes, and at W = 3, the widest level, which does not."""
import pytest
import torch

from image2text_amd.decoding import phrase_trie, trie_widest_level
from image2text_amd.synth import synthetic_batch, tiny_config
from test_generate_captions_gpu import _ved

pytestmark = pytest.mark.gpu

B, P = 3, 3
EOS = 5
X = [[17], [17, 42], [17, 9, 30], [63, 8]]
SETS = dict(phrase_sets=[X], phrase_set_index=[0] * B)


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module', params=['tiny', 'llama'])
def model(request, tiny_weights, tmp_path_factory):
    """-> (model, images [3, ...], prompt [3, 3])"""
    if request.param == 'llama':
        from test_hf_decoder_gpu import _llama_model
        mp = pytest.MonkeyPatch()
        request.addfinalizer(mp.undo)
        _, m, _, V = _llama_model(tmp_path_factory.mktemp('llama'), mp, 'llama')
        m = m.to(dev()).eval()
        g = torch.Generator().manual_seed(8)
        images, prompt = torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, V, (B, P), generator=g)
    else:
        m = _ved(tiny_config(), tiny_weights)
        V = m._engine.dec.V
        images, labels = synthetic_batch(B, 32, 12, min(V, 384), seed=3)
        prompt = labels[:, :P].clamp(min=0)
    assert V > 90
    return m, images.to(dev()), prompt.to(dev())


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.is_floating_point():
        assert a.dtype == torch.float32, what
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), what


def test_generate_captions(model):
    m, images, prompt = model
    call = lambda **kw: m.generate_captions(images, prompt, max_new_tokens=4, eos_token_id=EOS, top_k=1, **kw)
    one, sets = call(phrases=X), call(**SETS)
    for field in ('ids', 'lengths', 'token_logprobs', 'phrase_index'):
        same_bits(getattr(one, field), getattr(sets, field), field)
    assert int(one.phrase_index.min()) >= 0


def test_search_phrases(model):
    m, images, prompt = model
    widest = trie_widest_level(phrase_trie(X, EOS, m._engine.dec.V, 1 << 30))
    assert widest == 3
    for W in (2, widest):
        call = lambda **kw: m.search_phrases(images, prompt, eos_token_id=EOS, num_beams=W, num_return_sequences=W, **kw)
        one, sets = call(phrases=X), call(**SETS)
        for field in ('phrase_index', 'logprob', 'scores', 'lengths'):
            same_bits(getattr(one, field), getattr(sets, field), f'W = {W}: {field}')
        assert one.exhaustive == sets.exhaustive == (W >= widest)


def test_score_phrases(model):
    m, images, prompt = model
    K = len(X)
    one, sets = m.score_phrases(images, prompt, X, EOS), m.score_phrases(images, prompt, eos_token_id=EOS, **SETS)
    same_bits(one.logprob[:, :K], sets.logprob[:, :K], 'logprob')
    same_bits(one.best, sets.best, 'best')
