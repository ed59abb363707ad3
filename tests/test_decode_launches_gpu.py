"""The kernel launches of every decoding mode, in order, against a recorded list (tests/golden/decode_launches.json).

The drivers of image2text_amd/decoding.py promise "launch for launch" in their docstrings; this file holds them to it.  ``ops._k`` -- the
one object through which every wrapper of ops.py reaches an entry point -- is replaced by a proxy that writes the entry point's name
down and then calls the real checked caller.  Each mode runs once, eagerly (``use_graph=False``; ``poll_every=0``, so the number of
steps does not depend on what the model emits), on the tiny dense model and the tiny Llama of tests/test_score_phrases_gpu.py: B = 2
images, a prompt of 3 tokens, 2 new tokens (3 under ``phrases``: the longest phrase + 1), 3 phrases of at most 2 tokens of which two
share their first.  The fixture holds names only.  ``I2T_RECORD_LAUNCHES=1`` writes it instead of comparing: that is done once, on the
commit BEFORE a change to the drivers, never on the changed code."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from image2text_amd import ops
from image2text_amd.decoding import (BeamDecoder, BeamSpec, CaptionBeamDecoder, CaptionDecoder, GreedyDecoder, PhraseBeamDecoder, Sampling,
                                     check_phrase_sets, phrase_trie)
from image2text_amd.synth import synthetic_batch, tiny_config
from test_generate_captions_gpu import _ved

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'decode_launches.json')
B, P, NEW = 2, 3, 2
EOS = 5
PHRASES = [[17, 42], [17, 9], [63]]
SAMPLED = Sampling(0.7, None, 0.6, seed=7)


def dev():
    return torch.device('cuda:0')


class Recorder:
    """stands in for ops._k: an attribute is the real checked caller behind a line in ``names``"""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


@pytest.fixture(scope='module', params=['tiny', 'llama'])
def model(request, tiny_weights, tmp_path_factory):
    """-> (name, model, images [2, ...], prompt [2, 3])"""
    name = request.param
    if name == 'llama':
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
    return name, m, images.to(dev()), prompt.to(dev())


def calls(m, images, prompt):
    """(tag, thunk) of every mode, each on a decoder of its own"""
    V = m._engine.dec.V
    trie = phrase_trie(PHRASES, EOS, V, 1 << 30)
    ngrams = tuple(int(n) for n in m.config.no_repeat_n_grams)
    cap = dict(eos=EOS, pad=V - 1, poll_every=0, use_graph=False)
    captions = lambda **kw: CaptionDecoder(m).generate_captions(images, prompt, kw.pop('new', NEW), **cap, **kw)
    sets = dict(phrase_sets=[PHRASES, PHRASES[:2]], phrase_set_index=[0, 1])
    return [
        ('generate greedy', lambda: GreedyDecoder(m).generate(images, prompt, NEW, use_graph=False)),
        ('generate sampled', lambda: GreedyDecoder(m).generate(images, prompt, NEW, use_graph=False, sampling=SAMPLED)),
        ('beam search W=2', lambda: BeamDecoder(m).search(images, prompt, P + NEW, BeamSpec(2, 2, 0.0, None, 0.0, None, 0.0, ngrams), seed=3,
                                                          use_graph=False)),
        ('captions', lambda: captions()),
        ('captions prompt_lengths', lambda: captions(prompt_lengths=[2, 3])),
        ('captions repetition_penalty', lambda: captions(repetition_penalty=1.5)),
        ('captions phrases', lambda: captions(new=3, phrases=PHRASES)),
        ('captions num_beams=2', lambda: CaptionBeamDecoder(m).generate_captions(images, prompt, NEW, 2, **cap)),
        ('score_phrases', lambda: m.score_phrases(images, prompt, PHRASES, EOS)),
        ('search_phrases W=2', lambda: PhraseBeamDecoder(m).search(images, prompt, trie, EOS, 2, 2, poll_every=0, use_graph=False)),
        # a phrase set per image, with every prompt column in use and with prompts of 2 and 3 tokens
        ('captions phrase_sets', lambda: captions(new=3, **sets)),
        ('captions phrase_sets prompt_lengths', lambda: captions(new=3, prompt_lengths=[2, 3], **sets)),
        ('score_phrases phrase_sets', lambda: m.score_phrases(images, prompt, None, EOS, **sets)),
        ('score_phrases phrase_sets prompt_lengths', lambda: m.score_phrases(images, prompt, None, EOS, prompt_lengths=[2, 3], **sets)),
        ('search_phrases phrase_sets W=2', lambda: PhraseBeamDecoder(m).search_sets(
            images, prompt, check_phrase_sets(None, sets['phrase_sets'], sets['phrase_set_index'], B, EOS, V), EOS, 2, 1, poll_every=0,
            use_graph=False, plen=[2, 3])),
    ]


def test_every_mode_launches_what_it_launched(model, monkeypatch):
    name, m, images, prompt = model
    m._engine.prepare(False)                                    # the weight shadow's casts: whichever mode ran first would carry them
    torch.cuda.synchronize()
    got = {}
    for tag, run in calls(m, images, prompt):
        rec = Recorder(ops._k)
        with monkeypatch.context() as mp:
            mp.setattr(ops, '_k', rec)
            run()
        torch.cuda.synchronize()
        assert rec.names, tag
        got[tag] = rec.names
    if os.environ.get('I2T_RECORD_LAUNCHES') == '1':
        held = {}
        if os.path.exists(FIXTURE):
            with open(FIXTURE) as f:
                held = json.load(f)
        held[name] = got
        with open(FIXTURE, 'w') as f:
            json.dump(held, f, indent=0, sort_keys=True)
        return
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    assert sorted(got) == sorted(want)
    for tag in got:
        diff = next((i for i, (a, b) in enumerate(zip(got[tag], want[tag])) if a != b), min(len(got[tag]), len(want[tag])))
        assert got[tag] == want[tag], (f'{name}, {tag}: {len(got[tag])} launches against {len(want[tag])} recorded; first difference at {diff}: '
                                       f'{got[tag][diff:diff + 3]} against {want[tag][diff:diff + 3]}')
