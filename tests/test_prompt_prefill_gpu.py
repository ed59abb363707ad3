"""generate_captions(prompt_prefill='pass') on the MI355X: prompt columns 0 .. Pmin - 2 through ONE forward pass per image,
their K/V scattered into the N cache rows of the image by i2t_kv_prefill, then the same full steps as 'steps'.

Models: tiny (trained weights), a decoder of width 64, a Hugging Face GPT-2 with the soft prefix ([encoder outputs | text] in one pass)
and without it, and the fixture-size Llama (row-major cache, rotated keys, per-layer hand-over).  B = 3, P = 6, 8 new tokens.

The two modes are NOT bit-equal -- the prompt's K/V come from the forward's GEMM and attention shapes --, so the bars are those of
tests/test_generate_captions_gpu.py: token_logprobs against fp64 log_softmax of the model's own forward at the generated ids and
against score(), both within 4 . logits_tol(logits); a cache that held wrong, misplaced or another image's K/V fails it, and for
N = 2 it is the check that both rows of an image got that image's prompt.  Greedy ids may leave the 'steps' run only at a column whose
top-2 margin in the 'steps' run is below 2 . logits_tol (each run's logits are within logits_tol of the oracle's)."""
import pytest
import torch

from image2text_amd.decoding import GreedyDecoder
from image2text_amd.synth import mini_config, synthetic_batch, tiny_config
from test_generate_captions_gpu import GREEDY, SAMPLING, _ved, check_logprobs, check_shapes
from test_model_gpu import logits_tol

pytestmark = pytest.mark.gpu

B, P, T = 3, 6, 8
PLEN = [2, 6, 4]
PASS, STEPS = dict(prompt_prefill='pass'), dict(prompt_prefill='steps')


def dev():
    return torch.device('cuda:0')


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.fixture(params=['tiny', 'dense64', 'hf_gpt2_soft', 'hf_gpt2', 'llama'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    """-> (name, model, images [3, ...], prompt [3, 6])"""
    name = request.param
    if name == 'tiny':
        m = _ved(tiny_config(), tiny_weights)
    elif name == 'dense64':
        m = _ved(tiny_config(dec_d=64, dec_heads=1))
    elif name.startswith('hf_gpt2'):
        from test_hf_decoder_gpu import _build
        _, m = _build(tmp_path, monkeypatch, True, name == 'hf_gpt2_soft')
        m = m.to(dev()).eval()
        assert m._engine.dec.prefixed == (name == 'hf_gpt2_soft') and m._engine.dec.llama is None
    else:
        from test_hf_decoder_gpu import _llama_model
        _, m, _, _ = _llama_model(tmp_path, monkeypatch, 'llama')
        m = m.to(dev()).eval()
        assert m._engine.dec.llama is not None and m._engine.dec.prefixed
    assert m._engine.dec.causal and m._engine.dec.fam is None
    images, labels = synthetic_batch(B, 32, 12, min(m._engine.dec.V, 384), seed=11)
    return name, m, images.to(dev()), labels[:, :P].clamp(min=0).to(dev())


def test_one_token_prompts_and_nothing_to_emit_are_steps(model):
    """Pmin = 1 leaves nothing to prefill: 'pass' launches nothing new and is bit-equal to 'steps'; so is max_new_tokens = 0"""
    name, m, images, prompt = model
    for mode in (GREEDY, dict(seed=9, num_return_sequences=2, **SAMPLING)):
        want = m.generate_captions(images, prompt[:, :1].contiguous(), max_new_tokens=T, **mode, **STEPS)
        got = m.generate_captions(images, prompt[:, :1].contiguous(), max_new_tokens=T, **mode, **PASS)
        assert same(got, want), f'{name}: P = 1 under pass differs from steps'
        assert m._captioner.last_prefill_steps == 0 and m._captioner.last_replays == T
    want = m.generate_captions(images, prompt, max_new_tokens=0, **GREEDY, **STEPS)
    got = m.generate_captions(images, prompt, max_new_tokens=0, **GREEDY, **PASS)
    assert same(got, want) and torch.equal(got.ids[:, 0], prompt) and got.token_logprobs.shape[-1] == 0
    assert m._captioner.last_prefill_steps == 0 and m._captioner.last_replays == 0


@pytest.mark.parametrize('mode', [GREEDY, dict(seed=21, **SAMPLING), dict(seed=21, num_return_sequences=2, **SAMPLING)],
                         ids=['greedy', 'sampling', 'sampling_n2'])
def test_log_probs_of_a_prefilled_run(model, mode):
    """P = 6: shapes, replays, and every chosen token's log-prob against the model's own forward and score() -- the prompt's K/V in the
    cache are the right ones, at the right slots, of the right image, in every one of an image's rows"""
    name, m, images, prompt = model
    N = mode.get('num_return_sequences', 1)
    out = m.generate_captions(images, prompt, max_new_tokens=T, **mode, **PASS)
    assert m._captioner.last_prefill_steps == 0 and m._captioner.last_replays == T
    check_shapes(out, B, N, P)
    assert bool((out.ids[:, :, :P] == prompt[:, None]).all()) and bool((out.lengths == P + T).all())
    check_logprobs(m, images, out, P, f'{name} pass N={N} {"greedy" if mode is GREEDY else "sampling"}')
    m.generate_captions(images, prompt, max_new_tokens=T, **mode, **STEPS)
    assert m._captioner.last_prefill_steps == P - 1 and m._captioner.last_replays == T


def test_greedy_ids_against_steps(model):
    """a row leaves the 'steps' run only at a column whose top-2 margin there is below 2 . logits_tol; tiny: at most 1 row of 3"""
    name, m, images, prompt = model
    steps = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY, **STEPS).ids[:, 0]
    got = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY, **PASS).ids[:, 0]
    ref_ids, margins = GreedyDecoder(m).generate(images, prompt, T, return_margins=True)
    with torch.no_grad():
        tol = logits_tol(m(images=images, ids=steps).logits.float().cpu().numpy())
    diverged = 0
    for b in range(B):
        diff = (got[b] != steps[b]).nonzero()
        if diff.numel() == 0:
            continue
        c = int(diff[0])
        diverged += 1
        assert c >= P and torch.equal(ref_ids[b, :c], steps[b, :c]), f'{name} row {b}: the margins are not those of the steps run up to column {c}'
        margin = float(margins[b, c - P])
        print(f'{name} row {b}: leaves the steps run at column {c}, margin there {margin:.3g} (2 logits_tol = {2 * tol:.3g})')
        assert margin < 2 * tol, f'{name} row {b}: diverges at column {c} where the steps run is decided by {margin:.3g} >= {2 * tol:.3g}'
    print(f'{name}: {diverged} of {B} greedy rows diverged from the steps run')
    if name == 'tiny':
        assert diverged <= 1


def test_modes_share_one_state(model):
    """steps, pass, steps on ONE model: the first and third are bit-equal -- state, graphs and counters_init are undisturbed --; the
    'pass' run without the captured graph equals the one with it"""
    name, m, images, prompt = model
    first = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY, **STEPS)
    st = m._captioner._state
    keys, init = set(st.graphs), st.counters_init.clone()
    mid = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY, **PASS)
    assert m._captioner._state is st and set(st.graphs) == keys, 'a pass call rebuilt the state or captured a graph of its own'
    assert torch.equal(st.counters_init, init)
    third = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    assert m._captioner.last_prefill_steps == P - 1
    assert same(third, first), f'{name}: a steps call after a pass call differs from the one before it'
    eager = m._captioner.generate_captions(images, prompt, T, use_graph=False, prompt_prefill='pass')
    assert m._captioner.last_prefill_steps == 0
    assert same(eager, mid), f'{name}: use_graph=False under pass differs from the captured step'


def test_prompt_lengths_keep_their_forced_steps(model):
    """prompt_lengths = [2, 6, 4] under 'pass': column 0 is prefilled (m = Pmin - 1 = 1), columns 1 .. 5 stay forced steps; the emitted
    tokens' log-probs on the same bar, forced columns and columns past a row's end exactly 0.0"""
    name, m, images, prompt = model
    for mode in (GREEDY, dict(seed=5, num_return_sequences=2, **SAMPLING)):
        N = mode.get('num_return_sequences', 1)
        out = m.generate_captions(images, prompt, max_new_tokens=T, prompt_lengths=PLEN, **mode, **PASS)
        assert m._captioner.last_prefill_steps == 0 and m._captioner.last_replays == max(PLEN) - min(PLEN) + T
        pmin, L = min(PLEN), out.ids.shape[-1]
        plen = torch.tensor(PLEN, device=dev()).repeat_interleave(N)
        assert L == max(PLEN) + T and tuple(out.token_logprobs.shape) == (B, N, L - pmin)
        assert torch.equal(out.lengths.reshape(-1), (plen + T).int())
        ids, rep = out.ids.reshape(B * N, L), images.repeat_interleave(N, dim=0)
        for b, p in enumerate(PLEN):
            assert bool((out.ids[b, :, :p] == prompt[b, :p]).all())
        with torch.no_grad():
            logits = m(images=rep, ids=ids).logits
        bar = 4 * logits_tol(logits.float().cpu().numpy())
        ref = torch.log_softmax(logits.double(), dim=-1)[:, pmin - 1:L - 1].gather(-1, ids[:, pmin:, None])[..., 0]
        col = torch.arange(pmin, L, device=dev())[None, :]
        live = (col >= plen[:, None]) & (col < out.lengths.reshape(B * N, 1))
        got = out.token_logprobs.reshape(B * N, L - pmin)
        err = float(((got.double() - ref).abs() * live).max())
        print(f'{name} pass, prompt_lengths {PLEN} x {N}: token_logprobs worst error / bar {err / bar:.3g} (bar {bar:.3g})')
        assert torch.isfinite(got).all() and err <= bar and bool((got[live] <= bar).all()) and bool((got[live] < 0).any())
        assert bool((got[~live] == 0).all()), 'a forced or finished column holds a log-prob'
        m.generate_captions(images, prompt, max_new_tokens=T, prompt_lengths=PLEN, **mode, **STEPS)
        assert m._captioner.last_prefill_steps == pmin - 1


def test_the_family_refuses_and_bad_modes_are_named(tiny_weights):
    mini = _ved(mini_config(), sharpen=True)
    assert mini._engine.dec.fam is not None
    images, labels = synthetic_batch(B, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :P].clamp(min=0).to(dev())
    with pytest.raises(NotImplementedError, match='nano-mini decoder family'):
        mini.generate_captions(images, prompt, max_new_tokens=T, **GREEDY, **PASS)
    want = mini.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    got = mini.generate_captions(images, prompt, max_new_tokens=T, **GREEDY, **STEPS)
    assert same(got, want) and mini._captioner.last_prefill_steps == P - 1
    tiny = _ved(tiny_config(), tiny_weights)
    for bad in ('graph', None, 'PASS'):
        with pytest.raises(ValueError, match='prompt_prefill'):
            tiny.generate_captions(images, prompt, max_new_tokens=T, prompt_prefill=bad, **GREEDY)
