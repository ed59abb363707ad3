"""decoding.slot_positions (no GPU): the text position held at each cache slot of a sparse decoder layer, the table through which
beam search on the KV cache reads a sparse layer's keys (i2t_beam_gq_decode_attention's slot_pos)."""
import numpy as np
import pytest

from image2text_amd.decoding import slot_positions, text_window
from image2text_amd.synth import mini_config, nano_mini_config


@pytest.mark.parametrize('name', ['mini', 'nano_mini'])
def test_slot_positions_of_the_sparse_decoder_sets(name):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    cfg = {'mini': mini_config, 'nano_mini': nano_mini_config}[name]()
    m = VisionEncoderDecoder(cfg)
    eng = m._engine
    off = eng.enc.ncls if cfg.use_soft_prompting else 0
    tmax = text_window(eng.dec.block, off, 0)
    width = tmax                                    # the beam history table: prefix (0: no Hugging Face prompt rows) + tmax columns
    sets = eng._sparse_idx['dec']
    assert len(sets) == cfg.decoder_config.n_layer
    # plain statement: layer l keeps text position p when off + p is in its kept set
    member = np.zeros((len(sets), tmax), dtype=np.int32)
    for l, (idx, _not) in enumerate(sets):
        for i in idx.tolist():
            if off <= i < off + tmax:
                member[l, i - off] = 1
    rank = np.cumsum(member, axis=1) - member
    kpos = slot_positions(member)
    assert kpos.dtype == np.int32 and kpos.shape == (len(sets), max(int(member.sum(1).max()), 1))
    assert kpos.shape[1] < tmax, 'the sets are sparse: fewer slots than text positions'
    for l in range(len(sets)):
        kept = [p for p in range(tmax) if member[l, p]]
        assert kept, (name, l)
        for p in kept:
            assert kpos[l, rank[l, p]] == p, (name, l, p)
        assert kpos[l, :len(kept)].tolist() == kept
        assert (kpos[l, len(kept):] == 0).all()
    assert int(kpos.min()) >= 0 and int(kpos.max()) < width


def test_slot_positions_edge_rows():
    member = np.array([[1, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]], dtype=np.int32)
    assert slot_positions(member).tolist() == [[0, 2, 3], [0, 0, 0], [5, 0, 0]]
    assert slot_positions(np.zeros((2, 4), dtype=np.int32)).tolist() == [[0], [0]]
