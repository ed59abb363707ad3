"""bench.py's command line and its --dump-outputs writer, on the host (a small CPU module stands in for the model)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('i2t_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_times_the_given_steps_only(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '3', '--full', '--dump-outputs', 'out'])
    a = bench.parse()
    assert (a.steps, a.full, a.dump_outputs) == (3, True, 'out')


def test_dump_outputs_writes_loss_and_fixed_gradient_samples(tmp_path):
    bench = _bench()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 400), torch.nn.Linear(400, 3))
    bench.dump_outputs(str(tmp_path / 'a'), torch.tensor(2.5), list(model.named_parameters()))
    bench.dump_outputs(str(tmp_path / 'b'), torch.tensor(2.5), list(model.named_parameters()))
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['grad.0.bias.npy', 'grad.0.weight.npy', 'grad.1.bias.npy', 'grad.1.weight.npy', 'loss.npy']
    loss = np.load(tmp_path / 'a' / 'loss.npy')
    assert loss.dtype == np.float64 and loss.tolist() == [2.5]
    big = np.load(tmp_path / 'a' / 'grad.0.weight.npy')                   # 120000 elements: a sample of DUMP_SAMPLE
    assert big.dtype == np.float32 and big.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(big, model[0].weight.detach().numpy().ravel()).all()
    small = np.load(tmp_path / 'a' / 'grad.1.weight.npy')                 # 1200 elements: in full
    assert np.array_equal(small, model[1].weight.detach().numpy().ravel())
    for f in files:                                                        # the same positions on every dump
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) < 64 * 2**20
