"""CPU: bench.py --dump-outputs writes what the step returned as float32 / float64 .npy files, samples large arrays at fixed
indices, repeats itself exactly and stays within its 64 MB budget."""
import os

import numpy as np
import pytest
import torch

import bench


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(3000, 1000), torch.nn.Linear(1000, 10))
    m(torch.randn(4, 3000)).sum().backward()
    return m


def _result():
    g = torch.Generator().manual_seed(1)
    return (torch.tensor(1.5),
            {'loss_ce': torch.tensor(0.25, dtype=torch.bfloat16), 'n': 3, 'mask': torch.tensor([True, False])},
            [{'scores': torch.randn(3000, 500, generator=g), 'labels': torch.arange(4)}], None)


def test_dump_outputs_dtypes_names_and_sampling(tmp_path):
    m = _model()
    shapes = bench.dump_outputs(str(tmp_path), _result(), m, train=True)
    files = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert files == sorted(shapes) == sorted(['out.0', 'out.1.loss_ce', 'out.1.n', 'out.1.mask', 'out.2.0.scores', 'out.2.0.labels',
                                              'params', 'grads'])
    load = {n: np.load(tmp_path / f'{n}.npy') for n in files}
    assert load['out.0'].dtype == np.float32 and float(load['out.0']) == 1.5
    assert load['out.1.loss_ce'].dtype == np.float32 and float(load['out.1.loss_ce']) == 0.25
    assert load['out.1.n'].dtype == np.float64 and float(load['out.1.n']) == 3
    assert load['out.1.mask'].dtype == np.float64 and load['out.1.mask'].tolist() == [1.0, 0.0]
    assert load['out.2.0.labels'].tolist() == [0, 1, 2, 3]
    # 1.5 M scores: a sample of at most DUMP_MAX_ELEMS elements, each one an element of the array
    s = load['out.2.0.scores']
    assert s.dtype == np.float32 and 0 < s.size <= bench.DUMP_MAX_ELEMS
    assert np.isin(s, _result()[2][0]['scores'].numpy()).all()
    # parameters and gradients: the same indices in both, so params[i] and grads[i] belong to the same element
    assert load['params'].shape == load['grads'].shape
    flat_p = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    flat_g = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).numpy()
    idx = np.unique(np.random.default_rng(0).integers(0, flat_p.size, 2 * bench.DUMP_MAX_ELEMS))
    assert np.array_equal(load['params'], flat_p[idx]) and np.array_equal(load['grads'], flat_g[idx])
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_BUDGET + 8192


def test_dump_outputs_repeats_exactly(tmp_path):
    m = _model()
    bench.dump_outputs(str(tmp_path / 'a'), _result(), m, train=True)
    bench.dump_outputs(str(tmp_path / 'b'), _result(), m, train=True)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b'))
    for n in names:
        assert np.array_equal(np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)), n


def test_dump_outputs_refuses_more_than_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET', 1 << 20)
    with pytest.raises(RuntimeError, match='--dump-outputs'):
        bench.dump_outputs(str(tmp_path / 'd'), _result(), _model(), train=True)
    assert not os.path.exists(tmp_path / 'd')          # nothing written when the budget is exceeded


def test_eval_dump_has_no_parameters(tmp_path):
    shapes = bench.dump_outputs(str(tmp_path), {'loss': torch.tensor(2.0)}, _model(), train=False)
    assert list(shapes) == ['out.loss']
