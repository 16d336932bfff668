"""CPU checks of the posterior-predictive spread (vihmc.postprocess): Predictive.var / std / band from running sums,
error_uncertainty against a direct numpy restatement of the reference's plot_correlation lists
(Operator_network/VI_HMC/post_process_burgers.py:165-197), pool_ranks all-reducing the sum of squares on a gloo world
of 2, and the reference-generated fixture tests/golden/deeponet_predictive_std.npz against its own fp64 values."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from goldens import load
from vihmc.postprocess import Predictive, error_uncertainty, pool_ranks, predictive_moments  # noqa: F401


def _sums(x):
    return Predictive(n=x.shape[0], pred_sum=x.sum(0), pred_sqsum=(x * x).sum(0))


def test_std_and_var_match_numpy_and_torch():
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((9, 5, 13)) * 0.3 + 1.7)
    p = _sums(x)
    assert p.pred_sqsum.dtype == torch.float64
    np.testing.assert_allclose(p.std().numpy(), np.std(x.numpy(), axis=0), rtol=1e-12)
    np.testing.assert_allclose(p.std(0).numpy(), np.std(x.numpy(), axis=0, ddof=0), rtol=1e-12)
    np.testing.assert_allclose(p.std(1).numpy(), torch.std(x, dim=0).numpy(), rtol=1e-12)
    np.testing.assert_allclose(p.var(1).numpy(), torch.var(x, dim=0).numpy(), rtol=1e-12)
    lo, hi = p.band()
    np.testing.assert_allclose(lo.numpy(), x.numpy().mean(0) - 3 * np.std(x.numpy(), axis=0), rtol=1e-12)
    np.testing.assert_allclose(hi.numpy(), x.numpy().mean(0) + 3 * np.std(x.numpy(), axis=0), rtol=1e-12)
    lo2, hi2 = p.band(k=1.5)
    np.testing.assert_allclose((hi2 - lo2).numpy(), 3 * np.std(x.numpy(), axis=0), rtol=1e-12)


def test_single_sample_and_missing_sqsum():
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 3, 4)))
    p = _sums(x)
    assert torch.equal(p.var(0), torch.zeros(3, 4, dtype=torch.float64))    # one sample: no spread, never negative
    with pytest.raises(ValueError):
        p.std(1)                                                            # n - ddof = 0
    old = Predictive(n=4, pred_sum=torch.zeros(3, 4, dtype=torch.float64))  # what predictive() returns
    assert old.pred_sqsum is None
    with pytest.raises(ValueError):
        old.std()
    with pytest.raises(ValueError):
        old.band()


def test_var_is_clamped_and_nan_propagates():
    c = torch.full((4, 2, 3), 0.1, dtype=torch.float64)                      # constant predictions: cancellation
    assert (_sums(c).var() >= 0).all() and float(_sums(c).std().max()) < 1e-7
    x = torch.ones(3, 2, 2, dtype=torch.float64)
    x[1, 0, 1] = float("inf")
    sd = _sums(x).std()
    assert torch.isnan(sd[0, 1]) and float(sd[1, 1]) == 0.0                   # as np.std over such a list


@pytest.mark.parametrize("reference_mean", [False, True])
def test_error_uncertainty_matches_numpy_restatement(reference_mean):
    rng = np.random.default_rng(2)
    S, N, nx, nt = 7, 5, 6, 4
    y = rng.standard_normal((N, nt * nx))
    preds = y[None] + 0.2 * rng.standard_normal((S, N, nt * nx)) * (1 + np.abs(y[None]))
    p = _sums(torch.from_numpy(preds))
    err, std, corr = error_uncertainty(p.mean(), p.std(1), torch.from_numpy(y), nx, reference_mean=reference_mean)
    assert len(err) == len(std) == len(corr) == nt
    for t in range(nt):
        pt = torch.from_numpy(preds[:, :, t * nx:(t + 1) * nx])               # the reference's pred_tensor
        truth = torch.from_numpy(y[:, t * nx:(t + 1) * nx])
        mean_pred = torch.mean(pt) if reference_mean else torch.mean(pt, dim=0)
        std_pred = torch.std(pt, dim=0)
        err_pred = torch.abs(mean_pred - truth)
        cc = np.corrcoef(err_pred.flatten(), std_pred.flatten())[0][1]
        assert err[t] == pytest.approx(float(torch.mean(err_pred)), rel=1e-12)
        assert std[t] == pytest.approx(float(torch.mean(std_pred)), rel=1e-12)
        assert corr[t] == pytest.approx(cc, rel=1e-9, abs=1e-12)
    with pytest.raises(ValueError):
        error_uncertainty(p.mean(), p.std(1), torch.from_numpy(y), nx + 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_data(rank):
    return torch.from_numpy(np.random.default_rng(40 + rank).standard_normal((3 + rank, 4, 5)))


def _pool_worker(rank, ws, port, out_path):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.join(here, ".."), os.path.join(here, "..", "vi-hmc_amd")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    x = _rank_data(rank)
    p = _sums(x)
    p.mse = [float(rank)] * x.shape[0]
    p.log_prob = [-float(rank)] * x.shape[0]
    p = pool_ranks(p)
    old = pool_ranks(Predictive(n=2, pred_sum=torch.ones(4, 5, dtype=torch.float64)))   # no sum of squares: still fine
    if rank == 0:
        torch.save({"n": p.n, "sum": p.pred_sum, "sq": p.pred_sqsum, "std": p.std(1), "mse": p.mse,
                    "old_n": old.n, "old_sq_none": old.pred_sqsum is None}, out_path)
    dist.barrier()
    dist.destroy_process_group()


def test_pool_ranks_all_reduces_the_sum_of_squares(tmp_path):
    out = str(tmp_path / "pool.pt")
    mp.start_processes(_pool_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    x = torch.cat([_rank_data(0), _rank_data(1)])
    assert got["n"] == x.shape[0] == 7 and got["old_n"] == 4 and got["old_sq_none"]
    assert torch.equal(got["sum"], _rank_data(0).sum(0) + _rank_data(1).sum(0))
    assert torch.equal(got["sq"], (_rank_data(0) ** 2).sum(0) + (_rank_data(1) ** 2).sum(0))
    np.testing.assert_allclose(got["std"].numpy(), torch.std(x, dim=0).numpy(), rtol=1e-12)
    assert got["mse"] == [0.0] * 3 + [1.0] * 4


@pytest.mark.parametrize("name", ["deeponet_small", "deeponet_refshape"])
def test_fixture_reference_std_is_its_own_fp64_std(name):
    """Guards the generator (tests/golden/make_golden_predictive.py): the reference's fp32 np.std of its fp32
    predictions sits within 1e-5 relative norm of the fp64 oracle's std of the same samples (measured 6.3e-7 on
    deeponet_small, 3.1e-7 on deeponet_refshape), likewise the mean; and the sample vectors are the documented ones."""
    from goldens import deeponet_case, sha
    from golden.make_golden_predictive import N_SAMPLES, predictive_thetas
    g = load("deeponet_predictive_std")
    std32, std64 = g[f"{name}_std32"], g[f"{name}_std64"]
    assert std32.dtype == np.float32 and std64.dtype == np.float64 and std32.shape == std64.shape
    assert np.linalg.norm(std32 - std64) / np.linalg.norm(std64) <= 1e-5
    assert np.linalg.norm(g[f"{name}_mean32"] - g[f"{name}_mean64"]) / np.linalg.norm(g[f"{name}_mean64"]) <= 1e-5
    th = predictive_thetas(deeponet_case(name).thetas[0])
    assert th.shape[0] == N_SAMPLES == int(g["n_samples"]) == 12 and th.dtype == np.float32
    assert [sha(t) for t in th] == [str(s) for s in g[f"{name}_theta_sha"]]
