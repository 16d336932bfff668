"""Layer backward, hidden layers of a row chunk in one launch (k_bwd_bf2_layers, plan option bwd_layers) against the
per-layer k_bwd_bf2 launches (bwd_layers = 0) and the whole-network k_bwd_chain: the same products in the same order
into the same partial slabs, so every comparison here is torch.equal.

The workgroup of (net, chain, row chunk) walks layers nl - 1 .. 1 of its own rows; the deltas round-trip through
global memory between the layers, so the shapes exercise what can go wrong at a layer boundary: chunks of several
32-row sub-tiles (odd and even counts, partial tails), distinct chains, and fewer chains than the plan was made for.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, NT, NX = 40, 45, 45           # P = 2,025 trunk rows


@functools.lru_cache(maxsize=None)
def _problem(depth_branch=9, depth_trunk=9):
    from vihmc.data import deeponet_problem
    from vihmc.layout import DeepONetSpec
    spec = DeepONetSpec(depth_branch=depth_branch, depth_trunk=depth_trunk)
    return deeponet_problem(seed=11, n=N, nt=NT, nx=NX, spec=spec)


def _engine(p, max_chains, dev, **options):
    from vihmc.engine import DeepONetEngine, trunk_features
    eng = DeepONetEngine(p.spec, p.branch_in, trunk_features(p.trunk_in), p.y, p.mu, p.grad_ind, 0.0, 0.1, "NLL", 1.0,
                         max_chains=max_chains, device=dev)
    for k, v in options.items():
        eng.option(k, v)
    return eng


def _thetas(p, C, dev, seed=3):
    """distinct chains: mu plus seeded jitter of ~0.02, different per chain"""
    rng = np.random.default_rng(seed)
    mu = p.mu[p.grad_ind].astype(np.float32)
    return torch.tensor(mu[None] + 0.02 * rng.standard_normal((C, mu.size)).astype(np.float32), device=dev)


def _evaluate(eng, th, ran):
    """grad (the Gram-form inner step at 4+ chains) and logp_grad, twice each; `ran` is the expected get_option value"""
    g = eng.grad(th).clone()
    assert eng.get_option("bwd_layers") == ran
    lp, gl = (x.clone() for x in eng.logp_grad(th))
    assert eng.get_option("bwd_layers") == ran
    assert torch.equal(eng.grad(th), g), "grad: repeated call differs"
    lp2, gl2 = eng.logp_grad(th)
    assert torch.equal(lp2, lp) and torch.equal(gl2, gl), "logp_grad: repeated call differs"
    return g, lp, gl


def _same(a, b, note):
    for x, y, what in zip(a, b, ("grad", "logp", "logp_grad gradient")):
        assert torch.equal(x, y), (note, what, float((x - y).abs().max()))


def test_multi_subtile_chunks_fused_equals_per_layer(cuda_device):
    """16-chain plan: R = 160-row chunks (5 sub-tiles), 13 trunk chunks of which the last has 105 rows (4 sub-tiles,
    the last of 9 rows), one branch chunk of 40 rows (2 sub-tiles, the second partial). Fresh engines per setting,
    then both settings toggled on one engine."""
    p = _problem()
    th = _thetas(p, 16, cuda_device)
    fused = _evaluate(_engine(p, 16, cuda_device, bwd_layers=1), th, 3)
    eng = _engine(p, 16, cuda_device, bwd_layers=0)
    per_layer = _evaluate(eng, th, 0)
    _same(fused, per_layer, "fresh engines")
    eng.option("bwd_layers", 1)
    _same(_evaluate(eng, th, 3), per_layer, "toggled on")
    eng.option("bwd_layers", 0)
    _same(_evaluate(eng, th, 0), per_layer, "toggled off")


def test_64_row_chunks_three_way(cuda_device):
    """4-chain plan: 64-row chunks, where k_bwd_chain is eligible and chosen first; without it the fused launch,
    without that the per-layer launches -- all three bitwise equal."""
    p = _problem()
    th = _thetas(p, 4, cuda_device)
    eng = _engine(p, 4, cuda_device)
    chain = _evaluate(eng, th, 1)                      # bwd_layers on, but k_bwd_chain ran
    assert eng.get_option("bwd_chain") == 3
    eng.option("bwd_chain", 0)
    fused = _evaluate(eng, th, 3)
    assert eng.get_option("bwd_chain") == 0
    eng.option("bwd_layers", 0)
    per_layer = _evaluate(eng, th, 0)
    _same(fused, per_layer, "fused vs per layer")
    _same(fused, chain, "fused vs chain")


def test_fewer_chains_than_the_plan(cuda_device):
    """the 16-chain plan called with 3 chains: the block -> (net, chain, chunk) mapping follows the call's count"""
    p = _problem()
    th = _thetas(p, 3, cuda_device, seed=5)
    eng = _engine(p, 16, cuda_device)
    fused = _evaluate(eng, th, 3)
    eng.option("bwd_layers", 0)
    _same(fused, _evaluate(eng, th, 0), "C = 3 of 16")


def test_nets_of_different_depth(cuda_device):
    """branch of 4 layers, trunk of 6: each net walks its own layers, and the two input layers (at different
    distances from the top) keep their own launches"""
    p = _problem(4, 6)
    th = _thetas(p, 16, cuda_device, seed=7)
    eng = _engine(p, 16, cuda_device)
    fused = _evaluate(eng, th, 3)
    eng.option("bwd_layers", 0)
    _same(fused, _evaluate(eng, th, 0), "depths 4 / 6")


def test_fp32_backward_falls_back_to_per_layer(cuda_device):
    """bwd_bf16x6 = 0 selects the fp32 layer backward, which the fused launch must refuse: the per-layer path runs
    with bwd_layers on, and equals bwd_layers = 0."""
    p = _problem()
    th = _thetas(p, 16, cuda_device)
    eng = _engine(p, 16, cuda_device, bwd_bf16x6=0)
    on = _evaluate(eng, th, 1)
    assert eng.get_option("bwd_layers") & 2 == 0
    eng.option("bwd_layers", 0)
    _same(on, _evaluate(eng, th, 0), "fp32 backward")
