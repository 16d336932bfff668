"""Generate tests/golden/deeponet_predictive_std.npz: the posterior-predictive mean and standard deviation of a small
seeded sample list, by running the REFERENCE's own functional forward.

Run in the build container only, on the CPU (it reads /root/reference, which the GPU box does not have):

    python tests/golden/make_golden_predictive.py

For the golden cases ``deeponet_small`` and ``deeponet_refshape`` it takes 12 sample vectors
``th0 + 0.01 * default_rng(11).standard_normal(K)`` (fp32, consecutive draws of one generator; ``predictive_thetas``
below, which the tests import), evaluates the reference's ``Functional_DeepONet.functional_model``
(Operator_network/VI_HMC/my_make_func.py:44-83) on each, and reduces the prediction list exactly as
post_process_burgers.py:85-86 does -- ``np.mean(pred_list, axis=0)`` and ``np.std(pred_list, axis=0)`` on the fp32
predictions. Next to them it stores the fp64 mean and std of the same samples from oracle.deeponet_ref.np_forward, and
the SHA-256 of every sample vector. The reference modules are imported the way make_golden.py imports them.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for d in (os.path.join(ROOT, "vi-hmc_amd"), ROOT, os.path.join(ROOT, "tests"), HERE):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402

CASES = ("deeponet_small", "deeponet_refshape")
N_SAMPLES = 12
SEED = 11
SCALE = 0.01


def predictive_thetas(th0: np.ndarray) -> np.ndarray:
    """The fixture's [12, K] fp32 sample vectors around th0."""
    rng = np.random.default_rng(SEED)
    return np.stack([(th0 + SCALE * rng.standard_normal(th0.size)).astype(np.float32) for _ in range(N_SAMPLES)])


def main():
    import torch
    from goldens import deeponet_case, sha
    from make_golden import import_ref, stub_hamiltorch
    from oracle.deeponet_ref import deeponet_layout, np_forward, trunk_feats_np

    stub_hamiltorch()
    M = import_ref("Operator_network/VI_HMC", "main_VI_HMC_burgers")
    from my_make_func import Functional_DeepONet          # the module main_VI_HMC_burgers itself imported

    out = {}
    for name in CASES:
        c = deeponet_case(name)
        s, p = c.spec, c.prob
        thetas = predictive_thetas(c.thetas[0])
        net = M.DeepONet(s.width_branch, s.width_trunk, s.in_branch, s.in_trunk, s.depth_branch, s.depth_trunk,
                         s.activation, s.output_neurons)
        f = Functional_DeepONet(depth_branch=s.depth_branch, depth_trunk=s.depth_trunk, mus=torch.from_numpy(p.mu.copy()),
                                sigmas=torch.from_numpy(p.sigma.copy()), activation=s.activation,
                                sensitive_ind=p.grad_ind, model=net)
        x1, x2 = torch.from_numpy(p.branch_in), torch.from_numpy(p.trunk_in)
        pred_list = []
        with torch.no_grad():
            for th in thetas:
                pred = f.functional_model(x1, x2, torch.from_numpy(th.copy()))
                pred_list.append(pred.squeeze().detach().numpy().reshape(p.y.shape))
        mean32 = np.mean(pred_list, axis=0)
        std32 = np.std(pred_list, axis=0)
        assert mean32.dtype == np.float32 and std32.dtype == np.float32
        lay = deeponet_layout(s.in_branch, s.width_branch, s.depth_branch, s.in_trunk, s.width_trunk, s.depth_trunk, s.out)
        feats = trunk_feats_np(p.trunk_in)
        p64 = []
        for th in thetas:
            flat = p.mu.astype(np.float64).copy()
            flat[p.grad_ind] = th.astype(np.float64)
            p64.append(np_forward(lay, flat, p.branch_in, feats, s.activation)[0])
        mean64, std64 = np.mean(p64, axis=0), np.std(p64, axis=0)
        e = np.linalg.norm(std32 - std64) / np.linalg.norm(std64)
        e2 = np.linalg.norm(np.std(np.asarray(pred_list, np.float64), axis=0) - std64) / np.linalg.norm(std64)
        print(f"{name}: reference fp32 std vs fp64 {e:.3e}; fp64 moments of the fp32 predictions {e2:.3e}")
        out.update({f"{name}_mean32": mean32, f"{name}_std32": std32, f"{name}_mean64": mean64, f"{name}_std64": std64,
                    f"{name}_theta_sha": np.array([sha(th) for th in thetas])})
    out.update(n_samples=N_SAMPLES, seed=SEED, scale=SCALE)
    np.savez_compressed(os.path.join(HERE, "deeponet_predictive_std.npz"), **out)


if __name__ == "__main__":
    main()
