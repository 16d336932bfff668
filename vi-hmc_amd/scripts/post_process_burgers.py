#!/usr/bin/env python3
"""Offline pooling of saved VI-HMC chains -- mirrors Operator_network/VI_HMC/post_process_burgers.py
(get_list_fnames :261-282, the pool of hmc_params_{uid}.npy[burn:] :285-288, print_error :124-146,
l2_relative_error :105-121) on the HIP engine: every pooled sample's prediction on the validation set in
batches of 16 per launch, the per-sample per-function relative L2 errors print_error reports, and the
posterior-predictive mean with its relative L2 error. ``--std`` adds the spread: the posterior-predictive standard
deviation (np.std(pred_list, axis=0), :85-86) from the fused moments path, saved as prediction_std_{test_ind}.npy (the
last Nx points of function test_ind, plot_predictions :241,252) and posterior_std_pooled.npy (the full field), and the
error-vs-sigma correlation per time slice (plot_correlation :165-197). Plotting / animation are out of scope
(DESIGN.md §8).

    python vi-hmc_amd/scripts/post_process_burgers.py [--out-dir samples/Burgers/] [--std [--test-ind 79]]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vihmc import configs  # noqa: E402
from vihmc.data import load_vi_artefacts  # noqa: E402
from vihmc.engine import DeepONetEngine, trunk_features  # noqa: E402
from vihmc.operator import DeepONet, get_burgers_data  # noqa: E402
from vihmc.postprocess import (error_uncertainty, get_list_fnames, load_pooled_samples, predictive,  # noqa: E402
                               predictive_moments, print_summary)

NX = 101    # grid points per time slice of the Burgers data (post_process_burgers.py:87,166)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--burn", type=int, default=None)
    ap.add_argument("--n-train", type=int, default=None)
    ap.add_argument("--std", action="store_true", help="posterior-predictive std, its artefacts and the error-vs-sigma "
                                                       "correlation (predictive_moments)")
    ap.add_argument("--test-ind", type=int, default=79, help="function of prediction_std_{test_ind}.npy (with --std)")
    args = ap.parse_args()
    over = {"out_dir": args.out_dir.rstrip("/") + "/"} if args.out_dir else {}
    if args.n_train:
        over.update(N_train=args.n_train, N_valid=args.n_train)
    if args.burn is not None:
        over["burn"] = args.burn
    cfg = configs.load("burgers_vi_hmc", **over)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    uids = get_list_fnames(cfg.out_dir)
    samples = load_pooled_samples(cfg.out_dir, uids, cfg.burn)
    print(f"pooled {len(uids)} runs, {sum(s.shape[0] for s in samples)} post-burn samples")
    net = DeepONet(cfg.width_branch, cfg.width_trunk, cfg.in_branch, cfg.in_trunk, cfg.branch_depth, cfg.trunk_depth,
                   cfg.activation, cfg.output_neurons)
    mu, sigma, grad_ind = load_vi_artefacts(cfg.prior_file, cfg.prior_uid)
    _, (x1, x2, yv) = get_burgers_data(cfg)
    eng = DeepONetEngine(net.spec, x1.numpy(), trunk_features(x2), yv.numpy(), mu, grad_ind, 0.0, cfg.prior_var ** 0.5,
                         cfg.loss, cfg.tau_out, max_chains=16, device=dev)
    p = (predictive_moments if args.std else predictive)(eng, samples, yv, with_rel_l2=True)
    print_summary(p, yv, with_rel_l2=True)
    np.save(f"{cfg.out_dir}posterior_mean_pooled.npy", p.mean().cpu().numpy().astype(np.float32))
    if args.std:
        sd = p.std(0).cpu()
        ti = args.test_ind
        if not 0 <= ti < sd.shape[0]:
            ti = sd.shape[0] - 1
            print(f"--test-ind {args.test_ind} is outside the {sd.shape[0]} validation functions: using {ti}")
        np.save(f"{cfg.out_dir}prediction_std_{ti}.npy", sd[ti, -NX:].numpy().astype(np.float32))
        np.save(f"{cfg.out_dir}posterior_std_pooled.npy", sd.numpy().astype(np.float32))
        print("\nMean posterior-predictive std: {:.6f}".format(float(sd.mean())))
        if p.n > 1 and sd.shape[1] % NX == 0:
            err, std, corr = error_uncertainty(p.mean().cpu(), p.std(1).cpu(), yv, NX)
            print("Error-vs-sigma over {} time slices: mean |error| {:.6f}, mean sigma {:.6f}, correlation mean {:.4f} "
                  "min {:.4f} max {:.4f}".format(len(corr), float(np.mean(err)), float(np.mean(std)),
                                                 float(np.nanmean(corr)), float(np.nanmin(corr)), float(np.nanmax(corr))))


if __name__ == "__main__":
    main()
