#!/usr/bin/env python3
"""Time the posterior-predictive paths at the bench shape: postprocess.predictive (the [C, N, P] forward output reduced
by torch) against postprocess.predictive_moments (k_predict_moments: running fp64 sums, no output tensor), with and
without the per-sample relative L2 errors.

    python vi-hmc_amd/tools/predictive_time.py [--out profiles/predictive_moments_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python vi-hmc_amd/tools/predictive_time.py --kernel-run
    python vi-hmc_amd/tools/predictive_time.py --kernel-stats DIR/.../run_kernel_stats.csv --out ...   (adds the kernel's own time)

Shape: N = 1000, P = 10,201, K = 17,240, C = 16 of vihmc.data.deeponet_problem(seed=0). After a warm-up of every arm, each
arm is timed over ``--rounds`` windows of ``--batches`` batches (default 8 x 4 = 32 batches per arm), the arms
alternating inside every round; a window is one call of the function between two device events and ends in a
synchronise (both functions read their per-sample lists back, so each also ends synchronised by itself).
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vihmc.data import deeponet_problem  # noqa: E402
from vihmc.engine import DeepONetEngine, trunk_features  # noqa: E402
from vihmc.postprocess import predictive, predictive_moments  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3
C = 16


def setup(dev):
    p = deeponet_problem(seed=0)
    eng = DeepONetEngine(p.spec, p.branch_in, trunk_features(p.trunk_in), p.y, p.mu, p.grad_ind, 0.0, 0.1, "NLL", 1.0,
                         max_chains=C, device=dev)
    rng = np.random.default_rng(1)
    th0 = p.mu[p.grad_ind]
    return p, eng, th0, rng


def kernel_fields(path, N, P, W):
    """k_predict_moments' own time from a rocprofv3 kernel_stats.csv: achieved FLOP/s of its 2 N P W C contraction and
    its HBM bytes counted from shapes (both fp64 states read and written once, the operands of C chains, y)."""
    rows = [r for r in csv.DictReader(open(path)) if "k_predict_moments" in r["Name"]]
    if not rows:
        raise SystemExit(f"no k_predict_moments row in {path}")
    calls = sum(int(r["Calls"]) for r in rows)
    avg_us = sum(float(r["TotalDurationNs"]) for r in rows) / calls / 1e3
    flops = 2.0 * N * P * W * C
    hbm = 2 * 2 * 8.0 * N * P + 4.0 * C * (N + P) * W + 4.0 * N * P
    return {"kernel": "k_predict_moments", "calls": calls, "avg_us": avg_us, "flops_per_launch": flops,
            "achieved_tflops": flops / (avg_us * 1e-6) / 1e12,
            "frac_of_fp32_mfma_peak": flops / (avg_us * 1e-6) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
            "peak_tflops": PEAK_FP32_MFMA_TFLOPS, "hbm_bytes_from_shapes": hbm,
            "hbm_gb_per_s_from_shapes": hbm / (avg_us * 1e-6) / 1e9,
            "note": "accumulate = 1 launches (state read and written); time from rocprofv3 --kernel-trace --stats"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles",
                                                  "predictive_moments_time.json"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--kernel-run", action="store_true", help="only 16 predict_moments batches (the profiler's run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv: add the kernel's time to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        rec = json.load(open(args.out))
        s = rec["shape"]
        rec["kernel"] = kernel_fields(args.kernel_stats, s["N"], s["P"], s["W"])
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["kernel"]))
        return
    dev = torch.device("cuda", 0)
    p, eng, th0, rng = setup(dev)
    N, P = eng.out_shape
    y = torch.from_numpy(p.y)
    nb = args.batches
    th = torch.from_numpy((th0 + 0.01 * rng.standard_normal((nb * C, th0.size))).astype(np.float32)).to(dev)
    if args.kernel_run:
        predictive_moments(eng, [th], y)
        predictive_moments(eng, [torch.cat([th] * 4)], y)
        torch.cuda.synchronize(dev)
        return
    arms = {"predictive": lambda: predictive(eng, [th], y, with_rel_l2=False),
            "predictive_rel_l2": lambda: predictive(eng, [th], y, with_rel_l2=True),
            "moments": lambda: predictive_moments(eng, [th], y, with_rel_l2=False),
            "moments_rel_l2": lambda: predictive_moments(eng, [th], y, with_rel_l2=True)}
    for f in arms.values():                      # warm-up of every path (allocations, first-call work)
        f()
        f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize(dev)
            ms[k].append(e0.elapsed_time(e1) / nb)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"shape": {"N": N, "P": P, "K": int(eng.K), "C": C, "W": int(p.spec.out), "problem": "deeponet_problem(seed=0)"},
           "method": f"{args.rounds} rounds x {nb} batches per arm, arms alternating inside a round, device events around "
                     "one call per window, synchronise after every window, 2 warm-up calls per arm; ms per batch of 16",
           "ms_per_batch_median": med, "ms_per_batch_min": {k: float(np.min(v)) for k, v in ms.items()},
           "ms_per_batch_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "ratio_predictive_over_moments": med["predictive"] / med["moments"],
           "ratio_predictive_over_moments_rel_l2": med["predictive_rel_l2"] / med["moments_rel_l2"],
           "device": torch.cuda.get_device_name(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({k: rec[k] for k in ("ms_per_batch_median", "ratio_predictive_over_moments",
                                          "ratio_predictive_over_moments_rel_l2")}))


if __name__ == "__main__":
    main()
