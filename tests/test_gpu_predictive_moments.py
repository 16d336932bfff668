"""The fused posterior-predictive moments path on the GPU: vihmc_predict_moments (k_predict_moments) through
DeepONetEngine.predict_moments and postprocess.predictive_moments.

The running sums are compared BITWISE with a Python loop over ``engine.forward``'s outputs in chain order (every S the
kernel folds in is the forward's fp32 value, the fp64 square of an fp32 value is exact, and the additions run in chain
order); the per-function squared errors and the log-probability, which sum the same fp64 terms in another order,
against bounds of 4x the measured maximum (tests/parity.py; registered below). The reference-generated fixture
tests/golden/deeponet_predictive_std.npz sets the accuracy bar of the standard deviation itself.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity
from goldens import bnn_case, deeponet_case, load

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCRIPTS = os.path.join(ROOT, "vi-hmc_amd", "scripts")

# quantities of this module (dimensionless):
#   moment_maxabs   max |sum - forward-loop sum| over both states (bitwise: bound 0)
#   sse_rel         max over (sample, function) of |sse_rows - ref| / ref
#   mse_rel, rel_l2_rel   the same for predictive()'s per-sample MSE / relative L2 lists
#   std_err_ratio, mean_err_ratio   error of the engine's std / mean against the fixture's fp64 values over the error
#                   of the reference's own fp32 values (bar: 2, the bar test_gram_precision_vs_fit uses)
parity.LOOSE.update({"moment_maxabs": 0.0, "sse_rel": 1e-6, "mse_rel": 1e-4, "rel_l2_rel": 1e-4, "std_err_ratio": 2.0,
                     "mean_err_ratio": 2.0})
# Bounds: 4x the maximum measured on the MI355X (profiles/predictive_moments_parity.json, the calibration run of this
# module), rounded up to one digit, as tests/parity.py's own table. Where the measured maximum is 0 and the two sides
# sum the same fp64 terms in different orders, the bound is the floor parity.py uses for such pairs (one fp32 ulp-level
# difference of the rounded result, 2e-07); the std / mean ratios keep the fixed bar of 2 (measured <= 1.02).
parity.BOUNDS.update({
    ("test_moments_bitwise_against_forward", "moment_maxabs"): 0.0,   # bitwise
    ("test_moments_bitwise_against_forward", "sse_rel"): 9e-16,   # max 2.20e-16 over 3
    ("test_moments_bitwise_against_forward", "logp_rel"): 2e-07,   # max 0 over 3 (floor)
    ("test_ragged_multi_tile", "moment_maxabs"): 0.0,   # bitwise
    ("test_ragged_multi_tile", "sse_rel"): 2e-15,   # max 3.97e-16 over 2
    ("test_ragged_multi_tile", "logp_rel"): 2e-07,   # max 0 over 2 (floor)
    ("test_masked_targets", "moment_maxabs"): 0.0,   # bitwise
    ("test_masked_targets", "sse_rel"): 6e-16,   # max 1.43e-16 over 1
    ("test_masked_targets", "logp_rel"): 2e-07,   # max 0 over 1 (floor)
    ("test_reference_std_fixture", "std_err_ratio"): 2.0,   # max 1.012 over 2 (the bar, not 4x)
    ("test_reference_std_fixture", "mean_err_ratio"): 2.0,   # max 0.954 over 2 (the bar, not 4x)
    ("test_predictive_moments_agrees_with_predictive", "mse_rel"): 5e-07,   # max 1.21e-07 over 1 (predictive()'s fp32 mean)
    ("test_predictive_moments_agrees_with_predictive", "rel_l2_rel"): 4e-08,   # max 9.51e-09 over 1
    ("test_predictive_moments_agrees_with_predictive", "logp_rel"): 2e-07,   # max 0 over 1 (floor)
    ("test_predictive_moments_agrees_with_predictive", "mean_rel_l2"): 2e-15,   # max 0 over 1 (floor: 7 fp64 additions
                                                                               # in another order, 7 x 2.2e-16)
    ("test_post_process_script_std", "mean_rel_l2"): 2e-07,   # max 0 over 1 (floor: the saved means are rounded to fp32)
})


def engine_for(c, max_chains, device, y=None):
    from vihmc.engine import DeepONetEngine, trunk_features
    p = c.prob
    return DeepONetEngine(c.spec, p.branch_in, trunk_features(p.trunk_in), p.y if y is None else y, p.mu, p.grad_ind,
                          c.prior_mu, c.prior_sd, c.loss, c.tau_out, max_chains=max_chains, device=device)


def jittered(c, n, seed=17, scale=0.01):
    """n sample vectors: the case's thetas, then seeded jitters of its first."""
    rng = np.random.default_rng(seed)
    th = [np.asarray(t, np.float32) for t in c.thetas]
    while len(th) < n:
        th.append((th[0] + scale * rng.standard_normal(th[0].size)).astype(np.float32))
    return np.stack(th[:n])


def forward_loop(eng, th, y, masked=False):
    """(sum1, sum2, sse_rows [S, N], logp [S]) from engine.forward, max_chains samples per call, chain order."""
    a1 = torch.zeros(eng.out_shape, dtype=torch.float64, device=eng.device)
    a2 = torch.zeros_like(a1)
    sse, lps = [], []
    yd = torch.as_tensor(y).to(eng.device).reshape(eng.out_shape)
    for i in range(0, th.shape[0], eng.max_chains):
        lp, out = eng.forward(th[i:i + eng.max_chains])
        for c in range(out.shape[0]):
            a1 += out[c].double()
            a2 += out[c].double() ** 2
        r = (out - yd).double()
        if masked:
            r = torch.where(torch.isnan(yd), torch.zeros_like(r), r)
        sse.append((r * r).sum(-1))
        lps.append(lp)
    return a1, a2, torch.cat(sse), torch.cat(lps)


def moments(eng, th, cuts=None, pad=0, sentinel=-7.5):
    """(sum1, sum2, sse_rows, logp, tails) from predict_moments, the samples cut into calls of ``cuts`` (default:
    max_chains each); accumulate = 0 on the first call over a NaN-filled state. pad > 0: ``pad`` sentinel doubles behind
    each state array, returned as ``tails``."""
    N, P = eng.out_shape
    raw = [torch.full((N * P + pad,), float("nan"), dtype=torch.float64, device=eng.device) for _ in range(2)]
    for r in raw:
        r[N * P:] = sentinel
    s1, s2 = (r[:N * P].view(N, P) for r in raw)
    cuts = cuts or [eng.max_chains] * -(-th.shape[0] // eng.max_chains)
    sse, lps, i = [], [], 0
    for k, n in enumerate(cuts):
        part = th[i:i + n]
        rows = torch.full((part.shape[0], N), float("nan"), dtype=torch.float64, device=eng.device)
        lps.append(eng.predict_moments(part, s1, s2, accumulate=k > 0, sse_rows=rows))
        sse.append(rows)
        i += n
    assert i >= th.shape[0]
    return s1, s2, torch.cat(sse), torch.cat(lps), [r[N * P:] for r in raw]


def check_against_forward(eng, th, y, masked=False, cuts=None, pad=0, note=""):
    a1, a2, sse_ref, lp_ref = forward_loop(eng, th, y, masked)
    s1, s2, sse, lp, tails = moments(eng, th, cuts, pad)
    d = max(float((s1 - a1).abs().max()), float((s2 - a2).abs().max()))
    print(f"{note}: moment max abs diff {d:.3e}")
    parity.check("moment_maxabs", d if np.isfinite(d) else np.inf, note)
    assert torch.equal(s1, a1) and torch.equal(s2, a2)
    e_sse = float(((sse - sse_ref).abs() / sse_ref.abs().clamp_min(1e-300)).max())
    e_lp = float(((lp - lp_ref).abs() / lp_ref.abs().clamp_min(1.0)).max())
    print(f"{note}: sse_rel {e_sse:.3e} logp_rel {e_lp:.3e}")
    parity.check("sse_rel", e_sse, note)
    parity.check("logp_rel", e_lp, note)
    for t in tails:
        assert bool((t == -7.5).all()), "sentinel behind a state array overwritten"
    return s1, s2, sse, lp


# ---- 1. bitwise against the forward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deeponet_small", "deeponet_odd_full", "deeponet_refshape"])
def test_moments_bitwise_against_forward(name, cuda_device):
    c = deeponet_case(name)
    eng = engine_for(c, 4, cuda_device)
    th = torch.tensor(jittered(c, 4), device=cuda_device)
    check_against_forward(eng, th, c.prob.y, note=name)
    # sse_rows is optional; without it the log-probability is the same
    N, P = eng.out_shape
    s1 = torch.empty(N, P, dtype=torch.float64, device=cuda_device)
    s2 = torch.empty_like(s1)
    lp0 = eng.predict_moments(th, s1, s2, accumulate=False)
    rows = torch.empty(4, N, dtype=torch.float64, device=cuda_device)
    lp1 = eng.predict_moments(th, s1.clone(), s2.clone(), accumulate=False, sse_rows=rows)
    assert torch.equal(lp0, lp1)
    eng.close()


# ---- 2. batch-split invariance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deeponet_odd_full", "deeponet_refshape"])
def test_batch_split_invariance(name, cuda_device):
    c = deeponet_case(name)
    th = torch.tensor(jittered(c, 16), device=cuda_device)
    e16 = engine_for(c, 16, cuda_device)
    one = moments(e16, th, cuts=[16])
    split = moments(e16, th, cuts=[5, 5, 6])
    e16.close()
    e3 = engine_for(c, 3, cuda_device)
    six = moments(e3, th, cuts=[3, 3, 3, 3, 3, 1])
    e3.close()
    for other in (split, six):
        assert torch.equal(one[0], other[0]) and torch.equal(one[1], other[1])
        assert torch.equal(one[2], other[2])                   # per-sample sums: no cross-sample term at all
    assert torch.isfinite(one[0]).all() and torch.isfinite(one[1]).all()


# ---- 3. ragged multi-tile --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_problem():
    """N = 131 = 2 x 64 + 3 and P = 273 = 2 x 128 + 17: three tiles each way, the last one ragged (k_predict_moments'
    workgroup tile is 64 x 128, its wave tile 64 x 32), width 100."""
    from types import SimpleNamespace
    from vihmc.data import deeponet_problem
    p = deeponet_problem(seed=21, n=131, nt=13, nx=21, k=17240)
    assert p.y.shape == (131, 273)
    th0 = p.mu[p.grad_ind]
    return SimpleNamespace(spec=p.spec, prob=p, thetas=[th0], prior_mu=0.0, prior_sd=0.1, loss="NLL", tau_out=1.0)


@pytest.mark.parametrize("C", [16, 3])
def test_ragged_multi_tile(C, ragged_problem, cuda_device, monkeypatch):
    c = ragged_problem
    monkeypatch.setenv("VIHMC_CANARY", "1")
    eng = engine_for(c, C, cuda_device)
    monkeypatch.delenv("VIHMC_CANARY")
    th = torch.tensor(jittered(c, 2 * C), device=cuda_device)       # two calls: accumulate = 0, then 1
    check_against_forward(eng, th, c.prob.y, pad=64, note=f"ragged C={C}")
    assert eng.check_canaries() == 0
    eng.close()


# ---- 4. against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deeponet_small", "deeponet_refshape"])
def test_reference_std_fixture(name, cuda_device):
    """The 12 fixture samples through predictive_moments: the error of the engine's std against the fp64 oracle's is
    at most twice the error of the reference's own fp32 np.std (measured on the CPU: 6.27e-7 deeponet_small, 3.11e-7
    deeponet_refshape; fp64 moments of the reference's fp32 predictions score 6.26e-7 / 3.08e-7, so all of it is the
    fp32 forward's). Likewise the mean."""
    from golden.make_golden_predictive import predictive_thetas
    from vihmc.postprocess import predictive_moments
    c = deeponet_case(name)
    g = load("deeponet_predictive_std")
    eng = engine_for(c, 5, cuda_device)                              # batches of 5 + 5 + 2
    th = torch.from_numpy(predictive_thetas(c.thetas[0]))
    p = predictive_moments(eng, [th], torch.from_numpy(c.prob.y))
    assert p.n == 12

    def err(a, ref):
        return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / np.linalg.norm(ref))

    e_ref, e_eng = err(g[f"{name}_std32"], g[f"{name}_std64"]), err(p.std().cpu().numpy(), g[f"{name}_std64"])
    m_ref, m_eng = err(g[f"{name}_mean32"], g[f"{name}_mean64"]), err(p.mean().cpu().numpy(), g[f"{name}_mean64"])
    print(f"{name}: std e_eng {e_eng:.3e} e_ref {e_ref:.3e} ratio {e_eng / e_ref:.3f}; "
          f"mean e_eng {m_eng:.3e} e_ref {m_ref:.3e} ratio {m_eng / m_ref:.3f}")
    parity.check("std_err_ratio", e_eng / e_ref, name)
    parity.check("mean_err_ratio", m_eng / m_ref, name)
    assert e_eng <= 2 * e_ref and m_eng <= 2 * m_ref
    eng.close()


# ---- 5. masked targets and trunk rows --------------------------------------------------------------------------------
def test_masked_targets(cuda_device):
    c = deeponet_case("deeponet_small")
    y = c.prob.y.copy()
    rng = np.random.default_rng(5)
    hole = rng.random(y.shape) < 0.2
    hole[1, :] = False
    y[hole] = np.nan
    eng = engine_for(c, 4, cuda_device, y=y)
    eng.option("y_masked", 1)
    eng.option("lik_count", int((~hole).sum()))
    th = torch.tensor(jittered(c, 4), device=cuda_device)
    _, _, sse, lp = check_against_forward(eng, th, y, masked=True, note="masked")
    assert torch.isfinite(sse).all() and torch.isfinite(lp).all()
    eng.close()


def test_after_set_trunk_rows_equals_fresh_plan(cuda_device):
    from types import SimpleNamespace
    from vihmc.engine import trunk_features
    c = deeponet_case("deeponet_refshape")
    p = c.prob
    P_all = p.y.shape[1]
    ind = np.sort(np.random.default_rng(9).choice(P_all, 77, replace=False))
    sub = SimpleNamespace(spec=c.spec, prior_mu=c.prior_mu, prior_sd=c.prior_sd, loss=c.loss, tau_out=c.tau_out,
                          prob=SimpleNamespace(branch_in=p.branch_in, trunk_in=p.trunk_in[:, ind], y=p.y[:, ind], mu=p.mu,
                                               grad_ind=p.grad_ind))
    first = SimpleNamespace(**{**vars(sub), "prob": SimpleNamespace(**{**vars(sub.prob), "trunk_in": p.trunk_in[:, :77],
                                                                       "y": p.y[:, :77]})})
    th = torch.tensor(jittered(c, 3), device=cuda_device)
    fresh = engine_for(sub, 3, cuda_device)
    want = moments(fresh, th)
    fresh.close()
    eng = engine_for(first, 3, cuda_device)                          # built on other rows, then moved to `ind`
    eng.set_sample_grid(torch.tensor(trunk_features(p.trunk_in), device=cuda_device), torch.tensor(p.y, device=cuda_device))
    eng.set_trunk_rows(ind)
    got = moments(eng, th)
    eng.close()
    for a, b in zip(want[:4], got[:4]):
        assert torch.equal(a, b)


# ---- 6. API ----------------------------------------------------------------------------------------------------------
def test_predictive_moments_agrees_with_predictive(cuda_device):
    from vihmc.postprocess import predictive, predictive_moments
    c = deeponet_case("deeponet_refshape")
    eng = engine_for(c, 3, cuda_device)
    th = torch.from_numpy(jittered(c, 7))
    y = torch.from_numpy(c.prob.y)
    sets = [th[:4], th[4:]]                                          # two "files": batches of 3 + 1 and 3
    old = predictive(eng, sets, y, with_rel_l2=True)
    new = predictive_moments(eng, sets, y, with_rel_l2=True)
    assert old.n == new.n == 7 and old.pred_sqsum is None and new.pred_sqsum is not None
    assert len(new.mse) == len(new.log_prob) == len(new.rel_l2) == 7
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) /   # noqa: E731
                                    np.maximum(np.abs(np.asarray(b, np.float64)), 1e-300)))
    parity.check("mse_rel", rel(new.mse, old.mse))
    parity.check("rel_l2_rel", rel(np.stack(new.rel_l2), np.stack(old.rel_l2)))
    parity.check("logp_rel", float(np.max(np.abs(np.array(new.log_prob) - np.array(old.log_prob)) /
                                          np.maximum(np.abs(np.array(old.log_prob)), 1.0))))
    # predictive() sums each batch before adding it to the running sum: not the chain order, so not bitwise
    m_old, m_new = old.mean().cpu().numpy(), new.mean().cpu().numpy()
    parity.check("mean_rel_l2", float(np.linalg.norm(m_new - m_old) / np.linalg.norm(m_old)))
    assert float(new.std().min()) >= 0.0 and torch.isfinite(new.std()).all()
    lo, hi = new.band()
    assert bool((hi >= lo).all())
    eng.close()


def test_mlp_fallback_and_mlp_plan_error(cuda_device):
    from vihmc.engine import MLPEngine
    from vihmc.postprocess import predictive_moments
    b = bnn_case("bnn_vi_hmc")
    eng = MLPEngine(b.spec, b.data["x_train"], b.data["y_train"], b.g["mu"], b.idx, b.prior_mu, b.prior_sd, b.loss,
                    b.tau_out, max_chains=3, device=cuda_device)
    rng = np.random.default_rng(2)
    th = torch.from_numpy(np.stack([(b.thetas[0] + 0.05 * rng.standard_normal(b.thetas[0].size)).astype(np.float32)
                                    for _ in range(7)]))
    p = predictive_moments(eng, [th], torch.from_numpy(np.asarray(b.data["y_train"], np.float32)), with_rel_l2=True)
    outs = torch.cat([eng.forward(th[i:i + 3].to(cuda_device))[1] for i in range(0, 7, 3)]).double().cpu().numpy()
    assert p.n == 7 and len(p.mse) == len(p.rel_l2) == 7
    np.testing.assert_allclose(p.std().cpu().numpy(), np.std(outs, axis=0), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(p.mean().cpu().numpy(), np.mean(outs, axis=0), rtol=1e-12)
    # the C entry on an MLP plan: an error with a message, not a crash
    N, od = eng.out_shape
    s1 = torch.zeros(N, od, dtype=torch.float64, device=cuda_device)
    s2 = torch.zeros_like(s1)
    lp = torch.zeros(1, device=cuda_device)
    t1 = th[:1].to(cuda_device).contiguous()
    rc = eng.L.vihmc_predict_moments(eng._plan, t1.data_ptr(), 1, lp.data_ptr(), s1.data_ptr(), s2.data_ptr(), 0, None,
                                     ctypes.c_void_p(0))
    assert rc != 0 and b"DeepONet plans only" in eng.L.vihmc_last_error()
    rc = eng.L.vihmc_predict_moments(eng._plan, t1.data_ptr(), 1, lp.data_ptr(), None, s2.data_ptr(), 0, None,
                                     ctypes.c_void_p(0))
    assert rc != 0 and b"null" in eng.L.vihmc_last_error()
    assert not hasattr(eng, "predict_moments")
    eng.close()


def test_predict_moments_argument_checks(cuda_device):
    c = deeponet_case("deeponet_small")
    eng = engine_for(c, 2, cuda_device)
    th = torch.tensor(jittered(c, 2), device=cuda_device)
    N, P = eng.out_shape
    ok = torch.zeros(N, P, dtype=torch.float64, device=cuda_device)
    with pytest.raises(ValueError):
        eng.predict_moments(th, ok, ok)                               # one tensor for both states
    with pytest.raises(ValueError):
        eng.predict_moments(th, ok.float(), torch.zeros_like(ok))     # fp32 state
    with pytest.raises(ValueError):
        eng.predict_moments(th, ok, torch.zeros(N, P + 1, dtype=torch.float64, device=cuda_device))
    with pytest.raises(ValueError):
        eng.predict_moments(th, ok, torch.zeros_like(ok), sse_rows=torch.zeros(3, N, dtype=torch.float64,
                                                                                device=cuda_device))
    eng.close()


# ---- 7. script -------------------------------------------------------------------------------------------------------
def _run(script, args, cwd):
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, cwd=cwd, capture_output=True, text=True,
                       timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout


def test_post_process_script_std(tmp_path):
    """post_process_burgers.py --std on a small saved run (the flow of test_vi_hmc_burgers_sample_evaluate_and_pool):
    both artefacts with their shapes, the pooled mean that of the run without the flag, whose output has no new line."""
    out = str(tmp_path / "samples") + "/"
    _run("main_VI_HMC_burgers.py", ["--num-samples", "6", "--chains", "2", "--n-train", "12", "--out-dir", out], tmp_path)
    plain = _run("post_process_burgers.py", ["--out-dir", out, "--burn", "1", "--n-train", "12"], tmp_path)
    mean_plain = np.load(os.path.join(out, "posterior_mean_pooled.npy"))
    assert "Mean Relative L2 error" in plain and "pooled 2 runs" in plain
    assert "std" not in plain and "sigma" not in plain
    assert not [f for f in os.listdir(out) if "std" in f]
    so = _run("post_process_burgers.py", ["--out-dir", out, "--burn", "1", "--n-train", "12", "--std", "--test-ind", "7"],
              tmp_path)
    assert "Mean Relative L2 error" in so and "Mean posterior-predictive std" in so and "Error-vs-sigma" in so
    sd = np.load(os.path.join(out, "prediction_std_7.npy"))
    full = np.load(os.path.join(out, "posterior_std_pooled.npy"))
    mean_std = np.load(os.path.join(out, "posterior_mean_pooled.npy"))
    assert sd.shape == (101,) and sd.dtype == np.float32
    assert full.shape == mean_plain.shape and full.shape[0] == 12 and full.dtype == np.float32
    assert np.array_equal(sd, full[7, -101:]) and (full >= 0).all() and full.max() > 0
    parity.check("mean_rel_l2", float(np.linalg.norm(mean_std.astype(np.float64) - mean_plain) /
                                      np.linalg.norm(mean_plain.astype(np.float64))))
    # the lines both runs print are the same text up to the last digits of the fp32 / fp64 reductions
    head = [ln for ln in plain.splitlines() if ln.startswith("pooled")]
    assert head and head == [ln for ln in so.splitlines() if ln.startswith("pooled")]
