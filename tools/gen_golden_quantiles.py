"""Generate the fixtures of the exact predictive quantiles (tests/golden/q_*.npz) by executing the reference's own files
(build container only; never runs on the GPU box).

Run:  python tools/gen_golden_quantiles.py

The reference has no quantile code to compare with (trainers_regression.py:171 says the sampled ones "could be replaced by
taking the quantiles directly"), so a fixture holds what the reference does compute: the q(f) moments of
marginal_variational_qf_parameters, the noise, the reference flow's own values at the Gauss-Hermite nodes
G(mu + sqrt(2 v) xs_s) -- F can be formed from the reference's numbers alone -- and the reference's SAMPLED quantiles:
numpy.quantile over sample_from_predictive_distribution with S = 200 000 at probs = [0.025, 0.5, 0.975] on 8 rows (all 7 of the tiny case).  The
rows are the ones of the smallest q(f) variance: the samples come from the continuous predictive, the exact quantiles from
its S-node quadrature, and the two are the same distribution only as far as the quadrature resolves
Phi((t - G(f)) / sigma) under q(f), i.e. where sqrt(v) G' is not large against sigma.

The generator asserts, per case, that the roots of the CPU restatement (tests/quantile_model.py) on the reference's node
values lie within six standard errors of a sample quantile, |t_exact - t_sampled| <= 6 sqrt(p (1 - p) / S) / F'(t_exact).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import gen_golden as gg        # noqa: E402  (sets up the reference, the shims and float64)

import math                                 # noqa: E402

import numpy as np                          # noqa: E402
import torch                                # noqa: E402

import gen_golden_flows as gf               # noqa: E402  (rebinds gg.build_reference_model; the original is gf._svgp_model)
import quantile_model as qm                 # noqa: E402
from oracle import tgp_oracle as orc        # noqa: E402


def flow_scalar_params(model, program):
    """Reference nn.Parameters in theta order for every kind: gen_golden.py's rule (tanh steps, per-row blocks skipped) with
    the block table of gen_golden_flows.py for the rest."""
    out = []
    for blk, (kind, K, poff, flags) in zip(model.G_matrix[0].flow_arr, program):
        if flags & orc.FLAG_PER_ROW:
            continue
        if kind == orc.FLOW_STEPTANH:
            for t in blk.flow_arr:
                out += [t.a, t.b, t.c, t.d]
        else:
            out += gf.program_of(type("C", (), {"flow_arr": [blk]}))[1]
    return out


gg.flow_scalar_params = flow_scalar_params      # (gen_golden.load_theta looks the name up at call time)

PROBS = [0.025, 0.5, 0.975]
S_SAMPLES = 200000
ROWS = 8


def build(prob, flow):
    """(reference model in eval state, program, theta, rowp or None)."""
    torch.manual_seed(0)
    if flow is None:
        # the identity flow under the quadrature likelihood: the reference's sparse_MF_GP with GaussianNonLinearMean
        X, p = prob["X"], prob["params"]
        N, D = X.shape
        M = p["Z"].shape[0]
        K = gg.instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False, init_params=gg.KINIT)
        lik = gg.GaussianNonLinearMean(out_dim=1, noise_init=0.05, noise_is_shared=False, quadrature_points=prob["xs"].shape[0])
        model = gg.sparse_MF_GP(["zero", K], X, p["Z"].clone(), N, lik, 1, True, False, False, False, False, 0.0,
                                init_params=gg.IP)
        with torch.no_grad():
            model.Z.data = p["Z"].reshape(1, M, D).clone()
            model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
            model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
            model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
            model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
            model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        prob["program"], p["theta"] = [], torch.zeros(0, dtype=torch.float64)
    elif flow in gf.FLOWS:
        model = gf.build_reference_model(prob, flow)
    else:
        model = gf._svgp_model(prob, flow)
        if flow.startswith("idsal"):
            # network output layers shrunk around the identity flow (a_n ~ 0, b_n ~ 1), as gen_golden.id_model_with_weights
            with torch.no_grad():
                for blk in model.G_matrix[0].flow_arr:
                    if hasattr(blk, "NNets_a"):
                        for nm, bias in (("a", 0.0), ("b", 1.0)):
                            last = list(getattr(blk, "NNets_" + nm))[-1].w
                            last.weight.mul_(0.3)
                            last.bias.fill_(bias)
    model.set_is_training(False)
    model.eval()
    return model


def capture_rowp(model, X):
    """Per-row flow parameters of the rows of X (dropout off): the outputs of the blocks' networks, in program order."""
    captured, hooks = {}, []
    for bi, blk in enumerate(model.G_matrix[0].flow_arr):
        if hasattr(blk, "NNets_a"):
            for nm in ("a", "b"):
                def hook(mod, inp, out, key=(bi, nm)):
                    captured[key] = out.detach().reshape(-1).clone()
                hooks.append(getattr(blk, "NNets_" + nm).register_forward_hook(hook))
    if not hooks:
        return None
    with torch.no_grad():
        model.G_matrix[0](torch.zeros(X.shape[0], dtype=torch.float64), X)
    for h in hooks:
        h.remove()
    return torch.stack([captured[k] for k in sorted(captured)], 1)


def case(name, N, D, M, S, flow, seed=0):
    if flow in gf.FLOWS:
        prob = gf.problem(N, D, M, S, flow, seed)
    else:
        prob = orc.synthetic_problem(N, D, M, seed=seed, flow=flow, S=S)
    model = build(prob, flow)
    X, p = prob["X"], prob["params"]
    xs, ws = prob["xs"], prob["ws"]
    wn = ws / math.sqrt(math.pi)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X.repeat(1, 1, 1), diagonal=True, is_duvenaud=False, init_Z=None)
        mu, v = mu.reshape(-1), v.reshape(-1)
        # the reference's own node values G(mu + sqrt(2 v) xs_s), (S,N) (GaussianNonLinearMean.marginal_moments :180-185)
        f = mu.unsqueeze(0) + torch.sqrt(2.0 * v).unsqueeze(0) * xs.unsqueeze(1)
        g = model.G_matrix[0](f.clone(), X).detach()
        rowp = capture_rowp(model, X)
        rows = torch.argsort(v)[:ROWS].sort().values
        torch.manual_seed(100 + seed)
        samples, _, _ = model.sample_from_predictive_distribution(X[rows], S_SAMPLES)       # (1,S,8,1)
    sampled = torch.tensor(np.quantile(samples[0, :, :, 0].numpy(), PROBS, axis=0))          # (3,8)
    lvn = p["log_var_noise"]
    program = np.array(prob["program"] if len(prob["program"]) else np.zeros((0, 4)), dtype=np.int32)
    # ---- the generator's own check: restatement root on the reference's nodes against the reference's samples
    sigma = math.sqrt(math.exp(float(lvn)))
    t, failed = qm.quantiles(mu, v, lvn, PROBS, xs, wn, program, p["theta"], rowp)
    assert failed == 0, name
    worst = 0.0
    for qi, pr in enumerate(PROBS):
        if len(program):
            _, _, dens = qm.tails(g[:, rows], wn, sigma, t[qi, rows])
        else:
            sd = torch.sqrt(v[rows] + sigma * sigma)
            dens = torch.exp(-0.5 * ((t[qi, rows] - mu[rows]) / sd) ** 2) * qm.INV_SQRT_2PI / sd
        bound = 6.0 * math.sqrt(pr * (1.0 - pr) / S_SAMPLES) / dens
        ratio = ((t[qi, rows] - sampled[qi]).abs() / bound).max()
        worst = max(worst, float(ratio))
        if len(program):
            res = qm.residual(g, wn, sigma, t[qi], pr).max()
        else:       # the identity: one Gaussian of variance v + noise, not its S-node mixture
            res = qm.residual(torch.zeros(1, mu.numel(), dtype=torch.float64), torch.ones(1, dtype=torch.float64), 1.0,
                              (t[qi] - mu) / torch.sqrt(v + sigma * sigma), pr).max()
        print("  %s p=%.3f  |exact - sampled| / bound = %.3f   residual on the reference's nodes %.2e" % (name, pr, float(ratio),
                                                                                                        float(res)))
    assert worst <= 1.0, "%s: sampled quantiles %.3f bounds away" % (name, worst)
    out = {"mu": mu, "v": v, "xs": xs, "ws": ws, "p_log_var_noise": lvn, "p_theta": p["theta"], "program": program,
           "g_nodes": g, "probs": np.array(PROBS), "samp_rows": rows, "samp_S": np.int64(S_SAMPLES), "samp_q": sampled}
    if rowp is not None:
        out["rowp"] = rowp
    gg.save(name, out)


def main():
    case("q_tiny_svgp", 7, 3, 4, 16, None)
    case("q_med_sal2", 65, 4, 20, 32, "sal2")
    case("q_med_tanh3x2", 257, 4, 20, 50, "tanh3x2")
    case("q_bcl_al1", 65, 4, 20, 32, "bcl_al1")
    case("q_idsal1", 65, 4, 20, 32, "idsal1")
    case("q_s100_sal2", 33, 4, 16, 100, "sal2", seed=1)


if __name__ == "__main__":
    main()
