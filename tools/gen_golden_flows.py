"""Generate the fixtures of the arcsinh / Box-Cox / inverse Box-Cox flow kinds (tests/golden/flows_*.npz) by executing
the reference's own files (build container only; never runs on the GPU box).

Run:  python tools/gen_golden_flows.py

Everything but the flow comes from oracle/gen_golden.py, imported read-only: the reference on sys.path with the
oracle/shims stand-ins, the model builder's parameter recipe (oracle.tgp_oracle.synthetic_problem(flow=None)), the
step-0 / Adam / full-size fixture writers and their key schema (p_*, g_*, program, xs/ws, ELBO/ELL/KLD, history, final_*,
test_logp_sum, pred_m1/pred_m2, data).  This file adds the flows: the reference's generators (dsp/flows.py ArcSL, BoxCoxL,
InverseBoxCoxL, Affine, build_chain) under fixed numpy seeds, their raw values perturbed by 0.3 N(0,1) (lam kept in
[0.5, 2] where the float64 parity tests need it), and the program rows of include/tgp_hip.h.  Fixtures are data only.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from oracle import gen_golden as gg        # noqa: E402  (sets up the reference, the shims and float64)

import numpy as np                          # noqa: E402
import torch                                # noqa: E402

from dsp import flows as rflows             # noqa: E402
from dsp.models.flow import (AffineFlow, ArcsinhFlow, BoxCoxFlow, InverseBoxCoxFlow, Sinh_ArcsinhFlow,  # noqa: E402
                             instance_flow)

from oracle import tgp_oracle as orc        # noqa: E402

FLOW_AFFINE, FLOW_SAL, FLOW_ARCSINH, FLOW_BOXCOX, FLOW_INV_BOXCOX = 0, 1, 3, 4, 5
FLAG_RESTRICT, FLAG_ADD_F0 = 1, 2


def _sal_al_f0(nb):
    specs = []
    for _ in range(nb):
        specs += rflows.SAL(1, add_f0=True) + rflows.ArcSL(1, add_f0=True)
    return specs


# fixture flow name -> (numpy seed, spec generator, lam policy).  lam policy "parity": 1 + 0.3 N(0,1) clipped to [0.5, 2];
# "default": the generator's own value (5) plus the perturbation
FLOWS = {
    "arcsl2": (11, lambda: rflows.ArcSL(2), "parity"),
    "bcl1": (12, lambda: rflows.BoxCoxL(1), "parity"),
    "invbcl1": (13, lambda: rflows.InverseBoxCoxL(1), "parity"),
    "sal_bcl1": (14, lambda: rflows.build_chain("SAL_BCL", 1, constraint=None), "parity"),
    "invbcl_al1": (15, lambda: rflows.build_chain("InvBCL_AL", 1, constraint=None), "parity"),
    "sal_al2f0": (16, lambda: _sal_al_f0(2), "parity"),
    "bcl1lam5": (17, lambda: rflows.BoxCoxL(1), "default"),
    "bcl_al1": (18, lambda: rflows.build_chain("BCL_AL", 1, constraint=None), "parity"),
    "arcsl1": (19, lambda: rflows.ArcSL(1, set_res=True), "parity"),
}


def flow_specs(flow):
    seed, gen, _ = FLOWS[flow]
    np.random.seed(seed)
    return gen()


def program_of(comp):
    """Reference CompositeFlow -> (program rows, [nn.Parameter] in theta order, [is lam] per theta entry)."""
    prog, prm, islam = [], [], []
    for fl in comp.flow_arr:
        poff = len(prm)
        if isinstance(fl, AffineFlow):
            prog.append((FLOW_AFFINE, 0, poff, FLAG_RESTRICT if fl.set_restrictions else 0))
            new, lam = [fl.a, fl.b], [False, False]
        elif isinstance(fl, Sinh_ArcsinhFlow):
            flags = (FLAG_RESTRICT if fl.set_restrictions else 0) | (FLAG_ADD_F0 if fl.add_init_f0 else 0)
            prog.append((FLOW_SAL, 0, poff, flags))
            new, lam = [fl.a, fl.b], [False, False]
        elif isinstance(fl, ArcsinhFlow):
            flags = (FLAG_RESTRICT if fl.set_restrictions else 0) | (FLAG_ADD_F0 if fl.add_init_f0 else 0)
            prog.append((FLOW_ARCSINH, 0, poff, flags))
            new, lam = [fl.a, fl.b, fl.c, fl.d], [False] * 4
        elif isinstance(fl, BoxCoxFlow):        # (InverseBoxCoxFlow is a BoxCoxFlow)
            assert fl.constraint is None
            kind = FLOW_INV_BOXCOX if isinstance(fl, InverseBoxCoxFlow) else FLOW_BOXCOX
            prog.append((kind, 0, poff, FLAG_ADD_F0 if fl.add_init_f0 else 0))
            new, lam = [fl.lam], [True]
        else:
            raise TypeError(type(fl).__name__)
        prm += new
        islam += lam
    return prog, prm, islam


def attach_flow(prob, flow, seed=0):
    """prob (synthetic_problem(flow=None)) -> + program, + params['theta'] (perturbed raw values of the generator's specs)."""
    if prob.get("program") is not None:
        return
    prog, prm, islam = program_of(instance_flow(flow_specs(flow)))
    theta = torch.stack([p.detach().reshape(()) for p in prm]).clone()
    g = torch.Generator().manual_seed(1000 + seed)
    noise = 0.3 * torch.randn(theta.shape, generator=g, dtype=torch.float64)
    lam = torch.tensor(islam)
    if FLOWS[flow][2] == "parity":
        theta = torch.where(lam, (1.0 + noise).clamp(0.5, 2.0), theta + noise)
    else:
        theta = theta + noise
    prob["program"] = prog
    prob["params"]["theta"] = theta


def flow_scalar_params(model, program):
    return program_of(model.G_matrix[0])[1]


def build_reference_model(prob, flow, kernel="scale_rbf"):
    """gen_golden.build_reference_model with the flow taken from FLOWS (and the theta of attach_flow loaded)."""
    attach_flow(prob, flow)
    base = _svgp_model(prob, None, kernel)                      # the SVGP of the same parameters: its kernel and q(u)
    X, p = prob["X"], prob["params"]
    N, D = X.shape
    M = p["Z"].shape[0]
    S = prob["xs"].shape[0]
    K = base.covariance_function
    lik = gg.GaussianNonLinearMean(out_dim=1, noise_init=0.05, noise_is_shared=False, quadrature_points=S)
    model = gg.sparse_MF_SP(["zero", K], X, p["Z"].clone(), N, lik, 1, True, False, False, False, False,
                            [flow_specs(flow)], "single", 0.0, init_params=gg.IP)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        for prm, val in zip(flow_scalar_params(model, prob["program"]), p["theta"]):
            prm.data = val.clone().reshape(prm.shape)
    return model


# the writers of gen_golden.py look these two names up at call time
_svgp_model = gg.build_reference_model
gg.build_reference_model, gg.flow_scalar_params = build_reference_model, flow_scalar_params


def problem(N, D, M, S, flow, seed=0):
    prob = orc.synthetic_problem(N, D, M, seed=seed, flow=None, S=S)
    attach_flow(prob, flow, seed)
    return prob


def power_dc():
    """The committed power_seed1 fixture as the `dc` the full-size writer expects (the reference loader's output)."""
    z = np.load(os.path.join(gg.GOLDEN, "power_seed1.npz"))
    dc = {k: torch.tensor(z[k]) for k in ("X_tr", "Y_tr", "X_te", "Y_te")}
    dc["Y_std"] = z["Y_std"]
    return dc, torch.tensor(z["Z_kmeans_n1_seed0"])


def spec_fixture():
    """The generators' spec lists under fixed numpy seeds (tests/test_flow_kinds_host.py compares this package's)."""
    out = {}
    calls = [("ArcSL", lambda: rflows.ArcSL(2)), ("ArcSL_random", lambda: rflows.ArcSL(2, init_random=True)),
             ("ArcSL_f0", lambda: rflows.ArcSL(1, add_f0=True, set_res=True)),
             ("BoxCoxL", lambda: rflows.BoxCoxL(2)), ("BoxCoxL_random", lambda: rflows.BoxCoxL(2, init_random=True)),
             ("InverseBoxCoxL", lambda: rflows.InverseBoxCoxL(2, add_f0=True)),
             ("InverseBoxCoxL_random", lambda: rflows.InverseBoxCoxL(2, init_random=True)),
             ("Affine", lambda: rflows.Affine(3)), ("Affine_random", lambda: rflows.Affine(3, init_random=True, set_res=True))]
    for ch in ("SAL_BCL", "SAL_InvBCL", "SAL_AL", "BCL_AL", "InvBCL_AL"):
        calls.append((ch, lambda ch=ch: rflows.build_chain(ch, 2, constraint=None)))
    for i, (name, fn) in enumerate(calls):
        np.random.seed(100 + i)
        specs = fn()
        names, values = [], []
        for kind, init in specs:
            names.append(kind)
            row = []
            for key in ("init_a", "init_b", "init_c", "init_d", "init_lam"):
                if key in init:
                    row.append(float(np.asarray(init[key]).reshape(-1)[0]))
            flags = [bool(init.get(k, False)) for k in ("add_init_f0", "set_restrictions")]
            values.append(row + [float(f) for f in flags] + [np.nan] * (6 - len(row) - 2))
        out[name + ".seed"] = np.int64(100 + i)
        out[name + ".names"] = np.array(names)
        out[name + ".values"] = np.array(values, dtype=np.float64)
    gg.save("flows_specs", out)


def main():
    spec_fixture()
    tiny = ["arcsl2", "bcl1", "invbcl1", "sal_bcl1", "invbcl_al1", "sal_al2f0"]
    for flow in tiny:
        gg.reference_step0(problem(64, 3, 8, 8, flow), flow, "flows_tiny_" + flow)
    for flow in ("arcsl2", "sal_bcl1", "invbcl_al1", "bcl1lam5"):
        gg.reference_step0(problem(512, 4, 60, 16, flow), flow, "flows_med_" + flow)
    # general-M path (M > 128)
    for flow in ("sal_bcl1", "invbcl_al1"):
        gg.reference_step0(problem(300, 4, 136, 8, flow), flow, "flows_bigm_" + flow)
    for flow in ("arcsl2", "sal_bcl1"):
        gg.reference_adam_steps(problem(64, 3, 8, 8, flow), flow, "flows_adam5_" + flow)
    dc, Z = power_dc()
    for flow in ("arcsl1", "bcl_al1"):
        _full_size(dc, Z, flow, "flows_power_" + flow)


def _full_size(dc, Z, flow, name):
    """gen_golden.full_size_fixture for a FLOWS name (its problem_on would hand the name to synthetic_problem)."""
    real = gg.problem_on

    def problem_on(dc_, Z_, flow_, S, perturb, seed=0):
        prob = real(dc_, Z_, None, S, perturb, seed)
        attach_flow(prob, flow_, seed)
        return prob
    gg.problem_on = problem_on
    try:
        gg.full_size_fixture(dc, "power_seed1", Z, flow, name)
    finally:
        gg.problem_on = real


if __name__ == "__main__":
    main()
