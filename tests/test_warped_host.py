"""CPU: the warped Gaussian likelihood (WGP) without a GPU -- the torch restatement of csrc/tgp_warp.hip (tests/warp_model.py)
against the reference's fixtures (tests/golden/warp_*.npz, tools/gen_golden_warped.py), the flow inverse's round trip for
every kind, the fixture-set size rule, the class surface, the ABI constant / exports and the command line.

Round-trip bounds (measured here, float64, the grids of `roundtrip_inputs`): one per case, ROUNDTRIP_CPU[case] =
(worst |T(T^-1(t)) - t| / max(1, |t|), worst |T^-1(T(y)) - y| / max(1, |y|)).  The bracketed-Newton cases (tanh steps, ADD_F0)
measure between 2.2e-16 (tanh3) and 1.25e-15 (sal_f0); the largest residual of all, 2.15e-14, belongs to a closed-form chain
(affine + SAL).  This file holds the restatement to 2x each figure (head room for another libm); the GPU test allows the
device 10x each figure, case by case, with zero non-converged elements."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_model as wm          # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
F64 = torch.float64

STEP0 = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "warp_*.npz"))
               if "adam5" not in p and "param_names" not in p)
EXPECTED = ["warp_bigm_sal2", "warp_med_arcsl2", "warp_med_matern_sal2", "warp_med_sal2", "warp_med_sal_al1", "warp_med_tanh3x2",
            "warp_tiny_bcl_al1", "warp_tiny_empty", "warp_tiny_sal2"]

# measured per case by test_round_trip_all_kinds (it prints both figures): (residual in t, error in y), see the docstring
ROUNDTRIP_CPU = {
    "affine_sal": (2.148e-14, 1.475e-14),
    "sal_f0": (1.252e-15, 6.767e-16),
    "tanh3": (2.184e-16, 2.632e-16),
    "tanh2_affine": (3.584e-16, 3.947e-16),
    "arcsinh": (1.407e-15, 1.087e-15),
    "arcsinh_f0": (7.858e-16, 6.579e-16),
    "boxcox": (4.374e-16, 3.829e-16),
    "inv_boxcox": (2.997e-16, 4.574e-16),
    "boxcox_f0": (3.037e-16, 2.393e-16),
    "sal_al_f0": (8.327e-16, 1.974e-15),
    "per_row_sal": (6.837e-15, 4.014e-15),
    "inv_boxcox_f0": (2.678e-16, 3.823e-16),
    "sal_restrict": (3.129e-15, 1.805e-15),
}
CPU_HEADROOM = 2.0          # this file's own assert: the same restatement on another host libm


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def load(name):
    return wm.load_case(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_fixture_set_is_complete_and_small():
    assert STEP0 == EXPECTED
    files = glob.glob(os.path.join(GOLDEN, "warp_*.npz"))
    assert len(files) == len(EXPECTED) + 3           # + two Adam histories and the parameter names
    sizes = [os.path.getsize(f) for f in files]
    assert max(sizes) <= 300 * 1024 and sum(sizes) <= 1.5 * 1024 * 1024


@pytest.mark.parametrize("name", EXPECTED)
def test_restatement_matches_reference(name):
    z = load(name)
    assert float(z["min_dT"]) > 0.0
    theta = z["p_theta"].clone().requires_grad_(True)
    mu, v = z["mu"].clone().requires_grad_(True), z["v"].clone().requires_grad_(True)
    lvn = z["p_log_var_noise"].clone().requires_grad_(True)
    ell, ld, t = wm.ell_warp_torch(z["Y"].reshape(-1), mu, v, lvn, z["program"], theta)
    assert rel(ell.detach(), z["lik_ELL"]) < 1e-10
    assert rel(ld.detach(), z["logdet"]) < 1e-10
    assert rel(t.detach(), z["t"]) < 1e-12
    ell.backward()
    assert rel(mu.grad, z["g_mu"]) < 1e-10 and rel(v.grad, z["g_v"]) < 1e-10
    assert rel(lvn.grad, z["lik_g_log_var_noise"]) < 1e-10
    if z["program"]:
        assert rel(theta.grad, z["lik_g_theta"]) < 1e-10
    # N / MB = 1 in every fixture: the full ELBO's likelihood term is the same number
    assert rel(ell.detach(), z["ELL"]) < 1e-10 and rel(z["ELL"] - z["KLD"], z["ELBO"]) < 1e-12


@pytest.mark.parametrize("name", [n for n in EXPECTED if "bcl" not in n and "tanh" not in n])
def test_inverse_and_moments_match_reference(name):
    z = load(name)
    x, nfail = wm.inverse_torch(z["inv_grid"], z["program"], z["p_theta"])
    assert nfail == 0 and rel(x, z["inv_x"]) < 1e-12
    wn = z["ws"] / np.sqrt(np.pi)
    m1, m2, _ = wm.predict_torch(z["pred_mu"], z["pred_v"], z["p_log_var_noise"], z["program"], z["p_theta"], z["xs"], wn)
    assert rel(m1, z["pred_m1"]) < 1e-12 and rel(m2, z["pred_m2"]) < 1e-12


def sp_inv(x):
    return float(np.log(np.expm1(x)))


# (program, theta, rowp columns or None): every kind, with and without ADD_F0 / RESTRICT, a PER_ROW program
ROUNDTRIP_CASES = {
    "affine_sal": ([(0, 0, 0, 1), (1, 0, 2, 0)], [sp_inv(1.3), -0.2, 0.3, 1.2], None),
    "sal_f0": ([(1, 0, 0, 2 | 1)], [0.2, sp_inv(0.8)], None),
    "tanh3": ([(2, 3, 0, 2)], [0.1, sp_inv(0.6), -0.5, sp_inv(0.7), -0.2, sp_inv(0.4), 0.4, sp_inv(0.5), 0.05, sp_inv(0.3), 1.1,
                               sp_inv(0.9)], None),
    "tanh2_affine": ([(2, 2, 0, 2), (0, 0, 8, 0)], [0.1, sp_inv(0.6), -0.5, sp_inv(0.7), -0.2, sp_inv(0.4), 0.4, sp_inv(0.5), 1.4,
                                                     0.3], None),
    "arcsinh": ([(3, 0, 0, 0)], [0.1, 1.5, -0.3, 0.8], None),
    "arcsinh_f0": ([(3, 0, 0, 2 | 1)], [0.1, sp_inv(1.5), -0.3, sp_inv(0.8)], None),
    "boxcox": ([(4, 0, 0, 0)], [0.7], None),
    "inv_boxcox": ([(5, 0, 0, 0)], [1.4], None),
    "boxcox_f0": ([(4, 0, 0, 2)], [1.6], None),
    "sal_al_f0": ([(1, 0, 0, 2), (0, 0, 2, 0), (3, 0, 4, 2 | 1), (0, 0, 8, 0)],
                  [0.1, 0.9, 1.1, -0.1, 0.2, sp_inv(0.7), 0.1, sp_inv(1.2), 0.9, 0.05], None),
    "per_row_sal": ([(1, 0, 0, 4), (0, 0, 0, 0)], [1.2, 0.1], "sal"),
    "inv_boxcox_f0": ([(5, 0, 0, 2)], [1.4], None),
    "sal_restrict": ([(1, 0, 0, 1)], [-0.3, sp_inv(1.1)], None),
}
# likelihood-only cases (test_gpu_warped.test_ell_warp_matches_autograd): tanh steps without ADD_F0 have a bounded range and
# flat ends, where an inverse is ill-conditioned -- forward and adjoints only
ELL_EXTRA_CASES = {
    "tanh3_nof0": ([(2, 3, 0, 0)], ROUNDTRIP_CASES["tanh3"][1], None),
}


def roundtrip_inputs(name, device="cpu"):
    prog, theta, rp = (ROUNDTRIP_CASES.get(name) or ELL_EXTRA_CASES[name])
    theta = torch.tensor(theta, dtype=F64, device=device)
    y = torch.linspace(0.3, 4.0, 129, dtype=F64, device=device) if "boxcox" in name else \
        torch.linspace(-3.0, 3.0, 129, dtype=F64, device=device)
    rowp = None
    if rp is not None:
        g = torch.Generator().manual_seed(5)
        rowp = (torch.tensor([0.0, 1.0], dtype=F64) + 0.2 * torch.randn(129, 2, generator=g, dtype=F64)).to(device)
    return prog, theta, y, rowp


def round_trip_figures(t, t2, x, y):
    """(worst |t2 - t| / max(1, |t|), worst |x - y| / max(1, |y|))"""
    return (float(((t2 - t).abs() / t.abs().clamp(min=1.0)).max()), float(((x - y).abs() / y.abs().clamp(min=1.0)).max()))


def test_round_trip_all_kinds():
    """T(T^-1(t)) over a grid of t = T(y) for every kind, the Newton blocks included: nothing fails to converge, and each
    case stays within its recorded figures (which the GPU test scales by 10)."""
    assert sorted(ROUNDTRIP_CPU) == sorted(ROUNDTRIP_CASES)
    for name in ROUNDTRIP_CASES:
        prog, theta, y, rowp = roundtrip_inputs(name)
        t, _ = wm.flow_forward(y, prog, theta, rowp)
        x, nfail = wm.inverse_torch(t, prog, theta, rowp)
        assert nfail == 0, name
        t2, _ = wm.flow_forward(x, prog, theta, rowp)
        r, e = round_trip_figures(t, t2, x, y)
        print("round trip %-14s %.3e   |x - y| %.3e" % (name, r, e))
        assert r <= CPU_HEADROOM * ROUNDTRIP_CPU[name][0] and e <= CPU_HEADROOM * ROUNDTRIP_CPU[name][1], name


def test_newton_reports_what_it_cannot_invert():
    """A target outside a bounded block's range: counted, never an endless loop."""
    prog, theta, _, _ = roundtrip_inputs("tanh3")
    prog = [(2, 3, 0, 0)]                          # no ADD_F0: the range is bounded
    x, nfail = wm.inverse_torch(torch.tensor([0.0, 50.0], dtype=F64), prog, theta)
    assert nfail == 1


def test_class_surface_and_parameter_names():
    from tgp.pytorch_amd import likelihoods
    from tgp.pytorch_amd.flows import SAL
    z = np.load(os.path.join(GOLDEN, "warp_param_names.npz"))
    lik = likelihoods.WarpedGaussianLinearMean(1, 0.05, False, SAL(2), 16)
    assert isinstance(lik, likelihoods.GaussianLinearMean) and isinstance(lik.flow, torch.nn.ModuleList) and len(lik.flow) == 1
    assert lik.quad_points == 16
    assert [n for n, _ in lik.named_parameters()] == list(z["lik_param_names"])
    for meth in ("expected_log_prob", "marginal_moments", "unwarped_marginal_moments", "sample_from_output", "log_marginal"):
        assert callable(getattr(lik, meth))
    assert callable(lik.flow[0].inverse)


def test_abi_constant_and_exports():
    from tgp.pytorch_amd import lib as L
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_WARPED 4\b", hdr) and L.LIK_WARPED == 4
    for sym in ("tgp_ell_warp_f64", "tgp_ell_warp_workspace_bytes", "tgp_flow_inverse_f64"):
        assert sym in L.EXPORTS and re.search(r"\b%s\s*\(" % sym, hdr)
    lib = L.load()
    # host-only queries: the warped step's workspace = the Gaussian step's + targets, moments and partials
    g = lib.tgp_workspace_bytes_plan(8611, 4, 100, 1, 0, 0, 0, 0, 0)
    w = lib.tgp_workspace_bytes_lik(8611, 4, 100, 1, 4, 8, 0, 0, 0, L.LIK_WARPED)
    assert w >= g + 3 * 8611 * 8 + lib.tgp_ell_warp_workspace_bytes(8611, 8) > g
    assert lib.tgp_ell_warp_f64(None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.tgp_flow_inverse_f64(None, None, 1, 1, None, None, None, None) == -1


def test_abi_refuses_per_row_programs_for_the_warp():
    """RP != 0 in the likelihood and training entries: TGP_E_UNSUPPORTED from the C entry itself, before anything touches the
    device (the pointers only have to be non-NULL to get past the argument checks)."""
    import ctypes as C
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    prog = (C.c_int32 * 4)(1, 0, 0, 4)             # one PER_ROW SAL block
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.nblk, md.P, md.RP, md.lik = 8, 2, 4, 1, 1, 0, 2, L.LIK_WARPED
    md.scale, md.kl_scale = 1.0, 1.0
    for f in ("Z", "raw_ls", "raw_os", "m", "Lam", "log_var_noise"):
        setattr(md, f, ptr)
    md.program = C.cast(prog, C.c_void_p)
    assert lib.tgp_ell_warp_f64(md, ptr, ptr, ptr, ptr, None, None, None, None, ptr, 1 << 20, None) == -100
    gs = L.TgpGrads()
    for f in ("Z", "raw_ls", "raw_os", "m", "Lam", "log_var_noise", "rowp"):
        setattr(gs, f, ptr)
    assert lib.tgp_elbo_step_f64(md, ptr, ptr, ptr, ptr, gs, None, None, ptr, ptr, 1 << 20, None) == -100
    ad = L.TgpAdamArgs()
    assert lib.tgp_elbo_step_adam_f64(md, ptr, ptr, ptr, ptr, gs, None, None, ptr, ptr, 1 << 20, ad, None) == -100
    md.RP, md.nblk, md.P = 0, 0, 3                 # parameters of no block
    assert lib.tgp_elbo_step_f64(md, ptr, ptr, None, ptr, gs, None, None, ptr, ptr, 1 << 20, None) == -1


def test_engines_refuse_what_is_out_of_scope():
    from tgp.pytorch_amd import engine
    with pytest.raises(NotImplementedError, match="minibatch"):
        engine.MinibatchEngine(None, None, {}, 1.0, 10, likelihood="warped")


def _main(*argv):
    return subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", *argv], cwd=REPO, capture_output=True, text=True)


def test_main_lists_wgp_and_refuses_classification():
    r = _main("--help")
    assert r.returncode == 0 and "WGP" in r.stdout
    r = _main("--model", "WGP", "--dataset", "synthetic_heart", "--train_test_seed_split", "1", "--num_inducing", "10",
              "--likelihood", "bernoulli")
    assert r.returncode == 2 and "WGP" in r.stderr
