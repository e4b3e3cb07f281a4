"""CPU: the sinh / normal-CDF / Tukey / exp / softplus flow kinds above the kernels -- the ABI's constants and refusals (nothing
is launched: test_api_refusals' call()), the flow classes against the restated formulas (flow_shapes_model), compile_flow's rows
and theta order, the generators, the host refusals, and the patched oracle against the reference's fixtures
(tools/gen_golden_flow_shapes.py), which ties the tests' own model to the reference."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err

import flow_shapes_model as fm
import test_api_refusals as tar
import test_flow_kinds_host as tfk

from tgp.pytorch_amd import flow as F
from tgp.pytorch_amd import flows as G
from tgp.pytorch_amd import lib as L

SHAPES = ["shapes_tiny_sinh2", "shapes_tiny_ncdf1", "shapes_tiny_tukeyr1", "shapes_tiny_tukeyl1", "shapes_tiny_salexp1",
          "shapes_med_sinh2", "shapes_med_tukeyr1", "shapes_bigm_sinh1"]
NEW_KINDS = (L.FLOW_SINH, L.FLOW_NORMCDF, L.FLOW_TUKEY, L.FLOW_EXP, L.FLOW_SOFTPLUS)
R, A, PR, NG = L.FLAG_RESTRICT, L.FLAG_ADD_F0, L.FLAG_PER_ROW, L.FLAG_NEGATE


def test_constants_mirror_the_header():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    for name, val in (("SINH", 7), ("NORMCDF", 8), ("TUKEY", 9), ("EXP", 10), ("SOFTPLUS", 11)):
        assert getattr(L, "FLOW_" + name) == val
        assert re.search(r"#define TGP_FLOW_%s %d\b" % (name, val), hdr)
    assert L.FLAG_NEGATE == 8 and re.search(r"#define TGP_FLAG_NEGATE 8\b", hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)
    assert not re.search(r"#define TGP_FLOW_\w+ 6\b", hdr)          # kind 6 stays unassigned
    assert (fm.SINH, fm.NORMCDF, fm.TUKEY, fm.EXP, fm.SOFTPLUS, fm.NEGATE) == NEW_KINDS + (L.FLAG_NEGATE,)


# (entry, program, P, code): every row is refused before any device is touched
REFUSALS = [("tgp_flow_eval_f64", [(6, 0, 0, 0)], 4, -1)]
REFUSALS += [("tgp_flow_eval_f64", [(k, 0, 0, PR)], 4, -1) for k in NEW_KINDS]
REFUSALS += [("tgp_ell_flow_f64", [(k, 0, 0, PR | R)], 4, -1) for k in NEW_KINDS]
REFUSALS += [("tgp_flow_eval_f64", [(k, 0, 0, A)], 4, -1) for k in (L.FLOW_TUKEY, L.FLOW_EXP, L.FLOW_SOFTPLUS)]
REFUSALS += [("tgp_flow_eval_f64", [(k, 0, 0, R | NG)], 4, -1)
             for k in (L.FLOW_AFFINE, L.FLOW_SAL, L.FLOW_ARCSINH, L.FLOW_BOXCOX, L.FLOW_SINH, L.FLOW_NORMCDF, L.FLOW_EXP, L.FLOW_SOFTPLUS)]
REFUSALS += [("tgp_flow_eval_f64", [(L.FLOW_TUKEY, 0, 0, NG)], 4, -1),                # NEGATE without RESTRICT
             ("tgp_flow_eval_f64", [(L.FLOW_SINH, 0, 1, 0)], 4, -1),                  # four parameters from offset 1 of 4
             ("tgp_flow_eval_f64", [(L.FLOW_TUKEY, 0, 3, R)], 4, -1),                 # two from offset 3 of 4
             ("tgp_flow_eval_f64", [(L.FLOW_EXP, 0, 5, 0)], 4, -1),                   # an offset past theta, even with no parameter
             ("tgp_ell_warp_f64", [(L.FLOW_NORMCDF, 0, 0, R)], 4, L.E_UNSUPPORTED),   # not onto the real line
             ("tgp_ell_warp_f64", [(L.FLOW_AFFINE, 0, 0, 0), (L.FLOW_EXP, 0, 2, 0)], 2, L.E_UNSUPPORTED),
             ("tgp_flow_inverse_f64", [(L.FLOW_SOFTPLUS, 0, 0, 0)], 0, L.E_UNSUPPORTED),
             ("tgp_predict_f64", [(L.FLOW_NORMCDF, 0, 0, 0)], 4, L.E_UNSUPPORTED)]


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=lambda i: "%s-%s" % (REFUSALS[i][0][4:-4], REFUSALS[i][1][-1]))
def test_abi_refusal(i):
    entry, prog, P, code = REFUSALS[i]
    assert tar.call(L.load(), entry, dict(program=prog, P=P)) == code


def test_warp_refusal_names_the_entry_and_the_kind():
    lib = L.load()
    assert tar.call(lib, "tgp_ell_warp_f64", dict(program=[(L.FLOW_NORMCDF, 0, 0, 0)], P=4)) == L.E_UNSUPPORTED
    msg = lib.tgp_last_error().decode()
    assert "tgp_ell_warp_f64" in msg and "TGP_FLOW_NORMCDF" in msg


def test_accepted_flag_combinations_pass_the_program_check():
    # The softmax entry checks its classes' blocks in order and launches nothing here: class 0 holds the program under test,
    # class 2 a per-row block, which that entry refuses with TGP_E_UNSUPPORTED -- reached only when class 0 was accepted
    # (a refused block of class 0 gives -1, as the last assertion shows).
    lib = L.load()

    def code(prog, P):
        n = len(prog)
        return tar.call(lib, "tgp_predict_softmax_f64",
                        dict(program=list(prog) + [(L.FLOW_AFFINE, 0, 0, 0), (L.FLOW_AFFINE, 0, 0, PR)],
                             blk_off=[0, n, n + 1, n + 2], theta_off=[0, P, P + 2, P + 4]))
    for name, prog in fm.PROGRAMS.items():
        assert code(prog, fm.P_OF[name]) == L.E_UNSUPPORTED, name
    assert code([(L.FLOW_TUKEY, 0, 0, NG)], 2) == -1


# ---- the host classes against the restated formulas ----
def _points(n=2000, seed=3, clamp=None):
    g = torch.Generator().manual_seed(seed)
    f = 2.0 * torch.randn(n, generator=g, dtype=torch.float64)
    return f if clamp is None else f.clamp(-clamp, clamp)


CLASS_CASES = {
    "sinh": (lambda: F.SinhFlow(0.3, 1.2, -0.4, 1.8, False, False), [(7, 0, 0, 0)], 4.0),
    "sinh_rf0": (lambda: F.SinhFlow(-0.2, 0.4, 0.3, 1.1, True, False), [(7, 0, 0, R | A)], 4.0),
    "ncdf_r": (lambda: F.NormalCDFFlow(0.1, 1.5, -0.3, 0.4, False, True, is_learnable=True), [(8, 0, 0, R)], None),
    "tukey": (lambda: F.TukeyFlow(0.35, -2.5, False), [(9, 0, 0, 0)], 4.0),
    "tukey_right": (lambda: F.TukeyRightFlow(-1.2, -3.0, False), [(9, 0, 0, R)], 4.0),
    "tukey_left": (lambda: F.TukeyLeftFlow(-2.2, -2.0, False), [(9, 0, 0, R | NG)], 4.0),
    "exp": (lambda: F.ExpFlow(), [(10, 0, 0, 0)], None),
    "softplus": (lambda: F.SoftplusFlow(), [(11, 0, 0, 0)], None),
}


@pytest.mark.parametrize("name", list(CLASS_CASES))
def test_flow_classes_equal_the_restated_formulas(name):
    torch.set_default_dtype(torch.float64)
    make, prog, clamp = CLASS_CASES[name]
    fl = make()
    spec, theta_list, nets = F.compile_flow(F.CompositeFlow([fl]))
    assert nets == [] and [tuple(b) for b in spec.blocks] == prog
    theta = torch.stack([p.detach().reshape(()) for p in theta_list]) if theta_list else torch.zeros(0, dtype=torch.float64)
    f = _points(clamp=clamp)
    if name == "softplus":
        f = torch.cat((f, torch.tensor([19.9, 20.0, 20.1, 35.0, -40.0], dtype=torch.float64)))      # both sides of torch's threshold
    fa, fb = f.clone().requires_grad_(True), f.clone().requires_grad_(True)
    ga, gb = fl.torch_map(fa), fm.flow(fb, prog, theta)
    assert rel_err(ga.detach(), gb.detach()) < 1e-14
    da, = torch.autograd.grad(ga.sum(), fa)
    db, = torch.autograd.grad(gb.sum(), fb)
    assert torch.isfinite(db).all() and (db > 0).all() and rel_err(da, db) < 1e-14


def test_restated_derivatives_equal_the_header_formulas():
    """The closed forms the kernels implement (include/tgp_hip.h), against autograd of the restated maps."""
    f = _points(clamp=4.0).requires_grad_(True)
    th = torch.tensor(fm.THETA["tukey_left"], dtype=torch.float64)
    g = fm.flow(f, fm.PROGRAMS["tukey_left"], th)
    dg, = torch.autograd.grad(g.sum(), f)
    gam, h = -torch.nn.functional.softplus(th[0]), torch.nn.functional.softplus(th[1])
    fd = f.detach()
    E, eg, u = torch.exp(h * fd ** 2 / 2), torch.exp(gam * fd), torch.expm1(gam * fd) / gam
    assert rel_err(E * (eg + h * fd * u), dg) < 1e-13
    th = torch.tensor(fm.THETA["ncdf"], dtype=torch.float64)
    f2 = _points().requires_grad_(True)
    dg, = torch.autograd.grad(fm.flow(f2, fm.PROGRAMS["ncdf"], th).sum(), f2)
    x = (f2.detach() - th[2]) / th[3]
    assert rel_err(th[1] / th[3] * torch.exp(-x ** 2 / 2) / math.sqrt(2 * math.pi), dg) < 1e-13


def test_compile_flow_of_a_mixed_chain():
    specs = (G.SAL(1) + G.SinhL(1, add_f0=True) + G.TukeyL(1, side="left") + G.NormalCDFL(1, set_res=True) + G.TukeyL(1)
             + G.SALSoftplus(1) + [("exp", {})])
    comp = F.instance_flow(specs)
    spec, theta, nets = F.compile_flow(comp)
    AFF = L.FLOW_AFFINE
    assert nets == []
    assert spec.blocks == [(L.FLOW_SAL, 0, 0, 0), (AFF, 0, 2, 0), (L.FLOW_SINH, 0, 4, R | A), (AFF, 0, 8, 0),
                           (L.FLOW_TUKEY, 0, 10, R | NG), (AFF, 0, 12, 0), (L.FLOW_NORMCDF, 0, 14, R), (AFF, 0, 18, R),
                           (L.FLOW_TUKEY, 0, 20, 0), (AFF, 0, 22, 0), (L.FLOW_SAL, 0, 24, 0), (AFF, 0, 26, 0),
                           (L.FLOW_SOFTPLUS, 0, 28, 0), (L.FLOW_EXP, 0, 28, 0)]
    fl = comp.flow_arr
    expect = [fl[0].a, fl[0].b, fl[1].a, fl[1].b, fl[2].a, fl[2].b, fl[2].c, fl[2].d, fl[3].a, fl[3].b, fl[4].g, fl[4].h,
              fl[5].a, fl[5].b, fl[6].a, fl[6].b, fl[6].c, fl[6].d, fl[7].a, fl[7].b, fl[8].g, fl[8].h, fl[9].a, fl[9].b,
              fl[10].a, fl[10].b, fl[11].a, fl[11].b]
    assert len(theta) == len(expect) == spec.P == 28
    assert all(t is e for t, e in zip(theta, expect))


def test_instance_flow_names():
    four = dict(init_a=0.1, init_b=0.2, init_c=0.3, init_d=0.4, add_init_f0=False, set_restrictions=False)
    gh = dict(init_g=0.2, init_h=-1.0, add_init_f0=False)
    comp = F.instance_flow([("sinh", four), ("normalCDF", dict(four, is_learnable=True)), ("tukey", gh), ("tukey_left", gh),
                            ("tukey_right", gh), ("exp", {}), ("softplus", {})])
    assert [type(f).__name__ for f in comp.flow_arr] == ["SinhFlow", "NormalCDFFlow", "TukeyFlow", "TukeyLeftFlow",
                                                        "TukeyRightFlow", "ExpFlow", "SoftplusFlow"]
    names = [n for n, _ in comp.named_parameters()]
    assert names == ["flow_arr.%d.%s" % (i, p) for i in (0, 1) for p in "abcd"] + \
                    ["flow_arr.%d.%s" % (i, p) for i in (2, 3, 4) for p in "gh"]
    assert F.SinhFlow(0.0, 1.0, 0.0, 1.0, add_init_f0=True, set_restrictions=False).set_restrictions is True
    assert F.NormalCDFFlow(0.0, 1.0, 0.0, 1.0, True, False, True).set_restrictions is True
    with pytest.raises(ValueError, match="Unkown flow identifier"):
        F.instance_flow([("log", {})])


def test_generators_under_a_fixed_seed():
    sp_inv = lambda v: math.log(math.expm1(v))      # noqa: E731
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    s = G.SinhL(2)
    assert [n for n, _ in s] == ["sinh", "affine"] * 2
    assert all(b[1] == dict(init_a=0.0, init_b=3.0, init_c=0.0, init_d=3.0, add_init_f0=False, set_restrictions=False)
               for b in s[::2])
    assert all(b[1] == dict(init_a=1.0, init_b=0.0, set_restrictions=False) for b in s[1::2])
    n = G.NormalCDFL(1)[0][1]
    b = 3.0 * math.sqrt(2.0 * math.pi)
    assert (n["init_a"], n["init_b"], n["init_c"], n["init_d"], n["is_learnable"]) == (-0.5 * b, b, 0.0, 3.0, True)
    r = G.SinhL(1, set_res=True)[0][1]           # restricted: the raw values whose softplus is 3
    assert abs(r["init_b"] - sp_inv(3.0)) < 1e-12 and abs(r["init_d"] - sp_inv(3.0)) < 1e-12 and r["set_restrictions"]
    for side, name, graw in ((None, "tukey", 0.1), ("right", "tukey_right", sp_inv(0.1)), ("left", "tukey_left", sp_inv(0.1))):
        t = G.TukeyL(1, side=side)
        assert [k for k, _ in t] == [name, "affine"]
        assert abs(t[0][1]["init_g"] - graw) < 1e-12 and abs(t[0][1]["init_h"] - sp_inv(0.01)) < 1e-12
    assert [k for k, _ in G.SALSoftplus(2)] == ["sinh_arcsinh", "affine"] * 2 + ["softplus"]
    assert [k for k, _ in G.SALExp(1)] == ["sinh_arcsinh", "affine", "exp"]
    assert (np.random.get_state()[1] == before).all()          # the defaults draw nothing
    # init_random: per block randn(2) for the affine block, then the block's own parameters
    np.random.seed(5)
    s = G.SinhL(2, init_random=True)
    np.random.seed(5)
    for k in range(2):
        aff, own = np.random.randn(2), np.random.randn(4)
        assert [s[2 * k][1]["init_" + c] for c in "abcd"] == list(own)
        assert [s[2 * k + 1][1]["init_a"], s[2 * k + 1][1]["init_b"]] == list(aff)
    np.random.seed(6)
    t = G.TukeyL(1, side="left", init_random=True)
    np.random.seed(6)
    aff, own = np.random.randn(2), np.random.randn(2)
    assert [t[0][1]["init_g"], t[0][1]["init_h"]] == list(own) and [t[1][1]["init_a"], t[1][1]["init_b"]] == list(aff)
    with pytest.raises(ValueError):
        G.TukeyL(1, side="up")


def test_default_generators_are_near_the_identity():
    torch.set_default_dtype(torch.float64)
    f = torch.linspace(-1.0, 1.0, 41, dtype=torch.float64)
    for specs, tol in ((G.SinhL(2), 0.05), (G.NormalCDFL(1), 0.03), (G.TukeyL(1), 0.07), (G.TukeyL(1, side="left"), 0.07)):
        spec, theta, _ = F.compile_flow(F.instance_flow(specs))
        th = torch.stack([p.detach().reshape(()) for p in theta])
        assert float((fm.flow(f, [tuple(b) for b in spec.blocks], th) - f).abs().max()) < tol


def test_host_refusals():
    four = (0.0, 1.0, 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="is_learnable"):
        F.NormalCDFFlow(*four, add_init_f0=False, set_restrictions=False, is_learnable=False)
    for cls in (F.TukeyFlow, F.TukeyLeftFlow, F.TukeyRightFlow):
        with pytest.raises(ValueError, match="add_init_f0"):
            cls(0.1, -2.0, add_init_f0=True)
    with pytest.raises(ValueError, match="add_f0"):
        G.TukeyL(1, add_f0=True)
    with pytest.raises(NotImplementedError, match="input-dependent"):
        F.compile_flow(F.CompositeFlow([F.SinhFlow(*four, False, False, input_dependent=True)]))
    with pytest.raises(NotImplementedError, match="input-dependent"):
        F.compile_flow(F.CompositeFlow([F.TukeyRightFlow(0.1, -2.0, False, input_dependent=True)]))
    from tgp.pytorch_amd.likelihoods import WarpedGaussianLinearMean
    for specs in (G.NormalCDFL(1), G.SALExp(1), G.SALSoftplus(1)):
        with pytest.raises(ValueError, match="onto the real line"):
            WarpedGaussianLinearMean(1, 0.05, False, flow=specs, quad_points=8)
    WarpedGaussianLinearMean(1, 0.05, False, flow=G.SinhL(1) + G.TukeyL(1, side="right"), quad_points=8)      # these are onto


def test_chains_and_cli_choices():
    from tgp.pytorch_amd import main as M
    assert G.CHAINS == ("SAL_BCL", "SAL_InvBCL", "SAL_AL", "BCL_AL", "InvBCL_AL")
    assert set(("SinhL", "NormalCDFL", "TukeyL", "TukeyLeftL", "TukeyRightL", "SALSoftplus", "SALExp")) <= set(M.FLOW_ARCHS)
    assert [k for k, _ in M._PLAIN_GENERATORS["TukeyLeftL"](1)] == ["tukey_left", "affine"]


# ---- the tests' own model against the reference ----
@pytest.mark.parametrize("name", SHAPES)
def test_patched_oracle_reproduces_the_reference_fixture(name):
    """ELBO, ELL, KLD to 1e-12, every gradient to 1e-10.  Measured (CPU float64): values <= 9e-15 and gradients <= 2.1e-12 on every
    fixture.  The general-M fixture (M = 136) is written at length-scale 0.75, cond(K_ZZ) = 2e4: at the recipe's length-scale 2
    (cond 2e9) float64 itself does not carry g_Z to 1e-10 -- tools/gen_golden_flow_shapes.py bigm_problem has the figures."""
    from oracle import tgp_oracle as orc
    g = load_golden(name)
    assert any(b[0] in NEW_KINDS for b in g["program"])
    with pytest.raises(ValueError):
        orc.flow_forward(torch.zeros(3, dtype=torch.float64), g["program"], g["params"]["theta"])      # the oracle alone has no such kind
    with fm.patched():
        (elbo, ell, kld), og = orc.elbo_and_grads(g["X"], g["Y"], g["params"], float(g["N_total"]), g["program"], g["xs"], g["ws"])
    assert orc.flow_forward is fm._ORIG
    pairs = (("Z", "g_Z"), ("raw_lengthscale", "g_raw_lengthscale"), ("raw_outputscale", "g_raw_outputscale"), ("m", "g_m"),
             ("Lam", "g_Lam"), ("log_var_noise", "g_log_var_noise"), ("theta", "g_theta"))
    print(name, "ELBO %.1e ELL %.1e KLD %.1e" % (rel_err(elbo, g["ELBO"]), rel_err(ell, g["ELL"]), rel_err(kld, g["KLD"])),
          " ".join("%s %.1e" % (gk, rel_err(og[k], g[gk])) for k, gk in pairs))
    assert rel_err(elbo, g["ELBO"]) < 1e-12 and rel_err(ell, g["ELL"]) < 1e-12 and rel_err(kld, g["KLD"]) < 1e-12
    for k, gk in (("Z", "g_Z"), ("raw_lengthscale", "g_raw_lengthscale"), ("raw_outputscale", "g_raw_outputscale"), ("m", "g_m"),
                  ("Lam", "g_Lam"), ("log_var_noise", "g_log_var_noise"), ("theta", "g_theta")):
        assert rel_err(og[k], g[gk]) < 1e-10, (k, rel_err(og[k], g[gk]))


def test_generator_specs_compile_to_the_fixture_programs():
    """This package's generators and compile_flow give the rows the fixtures were written with."""
    for name, specs in (("shapes_tiny_sinh2", G.SinhL(2)), ("shapes_tiny_ncdf1", G.NormalCDFL(1)),
                        ("shapes_tiny_tukeyr1", G.TukeyL(1, side="right")), ("shapes_tiny_tukeyl1", G.TukeyL(1, side="left")),
                        ("shapes_tiny_salexp1", G.SALExp(1)), ("shapes_bigm_sinh1", G.SinhL(1, set_res=True))):
        spec = F.compile_flow(F.instance_flow(specs))[0]
        assert [tuple(b) for b in spec.blocks] == load_golden(name)["program"], name


# ---- the build keeps every kernel the earlier kinds had ----
@pytest.mark.parametrize("mt", range(1, 9))
def test_every_earlier_row_kernel_symbol_is_still_there(mt):
    tfk.test_row_kernel_instantiations(mt)
    ext2 = tfk._symbols("tgp_rowsx2_mt%d.o" % mt)
    if os.path.exists(os.path.join(tfk.BUILD, "tgp_rowsx2_mt%d_dp16.o" % mt)):
        ext2 |= tfk._symbols("tgp_rowsx2_mt%d_dp16.o" % mt)
    X2 = 128        # TGP_FLOWX2 (tgp_dev.hpp)
    for dp in (4, 8, 16):
        for sym in [tfk._k_rows(mt, dp, m | X2, 16) for m in (1, 2)] + [tfk._k_rows(mt, dp, 1 | X2, 10)] + \
                   [tfk._k_rows4(mt, dp, True, nw | X2) for nw in (4, 8)]:
            assert sym in ext2, sym


def test_every_earlier_ell_kernel_symbol_is_still_there():
    tfk.test_ell_flow_instantiations()
    syms = tfk._symbols("tgp_lik.o")
    for lpr, nbs in ((4, (8, 4, 2, 1)), (16, (4, 2, 1)), (32, (4, 2, 1))):
        for nb in nbs:
            assert any(s.startswith("_ZN3tgp10k_ell_quadINS_8EllGaussELi%dELi%dEEE" % (lpr, nb | 128)) for s in syms), (lpr, nb)
