"""Multi-class likelihood on the GPU: tgp_ell_softmax_f64 / tgp_predict_softmax_f64 / tgp_mc_normals_f64 and the C-output
model classes against the reference fixtures (tools/gen_golden_multiclass.py) and the torch restatement
(tests/softmax_model.py).  The project's bars: 1e-9 on values, 1e-7 on gradients, 1e-8 on the Adam history."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_model as sm          # noqa: E402

from conftest import load_golden, rel_err     # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F64 = torch.float64
CASES = ["mc_id3", "mc_sal2x4", "mc_mixed5", "mc_bigm3"]
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
# fixture -> the flow of each class (tools/gen_golden_multiclass.py main(); names of tools/gen_golden_warped.py FLOWS)
FLOWS = {"mc_id3": [None] * 3, "mc_sal2x4": ["sal2"] * 4, "mc_mixed5": ["tanh3x2", "arcsl2", "bcl_al1", "sal2", "sal_al1"],
         "mc_bigm3": ["sal2", None, "sal_al1"]}


def spec_of(g):
    from tgp.pytorch_amd import ops
    bo, to = [int(b) for b in g["blk_off"]], [int(t) for t in g["theta_off"]]
    prog = [tuple(r) for r in g["program"]]
    return ops.SoftmaxSpec([ops.FlowSpec(prog[bo[c]:bo[c + 1]], to[c + 1] - to[c], 0, None) for c in range(len(bo) - 1)])


def theta_dev(g):
    th = g["params"]["theta"]
    return th.to(DEV) if th.numel() else None


def programs_of(g):
    bo = [int(b) for b in g["blk_off"]]
    prog = [tuple(r) for r in g["program"]]
    return [prog[bo[c]:bo[c + 1]] for c in range(len(bo) - 1)]


def _flow_spec(name):
    from tgp.pytorch_amd import flows as F
    if name is None:
        return [("identity", [])]
    if name == "sal2":
        return F.SAL(2)
    if name == "arcsl2":
        return F.ArcSL(2)
    if name == "sal_al1":
        return F.build_chain("SAL_AL", 1)
    if name == "bcl_al1":
        return F.build_chain("BCL_AL", 1, constraint=None)
    np.random.seed(0)
    return F.StepTanhL(3, 2, add_f0=True)


def build_model(g, name, eps=None):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import MulticlassCategorical
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    cg.set_maximum_precission()
    p = g["params"]
    Cn, M, D = p["Z"].shape
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=Cn, kernel_is_shared=False)
    lik = MulticlassCategorical(Cn, eps=eps)
    lik.SMC = int(g["S"])
    args = (["zero", K], g["X"], p["Z"][0].clone(), float(g["N_total"]), lik, Cn, True, False, False, False, False)
    if all(f is None for f in FLOWS[name]):
        model = sparse_MF_GP(*args, 0.0)
    else:
        model = sparse_MF_SP(*args, [_flow_spec(f) for f in FLOWS[name]], "single", 0.0)
    with torch.no_grad():
        model.Z.data = p["Z"].clone()
        model.q_U.variational_mean.data = p["m"].clone()
        model.q_U.chol_variational_covar.data = p["Lam"].clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(Cn).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(Cn, 1, D).clone()
        to = [int(t) for t in g["theta_off"]]
        for c, fl in enumerate(model.G_matrix):
            prm = compile_flow(fl)[1]
            assert len(prm) == to[c + 1] - to[c]
            for q, val in zip(prm, p["theta"][to[c]:to[c + 1]]):
                q.data = val.clone().reshape(q.shape)
    return model.to(DEV)


def model_theta(model):
    from tgp.pytorch_amd.flow import compile_flow
    return [q for fl in model.G_matrix for q in compile_flow(fl)[1]]


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_reference(name):
    from tgp.pytorch_amd import ops
    g = load_golden(name)
    res = ops.ell_softmax(g["Y"].to(DEV), g["mu"].to(DEV), g["v"].to(DEV), spec_of(g), theta_dev(g), int(g["S"]),
                          eps=g["eps"].to(DEV))
    print(name, "ELL", rel_err(res["ell"].cpu(), g["lik_ELL"]), "g_mu", rel_err(res["g_mu"].cpu(), g["g_mu"]),
          "g_v", rel_err(res["g_v"].cpu(), g["g_v"]))
    assert rel_err(res["ell"].cpu(), g["lik_ELL"]) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), g["g_mu"]) < TOL_GRAD
    assert rel_err(res["g_v"].cpu(), g["g_v"]) < TOL_GRAD
    if g["lik_g_theta"].numel():
        print(name, "g_theta", rel_err(res["g_theta"].cpu(), g["lik_g_theta"]))
        assert rel_err(res["g_theta"].cpu(), g["lik_g_theta"]) < TOL_GRAD
    # forward only: the same value
    fwd = ops.ell_softmax(g["Y"].to(DEV), g["mu"].to(DEV), g["v"].to(DEV), spec_of(g), theta_dev(g), int(g["S"]),
                          eps=g["eps"].to(DEV), want_grads=False)
    assert torch.equal(fwd["ell"], res["ell"])
    P, lp = ops.predict_softmax(g["pred_mu"].to(DEV), g["pred_v"].to(DEV), spec_of(g), theta_dev(g), int(g["S"]),
                                eps=g["eps_te"].to(DEV), Y=g["Yte"].to(DEV))
    assert rel_err(P.cpu(), g["pred_P"]) < TOL_VAL
    assert rel_err(lp.sum().cpu(), g["pred_logp"]) < TOL_VAL


@pytest.mark.parametrize("name", CASES)
def test_model_elbo_and_gradients_match_reference(name):
    g = load_golden(name)
    model = build_model(g, name, eps=g["eps"].to(DEV))
    X, Y = g["X"].to(DEV), g["Y"].to(DEV)
    elbo, ell, kld = model.ELBO(X, Y)
    assert rel_err(elbo.detach().cpu(), g["ELBO"]) < TOL_VAL
    assert rel_err(ell.detach().cpu(), g["ELL"]) < TOL_VAL
    assert rel_err(kld.detach().cpu(), g["KLD"].sum()) < TOL_VAL
    elbo.backward()
    k = model.covariance_function
    got = {"g_Z": model.Z.grad, "g_m": model.q_U.variational_mean.grad, "g_Lam": model.q_U.chol_variational_covar.grad,
           "g_raw_outputscale": k.raw_outputscale.grad.reshape(-1),
           "g_raw_lengthscale": k.base_kernel.raw_lengthscale.grad.reshape(g["g_raw_lengthscale"].shape)}
    th = model_theta(model)
    if th:
        got["g_theta"] = torch.stack([q.grad.reshape(()) for q in th])
    for key, val in got.items():
        ref = g[key]
        if key == "g_Lam":     # the reference's gradient lives on the lower triangle
            val = torch.tril(val)
        print(name, key, rel_err(val.cpu(), ref))
        assert rel_err(val.cpu(), ref) < TOL_GRAD, key
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
        assert mu.shape == (g["mu"].shape[0], X.shape[0], 1) and model.KLD().shape == (g["mu"].shape[0],)
        assert rel_err(mu.squeeze(2).cpu(), g["mu"]) < TOL_VAL and rel_err(v.squeeze(2).cpu(), g["v"]) < TOL_VAL
        assert rel_err(model.KLD().cpu(), g["KLD"]) < TOL_VAL
    # evaluation path
    model.set_is_training(False)
    Xte, Yte = g["Xte"].to(DEV), g["Yte"].to(DEV)
    with torch.no_grad():
        pm, pv = model.marginal_variational_qf_parameters(Xte, diagonal=True, is_duvenaud=False)
        P, lp = model.likelihood.marginal_moments(pm.squeeze(2), pv.squeeze(2), flow=model.G_matrix,
                                                  X=Xte.repeat(P_classes(g), 1, 1), eps=g["eps_te"].to(DEV), Y=Yte.reshape(-1))
    assert rel_err(P.cpu(), g["pred_P"]) < TOL_VAL and rel_err(lp.sum().cpu(), g["pred_logp"]) < TOL_VAL
    m1, m2, _, _ = model.predictive_distribution(Xte)
    assert m2 is None and m1.shape == (Xte.shape[0], P_classes(g))
    assert float((m1.sum(1) - 1.0).abs().max()) < 1e-12
    model.set_is_training(False)
    logp, (probs,) = model.test_log_likelihood(Xte, Yte, return_moments=True, Y_std=torch.ones(1, device=DEV))
    assert logp.dtype == F64 and torch.isfinite(logp).all() and probs.shape == m1.shape


def P_classes(g):
    return int(g["mu"].shape[0])


@pytest.mark.parametrize("name", CASES)
def test_trainer_first_steps_match_reference(name):
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_classification
    g = load_golden(name)
    model = build_model(g, name, eps=g["adam_eps"].to(DEV))
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_classification(model, [loader, None, None], 1e20, False, False, torch.ones(P_classes(g), device=DEV), -1,
                                   100, True)
    tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    print(name, "history", rel_err(hist, g["history"]))
    assert rel_err(hist, g["history"]) < 1e-8
    assert rel_err(model.Z.detach().cpu(), g["final_Z"]) < 1e-8
    assert rel_err(model.q_U.variational_mean.detach().cpu(), g["final_m"]) < 1e-8
    th = model_theta(model)
    if th:
        assert rel_err(torch.stack([q.detach().reshape(()) for q in th]).cpu(), g["final_theta"]) < 1e-8


def _counter_case():
    g = load_golden("mc_sal2x4")
    return g, spec_of(g), theta_dev(g), g["Y"].to(DEV), g["mu"].to(DEV), g["v"].to(DEV), int(g["S"])


def test_counter_mode_equals_explicit_mode_bit_for_bit():
    from tgp.pytorch_amd import ops
    g, spec, theta, Y, mu, v, S = _counter_case()
    N = mu.shape[1]
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    kw = dict(seed=2024, step_dev=step, row0=1000)
    eps = ops.mc_normals(S, spec.C, N, device=DEV, **kw)
    a = ops.ell_softmax(Y, mu, v, spec, theta, S, **kw)
    b = ops.ell_softmax(Y, mu, v, spec, theta, S, eps=eps)
    for key in ("ell", "g_mu", "g_v", "g_theta"):
        assert torch.equal(a[key], b[key]), key
    Pa, la = ops.predict_softmax(mu, v, spec, theta, S, Y=Y, **kw)
    Pb, lb = ops.predict_softmax(mu, v, spec, theta, S, Y=Y, eps=eps)
    assert torch.equal(Pa, Pb) and torch.equal(la, lb)
    # the draws are the documented recipe
    ref = sm.mc_normals(S, spec.C, 24, seed=2024, step=3, row0=1000)
    err = float((eps[:, :, :24].cpu() - ref).abs().max())
    print("draws vs recipe", err)
    assert err < 1e-14
    # the next step draws afresh
    step += 1
    c = ops.ell_softmax(Y, mu, v, spec, theta, S, **kw)
    assert not torch.equal(c["ell"], a["ell"])
    assert not torch.equal(ops.mc_normals(S, spec.C, N, device=DEV, **kw), eps)


def test_consecutive_model_steps_use_different_draws():
    g = load_golden("mc_id3")
    model = build_model(g, "mc_id3")
    X, Y = g["X"].to(DEV), g["Y"].to(DEV)
    with torch.no_grad():
        e1, e2 = model.ELBO(X, Y)[1], model.ELBO(X, Y)[1]
    assert torch.isfinite(e1) and torch.isfinite(e2) and not torch.equal(e1, e2)


def test_row_shards_sum_to_the_whole():
    from tgp.pytorch_amd import ops
    g, spec, theta, Y, mu, v, S = _counter_case()
    N, k = mu.shape[1], 47
    kw = dict(seed=7, step_dev=torch.tensor([1], dtype=torch.int32, device=DEV))
    whole = ops.ell_softmax(Y, mu, v, spec, theta, S, row0=0, **kw)
    lo = ops.ell_softmax(Y[:k], mu[:, :k].contiguous(), v[:, :k].contiguous(), spec, theta, S, row0=0, **kw)
    hi = ops.ell_softmax(Y[k:], mu[:, k:].contiguous(), v[:, k:].contiguous(), spec, theta, S, row0=k, **kw)
    assert rel_err((lo["ell"] + hi["ell"]).cpu(), whole["ell"].cpu()) < 1e-11
    assert rel_err((lo["g_theta"] + hi["g_theta"]).cpu(), whole["g_theta"].cpu()) < 1e-11
    assert rel_err(torch.cat([lo["g_mu"], hi["g_mu"]], 1).cpu(), whole["g_mu"].cpu()) < 1e-11
    assert rel_err(torch.cat([lo["g_v"], hi["g_v"]], 1).cpu(), whole["g_v"].cpu()) < 1e-11


def test_run_to_run_and_edge_rows():
    from tgp.pytorch_amd import ops
    g, spec, theta, Y, mu, v, S = _counter_case()
    eps = g["eps"].to(DEV)
    a = ops.ell_softmax(Y, mu, v, spec, theta, S, eps=eps)
    b = ops.ell_softmax(Y, mu, v, spec, theta, S, eps=eps)
    for key in ("ell", "g_mu", "g_v", "g_theta"):
        assert torch.equal(a[key], b[key]), key
    # rows with v = 0 (and a negative one): finite outputs, no gradient with respect to v there
    v0 = v.clone()
    v0[:, ::3] = 0.0
    v0[1, 1] = -1e-3
    r = ops.ell_softmax(Y, mu, v0, spec, theta, S, eps=eps)
    assert all(torch.isfinite(r[key]).all() for key in ("ell", "g_mu", "g_v", "g_theta"))
    assert float(r["g_v"][:, ::3].abs().max()) == 0.0 and float(r["g_v"][1, 1]) == 0.0
    assert float(r["g_v"][:, 2::3].abs().max()) > 0.0
    th = g["params"]["theta"].clone().requires_grad_(True)
    ref = sm.ell_softmax_torch(g["Y"], g["mu"], v0.cpu().clamp_min(0.0), g["eps"], programs_of(g), th, g["theta_off"])
    assert rel_err(r["ell"].cpu(), ref.detach()) < TOL_VAL
    # logits of +-700 through identity flows: the max-subtracted value, exactly
    ident = ops.SoftmaxSpec([ops.FlowSpec([], 0, 0, None) for _ in range(3)])
    mu3 = torch.tensor([[700.0, -700.0, 0.0, 700.0], [-700.0, 700.0, 0.0, 700.0], [0.0, 0.0, 0.0, 700.0]], dtype=F64, device=DEV)
    y3 = torch.tensor([0.0, 0.0, 2.0, 1.0], dtype=F64, device=DEV)
    r3 = ops.ell_softmax(y3, mu3, torch.zeros_like(mu3), ident, None, 4, eps=torch.randn(4, 3, 4, dtype=F64, device=DEV))
    want = 0.0 + (-1400.0) + (-float(np.log(3.0))) + (-float(np.log(3.0)))
    assert torch.isfinite(r3["ell"]) and abs(float(r3["ell"]) - want) <= 1e-12 * abs(want)
    assert torch.isfinite(r3["g_mu"]).all() and float(r3["g_v"].abs().max()) == 0.0
    P3, lp3 = ops.predict_softmax(mu3, torch.zeros_like(mu3), ident, None, 4, seed=1, Y=y3)
    assert torch.isfinite(P3).all() and float(P3[0, 0]) == 1.0 and float(P3[1, 0]) == 0.0
    # (row 3: logsumexp = 700 + log 3 is rounded at ulp(701) = 1.1e-13, so log P carries that much)
    assert abs(float(lp3[2]) + float(np.log(3.0))) < 1e-15 and abs(float(lp3[3]) + float(np.log(3.0))) < 2.3e-13


def _desc(Cn, S, N, blk_off, theta_off, program=None):
    from tgp.pytorch_amd import lib as L
    d = L.TgpSoftmax()
    d.N, d.C, d.S, d.scale = N, Cn, S, 1.0
    keep = [np.ascontiguousarray(blk_off, dtype=np.int32), np.ascontiguousarray(theta_off, dtype=np.int32)]
    d.blk_off, d.theta_off = C.c_void_p(keep[0].ctypes.data), C.c_void_p(keep[1].ctypes.data)
    if program is not None:
        keep.append(np.ascontiguousarray(program, dtype=np.int32))
        d.program = C.c_void_p(keep[2].ctypes.data)
    return d, keep


def test_limits_are_return_values():
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    N = 8
    buf = torch.zeros(4096, dtype=F64, device=DEV)
    ws = torch.zeros(256, dtype=F64, device=DEV)

    def call(d):
        return lib.tgp_ell_softmax_f64(d, L.ptr(buf), L.ptr(buf), L.ptr(buf), None, L.ptr(buf), None, None, None, L.ptr(ws),
                                       ws.numel() * 8, L.stream_ptr())
    for Cn, S in ((2, 4), (33, 4), (3, 0), (3, 257)):
        d, keep = _desc(Cn, S, N, [0] * (Cn + 1), [0] * (Cn + 1))
        assert call(d) == L.E_UNSUPPORTED, (Cn, S)
        assert lib.tgp_mc_normals_f64(d, L.ptr(buf), L.stream_ptr()) == L.E_UNSUPPORTED
        assert lib.tgp_predict_softmax_f64(d, L.ptr(buf), L.ptr(buf), None, None, L.ptr(buf), None, L.stream_ptr()) == L.E_UNSUPPORTED
    # 65 blocks over the three programs
    prog = [(0, 0, 0, 0)] * 65
    d, keep = _desc(3, 4, N, [0, 30, 60, 65], [0, 2, 4, 6], prog)
    d.theta = L.ptr(buf)
    assert call(d) == L.E_UNSUPPORTED
    # a per-row block (RP != 0)
    d, keep = _desc(3, 4, N, [0, 1, 1, 1], [0, 2, 2, 2], [(1, 0, 0, L.FLAG_PER_ROW)])
    d.theta = L.ptr(buf)
    assert call(d) == L.E_UNSUPPORTED
    # and the smallest accepted call still runs
    d, keep = _desc(3, 1, N, [0, 0, 0, 0], [0, 0, 0, 0])
    assert call(d) == 0
    torch.cuda.synchronize()


def test_training_step_entry_refuses_the_softmax_likelihood():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.synthetic import synthetic_problem
    pr = synthetic_problem(64, 3, 8, flow=None)
    p = {k: t.to(DEV) for k, t in pr["params"].items()}
    with pytest.raises(L.TgpError, match="-100.*tgp_ell_softmax_f64"):
        ops.elbo_step(pr["X"].to(DEV), pr["Y"].to(DEV), p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"],
                      p["log_var_noise"], 64.0, flow=ops.FlowSpec([], 0, 0, None), S=4, lik=L.LIK_SOFTMAX)


# The bar of the CLI run: what the CPU restatement trained on the same split reaches, minus 0.05.
# softmax_model.train_blobs_cpu(split_seed=1, M=20, epochs=300) -- the CPU oracle's q(f) moments and KL per class, SAL x 2
# flows, the restated likelihood, Adam lr 0.01 -- ends at test NLL 0.108 per row and test accuracy 0.975 (majority-class
# share of that split: 0.275), so the run must reach 0.925.
BLOBS_CPU_ACCURACY = 0.975


def test_cli_multiclass_run_beats_the_majority_class():
    from tgp.pytorch_amd.data import return_dataset
    _, dc = return_dataset("synthetic_blobs", 10000, seed=1)
    yte = dc["Y_te"].reshape(-1).long()
    majority = float(torch.bincount(yte).max()) / yte.numel()
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--likelihood", "multiclass", "--dataset",
           "synthetic_blobs", "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "300"]
    r = subprocess.run(["timeout", "-k", "10", "600"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    nll = float(r.stdout.split("Test Negative LOGL")[1].split()[0])
    acc = float(r.stdout.split("Test Accuracy")[1].split()[0])
    print("blobs: NLL", nll, "accuracy", acc, "majority", majority)
    assert np.isfinite(nll)
    assert acc > majority and acc >= BLOBS_CPU_ACCURACY - 0.05
