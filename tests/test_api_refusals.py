"""CPU: what the C entry points refuse, and with which code -- one literal table, recorded from the library BEFORE the host
layer's checks were folded into shared helpers (check_flow_args, check_block, check_adam, fused_plan, gauss_copy in
tgp_api.hip) and required of every build since.  Nothing is launched: every row ends in a refusal, and the pointers only have
to be non-NULL to get past the checks in front of it (nothing is dereferenced before a refusal but the HOST arrays: the flow
program, blk_off and theta_off).

A row is (entry, overrides, code).  `overrides` change the entry's base call (ENTRIES): a key that names a tgp_model /
tgp_softmax / tgp_adam_args / tgp_grads / tgp_mlp field changes that struct, "model": None passes a NULL struct, "program" takes
a list of (kind, K, poff, flags) blocks (nblk follows unless given), every other key is an argument of the entry.  Where
the check under test is one the entry does NOT make (a negative count it lets through), the row carries a later violation
as well, so that the code shows the call got that far."""
import ctypes as C

import pytest

from tgp.pytorch_amd import lib as L

PTR = C.c_void_p(8)             # non-NULL, never dereferenced
UNSUP, WSP = L.E_UNSUPPORTED, L.E_WORKSPACE
AFF, SAL, TANH, PER_ROW = L.FLOW_AFFINE, L.FLOW_SAL, L.FLOW_STEPTANH, L.FLAG_PER_ROW
BIG = 1 << 30
ADAM_BASE, F64 = 0x100000, 8    # the flat gradient buffer of the Adam rows: an address range, never read
GP = ("Z", "raw_ls", "raw_os", "m", "Lam", "log_var_noise")


# entry -> (base model fields, ordered (argument, base value) after the model)
FLOW_MODEL = dict(N=64, D=2, M=16, S=4, lik=L.LIK_FLOW, nblk=1, P=2, RP=0, program=[(AFF, 0, 0, 0)])
STEP_ARGS = [("X", PTR), ("Y", PTR), ("rowp", None), ("out", PTR), ("grads", "grads"), ("mu", None), ("v", None),
             ("status", PTR), ("workspace", PTR), ("workspace_bytes", 0)]
ENTRIES = {
    "tgp_ell_flow_f64": (FLOW_MODEL, [("Y", PTR), ("mu", PTR), ("v", PTR), ("rowp", None), ("out", PTR), ("g_mu", None),
                                      ("g_v", None), ("g_theta", None), ("g_rowp", None), ("workspace", PTR),
                                      ("workspace_bytes", BIG), ("stream", None)]),
    "tgp_flow_eval_f64": (FLOW_MODEL, [("f", PTR), ("S_", 1), ("N_", 64), ("rowp", None), ("G", PTR), ("dG", None),
                                       ("logdG", None), ("stream", None)]),
    "tgp_flow_logdet_f64": (FLOW_MODEL, [("f", PTR), ("S_", 1), ("N_", 64), ("rowp", None), ("G", None), ("out", PTR),
                                         ("workspace", PTR), ("workspace_bytes", BIG), ("stream", None)]),
    "tgp_ell_warp_f64": (dict(FLOW_MODEL, lik=L.LIK_WARPED, S=1),
                         [("Y", PTR), ("mu", PTR), ("v", PTR), ("out", PTR), ("g_mu", None), ("g_v", None), ("g_theta", None),
                          ("t_out", None), ("workspace", PTR), ("workspace_bytes", BIG), ("stream", None)]),
    "tgp_flow_inverse_f64": (FLOW_MODEL, [("t", PTR), ("S_", 1), ("N_", 64), ("rowp", None), ("x", PTR), ("status", PTR),
                                          ("stream", None)]),
    "tgp_predict_f64": (dict(FLOW_MODEL, lik=L.LIK_WARPED),
                        [("mu", PTR), ("v", PTR), ("rowp", None), ("Y", None), ("Y_std", 1.0), ("m1", PTR), ("m2", PTR),
                         ("logp", None), ("stream", None)]),
    "tgp_predict_quantile_f64": (FLOW_MODEL, [("mu", PTR), ("v", PTR), ("rowp", None), ("probs", PTR), ("zq", PTR), ("Q", 1),
                                              ("t", PTR), ("status", PTR), ("stream", None)]),
    "tgp_predict_cdf_f64": (FLOW_MODEL, [("mu", PTR), ("v", PTR), ("rowp", None), ("Y", PTR), ("cdf", PTR), ("sf", None),
                                         ("stream", None)]),
    # the training step: Gaussian unless a row says otherwise; workspace_bytes 0 is the refusal behind every other check
    "tgp_elbo_step_f64": (dict(FLOW_MODEL, lik=L.LIK_GAUSS, S=1, nblk=0, P=0, program=None), STEP_ARGS + [("stream", None)]),
    "tgp_elbo_step_adam_f64": (dict(FLOW_MODEL, lik=L.LIK_GAUSS, S=1, nblk=0, P=0, program=None),
                               STEP_ARGS + [("adam", "adam"), ("stream", None)]),
    "tgp_qf_moments_f64": (dict(FLOW_MODEL, lik=L.LIK_GAUSS, S=1, nblk=0, P=0, program=None),
                           [("X", PTR), ("mu", PTR), ("v", PTR), ("status", PTR), ("workspace", PTR), ("workspace_bytes", 0),
                            ("stream", None)]),
    "tgp_qf_moments_bwd_f64": (dict(FLOW_MODEL, lik=L.LIK_GAUSS, S=1, nblk=0, P=0, program=None),
                               [("X", PTR), ("mu_bar", PTR), ("v_bar", PTR), ("grads", "grads"), ("status", PTR),
                                ("workspace", PTR), ("workspace_bytes", 0), ("stream", None)]),
    "tgp_predict_softmax_f64": (None, [("mu", None), ("v", PTR), ("eps", None), ("Y", None), ("P_", PTR), ("logp", None),
                                       ("stream", None)]),
    "tgp_mlp_backward_adam_f64": (None, [("X", PTR), ("W", C.c_void_p(ADAM_BASE)), ("step_dev", PTR), ("g_out", PTR),
                                         ("g_W", C.c_void_p(ADAM_BASE + 0x10000)), ("workspace", PTR), ("workspace_bytes", BIG),
                                         ("adam", "adam"), ("weight_decay", 0.0), ("stream", None)]),
}
FLOW8 = ("tgp_ell_flow_f64", "tgp_flow_eval_f64", "tgp_flow_logdet_f64", "tgp_ell_warp_f64", "tgp_flow_inverse_f64",
         "tgp_predict_f64", "tgp_predict_quantile_f64", "tgp_predict_cdf_f64")
ROWP = dict(RP=1, rowp=None)            # the later violation of a row whose own is let through: per-row parameters, no rowp
NBLK65 = dict(nblk=65)                  # ... or, where rowp cannot serve: more blocks than TGP_MAX_BLOCKS (make_prog)
TANH_PER_ROW = [(TANH, 1, 0, PER_ROW)]
# the three classes of the softmax rows: one AFFINE block and two parameters each unless a row changes them
SMX = dict(N=64, C=3, S=4, program=[(AFF, 0, 0, 0)] * 3, blk_off=[0, 1, 2, 3], theta_off=[0, 2, 4, 6])
# the gradients of a Gaussian step at M = 16, D = 2 as views of one flat buffer of 308 doubles (offsets in doubles)
ADAM_OFF = dict(Z=0, raw_ls=32, raw_os=34, m=35, Lam=51, log_var_noise=307)
MLP = dict(N=64, D=2, H=4, L=1, nnets=2)          # 2 nets of 2 -> 4 -> 1: 17 weights each

ROWS = [
    # ---- the flow-argument checks of the eight entries that take a flow (and of the warped step, below) ----
    ("tgp_ell_flow_f64", dict(model=None), -1),
    ("tgp_ell_flow_f64", dict(program=None, nblk=1), -1),
    ("tgp_ell_flow_f64", dict(theta=None), -1),
    ("tgp_ell_flow_f64", dict(nblk=-1, workspace_bytes=0), WSP),
    ("tgp_ell_flow_f64", dict(P=-1, workspace_bytes=0), WSP),
    ("tgp_ell_flow_f64", dict(RP=-1, workspace_bytes=0), WSP),
    ("tgp_ell_flow_f64", dict(Y=None), -2),
    ("tgp_ell_flow_f64", dict(mu=None), -3),
    ("tgp_flow_eval_f64", dict(model=None), -1),
    ("tgp_flow_eval_f64", dict(program=None, nblk=1), -1),
    ("tgp_flow_eval_f64", dict(theta=None), -1),
    ("tgp_flow_eval_f64", dict(nblk=-1, **ROWP), -5),
    ("tgp_flow_eval_f64", dict(P=-1, **ROWP), -5),
    ("tgp_flow_eval_f64", dict(RP=-1, **NBLK65), UNSUP),
    ("tgp_flow_eval_f64", dict(f=None), -2),
    ("tgp_flow_eval_f64", dict(S_=0), -3),
    ("tgp_flow_logdet_f64", dict(model=None), -1),
    ("tgp_flow_logdet_f64", dict(program=None, nblk=1), -1),
    ("tgp_flow_logdet_f64", dict(theta=None), -1),
    ("tgp_flow_logdet_f64", dict(nblk=-1, **ROWP), -5),
    ("tgp_flow_logdet_f64", dict(P=-1, **ROWP), -5),
    ("tgp_flow_logdet_f64", dict(RP=-1, workspace_bytes=0), WSP),
    ("tgp_flow_logdet_f64", dict(f=None), -2),
    ("tgp_flow_logdet_f64", dict(S_=0), -3),
    ("tgp_ell_warp_f64", dict(model=None), -1),
    ("tgp_ell_warp_f64", dict(program=None, nblk=1), -1),
    ("tgp_ell_warp_f64", dict(theta=None), -1),
    ("tgp_ell_warp_f64", dict(nblk=-1), -1),
    ("tgp_ell_warp_f64", dict(P=-1), -1),
    ("tgp_ell_warp_f64", dict(RP=-1), UNSUP),
    ("tgp_ell_warp_f64", dict(nblk=-1, RP=1), -1),              # (the counts are looked at before RP)
    ("tgp_ell_warp_f64", dict(program=None, nblk=1, RP=1), UNSUP),      # (RP before the program)
    ("tgp_ell_warp_f64", dict(Y=None), -2),
    ("tgp_ell_warp_f64", dict(mu=None), -3),
    ("tgp_flow_inverse_f64", dict(model=None), -1),
    ("tgp_flow_inverse_f64", dict(program=None, nblk=1), -1),
    ("tgp_flow_inverse_f64", dict(theta=None), -1),
    ("tgp_flow_inverse_f64", dict(nblk=-1), -1),
    ("tgp_flow_inverse_f64", dict(P=-1), -1),
    ("tgp_flow_inverse_f64", dict(RP=-1), -1),
    ("tgp_flow_inverse_f64", dict(t=None), -2),
    ("tgp_flow_inverse_f64", dict(S_=0), -3),
    ("tgp_predict_f64", dict(model=None), -1),                  # (lik = TGP_LIK_WARPED: the branch with the flow checks)
    ("tgp_predict_f64", dict(program=None, nblk=1), -1),
    ("tgp_predict_f64", dict(theta=None), -1),
    ("tgp_predict_f64", dict(nblk=-1), -1),
    ("tgp_predict_f64", dict(P=-1), -1),
    ("tgp_predict_f64", dict(RP=-1, mu=None), -2),              # (RP is ignored there)
    ("tgp_predict_f64", dict(mu=None), -2),
    ("tgp_predict_f64", dict(v=None), -3),
    ("tgp_predict_f64", dict(lik=L.LIK_FLOW, nblk=-1, **ROWP), -4),      # (the other branch checks no count)
    ("tgp_predict_quantile_f64", dict(model=None), -1),
    ("tgp_predict_quantile_f64", dict(program=None, nblk=1, mu=None), -2),      # (a missing program: make_prog's, last)
    ("tgp_predict_quantile_f64", dict(program=None, nblk=1), -1),
    ("tgp_predict_quantile_f64", dict(theta=None), -1),
    ("tgp_predict_quantile_f64", dict(nblk=-1), -1),
    ("tgp_predict_quantile_f64", dict(P=-1), -1),
    ("tgp_predict_quantile_f64", dict(RP=-1), -1),
    ("tgp_predict_quantile_f64", dict(mu=None), -2),
    ("tgp_predict_quantile_f64", dict(v=None), -3),
    ("tgp_predict_cdf_f64", dict(model=None), -1),
    ("tgp_predict_cdf_f64", dict(program=None, nblk=1, mu=None), -2),
    ("tgp_predict_cdf_f64", dict(program=None, nblk=1), -1),
    ("tgp_predict_cdf_f64", dict(theta=None), -1),
    ("tgp_predict_cdf_f64", dict(nblk=-1), -1),
    ("tgp_predict_cdf_f64", dict(P=-1), -1),
    ("tgp_predict_cdf_f64", dict(RP=-1), -1),
    ("tgp_predict_cdf_f64", dict(mu=None), -2),
    ("tgp_predict_cdf_f64", dict(v=None), -3),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, model=None), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, nblk=1, P=2, program=None), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, nblk=1, P=2, program=[(AFF, 0, 0, 0)], theta=None), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, nblk=-1), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, P=-1), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, RP=-1), UNSUP),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, nblk=0, P=3), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, X=None), -2),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, Y=None), -3),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_WARPED, nblk=1, P=2, program=[(AFF, 0, 0, 0)], g_theta=0), WSP),
    # ---- make_prog, through tgp_flow_eval_f64 ----
    ("tgp_flow_eval_f64", dict(program=[(-1, 0, 0, 0)]), -1),
    ("tgp_flow_eval_f64", dict(program=[(6, 0, 0, 0)]), -1),
    ("tgp_flow_eval_f64", dict(program=[(TANH, 0, 0, 0)]), -1),
    ("tgp_flow_eval_f64", dict(program=TANH_PER_ROW, RP=4, rowp=PTR), -1),
    ("tgp_flow_eval_f64", dict(program=[(AFF, 0, 1, 0)]), -1),                   # poff + np one past P
    ("tgp_flow_eval_f64", dict(program=[(AFF, 0, -1, 0)], P=4), -1),
    ("tgp_flow_eval_f64", dict(program=[(AFF, 0, 0, 0), (SAL, 0, 1, 0)], P=2), -1),
    ("tgp_flow_eval_f64", dict(program=[(AFF, 0, 0, PER_ROW)], RP=1, rowp=PTR), -1),     # ... past RP for a per-row block
    ("tgp_flow_eval_f64", dict(program=[(AFF, 0, 0, 0)] * 65), UNSUP),
    # (poff + np == P exactly: the step is the entry with a refusal behind make_prog -- its workspace check)
    ("tgp_elbo_step_f64", dict(lik=L.LIK_FLOW, S=4, nblk=1, P=2, program=[(AFF, 0, 1, 0)], g_theta=0), -1),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_FLOW, S=4, nblk=1, P=3, program=[(AFF, 0, 1, 0)], g_theta=0), WSP),
    ("tgp_elbo_step_f64", dict(lik=L.LIK_FLOW, S=4, nblk=1, P=4, program=[(TANH, 1, 0, 0)], g_theta=0), WSP),
    # ---- make_softmax, through tgp_predict_softmax_f64 (mu = NULL is the refusal behind the descriptor's checks) ----
    ("tgp_predict_softmax_f64", dict(model=None), -1),
    ("tgp_predict_softmax_f64", dict(), -2),
    ("tgp_predict_softmax_f64", dict(program=[(-1, 0, 0, 0)] + [(AFF, 0, 0, 0)] * 2), -1),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0)] * 2 + [(6, 0, 0, 0)]), -1),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0), (TANH, 0, 0, 0), (AFF, 0, 0, 0)]), -1),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0), (AFF, 0, 0, PER_ROW), (AFF, 0, 0, 0)]), UNSUP),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0)] * 2 + TANH_PER_ROW, theta_off=[0, 2, 4, 8]), UNSUP),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0)] * 2 + [(AFF, 0, 1, PER_ROW)]), UNSUP),    # (per-row before the offsets)
    ("tgp_predict_softmax_f64", dict(program=[(-1, 0, 0, PER_ROW)] + [(AFF, 0, 0, 0)] * 2), -1),        # (the kind before per-row)
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0), (AFF, 0, 1, 0), (AFF, 0, 0, 0)]), -1),    # one past the CLASS's P
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0), (AFF, 0, 1, 0), (AFF, 0, 0, 0)], theta_off=[0, 2, 5, 7]), -2),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0), (AFF, 0, -1, 0), (AFF, 0, 0, 0)]), -1),
    ("tgp_predict_softmax_f64", dict(program=[(AFF, 0, 0, 0)] * 65, blk_off=[0, 1, 2, 65]), UNSUP),
    ("tgp_predict_softmax_f64", dict(C=2), UNSUP),
    ("tgp_predict_softmax_f64", dict(C=33), UNSUP),
    ("tgp_predict_softmax_f64", dict(S=L.SOFTMAX_MAX_S + 1), UNSUP),
    ("tgp_predict_softmax_f64", dict(S=0), UNSUP),
    ("tgp_predict_softmax_f64", dict(blk_off=[0, 2, 1, 3]), -1),
    ("tgp_predict_softmax_f64", dict(theta_off=[0, 4, 2, 6]), -1),
    ("tgp_predict_softmax_f64", dict(blk_off=[1, 1, 2, 3]), -1),
    ("tgp_predict_softmax_f64", dict(program=None), -1),
    ("tgp_predict_softmax_f64", dict(theta=None), -1),
    ("tgp_predict_softmax_f64", dict(mu=PTR, v=None), -3),
    # ---- tgp_adam_args: the step, the warped step, the MLP backward ----
    ("tgp_elbo_step_adam_f64", dict(adam=None), -12),
    ("tgp_elbo_step_adam_f64", dict(), WSP),                    # (every view inside the buffer: on to the workspace check)
    ("tgp_elbo_step_adam_f64", dict(params=None), -12),
    ("tgp_elbo_step_adam_f64", dict(grads_buf=None), -12),
    ("tgp_elbo_step_adam_f64", dict(exp_avg=None), -12),
    ("tgp_elbo_step_adam_f64", dict(exp_avg_sq=None), -12),
    ("tgp_elbo_step_adam_f64", dict(step_dev=None), -12),
    ("tgp_elbo_step_adam_f64", dict(n=0), -12),
    ("tgp_elbo_step_adam_f64", dict(g_m=-16), -12),             # a gradient in front of the buffer
    ("tgp_elbo_step_adam_f64", dict(g_log_var_noise=308), -12),         # ... behind it
    ("tgp_elbo_step_adam_f64", dict(g_Lam=53), -12),            # ... a block that starts inside and runs past the end
    ("tgp_elbo_step_adam_f64", dict(n=307), -12),
    ("tgp_elbo_step_adam_f64", dict(phases=3, g_m=-16), WSP),   # (no backward phase: no update, adam is not looked at)
    ("tgp_elbo_step_adam_f64", dict(lik=L.LIK_WARPED, exp_avg=None), -12),
    ("tgp_elbo_step_adam_f64", dict(lik=L.LIK_WARPED, n=0), -12),
    ("tgp_elbo_step_adam_f64", dict(lik=L.LIK_WARPED, nblk=1, P=2, program=[(AFF, 0, 0, 0)], g_theta=307), -12),
    ("tgp_elbo_step_adam_f64", dict(lik=L.LIK_WARPED, nblk=1, P=2, program=[(AFF, 0, 0, 0)], g_theta=308, n=310), WSP),
    ("tgp_mlp_backward_adam_f64", dict(model=None), -1),
    ("tgp_mlp_backward_adam_f64", dict(adam=None), -9),
    ("tgp_mlp_backward_adam_f64", dict(exp_avg=None), -9),
    ("tgp_mlp_backward_adam_f64", dict(exp_avg_sq=None), -9),
    ("tgp_mlp_backward_adam_f64", dict(step_dev_adam=None), -9),
    ("tgp_mlp_backward_adam_f64", dict(params=PTR), -9),        # not the W of the call
    ("tgp_mlp_backward_adam_f64", dict(grads_buf=PTR), -9),
    ("tgp_mlp_backward_adam_f64", dict(n=33), -9),              # 2 nets x 17 weights = 34
    ("tgp_mlp_backward_adam_f64", dict(n=35), -9),
    ("tgp_mlp_backward_adam_f64", dict(n=0), -9),
    # ---- TGP_E_WORKSPACE: one byte less than the query, fused (M = 16) and general-M (M = 136) ----
    ("tgp_elbo_step_f64", dict(M=16, workspace_bytes="query-1"), WSP),
    ("tgp_elbo_step_f64", dict(M=136, workspace_bytes="query-1"), WSP),
    # (the fused forward plan is smaller than the query, which sizes the training step: one byte less would still run, so
    #  this row gives the entry no workspace at all)
    ("tgp_qf_moments_f64", dict(M=16, workspace_bytes=0), WSP),
    ("tgp_qf_moments_f64", dict(M=136, workspace_bytes="query-1"), WSP),
    ("tgp_qf_moments_bwd_f64", dict(M=16, workspace_bytes="query-1"), WSP),
    ("tgp_qf_moments_bwd_f64", dict(M=136, workspace_bytes="query-1"), WSP),
    ("tgp_elbo_step_f64", dict(M=16, kernel=1, workspace_bytes="query-1"), WSP),        # (Matern: general path at any M)
    ("tgp_qf_moments_f64", dict(model=None), -1),
    ("tgp_qf_moments_f64", dict(X=None), -2),
    ("tgp_qf_moments_bwd_f64", dict(model=None), -1),
    ("tgp_qf_moments_bwd_f64", dict(X=None), -2),
]


def _host_i32(keep, values):
    arr = (C.c_int32 * len(values))(*values)
    keep.append(arr)
    return C.cast(arr, C.c_void_p)


def _model(base, over, keep):
    if "model" in over:
        return None
    f = dict(base, **{k: v for k, v in over.items() if k in dict(L.TgpModel._fields_)})
    md = L.TgpModel()
    md.scale, md.kl_scale = 1.0, 1.0
    for k in GP + ("theta", "xs", "wn"):
        setattr(md, k, f.pop(k, PTR))
    prog = f.pop("program")
    if prog is not None:
        md.program = _host_i32(keep, [x for blk in prog for x in blk])
        f["nblk"] = over.get("nblk", len(prog))
    for k, v in f.items():
        setattr(md, k, v)
    return md


def _softmax(over, keep):
    if "model" in over:
        return None
    f = dict(SMX, theta=PTR)
    f.update((k, v) for k, v in over.items() if k in dict(L.TgpSoftmax._fields_))
    d = L.TgpSoftmax()
    d.N, d.C, d.S, d.scale, d.theta = f["N"], f["C"], f["S"], 1.0, f["theta"]
    if f["program"] is not None:
        d.program = _host_i32(keep, [x for blk in f["program"] for x in blk])
    d.blk_off = _host_i32(keep, f["blk_off"] + [f["blk_off"][-1]] * 30)      # (read up to index C)
    d.theta_off = _host_i32(keep, f["theta_off"] + [f["theta_off"][-1]] * 30)
    return d


def _grads(over):
    gs = L.TgpGrads()
    off = dict(ADAM_OFF, **{k[2:]: v for k, v in over.items() if k.startswith("g_")})
    for k, o in off.items():
        setattr(gs, k, C.c_void_p(ADAM_BASE + F64 * o))
    return gs


def _adam(over, mlp):
    if "adam" in over:
        return None
    ad = L.TgpAdamArgs()
    ad.params, ad.grads, ad.exp_avg, ad.exp_avg_sq, ad.step_dev = PTR, C.c_void_p(ADAM_BASE), PTR, PTR, PTR
    ad.n, ad.lr, ad.beta1, ad.beta2, ad.eps = 308, 1e-2, 0.9, 0.999, 1e-8
    if mlp:
        ad.params, ad.grads, ad.n = C.c_void_p(ADAM_BASE), C.c_void_p(ADAM_BASE + 0x10000), 34
    names = dict(params="params", grads_buf="grads", exp_avg="exp_avg", exp_avg_sq="exp_avg_sq", step_dev="step_dev",
                 step_dev_adam="step_dev", n="n", phases="phases")
    for k, field in names.items():
        if k in over and not (mlp and k == "step_dev"):
            setattr(ad, field, over[k])
    return ad


def call(lib, entry, over):
    """The return code of `entry` for the table's base call changed by `over`."""
    base, args = ENTRIES[entry]
    keep = []
    if entry == "tgp_predict_softmax_f64":
        first = _softmax(over, keep)
    elif entry == "tgp_mlp_backward_adam_f64":
        first = None
        if "model" not in over:
            first = L.TgpMlp()
            for k, v in MLP.items():
                setattr(first, k, v)
    else:
        first = _model(base, over, keep)
    vals = []
    for name, v in args:
        v = over.get(name, v)
        if isinstance(v, str) and v == "grads":
            v = _grads(over)
        elif isinstance(v, str) and v == "adam":
            v = _adam(over, entry == "tgp_mlp_backward_adam_f64")
        elif isinstance(v, str) and v == "query-1":       # the Gaussian step's / the q(f) entries' own query, less one byte
            v = lib.tgp_workspace_bytes_plan(base["N"], base["D"], over["M"], 1, 0, 0, 0, over.get("kernel", 0), 0) - 1
        vals.append(v)
    return getattr(lib, entry)(first, *vals)


def test_the_table_is_large_enough_and_every_row_is_a_refusal():
    assert len(ROWS) >= 60 and all(code < 0 for _, _, code in ROWS)
    assert set(FLOW8) <= {e for e, _, _ in ROWS}
    assert len({(e, repr(sorted(o.items(), key=str))) for e, o, _ in ROWS}) == len(ROWS)      # no row twice


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: "%s-%d" % (ROWS[i][0][4:-4], i))
def test_refusal(row):
    entry, over, code = ROWS[row]
    assert call(L.load(), entry, over) == code, (entry, over)
