"""Operator layer: torch tensors in, HIP kernels underneath (through the C ABI in lib.py).

`elbo_step` is the fused replacement of `sparse_MF_SP.ELBO` + `loss.backward()` for one minibatch
(reference: code/dsp/models/sparse_MF_SP.py:552-598, code/dsp/trainers/trainer_base.py:337-341);
`ElboFunction` wraps it as a torch.autograd.Function so the reference's trainer idiom
(`loss = -ELBO; loss.backward(); optimizer.step()`) keeps working on the drop-in model classes.
The other functions expose the stand-alone operators of the path.
"""
import math
import warnings

import numpy as np
import torch

from . import lib as L


class NanError(RuntimeError):
    """Same role as gpytorch.utils.errors.NanError raised by dsp/utils.py:241-254."""


STATUS_SYNC_TIMEOUT = -77   # include/tgp_hip.h TGP_STATUS_SYNC_TIMEOUT: status[0] of a launch whose hand-off wait expired


class HandoffTimeoutError(RuntimeError):
    """A workgroup of the prepare or of the M x M backward launch gave up waiting for a hand-off word (status[0] == TGP_STATUS_SYNC_TIMEOUT):
    the status buffer's hand-off words (status[4..7]) were not zero at the call, or the launch's producer workgroups
    never became resident.  The results of that call are invalid; this is NOT a Cholesky failure."""


class NotPSDError(RuntimeError):
    pass


class NumericalWarning(RuntimeWarning):
    pass


# ---------------------------------------------------------------------------------------------------
# quadrature nodes (gpytorch GaussHermiteQuadrature1D: numpy hermgauss) and workspace cache
# ---------------------------------------------------------------------------------------------------
_quad_cache = {}


def gauss_hermite(S, device):
    """(xs, wn = w/sqrt(pi), logw) as float64 device tensors."""
    key = (int(S), str(device))
    if key not in _quad_cache:
        x, w = np.polynomial.hermite.hermgauss(int(S))
        xs = torch.tensor(x, dtype=torch.float64, device=device)
        wn = torch.tensor(w / math.sqrt(math.pi), dtype=torch.float64, device=device)
        _quad_cache[key] = (xs, wn)
    return _quad_cache[key]


_ws_cache = {}


def kernel_id(kernel):
    """A name of lib.KERNELS ('scale_rbf', 'scale_matern32': instance_kernel names, models/utils_models.py:188-204;
    'scale_matern52', 'scale_rq') or a TGP_KERNEL_* id."""
    if isinstance(kernel, str):
        if kernel not in L.KERNELS:
            raise L.TgpError("kernel '%s' has no HIP implementation (have: %s)" % (kernel, ", ".join(L.KERNELS)))
        return L.KERNELS[kernel]
    return int(kernel)


def workspace_bytes(N, D, M, S, nblk, P, RP, kernel=0, plan=0, lik=L.LIK_GAUSS):
    """Bytes of device workspace one ELBO step of this shape needs: the one place the library is asked."""
    nbytes = L.load().tgp_workspace_bytes_lik(N, D, M, max(S, 1), nblk, P, RP, kernel, int(plan), int(lik))
    if nbytes == 0:
        raise L.TgpError("unsupported problem shape N=%d D=%d M=%d (this build: D<=16, M<=4096)" % (N, D, M))
    return nbytes


def new_workspace(N, D, M, S, nblk, P, RP, device, kernel=0, plan=0, lik=L.LIK_GAUSS):
    """A workspace of the caller's own (engine.ElboEngine: a step split into phases keeps its intermediates there)."""
    return torch.empty(workspace_bytes(N, D, M, S, nblk, P, RP, kernel, plan, lik) // 8 + 16, dtype=torch.float64, device=device)


def workspace(N, D, M, S, nblk, P, RP, device, kernel=0, plan=0, lik=L.LIK_GAUSS):
    """The cached workspace of the stateless one-shot calls of this module: one buffer per shape and stream, valid for the
    duration of ONE call -- nothing that keeps state between calls may hold it."""
    key = (N, D, M, S, nblk, P, RP, str(device), torch.cuda.current_stream().cuda_stream, kernel, int(plan), int(lik))
    buf = _ws_cache.get(key)
    if buf is None:
        buf = _ws_cache[key] = new_workspace(N, D, M, S, nblk, P, RP, device, kernel, plan, lik)
    return buf


def _scratch(nbytes, device, override=None):
    """(workspace, its byte count for the library) of a stand-alone operator whose sizer gave `nbytes`; `override` replaces
    that count (tests of the library's refusal).  Never an empty tensor: the library wants an address."""
    nbytes = int(nbytes if override is None else override)
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device), nbytes


def _status(device):
    """The zeroed status words of one call (include/tgp_hip.h: [0] pivot, [1] NaN, [3] expired waits, [4..7] hand-off words)."""
    return torch.zeros(8, dtype=torch.int32, device=device)


def _c(t, name):
    if t is None:
        return None
    if t.dtype != torch.float64:
        raise L.TgpError("%s must be float64 (the reference's main.py runs in float64), got %s" % (name, t.dtype))
    return t.contiguous()


class FlowSpec:
    """Device-side description of a flow: program (nblk,4) int32, P shared scalars, RP per-row columns."""

    def __init__(self, program, P, RP, device):
        self.blocks = [tuple(int(v) for v in b) for b in program]
        self.nblk = len(self.blocks)
        self.P, self.RP = int(P), int(RP)
        # host array: the C ABI copies the program into the kernel arguments
        self.program = np.ascontiguousarray(np.array(self.blocks if self.blocks else [(0, 0, 0, 0)], dtype=np.int32))

    @property
    def program_ptr(self):
        import ctypes
        return ctypes.c_void_p(self.program.ctypes.data)

    def to(self, device):
        return FlowSpec(self.blocks, self.P, self.RP, device)


def _model_struct(X, Z, raw_ls, raw_os, m, Lam, lvn, scale, jitter, kl_scale, flow, theta, S, kernel=0, plan=0, lik=None):
    """`lik` None: LIK_GAUSS without a flow, LIK_FLOW with one; LIK_BERNOULLI needs a FlowSpec (empty for SVGP)."""
    md = L.TgpModel()
    md.kernel = kernel_id(kernel)
    _os(raw_os, md.kernel)       # (two doubles behind the pointer for 'scale_rq')
    md.plan = int(plan)          # lib.PLAN_*: which of the equivalent kernels this call runs; 0 = the library's choice
    md.N, md.D = X.shape[0], X.shape[1]
    md.M = m.numel()
    md.scale, md.jitter, md.kl_scale = float(scale), float(jitter), float(kl_scale)
    md.Z, md.raw_ls, md.raw_os = L.ptr(Z), L.ptr(raw_ls), L.ptr(raw_os)
    md.m, md.Lam, md.log_var_noise = L.ptr(m), L.ptr(Lam), L.ptr(lvn)
    keep = []
    if flow is None:
        md.lik, md.S, md.nblk, md.P, md.RP = L.LIK_GAUSS, 1, 0, 0, 0
    else:
        xs, wn = gauss_hermite(S, X.device)
        keep += [xs, wn]
        md.lik, md.S, md.nblk, md.P, md.RP = L.LIK_FLOW if lik is None else int(lik), int(S), flow.nblk, flow.P, flow.RP
        md.program, md.xs, md.wn = flow.program_ptr, L.ptr(xs), L.ptr(wn)
        md.theta = L.ptr(theta) if flow.P > 0 else None
    return md, keep


def student_noise(lvn, df):
    """The two doubles {log sigma^2, nu} a TGP_LIK_STUDENT call's log_var_noise points to, as one float64 tensor on lvn's device:
    `lvn` the one-element log squared scale, `df` the degrees of freedom (a number or a one-element tensor).  ValueError
    outside the supported range 2 < nu <= lib.STUDENT_MAX_DF when `df` is a number (a tensor is not read back)."""
    if df is None:
        raise L.TgpError("the Student-t likelihood needs its degrees of freedom (df)")
    if not torch.is_tensor(df):
        check_student_df(df)
        df = torch.tensor([float(df)], dtype=torch.float64, device=lvn.device)
    return torch.cat((lvn.detach().reshape(-1)[:1].to(torch.float64), df.detach().reshape(-1)[:1].to(lvn.device, torch.float64)))


_EDGES_SEEN = {}      # (data_ptr, version, numel, device) of the last device tensor of bin edges check_ordinal_edges passed


def check_ordinal_edges(edges):
    """The bin edges of the ordinal likelihood as a float64 vector; ValueError unless they are finite, strictly increasing and
    1 <= len <= lib.ORDINAL_MAX_K - 1.  A device tensor is read back once: the check of an unchanged buffer is remembered."""
    e = torch.as_tensor(edges, dtype=torch.float64).detach().reshape(-1)
    key = (e.data_ptr(), e._version, e.numel(), str(e.device))
    if e.is_cuda and _EDGES_SEEN.get("key") == key:
        return e
    if not 1 <= e.numel() <= L.ORDINAL_MAX_K - 1:
        raise ValueError("the ordinal likelihood takes 1 to %d bin edges (2 to %d classes), got %d"
                         % (L.ORDINAL_MAX_K - 1, L.ORDINAL_MAX_K, e.numel()))
    h = e.cpu()
    if not bool(torch.isfinite(h).all()):
        raise ValueError("the bin edges of the ordinal likelihood must be finite, got %s" % h.tolist())
    if not bool((h[1:] > h[:-1]).all()):
        raise ValueError("the bin edges of the ordinal likelihood must be strictly increasing, got %s" % h.tolist())
    if e.is_cuda:
        _EDGES_SEEN["key"] = key
    return e


def ordinal_noise(lvn, edges):
    """The K + 1 doubles {log sigma^2, K, b_1, .., b_{K-1}} a TGP_LIK_ORDINAL call's log_var_noise points to, as one float64 tensor
    on lvn's device: `lvn` the one-element log noise variance, `edges` the K - 1 bin edges (a sequence or a tensor; no gradient).
    ValueError unless the edges are finite, strictly increasing and 1 <= len <= 63 (check_ordinal_edges)."""
    if edges is None:
        raise L.TgpError("the ordinal likelihood needs its bin edges")
    e = check_ordinal_edges(edges).to(lvn.device)
    K = torch.full((1,), float(e.numel() + 1), dtype=torch.float64, device=lvn.device)     # (a fill: no host-to-device copy)
    return torch.cat((lvn.detach().reshape(-1)[:1].to(torch.float64), K, e))


def noise_slot(lvn, lik, extras):
    """What sits behind the ABI's noise pointer in a call at likelihood `lik`: `lvn` itself, or, for the likelihoods that carry
    fixed hyper-parameters beside the noise, lvn[0] followed by them -- `extras` is what rides there: the degrees of freedom of
    LIK_STUDENT (student_noise), the bin edges of LIK_ORDINAL (ordinal_noise)."""
    if lik == L.LIK_STUDENT:
        return student_noise(lvn, extras)
    if lik == L.LIK_ORDINAL:
        return ordinal_noise(lvn, extras)
    return lvn


def rq_scale(raw_os, alpha):
    """The two doubles {raw_outputscale, alpha} a TGP_KERNEL_SCALE_RQ call's raw_os points to, as one float64 tensor on raw_os's
    device: `raw_os` the one-element raw output scale (autograd flows through to it), `alpha` a number or a one-element tensor.
    ValueError outside lib.RQ_MIN_ALPHA <= alpha <= lib.RQ_MAX_ALPHA when `alpha` is a number (a tensor is not read back)."""
    if alpha is None:
        raise L.TgpError("the rational-quadratic kernel needs its alpha")
    if not torch.is_tensor(alpha):
        alpha = torch.tensor([check_rq_alpha(alpha)], dtype=torch.float64, device=raw_os.device)
    return torch.cat((raw_os.reshape(-1)[:1].to(torch.float64), alpha.detach().reshape(-1)[:1].to(raw_os.device, torch.float64)))


def check_rq_alpha(alpha):
    """ValueError unless lib.RQ_MIN_ALPHA <= alpha <= lib.RQ_MAX_ALPHA: above, the kernel is the RBF to O(1/alpha)."""
    alpha = float(alpha)
    if not (L.RQ_MIN_ALPHA <= alpha <= L.RQ_MAX_ALPHA):
        raise ValueError("the rational-quadratic alpha must be in [%g, %g], got %g" % (L.RQ_MIN_ALPHA, L.RQ_MAX_ALPHA, alpha))
    return alpha


def _os(raw_os, kernel):
    """The contiguous float64 raw_os of a call with `kernel`: one element, or rq_scale's two for 'scale_rq' -- the library reads
    raw_os[1] for that kernel, so a shorter tensor is refused here."""
    raw_os = _c(raw_os, "raw_os")
    want = 2 if kernel_id(kernel) == L.KERNEL_SCALE_RQ else 1
    if raw_os.numel() != want:
        raise ValueError("raw_os: %d element%s for this kernel (ops.rq_scale packs {raw_outputscale, alpha} for 'scale_rq'), got %d"
                         % (want, "s" if want > 1 else "", raw_os.numel()))
    return raw_os


def _os_grad(raw_os):
    """Where a call writes d/d raw_outputscale: raw_os's shape, the library fills element 0 and alpha's slot stays zero."""
    return torch.empty_like(raw_os) if raw_os.numel() == 1 else torch.zeros_like(raw_os)


def check_student_df(df):
    """ValueError unless 2 < df <= lib.STUDENT_MAX_DF: below, the Student-t has no variance; above, its constant's two lgamma
    cancel to ~1e-9 and the Gaussian likelihood is the one to take."""
    df = float(df)
    if not (2.0 < df <= L.STUDENT_MAX_DF):
        raise ValueError("Student-t degrees of freedom must be in (2, %g], got %g" % (L.STUDENT_MAX_DF, df))
    return df


def elbo_step(X, Y, Z, raw_ls, raw_os, m, Lam, lvn, N_total, flow=None, theta=None, rowp=None, S=None, jitter=0.0,
              kl_scale=1.0, mb_global=None, want_moments=False, kernel="scale_rbf", plan=0, lik=None, df=None):
    """One fused ELBO evaluation + all gradients on the GPU.  Returns (out[4], grads dict, status[8], (mu, v)); status[0..2] are the
    Cholesky words of include/tgp_hip.h, status[4..7] the in-launch hand-off words (zero before and after every call).

    out = [ELL_shard - KL, ELL_shard, KL, 0]; grads are d(ELL_shard - kl_scale*KL)/d(param).
    `mb_global` = global minibatch size when X is a row shard (defaults to X.shape[0]).
    `lik` = lib.LIK_BERNOULLI: probit likelihood through `flow` (a FlowSpec, possibly empty); lvn is read by no kernel and
    its gradient is 0.  `lik` = lib.LIK_POISSON: counts Y with the flow as the log-rate, the same conventions.
    `lik` = lib.LIK_STUDENT: Student-t noise of `df` degrees of freedom around the flow; lvn (one element) is the log of the
    squared scale and grads["lvn"] its one-element gradient; `df` has none.
    `lik` = lib.LIK_NEGBIN: negative-binomial counts with the flow as the log-mean; lvn (one element) is the log dispersion
    log r and grads["lvn"] its gradient.
    `lik` = lib.LIK_ORDINAL: ordered classes Y in {0, .., K-1} (cumulative probit around the flow); lvn (one element) is the log
    noise variance and grads["lvn"] its gradient.  `df` is the slot for what rides beside the noise (noise_slot): here the K - 1
    fixed bin edges, which have no gradient.
    `lik` = lib.LIK_GAMMA / lib.LIK_BETA: positive targets with the flow as the log-mean / proportions in (0, 1) with the flow as
    the log-odds of the mean; lvn (one element) is the log shape / the log precision and grads["lvn"] its gradient."""
    lib = L.load()
    X, Y = _c(X, "X"), _c(Y.reshape(-1), "Y")
    Z, raw_ls, raw_os, m, Lam, lvn = (_c(t, n) for t, n in ((Z, "Z"), (raw_ls, "raw_ls"), (raw_os, "raw_os"), (m, "m"),
                                                               (Lam, "Lam"), (lvn, "log_var_noise")))
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    dev = X.device
    N, D = X.shape
    M = m.numel()
    scale = float(N_total) / float(mb_global if mb_global is not None else N)
    if lik in L.LIK_DISPLAY and flow is None:
        raise L.TgpError(L.NEEDS_FLOWSPEC % L.LIK_DISPLAY[lik])
    # (LIK_STUDENT: the library reads {log sigma^2, nu} behind the noise pointer and writes one gradient, that of log sigma^2)
    if lik == L.LIK_STUDENT and lvn.numel() != 1:
        raise L.TgpError("the Student-t step takes a one-element log_var_noise (log sigma^2); the degrees of freedom go in `df`")
    if lik == L.LIK_ORDINAL and lvn.numel() != 1:
        raise L.TgpError("the ordinal step takes a one-element log_var_noise (log sigma^2); the bin edges go in `df`")
    noise = noise_slot(lvn, lik, df)
    md, keep = _model_struct(X, Z, raw_ls, raw_os, m, Lam, noise, scale, jitter, kl_scale, flow, theta, S, kernel, plan, lik)
    ws = workspace(N, D, M, md.S, md.nblk, md.P, md.RP, dev, md.kernel, plan, md.lik)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    status = _status(dev)
    g = {"Z": torch.empty_like(Z), "raw_ls": torch.empty_like(raw_ls), "raw_os": _os_grad(raw_os),
         "m": torch.empty_like(m), "Lam": torch.empty_like(Lam), "lvn": torch.empty_like(lvn)}
    gs = L.TgpGrads()
    gs.Z, gs.raw_ls, gs.raw_os, gs.m, gs.Lam, gs.log_var_noise = (L.ptr(g[k]) for k in ("Z", "raw_ls", "raw_os", "m",
                                                                                          "Lam", "lvn"))
    if md.P > 0:
        g["theta"] = torch.empty_like(theta)
        gs.theta = L.ptr(g["theta"])
    if md.RP > 0:
        g["rowp"] = torch.empty_like(rowp)
        gs.rowp = L.ptr(g["rowp"])
    mu = v = None
    if want_moments:
        mu = torch.empty(N, dtype=torch.float64, device=dev)
        v = torch.empty(N, dtype=torch.float64, device=dev)
    rc = lib.tgp_elbo_step_f64(md, L.ptr(X), L.ptr(Y), L.ptr(rowp) if md.RP > 0 else None, L.ptr(out), gs, L.ptr(mu),
                               L.ptr(v), L.ptr(status), L.ptr(ws), ws.numel() * 8, L.stream_ptr())
    L.check(rc, "tgp_elbo_step_f64")
    return out, g, status, (mu, v)


def jitter_ladder(dtype=torch.float64, jitter=None):
    """The retry values of psd_safe_cholesky (dsp/utils.py:256-269): jitter * 10^i, i = 0..2."""
    if jitter is None:
        jitter = 1e-6 if dtype == torch.float32 else 1e-8
    return [jitter * (10 ** i) for i in range(3)]


def raise_for_status(status):
    """Translate the device status words into the reference's exceptions; returns True if a retry with more
    jitter is needed."""
    info, nan = int(status[0]), int(status[1])
    sticky = int(status[3]) if len(status) > 3 else 0
    if info == STATUS_SYNC_TIMEOUT or sticky:
        # status[3] counts the expired waits since the caller last zeroed it: status[0] is rewritten by every prepare launch, so a
        # timeout inside a replayed multi-step graph is only visible there
        raise HandoffTimeoutError("a hand-off wait inside the prepare / backward launch expired (status[0] = %d, %d expired wait(s) "
                                  "counted in status[3]): status[4..7] must be zero before the first call and untouched while a "
                                  "call is in flight; the step's results are invalid and the fused update was skipped where the "
                                  "launch could tell (Lam rows may have moved): restore the parameters" % (info, sticky))
    if nan:
        raise NanError("cholesky: K_MM contains NaN")
    return info != 0


def run_jitter_ladder(attempt, jitter=0.0, ladder=None, info=None, what="K_MM"):
    """psd_safe_cholesky's retry protocol (dsp/utils.py:222-270) around one factorising call: the only retry loop of this module.
    `attempt(jit)` runs the call at jitter `jit` and returns a true value when the factorisation FAILED -- the failing pivot
    as an int where it is known.  The first try is at `jitter`; after a failure the values of `ladder` (default:
    jitter_ladder()) above `jitter` are tried in turn, each success after a failure warns (NumericalWarning).  Returns the jitter
    it ended with (also in `info["jitter"]`); NotPSDError, naming `what`, when every value failed."""
    jitter = float(jitter)
    if info is not None:
        info["jitter"] = jitter
    bad = attempt(jitter)
    if not bad:
        return jitter
    last = jitter
    for jit in (jitter_ladder() if ladder is None else ladder):
        jit = float(jit)
        if jit <= jitter:
            continue
        last = jit
        bad = attempt(jit)
        if not bad:
            warnings.warn("A not p.d., added jitter of %g to the diagonal" % jit, NumericalWarning)
            if info is not None:
                info["jitter"] = jit
            return jit
    pivot = " (pivot %d)" % bad if isinstance(bad, int) and not isinstance(bad, bool) else ""
    raise NotPSDError("%s not positive definite even with jitter %g%s" % (what, last, pivot))


def _failed_pivot(status):
    """An `attempt` result from the status words of a call (one device sync): False, or the failing pivot."""
    status = status.cpu()
    return raise_for_status(status) and int(status[0])


def _laddered(call, status, jitter, ladder=None, info=None, check=True, what="K_MM"):
    """run_jitter_ladder around the library call `call(jit)` that factorises with `status`: the words are read after every
    launch (one host sync each) unless `check` is false -- then there is one launch and no retry."""
    def attempt(jit):
        call(jit)
        return check and raise_for_status(status.cpu())
    return run_jitter_ladder(attempt, jitter, ladder, info, what)


def elbo_step_safe(*args, global_jitter=None, **kw):
    """elbo_step + the reference's psd_safe_cholesky protocol (one device sync per call to read the status)."""
    res = None

    def attempt(jit):
        nonlocal res
        kw["jitter"] = jit
        res = elbo_step(*args, **kw)
        return _failed_pivot(res[2])
    run_jitter_ladder(attempt, kw.get("jitter", 0.0), jitter_ladder(jitter=global_jitter))
    return res


_STEP_PARAMS = ("Z", "raw_ls", "raw_os", "m", "Lam", "lvn", "theta", "rowp")


def _step_kwargs(cfg):
    """The keyword arguments of elbo_step a model's `cfg` dict stands for."""
    kw = dict(flow=cfg.get("flow"), S=cfg.get("S"), kl_scale=cfg.get("kl_scale", 1.0), mb_global=cfg.get("mb_global"),
              kernel=cfg.get("kernel", "scale_rbf"), lik=cfg.get("lik"), jitter=cfg.get("jitter", 0.0))
    if cfg.get("df") is not None:       # what rides beside the noise: a Student-t model's degrees of freedom, an ordinal one's edges
        kw["df"] = cfg["df"]
    return kw


def _step_save(ctx, grads, params, g_Y=None):
    ctx.grads = grads
    ctx.shapes = tuple(None if t is None else t.shape for t in params)
    ctx.g_Y = g_Y


def _gauss_target_adjoint(cfg, Y, lvn, mu):
    """d ELL / d Y of the Gaussian likelihood's closed form, -scale e^-eta (Y - mu), shape of Y: what the residual route of a
    mean function (the step runs on Y - m(X), cfg["grad_Y"]) sends back to m(X) with the sign turned."""
    if cfg.get("flow") is not None or cfg.get("lik") is not None:
        raise L.TgpError("grad_Y: the adjoint of the targets exists for the Gaussian likelihood's closed form only")
    scale = float(cfg["N_total"]) / float(cfg.get("mb_global") or Y.shape[0])
    return (mu - Y.detach().reshape(-1)).mul_(scale * torch.exp(-lvn.detach().reshape(-1)[0])).reshape(Y.shape)


def _step_backward(ctx, g_out):
    """The saved gradients of a step times the cotangent of its differentiable output, one per argument of forward."""
    res = tuple(None if shp is None or k not in ctx.grads else (ctx.grads[k] * g_out).reshape(shp)
                for k, shp in zip(_STEP_PARAMS, ctx.shapes))
    return (None, None if ctx.g_Y is None else ctx.g_Y * g_out) + res + (None,)


class ElboFunction(torch.autograd.Function):
    """(ELBO, ELL, KLD) = f(Z, raw_ls, raw_os, m, Lam, log_var_noise, theta, rowp); gradients flow through ELBO
    (the reference trainer differentiates `-ELBO`, trainers/trainers_regression.py:85-86); ELL and KLD are
    returned for logging and marked non-differentiable."""

    @staticmethod
    def forward(ctx, X, Y, Z, raw_ls, raw_os, m, Lam, lvn, theta, rowp, cfg):
        step, kw = elbo_step, _step_kwargs(cfg)
        if cfg.get("check_status", True):
            step, kw["global_jitter"] = elbo_step_safe, cfg.get("global_jitter")
        want_gy = bool(cfg.get("grad_Y"))
        out, g, status, (mu, _) = step(X, Y, Z, raw_ls, raw_os, m, Lam, lvn, cfg["N_total"], theta=theta, rowp=rowp,
                                       want_moments=want_gy, **kw)
        _step_save(ctx, g, (Z, raw_ls, raw_os, m, Lam, lvn, theta, rowp), _gauss_target_adjoint(cfg, Y, lvn, mu) if want_gy else None)
        cfg["last_status"] = status
        elbo, ell, kld = out[0].clone(), out[1].clone(), out[2].clone()
        ctx.mark_non_differentiable(ell, kld)
        return elbo, ell, kld

    @staticmethod
    def backward(ctx, g_elbo, g_ell, g_kld):
        return _step_backward(ctx, g_elbo)


# ---------------------------------------------------------------------------------------------------
# stand-alone operators
# ---------------------------------------------------------------------------------------------------
def _qf_model(X, Z, raw_ls, raw_os, m, Lam, jitter, kl_scale, kernel, plan=0):
    """What the q(f) operators open with: (TgpModel, X, (Z, raw_ls, raw_os, m, Lam), lvn) -- the contiguous float64 operands,
    a zero log_var_noise (a required pointer their kernels do not read) and the Gaussian model over them."""
    X = _c(X, "X")
    par = tuple(_c(t, "param") for t in (Z, raw_ls, raw_os, m, Lam))
    lvn = torch.zeros(1, dtype=torch.float64, device=X.device)
    md, _ = _model_struct(X, *par, lvn, 1.0, jitter, kl_scale, None, None, None, kernel, plan)
    return md, X, par, lvn


def qf_moments(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, check=True, kernel="scale_rbf", info=None, plan=0):
    """q(f) marginals (models/sparse_MF_SP.py:274-396): returns mu, v of shape (N,).  `info` (a dict) receives the
    jitter the factorisation ended with (info["jitter"]: the ladder of psd_safe_cholesky may have raised it).  `check` False:
    one call, the status is not read (no host sync)."""
    lib = L.load()
    md, X, par, lvn = _qf_model(X, Z, raw_ls, raw_os, m, Lam, jitter, 1.0, kernel, plan)
    dev = X.device
    ws = workspace(X.shape[0], X.shape[1], md.M, 1, 0, 0, 0, dev, md.kernel, plan)
    mu = torch.empty(X.shape[0], dtype=torch.float64, device=dev)
    v = torch.empty_like(mu)
    status = _status(dev)

    def call(jit):
        md.jitter = jit
        L.check(lib.tgp_qf_moments_f64(md, L.ptr(X), L.ptr(mu), L.ptr(v), L.ptr(status), L.ptr(ws), ws.numel() * 8,
                                       L.stream_ptr()), "tgp_qf_moments_f64")
    _laddered(call, status, jitter, info=info, check=check)
    return mu, v


def qf_cov(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, check=True, kernel="scale_rbf", info=None, workspace_bytes=None):
    """Full-covariance q(f) (models/sparse_MF_SP.py:274-396, diagonal=False; tgp_qf_cov_f64): returns mu (N,) and the
    symmetric Sigma (N, N) = K(X, X) + A^T (L_q L_q^T - I) A.  No autograd.  `check`: the jitter ladder of
    psd_safe_cholesky on K_MM, as in qf_moments; `info["jitter"]` receives the value the factorisation ended with.
    `workspace_bytes` overrides the size of the workspace handed to the library (tests of its refusal)."""
    lib = L.load()
    md, X, par, lvn = _qf_model(X, Z, raw_ls, raw_os, m, Lam, jitter, 1.0, kernel)
    dev = X.device
    N, D = X.shape
    if N > 4096:       # refused by the library before anything is allocated for an N x N result
        L.check(lib.tgp_qf_cov_f64(md, L.ptr(X), None, None, None, None, 0, L.stream_ptr()), "tgp_qf_cov_f64")
    ws, nbytes = _scratch(lib.tgp_qf_cov_workspace_bytes(N, D, md.M), dev, workspace_bytes)
    mu = torch.empty(N, dtype=torch.float64, device=dev)
    Sigma = torch.empty(N, N, dtype=torch.float64, device=dev)
    status = _status(dev)

    def call(jit):
        md.jitter = jit
        L.check(lib.tgp_qf_cov_f64(md, L.ptr(X), L.ptr(mu), L.ptr(Sigma), L.ptr(status), L.ptr(ws), nbytes, L.stream_ptr()),
                "tgp_qf_cov_f64")
    _laddered(call, status, jitter, info=info, check=check)
    return mu, Sigma


def qf_input_grad(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, check=True, kernel="scale_rbf", info=None, workspace_bytes=None):
    """Input gradients of the q(f) marginals (tgp_qf_input_grad_f64): returns (dmu, dv), each (N, D), the derivatives of
    qf_moments' mu_n and v_n in the row x_n they are evaluated at.  A row's moments depend on that row alone, so the adjoint of
    (g_mu, g_v) in X is g_mu[:, None] * dmu + g_v[:, None] * dv.  No autograd.  `check`: the jitter ladder of psd_safe_cholesky
    on K_MM, as in qf_moments; `info["jitter"]` receives the value the factorisation ended with.  `workspace_bytes` overrides
    the size of the workspace handed to the library (tests of its refusal)."""
    lib = L.load()
    md, X, par, lvn = _qf_model(X, Z, raw_ls, raw_os, m, Lam, jitter, 1.0, kernel)
    dev = X.device
    N, D = X.shape
    ws, nbytes = _scratch(lib.tgp_qf_input_grad_workspace_bytes(N, D, md.M), dev, workspace_bytes)
    dmu = torch.empty(N, D, dtype=torch.float64, device=dev)
    dv = torch.empty_like(dmu)
    status = _status(dev)

    def call(jit):
        md.jitter = jit
        L.check(lib.tgp_qf_input_grad_f64(md, L.ptr(X), L.ptr(dmu), L.ptr(dv), L.ptr(status), L.ptr(ws), nbytes, L.stream_ptr()),
                "tgp_qf_input_grad_f64")
    _laddered(call, status, jitter, info=info, check=check)
    return dmu, dv


def qf_input_grad_var(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, check=True, kernel="scale_rbf", info=None, workspace_bytes=None):
    """dvar (N, D): the variance of the derivative process under q(f), Var_q[d f(x_n) / d x_nd] = k_g(0) / l_d^2 +
    J_d^T L^-T W L^-1 J_d at the rows of X (tgp_qf_input_grad_var_f64) -- the error bar of qf_input_grad's dmu.  Stored as
    computed, never clamped: clamp at 0 where a square root is taken.  No autograd.  `check`, `info` and `workspace_bytes` as in
    qf_input_grad."""
    lib = L.load()
    md, X, par, lvn = _qf_model(X, Z, raw_ls, raw_os, m, Lam, jitter, 1.0, kernel)
    dev = X.device
    N, D = X.shape
    ws, nbytes = _scratch(lib.tgp_qf_input_grad_var_workspace_bytes(N, D, md.M), dev, workspace_bytes)
    dvar = torch.empty(N, D, dtype=torch.float64, device=dev)
    status = _status(dev)

    def call(jit):
        md.jitter = jit
        L.check(lib.tgp_qf_input_grad_var_f64(md, L.ptr(X), L.ptr(dvar), L.ptr(status), L.ptr(ws), nbytes, L.stream_ptr()),
                "tgp_qf_input_grad_var_f64")
    _laddered(call, status, jitter, info=info, check=check)
    return dvar


def qf_joint_sample(mu, Sigma, eps, jitter=0.0, want_L=False, workspace_bytes=None):
    """Joint draws F0 (S, N) = mu + eps chol(Sigma + jitter I)^T (tgp_qf_joint_sample_f64); eps (S, N) standard normals.
    Returns (F0, L_Sigma or None, status): status[0] is the Cholesky's pivot (no ladder here: see qf_joint_sample_safe)."""
    lib = L.load()
    mu, Sigma, eps = _c(mu.reshape(-1), "mu"), _c(Sigma, "Sigma"), _c(eps, "eps")
    N = mu.numel()
    if Sigma.shape != (N, N) or eps.dim() != 2 or eps.shape[1] != N:
        raise ValueError("qf_joint_sample: mu (N), Sigma (N, N), eps (S, N)")
    S = eps.shape[0]
    dev = mu.device
    ws, nbytes = _scratch(lib.tgp_qf_joint_sample_workspace_bytes(N, S), dev, workspace_bytes)
    F0 = torch.empty(S, N, dtype=torch.float64, device=dev)
    Ls = torch.empty(N, N, dtype=torch.float64, device=dev) if want_L else None
    status = _status(dev)
    L.check(lib.tgp_qf_joint_sample_f64(L.ptr(mu), L.ptr(Sigma), N, float(jitter), L.ptr(eps), S, L.ptr(F0), L.ptr(Ls),
                                        L.ptr(status), L.ptr(ws), nbytes, L.stream_ptr()), "tgp_qf_joint_sample_f64")
    return F0, Ls, status


def qf_joint_sample_safe(mu, Sigma, eps, jitter=None, info=None):
    """qf_joint_sample under psd_safe_cholesky's protocol (dsp/utils.py:222-270): the first factorisation with jitter 0,
    then jitter * 10^i, i = 0..2 (1e-8 in float64 unless given).  Returns F0; `info["jitter"]` = the value that succeeded."""
    F0 = None

    def attempt(jit):
        nonlocal F0
        F0, _, status = qf_joint_sample(mu, Sigma, eps, jit)
        return _failed_pivot(status)
    run_jitter_ladder(attempt, 0.0, jitter_ladder(jitter=jitter), info, what="Sigma")
    return F0


def qf_moments_bwd(X, Z, raw_ls, raw_os, m, Lam, mu_bar, v_bar, jitter=0.0, kernel="scale_rbf", plan=0):
    """Adjoint of qf_moments (tgp_qf_moments_bwd_f64): d(sum mu_bar*mu + v_bar*v)/d{Z, raw_ls, raw_os, m, Lam} as a dict."""
    lib = L.load()
    md, X, par, lvn = _qf_model(X, Z, raw_ls, raw_os, m, Lam, jitter, 0.0, kernel, plan)
    mu_bar, v_bar = _c(mu_bar.reshape(-1), "mu_bar"), _c(v_bar.reshape(-1), "v_bar")
    if mu_bar.numel() != X.shape[0] or v_bar.numel() != X.shape[0]:
        raise ValueError("mu_bar / v_bar must have one entry per row of X")
    dev = X.device
    ws = workspace(X.shape[0], X.shape[1], md.M, 1, 0, 0, 0, dev, md.kernel, plan)
    g = {k: torch.empty_like(t) for k, t in zip(("Z", "raw_ls", "raw_os", "m", "Lam"), par)}
    g["raw_os"] = _os_grad(par[2])
    glvn = torch.empty_like(lvn)
    gs = L.TgpGrads()
    gs.Z, gs.raw_ls, gs.raw_os, gs.m, gs.Lam = (L.ptr(g[k]) for k in ("Z", "raw_ls", "raw_os", "m", "Lam"))
    gs.log_var_noise = L.ptr(glvn)
    status = _status(dev)
    rc = lib.tgp_qf_moments_bwd_f64(md, L.ptr(X), L.ptr(mu_bar), L.ptr(v_bar), gs, L.ptr(status), L.ptr(ws), ws.numel() * 8,
                                    L.stream_ptr())
    L.check(rc, "tgp_qf_moments_bwd_f64")
    return g


class QfMomentsFunction(torch.autograd.Function):
    """(mu, v) = q(f) marginals with autograd in Z, raw_ls, raw_os, m, Lam (what differentiating the reference's
    marginal_variational_qf_parameters, models/sparse_MF_SP.py:274-396, gives outside ELBO()), and in X when X requires grad.
    Forward tgp_qf_moments_f64 (with psd_safe_cholesky's jitter ladder), backward tgp_qf_moments_bwd_f64 at the jitter
    the forward ended with; the gradient in X is g_mu[:, None] * dmu + g_v[:, None] * dv from tgp_qf_input_grad_f64 at that
    jitter (each row's moments depend on that row only), and nothing is launched for it when X does not require grad."""

    @staticmethod
    def forward(ctx, X, Z, raw_ls, raw_os, m, Lam, kernel):
        info = {}
        mu, v = qf_moments(X, Z, raw_ls, raw_os, m, Lam, kernel=kernel, info=info)
        ctx.save_for_backward(X, Z, raw_ls, raw_os, m, Lam)
        ctx.kernel = kernel
        ctx.jitter = info["jitter"]
        return mu, v

    @staticmethod
    def backward(ctx, g_mu, g_v):
        X, Z, raw_ls, raw_os, m, Lam = ctx.saved_tensors
        if g_mu is None:
            g_mu = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
        if g_v is None:
            g_v = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
        g = qf_moments_bwd(X, Z, raw_ls, raw_os, m, Lam, g_mu, g_v, jitter=ctx.jitter, kernel=ctx.kernel)
        g_X = None
        if ctx.needs_input_grad[0]:
            dmu, dv = qf_input_grad(X, Z, raw_ls, raw_os, m, Lam, jitter=ctx.jitter, kernel=ctx.kernel)
            g_X = (g_mu.reshape(-1, 1) * dmu + g_v.reshape(-1, 1) * dv).reshape(X.shape)
        return (g_X, g["Z"].reshape(Z.shape), g["raw_ls"].reshape(raw_ls.shape), g["raw_os"].reshape(raw_os.shape),
                g["m"].reshape(m.shape), g["Lam"].reshape(Lam.shape), None)


class KlFunction(torch.autograd.Function):
    """Whitened KL with autograd in (m, Lam): tgp_kl_whitened_f64 returns the value and both gradients in one launch."""

    @staticmethod
    def forward(ctx, m, Lam):
        kl, gm, gL = kl_whitened(m, Lam)
        ctx.save_for_backward(gm, gL)
        ctx.shapes = (m.shape, Lam.shape)
        return kl.clone()

    @staticmethod
    def backward(ctx, g):
        gm, gL = ctx.saved_tensors
        return (g * gm).reshape(ctx.shapes[0]), (g * gL).reshape(ctx.shapes[1])


# ---------------------------------------------------------------------------------------------------
# unwhitened q(u) (is_whiten=False): the change of variables to the whitened kernels
# ---------------------------------------------------------------------------------------------------
KL_PRIOR_JITTERS = tuple(1e-8 * (10 ** i) for i in range(5))     # add_jitter_MultivariateNormal (dsp/utils.py:200-218), float64


def unwhiten(Z, raw_ls, raw_os, m, L_q, jitter=0.0, check=True, kernel="scale_rbf", info=None, ladder=None,
             workspace_bytes=None):
    """(m_w, Lam_w, L, Linv) with L L^T = K_ZZ + jitter I, m_w = L^-1 m, Lam_w = L^-1 tril(L_q) (tgp_unwhiten_f64): the
    whitened parameters with the same q(f) and KL as q(u) = N(m, L_q L_q^T).  `check`: the status word is read after every
    call (one host sync each; the model's two transforms per ELBO always check, whatever config.status_check says) and a failed
    factorisation goes through run_jitter_ladder with `ladder` (default: psd_safe_cholesky's, as in qf_moments);
    `info["jitter"]` receives the value it ended with.  `workspace_bytes` overrides the size of the workspace handed to the
    library (tests of its refusal)."""
    lib = L.load()
    Z, raw_ls, raw_os, m, L_q = (_c(t, n) for t, n in ((Z, "Z"), (raw_ls, "raw_ls"), (raw_os, "raw_os"), (m, "m"), (L_q, "L_q")))
    _os(raw_os, kernel)
    M, D = Z.shape
    dev = Z.device
    kid = kernel_id(kernel)
    nbytes = lib.tgp_unwhiten_workspace_bytes(M, D)
    if nbytes == 0:              # outside the library's limits: let it say so, before anything is allocated
        L.check(lib.tgp_unwhiten_f64(kid, L.ptr(Z), L.ptr(raw_ls), L.ptr(raw_os), M, D, float(jitter), None, None, None, None,
                                     None, None, None, None, 0, L.stream_ptr()), "tgp_unwhiten_f64")
    if m.numel() != M or tuple(L_q.shape) != (M, M):
        raise ValueError("unwhiten: Z (M, D), m (M), L_q (M, M)")
    ws, nbytes = _scratch(nbytes, dev, workspace_bytes)
    m_w = torch.empty(M, dtype=torch.float64, device=dev)
    Lam_w, Lo, Li = (torch.empty(M, M, dtype=torch.float64, device=dev) for _ in range(3))
    status = _status(dev)

    def call(jit):
        L.check(lib.tgp_unwhiten_f64(kid, L.ptr(Z), L.ptr(raw_ls), L.ptr(raw_os), M, D, float(jit), L.ptr(m), L.ptr(L_q),
                                     L.ptr(m_w), L.ptr(Lam_w), L.ptr(Lo), L.ptr(Li), L.ptr(status), L.ptr(ws), nbytes,
                                     L.stream_ptr()), "tgp_unwhiten_f64")
    _laddered(call, status, jitter, ladder, info, check)
    return m_w, Lam_w, Lo, Li


def unwhiten_bwd(Z, raw_ls, raw_os, Lo, Li, m_w, Lam_w, m_w_bar, Lam_w_bar, kernel="scale_rbf", workspace_bytes=None):
    """Adjoint of `unwhiten` (tgp_unwhiten_bwd_f64): dict(m, L_q, Z, raw_ls, raw_os) for the cotangents of (m_w, Lam_w)."""
    lib = L.load()
    Z, raw_ls, raw_os = _c(Z, "Z"), _c(raw_ls, "raw_ls"), _os(raw_os, kernel)
    Lo, Li, m_w, Lam_w = _c(Lo, "L"), _c(Li, "Linv"), _c(m_w, "m_w"), _c(Lam_w, "Lam_w")
    m_w_bar, Lam_w_bar = _c(m_w_bar.reshape(-1), "m_w_bar"), _c(Lam_w_bar, "Lam_w_bar")
    M, D = Z.shape
    if m_w_bar.numel() != M or tuple(Lam_w_bar.shape) != (M, M):
        raise ValueError("unwhiten_bwd: m_w_bar (M), Lam_w_bar (M, M)")
    dev = Z.device
    ws, nbytes = _scratch(lib.tgp_unwhiten_bwd_workspace_bytes(M, D), dev, workspace_bytes)
    g = {"m": torch.empty(M, dtype=torch.float64, device=dev), "L_q": torch.empty(M, M, dtype=torch.float64, device=dev),
         "Z": torch.empty_like(Z), "raw_ls": torch.empty_like(raw_ls), "raw_os": _os_grad(raw_os)}
    L.check(lib.tgp_unwhiten_bwd_f64(kernel_id(kernel), L.ptr(Z), L.ptr(raw_ls), L.ptr(raw_os), M, D, L.ptr(Lo), L.ptr(Li),
                                     L.ptr(m_w), L.ptr(Lam_w), L.ptr(m_w_bar), L.ptr(Lam_w_bar), L.ptr(g["m"]), L.ptr(g["L_q"]),
                                     L.ptr(g["Z"]), L.ptr(g["raw_ls"]), L.ptr(g["raw_os"]), L.ptr(ws), nbytes, L.stream_ptr()),
            "tgp_unwhiten_bwd_f64")
    return g


class UnwhitenFunction(torch.autograd.Function):
    """(m_w, Lam_w) = unwhiten(Z, raw_ls, raw_os, m, L_q) with autograd in all five.  `jitter`: the value the factorisation
    starts from; `ladder`: the values tried when it fails (None: psd_safe_cholesky's); `info["jitter"]`: what it ended with."""

    @staticmethod
    def forward(ctx, Z, raw_ls, raw_os, m, L_q, kernel, jitter, ladder, info):
        if info is None:
            info = {}
        m_w, Lam_w, Lo, Li = unwhiten(Z.detach(), raw_ls.detach(), raw_os.detach(), m.detach(), L_q.detach(), jitter=jitter,
                                      kernel=kernel, info=info, ladder=ladder)
        ctx.save_for_backward(Z, raw_ls, raw_os, Lo, Li, m_w, Lam_w)
        ctx.kernel = kernel
        ctx.shapes = (Z.shape, raw_ls.shape, raw_os.shape, m.shape, L_q.shape)
        return m_w, Lam_w

    @staticmethod
    def backward(ctx, g_m, g_Lam):
        Z, raw_ls, raw_os, Lo, Li, m_w, Lam_w = ctx.saved_tensors
        if g_m is None:
            g_m = torch.zeros_like(m_w)
        if g_Lam is None:
            g_Lam = torch.zeros_like(Lam_w)
        g = unwhiten_bwd(Z.detach(), raw_ls.detach(), raw_os.detach(), Lo, Li, m_w, Lam_w, g_m, g_Lam, kernel=ctx.kernel)
        return tuple(g[k].reshape(s) for k, s in zip(("Z", "raw_ls", "raw_os", "m", "L_q"), ctx.shapes)) + (None,) * 4


class EllStepFunction(torch.autograd.Function):
    """The likelihood term of the training step alone: ELL = out[1] of elbo_step with kl_scale = 0, so that the gradients are
    those of ELL only, at a caller-chosen jitter (the unwhitened ELBO evaluates the step at the jitter its transform used and
    adds its own KL).  A factorisation that fails at that jitter raises NotPSDError."""

    @staticmethod
    def forward(ctx, X, Y, Z, raw_ls, raw_os, m, Lam, lvn, theta, rowp, cfg):
        kw = dict(_step_kwargs(cfg), kl_scale=0.0)
        want_gy = bool(cfg.get("grad_Y"))
        out, g, status, (mu, _) = elbo_step(X, Y, Z, raw_ls, raw_os, m, Lam, lvn, cfg["N_total"], theta=theta, rowp=rowp,
                                            want_moments=want_gy, **kw)
        cfg["last_status"] = status
        if cfg.get("check_status", True) and raise_for_status(status.cpu()):
            raise NotPSDError("K_MM not positive definite in the step at jitter %g (pivot %d)" % (kw["jitter"], int(status[0])))
        _step_save(ctx, g, (Z, raw_ls, raw_os, m, Lam, lvn, theta, rowp), _gauss_target_adjoint(cfg, Y, lvn, mu) if want_gy else None)
        return out[1].clone()

    @staticmethod
    def backward(ctx, g_ell):
        return _step_backward(ctx, g_ell)


# ---------------------------------------------------------------------------------------------------
# closed-form optimal q(u) of the Gaussian likelihood (the maximiser behind the collapsed bound)
# ---------------------------------------------------------------------------------------------------
def kxxk(X, Z, raw_ls, raw_os, Y=None, kernel="scale_rbf", workspace_bytes=None):
    """(C, b) = (K_ZX K_XZ (M, M), K_ZX y (M) or None) in one pass over the rows of X, K_ZX generated on chip (tgp_kxxk_f64).
    C is exactly symmetric; fixed summation order: two calls give the same bits."""
    lib = L.load()
    X, Z, raw_ls, raw_os = _c(X, "X"), _c(Z, "Z"), _c(raw_ls, "raw_ls"), _os(raw_os, kernel)
    Y = _c(None if Y is None else Y.reshape(-1), "Y")
    N, D = X.shape
    M = Z.shape[0]
    if Z.shape[1] != D or (Y is not None and Y.numel() != N):
        raise ValueError("kxxk: X (N, D), Z (M, D), Y (N)")
    dev = X.device
    ws, nbytes = _scratch(lib.tgp_kxxk_workspace_bytes(N, M), dev, workspace_bytes)
    C = torch.empty(M, M, dtype=torch.float64, device=dev)
    b = torch.empty(M, dtype=torch.float64, device=dev) if Y is not None else None
    L.check(lib.tgp_kxxk_f64(kernel_id(kernel), L.ptr(X), N, L.ptr(Z), M, D, L.ptr(raw_ls), L.ptr(raw_os), L.ptr(Y), L.ptr(C),
                             L.ptr(b), L.ptr(ws), nbytes, L.stream_ptr()), "tgp_kxxk_f64")
    return C, b


def optimal_qu(X, Y, Z, raw_ls, raw_os, lvn, N_total, jitter=0.0, kernel="scale_rbf", info=None, check=True, ladder=None,
               out=None, workspace_bytes=None):
    """(m*, Lam*): the whitened q(u) = N(m*, Lam* Lam*^T) that maximises the Gaussian ELBO of `elbo_step` at these
    hyper-parameters -- the q(u) behind the collapsed bound (tgp_optimal_qu_f64).  With K_ZZ + jitter I = L L^T,
    c = N_total / N and sigma^2 = exp(lvn):  B = I + (c / sigma^2) L^-1 K_ZX K_XZ L^-T,  Lam* Lam*^T = B^-1,
    m* = (c / sigma^2) B^-1 L^-1 K_ZX y.  The factorisation of K runs under psd_safe_cholesky's ladder as in qf_moments;
    `info["jitter"]` receives the value it ended with.  `out` = (m, Lam): written in place.  No autograd."""
    lib = L.load()
    X, Y = _c(X, "X"), _c(Y.reshape(-1), "Y")
    Z, raw_ls, raw_os, lvn = _c(Z, "Z"), _c(raw_ls, "raw_ls"), _c(raw_os, "raw_os"), _c(lvn, "log_var_noise")
    N, D = X.shape
    M = Z.shape[0]
    if Z.shape[1] != D or Y.numel() != N:
        raise ValueError("optimal_qu: X (N, D), Y (N), Z (M, D)")
    dev = X.device
    m, Lam = out if out is not None else (torch.empty(M, dtype=torch.float64, device=dev),
                                          torch.empty(M, M, dtype=torch.float64, device=dev))
    md, _ = _model_struct(X, Z, raw_ls, raw_os, m, Lam, lvn, float(N_total) / float(N), jitter, 1.0, None, None, None, kernel)
    ws, nbytes = _scratch(lib.tgp_optimal_qu_workspace_bytes(N, D, M), dev, workspace_bytes)
    status = _status(dev)

    def attempt(jit):
        md.jitter = jit
        L.check(lib.tgp_optimal_qu_f64(md, L.ptr(X), L.ptr(Y), L.ptr(m), L.ptr(Lam), L.ptr(status), L.ptr(ws), nbytes,
                                       L.stream_ptr()), "tgp_optimal_qu_f64")
        return check and _failed_pivot(status)
    run_jitter_ladder(attempt, jitter, ladder, info=info)
    return m, Lam


# ---------------------------------------------------------------------------------------------------
# natural-gradient step of q(u) for any likelihood: the closed form above with per-row pseudo-observations
# ---------------------------------------------------------------------------------------------------
def kxwxk(X, Z, raw_ls, raw_os, w, r=None, kernel="scale_rbf", workspace_bytes=None):
    """(C, b) = (K_ZX diag(w) K_XZ (M, M), K_ZX r (M) or None) in one pass over the rows of X, K_ZX generated on chip
    (tgp_kxwxk_f64).  w (N) may have any sign.  C is exactly symmetric; fixed summation order: two calls give the same bits, and
    w = 1 gives kxxk's."""
    lib = L.load()
    X, Z, raw_ls, raw_os = _c(X, "X"), _c(Z, "Z"), _c(raw_ls, "raw_ls"), _os(raw_os, kernel)
    w = _c(w.reshape(-1), "w")
    r = _c(None if r is None else r.reshape(-1), "r")
    N, D = X.shape
    M = Z.shape[0]
    if Z.shape[1] != D or w.numel() != N or (r is not None and r.numel() != N):
        raise ValueError("kxwxk: X (N, D), Z (M, D), w (N), r (N)")
    dev = X.device
    ws, nbytes = _scratch(lib.tgp_kxwxk_workspace_bytes(N, M), dev, workspace_bytes)
    C = torch.empty(M, M, dtype=torch.float64, device=dev)
    b = torch.empty(M, dtype=torch.float64, device=dev) if r is not None else None
    L.check(lib.tgp_kxwxk_f64(kernel_id(kernel), L.ptr(X), N, L.ptr(Z), M, D, L.ptr(raw_ls), L.ptr(raw_os), L.ptr(w), L.ptr(r),
                              L.ptr(C), L.ptr(b), L.ptr(ws), nbytes, L.stream_ptr()), "tgp_kxwxk_f64")
    return C, b


def natgrad_qu(X, Z, raw_ls, raw_os, m, Lam, mu, mu_bar, v_bar, rho=1.0, site_floor=0.0, jitter=0.0, kernel="scale_rbf",
               info=None, ladder=None, out=None, check=True, workspace_bytes=None):
    """(m', Lam'): one natural-gradient step of the whitened q(u) = N(m, Lam Lam^T), step size `rho` in (0, 1], from the adjoints
    mu_bar = d(c ELL)/d mu, v_bar = d(c ELL)/d v of the likelihood at the moments of q(f) (mu = a^T m; the adjoints carry c)
    (tgp_natgrad_qu_f64).  Sites lambda = max(-2 v_bar, site_floor) (site_floor None: no floor), r = mu_bar + lambda mu; with
    K_ZZ + jitter I = L L^T:  P' = (1 - rho) (Lam Lam^T)^-1 + rho (I + L^-1 K_ZX diag(lambda) K_XZ L^-T),  Lam' Lam'^T = P'^-1,
    m' = P'^-1 ((1 - rho) (Lam Lam^T)^-1 m + rho L^-1 K_ZX r).  With the Gaussian likelihood's adjoints and rho = 1 it is
    optimal_qu.  The factorisation of K runs under psd_safe_cholesky's ladder as in optimal_qu (`info["jitter"]`); a q(u)-side
    matrix that is not positive definite -- Lam Lam^T, or P' for a likelihood that is not log-concave without a floor -- raises
    NotPSDError naming it (`info["not_pd"]`), no jitter tried, and nothing is written.  `out` = (m, Lam): written in place (they
    may be the inputs).  `check` False: one call, the status is not read (no host sync).  No autograd."""
    lib = L.load()
    X = _c(X, "X")
    Z, raw_ls, raw_os, m, Lam = _c(Z, "Z"), _c(raw_ls, "raw_ls"), _c(raw_os, "raw_os"), _c(m.reshape(-1), "m"), _c(Lam, "Lam")
    mu, mu_bar, v_bar = _c(mu.reshape(-1), "mu"), _c(mu_bar.reshape(-1), "mu_bar"), _c(v_bar.reshape(-1), "v_bar")
    N, D = X.shape
    M = Z.shape[0]
    if Z.shape[1] != D or m.numel() != M or tuple(Lam.shape) != (M, M) or not mu.numel() == mu_bar.numel() == v_bar.numel() == N:
        raise ValueError("natgrad_qu: X (N, D), Z (M, D), m (M), Lam (M, M), mu, mu_bar, v_bar (N)")
    dev = X.device
    m_out, Lam_out = out if out is not None else (torch.empty(M, dtype=torch.float64, device=dev),
                                                  torch.empty(M, M, dtype=torch.float64, device=dev))
    lvn = torch.zeros(1, dtype=torch.float64, device=dev)      # required pointer of the struct, not read
    md, _ = _model_struct(X, Z, raw_ls, raw_os, m, Lam, lvn, 1.0, jitter, 1.0, None, None, None, kernel)
    ws, nbytes = _scratch(lib.tgp_natgrad_qu_workspace_bytes(N, D, M), dev, workspace_bytes)
    status = _status(dev)
    floor = float("nan") if site_floor is None else float(site_floor)
    q_side = [0]

    def attempt(jit):
        md.jitter = jit
        L.check(lib.tgp_natgrad_qu_f64(md, L.ptr(X), L.ptr(mu), L.ptr(mu_bar), L.ptr(v_bar), float(rho), floor, L.ptr(m_out),
                                       L.ptr(Lam_out), L.ptr(status), L.ptr(ws), nbytes, L.stream_ptr()), "tgp_natgrad_qu_f64")
        if not check:
            return False
        st = status.cpu()
        if int(st[0]) != 0 or int(st[3]) != 0 or int(st[1]) == 1:   # K's factorisation (status[1] == 1: its NaN flag): the ladder's
            return raise_for_status(st) and int(st[0])
        q_side[0] = int(st[1])                      # K succeeded: status[1] reports Lam Lam^T (-pivot) or P' (1 + pivot)
        return False
    run_jitter_ladder(attempt, jitter, ladder, info=info)
    if q_side[0] != 0:
        of_p = q_side[0] > 0
        what = "P' = (1 - rho) (Lam Lam^T)^-1 + rho (I + L^-1 K_ZX diag(lambda) K_XZ L^-T)" if of_p else "Lam Lam^T"
        pivot = q_side[0] - 1 if of_p else -q_side[0]
        if info is not None:
            info["not_pd"] = "P'" if of_p else "Lam Lam^T"
        raise NotPSDError("natgrad_qu: %s not positive definite (%s): q(u) is left as it was; more jitter on K_ZZ does not "
                          "help -- use a site floor (site_floor=0.0) or a smaller step"
                          % (what, "pivot %d" % pivot if pivot <= M else "it holds NaNs"))
    return m_out, Lam_out


def _ell_rows(Y, mu, v, lvn, flow, theta, S, rowp=None, scale=1.0, lik=None, df=None):
    """The row-wise ELL launch of a likelihood by its traits, the one its Ell*Function runs (natgrad_step_qu asks by trait, not by
    class): `flow` None -> ell_gauss, else the quadrature launch at `lik` (None: LIK_FLOW).  `df` is the slot for what rides beside
    the noise (noise_slot): the Student-t's degrees of freedom, the ordinal likelihood's bin edges.  `lvn` None: a likelihood
    without a noise parameter.  dict(ell, g_mu, g_v, ...)."""
    if flow is None:
        return dict(zip(("ell", "g_lvn", "g_mu", "g_v"), ell_gauss(Y, mu, v, lvn, scale=scale)))
    if lvn is None:
        return _ell_noiseless(Y, mu, v, flow, theta, S, rowp, scale, lik)
    if df is not None:
        lvn = noise_slot(lvn, lik, df)
    return _ell_quad(Y, mu, v, lvn, flow, theta, S, rowp, scale, L.LIK_FLOW if lik is None else lik)


# ---------------------------------------------------------------------------------------------------
# greedy conditional-variance selection of inducing points (the pivoted Cholesky factorisation of K_XX)
# ---------------------------------------------------------------------------------------------------
def greedy_inducing(X, M, raw_ls, raw_os, kernel="scale_rbf", min_var=1e-8, workspace_bytes=None):
    """(idx (M_eff,) int64, Z (M_eff, D) = X[idx] bit for bit, trace (M_eff + 1,), M_eff): the M rows of X that greedily most reduce
    tr(K_XX - Q_XX), Q_XX = K_XZ K_ZZ^-1 K_ZX, and that trace after every pick (tgp_greedy_inducing_f64).  With d_n = s2 at the
    start, step j picks p_j = argmax_n d_n over the rows not yet picked (ties: the smallest index, so p_0 = 0), stops with
    M_eff = j if d_{p_j} <= min_var, else c_n = (k(x_n, x_{p_j}) - sum_{l<j} C[l,n] C[l,p_j]) / sqrt(d_{p_j}), C[j,n] = c_n,
    d_n <- max(d_n - c_n^2, 0), trace[j+1] = sum of d over the rows not picked; trace[0] = N s2.  M + 1 launches and one host
    read, at the end.  Fixed reduction orders: two calls give the same bits."""
    lib = L.load()
    X, raw_ls, raw_os = _c(X, "X"), _c(raw_ls.reshape(-1), "raw_ls"), _os(raw_os.reshape(-1), kernel)
    if X.dim() != 2 or raw_ls.numel() != X.shape[1]:
        raise ValueError("greedy_inducing: X (N, D), raw_ls (D), raw_os (1)")
    N, D = X.shape
    M = int(M)
    dev = X.device
    ws, nbytes = _scratch(lib.tgp_greedy_inducing_workspace_bytes(N, D, M), dev, workspace_bytes)
    idx = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
    Z = torch.empty(max(M, 1), D, dtype=torch.float64, device=dev)
    trace = torch.empty(max(M, 1) + 1, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.tgp_greedy_inducing_f64(L.ptr(X), N, D, L.ptr(raw_ls), L.ptr(raw_os), kernel_id(kernel), M, float(min_var),
                                        L.ptr(idx), L.ptr(Z), L.ptr(trace), L.ptr(count), L.ptr(ws), nbytes, L.stream_ptr()),
            "tgp_greedy_inducing_f64")
    m_eff = int(count.item())
    return idx[:m_eff].to(torch.int64), Z[:m_eff], trace[:m_eff + 1], m_eff


# ---------------------------------------------------------------------------------------------------
# pathwise posterior function draws (Wilson et al. 2020): Fourier features of the prior + kernel columns at the inducing points
# ---------------------------------------------------------------------------------------------------
def pathwise_coeff(Z, raw_ls, raw_os, m, Lam, omega, W, eps, jitter=0.0, kernel="scale_rbf", check=True, info=None,
                   workspace_bytes=None):
    """coef (2 R2 + M, S) of S pathwise draws of the whitened sparse GP (tgp_pathwise_coeff_f64): rows [0, 2 R2) hold
    amp W[s, j], amp = sqrt(s2 / R2), rows [2 R2, 2 R2 + M) hold nu_s = L^-T (m + Lam eps_s - L^-1 Phi_Z W_s^T) with
    K_ZZ + jitter I = L L^T.  omega (R2, D): frequencies of the unit-length-scale kernel (pathwise.spectral_frequencies);
    W (S, 2 R2), eps (S, M): standard normals.  The factorisation runs under psd_safe_cholesky's ladder as in qf_cov;
    `info["jitter"]` receives the value it ended with.  Fixed summation orders: two calls give the same bits.  No autograd."""
    lib = L.load()
    Z, raw_ls, raw_os = _c(Z, "Z"), _c(raw_ls.reshape(-1), "raw_ls"), _os(raw_os.reshape(-1), kernel)
    m, Lam, omega, W, eps = _c(m.reshape(-1), "m"), _c(Lam, "Lam"), _c(omega, "omega"), _c(W, "W"), _c(eps, "eps")
    M, D = Z.shape
    if omega.dim() != 2 or W.dim() != 2 or eps.dim() != 2:
        raise ValueError("pathwise_coeff: omega (R2, D), W (S, 2 R2), eps (S, M)")
    R2, S = omega.shape[0], W.shape[0]
    if (omega.shape[1] != D or W.shape[1] != 2 * R2 or eps.shape != (S, M) or m.numel() != M or Lam.shape != (M, M)
            or raw_ls.numel() != D):
        raise ValueError("pathwise_coeff: Z (M, D), raw_ls (D), raw_os (1), m (M), Lam (M, M), omega (R2, D), W (S, 2 R2), "
                         "eps (S, M)")
    dev = Z.device
    lvn = torch.zeros(1, dtype=torch.float64, device=dev)
    md, _ = _model_struct(Z, Z, raw_ls, raw_os, m, Lam, lvn, 1.0, jitter, 1.0, None, None, None, kernel)
    ws, nbytes = _scratch(lib.tgp_pathwise_workspace_bytes(1, D, M, R2, S), dev, workspace_bytes)
    coef = torch.empty(max(2 * R2 + M, 1), max(S, 1), dtype=torch.float64, device=dev)
    status = _status(dev)

    def call(jit):
        md.jitter = jit
        L.check(lib.tgp_pathwise_coeff_f64(md, L.ptr(omega), R2, L.ptr(W), L.ptr(eps), S, L.ptr(coef), L.ptr(status), L.ptr(ws),
                                           nbytes, L.stream_ptr()), "tgp_pathwise_coeff_f64")
    _laddered(call, status, jitter, info=info, check=check)
    return coef


def pathwise_eval(X, Z, raw_ls, raw_os, omega, coef, kernel="scale_rbf", batch_rows=None):
    """F0 (S, N): the draws of `coef` (pathwise_coeff) on the rows of X (tgp_pathwise_eval_f64).  A value depends on its row of
    X and on coef only: `batch_rows` evaluates X in pieces of that many rows (bounded operands) and returns the same bits."""
    lib = L.load()
    X, Z, raw_ls, raw_os = _c(X, "X"), _c(Z, "Z"), _c(raw_ls.reshape(-1), "raw_ls"), _os(raw_os.reshape(-1), kernel)
    omega, coef = _c(omega, "omega"), _c(coef, "coef")
    if X.dim() != 2 or Z.dim() != 2 or omega.dim() != 2 or coef.dim() != 2:
        raise ValueError("pathwise_eval: X (N, D), Z (M, D), omega (R2, D), coef (2 R2 + M, S)")
    (N, D), M, R2, S = X.shape, Z.shape[0], omega.shape[0], coef.shape[1]
    if Z.shape[1] != D or omega.shape[1] != D or coef.shape[0] != 2 * R2 + M or raw_ls.numel() != D:
        raise ValueError("pathwise_eval: X (N, D), Z (M, D), raw_ls (D), raw_os (1), omega (R2, D), coef (2 R2 + M, S)")
    if batch_rows is not None and int(batch_rows) < 1:
        raise ValueError("pathwise_eval: batch_rows >= 1")
    kid = kernel_id(kernel)
    dev = X.device

    def piece(Xp):
        n = Xp.shape[0]
        F = torch.empty(max(S, 1), max(n, 1), dtype=torch.float64, device=dev)
        L.check(lib.tgp_pathwise_eval_f64(kid, L.ptr(Xp), n, D, L.ptr(Z), M, L.ptr(raw_ls), L.ptr(raw_os), L.ptr(omega), R2,
                                          L.ptr(coef), S, L.ptr(F), L.stream_ptr()), "tgp_pathwise_eval_f64")
        return F
    if batch_rows is None or int(batch_rows) >= N:
        return piece(X)
    F0 = torch.empty(S, N, dtype=torch.float64, device=dev)
    for a in range(0, N, int(batch_rows)):
        b = min(N, a + int(batch_rows))
        F0[:, a:b] = piece(X[a:b])
    return F0


def pathwise_grad(X, Z, raw_ls, raw_os, omega, coef, kernel="scale_rbf", batch_rows=None):
    """(S, N, D): the gradients d f0_s(x_n) / d x_nd of the draws of `coef` in the rows of X they are evaluated at
    (tgp_pathwise_grad_f64) -- a permuted view of the library's (D, S, N).  An element depends on its row of X, its d and coef
    only: `batch_rows` evaluates X in pieces of that many rows and returns the same bits.  No autograd."""
    lib = L.load()
    X, Z, raw_ls, raw_os = _c(X, "X"), _c(Z, "Z"), _c(raw_ls.reshape(-1), "raw_ls"), _os(raw_os.reshape(-1), kernel)
    omega, coef = _c(omega, "omega"), _c(coef, "coef")
    if X.dim() != 2 or Z.dim() != 2 or omega.dim() != 2 or coef.dim() != 2:
        raise ValueError("pathwise_grad: X (N, D), Z (M, D), omega (R2, D), coef (2 R2 + M, S)")
    (N, D), M, R2, S = X.shape, Z.shape[0], omega.shape[0], coef.shape[1]
    if Z.shape[1] != D or omega.shape[1] != D or coef.shape[0] != 2 * R2 + M or raw_ls.numel() != D:
        raise ValueError("pathwise_grad: X (N, D), Z (M, D), raw_ls (D), raw_os (1), omega (R2, D), coef (2 R2 + M, S)")
    if batch_rows is not None and int(batch_rows) < 1:
        raise ValueError("pathwise_grad: batch_rows >= 1")
    kid = kernel_id(kernel)
    dev = X.device

    def piece(Xp):
        n = Xp.shape[0]
        G = torch.empty(max(D, 1), max(S, 1), max(n, 1), dtype=torch.float64, device=dev)
        L.check(lib.tgp_pathwise_grad_f64(kid, L.ptr(Xp), n, D, L.ptr(Z), M, L.ptr(raw_ls), L.ptr(raw_os), L.ptr(omega), R2,
                                          L.ptr(coef), S, L.ptr(G), L.stream_ptr()), "tgp_pathwise_grad_f64")
        return G
    if batch_rows is None or int(batch_rows) >= N:
        return piece(X).permute(1, 2, 0)
    G = torch.empty(D, S, N, dtype=torch.float64, device=dev)
    for a in range(0, N, int(batch_rows)):
        b = min(N, a + int(batch_rows))
        G[:, :, a:b] = piece(X[a:b])
    return G.permute(1, 2, 0)


# ---------------------------------------------------------------------------------------------------
# mean functions (models/means.py): m(x) = x a + b on the rows of X, and its adjoint
# ---------------------------------------------------------------------------------------------------
def mean_forward(X, a, b=None, alpha=1.0, inp=None, out=None, col=0, one_col=-1):
    """out[:, col] = alpha (X a + b) + inp (tgp_mean_forward_f64); b None counts as 0, inp None as 0; one_col >= 0 also writes 1.0
    to out[:, one_col].  `out` None: a fresh (N,) vector, or with one_col >= 0 a fresh (N, 2) tensor; otherwise a contiguous
    (N,) or (N, ld) tensor of which no other column is touched.  Returns out."""
    lib = L.load()
    X, a, b, inp = _c(X, "X"), _c(a.reshape(-1), "a"), _c(None if b is None else b.reshape(-1), "b"), _c(inp, "in")
    N, D = X.shape
    if a.numel() != D or (b is not None and b.numel() != 1) or (inp is not None and inp.numel() != N):
        raise ValueError("mean_forward: X (N, D), a (D), b (1), in (N)")
    if out is None:
        out = torch.empty((N, 2) if one_col >= 0 else (N,), dtype=torch.float64, device=X.device)
    if out.dtype != torch.float64 or not out.is_contiguous() or out.shape[0] != N or out.dim() > 2:
        raise ValueError("mean_forward: out must be a contiguous float64 (N,) or (N, ld) tensor")
    ld = out.shape[1] if out.dim() == 2 else 1
    L.check(lib.tgp_mean_forward_f64(L.ptr(X), N, D, L.ptr(a), L.ptr(b), float(alpha), L.ptr(inp), L.ptr(out), ld, int(col),
                                     int(one_col), L.stream_ptr()), "tgp_mean_forward_f64")
    return out


def mean_backward(X, g, a=None, col=0, want_b=True, want_X=False):
    """(g_a (D), g_b (1) or None, g_X (N, D) or None) = (X^T g_n, sum g_n, g_n a^T) with g_n = g[n] or g[n, col], read in place
    (tgp_mean_backward_f64).  Fixed summation order: two calls give the same bits."""
    lib = L.load()
    X, g, a = _c(X, "X"), _c(g, "g"), _c(None if a is None else a.reshape(-1), "a")
    N, D = X.shape
    if g.shape[0] != N or g.dim() > 2 or (want_X and (a is None or a.numel() != D)):
        raise ValueError("mean_backward: X (N, D), g (N) or (N, ld), a (D) when g_X is wanted")
    ldg = g.shape[1] if g.dim() == 2 else 1
    dev = X.device
    ws, nbytes = _scratch(lib.tgp_mean_backward_workspace_bytes(N, D), dev)
    g_a = torch.empty(D, dtype=torch.float64, device=dev)
    g_b = torch.empty(1, dtype=torch.float64, device=dev) if want_b else None
    g_X = torch.empty(N, D, dtype=torch.float64, device=dev) if want_X else None
    L.check(lib.tgp_mean_backward_f64(L.ptr(X), N, D, L.ptr(a), L.ptr(g), ldg, int(col), L.ptr(g_a), L.ptr(g_b), L.ptr(g_X),
                                      L.ptr(ws), nbytes, L.stream_ptr()), "tgp_mean_backward_f64")
    return g_a, g_b, g_X


class MeanFunction(torch.autograd.Function):
    """m(X) = X a + b with autograd in a, b and (when it requires grad: the inducing points) X.  `rowp` True: the (N, 2) row
    parameters (1, m(x_n)) of the per-row TGP_FLOW_AFFINE block that turns G(f) into G(f + m(x_n)); the backward reads column 1
    of the incoming gradient in place (column 0, the adjoint of the constant 1, is ignored).  `rowp` False: the (N,) vector
    alpha m(X) + inp (inp without gradient).  b None: no offset (identity mean)."""

    @staticmethod
    def forward(ctx, X, a, b, rowp, alpha, inp):
        Xd, ad = X.detach(), a.detach()
        out = mean_forward(Xd, ad, None if b is None else b.detach(), alpha=1.0 if rowp else alpha, inp=None if rowp else inp,
                           col=1 if rowp else 0, one_col=0 if rowp else -1)
        ctx.save_for_backward(Xd, ad)
        ctx.cfg = (bool(rowp), float(alpha), a.shape, None if b is None else b.shape, X.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        X, a = ctx.saved_tensors
        rowp, alpha, a_shape, b_shape, X_shape = ctx.cfg
        if not rowp and alpha != 1.0:
            g = g * alpha
        g_a, g_b, g_X = mean_backward(X, g.contiguous(), a, col=1 if rowp else 0, want_b=b_shape is not None and ctx.needs_input_grad[2],
                                      want_X=ctx.needs_input_grad[0])
        return (None if g_X is None else g_X.reshape(X_shape), g_a.reshape(a_shape) if ctx.needs_input_grad[1] else None,
                None if g_b is None else g_b.reshape(b_shape), None, None, None)



def kernel_matrix(X1, X2, raw_ls, raw_os, kernel="scale_rbf", jitter=0.0):
    """K(X1, X2) (X2 None: K(X1, X1) + jitter I) for 'scale_rbf' / 'scale_matern32' (tgp_kernel_matrix_f64)."""
    lib = L.load()
    X1, raw_ls, raw_os = _c(X1, "X1"), _c(raw_ls, "raw_ls"), _os(raw_os, kernel)
    X2 = _c(X2, "X2")
    N1, D = X1.shape
    N2 = X2.shape[0] if X2 is not None else N1
    K = torch.empty(N1, N2, dtype=torch.float64, device=X1.device)
    L.check(lib.tgp_kernel_matrix_f64(kernel_id(kernel), L.ptr(X1), N1, L.ptr(X2), N2, D, L.ptr(raw_ls), L.ptr(raw_os),
                                      float(jitter), L.ptr(K), L.stream_ptr()), "tgp_kernel_matrix_f64")
    return K


def kmm(Z, raw_ls, raw_os, jitter=0.0):
    lib = L.load()
    Z, raw_ls, raw_os = _c(Z, "Z"), _c(raw_ls, "raw_ls"), _c(raw_os, "raw_os")
    M, D = Z.shape
    K = torch.empty(M, M, dtype=torch.float64, device=Z.device)
    L.check(lib.tgp_kmm_f64(L.ptr(Z), L.ptr(raw_ls), L.ptr(raw_os), M, D, float(jitter), L.ptr(K), L.stream_ptr()),
            "tgp_kmm_f64")
    return K


def knm(X, Z, raw_ls, raw_os):
    lib = L.load()
    X, Z, raw_ls, raw_os = _c(X, "X"), _c(Z, "Z"), _c(raw_ls, "raw_ls"), _c(raw_os, "raw_os")
    N, D = X.shape
    M = Z.shape[0]
    K = torch.empty(N, M, dtype=torch.float64, device=X.device)
    L.check(lib.tgp_knm_f64(L.ptr(X), L.ptr(Z), L.ptr(raw_ls), L.ptr(raw_os), N, M, D, L.ptr(K), L.stream_ptr()),
            "tgp_knm_f64")
    return K


def cholesky(A, want_inverse=False):
    """Lower Cholesky with LAPACK-style info (no jitter ladder here): returns (L, Linv or None, status)."""
    lib = L.load()
    A = _c(A, "A")
    M = A.shape[0]
    Lo = torch.empty_like(A)
    Li = torch.empty_like(A) if want_inverse else None
    status = _status(A.device)
    nws = lib.tgp_cholesky_workspace_bytes(M)
    ws = torch.empty(nws // 8 + 16, dtype=torch.float64, device=A.device) if nws else None
    L.check(lib.tgp_cholesky_f64(L.ptr(A), M, L.ptr(Lo), L.ptr(Li), L.ptr(status), L.ptr(ws),
                                 ws.numel() * 8 if ws is not None else 0, L.stream_ptr()), "tgp_cholesky_f64")
    return Lo, Li, status


def cholesky_bwd(Lo, Li, L_bar):
    """Adjoint of `cholesky` (tgp_cholesky_bwd_f64): the symmetric A_bar for a factor adjoint L_bar, given L and L^-1."""
    lib = L.load()
    Lo, Li, L_bar = _c(Lo, "L"), _c(Li, "Linv"), _c(L_bar, "L_bar")
    M = Lo.shape[0]
    A_bar = torch.empty_like(Lo)
    ws = torch.empty(lib.tgp_cholesky_bwd_workspace_bytes(M) // 8 + 16, dtype=torch.float64, device=Lo.device)
    L.check(lib.tgp_cholesky_bwd_f64(L.ptr(Lo), L.ptr(Li), L.ptr(L_bar), M, L.ptr(A_bar), L.ptr(ws), ws.numel() * 8,
                                     L.stream_ptr()), "tgp_cholesky_bwd_f64")
    return A_bar


class CholeskyFunction(torch.autograd.Function):
    """L = chol(A) with autograd (torch.cholesky inside psd_safe_cholesky, dsp/utils.py:239, is differentiable in the
    reference): forward tgp_cholesky_f64 (L and L^-1 in one call), backward tgp_cholesky_bwd_f64.  Raises NotPSDError on a
    non-positive pivot (the jitter ladder is psd_safe_cholesky's)."""

    @staticmethod
    def forward(ctx, A):
        Lo, Li, status = cholesky(A, want_inverse=True)
        if raise_for_status(status.cpu()):
            raise NotPSDError("matrix not positive definite (pivot %d)" % int(status[0]))
        ctx.save_for_backward(Lo, Li)
        return Lo

    @staticmethod
    def backward(ctx, g):
        Lo, Li = ctx.saved_tensors
        return cholesky_bwd(Lo, Li, g)


def psd_safe_cholesky(A, jitter=None):
    """dsp/utils.py:222-270 on the GPU: returns (L, A_used).  With autograd on and A requiring grad the factor carries a
    gradient to A (CholeskyFunction), as the reference's torch.cholesky does."""
    diff = torch.is_grad_enabled() and A.requires_grad
    Ax, prev, Lo = A, 0.0, None

    def attempt(jit):
        nonlocal Ax, prev, Lo
        if jit != 0.0:
            if Ax is A:
                Ax = A.clone()          # (a non-leaf copy: the in-place diagonal updates below are autograd-safe)
            Ax.diagonal().add_(jit - prev)     # (from one rung to the next, as the reference's loop adds them)
            prev = jit
        if diff:
            try:
                Lo = CholeskyFunction.apply(Ax)
            except NotPSDError:
                return True
            return False
        Lo, _, status = cholesky(Ax)
        return raise_for_status(status.cpu())
    run_jitter_ladder(attempt, 0.0, jitter_ladder(A.dtype, jitter), what="matrix")
    return Lo, Ax


TRI_A_LOWER, TRI_A_UPPER, TRI_B_LOWER, TRI_B_UPPER, TRI_C_LOWER = 1, 2, 4, 8, 16


def gemm(A, B, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, C=None, tri=0):
    """C = alpha op(A) op(B) + beta C on the float64 matrix cores (tgp_gemm_f64); m, n multiples of 128, k of 16.

    The building block of the M > 128 path: stands in for the reference's torch.bmm / triangular_solve on
    (M,M)x(M,N) operands (models/sparse_MF_SP.py:354,376-382).  `tri` declares triangular operands (TRI_*)."""
    A, B = _c(A, "A"), _c(B, "B")
    m, k = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    k2, n = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if k != k2:
        raise L.TgpError("gemm: inner dimensions differ (%d vs %d)" % (k, k2))
    if C is None:
        C = torch.zeros(m, n, dtype=torch.float64, device=A.device)
    L.check(L.load().tgp_gemm_f64(int(trans_a), int(trans_b), int(tri), m, n, k, float(alpha), L.ptr(A), A.shape[1],
                                  L.ptr(B), B.shape[1], float(beta), L.ptr(C), C.shape[1], L.stream_ptr()),
            "tgp_gemm_f64")
    return C


def _rows(t, name):
    """(pointer, leading dimension) of a 2-D float64 device tensor whose rows are contiguous: a view into a wider buffer
    keeps its stride as the leading dimension."""
    if t is None:
        return None, 0
    if not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2 or t.stride(1) != 1:
        raise L.TgpError("gemm: %s must be a 2-D float64 device tensor with contiguous rows" % name)
    return L.C.c_void_p(t.data_ptr()), t.stride(0)


def gemm_desc(A, B, C, trans_a=False, trans_b=False, tri=0, alpha=1.0, beta=0.0, a_mul=None, k_scale=None, add=None, gamma=0.0,
              col_scale=None, row_scale=None, rowv=None, colv=None, ksplit=1, xcd=0, scratch=None):
    """The tgp_gemm_ex descriptor of C = epilogue(alpha (op(A) o a_mul diag(k_scale)) op(B)) (include/tgp_hip.h).  A, B, C,
    a_mul and add may be row-strided views; with ksplit > 1 and no scratch, C is (ksplit, m, n): slab z at C[z]."""
    d = L.TgpGemmEx()
    d.A, d.lda = _rows(A, "A")
    d.B, d.ldb = _rows(B, "B")
    m, k = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    k2, n = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if k != k2:
        raise L.TgpError("gemm: inner dimensions differ (%d vs %d)" % (k, k2))
    if C.dim() == 3:
        if C.shape[0] != ksplit or scratch is not None:
            raise L.TgpError("gemm: a 3-D C holds the ksplit slabs of a product without scratch")
        d.cz, C = C.stride(0), C[0]
    if tuple(C.shape) != (m, n):
        raise L.TgpError("gemm: C is %s, the product %d x %d" % (tuple(C.shape), m, n))
    d.C, d.ldc = _rows(C, "C")
    if a_mul is not None:
        d.a_mul, ldm = _rows(a_mul, "a_mul")
        if tuple(a_mul.shape) != tuple(A.shape) or ldm != d.lda:
            raise L.TgpError("gemm: a_mul must have A's shape and leading dimension")
    d.add, d.ldadd = _rows(add, "add")
    for name, v, length in (("k_scale", k_scale, k), ("col_scale", col_scale, n), ("row_scale", row_scale, m), ("rowv", rowv, m),
                            ("colv", colv, n)):
        if v is not None:
            if v.numel() != length:
                raise L.TgpError("gemm: %s has %d entries, not %d" % (name, v.numel(), length))
            setattr(d, name, L.ptr(v))
    d.trans_a, d.trans_b, d.tri, d.m, d.n, d.k = int(bool(trans_a)), int(bool(trans_b)), int(tri), m, n, k
    d.alpha, d.beta, d.gamma, d.ksplit, d.xcd = float(alpha), float(beta), float(gamma), int(ksplit), int(xcd)
    if scratch is not None:
        d.scratch, d.scratch_doubles = L.ptr(scratch), scratch.numel()
    return d


def gemm_ex(A, B, C, **kw):
    """tgp_gemm_ex_f64 on gemm_desc's arguments: the tiled float64 GEMM with its operand modifiers, epilogue terms, split-K
    slabs (or, with `scratch`, the split-K + reduction route of the step's M x M products) and workgroup orders."""
    L.check(L.load().tgp_gemm_ex_f64(L.C.byref(gemm_desc(A, B, C, **kw)), L.stream_ptr()), "tgp_gemm_ex_f64")
    return C


def gemm_pair_ex(a, b):
    """tgp_gemm_pair_ex_f64: two gemm_desc products (a with op(B) transposed, b plain) in one launch where they qualify."""
    L.check(L.load().tgp_gemm_pair_ex_f64(L.C.byref(a), L.C.byref(b), L.stream_ptr()), "tgp_gemm_pair_ex_f64")


def gemm_route(m, n, k, trans_a=False, trans_b=False, tri=0, beta=0.0, ksplit=1, xcd=0, mod=False):
    """tgp_gemm_route: the kernel and workgroup order (lib.GEMM_ROUTE_*) the launcher gives a product of this shape, or its
    refusal code.  Host only: no device, no operand (mod: as if a_mul / k_scale were given)."""
    d = L.TgpGemmEx()
    d.trans_a, d.trans_b, d.tri, d.m, d.n, d.k = int(bool(trans_a)), int(bool(trans_b)), int(tri), m, n, k
    d.lda, d.ldb, d.ldc = (m if trans_a else k), (k if trans_b else n), n
    d.alpha, d.beta, d.ksplit, d.xcd = 1.0, float(beta), int(ksplit), int(xcd)
    d.cz = m * n
    if mod:
        d.k_scale = L.C.c_void_p(16)        # never dereferenced
    return L.load().tgp_gemm_route(L.C.byref(d))


def kl_whitened(m, Lam):
    """Whitened KL and gradients (models/sparse_MF_SP.py:406-431): returns (KL 0-d, g_m, g_Lam)."""
    lib = L.load()
    m, Lam = _c(m, "m"), _c(Lam, "Lam")
    out = torch.empty(1, dtype=torch.float64, device=m.device)
    gm, gL = torch.empty_like(m), torch.empty_like(Lam)
    L.check(lib.tgp_kl_whitened_f64(L.ptr(m), L.ptr(Lam), m.numel(), L.ptr(out), L.ptr(gm), L.ptr(gL),
                                    L.stream_ptr()), "tgp_kl_whitened_f64")
    return out[0], gm, gL


def ell_gauss(Y, mu, v, lvn, scale=1.0):
    """SVGP expected log-likelihood (likelihoods/GaussianLinearMean.py:60-87): (ELL, dELL/dlvn, g_mu, g_v)."""
    lib = L.load()
    Y, mu, v, lvn = _c(Y.reshape(-1), "Y"), _c(mu, "mu"), _c(v, "v"), _c(lvn, "lvn")
    N = Y.numel()
    ws = torch.empty(lib.tgp_ell_workspace_bytes(N, 0, 0) // 8 + 16, dtype=torch.float64, device=Y.device)
    out = torch.empty(2, dtype=torch.float64, device=Y.device)
    gmu, gv = torch.empty_like(mu), torch.empty_like(v)
    L.check(lib.tgp_ell_gauss_f64(L.ptr(Y), L.ptr(mu), L.ptr(v), N, L.ptr(lvn), float(scale), L.ptr(out), L.ptr(gmu),
                                  L.ptr(gv), L.ptr(ws), ws.numel() * 8, L.stream_ptr()), "tgp_ell_gauss_f64")
    return out[0], out[1], gmu, gv


def _flow_model(N, S, flow, theta, lvn, dev, scale=1.0, lik=None):
    """(TgpModel, tensors to keep referenced until the call returns) for the row-wise likelihood kernels, which read no GP
    field.  `flow` None: the Gaussian likelihood; else `lik` (None: LIK_FLOW) through `flow` at S Gauss-Hermite nodes."""
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = N, 1, 1, 1, L.LIK_GAUSS
    md.scale, md.jitter, md.kl_scale = float(scale), 0.0, 1.0
    md.log_var_noise = L.ptr(lvn)
    if flow is None:
        return md, ()
    md.S, md.lik = int(S), L.LIK_FLOW if lik is None else int(lik)
    md.nblk, md.P, md.RP = flow.nblk, flow.P, flow.RP
    xs, wn = gauss_hermite(S, dev)
    md.program, md.xs, md.wn = flow.program_ptr, L.ptr(xs), L.ptr(wn)
    md.theta = L.ptr(theta) if flow.P > 0 else None
    return md, (xs, wn)


def _ell_quad(Y, mu, v, lvn, flow, theta, S, rowp, scale, lik, entry="tgp_ell_flow_f64", rows=None):
    """One quadrature ELL launch, `entry` at likelihood `lik`: dict(ell, g_lvn, g_mu, g_v, g_theta, g_rowp).  `rows`: mu and v
    hold the moments of that many latent GPs, shape (rows, N), and so do g_mu and g_v (None: one GP, shape (N,))."""
    lib = L.load()
    Y, mu, v, lvn = _c(Y.reshape(-1), "Y"), _c(mu, "mu"), _c(v, "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    dev, N = Y.device, Y.numel()
    if rows is not None and (tuple(mu.shape) != (rows, N) or tuple(v.shape) != (rows, N)):
        raise L.TgpError("%s: mu and v must be (%d, N) = (%d, %d), got %s and %s"
                         % (entry[4:-4], rows, rows, N, tuple(mu.shape), tuple(v.shape)))
    md, keep = _flow_model(N, S, flow, theta, lvn, dev, scale, lik=lik)
    ws = torch.empty(lib.tgp_ell_workspace_bytes(N, flow.P, md.RP) // 8 + 16, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    gmu, gv = torch.empty_like(mu), torch.empty_like(v)
    gth = torch.empty(max(flow.P, 1), dtype=torch.float64, device=dev)
    grp = torch.empty_like(rowp) if rowp is not None else None
    L.check(getattr(lib, entry)(md, L.ptr(Y), L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(out), L.ptr(gmu), L.ptr(gv),
                                L.ptr(gth), L.ptr(grp), L.ptr(ws), ws.numel() * 8, L.stream_ptr()), entry)
    return {"ell": out[0], "g_lvn": out[1], "g_mu": gmu, "g_v": gv, "g_theta": gth[:flow.P], "g_rowp": grp}


def ell_flow(Y, mu, v, lvn, flow, theta, S, rowp=None, scale=1.0):
    """TGP quadrature ELL with gradients (likelihoods/GaussianNonLinearMean.py:64-150).
    Returns dict(ell, g_lvn, g_mu, g_v, g_theta, g_rowp)."""
    return _ell_quad(Y, mu, v, lvn, flow, theta, S, rowp, scale, L.LIK_FLOW)


def ell_bernoulli(Y, mu, v, flow, theta, S, rowp=None, scale=1.0):
    """Bernoulli (probit) quadrature ELL with gradients (likelihoods/Bernoulli.py expected_log_prob; tgp_ell_flow_f64 with
    TGP_LIK_BERNOULLI).  Returns dict(ell, g_mu, g_v, g_theta, g_rowp)."""
    return _ell_noiseless(Y, mu, v, flow, theta, S, rowp, scale, L.LIK_BERNOULLI)


def ell_poisson(Y, mu, v, flow, theta, S, rowp=None, scale=1.0):
    """Poisson quadrature ELL with gradients, the flow as the log-rate: scale sum_n E_q(f0)[y_n G(f0) - exp(G(f0))] -
    lgamma(y_n + 1) (tgp_ell_flow_f64 with TGP_LIK_POISSON).  Returns dict(ell, g_mu, g_v, g_theta, g_rowp)."""
    return _ell_noiseless(Y, mu, v, flow, theta, S, rowp, scale, L.LIK_POISSON)


def _ell_noiseless(Y, mu, v, flow, theta, S, rowp, scale, lik):
    """_ell_quad for a likelihood without a noise parameter (LIK_BERNOULLI, LIK_POISSON)."""
    lvn = torch.zeros(1, dtype=torch.float64, device=Y.device)      # required pointer, not read
    res = _ell_quad(Y, mu, v, lvn, flow, theta, S, rowp, scale, lik)
    del res["g_lvn"]
    return res


def ell_student(Y, mu, v, lvn, df, flow, theta, S, rowp=None, scale=1.0):
    """Student-t quadrature ELL with gradients: scale sum_n E_q(f0)[log StudentT(y_n | df, loc = G(f0), scale = sigma)], lvn =
    log sigma^2 (tgp_ell_flow_f64 with TGP_LIK_STUDENT).  Returns dict(ell, g_lvn, g_mu, g_v, g_theta, g_rowp); g_lvn =
    dELL/dlvn, `df` has no gradient."""
    return _ell_quad(Y, mu, v, student_noise(lvn, df), flow, theta, S, rowp, scale, L.LIK_STUDENT)


def ell_negbin(Y, mu, v, lvn, flow, theta, S, rowp=None, scale=1.0):
    """Negative-binomial quadrature ELL with gradients, the flow as the log-mean: scale sum_n E_q(f0)[log NB(y_n | mean =
    exp(G(f0)), dispersion r)], lvn = log r, 1e-3 <= r <= 1e3 (tgp_ell_flow_f64 with TGP_LIK_NEGBIN).  Returns dict(ell, g_lvn,
    g_mu, g_v, g_theta, g_rowp); g_lvn = dELL/dlvn."""
    return _ell_quad(Y, mu, v, lvn, flow, theta, S, rowp, scale, L.LIK_NEGBIN)


def ell_gamma(Y, mu, v, log_shape, flow, theta, S, rowp=None, scale=1.0):
    """Gamma quadrature ELL with gradients, the flow as the log-mean: scale sum_n E_q(f0)[log Gamma(y_n | shape a, rate
    a exp(-G(f0)))], log_shape = log a, 0.1 <= a <= 1e3, Y > 0 (tgp_ell_flow_f64 with TGP_LIK_GAMMA).  Returns dict(ell, g_lvn,
    g_mu, g_v, g_theta, g_rowp); g_lvn = dELL/dlog_shape."""
    return _ell_quad(Y, mu, v, log_shape, flow, theta, S, rowp, scale, L.LIK_GAMMA)


def ell_beta(Y, mu, v, log_precision, flow, theta, S, rowp=None, scale=1.0):
    """Beta quadrature ELL with gradients, the flow as the log-odds of the mean: scale sum_n E_q(f0)[log Beta(y_n | mu phi,
    (1 - mu) phi)], mu = sigmoid(G(f0)), log_precision = log phi, 0.5 <= phi <= 1e3, 0 < Y < 1 (tgp_ell_flow_f64 with
    TGP_LIK_BETA).  Returns dict(ell, g_lvn, g_mu, g_v, g_theta, g_rowp); g_lvn = dELL/dlog_precision."""
    return _ell_quad(Y, mu, v, log_precision, flow, theta, S, rowp, scale, L.LIK_BETA)


def ell_ordinal(Y, mu, v, lvn, edges, flow, theta, S, rowp=None, scale=1.0):
    """Ordinal (cumulative-probit) quadrature ELL with gradients: scale sum_n E_q(f0)[log(Phi((b_{y_n + 1} - G(f0)) / sigma) -
    Phi((b_{y_n} - G(f0)) / sigma))], Y the classes 0 .. K-1, lvn = log sigma^2, `edges` the K - 1 fixed bin edges b_1 < .. < b_{K-1}
    (tgp_ell_flow_f64 with TGP_LIK_ORDINAL).  Returns dict(ell, g_lvn, g_mu, g_v, g_theta, g_rowp); g_lvn = dELL/dlvn, the edges
    have no gradient."""
    return _ell_quad(Y, mu, v, ordinal_noise(lvn, edges), flow, theta, S, rowp, scale, L.LIK_ORDINAL)


def ell_hetero(Y, mu, v, lvn, flow, theta, S, rowp=None, scale=1.0):
    """Heteroscedastic Gaussian ELL with gradients, y ~ N(G(f), exp(lvn + h)): mu, v of shape (2, N), row 0 the moments of q(f),
    row 1 those of the log-noise GP q(h), which integrates out in closed form (tgp_ell_hetero_f64, one launch).  `flow` a
    FlowSpec (an empty one for the identity flow).  Returns ell_student's dict(ell, g_lvn, g_mu, g_v, g_theta, g_rowp) -- g_mu,
    g_v the row-0 adjoints, g_lvn = dELL/dlvn -- plus g_mu_h, g_v_h, the row-1 adjoints (views of the same (2, N) buffers)."""
    if flow is None:
        raise L.TgpError("the heteroscedastic likelihood needs a FlowSpec (an empty one for the identity flow)")
    res = _ell_quad(Y, mu, v, lvn, flow, theta, S, rowp, scale, L.LIK_HETERO, entry="tgp_ell_hetero_f64", rows=2)
    gmu, gv = res["g_mu"], res["g_v"]
    res.update(g_mu=gmu[0], g_v=gv[0], g_mu_h=gmu[1], g_v_h=gv[1])
    return res


def predict_hetero(mu, v, lvn, flow, theta=None, S=None, rowp=None, Y=None, Y_std=1.0, want_moments=True):
    """The heteroscedastic predictive from the moments of both latent GPs (mu, v of shape (2, N); tgp_predict_hetero_f64, one
    launch): (m1, m2, logp) in standardised units, m2 with the mean noise exp(lvn + mu_h + v_h / 2), logp = the exact log density
    of the raw target under the S x S product rule, constant and -log Y_std included (None without Y)."""
    lib = L.load()
    if flow is None:
        raise L.TgpError("the heteroscedastic likelihood needs a FlowSpec (an empty one for the identity flow)")
    mu, v, lvn = _c(mu, "mu"), _c(v, "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    if mu.dim() != 2 or mu.shape[0] != 2 or v.shape != mu.shape:
        raise L.TgpError("predict_hetero: mu and v must be (2, N), got %s and %s" % (tuple(mu.shape), tuple(v.shape)))
    dev, N = mu.device, mu.shape[1]
    md, keep = _flow_model(N, S, flow, theta, lvn, dev, lik=L.LIK_HETERO)
    m1, m2 = (torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev)) \
        if want_moments else (None, None)
    logp = torch.empty(N, dtype=torch.float64, device=dev) if Y is not None else None
    Yc = _c(Y.reshape(-1), "Y") if Y is not None else None
    L.check(lib.tgp_predict_hetero_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(Yc), float(Y_std), L.ptr(m1), L.ptr(m2),
                                       L.ptr(logp), L.stream_ptr()), "tgp_predict_hetero_f64")
    return m1, m2, logp


def ell_warp(Y, mu, v, lvn, flow, theta, scale=1.0, want_t=False):
    """Warped-GP ELL with gradients (likelihoods/WarpedGaussianLinearMean.py:65-85; tgp_ell_warp_f64, one launch).
    Returns dict(ell, g_lvn, logdet, g_mu, g_v, g_theta, t)."""
    lib = L.load()
    Y, mu, v, lvn = _c(Y.reshape(-1), "Y"), _c(mu, "mu"), _c(v, "v"), _c(lvn, "lvn")
    theta = _c(theta, "theta")
    dev, N = Y.device, Y.numel()
    if flow.RP:
        raise L.TgpError("a warped likelihood takes shared flow parameters only (no input-dependent blocks)")
    md, keep = _flow_model(N, 1, flow, theta, lvn, dev, scale, lik=L.LIK_WARPED)
    ws = torch.empty(lib.tgp_ell_warp_workspace_bytes(N, flow.P) // 8 + 16, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    gmu, gv = torch.empty_like(mu), torch.empty_like(v)
    gth = torch.empty(max(flow.P, 1), dtype=torch.float64, device=dev)
    t = torch.empty_like(Y) if want_t else None
    L.check(lib.tgp_ell_warp_f64(md, L.ptr(Y), L.ptr(mu), L.ptr(v), L.ptr(out), L.ptr(gmu), L.ptr(gv), L.ptr(gth), L.ptr(t),
                                 L.ptr(ws), ws.numel() * 8, L.stream_ptr()), "tgp_ell_warp_f64")
    return {"ell": out[0], "g_lvn": out[1], "logdet": out[2], "g_mu": gmu, "g_v": gv, "g_theta": gth[:flow.P], "t": t}


class EllFunction(torch.autograd.Function):
    """The one autograd wrapper of the row-wise ELL launches.  forward(Y, mu, v, lvn | None, theta | None, rowp | None, ell):
    `ell(Y, mu, v, lvn, theta, rowp)` is the launch -- an ell_* of this module bound to its extras (flow, S, lik, df, scale) --
    and gets the tensors detached; of its dict(ell, g_mu, g_v, g_lvn, g_theta, g_rowp) the gradients of the inputs that are
    present are kept for the backward.  Value and every gradient come from that one launch."""

    GRADS = (None, "g_mu", "g_v", "g_lvn", "g_theta", "g_rowp")     # by input, in forward's order (Y has none)

    @staticmethod
    def forward(ctx, Y, mu, v, lvn, theta, rowp, ell):
        ins = (Y, mu, v, lvn, theta, rowp)
        res = ell(*(t.detach() if t is not None else None for t in ins))
        ctx.has = tuple(k is not None and t is not None for k, t in zip(EllFunction.GRADS, ins))
        ctx.save_for_backward(*(res[k] for k, has in zip(EllFunction.GRADS, ctx.has) if has))
        ctx.lvn_shape = lvn.shape if lvn is not None else None
        return res["ell"].reshape(1)

    @staticmethod
    def backward(ctx, g):
        g, saved = g.reshape(()), iter(ctx.saved_tensors)
        grads = [g * next(saved) if has else None for has in ctx.has]
        if grads[3] is not None:
            grads[3] = grads[3].reshape(ctx.lvn_shape)
        return (*grads, None)


class _EllOf:
    """A public Ell*Function name: `apply` keeps that name's own argument list and binds it to EllFunction -- `bind(*args)`
    gives EllFunction's (Y, mu, v, lvn, theta, rowp, ell)."""

    def __init__(self, bind, doc):
        self.bind, self.__doc__ = bind, doc

    def apply(self, *args):
        return EllFunction.apply(*self.bind(*args))


def _gauss_dict(Y, mu, v, lvn, theta, rowp):
    return dict(zip(("ell", "g_lvn", "g_mu", "g_v"), ell_gauss(Y, mu, v, lvn)))


def _hetero_pairs(res):
    """ell_hetero's dict with g_mu, g_v as the (2, N) pairs the (2, N) inputs take."""
    return dict(res, g_mu=torch.stack((res["g_mu"], res["g_mu_h"])), g_v=torch.stack((res["g_v"], res["g_v_h"])))


def _ell_noiseless_of(lik):
    return lambda Y, mu, v, theta, rowp, flow, S: (
        Y, mu, v, None, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: _ell_noiseless(Y, mu, v, flow, theta, S, rowp, 1.0, lik))


EllGaussFunction = _EllOf(
    lambda Y, mu, v, lvn: (Y, mu, v, lvn, None, None, _gauss_dict),
    """apply(Y, mu, v, lvn): ELL = GaussianLinearMean.expected_log_prob (likelihoods/GaussianLinearMean.py:60-87) with autograd
    in (mu, v, log_var_noise) -- the reference's method is plain torch code, differentiable wherever it is called.""")
EllFlowFunction = _EllOf(
    lambda Y, mu, v, lvn, theta, rowp, flow, S: (
        Y, mu, v, lvn, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: ell_flow(Y, mu, v, lvn, flow, theta, S, rowp)),
    """apply(Y, mu, v, lvn, theta, rowp, flow, S): ELL = GaussianNonLinearMean.expected_log_prob
    (likelihoods/GaussianNonLinearMean.py:64-150) with autograd in (mu, v, log_var_noise, theta, rowp).""")
EllBernoulliFunction = _EllOf(
    _ell_noiseless_of(L.LIK_BERNOULLI),
    """apply(Y, mu, v, theta, rowp, flow, S): ELL = Bernoulli.expected_log_prob (likelihoods/Bernoulli.py) with autograd in
    (mu, v, theta, rowp).""")
EllPoissonFunction = _EllOf(
    _ell_noiseless_of(L.LIK_POISSON),
    """apply(Y, mu, v, theta, rowp, flow, S): ELL of the Poisson likelihood with autograd in (mu, v, theta, rowp).""")
EllStudentFunction = _EllOf(
    lambda Y, mu, v, lvn, df, theta, rowp, flow, S: (
        Y, mu, v, lvn, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: ell_student(Y, mu, v, lvn, df, flow, theta, S, rowp)),
    """apply(Y, mu, v, lvn, df, theta, rowp, flow, S): ELL of the Student-t likelihood with autograd in (mu, v, log_var_noise,
    theta, rowp) and none in `df`.""")
EllNegBinFunction = _EllOf(
    lambda Y, mu, v, lvn, theta, rowp, flow, S: (
        Y, mu, v, lvn, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: ell_negbin(Y, mu, v, lvn, flow, theta, S, rowp)),
    """apply(Y, mu, v, lvn, theta, rowp, flow, S): ELL of the negative-binomial likelihood with autograd in (mu, v, the log
    dispersion, theta, rowp).""")
EllGammaFunction = _EllOf(
    lambda Y, mu, v, lvn, theta, rowp, flow, S: (
        Y, mu, v, lvn, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: ell_gamma(Y, mu, v, lvn, flow, theta, S, rowp)),
    """apply(Y, mu, v, log_shape, theta, rowp, flow, S): ELL of the Gamma likelihood with autograd in (mu, v, the log shape,
    theta, rowp).""")
EllBetaFunction = _EllOf(
    lambda Y, mu, v, lvn, theta, rowp, flow, S: (
        Y, mu, v, lvn, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: ell_beta(Y, mu, v, lvn, flow, theta, S, rowp)),
    """apply(Y, mu, v, log_precision, theta, rowp, flow, S): ELL of the Beta likelihood with autograd in (mu, v, the log
    precision, theta, rowp).""")
EllOrdinalFunction = _EllOf(
    lambda Y, mu, v, lvn, edges, theta, rowp, flow, S: (
        Y, mu, v, lvn, theta, rowp, lambda Y, mu, v, lvn, theta, rowp: ell_ordinal(Y, mu, v, lvn, edges, flow, theta, S, rowp)),
    """apply(Y, mu, v, lvn, edges, theta, rowp, flow, S): ELL of the ordinal likelihood with autograd in (mu, v, log_var_noise,
    theta, rowp) and none in the bin edges.""")
EllHeteroFunction = _EllOf(
    lambda Y, mu, v, lvn, theta, rowp, flow, S, scale: (
        Y, mu, v, lvn, theta, rowp,
        lambda Y, mu, v, lvn, theta, rowp: _hetero_pairs(ell_hetero(Y, mu, v, lvn, flow, theta, S, rowp, scale=scale))),
    """apply(Y, mu, v, lvn, theta, rowp, flow, S, scale): ELL of the heteroscedastic Gaussian likelihood with autograd in (mu, v,
    log_var_noise, theta, rowp); mu, v (2, N).  `scale` multiplies value and gradients inside the launch.""")
EllWarpFunction = _EllOf(
    lambda Y, mu, v, lvn, theta, flow: (
        Y, mu, v, lvn, theta, None, lambda Y, mu, v, lvn, theta, rowp: ell_warp(Y, mu, v, lvn, flow, theta)),
    """apply(Y, mu, v, lvn, theta, flow): ELL = WarpedGaussianLinearMean.expected_log_prob with autograd in (mu, v, log_var_noise,
    theta).""")


class SoftmaxSpec:
    """The C flow programs of a multi-class model, one after the other (tgp_softmax.program / blk_off / theta_off): block
    offsets stay relative to each class's own parameters; theta is the concatenation of the classes' shared scalars."""

    def __init__(self, flows):
        self.C = len(flows)
        if any(f.RP for f in flows):
            raise L.TgpError("the multi-class likelihood takes shared flow parameters only (no input-dependent blocks)")
        self.flows = list(flows)
        blocks = [b for f in flows for b in f.blocks]
        self.nblk = len(blocks)
        self.P = sum(f.P for f in flows)
        self.program = np.ascontiguousarray(np.array(blocks if blocks else [(0, 0, 0, 0)], dtype=np.int32))
        self.blk_off = np.ascontiguousarray(np.cumsum([0] + [f.nblk for f in flows]), dtype=np.int32)
        self.theta_off = np.ascontiguousarray(np.cumsum([0] + [f.P for f in flows]), dtype=np.int32)


def _softmax_desc(spec, N, S, theta, scale=1.0, seed=0, step_dev=None, row0=0):
    import ctypes
    d = L.TgpSoftmax()
    d.N, d.C, d.S = int(N), int(spec.C), int(S)
    d.program = ctypes.c_void_p(spec.program.ctypes.data) if spec.nblk else None
    d.blk_off = ctypes.c_void_p(spec.blk_off.ctypes.data)
    d.theta_off = ctypes.c_void_p(spec.theta_off.ctypes.data)
    d.theta = L.ptr(theta) if spec.P > 0 else None
    d.scale, d.seed, d.row0 = float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0)
    d.step_dev = L.ptr(step_dev)
    return d


def _softmax_args(Y, mu, v, spec, theta, eps, S):
    mu, v, theta, eps = _c(mu, "mu"), _c(v, "v"), _c(theta, "theta"), _c(eps, "eps")
    if mu.dim() != 2 or mu.shape[0] != spec.C or v.shape != mu.shape:
        raise ValueError("mu, v must be (C, N) with C = %d" % spec.C)
    N = mu.shape[1]
    if eps is not None and tuple(eps.shape) != (int(S), spec.C, N):
        raise ValueError("eps must be (S, C, N) = (%d, %d, %d), got %s" % (S, spec.C, N, tuple(eps.shape)))
    if Y is not None:
        Y = _c(Y.reshape(-1).to(torch.float64), "Y")
        if Y.numel() != N:
            raise ValueError("Y must have one label per row")
    if spec.P > 0 and (theta is None or theta.numel() != spec.P):
        raise ValueError("theta must hold the %d shared scalars of the C programs" % spec.P)
    return Y, mu, v, theta, eps, N


def ell_softmax(Y, mu, v, spec, theta, S, eps=None, seed=0, step_dev=None, row0=0, scale=1.0, want_grads=True):
    """Multi-class ELL (likelihoods/MulticlassCategorical.py:51-105) and its gradients in one launch (tgp_ell_softmax_f64).
    mu, v (C,N); Y (N) class indices; eps (S,C,N) standard normals or None: counter-based draws of (seed, step_dev, row0).
    Returns dict(ell, g_mu, g_v, g_theta)."""
    lib = L.load()
    Y, mu, v, theta, eps, N = _softmax_args(Y, mu, v, spec, theta, eps, S)
    dev = mu.device
    d = _softmax_desc(spec, N, S, theta, scale, seed, step_dev, row0)
    ws = torch.empty(lib.tgp_ell_softmax_workspace_bytes(N, spec.P) // 8 + 16, dtype=torch.float64, device=dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    gmu = gv = gth = None
    if want_grads:
        gmu, gv = torch.empty_like(mu), torch.empty_like(v)
        gth = torch.empty(max(spec.P, 1), dtype=torch.float64, device=dev)
    L.check(lib.tgp_ell_softmax_f64(d, L.ptr(Y), L.ptr(mu), L.ptr(v), L.ptr(eps), L.ptr(out), L.ptr(gmu), L.ptr(gv), L.ptr(gth),
                                    L.ptr(ws), ws.numel() * 8, L.stream_ptr()), "tgp_ell_softmax_f64")
    return {"ell": out[0], "g_mu": gmu, "g_v": gv, "g_theta": gth[:spec.P] if gth is not None else None}


def mc_normals(S, C, N, seed=0, step_dev=None, row0=0, device="cuda"):
    """The (S,C,N) standard normals the counter mode of ell_softmax / predict_softmax draws (tgp_mc_normals_f64)."""
    import ctypes
    d = L.TgpSoftmax()
    d.N, d.C, d.S, d.seed, d.row0, d.step_dev = int(N), int(C), int(S), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), L.ptr(step_dev)
    eps = torch.empty(int(S), int(C), int(N), dtype=torch.float64, device=device)
    L.check(L.load().tgp_mc_normals_f64(d, L.ptr(eps), L.stream_ptr()), "tgp_mc_normals_f64")
    return eps


def predict_softmax(mu, v, spec, theta, S, eps=None, seed=0, step_dev=None, row0=0, Y=None):
    """P (N,C) = Monte-Carlo mean of softmax(G(f0)) (MulticlassCategorical.marginal_moments) and, with Y, log P[n, y_n]."""
    Y, mu, v, theta, eps, N = _softmax_args(Y, mu, v, spec, theta, eps, S)
    d = _softmax_desc(spec, N, S, theta, 1.0, seed, step_dev, row0)
    P = torch.empty(N, spec.C, dtype=torch.float64, device=mu.device)
    logp = torch.empty(N, dtype=torch.float64, device=mu.device) if Y is not None else None
    L.check(L.load().tgp_predict_softmax_f64(d, L.ptr(mu), L.ptr(v), L.ptr(eps), L.ptr(Y), L.ptr(P), L.ptr(logp),
                                             L.stream_ptr()), "tgp_predict_softmax_f64")
    return P, logp


class SoftmaxEllFunction(torch.autograd.Function):
    """ELL = MulticlassCategorical.expected_log_prob with autograd in (mu, v, theta); mu, v (C,N).  The draws are either
    `eps` (S,C,N) or the counter-based ones of (seed, step_dev, row0); value and gradients come from one launch."""

    @staticmethod
    def forward(ctx, Y, mu, v, theta, spec, S, eps, seed, step_dev, row0, scale):
        res = ell_softmax(Y, mu.detach(), v.detach(), spec, theta.detach() if theta is not None else None, S, eps=eps,
                          seed=seed, step_dev=step_dev, row0=row0, scale=scale)
        ctx.save_for_backward(res["g_mu"], res["g_v"], res["g_theta"])
        ctx.has = theta is not None
        return res["ell"].reshape(1)

    @staticmethod
    def backward(ctx, g):
        gmu, gv, gth = ctx.saved_tensors
        g = g.reshape(())
        return (None, g * gmu, g * gv, g * gth if ctx.has else None) + (None,) * 7


def flow_inverse(t, flow, theta, rowp=None, check=True):
    """x = T^-1(t) for t of shape (S,N) or (N,) (tgp_flow_inverse_f64: closed forms, else a bracketed Newton iteration per
    block).  Returns (x, status) -- status int32[1] on the device, the number of elements that did not converge; with
    `check` it is read (one sync) and a non-zero count raises."""
    lib = L.load()
    t = _c(t, "t")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    t2 = t.reshape(1, -1) if t.dim() == 1 else t.reshape(t.shape[0], -1)
    S, N = t2.shape
    lvn = torch.zeros(1, dtype=torch.float64, device=t.device)
    md, keep = _flow_model(N, 1, flow, theta, lvn, t.device)
    x = torch.empty_like(t)
    status = torch.zeros(1, dtype=torch.int32, device=t.device)
    L.check(lib.tgp_flow_inverse_f64(md, L.ptr(t2), S, N, L.ptr(rowp) if flow.RP > 0 else None, L.ptr(x), L.ptr(status),
                                     L.stream_ptr()), "tgp_flow_inverse_f64")
    if check and int(status[0]) != 0:
        raise L.TgpError("flow_inverse: %d element(s) did not converge (outside the flow's range?)" % int(status[0]))
    return x, status


def flow_eval(f, flow, theta, rowp=None, want=("G", "dG", "logdG")):
    """G(f), dG/df, log dG/df for f of shape (S,N) or (N,) (CompositeFlow.forward / forward_grad)."""
    lib = L.load()
    f = _c(f, "f")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    f2 = f.reshape(1, -1) if f.dim() == 1 else f
    S, N = f2.shape
    lvn = torch.zeros(1, dtype=torch.float64, device=f.device)
    md, keep = _flow_model(N, 1, flow, theta, lvn, f.device)
    outs = {k: (torch.empty_like(f) if k in want else None) for k in ("G", "dG", "logdG")}
    L.check(lib.tgp_flow_eval_f64(md, L.ptr(f2), S, N, L.ptr(rowp), L.ptr(outs["G"]), L.ptr(outs["dG"]),
                                  L.ptr(outs["logdG"]), L.stream_ptr()), "tgp_flow_eval_f64")
    return outs


def flow_logdet(f, flow, theta, rowp=None, want_G=False):
    """sum log dG/df over f (S,N) or (N,) in one fused pass (tgp_flow_logdet_f64); returns (sum 0-d, G or None)."""
    lib = L.load()
    f = _c(f, "f")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    f2 = f.reshape(1, -1) if f.dim() == 1 else f
    S, N = f2.shape
    lvn = torch.zeros(1, dtype=torch.float64, device=f.device)
    md, keep = _flow_model(N, 1, flow, theta, lvn, f.device)
    G = torch.empty_like(f) if want_G else None
    out = torch.empty(1, dtype=torch.float64, device=f.device)
    ws = torch.empty(lib.tgp_flow_logdet_workspace_bytes(S, N) // 8, dtype=torch.float64, device=f.device)
    L.check(lib.tgp_flow_logdet_f64(md, L.ptr(f2), S, N, L.ptr(rowp), L.ptr(G), L.ptr(out), L.ptr(ws), ws.numel() * 8,
                                    L.stream_ptr()), "tgp_flow_logdet_f64")
    return out[0], G


def predict(mu, v, lvn, flow=None, theta=None, S=None, rowp=None, Y=None, Y_std=1.0, lik=None, want_moments=True, df=None):
    """Predictive moments m1, m2 and per-row test log-likelihood kernel (see tgp_predict_f64).  lik = lib.LIK_BERNOULLI:
    m1 = P(y = 1), m2 = P (1 - P), logp = y log P + (1 - y) log(1 - P) (`flow` a FlowSpec, possibly empty).
    lik = lib.LIK_POISSON: m1 = E[y], m2 = Var[y] in counts, logp = the log predictive pmf at Y (finite however small).
    lik = lib.LIK_STUDENT: Student-t noise of `df` degrees of freedom and squared scale exp(lvn): m1, m2 in standardised units
    (m2 includes sigma^2 df / (df - 2)), logp = the exact log predictive density of the raw target, every constant and
    -log Y_std included.
    lik = lib.LIK_NEGBIN: as LIK_POISSON with the dispersion r = exp(lvn): m2 = m1 + (1 + 1/r) E[mean^2] - m1^2.
    lik = lib.LIK_ORDINAL: m1 = E[y], m2 = Var[y] in classes, logp = the log predictive pmf of class Y (closed form for an
    empty `flow`).  `df` is the slot for what rides beside the noise (noise_slot): the Student-t's degrees of freedom, the
    ordinal likelihood's bin edges.
    lik = lib.LIK_GAMMA: m1 = E[y], m2 = Var[y] = (1 + 1/a) E[mean^2] - m1^2 with the shape a = exp(lvn), logp = the log predictive
    density of the raw target, -log Y_std included (targets divided by Y_std, not centred).
    lik = lib.LIK_BETA: m1 = E[y] = E[mean], m2 = Var[y] = E[mean (1 - mean)] / (1 + phi) + Var[mean] with the precision
    phi = exp(lvn), logp = the log predictive density of the proportion Y; Y_std is ignored."""
    lib = L.load()
    if lik in (L.LIK_STUDENT, L.LIK_ORDINAL):
        if flow is None:
            raise L.TgpError(L.NEEDS_FLOWSPEC % L.LIK_DISPLAY[lik])
        lvn = noise_slot(lvn, lik, df)
    mu, v, lvn = _c(mu, "mu"), _c(v, "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    dev, N = mu.device, mu.numel()
    md, keep = _flow_model(N, S, flow, theta, lvn, dev, lik=lik)
    # (want_moments=False: logp only -- the warped moments cost S flow inversions per row)
    m1, m2 = (torch.empty_like(mu), torch.empty_like(mu)) if want_moments else (None, None)
    logp = torch.empty_like(mu) if Y is not None else None
    Yc = _c(Y.reshape(-1), "Y") if Y is not None else None
    L.check(lib.tgp_predict_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(Yc), float(Y_std), L.ptr(m1), L.ptr(m2),
                                L.ptr(logp), L.stream_ptr()), "tgp_predict_f64")
    return m1, m2, logp


def quantile_probs(probs, device=None):
    """probs (a float, a sequence or a tensor, any order) -> (probs, zq = Phi^-1(probs)) as float64 (Q,) tensors on `device`.
    Checked on the host, before any launch: every entry strictly inside (0, 1).  (Their number, 1 <= Q <= lib.QUANTILE_MAX_Q,
    is the library's to refuse.)"""
    p = torch.as_tensor(probs, dtype=torch.float64).detach().to("cpu").reshape(-1)
    if not bool(((p > 0.0) & (p < 1.0)).all()):      # (a NaN fails both comparisons)
        raise ValueError("probabilities must lie strictly inside (0, 1), got %s" % p.tolist())
    zq = torch.special.ndtri(p)
    return (p, zq) if device is None else (p.to(device), zq.to(device))


def _quantile_model(mu, lvn, flow, theta, S, lik=None):
    if flow is not None and S is None:
        raise ValueError("a flow needs S, the number of Gauss-Hermite nodes")
    if lik in (L.LIK_GAMMA, L.LIK_BETA) and flow is None:
        raise L.TgpError(L.NEEDS_FLOWSPEC % L.LIK_DISPLAY[lik])
    return _flow_model(mu.numel(), S, flow, theta, lvn, mu.device, lik=lik)


def predict_quantiles(mu, v, lvn, probs, flow=None, theta=None, S=None, rowp=None, check=True, lik=None):
    """Exact quantiles of the predictive distribution ops.predict integrates (tgp_predict_quantile_f64): t of shape (Q,N), in
    the model's standardised units, t[q,n] the root of sum_s wn_s Phi((t - G(mu_n + sqrt(2 v_n) xs_s)) / sigma) = probs[q].
    flow=None: the Gaussian likelihood's closed form.  With `check` the status word is read (one sync) and a root that did
    not converge raises; check=False returns (t, status) and leaves NaN in its place.
    lik = lib.LIK_GAMMA (`flow` a FlowSpec, possibly empty; lvn the log shape): the quantiles of the mixture of Gammas, t > 0,
    the roots found in log t.  lik = lib.LIK_BETA (lvn the log precision): the quantiles of the mixture of Betas, 0 < t < 1, the
    roots found in logit t.  Every other value of `lik` but None is the library's to refuse."""
    lib = L.load()
    mu, v, lvn = _c(mu.reshape(-1), "mu"), _c(v.reshape(-1), "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    p, zq = quantile_probs(probs, mu.device)
    md, keep = _quantile_model(mu, lvn, flow, theta, S, lik)
    t = torch.empty(p.numel(), mu.numel(), dtype=torch.float64, device=mu.device)
    status = torch.zeros(1, dtype=torch.int32, device=mu.device)
    L.check(lib.tgp_predict_quantile_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(p), L.ptr(zq), p.numel(), L.ptr(t),
                                         L.ptr(status), L.stream_ptr()), "tgp_predict_quantile_f64")
    if not check:
        return t, status
    if int(status[0]) != 0:
        raise L.TgpError("predict_quantiles: %d root(s) did not converge" % int(status[0]))
    return t


def predict_cdf(mu, v, lvn, Y, flow=None, theta=None, S=None, rowp=None, lik=None):
    """(cdf, sf): the predictive CDF at Y per row -- the PIT values of a calibration plot -- and the upper tail 1 - cdf from
    its own sum (tgp_predict_cdf_f64); Y in the model's standardised units.  lik = lib.LIK_GAMMA: of the mixture of Gammas
    (lvn the log shape); a Y <= 0 has cdf 0.  lik = lib.LIK_BETA: of the mixture of Betas (lvn the log precision); a Y <= 0 has
    cdf 0 and a Y >= 1 has sf 0."""
    lib = L.load()
    mu, v, lvn = _c(mu.reshape(-1), "mu"), _c(v.reshape(-1), "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    Yc = _c(Y.reshape(-1), "Y")
    if Yc.numel() != mu.numel():
        raise ValueError("Y must hold one value per row (%d), got %d" % (mu.numel(), Yc.numel()))
    md, keep = _quantile_model(mu, lvn, flow, theta, S, lik)
    cdf, sf = torch.empty_like(mu), torch.empty_like(mu)
    L.check(lib.tgp_predict_cdf_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(Yc), L.ptr(cdf), L.ptr(sf), L.stream_ptr()),
            "tgp_predict_cdf_f64")
    return cdf, sf


def predict_crps(mu, v, lvn, Y, flow=None, theta=None, S=None, rowp=None, want_parts=False):
    """The continuous ranked probability score of the predictive at Y per row, int (F_n(t) - 1{t >= Y_n})^2 dt in closed form
    (tgp_predict_crps_f64): crps (N,), in the model's standardised units like Y.  want_parts: (crps, parts) with parts (2,N) =
    T1 = E|Y - y| and T2 = E|Y - Y'| / 2, crps = T1 - T2 bit for bit.  flow=None: the Gaussian likelihood's closed form."""
    lib = L.load()
    mu, v, lvn = _c(mu.reshape(-1), "mu"), _c(v.reshape(-1), "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    Yc = _c(Y.reshape(-1), "Y")
    if Yc.numel() != mu.numel():
        raise ValueError("Y must hold one value per row (%d), got %d" % (mu.numel(), Yc.numel()))
    md, keep = _quantile_model(mu, lvn, flow, theta, S)
    crps = torch.empty_like(mu)
    parts = torch.empty(2, mu.numel(), dtype=torch.float64, device=mu.device) if want_parts else None
    L.check(lib.tgp_predict_crps_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(Yc), L.ptr(crps), L.ptr(parts), L.stream_ptr()),
            "tgp_predict_crps_f64")
    return (crps, parts) if want_parts else crps


def predict_moment_grads(mu, v, lvn, flow=None, theta=None, S=None, rowp=None, lik=None):
    """(dm1, dm2), each (2, N): the partial derivatives of the predictive mean m1 and variance m2 that ops.predict reports
    (standardised units) in the q(f) marginals -- row 0 in mu, row 1 in v -- at fixed per-row parameters
    (tgp_predict_moment_grads_f64).  flow=None or an empty program: (1, 0) and (0, 1).  A row with v <= 0 has exact zeros in
    row 1.  Every `lik` but None, lib.LIK_GAUSS and lib.LIK_FLOW is the library's to refuse."""
    lib = L.load()
    mu, v, lvn = _c(mu.reshape(-1), "mu"), _c(v.reshape(-1), "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    md, keep = _quantile_model(mu, lvn, flow, theta, S, lik)
    dm1 = torch.empty(2, mu.numel(), dtype=torch.float64, device=mu.device)
    dm2 = torch.empty_like(dm1)
    L.check(lib.tgp_predict_moment_grads_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ptr(dm1), L.ptr(dm2), L.stream_ptr()),
            "tgp_predict_moment_grads_f64")
    return dm1, dm2


def predict_acquisition(mu, v, lvn, kind, best, flow=None, theta=None, S=None, rowp=None, maximize=True, want_partials=False,
                        jac=None):
    """An acquisition function of the predictive ops.predict integrates against the incumbent `best` (a float, standardised
    units), per row (tgp_predict_acquisition_f64): kind "ei" the expected improvement E[(c (y - best))_+], "log_ei" its
    logarithm (finite where EI underflows), "pi" the probability of improvement; c = +1 with `maximize`, else -1.  Returns
    value (N,); with want_partials (value, partials), partials (2, N) = the partials of value in mu (row 0) and v (row 1) at
    fixed flow parameters; with jac = (dmu_dx, dv_dx), each (N, D) -- ops.qf_input_grad's -- (value, grad_x), grad_x (N, D) =
    partials[0][:, None] dmu_dx + partials[1][:, None] dv_dx formed in the same launch (with both: all three).  flow=None: the
    Gaussian likelihood's closed form.  A row with v <= 0 has an exact zero in partials[1].  No autograd."""
    lib = L.load()
    if kind not in L.ACQ_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(repr(k) for k in L.ACQ_KINDS), kind))
    mu, v, lvn = _c(mu.reshape(-1), "mu"), _c(v.reshape(-1), "v"), _c(lvn, "lvn")
    theta, rowp = _c(theta, "theta"), _c(rowp, "rowp")
    N = mu.numel()
    md, keep = _quantile_model(mu, lvn, flow, theta, S)
    value = torch.empty_like(mu)
    partials = torch.empty(2, N, dtype=torch.float64, device=mu.device) if want_partials else None
    dmu_dx = dv_dx = grad_x = None
    D = 0
    if jac is not None:
        dmu_dx, dv_dx = (_c(t, "jac") for t in jac)
        if dmu_dx.dim() != 2 or dmu_dx.shape[0] != N or dv_dx.shape != dmu_dx.shape:
            raise ValueError("jac must be (dmu_dx, dv_dx), each of shape (%d, D), got %s and %s"
                             % (N, tuple(dmu_dx.shape), tuple(dv_dx.shape)))
        D = dmu_dx.shape[1]
        grad_x = torch.empty_like(dmu_dx)
    L.check(lib.tgp_predict_acquisition_f64(md, L.ptr(mu), L.ptr(v), L.ptr(rowp), L.ACQ_KINDS[kind], float(best),
                                            0 if maximize else 1, L.ptr(value), L.ptr(partials), L.ptr(dmu_dx), L.ptr(dv_dx), D,
                                            L.ptr(grad_x), L.stream_ptr()), "tgp_predict_acquisition_f64")
    out = (value,) + ((partials,) if want_partials else ()) + ((grad_x,) if jac is not None else ())
    return out[0] if len(out) == 1 else out


def crps_from_samples(draws, y):
    """The CRPS of the empirical distribution of `draws` (S,N) at y (N,), per row: the sorted-sample form
    1/S sum_i |x_i - y| - 1/S^2 sum_i (2 i - S - 1) x_(i), i = 1..S over the sorted draws, which is exactly the double sum
    1/S sum_i |x_i - y| - 1/(2 S^2) sum_ij |x_i - x_j|.  Plain torch on the tensors' device."""
    S = draws.shape[0]
    x = draws.reshape(S, -1)
    y = y.reshape(1, -1).to(x.dtype)
    xs, _ = torch.sort(x, dim=0)
    c = (2.0 * torch.arange(1, S + 1, dtype=x.dtype, device=x.device) - S - 1.0).reshape(S, 1)
    return (x - y).abs().sum(0) / S - (c * xs).sum(0) / (S * S)


def interval_score(lo, hi, y, alpha):
    """The interval score of the central (1 - alpha) interval [lo, hi] at y (Gneiting & Raftery 2007):
    (hi - lo) + 2/alpha (lo - y)_+ + 2/alpha (y - hi)_+, elementwise."""
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie strictly inside (0, 1), got %r" % alpha)
    return (hi - lo) + (2.0 / alpha) * (lo - y).clamp_min(0.0) + (2.0 / alpha) * (y - hi).clamp_min(0.0)


# ---------------------------------------------------------------------------------------------------
# per-row parameter networks of the input-dependent flows (models/flow.py:836-897)
# ---------------------------------------------------------------------------------------------------
MLP_LDS_MAX = 160 * 1024 - 1024     # what tgp_launch.hpp ensure_lds grants a kernel on gfx950 (160 KiB less the static words)


class MlpSpec:
    """nnets MLPs of one architecture D -> H x L -> 1 (Linear -> act -> Dropout per hidden layer)."""

    def __init__(self, D, H, L, nnets, act="relu", drop_p=0.0, seed=0):
        self.D, self.H, self.L, self.nnets = int(D), int(H), int(L), int(nnets)
        self.act = {"relu": 0, "tanh": 1}[act]
        self.drop_p, self.seed = float(drop_p), int(seed)

    def salted(self, salt):
        """The same networks with the dropout-mask stream of another call site (seed ^ salt): masks are a hash of (seed,
        step, net, layer, row, unit) and every call site counts its own steps from 0, so without a salt the masks of
        evaluation call k would be those of training step k."""
        return MlpSpec(self.D, self.H, self.L, self.nnets, act={0: "relu", 1: "tanh"}[self.act], drop_p=self.drop_p,
                       seed=self.seed ^ int(salt))

    @property
    def weights_per_net(self):
        return self.D * self.H + self.H + (self.L - 1) * (self.H * self.H + self.H) + self.H + 1

    def lds_bytes(self):
        """Dynamic LDS of the backward kernel, tgp_mlp.hip mlp_lds(D, H, L, bwd = true) restated term by term: the weight image
        padded to the kernel variant's R = 4 NKS units (32, 52 or 64 -- not to H), the input strip, the output layer's per-wave
        sums and L activation strips [H][66].  A shape is trainable on the kernels iff this is <= MLP_LDS_MAX (ensure_lds);
        tgp_mlp_backward_f64 answers TGP_E_LDS beyond it (L = 3 with H > 53, at D <= 8)."""
        R = 4 * (8 if self.H <= 32 else 13 if self.H <= 52 else 16)
        kp0, st = (self.D + 3) // 4 * 4, 66
        n = R * kp0 + R + (self.L - 1) * (R * R + R) + R + 2      # W_0, b_0, the hidden layers' W_l, b_l, then wo, bo
        n += kp0 * st                                             # x0
        n = (n + 4 * (self.H + 1) + 1) // 2 * 2                   # dwo
        return (n + self.L * self.H * st) * 8

    def struct(self, N, training):
        d = L.TgpMlp()
        d.N, d.D, d.H, d.L, d.nnets, d.act = int(N), self.D, self.H, self.L, self.nnets, self.act
        d.training, d.drop_p, d.seed = int(bool(training)), self.drop_p, self.seed
        return d


def mlp_forward(spec, X, W, training=False, step_dev=None):
    """out (N, nnets) = the nets' outputs for every row (tgp_mlp_forward_f64)."""
    X, W = _c(X, "X"), _c(W, "W")
    d = spec.struct(X.shape[0], training)
    out = torch.empty(X.shape[0], spec.nnets, dtype=torch.float64, device=X.device)
    L.check(L.load().tgp_mlp_forward_f64(d, L.ptr(X), L.ptr(W), L.ptr(step_dev), L.ptr(out), L.stream_ptr()),
            "tgp_mlp_forward_f64")
    return out


_mlp_ws = {}


def mlp_backward(spec, X, W, g_out, training=False, step_dev=None, g_W=None):
    """d(objective)/dW (packed like W) from g_out (N, nnets) (tgp_mlp_backward_f64; recomputes the forward)."""
    X, W, g_out = _c(X, "X"), _c(W, "W"), _c(g_out, "g_out")
    lib = L.load()
    d = spec.struct(X.shape[0], training)
    key = (X.shape[0], spec.D, spec.H, spec.L, spec.nnets, str(X.device), torch.cuda.current_stream().cuda_stream)
    ws = _mlp_ws.get(key)
    if ws is None:
        ws = torch.empty(lib.tgp_mlp_workspace_bytes(d) // 8 + 16, dtype=torch.float64, device=X.device)
        _mlp_ws[key] = ws
    if g_W is None:
        g_W = torch.empty_like(W)
    L.check(lib.tgp_mlp_backward_f64(d, L.ptr(X), L.ptr(W), L.ptr(step_dev), L.ptr(g_out), L.ptr(g_W), L.ptr(ws),
                                     ws.numel() * 8, L.stream_ptr()), "tgp_mlp_backward_f64")
    return g_W


class MlpFunction(torch.autograd.Function):
    """rowp = MLPs(X; W) with the HIP forward/backward; W is the packed weight vector (torch.cat of the nets'
    parameters, so autograd scatters g_W back onto the individual nn.Parameters)."""

    @staticmethod
    def forward(ctx, X, W, spec, training, step_dev):
        ctx.spec, ctx.training, ctx.step_dev = spec, training, step_dev
        ctx.save_for_backward(X, W)
        return mlp_forward(spec, X, W.detach(), training, step_dev)

    @staticmethod
    def backward(ctx, g_out):
        X, W = ctx.saved_tensors
        return None, mlp_backward(ctx.spec, X, W.detach(), g_out.contiguous(), ctx.training, ctx.step_dev), None, None, None


MASK_SALT_EVAL = 0x45564131     # model-class evaluation (test_log_likelihood, predictive moments)
MASK_SALT_NETS = 0x4E455453     # flow.nets_rowp (CompositeFlow.forward, sampling)


def mlp_keep_mask(seed, step, net, layer, rows, units, p):
    """The dropout keep mask of tgp_mlp.hip (rows x units, bool) restated in numpy: test infrastructure and the
    reference for anyone who needs to reproduce a training-mode forward elsewhere."""
    import numpy as np
    M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
    r = np.arange(rows, dtype=np.uint64).reshape(-1, 1)
    j = np.arange(units, dtype=np.uint64)
    ug = ((j >> np.uint64(4)) * np.uint64(4) + (j & np.uint64(3))).reshape(1, -1)    # group: the 4 accumulator regs of a lane
    lane = ((j >> np.uint64(2)) & np.uint64(3)).reshape(1, -1)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(step)) & M64
        z = z ^ (np.uint64(net) << np.uint64(56)) ^ (np.uint64(layer) << np.uint64(48)) ^ (ug << np.uint64(32)) ^ r
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
        z = z ^ (z >> np.uint64(31))
    bits = (z >> (np.uint64(16) * lane)) & np.uint64(0xFFFF)
    return bits >= np.uint64(int(p * 65536.0 + 0.5))


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              maximize=False):
    """In-place Adam on flat float64 buffers (torch.optim.Adam semantics)."""
    lib = L.load()
    L.check(lib.tgp_adam_f64(L.ptr(params), L.ptr(grads), L.ptr(exp_avg), L.ptr(exp_avg_sq), params.numel(), lr,
                             betas[0], betas[1], eps, weight_decay, int(step), int(bool(maximize)), L.stream_ptr()),
            "tgp_adam_f64")
