"""Step engine: the reference's inner training loop (code/dsp/trainers/trainer_base.py:329-349 --
ELBO -> (-ELBO).backward() -> Adam.step()) with everything resident on the GPU.

* every trainable tensor is a view into ONE flat float64 buffer (parameters, gradients, Adam moments),
  so the optimiser is a single launch and the multi-GPU exchange is a single all-reduce;
* the C-ABI model and gradient structs are built once (pointers never change), so one step is
  `tgp_elbo_step_adam_f64` = 4 kernel launches (M <= 128) with no host synchronisation, plus
  the MLP forward/backward launches for input-dependent flows;
* an engine owns its workspace; what the engines cover is `engine_refusal`, the step sequence is
  `ElboEngine._one_step`, and every switch is an argument (no environment variable is read here);
* `capture()` records that sequence into a HIP graph (torch.cuda.CUDAGraph is only the stream/graph
  plumbing) and `replay()` re-launches it;
* multi-GPU (one process per GPU): rows are sharded, every rank runs the same M x M work, and ONE
  all-reduce(sum) over RCCL/xGMI of [gradients | ELL | KL/W] makes every rank's buffer complete
  (SURVEY.md 8e); the KL gradient enters each rank with weight 1/world so the sum counts it once.
"""
import ctypes as C
import os.path
import warnings

import torch

from . import lib as L
from . import ops

# Stream-capture mode of every graph this package records.  "thread_local", not torch's default "global": with an NCCL
# (= RCCL) process group alive, its watchdog thread polls the events of earlier collectives with hipEventQuery, which the
# global mode forbids while ANY stream of the process captures -- measured on this stack (ROCm 7.0 / RCCL 2.26,
# tools/probes/rccl_smoke.py): the process dies with hipErrorStreamCaptureUnsupported; thread-local capture records the
# same graph (collective included) and replays it.
CAPTURE_MODE = "thread_local"

# "mean_a" / "mean_b": a linear mean function's parameters; "nn" (packed MLP weights) last: the weight-decay group
ORDER = ("Z", "raw_ls", "raw_os", "m", "Lam", "lvn", "theta", "mean_a", "mean_b", "nn")

# the `likelihood` names of the quadrature likelihoods that train through ops.ElboFunction only
EAGER_ONLY = {"bernoulli": L.LIK_BERNOULLI, "poisson": L.LIK_POISSON, "negbinomial": L.LIK_NEGBIN, "studentt": L.LIK_STUDENT,
              "ordinal": L.LIK_ORDINAL, "gamma": L.LIK_GAMMA, "beta": L.LIK_BETA}


def engine_refusal(is_whiten=True, mean=None, likelihood=None, world_size=1, collective=None, per_row=False, minibatch=False,
                   kernel=None):
    """What the step engines cover, stated once: None when ElboEngine (`minibatch` False) or MinibatchEngine (True) takes the
    combination, else the message both refuse it with (_refuse) before they load the library or touch the device; the
    trainers take the eager loop on a message.  A pure function of the description: `mean` = None / "linear" / "identity",
    `likelihood` = None (Gaussian or flow) / "warped" / "bernoulli" / "poisson" / "negbinomial" / "studentt" / "ordinal" / "gamma" / "beta" / "multiclass" / "hetero", `collective` as passed to the engine (asking
    for one counts as data-parallel, like world_size > 1), `per_row` = input-dependent flow parameters (an MLP or `rowp`),
    `kernel` = the covariance function's instance_kernel name (None: any but 'scale_rq')."""
    multi_rank = int(world_size) > 1 or collective is not None
    if not is_whiten:      # `params` of an unwhitened model describe q(u) itself; the captured step has no transform in it
        return "the step engines need is_whiten=True: an unwhitened q(u) trains on the eager path (Trainer_SP), on one rank"
    if likelihood in EAGER_ONLY:
        return ("the step engines have no %s likelihood: it trains on the eager path (ops.ElboFunction)"
                % L.LIK_DISPLAY[EAGER_ONLY[likelihood]])
    if likelihood == "multiclass":
        return "the step engines have no multi-class likelihood: its C latent GPs train on the eager path's composed step"
    if likelihood == "hetero":
        return ("the step engines have no heteroscedastic likelihood: its two latent GPs train on the eager path's composed "
                "step, on one rank")
    if mean is not None:
        if minibatch:
            return "the '%s' mean function has no minibatch engine: full batch on one rank (ElboEngine), or the eager loop" % mean
        if multi_rank:
            return "the '%s' mean function's engine is single-rank (world_size = 1): no data-parallel step with a mean" % mean
        if likelihood == "warped" or per_row:
            return "the '%s' mean function is not built for the warped likelihood or input-dependent flows" % mean
    if likelihood == "warped":
        if minibatch:
            return "the warped likelihood has no minibatch engine: full batch on one rank only (ElboEngine)"
        if multi_rank:
            return "the warped likelihood's engine is single-rank (world_size = 1): no data-parallel warped step"
        if per_row:
            return "the warped likelihood takes shared flow parameters only"
    if kernel == "scale_rq":   # (as the Student-t likelihood's nu behind log_var_noise)
        return ("the step engines have no rational-quadratic kernel: their flat parameter buffer has one slot behind raw_os and "
                "the kernel reads {raw_outputscale, alpha} there; 'scale_rq' trains on the eager path (ops.ElboFunction)")
    return None


def collapsed_refusal(flow_blocks=None, likelihood=None, mean=None, world_size=1, collective=None, per_row=False,
                      minibatch=False):
    """What ElboEngine(collapsed=True) does not cover, or None: the closed-form optimal q(u) is built into the captured step
    for the Gaussian likelihood with a zero mean, full batch, on one rank."""
    if flow_blocks is not None or per_row:
        return "the collapsed engine has no flow: q(u) has a closed-form optimum for a likelihood that is Gaussian in f only"
    if likelihood is not None:
        return "the collapsed engine takes the Gaussian likelihood only (got %r): set_optimal_qu serves the eager loop" % (likelihood,)
    if mean is not None:
        return "the collapsed engine takes the zero mean only (got %r): qu='optimal' with a mean trains on the eager loop" % (mean[0],)
    if int(world_size) > 1 or collective is not None:
        return "the collapsed engine is single-rank (world_size = 1): no data-parallel collapsed step"
    if minibatch:
        return "the collapsed engine is full batch: the optimum of q(u) belongs to the rows it was computed from"
    return None


def _refuse(**description):
    why = engine_refusal(**description)
    if why is not None:
        raise NotImplementedError(why)


def allreduce_flat(grad, n, world_size, group=None):
    """The ONE exchange of the data-parallel step: all-reduce(sum) of [gradients(n) | ELBO, ELL, KL, 0].
    Every rank enters with gradients of (ELL_shard - KL/world) and out = [ELL_shard - KL, ELL_shard, KL, 0]; KL is
    identical on all ranks, so it is pre-divided and the sum restores it; ELBO is rebuilt from the reduced parts.
    Works on any backend (RCCL on the GPUs, gloo in the CPU tests)."""
    if world_size > 1:
        pre_reduce(grad, n, world_size)
        torch.distributed.all_reduce(grad, op=torch.distributed.ReduceOp.SUM, group=group)
        post_reduce(grad, n)
    return grad


class RcclUnavailable(RuntimeError):
    """The ABI communicator could not be built on at least one rank (raised on EVERY rank of the group, so that all of
    them take the same fallback branch)."""


COMM_TIMEOUT_S = 120.0     # default bound of the communicator bootstrap (RcclComm(timeout_s=...), ElboEngine(comm_timeout_s=...))
_COMM_GENERATION = {}      # communicators built per group (key = the group's global ranks), counted by the group's rank 0


def _store_rendezvous(tag, world_size, timeout_s):
    """All ranks of the default process group's store arrive at `tag`, or TimeoutError after timeout_s: a rank that died
    on the way makes the others FAIL here instead of hanging inside ncclCommInitRank (VERDICT r4 #5a)."""
    import time
    try:
        store = torch.distributed.distributed_c10d._get_default_store()
    except Exception:
        return                                   # no store to meet at (a hand-made group): nothing to bound with
    store.add(tag, 1)
    t0 = time.time()
    while int(store.add(tag, 0)) < world_size:
        if time.time() - t0 > timeout_s:
            raise TimeoutError("only %d of %d ranks reached %s within %.0f s" % (int(store.add(tag, 0)), world_size, tag, timeout_s))
        time.sleep(0.005)


class RcclComm:
    """The C ABI's collective (tgp_comm_* / tgp_allreduce_f64: RCCL bound at run time, all-reduce on the CALLER's stream).
    One per process.  The group's rank 0 draws the 128-byte id; with more than one rank it travels through
    torch.distributed's object broadcast (any backend: it is a host-side exchange), so the bootstrap needs no second
    rendezvous.  The bootstrap is GUARDED (VERDICT r4 #5a): (1) the local steps (dlopen of RCCL, the id) never
    raise on their own -- every rank first learns through one MIN all-reduce whether ALL of them succeeded, and on a
    failure every rank raises RcclUnavailable together (nobody is left waiting in a broadcast); (2) the id is broadcast
    from the GLOBAL rank of the group's rank 0; (3) before ncclCommInitRank the ranks meet at the process group's store
    with a timeout, and the init call itself runs under a watchdog: a rank that cannot complete it raises TimeoutError
    (tgp_last_error() in the message) instead of hanging -- the caller exits non-zero, nothing re-execs."""

    def __init__(self, world_size=1, rank=0, group=None, timeout_s=None, uid=None):
        import threading
        timeout_s = COMM_TIMEOUT_S if timeout_s is None else float(timeout_s)
        self.comm = None
        dist = torch.distributed
        multi = world_size > 1 and dist.is_initialized() and uid is None
        if world_size > 1 and not multi and uid is None:
            #  a hand-made world: nothing here can carry rank 0's id to the others, and ncclCommInitRank with an
            # all-zero id never returns -- say so instead of hanging (and before the library is loaded: no build needed to test)
            raise RcclUnavailable("RcclComm(world_size=%d) needs torch.distributed initialised (the id travels through its "
                                  "object broadcast) or the 128-byte id of rank 0 passed as `uid`" % world_size)
        self.lib = L.load()
        given = uid
        uid = (C.c_char * 128)()
        if given is not None:
            uid.raw = bytes(given)[:128].ljust(128, b"\0")
        err = None
        try:
            path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")   # the RCCL this process already holds
            L.check(self.lib.tgp_comm_load(path.encode() if os.path.exists(path) else None), "tgp_comm_load")
            if rank == 0 and given is None:
                L.check(self.lib.tgp_comm_unique_id(C.cast(uid, C.c_void_p)), "tgp_comm_unique_id")
        except Exception as e:                      # (kept: all ranks must reach the agreement below)
            err = e
        if multi:
            dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
            ok = torch.tensor([0.0 if err is not None else 1.0], dtype=torch.float64, device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
            if float(ok.cpu()) < 0.5:
                raise RcclUnavailable("tgp_comm bootstrap failed on %s: %s" % ("this rank" if err is not None else "another rank",
                                                                              err if err is not None else "see its log"))
            src = dist.get_global_rank(group, 0) if group is not None else 0
            ranks = dist.get_process_group_ranks(group) if group is not None else list(range(dist.get_world_size()))
            key = "-".join(str(r) for r in ranks)
            # the rendezvous tag's generation is rank 0's count FOR THIS GROUP and travels with the id (a process-global
            # counter differs between ranks that are members of different sub-groups, and equal tags are what the ranks meet at)
            if rank == 0:
                _COMM_GENERATION[key] = _COMM_GENERATION.get(key, 0) + 1
            box = [bytes(uid.raw), _COMM_GENERATION.get(key, 0)]
            dist.broadcast_object_list(box, src=src, group=group)
            uid.raw = box[0]
            tag = "tgp_comm_init/%d/%s" % (int(box[1]), key)
            _store_rendezvous(tag, len(ranks), timeout_s)
        elif err is not None:
            raise RcclUnavailable(str(err))
        comm = C.c_void_p()
        res = {}

        def _init(device=torch.cuda.current_device() if torch.cuda.is_available() else None):
            try:
                if device is not None:
                    torch.cuda.set_device(device)    # (the watchdog thread starts on device 0: RCCL binds to the current one)
                res["rc"] = self.lib.tgp_comm_init(C.cast(uid, C.c_void_p), int(world_size), int(rank), C.byref(comm))
                res["err"] = self.lib.tgp_last_error().decode(errors="replace") if res["rc"] != 0 else ""
            except Exception as e:
                res["exc"] = e

        if world_size > 1:                           # any multi-rank init can block on a missing peer: always under the watchdog
            th = threading.Thread(target=_init, daemon=True)
            th.start()
            th.join(timeout_s)
            if th.is_alive():
                raise TimeoutError("tgp_comm_init (ncclCommInitRank, %d ranks) did not return within %.0f s on rank %d; "
                                   "tgp_last_error(): %s" % (world_size, timeout_s, rank,
                                                             self.lib.tgp_last_error().decode(errors="replace")))
        else:
            _init(None)
        if "exc" in res:
            raise res["exc"]
        if res.get("rc", -1) != 0:
            raise RuntimeError("tgp_comm_init failed (%d): %s" % (res.get("rc", -1), res.get("err", "")))
        self.comm = comm
        self.world_size, self.rank = int(world_size), int(rank)

    def allreduce(self, buf, n=None):
        """In-place sum of the first n doubles of `buf` over the ranks, on the current stream (capturable)."""
        n = buf.numel() if n is None else int(n)
        L.check(self.lib.tgp_allreduce_f64(self.comm, L.ptr(buf), n, L.stream_ptr()), "tgp_allreduce_f64")
        return buf

    def close(self):
        if self.comm:
            L.check(self.lib.tgp_comm_destroy(self.comm), "tgp_comm_destroy")
            self.comm = None


def choose_collective(requested, world_size, backend):
    """Which all-reduce a data-parallel engine starts with, and whether it has to prove itself first.
    Returns (candidate, needs_selfcheck): candidate in {"torch", "abi"}.
      "torch": torch.distributed.all_reduce between two graphs (any backend; one Python iteration per step);
      "abi"  : tgp_allreduce_f64 on the compute stream, a node of ONE captured graph (U steps per launch).
    `requested`: None / "auto" = pick; "torch" / "abi" = the caller's choice, taken as is.  "auto" proposes the ABI
    collective wherever RCCL is the transport (backend "nccl") and more than one rank exists -- subject to the
    self-check of ElboEngine._selfcheck_collective -- and torch.distributed everywhere else (gloo rehearsals, one rank)."""
    if requested in ("torch", "abi"):
        return requested, False
    if requested not in (None, "auto"):
        raise ValueError("collective must be None, 'auto', 'torch', 'abi' or an RcclComm")
    if backend == "nccl" and (world_size > 1 or requested == "auto"):
        return "abi", True
    return "torch", False


def pre_reduce(grad, n, world_size):
    """KL is identical on every rank: pre-divide so that the sum restores it."""
    grad[n + 2].div_(world_size)


def post_reduce(grad, n):
    """ELBO from the reduced parts."""
    grad[n] = grad[n + 1] - grad[n + 2]


def shard_rows(N, world_size, rank):
    """Contiguous row shard [lo, hi) of rank `rank`."""
    return (N * rank) // world_size, (N * (rank + 1)) // world_size


class FlatParams:
    """[Z | raw_ls | raw_os | m | Lam | lvn | theta] as views of one buffer (plus same-shaped grads/moments)."""

    def __init__(self, tensors, device):
        self.shapes = {k: tuple(tensors[k].shape) for k in ORDER if tensors.get(k) is not None}
        self.sizes = {k: int(torch.tensor(self.shapes[k]).prod()) if len(self.shapes[k]) else 1 for k in self.shapes}
        n = sum(self.sizes.values())
        self.n = n
        self.extra = 4  # [ELBO, ELL, KL, 0] ride at the end of the gradient buffer so one all-reduce carries them
        self.data = torch.zeros(n, dtype=torch.float64, device=device)
        self.grad = torch.zeros(n + self.extra, dtype=torch.float64, device=device)
        self.exp_avg = torch.zeros(n, dtype=torch.float64, device=device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float64, device=device)
        self.offsets = {}
        o = 0
        for k in ORDER:
            if k in self.shapes:
                self.offsets[k] = o
                self.view(k).copy_(tensors[k].to(device=device, dtype=torch.float64))
                o += self.sizes[k]

    def view(self, k, buf=None):
        buf = self.data if buf is None else buf
        o = self.offsets[k]
        return buf[o:o + self.sizes[k]].view(self.shapes[k])

    def gview(self, k):
        return self.view(k, self.grad)

    @property
    def out(self):
        return self.grad[self.n:self.n + self.extra]


class ElboEngine:
    def __init__(self, X, Y, params, N_total, flow_blocks=None, S=None, rowp=None, lr=0.01, betas=(0.9, 0.999),
                 eps=1e-8, device="cuda:0", world_size=1, rank=0, mb_global=None, process_group=None,
                 kernel="scale_rbf", mlp=None, mlp_weights=None, nn_weight_decay=1e-5, mlp_training=True,
                 jitter_ladder=1e-8, share=None, collective=None, plan=0, comm_timeout_s=None, likelihood=None,
                 is_whiten=True, mean=None, fused_adam=True, collapsed=False):
        """`collapsed` True: q(u) is not trained but set to its closed-form optimum inside every step (Titsias' collapsed
        bound).  A step is tgp_optimal_qu_f64 into the flat buffer's m / Lam segments -> tgp_elbo_step_phases_f64 (the unchanged
        step: its gradients for the hyper-parameters are the collapsed bound's, d ELBO / d q(u) vanishes at the optimum) -> Adam
        on the segments other than m and Lam (in front of them under the step counter, behind them under a twin counter that
        moves in lock step: the step counter advances once per step).  The scalars of a step are the bound at the
        hyper-parameters the step started from; after the last step q(u) belongs to those, so call refresh_qu() before the
        model is evaluated.  The optimum and the step factorise K at the same jitter (0) in the normal case; if the step's
        device ladder raises it, the step is still a valid ELBO, at a marginally sub-optimal q(u) -- the optimum itself has no
        device ladder, a failed factorisation of its own surfaces in check_status().  Full batch, one rank, Gaussian
        likelihood, zero mean: everything else raises NotImplementedError here (engine_refusal speaks for the Adam engines).
        `mean` = ("linear", a, b) or ("identity", W, None): m(x) = x a + b enters the step as a per-row affine block
        (a_n, b_n) = (1, m(x_n)) at the head of the flow program, G(f) -> G(f + m(x_n)).  Linear: a (D) and b (1) are segments
        of the flat buffer; a step is tgp_mean_forward_f64 -> the ELBO step (all phases) -> tgp_mean_backward_f64 from
        g_rowp[:, 1] into the flat gradient -> the separate Adam launch, all captured.  Identity: W is fixed, the rows'
        parameters are written once.  With the Gaussian likelihood (flow_blocks None) the step runs TGP_LIK_FLOW over the
        otherwise empty program: Gauss-Hermite integrates the quadratic integrand exactly, so the result differs from the
        closed form by rounding only.  One rank, full batch.
        `likelihood` = "warped": `flow_blocks` / theta describe T applied to the TARGETS (TGP_LIK_WARPED): pre-pass t = T(Y)
        -> the Gaussian step on t -> post-pass (theta's gradient, log-Jacobian) -> one Adam launch, captured like the
        others.  Full batch on one rank only.
        `mlp` (ops.MlpSpec) + `mlp_weights` (packed, nnets * weights_per_net): input-dependent flow (ID_TGP) whose
        per-row parameters come from the HIP MLP kernels inside the step; `nn_weight_decay` is the reference's Adam
        group for the 'NNets' parameters (main.py:276-288).  `share` = another ElboEngine of the same model whose flat
        parameter / gradient / Adam buffers, step counter and status words this one uses (two batch sizes of one training
        run).  The workspace is never shared: every engine allocates its own, so that two live engines of one shape cannot read
        each other's intermediates.  `fused_adam` False: Adam stays a launch of its own where the update could ride in the
        backward launches.  What is refused, and why, is engine_refusal()."""
        _refuse(is_whiten=is_whiten, mean=None if mean is None else mean[0], likelihood=likelihood, world_size=world_size,
                collective=collective, per_row=mlp is not None or rowp is not None, kernel=kernel)
        if likelihood not in (None, "warped"):
            raise ValueError("likelihood must be None or 'warped'")
        self.collapsed = bool(collapsed)
        if self.collapsed:
            why = collapsed_refusal(flow_blocks=flow_blocks, likelihood=likelihood, mean=mean, world_size=world_size,
                                    collective=collective, per_row=mlp is not None or rowp is not None,
                                    minibatch=mb_global is not None or share is not None)
            if why is not None:
                raise NotImplementedError(why)
        if mean is not None and mean[0] not in ("linear", "identity"):
            raise ValueError("mean must be ('linear', a, b) or ('identity', W, None), got %r" % (mean[0],))
        self.lib = L.load()
        self.device = torch.device(device)
        self.world_size, self.rank, self.pg = int(world_size), int(rank), process_group
        self.warped, self.mean = likelihood == "warped", None if mean is None else mean[0]
        self.mlp, self.mlp_training, self.nn_wd = mlp, bool(mlp_training), float(nn_weight_decay)
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        if self.mean is not None:
            rowp = torch.zeros(X.shape[0], 2, dtype=torch.float64)
            flow_blocks = [(L.FLOW_AFFINE, 0, 0, L.FLAG_PER_ROW)] + [tuple(b) for b in (flow_blocks or [])]
            S = S if S else 8
        if self.warped and flow_blocks is None:
            flow_blocks = []
        self._open_collective(collective, comm_timeout_s)
        self._flat_buffers(X, Y, params, rowp, mean, mlp_weights, share)
        self._abi_structs(flow_blocks, S, float(N_total) / float(mb_global if mb_global is not None else self.N), kernel, plan,
                          jitter_ladder)
        self._feature_scratch(plan)
        # One rank, shared flow parameters only: ELBO step + Adam in ONE C-ABI call (tgp_elbo_step_adam_f64: on the fused path the
        # update rides in the last two backward launches -- one launch and one pass over the buffers less).  `fused_update` is the
        # caller's choice (all the rotated ID_TGP unit goes by), `fused_adam` whether the WHOLE step is that one call.
        self.fused_update = bool(fused_adam)
        self.fused_adam = (self.fused_update and self.world_size == 1 and self.comm is None and self.mlp is None
                           and self.mean is None and not self.collapsed)
        if self.collapsed:
            # (16 bytes = 2 doubles of slack over what the sizer gives)
            self.qu_ws, _ = ops._scratch(self.lib.tgp_optimal_qu_workspace_bytes(self.N, self.D, self.M) + 16, self.device)
            self.qu_status = ops._status(self.device)
            self.step_tail = torch.zeros(2, dtype=torch.int32, device=self.device)    # the twin counter of the segments behind Lam
        self.pre_step = self.post_step = None   # callables launched (and captured) before / after the step: the minibatch gather
        self.pipeline_steps = True      # ID_TGP, one rank: capture the rotated unit (see capture())
        self._out = None                # redirected scalar output while the unrolled graph is being captured
        self.unroll, self.gU, self.hist_u = 1, None, None           # steps per replay of self.gU (capture())
        self.unroll_long, self.gL, self.hist_l = 1, None, None      # a longer unrolled graph for long runs (capture())
        self.graph, self._side, self._warm, self._warned_jitter = None, None, False, 0

    def _open_collective(self, collective, comm_timeout_s):
        """`collective`: "torch" = torch.distributed.all_reduce between two graphs; "abi" = tgp_allreduce_f64 on the
        compute stream, INSIDE the captured step (one graph, U steps per launch like a single rank's) -- an RcclComm or
        the string (a communicator is then created here; torch.distributed only carries its 128-byte id).  With "abi" a
        1-rank engine runs the collective too (sum over one rank): the path the GPU tests can reach on one GPU.
        Default (None / "auto"): with more than one rank over RCCL the engine builds the ABI communicator, reduces a seeded
        buffer through BOTH paths and keeps the ABI collective only if every rank saw the same sums (choose_collective,
        _selfcheck_collective); any other situation keeps torch.distributed.  `collective_info` records the decision."""
        self.comm, self._own_comm = None, False
        if isinstance(collective, RcclComm):
            self.comm = collective
            self.collective_info = {"collective": "abi", "selfcheck": "skipped", "why": "communicator passed in"}
            return
        dist, group = torch.distributed, self.pg
        backend = dist.get_backend(group) if dist.is_initialized() else None
        cand, check = choose_collective(collective, self.world_size, backend)
        self.collective_info = {"collective": cand, "selfcheck": "skipped",
                                "why": "requested" if collective in ("torch", "abi") else "backend %s, %d rank(s)" % (backend, self.world_size)}
        if cand != "abi":
            return
        # (RCCL binds the communicator and the stream to the CURRENT device: make that this engine's)
        with torch.cuda.device(self.device):
            # (the communicator spans the process group that carries its id, whatever `world_size` weights KL with)
            cw = dist.get_world_size(group) if dist.is_initialized() else self.world_size
            cr = dist.get_rank(group) if dist.is_initialized() else self.rank
            try:
                self.comm, self._own_comm = RcclComm(cw, cr, group, timeout_s=comm_timeout_s), True
            except RcclUnavailable as e:
                # every rank raised together (RcclComm's agreement step): with the automatic choice all of them
                # keep torch.distributed; an explicit "abi" request is an error
                if not check:
                    raise
                warnings.warn("ABI collective unavailable (%s): keeping torch.distributed.all_reduce" % e)
                self.collective_info.update(collective="torch", selfcheck="skipped", why="bootstrap failed: %s" % e)
                return
            if check:
                ok, why = self._selfcheck_collective(group)
                self.collective_info.update(selfcheck="pass" if ok else "fail", why=why)
                if not ok:
                    warnings.warn("tgp_allreduce_f64 failed its self-check (%s): keeping torch.distributed.all_reduce" % why)
                    self.close()
                    self.collective_info["collective"] = "torch"

    def _flat_buffers(self, X, Y, params, rowp, mean, mlp_weights, share):
        """The data; every trainable tensor as a segment of ONE flat buffer (`share`'s where given); step counter, status words."""
        self.X = X.to(self.device, torch.float64).contiguous()
        self.Y = Y.reshape(-1).to(self.device, torch.float64).contiguous()
        self.N, self.D = self.X.shape
        names = {"Z": "Z", "raw_ls": "raw_lengthscale", "raw_os": "raw_outputscale", "m": "m", "Lam": "Lam",
                 "lvn": "log_var_noise", "theta": "theta"}
        tensors = {k: params.get(v, params.get(k)) for k, v in names.items()}
        for k in ("raw_ls", "raw_os", "lvn"):
            tensors[k] = tensors[k].reshape(-1)
        if self.mlp is not None:
            tensors["nn"] = mlp_weights.reshape(-1)
            assert tensors["nn"].numel() == self.mlp.nnets * self.mlp.weights_per_net
            assert rowp is None, "per-row parameters come from the MLPs"
            rowp = torch.zeros(self.N, self.mlp.nnets, dtype=torch.float64)
        self.mean_W = None
        if self.mean == "linear":
            tensors["mean_a"], tensors["mean_b"] = mean[1].detach().reshape(-1), mean[2].detach().reshape(-1)
            assert tensors["mean_a"].numel() == self.D and tensors["mean_b"].numel() == 1
        elif self.mean == "identity":
            self.mean_W = mean[1].detach().reshape(-1).to(self.device, torch.float64).contiguous()
            assert self.mean_W.numel() == self.D
        self.fp = FlatParams(tensors, self.device) if share is None else share.fp
        self.M = self.fp.sizes["m"]
        # (with per-row networks the flat buffer's tail is their weights: an Adam group of its own -- weight decay, second stream)
        self.n_plain = self.fp.offsets["nn"] if self.mlp is not None else self.fp.n
        self.rowp = rowp.to(self.device, torch.float64).contiguous() if rowp is not None else None
        self.g_rowp = torch.zeros_like(self.rowp) if self.rowp is not None else None
        self.step_dev = torch.zeros(2, dtype=torch.int32, device=self.device) if share is None else share.step_dev
        self.status = ops._status(self.device) if share is None else share.status

    def _abi_structs(self, flow_blocks, S, scale, kernel, plan, jitter_ladder):
        """tgp_model and tgp_grads, built once: the pointers never change."""
        fp = self.fp
        P = fp.sizes.get("theta", 0)
        RP = self.rowp.shape[1] if self.rowp is not None else 0
        self.S = int(S) if S else 1
        self.flow = ops.FlowSpec(flow_blocks, P, RP, self.device) if flow_blocks is not None else None
        self.md, self._keep = ops._model_struct(self.X, fp.view("Z"), fp.view("raw_ls"), fp.view("raw_os"), fp.view("m"),
                                                fp.view("Lam"), fp.view("lvn"), scale, 0.0, 1.0 / self.world_size,
                                                self.flow, fp.view("theta") if P else None, self.S, kernel, plan,
                                                L.LIK_WARPED if self.warped else None)
        # psd_safe_cholesky's retry ladder (dsp/utils.py:256-269) runs on the device inside the captured step (fused path);
        # `jitter_ladder` is its base value (the reference: 1e-8 in float64, or cg.global_jitter), 0 disables it
        self.md.jitter_ladder = float(jitter_ladder or 0.0)
        self.gs = L.TgpGrads()
        self.gs.Z, self.gs.raw_ls, self.gs.raw_os = (L.ptr(fp.gview(k)) for k in ("Z", "raw_ls", "raw_os"))
        self.gs.m, self.gs.Lam, self.gs.log_var_noise = (L.ptr(fp.gview(k)) for k in ("m", "Lam", "lvn"))
        if P:
            self.gs.theta = L.ptr(fp.gview("theta"))
        if RP:
            self.gs.rowp = L.ptr(self.g_rowp)

    def _feature_scratch(self, plan):
        """Device scratch of this engine alone: the step's workspace (NOT ops.workspace()'s cached buffer, which every
        one-shot ops.* call of the same shape on the same stream shares), the mean's and the MLPs' partial sums."""
        md = self.md
        self.ws = ops.new_workspace(self.N, self.D, self.M, md.S, md.nblk, md.P, md.RP, self.device, md.kernel, plan, md.lik)
        self.mean_ws = self.mlp_ws = None
        if self.mean == "linear":
            self.mean_ws, _ = ops._scratch(self.lib.tgp_mean_backward_workspace_bytes(self.N, self.D), self.device)
        elif self.mean == "identity":
            self.mean_forward()      # W is fixed: the rows' parameters are written once
        if self.mlp is not None:
            d = self.mlp.struct(self.N, True)
            self.mlp_ws = torch.empty(self.lib.tgp_mlp_workspace_bytes(d) // 8 + 16, dtype=torch.float64, device=self.device)

    def _selfcheck_collective(self, group, n=4099, seed=1234):
        """First contact with the node: the same seeded buffer (different on every rank) summed through tgp_allreduce_f64
        and through torch.distributed.all_reduce; the ABI collective is kept only if EVERY rank got the same sums to
        1e-15 relative (a ring and a tree add in different orders: not bitwise).  One host sync, before any capture."""
        g = torch.Generator(device="cpu").manual_seed(seed + self.rank)
        ref = torch.randn(n, generator=g, dtype=torch.float64).to(self.device)
        a, b = ref.clone(), ref.clone()
        self.comm.allreduce(a, n)
        torch.distributed.all_reduce(b, op=torch.distributed.ReduceOp.SUM, group=group)
        err = float(((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).cpu())
        ok = torch.tensor([1.0 if err <= 1e-15 * max(self.world_size, 1) else 0.0], dtype=torch.float64, device=self.device)
        torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=group)
        good = bool(ok.item() > 0.5)
        return good, "max rel diff %.1e on rank %d, all ranks %s" % (err, self.rank, "agree" if good else "do NOT agree")

    def close(self):
        """Destroy the communicator this engine created (one it was handed stays its owner's)."""
        if self.comm is not None and self._own_comm:
            with torch.cuda.device(self.device):
                self.comm.close()
        if self._own_comm:
            self.comm, self._own_comm = None, False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the launches of a step --------------------------------------------------------------------
    def elbo(self, phases=7):
        out = self.fp.out if self._out is None else self._out      # (ELBO, ELL, KL) of this step: see capture(unroll)
        rc = self.lib.tgp_elbo_step_phases_f64(self.md, L.ptr(self.X), L.ptr(self.Y), L.ptr(self.rowp),
                                               L.ptr(out), self.gs, None, None, L.ptr(self.status),
                                               L.ptr(self.ws), self.ws.numel() * 8, phases, L.stream_ptr())
        L.check(rc, "tgp_elbo_step_phases_f64")
        self._warm = True

    def step_adam(self, phases=0):
        """forward_backward() + adam() as one call (fused_adam engines): same kernels' arithmetic, same results.
        `phases` != 0: only those phases (the update rides in the backward phase)."""
        out = self.fp.out if self._out is None else self._out
        ad = L.TgpAdamArgs(*self._adam_args(0, self.n_plain), L.ptr(self.step_dev), 1, phases)      # (maximize = 1)
        rc = self.lib.tgp_elbo_step_adam_f64(self.md, L.ptr(self.X), L.ptr(self.Y), L.ptr(self.rowp), L.ptr(out), self.gs,
                                             None, None, L.ptr(self.status), L.ptr(self.ws), self.ws.numel() * 8, ad,
                                             L.stream_ptr())
        L.check(rc, "tgp_elbo_step_adam_f64")
        self._warm = True

    def allreduce(self):
        """allreduce_flat(), through the ABI's collective on this stream where the engine has one (it sums over one rank too)."""
        if self.comm is None:
            return allreduce_flat(self.fp.grad, self.fp.n, self.world_size, self.pg)
        pre_reduce(self.fp.grad, self.fp.n, self.world_size)
        with torch.cuda.device(self.device):
            self.comm.allreduce(self.fp.grad, self.fp.n + self.fp.extra)
        post_reduce(self.fp.grad, self.fp.n)

    def _adam_args(self, lo, hi):
        """Segment [lo, hi) of the flat buffer as the leading arguments of every Adam entry point, which are also the
        leading fields of tgp_adam_args: params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps."""
        fp = self.fp
        return (L.ptr(fp.data[lo:hi]), L.ptr(fp.grad[lo:hi]), L.ptr(fp.exp_avg[lo:hi]), L.ptr(fp.exp_avg_sq[lo:hi]), hi - lo,
                self.lr, self.betas[0], self.betas[1], self.eps)

    def optimal_qu(self):
        """m, Lam of the flat buffer <- the closed-form optimum at the buffer's hyper-parameters (tgp_optimal_qu_f64)."""
        fp = self.fp
        L.check(self.lib.tgp_optimal_qu_f64(self.md, L.ptr(self.X), L.ptr(self.Y), L.ptr(fp.view("m")), L.ptr(fp.view("Lam")),
                                            L.ptr(self.qu_status), L.ptr(self.qu_ws), self.qu_ws.numel() * 8, L.stream_ptr()),
                "tgp_optimal_qu_f64")

    def refresh_qu(self):
        """Collapsed engine: recompute the optimum for the hyper-parameters the last step left (outside the graph)."""
        if not self.collapsed:
            raise NotImplementedError("refresh_qu() belongs to ElboEngine(collapsed=True): an Adam engine trains q(u)")
        self.optimal_qu()

    def adam(self):
        if self.collapsed:          # every segment but m and Lam: [0, m) and [end of Lam, n), one counter each, in lock step
            fp = self.fp
            lo, hi = fp.offsets["m"], fp.offsets["Lam"] + fp.sizes["Lam"]
            self._adam_segment(0, lo, 0.0, self.step_dev)
            self._adam_segment(hi, fp.n, 0.0, self.step_tail)
            return
        rc = self.lib.tgp_adam_dev_groups_f64(*self._adam_args(0, self.fp.n), self.n_plain,
                                              self.nn_wd if self.mlp is not None else 0.0, L.ptr(self.step_dev), 1,
                                              L.stream_ptr())
        L.check(rc, "tgp_adam_dev_groups_f64")

    def mean_forward(self):
        """rowp[:, 0] = 1, rowp[:, 1] = m(x_n) from the flat buffer's a, b (or the fixed W)."""
        a = self.fp.view("mean_a") if self.mean == "linear" else self.mean_W
        b = self.fp.view("mean_b") if self.mean == "linear" else None
        L.check(self.lib.tgp_mean_forward_f64(L.ptr(self.X), self.N, self.D, L.ptr(a), L.ptr(b), 1.0, None, L.ptr(self.rowp), 2,
                                              1, 0, L.stream_ptr()), "tgp_mean_forward_f64")

    def mean_backward(self):
        """a_bar, b_bar from g_rowp[:, 1] (read in place) into the flat gradient."""
        fp = self.fp
        L.check(self.lib.tgp_mean_backward_f64(L.ptr(self.X), self.N, self.D, None, L.ptr(self.g_rowp), 2, 1,
                                               L.ptr(fp.gview("mean_a")), L.ptr(fp.gview("mean_b")), None, L.ptr(self.mean_ws),
                                               self.mean_ws.numel() * 8, L.stream_ptr()), "tgp_mean_backward_f64")

    def mlp_forward(self, step=None):
        if self.mlp is not None:
            d = self.mlp.struct(self.N, self.mlp_training)
            L.check(self.lib.tgp_mlp_forward_f64(d, L.ptr(self.X), L.ptr(self.fp.view("nn")),
                                                 L.ptr(self.step_dev if step is None else step), L.ptr(self.rowp),
                                                 L.stream_ptr()), "tgp_mlp_forward_f64")

    def mlp_backward(self, step=None):
        if self.mlp is not None:
            d = self.mlp.struct(self.N, self.mlp_training)
            L.check(self.lib.tgp_mlp_backward_f64(d, L.ptr(self.X), L.ptr(self.fp.view("nn")),
                                                  L.ptr(self.step_dev if step is None else step), L.ptr(self.g_rowp),
                                                  L.ptr(self.fp.gview("nn")), L.ptr(self.mlp_ws), self.mlp_ws.numel() * 8,
                                                  L.stream_ptr()), "tgp_mlp_backward_f64")

    def mlp_backward_adam(self, step):
        """MLP backward + Adam on the network weights (their own group: weight decay, own step counter) in the launch that
        reduces the weight gradients (tgp_mlp_backward_adam_f64): one launch less on the side chain of the rotated unit."""
        fp = self.fp
        lo, hi = fp.offsets["nn"], fp.n
        ad = L.TgpAdamArgs(*self._adam_args(lo, hi), L.ptr(step), 1, 0)
        d = self.mlp.struct(self.N, self.mlp_training)
        L.check(self.lib.tgp_mlp_backward_adam_f64(d, L.ptr(self.X), L.ptr(fp.data[lo:hi]), L.ptr(step), L.ptr(self.g_rowp),
                                                   L.ptr(fp.grad[lo:hi]), L.ptr(self.mlp_ws), self.mlp_ws.numel() * 8, ad,
                                                   float(self.nn_wd), L.stream_ptr()), "tgp_mlp_backward_adam_f64")

    def _adam_segment(self, lo, hi, weight_decay, step):
        rc = self.lib.tgp_adam_dev_f64(*self._adam_args(lo, hi), float(weight_decay), L.ptr(step), 1, L.stream_ptr())
        L.check(rc, "tgp_adam_dev_f64")

    def forward_backward(self):
        """MLPs -> fused ELBO step -> MLP backward: every gradient of the flat buffer is written.

        With MLPs the two halves that do not depend on each other run on a side stream: the MLP forward (needs X and
        the weights only) under the M x M prepare phase (K_MM, Cholesky, KL), and the MLP backward (needs d/d rowp from
        the row kernel only) under the M x M adjoint.  Fork and join are event waits, valid under graph capture."""
        if self.mean == "linear":
            self.mean_forward()
            self.elbo()
            self.mean_backward()
            return
        if self.collapsed:
            self.optimal_qu()
            self.elbo()
            return
        if self.mlp is None:
            self.elbo()
            return
        self._forked(lambda: self.elbo(1), self.mlp_forward)     # prepare
        self.elbo(2)                                             # rows: consumes rowp, produces g_rowp
        self._forked(lambda: self.elbo(4), self.mlp_backward)    # M x M adjoint + gradient assembly

    def _forked(self, main_chain, side_chain):
        """main_chain() on the current stream with side_chain() beside it on the side stream, joined at the end.  The main
        chain is issued first: it is the longer one, and under graph replay ready nodes are dispatched in creation order --
        see _rotated_unit()."""
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        forked = torch.cuda.Event()
        forked.record(main)
        main_chain()
        self._side.wait_event(forked)
        with torch.cuda.stream(self._side):
            side_chain()
        main.wait_stream(self._side)

    # ---- THE step: pre -> (step_adam | forward_backward -> all-reduce -> adam) -> post, stated once, in two halves that meet
    # at the all-reduce.  step(), the "full" and the unrolled graphs run _one_step(); "split" records the halves as two graphs.
    def _to_the_reduce(self, split=False):
        if self.pre_step is not None:
            self.pre_step()
        (self.step_adam if self.fused_adam else self.forward_backward)()     # step_adam: the whole step, update included
        if split:
            pre_reduce(self.fp.grad, self.fp.n, self.world_size)

    def _from_the_reduce(self, split=False):
        if split:
            post_reduce(self.fp.grad, self.fp.n)
        if not self.fused_adam:
            self.adam()
        if self.post_step is not None:
            self.post_step()

    def _one_step(self):
        self._to_the_reduce()
        if not self.fused_adam:
            self.allreduce()
        self._from_the_reduce()

    def step(self):
        # ("rotated": the captured unit straddles two steps: eager steps would repeat half of one)
        return self.replay() if self.graph == "rotated" else self._one_step()

    # ---- HIP graph ----------------------------------------------------------------------------------
    def _graph_of(self, fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
            fn()
        return g

    def capture(self, with_allreduce=None, unroll=None, unroll_long=None):
        """Capture one full step.  With world_size > 1 the all-reduce stays outside (two graphs) unless
        with_allreduce=True.  `unroll` / `unroll_long`: steps per launch of the unrolled graphs (_capture_unrolled)."""
        if not self._warm:
            self.forward_backward()          # first launch sets kernel attributes; must happen outside capture
        torch.cuda.synchronize()
        if (self.mlp is not None and self.world_size == 1 and self.comm is None and self.pipeline_steps
                and self.pre_step is None):
            self.step_nn = self.step_dev.clone()
            self.elbo(1)                     # prepare(0) and MLP forward(0) run here, eagerly, once
            self.mlp_forward(self.step_nn)
            torch.cuda.synchronize()
            self.g1 = self._graph_of(self._rotated_unit)
            self._capture_unrolled(self._rotated_unit, unroll, unroll_long)
            self.graph = "rotated"
        elif self.world_size > 1 and not with_allreduce and self.comm is None:
            # [graph 1: step kernels + KL pre-division] -> RCCL all-reduce -> [graph 2: ELBO fix-up + Adam]
            self.g1 = self._graph_of(lambda: self._to_the_reduce(split=True))
            self.g2 = self._graph_of(lambda: self._from_the_reduce(split=True))
            self.graph = "split"
        else:
            self.g1 = self._graph_of(self._one_step)
            if self.world_size == 1 or self.comm is not None:   # (the ABI's all-reduce is a node of the graph like any kernel)
                self._capture_unrolled(self._one_step, unroll, unroll_long)
            self.graph = "full"

    def _rotated_unit(self):
        """ID_TGP on one rank: a different SCHEDULE of the step's operations, not a restatement of _one_step().  The long pole
        of an ID_TGP step is the MLP backward (97 us), and nothing of step t depends on it except the network weights' own Adam
        update and the NEXT step's MLP forward.  So the captured unit starts
        at the row kernel:   main: rows(t) -> M x M adjoint(t) -> Adam(GP params) -> prepare(t+1)
                             side:            MLP backward(t) -> Adam(network weights) -> MLP forward(t+1)
        joined at the end.  Same operations in the same per-step order as _one_step(); capture() runs prepare(0) and MLP
        forward(0).  Two device step counters (one per Adam group; the dropout masks follow the network group's) keep both
        launches graph-replayable."""
        self.elbo(2)

        # The main chain is issued BEFORE the side branch: graph replay dispatches ready nodes in creation order,
        # and with the MLP backward (408 workgroups) created first the slab reduction that heads the critical
        # chain found every CU taken (5 -> 12 us; the whole step 172 -> 150 us with this order).
        def main_chain():
            if self.fused_update:
                self.step_adam(4)            # M x M adjoint + gradient assembly + Adam on the GP / flow parameters
            else:
                self.elbo(4)
                self._adam_segment(0, self.n_plain, 0.0, self.step_dev)
            self.elbo(1)

        def side_chain():
            if self.fused_update:
                self.mlp_backward_adam(self.step_nn)     # backward + Adam on the network weights, one launch less
            else:
                self.mlp_backward(self.step_nn)
                self._adam_segment(self.n_plain, self.fp.n, self.nn_wd, self.step_nn)
            self.mlp_forward(self.step_nn)
        self._forked(main_chain, side_chain)

    def _capture_unrolled(self, unit, unroll, unroll_long=None):
        """A second graph of U consecutive steps (one rank only).  Launching a graph costs ~5 us of idle GPU between two
        replays of the launch chain (14 us with the two-stream ID_TGP unit): U steps per launch pay it once (Power TGP
        129.5 -> 125 us per step at U = 8-10, ID_TGP 148 -> 141).  The same kernels in the same order: results are
        bit-identical to U single-step replays.  The scalars of the first U - 1 steps go to self.hist_u (the step's `out`
        argument is redirected: no copy node), the last step's to fp.out as always.
        With the default U (no explicit `unroll`) a THIRD graph of 4 U steps serves long runs (round 5, Power TGP at 96 us per
        step: 10 406 steps/s at 10 steps per launch, 10 470 at 40); replay_many uses the longest graph that still fits, so a
        20-step run is two replays of the U-step graph as before."""
        U = int(unroll if unroll is not None else 10)
        self.unroll, self.gU = 1, None
        self.unroll_long, self.gL, self.hist_l = 1, None, None
        if U < 2 or (unroll is None and self.M > 128):      # general-M steps take milliseconds: nothing to gain, ~100 nodes each
            return
        # With a collective in the unit the step's scalars must stay where allreduce() / pre_reduce / post_reduce act on
        # them -- behind the gradients in fp.grad -- and reach hist_u by a captured 4-double copy AFTER the reduction; the
        # redirected `out` of the single-rank form would log rank-local, un-reduced values (and re-sum a stale slot).
        reduced = self.comm is not None or self.world_size > 1

        def capture_steps(nsteps):
            hist = torch.zeros(nsteps - 1, 4, dtype=torch.float64, device=self.device)

            def steps():
                for u in range(nsteps):
                    self._out = hist[u] if (u < nsteps - 1 and not reduced) else None
                    unit()
                    if reduced and u < nsteps - 1:
                        hist[u].copy_(self.fp.out)
            try:
                return self._graph_of(steps), hist
            finally:
                self._out = None        # a failed capture must not leave later steps writing their scalars into the history

        self.gU, self.hist_u = capture_steps(U)
        self.unroll = U
        UL = int(unroll_long) if unroll_long is not None else (4 * U if unroll is None else 0)
        if UL > U and not reduced:
            self.gL, self.hist_l = capture_steps(UL)
            self.unroll_long = UL

    def replay_many(self, n, hist=None, row0=0):
        """n steps: replays of the longest unrolled graph that fits, then of the U-step one, the rest one by one.
        hist[row0 + i] <- (ELBO, ELL, KL) of step i (device-to-device copies between replays, nothing synchronises)."""
        k = 0
        for g, U, hu in ((self.gL, self.unroll_long, self.hist_l), (self.gU, self.unroll, self.hist_u)):
            while g is not None and n - k >= U:
                g.replay()
                if hist is not None:
                    hist[row0 + k:row0 + k + U - 1].copy_(hu[:, :3])
                    hist[row0 + k + U - 1].copy_(self.fp.out[:3])
                k += U
        while k < n:
            self.replay()
            if hist is not None:
                hist[row0 + k].copy_(self.fp.out[:3])
            k += 1

    def replay(self):
        self.g1.replay()
        if self.graph == "split":
            torch.distributed.all_reduce(self.fp.grad, op=torch.distributed.ReduceOp.SUM, group=self.pg)
            self.g2.replay()

    # ---- bookkeeping ---------------------------------------------------------------------------------
    def check_status(self):
        """Lazy Cholesky check (one sync): raises like the reference's psd_safe_cholesky would."""
        if self.collapsed:
            sq = self.qu_status.cpu()
            if ops.raise_for_status(sq):
                raise ops.NotPSDError("K_MM not positive definite at pivot %d in the optimal q(u) of the last step (no jitter "
                                      "ladder there): train q(u) by Adam, or raise the model's jitter" % int(sq[0]))
        st = self.status.cpu()
        failed = ops.raise_for_status(st)       # an expired hand-off wait (sticky across a replayed graph's steps), NaN in K_MM
        if int(st[2]) > self._warned_jitter:
            self._warned_jitter = int(st[2])
            warnings.warn("A not p.d., added jitter of %g to the diagonal" % (self.md.jitter_ladder * 10 ** (int(st[2]) - 1)),
                          ops.NumericalWarning)
        if failed:
            raise ops.NotPSDError("K_MM not positive definite at pivot %d even with the largest jitter of the ladder "
                                  "(%g), like psd_safe_cholesky's final raise (dsp/utils.py:268-269)"
                                  % (int(st[0]), self.md.jitter_ladder * 100))

    def scalars(self):
        o = self.fp.out.cpu()
        return float(o[0]), float(o[1]), float(o[2])

    def set_lr(self, lr):
        self.lr = float(lr)          # a launch argument: re-capture afterwards


class MinibatchEngine:
    """The reference's minibatch loop (trainers/trainer_base.py:322-349 over a DataLoader(batch_size, shuffle,
    drop_last=False), code/main.py:74) with the data set resident in HBM and every step replayed from a HIP graph.

    * X, Y stay on the device; one epoch's row order is an int32 index buffer written once per epoch (`set_order`);
    * a captured step = [tgp_gather_rows_f64: batch rows -> fixed batch buffers, device cursor advanced by the launch]
      -> the ElboEngine step (ELBO + backward + Adam) on those buffers;
    * the ragged last batch of an epoch (N mod B rows) has its own engine + graph (and workspace) on the same flat
      parameter / Adam buffers (the ELL scale N_total / MB follows the batch's own size, sparse_MF_SP.py:623-626);
    * the three logged scalars of every step are copied device-to-device into a history buffer; nothing syncs.
    With world_size > 1 each rank gathers and processes its row shard of every batch (one all-reduce per step)."""

    def __init__(self, X, Y, params, N_total, batch_size, device="cuda:0", world_size=1, rank=0, **engine_kw):
        mean = engine_kw.get("mean")
        _refuse(is_whiten=engine_kw.get("is_whiten", True), mean=None if mean is None else mean[0],
                likelihood=engine_kw.get("likelihood"), world_size=world_size, collective=engine_kw.get("collective"),
                per_row=engine_kw.get("mlp") is not None or engine_kw.get("rowp") is not None, minibatch=True,
                kernel=engine_kw.get("kernel"))
        self.device = torch.device(device)
        self.lib = L.load()
        self.X = X.to(self.device, torch.float64).contiguous()
        self.Y = Y.reshape(-1).to(self.device, torch.float64).contiguous()
        self.N, self.D = self.X.shape
        self.B = int(min(batch_size, self.N))
        self.nfull, self.rest = divmod(self.N, self.B)
        self.steps_per_epoch = self.nfull + (1 if self.rest else 0)
        self.world_size, self.rank = int(world_size), int(rank)
        self.index = torch.arange(self.N, dtype=torch.int32, device=self.device)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.has_order = False
        lo, hi = shard_rows(self.B, world_size, rank)
        self.Xb = torch.zeros(hi - lo, self.D, dtype=torch.float64, device=self.device)
        self.Yb = torch.zeros(hi - lo, dtype=torch.float64, device=self.device)
        self.full = ElboEngine(self.Xb, self.Yb, params, N_total, device=self.device, world_size=world_size, rank=rank,
                               mb_global=self.B, **engine_kw)
        self.full.pipeline_steps = False
        self.full.pre_step = self._gather(lo, hi - lo, self.B)
        self.last = None
        if self.rest:
            lo2, hi2 = shard_rows(self.rest, world_size, rank)
            kw = dict(engine_kw)
            kw.pop("mlp_weights", None)
            self.last = ElboEngine(self.Xb[:hi2 - lo2], self.Yb[:hi2 - lo2], params, N_total, device=self.device,
                                   world_size=world_size, rank=rank, mb_global=self.rest, share=self.full,
                                   mlp_weights=(self.full.fp.view("nn") if self.full.mlp is not None else None), **kw)
            self.last.pipeline_steps = False
            self.last.pre_step = self._gather(lo2, hi2 - lo2, self.rest)
        self.fp = self.full.fp

    def _gather(self, offset, nrows, advance):
        def run():
            rc = self.lib.tgp_gather_rows_f64(L.ptr(self.X), L.ptr(self.Y), self.N, self.D,
                                              L.ptr(self.index) if self.has_order else None, L.ptr(self.cursor), offset, nrows,
                                              advance, self.N, L.ptr(self.Xb), L.ptr(self.Yb), L.stream_ptr())
            L.check(rc, "tgp_gather_rows_f64")
        return run

    def set_order(self, perm=None):
        """Row order of the coming epoch (a permutation of range(N), host or device; None = stored order).  Must be
        called before capture() with the kind of order (permuted or not) the run will use: the index pointer is a launch
        argument of the captured gather."""
        if perm is None:
            if self.has_order:
                self.index.copy_(torch.arange(self.N, dtype=torch.int32, device=self.device))
        else:
            self.has_order = True
            self.index.copy_(perm.to(torch.int32), non_blocking=True)
        self.cursor.zero_()

    def capture(self):
        self.full.capture(unroll=1)      # steps are replayed one by one (per-step history copies, the ragged last batch)
        if self.last is not None:
            self.last.capture(unroll=1)

    def run_epoch(self, hist=None, row0=0, replay=True):
        """One pass over the data: nfull full batches + the ragged one.  hist[row0 + i] <- (ELBO, ELL, KL) of step i."""
        for i in range(self.steps_per_epoch):
            eng = self.full if i < self.nfull else self.last
            (eng.replay if (replay and eng.graph is not None) else eng.step)()
            if hist is not None:
                hist[row0 + i].copy_(eng.fp.out[:3])
        return self.steps_per_epoch

    def check_status(self):
        self.full.check_status()

    @property
    def lr(self):
        return self.full.lr

    def set_lr(self, lr):
        self.full.set_lr(lr)
        if self.last is not None:
            self.last.set_lr(lr)
