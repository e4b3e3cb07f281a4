"""Trainer with the reference's constructor/`train`/`compute_metrics` surface
(code/dsp/trainers/trainer_base.py:250-391, trainers_regression.py:30-338).

Per minibatch: model.set_is_training(True) -> loss = -ELBO -> zero_grad -> backward -> optimizer.step()
(trainer_base.py:334-345), Adam lr as given, `optimisation_schedule` = (percentages, specifications) with
specifications entries [lr, name_substring] or [lr, weight_decay, name_substring] (main.py:274-298 puts the
'NNets' weights in a weight-decay group).  Data stay wherever the loader yields them; use data.DeviceLoader
to keep the split resident in HBM (removes the reference's per-step H2D copy and per-row collation).
`inference_in_cpu` is accepted for signature compatibility and ignored: metrics are computed on the GPU.
"""
import math
import time
from collections import OrderedDict

import numpy
import torch

from . import config as cg


def return_optimizer(opt, parameters, lr):
    """dsp/trainers/optimizers.py:10-22."""
    if opt == "adam":
        return torch.optim.Adam(parameters, lr, amsgrad=False)
    if opt == "adam_W":
        return torch.optim.AdamW(parameters, lr, amsgrad=False)
    if opt == "sgd":
        return torch.optim.SGD(parameters, lr)
    raise ValueError("opt must be adam, adam_W or sgd")


class Trainer_SP_regression:
    def __init__(self, model, data_loaders, validate_each, plot, track, Y_std, plot_each, S_test,
                 inference_in_cpu=False, coverage="sampled", qu="adam", natgrad_lr=1.0):
        self.model = model
        # q(u): "adam" = m and Lam are trained like every other parameter (the reference); "optimal" = they are set to their
        # closed-form optimum before every step and every evaluation and the optimiser trains the hyper-parameters on the
        # collapsed bound (models.collapsed_bound: Gaussian and warped likelihoods, whitened, one full batch per epoch);
        # "natgrad" = every minibatch opens with one natural-gradient step of q(u) at step size natgrad_lr
        # (models.natgrad_step_qu: any likelihood of one whitened latent GP, any number of minibatches -- natgrad_lr < 1 when
        # there is more than one), then the optimiser trains the other parameters on the ELBO, in the eager loop
        if qu not in ("adam", "optimal", "natgrad"):
            raise ValueError("qu must be 'adam', 'optimal' or 'natgrad', got %r" % (qu,))
        self.qu = qu
        self.natgrad_lr = float(natgrad_lr)
        if qu == "natgrad":
            why = model._natgrad_refusal() if hasattr(model, "_natgrad_refusal") else "the model has no natgrad_step_qu"
            if why is not None:
                raise NotImplementedError("qu='natgrad': " + why)
            if not 0.0 < self.natgrad_lr <= 1.0:
                raise ValueError("natgrad_lr must be in (0, 1], got %r" % (natgrad_lr,))
        if qu == "optimal":
            why = model._qu_refusal() if hasattr(model, "_qu_refusal") else "the model has no set_optimal_qu"
            if why is not None:
                raise NotImplementedError("qu='optimal': " + why)
            if len(data_loaders[0]) != 1:
                raise NotImplementedError("qu='optimal' takes one full batch per epoch: the optimum of q(u) belongs to the rows "
                                          "it was computed from (minibatch collapsed steps are not built)")
        # coverage of the 95 % interval: "sampled" = order statistics of S_test predictive draws per row, on the host (the
        # reference, trainers_regression.py:171); "exact" = the 2.5 % / 97.5 % roots of the predictive CDF, on the device
        if coverage not in ("sampled", "exact"):
            raise ValueError("coverage must be 'sampled' or 'exact', got %r" % (coverage,))
        self.coverage = coverage
        self._coverage_fallback_said = False
        self._scores_fallback_said = False
        # [train], [train, test] or [train, valid, test] (trainer_base.py:50-59)
        dl = list(data_loaders)
        self.train_loader, self.valid_loader, self.test_loader = dl[0], None, None
        if len(dl) == 3:
            self.valid_loader, self.test_loader = dl[1], dl[2]
        elif len(dl) == 2:
            self.test_loader = dl[1]
        self.is_valid, self.is_test = self.valid_loader is not None, self.test_loader is not None
        self.num_outputs = model.out_dim
        self.validate_each = validate_each
        self.S_test = S_test
        self.inference_in_cpu = inference_in_cpu
        if inference_in_cpu:
            # the reference moves the model to the CPU for compute_metrics (trainers_regression.py:321-338); the product has
            # no CPU implementation, so the flag is accepted and metrics stay on the GPU -- said once, not silently
            print("[tgp.pytorch_amd] inference_in_cpu=True ignored: metrics are computed on the GPU (no CPU path in this package)")
        assert len(Y_std.shape) == 1 and Y_std.shape[0] == self.num_outputs
        self.Y_std = Y_std
        self.optimizer = None
        self._engine = None
        self._names_added = []
        self.loss_arr, self.ELL_arr, self.KLD_arr = [], [], []
        self.total_trainer_epochs = 0

    # ---- optimiser groups (trainer_base.py:106-248) ---------------------------------------------------
    def _param_groups(self, specs, lr_all, already_added=()):
        """Parameter groups of one schedule stage.  `specs` entries are [lr, name_substring] or [lr, weight_decay,
        name_substring]; parameters no entry names take (lr_all, 0).  lr == 0.0 freezes: the parameter joins no group
        (and, with a kept optimiser, stays free to be added by a later stage).  `already_added`: names a kept optimiser
        holds already (keep_parameter_groups=True) -- skipped, and naming one again is an error like in the reference.
        Returns (groups, names placed in them)."""
        named = OrderedDict(self.model.named_parameters())
        if self.qu in ("optimal", "natgrad"):    # q(u) is set in closed form here: no optimiser holds it
            named = OrderedDict((n, q) for n, q in named.items() if not n.startswith("q_U."))
        taken, frozen, groups, placed = set(), set(), [], []
        seen_keys = set()
        for sp in (specs or []):
            if len(sp) == 3:
                lr, wd, key = sp
            elif len(sp) == 2:
                (lr, key), wd = sp, 0.0
            else:
                raise ValueError("Unvalid argument optimisation_schedule. Parameters should be specified as lr, param or "
                                 "lr, weight_decay, param")
            if key in seen_keys:
                raise ValueError("Parameter {} already added to the parameter list".format(key))
            seen_keys.add(key)
            names = [n for n in named if key in n]
            for n in names:
                if n in taken and lr != 0.0:
                    raise ValueError("Got repeated parameter {}".format(n))
                if n in already_added:
                    raise ValueError("Got repeated parameter {} with root {}. This parameter already belongs to a "
                                     "parameter group".format(n, key))
            if lr == 0.0:
                frozen.update(names)
                continue
            taken.update(names)
            if names:
                for g in groups:
                    if g["lr"] == lr and g["weight_decay"] == wd:
                        g["params"] += [named[n] for n in names]
                        break
                else:
                    groups.append({"params": [named[n] for n in names], "lr": lr, "weight_decay": wd})
                placed += names
        rest = [n for n in named if n not in taken and n not in frozen and n not in already_added]
        if rest:
            groups.append({"params": [named[n] for n in rest], "lr": lr_all, "weight_decay": 0.0})
            placed += rest
        return groups, placed

    # ---- resident fast path ---------------------------------------------------------------------------
    def _engine_for(self, groups, lr_ALL, opt):
        """The resident step engine (engine.ElboEngine: the same ELBO -> backward -> Adam sequence as the loop below, every
        launch captured in a HIP graph, no host synchronisation per step) when the run is what main.py sets up: Adam with
        one learning rate, weight decay on the 'NNets' group only, one full batch per epoch from a data.DeviceLoader.
        The model's nn.Parameters are re-pointed at the engine's flat buffer, so the modules stay the parameter holders
        and everything downstream (metrics, prediction, state_dict) sees the trained values.  Returns None otherwise: what
        the engines themselves do not cover is engine.engine_refusal's to say (this trainer is one rank); the conditions here
        are the run's -- optimiser, groups, frozen parameters, loader."""
        from .data import DeviceLoader
        from .engine import ElboEngine, MinibatchEngine, engine_refusal
        from .flow import compile_flow, mlp_spec, stack_theta
        if not getattr(cg, "use_step_engine", True) or opt != "adam":
            return None
        if self.qu == "optimal":
            return self._collapsed_engine_for(groups, lr_ALL)
        if self.qu == "natgrad":         # the step engines hold no natural-gradient step: the eager loop
            return None
        ld = self.train_loader
        if not isinstance(ld, DeviceLoader) or not ld.X.is_cuda or ld.Y.shape[1] != 1:
            return None
        model = self.model
        mean_fn = model.mean_function if getattr(model, "_has_mean", False) else None
        lik = getattr(model.likelihood, "engine_name", None)
        cover = dict(is_whiten=getattr(model, "is_whiten", True), mean=None if mean_fn is None else mean_fn.name, likelihood=lik,
                     minibatch=len(ld) != 1, kernel=getattr(getattr(model, "covariance_function", None), "hip_kernel", None))
        if engine_refusal(**cover) is not None:        # (before the flow is compiled: whether it is input-dependent comes below)
            return None
        if not hasattr(model, "_gp_params") or any(g["lr"] != lr_ALL for g in groups):
            return None
        # the engine updates EVERY parameter of its flat buffer: a stage that freezes some (lr = 0.0 entries,
        # trainer_base.py:155-179) or leaves some to a later stage must take the torch optimiser
        if {id(q) for g in groups for q in g["params"]} != {id(q) for q in model.parameters()}:
            return None
        nets, theta_list, blocks = [], [], None
        warped = getattr(model.likelihood, "flow_on_targets", False)
        if getattr(model.likelihood, "has_flow", True):
            spec, theta_list, nets = compile_flow(model.likelihood.flow[0] if warped else model.G_matrix[0])
            blocks = spec.blocks
        if engine_refusal(per_row=bool(nets), **cover) is not None:
            return None
        nn_params = [p for net in nets for p in net.parameters()]
        nn_ids = {id(p) for p in nn_params}
        wd = 0.0
        for g in groups:
            if g["weight_decay"] != 0.0:
                if {id(p) for p in g["params"]} != nn_ids or wd != 0.0:
                    return None
                wd = g["weight_decay"]
        mspec = mlp_spec(nets, seed=cg.config_seed) if nets else None
        if nets and mspec is None:
            return None
        Z, rl, ro, m, Lam, lvn = model._gp_params()
        params = {"Z": Z.detach(), "raw_lengthscale": rl.detach(), "raw_outputscale": ro.detach(), "m": m.detach(),
                  "Lam": Lam.detach(), "log_var_noise": lvn.detach()}
        if theta_list:
            params["theta"] = stack_theta(theta_list)
        W = torch.cat([p.detach().reshape(-1) for p in nn_params]) if nn_params else None
        kw = dict(flow_blocks=blocks, S=getattr(model, "quad_points", None), lr=lr_ALL,
                  kernel=model.covariance_function.hip_kernel, mlp=mspec, mlp_weights=W, nn_weight_decay=wd, mlp_training=True,
                  jitter_ladder=cg.global_jitter if cg.global_jitter is not None else 1e-8)
        if warped:
            kw["likelihood"] = "warped"
        if mean_fn is not None:
            a, b = mean_fn._ab()
            kw["mean"] = (mean_fn.name, a.detach(), None if b is None else b.detach())
            if blocks is None:           # Gaussian likelihood: the engine's quadrature over the affine block alone, exact at any S >= 2
                kw["S"] = None
        if len(ld) == 1:
            eng = ElboEngine(ld.X, ld.Y, params, float(model.N), device=ld.X.device, **kw)
        else:
            # several minibatches per epoch (the Airline recipe, main.py:74): rows gathered on the device by index,
            # one captured step per batch size (full batches + the ragged last one), see engine.MinibatchEngine
            eng = MinibatchEngine(ld.X, ld.Y, params, float(model.N), ld.batch_size, device=ld.X.device, **kw)
            eng.has_order = bool(ld.shuffle)
        # the modules' parameters become views of the engine's flat buffer
        fp, k = eng.fp, model.covariance_function
        with torch.no_grad():
            model.Z.data = fp.view("Z").view_as(model.Z)
            k.base_kernel.raw_lengthscale.data = fp.view("raw_ls").view_as(k.base_kernel.raw_lengthscale)
            k.raw_outputscale.data = fp.view("raw_os").view_as(k.raw_outputscale)
            model.q_U.variational_mean.data = fp.view("m").view_as(model.q_U.variational_mean)
            model.q_U.chol_variational_covar.data = fp.view("Lam").view_as(model.q_U.chol_variational_covar)
            model.likelihood.log_var_noise.data = fp.view("lvn").view_as(model.likelihood.log_var_noise)
            for i, p in enumerate(theta_list):
                p.data = fp.view("theta")[i:i + 1].view_as(p)
            if mean_fn is not None and mean_fn.name == "linear":
                mean_fn.a.data = fp.view("mean_a").view_as(mean_fn.a)
                mean_fn.b.data = fp.view("mean_b").view_as(mean_fn.b)
            o = 0
            for p in nn_params:
                p.data = fp.view("nn")[o:o + p.numel()].view_as(p)
                o += p.numel()
        eng.capture()
        return eng

    def _collapsed_engine_for(self, groups, lr_ALL):
        """qu="optimal": the collapsed step engine (engine.ElboEngine(collapsed=True): optimal q(u) -> the unchanged step -> Adam
        on the hyper-parameters, captured) for the Gaussian likelihood with a zero mean on one full batch from a
        data.DeviceLoader, every parameter but q(u) trained at one learning rate.  None otherwise: the eager loop
        (models.collapsed_bound + the torch optimiser) then serves the run."""
        from .data import DeviceLoader
        from .engine import ElboEngine, collapsed_refusal, engine_refusal
        ld, model = self.train_loader, self.model
        if engine_refusal(kernel=model.covariance_function.hip_kernel) is not None:
            return None
        if not isinstance(ld, DeviceLoader) or not ld.X.is_cuda or ld.Y.shape[1] != 1 or len(ld) != 1:
            return None
        mean_fn = model.mean_function if model._has_mean else None
        if collapsed_refusal(likelihood="warped" if getattr(model.likelihood, "flow_on_targets", False) else None,
                             mean=None if mean_fn is None else (mean_fn.name,)) is not None:
            return None
        if any(g["lr"] != lr_ALL or g["weight_decay"] != 0.0 for g in groups):
            return None
        if {id(q) for g in groups for q in g["params"]} != {id(q) for n, q in model.named_parameters() if not n.startswith("q_U.")}:
            return None
        Z, rl, ro, m, Lam, lvn = model._raw_params()
        params = {"Z": Z.detach(), "raw_lengthscale": rl.detach(), "raw_outputscale": ro.detach(), "m": m.detach(),
                  "Lam": Lam.detach(), "log_var_noise": lvn.detach()}
        eng = ElboEngine(ld.X, ld.Y, params, float(model.N), device=ld.X.device, lr=lr_ALL,
                         kernel=model.covariance_function.hip_kernel,
                         jitter_ladder=cg.global_jitter if cg.global_jitter is not None else 1e-8, collapsed=True)
        fp, k = eng.fp, model.covariance_function
        with torch.no_grad():
            model.Z.data = fp.view("Z").view_as(model.Z)
            k.base_kernel.raw_lengthscale.data = fp.view("raw_ls").view_as(k.base_kernel.raw_lengthscale)
            k.raw_outputscale.data = fp.view("raw_os").view_as(k.raw_outputscale)
            model.q_U.variational_mean.data = fp.view("m").view_as(model.q_U.variational_mean)
            model.q_U.chol_variational_covar.data = fp.view("Lam").view_as(model.q_U.chol_variational_covar)
            model.likelihood.log_var_noise.data = fp.view("lvn").view_as(model.likelihood.log_var_noise)
        eng.capture()
        return eng

    def refresh_qu(self):
        """qu="optimal": q(u) <- its optimum at the current hyper-parameters, on the training rows (before every evaluation; the
        last training step left the optimum of the hyper-parameters it started from)."""
        if self.qu != "optimal":
            return
        if self._engine is not None:
            self._engine.refresh_qu()
            return
        for x, y in self.train_loader:
            self.model.set_optimal_qu(x.to(cg.device), y.to(cg.device))

    def _train_resident(self, eng, n_epochs, epochs_total):
        from .engine import MinibatchEngine
        mb = isinstance(eng, MinibatchEngine)
        spe = eng.steps_per_epoch if mb else 1          # optimiser steps per epoch
        hist = torch.empty(max(n_epochs * spe, 1), 3, dtype=torch.float64, device=eng.device)
        t0 = time.time()
        last = 0
        ep_done = 0
        for ep in range(n_epochs):
            if mb:
                # the loader's own permutation stream (torch RandomSampler semantics), written to the device once per
                # epoch; the batches are then gathered by index inside the captured steps
                eng.set_order(self.train_loader.epoch_permutation())
                eng.run_epoch(hist, ep * spe)
            elif ep >= ep_done:
                # one full-batch step per epoch: all epochs up to the next report in as few graph launches as the engine's
                # unrolled graph allows (engine.replay_many); the scalars of every step land in `hist` on the device
                nxt = n_epochs if self.validate_each <= 0 else min(n_epochs, (ep // self.validate_each + 1) * self.validate_each)
                eng.replay_many(nxt - ep, hist, ep)
                ep_done = nxt
            self.total_trainer_epochs += 1
            if self.validate_each > 0 and (ep + 1) % self.validate_each == 0:
                h = hist[last * spe:(ep + 1) * spe].mean(0).cpu()     # the only host sync: once per `validate_each` epochs
                eng.check_status()                      # a failed Cholesky surfaces here, not thousands of epochs later
                print("| Epoch [{}/{}] ELBO {:.5f} ELL {:.5f} KLD {:.5f} ({:.3f}s)".format(
                    ep + 1, epochs_total, float(h[0]), float(h[1]), float(h[2]), time.time() - t0))
                t0, last = time.time(), ep + 1
        eng.check_status()
        h = hist[:n_epochs * spe].cpu()
        self.loss_arr += (-h[:, 0]).tolist()
        self.ELL_arr += h[:, 1].tolist()
        self.KLD_arr += h[:, 2].tolist()

    def ELBO_call(self, x, y):
        if self.qu == "optimal":
            loss, elogl, kld = self.model.collapsed_bound(x, y)
        elif self.qu == "natgrad":
            # one step of q(u), then the ELBO with q(u) as a constant at the jitter the step ended with (as collapsed_bound does):
            # the backward computes nothing for q_U, whose .grad no optimiser would ever clear
            info = self.model.natgrad_step_qu(x, y, lr=self.natgrad_lr)
            loss, elogl, kld = self.model.ELBO(x, y, _qu_jitter=info["jitter"])
        else:
            loss, elogl, kld = self.model.ELBO(x, y)
        loss = -loss
        self.param_elbo = [loss, elogl, kld]
        return loss

    def train(self, epochs, lr_ALL, opt, keep_parameter_groups, lr_groups=None, optimisation_schedule=None):
        """trainer_base.py:250-361.  keep_parameter_groups=True keeps the optimiser (its groups and moments) across
        stages and calls: later stages ADD the groups of parameters not yet held, earlier groups take `lr_groups` (or
        lr_ALL).  keep_parameter_groups=False starts from a fresh optimiser and re-creates it at every stage."""
        if optimisation_schedule is None:
            optimisation_schedule = ([1.0], [None])
        percentages, specifications = optimisation_schedule
        if abs(sum(percentages) - 1.0) > 1e-12:
            raise ValueError("percentages must sum 1, got {}".format(sum(percentages)))
        if len(percentages) != len(specifications):
            raise ValueError("Percentages and specifications must have same length")
        if keep_parameter_groups:
            if self.optimizer is None and self._engine is None:
                self._names_added = []
            elif self.optimizer is not None:
                if lr_groups is not None and len(lr_groups) != len(self.optimizer.param_groups):
                    raise ValueError("The provided `lr_groups` {} does not match the number of parameter groups in the "
                                     "optimizer {}".format(lr_groups, len(self.optimizer.param_groups)))
                for g, lr_i in zip(self.optimizer.param_groups, lr_groups or [lr_ALL] * len(self.optimizer.param_groups)):
                    g["lr"] = lr_i
            elif lr_groups is not None and any(v != lr_ALL for v in lr_groups):
                raise ValueError("the resident step engine holds one learning rate: pass lr_groups=None (or all equal to "
                                 "lr_ALL), or set config.use_step_engine = False")
        else:
            self.optimizer, self._engine, self._names_added = None, None, []
        single = len(percentages) == 1
        for per, specs in zip(percentages, specifications):
            fresh = not keep_parameter_groups or (self.optimizer is None and self._engine is None)
            groups, placed = self._param_groups(specs, lr_ALL, () if fresh else self._names_added)
            n_ep = int(epochs * per)
            if self._engine is not None and not fresh:
                if groups:
                    raise ValueError("the resident step engine already trains every parameter; new groups cannot be added")
                if self._engine.lr != float(lr_ALL):       # the learning rate is a launch argument of the captured step
                    self._engine.set_lr(float(lr_ALL))
                    self._engine.capture()
                self._train_resident(self._engine, n_ep, epochs)
                continue
            if fresh:
                self._engine = self._engine_for(groups, lr_ALL, opt) if single else None
                self._names_added = list(placed) if keep_parameter_groups else []
                if self._engine is not None:
                    self._train_resident(self._engine, n_ep, epochs)
                    continue
                self.optimizer = return_optimizer(opt, groups, lr_ALL)
            else:
                for g in groups:
                    self.optimizer.add_param_group(g)
                self._names_added += placed
            self._train_eager(n_ep, epochs)
        self.refresh_qu()
        if not keep_parameter_groups:
            self.optimizer = None
            self._engine = None

    def _train_eager(self, n_epochs, epochs_total):
        """The reference's loop as is: per minibatch ELBO -> zero_grad -> backward -> optimizer.step
        (trainer_base.py:329-349), autograd through ops.ElboFunction."""
        for ep in range(n_epochs):
            t0 = time.time()
            acc = [0.0, 0.0, 0.0]
            nb = 0
            for x, y in self.train_loader:
                x, y = x.to(cg.device), y.to(cg.device)
                assert x.dim() == 2 and y.dim() == 2, "x and y must be (MB,D) and (MB,D')"
                self.model.set_is_training(True)
                loss = self.ELBO_call(x, y)
                self.optimizer.zero_grad()
                loss.backward()
                self.optimizer.step()
                self.model.set_is_training(False)
                lv = loss.item()
                self.loss_arr.append(lv)
                self.ELL_arr.append(self.param_elbo[1].item())
                self.KLD_arr.append(self.param_elbo[2].item())
                acc[0] += -lv
                acc[1] += self.ELL_arr[-1]
                acc[2] += self.KLD_arr[-1]
                nb += 1
            self.total_trainer_epochs += 1
            if self.validate_each > 0 and (ep + 1) % self.validate_each == 0:
                print("| Epoch [{}/{}] ELBO {:.5f} ELL {:.5f} KLD {:.5f} ({:.3f}s)".format(
                    ep + 1, epochs_total, acc[0] / nb, acc[1] / nb, acc[2] / nb, time.time() - t0))

    # ---- metrics (trainers_regression.py:108-224, 317-338) ----------------------------------------------
    def performance_metrics(self, X, Y):
        self.model.set_is_training(False)
        logp, (m1, _m2) = self.model.test_log_likelihood(X, Y, return_moments=True, Y_std=self.Y_std.to(X.device),
                                                         S_MC_NNet=self.S_test if self.model.fully_bayesian else None)
        exact = self.coverage == "exact"
        lik = getattr(self.model, "likelihood", None)          # (a foreign model's may carry no traits: the exact route then)
        no_cdf = getattr(lik, "refuses_cdf", None) is not None
        if exact and (self.model.fully_bayesian or no_cdf):
            # an MC-dropout mixture over parameter draws has no closed CDF here, a count model no continuous quantiles, a
            # Student-t or heteroscedastic model no CDF kernel: the sampled recipe, said once
            if not self._coverage_fallback_said:
                print("[tgp.pytorch_amd] coverage='exact' is not built for the %s model: sampled coverage instead"
                      % (lik.display if no_cdf else "fully Bayesian"))
                self._coverage_fallback_said = True
            exact = False
        if exact:
            q = self.model.predictive_quantiles(X, [0.025, 0.975])[0]                              # (2,N), stays on the device
            cover = ((Y[:, 0] >= q[0]) & (Y[:, 0] <= q[1])).sum().item()
            cover = float(cover)
        else:
            samples, _, _ = self.model.sample_from_predictive_distribution(X, S=self.S_test)      # (Dy,S,N,1)
            q = numpy.quantile(samples.to("cpu").numpy(), [0.025, 0.975], axis=1)                  # (2,Dy,N,1)
            y = Y[:, 0].to("cpu")
            cover = ((y >= torch.tensor(q[0, 0, :, 0])) & (y <= torch.tensor(q[1, 0, :, 0]))).float().sum().item()
        se = ((m1.reshape(-1) - Y[:, 0]) ** 2).sum().item()
        return float(logp.reshape(-1)[0]), se, cover

    def _loader_metrics(self, loader):
        tot, lp, se, cov = 0.0, 0.0, 0.0, 0.0
        for x, y in loader:
            x, y = x.to(cg.device), y.to(cg.device)
            a, b, c = self.performance_metrics(x, y)
            lp, se, cov, tot = lp + a, se + b, cov + c, tot + x.size(0)
        ystd = float(self.Y_std.reshape(-1)[0])
        return lp / tot, ystd * numpy.sqrt(se / tot), cov / tot

    def compute_metrics(self):
        """(logL, rmse, coverage) for train, valid, test -- nine floats like the reference."""
        self.refresh_qu()
        out = list(self._loader_metrics(self.train_loader))
        out += list(self._loader_metrics(self.valid_loader)) if self.is_valid else [0.0, 0.0, 0.0]
        out += list(self._loader_metrics(self.test_loader)) if self.is_test else [0.0, 0.0, 0.0]
        return tuple(out)

    # ---- proper scores beside the log score ----------------------------------------------------------------
    def _loader_scores(self, loader, samples):
        model = self.model
        sampled = samples is not None or model.fully_bayesian or any(
            getattr(getattr(model, "likelihood", None), a, None) is not None for a in ("refuses_cdf", "refuses_crps"))
        if sampled and samples is None and not self._scores_fallback_said:
            print("[tgp.pytorch_amd] the exact CRPS is not built for this model: the CRPS of %d predictive draws per row instead, "
                  "and no interval score" % self.S_test)
            self._scores_fallback_said = True
        ystd = self.Y_std.reshape(-1)[:1].to(cg.device)
        tot, crps, isc = 0.0, 0.0, 0.0
        for x, y in loader:
            x, y = x.to(cg.device), y.to(cg.device)
            model.set_is_training(False)
            if sampled:
                crps += model.predictive_crps(x, y, Y_std=ystd, samples=self.S_test if samples is None else samples).sum().item()
            else:
                crps += model.predictive_crps(x, y, Y_std=ystd).sum().item()
                isc += model.predictive_interval_score(x, y, 0.05, Y_std=ystd).sum().item()
            tot += x.size(0)
        return {"crps": crps / tot, "interval_score": None if sampled else isc / tot}

    def compute_scores(self, samples=None):
        """{"train" | "valid" | "test": {"crps": mean, "interval_score": mean}} in raw units (standardised scores times Y_std):
        the exact CRPS (model.predictive_crps) and the 95 % interval score of the exact quantiles where they exist; otherwise --
        or with samples=S -- the CRPS of S (default S_test) predictive draws per row, said once, and interval_score None.  A
        split without a loader is None."""
        self.refresh_qu()
        return {"train": self._loader_scores(self.train_loader, samples),
                "valid": self._loader_scores(self.valid_loader, samples) if self.is_valid else None,
                "test": self._loader_scores(self.test_loader, samples) if self.is_test else None}


    def compute_relevance(self):
        """(relevance (D,), inverse length-scales (D,) or None): utils.input_relevance of the model over the rows of the test
        split -- the root-mean-square slope of the predictive mean in each input, standardised units -- beside 1 / l_d of the ARD
        kernel (None for a model of several latent GPs, which has a set per GP).  NotImplementedError where
        predictive_input_gradients has none."""
        from .utils import input_relevance
        assert self.is_test, "compute_relevance reads the test split"
        self.refresh_qu()
        self.model.set_is_training(False)
        X = torch.cat([x for x, _ in self.test_loader]).to(cg.device)
        rel = input_relevance(self.model, X).cpu()
        raw = self.model.covariance_function.base_kernel.raw_lengthscale.detach().reshape(-1, X.shape[1])
        ils = (1.0 / torch.nn.functional.softplus(raw[0])).cpu() if raw.shape[0] == 1 else None
        return rel, ils


    def compute_slope_significance(self, z=1.96):
        """(D,): utils.slope_significance of the model over the rows of the test split -- the share of rows at which the
        posterior slope in each input is further than z posterior standard deviations from zero."""
        from .utils import slope_significance
        assert self.is_test, "compute_slope_significance reads the test split"
        self.refresh_qu()
        self.model.set_is_training(False)
        X = torch.cat([x for x, _ in self.test_loader]).to(cg.device)
        return slope_significance(self.model, X, z=z).cpu()

    def compute_suggestions(self, K, kind="log_ei", num_starts=64, steps=50, seed=0):
        """[(x (D,), value)] of at most K entries, best first: the K best distinct candidates for the next evaluation, maximising,
        inside the bounding box of the training inputs -- utils.suggest_candidates from `num_starts` seeded starts against the
        best training target (standardised units, as the loaders hold them), the per-start finals ranked by their acquisition
        value; two finals closer than 1e-6 of the box in every input count as one."""
        from .utils import suggest_candidates
        self.refresh_qu()
        self.model.set_is_training(False)
        X = torch.cat([x for x, _ in self.train_loader]).to(cg.device)
        best = float(torch.cat([y for _, y in self.train_loader]).max())
        bounds = torch.stack((X.min(0).values, X.max(0).values))
        _, _, finals = suggest_candidates(self.model, bounds, kind=kind, best=best, maximize=True, num_starts=num_starts, steps=steps,
                                          generator=torch.Generator().manual_seed(int(seed)))
        Xf = finals["X"]
        vals = self.model.acquisition(Xf, kind=kind, best=best, maximize=True).cpu()     # (kind="ei": finals hold its logarithm)
        Xf = Xf.cpu()
        tol = 1e-6 * (bounds[1] - bounds[0]).cpu()
        out = []
        for i in torch.argsort(vals, descending=True).tolist():
            if not math.isfinite(float(vals[i])):
                continue
            if all(bool(((Xf[i] - x).abs() > tol).any()) for x, _ in out):
                out.append((Xf[i], float(vals[i])))
            if len(out) == int(K):
                break
        return out


class Trainer_SP_classification(Trainer_SP_regression):
    """trainers_classification.py: the same training loop, metrics (logL, accuracy) per split.  Bernoulli models train on
    the eager path (ops.ElboFunction): the resident step engine has no Bernoulli likelihood (engine.engine_refusal).  Multi-class models
    (MulticlassCategorical, C latent GPs) train on the eager path too, on the composed step of models._elbo_composed; their
    accuracy is the argmax over the C class probabilities (trainers_classification.py:132)."""

    def performance_metrics(self, X, Y):
        """(sum_n log p(y_n), number of correct labels): argmax over [1 - P, P] (binary) or over the C class probabilities
        (multi-class); a tie goes to the lower class."""
        self.model.set_is_training(False)
        logp, (probs,) = self.model.test_log_likelihood(X, Y, return_moments=True, Y_std=self.Y_std.to(X.device),
                                                        S_MC_NNet=self.S_test if self.model.fully_bayesian else None)
        pred = probs.argmax(dim=1)                    # first maximum: class 0 on a tie
        correct = (pred == Y.reshape(-1).to(pred.dtype)).sum().item()
        return float(logp.reshape(-1)[0]), correct

    def _loader_metrics(self, loader):
        tot, lp, ok = 0, 0.0, 0
        for x, y in loader:
            x, y = x.to(cg.device), y.to(cg.device)
            a, b = self.performance_metrics(x, y)
            lp, ok, tot = lp + a, ok + b, tot + x.size(0)
        return lp / tot, ok / tot

    def compute_metrics(self):
        """(logL_train, acc_train, logL_valid, acc_valid, logL_test, acc_test): logL is the mean per-row log p(y)."""
        out = list(self._loader_metrics(self.train_loader))
        out += list(self._loader_metrics(self.valid_loader)) if self.is_valid else [0.0, 0.0]
        out += list(self._loader_metrics(self.test_loader)) if self.is_test else [0.0, 0.0]
        return tuple(out)
