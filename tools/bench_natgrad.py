"""Measurements of the natural-gradient step of q(u).  Not a bench.py workload, no threshold:

  kxwxk        tgp_kxwxk_f64 (the weighted row pass) against tgp_kxxk_f64 (the parent's kernel: the yardstick) on the same inputs,
               N = 8611 and N = 10000 at M = 100 and M = 1000
  natgrad_qu   tgp_natgrad_qu_f64 at rho = 1 and rho = 0.5 against tgp_optimal_qu_f64, Gaussian sites, same shapes, jitter 1e-6
               (1000 inducing points in 4 dimensions do not factorise without)
  epoch        one natgrad + Adam epoch of the eager Poisson loop (natgrad_step_qu -> ELBO -> backward -> Adam on the other
               parameters) against one Adam epoch of the same loop (q(u) trained by Adam): two trainers as main.py builds them for
               synthetic_counts (TGP, M = 20, one full batch), alternating blocks after a warm-up
  convergence  the same recipe, seed 1: the ELBO --qu adam reaches after 300 epochs, and the epochs / seconds after which
               --qu natgrad first passes it at --natgrad_lr 1, 0.5 and 0.1; every run follows an untimed run of its own recipe in
               the same process (first-use costs stay out), host clock from the first step to the stamped ELBO
The pairs are timed in ALTERNATING blocks in one process on one device, HIP events around each block, medians over the blocks.

    python tools/bench_natgrad.py > profiles/natgrad_step.txt
"""
import argparse
import contextlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from bench_collapsed import DEV, F64, alternate, problem          # noqa: E402  (tools/ is the script's directory)

JITTER = 1e-6
SHAPES = ((8611, 4, 100), (8611, 4, 1000), (10000, 8, 100), (10000, 8, 1000))


def bench_kxwxk(N, D, M, reps, blocks, warmup):
    from tgp.pytorch_amd import ops
    X, Y, p, _ = problem(N, D, M)
    Z, rl, ro = p["Z"], p["raw_lengthscale"].reshape(-1), p["raw_outputscale"].reshape(-1)
    w = torch.randn(N, dtype=F64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    one = torch.ones(N, dtype=F64, device=DEV)
    same = all(torch.equal(a, b) for a, b in zip(ops.kxxk(X, Z, rl, ro, Y), ops.kxwxk(X, Z, rl, ro, one, Y)))
    res = alternate({"kxxk": lambda: ops.kxxk(X, Z, rl, ro, Y), "kxwxk": lambda: ops.kxwxk(X, Z, rl, ro, w, Y)}, reps, blocks, warmup)
    return {"N": N, "D": D, "M": M, "kxxk_ms": res["kxxk"]["median_ms"], "kxwxk_ms": res["kxwxk"]["median_ms"],
            "kxwxk_over_kxxk": res["kxwxk"]["median_ms"] / res["kxxk"]["median_ms"], "unit_weights_bit_identical": same, "blocks": res}


def bench_natgrad_qu(N, D, M, reps, blocks, warmup):
    from tgp.pytorch_amd import ops
    X, Y, p, N_total = problem(N, D, M)
    Z, rl, ro, lvn = p["Z"], p["raw_lengthscale"].reshape(-1), p["raw_outputscale"].reshape(-1), p["log_var_noise"].reshape(-1)
    m, Lam = p["m"].reshape(-1).contiguous(), p["Lam"].contiguous()
    mu, v = ops.qf_moments(X, Z, rl, ro, m, Lam, jitter=JITTER)
    _, _, mb, vb = ops.ell_gauss(Y, mu, v, lvn, scale=N_total / N)
    out = (torch.empty(M, dtype=F64, device=DEV), torch.empty(M, M, dtype=F64, device=DEV))
    out2 = (torch.empty(M, dtype=F64, device=DEV), torch.empty(M, M, dtype=F64, device=DEV))

    def optimal():
        return ops.optimal_qu(X, Y, Z, rl, ro, lvn, N_total, jitter=JITTER, out=out, check=False)

    def natgrad(rho):
        return lambda: ops.natgrad_qu(X, Z, rl, ro, m, Lam, mu, mb, vb, rho=rho, jitter=JITTER, out=out2, check=False)
    m1 = optimal()[0].clone()
    m2 = natgrad(1.0)()[0].clone()
    res = alternate({"optimal_qu": optimal, "natgrad_rho1": natgrad(1.0), "natgrad_rho05": natgrad(0.5)}, reps, blocks, warmup)
    t = {k: r["median_ms"] for k, r in res.items()}
    return {"N": N, "D": D, "M": M, "optimal_qu_ms": t["optimal_qu"], "natgrad_rho1_ms": t["natgrad_rho1"],
            "natgrad_rho05_ms": t["natgrad_rho05"], "rho1_over_optimal": t["natgrad_rho1"] / t["optimal_qu"],
            "rho05_over_optimal": t["natgrad_rho05"] / t["optimal_qu"],
            "m_rel_diff_rho1_vs_optimal": float(((m1 - m2).abs().max() / m1.abs().max()).cpu()), "blocks": res}


RECIPE = ["--model", "TGP", "--likelihood", "poisson", "--dataset", "synthetic_counts", "--train_test_seed_split", "1",
          "--num_inducing", "20"]


def run_recipe(qu, epochs, stop_above=None, natgrad_lr=1.0, keep=None):
    """main.py's run with the trainer's ELBO calls stamped: (ELBO per epoch, seconds since the first step at each).  `stop_above`:
    the run ends at the first epoch whose ELBO passes it.  `keep` (a list): receives the trainer."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import main as M
    from tgp.pytorch_amd.trainers import Trainer_SP_regression

    class Passed(Exception):
        pass
    log = {"elbo": [], "t": [], "t0": None}

    class Stamped(Trainer_SP_regression):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            if keep is not None:
                keep.append(self)

        def ELBO_call(self, x, y):
            if log["t0"] is None:
                torch.cuda.synchronize()
                log["t0"] = time.time()
            loss = super().ELBO_call(x, y)
            log["elbo"].append(-float(loss.detach()))          # (a host sync, as the loop's own loss.item())
            log["t"].append(time.time() - log["t0"])
            if stop_above is not None and log["elbo"][-1] > stop_above:
                raise Passed()
            return loss

        def compute_metrics(self):
            return (0.0,) * 9
    old, old_engine = M.Trainer_SP_regression, cg.use_step_engine
    M.Trainer_SP_regression, cg.use_step_engine = Stamped, False       # the eager loop for every run: the same yardstick
    try:
        with contextlib.redirect_stdout(sys.stderr):                   # (main's own report lines: not this tool's result)
            M.main(RECIPE + ["--epochs", str(epochs), "--qu", qu, "--natgrad_lr", str(natgrad_lr)])
    except Passed:
        pass
    finally:
        M.Trainer_SP_regression, cg.use_step_engine = old, old_engine
    return log


def bench_epoch(reps, blocks, warmup):
    """Two trainers of the recipe, three epochs old; an epoch = Trainer._train_eager(1): the loop as it trains, its host reads included."""
    tr = {}
    for qu in ("adam", "natgrad"):
        keep = []
        run_recipe(qu, 3, natgrad_lr=0.5, keep=keep)
        tr[qu] = keep[0]
        tr[qu].ELBO_call = super(type(keep[0]), keep[0]).ELBO_call      # (unstamped)
        tr[qu].validate_each = 0

    def epoch(t):
        return lambda: t._train_eager(1, 1)
    res = alternate({"adam": epoch(tr["adam"]), "natgrad_adam": epoch(tr["natgrad"])}, reps, blocks, warmup)
    a, n = res["adam"]["median_ms"], res["natgrad_adam"]["median_ms"]
    return {"recipe": " ".join(RECIPE), "natgrad_lr": 0.5, "adam_epoch_ms": a, "natgrad_adam_epoch_ms": n, "natgrad_over_adam": n / a,
            "blocks": res}


def convergence(epochs, max_epochs, warm=20):
    run_recipe("adam", warm)                                           # untimed: first-use costs of the recipe
    adam = run_recipe("adam", epochs)
    target = adam["elbo"][-1]
    res = {"recipe": " ".join(RECIPE), "adam_epochs": len(adam["elbo"]), "adam_first_elbo": adam["elbo"][0], "adam_final_elbo": target,
           "adam_wall_s": adam["t"][-1], "adam_ms_per_epoch": 1e3 * adam["t"][-1] / max(len(adam["t"]) - 1, 1), "natgrad": [],
           "note": "one full batch per epoch; the ELBO of epoch k is evaluated before its Adam step (natgrad: after its q(u) step); "
                   "every run follows an untimed %d-epoch run of its own recipe; seconds: host clock from the first step to the "
                   "stamped ELBO, eager loop for all runs" % warm}
    run_recipe("natgrad", warm, natgrad_lr=0.5)                        # untimed
    for rho in (1.0, 0.5, 0.1):
        nat = run_recipe("natgrad", max_epochs, stop_above=target, natgrad_lr=rho)
        n = len(nat["elbo"])
        res["natgrad"].append({"natgrad_lr": rho, "first_elbo": nat["elbo"][0], "lowest_elbo": min(nat["elbo"]),
                               "elbo_at_epochs_10_50_100": [nat["elbo"][k - 1] if n >= k else None for k in (10, 50, 100)],
                               "epochs_to_pass": n if nat["elbo"][-1] > target else None, "epochs_run": n, "wall_s": nat["t"][-1],
                               "last_elbo": nat["elbo"][-1], "ms_per_epoch": 1e3 * nat["t"][-1] / max(n - 1, 1)})
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="alternating timed blocks per candidate")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=300, help="Adam epochs of the run the natgrad run has to pass")
    ap.add_argument("--max-epochs", type=int, default=600)
    args = ap.parse_args(argv)
    small = lambda M: (args.reps, args.warmup) if M <= 100 else (max(args.reps // 5, 5), max(args.warmup // 5, 3))    # noqa: E731
    res = {"kxwxk": [bench_kxwxk(N, D, M, small(M)[0], args.blocks, small(M)[1]) for N, D, M in SHAPES],
           "natgrad_qu": [bench_natgrad_qu(N, D, M, small(M)[0], args.blocks, small(M)[1]) for N, D, M in SHAPES],
           "epoch": bench_epoch(args.reps, args.blocks, args.warmup), "convergence": convergence(args.epochs, args.max_epochs)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
