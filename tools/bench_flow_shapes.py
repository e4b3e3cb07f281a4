"""Step time of the eager training step (ops.elbo_step) on the Power shape (N = 8611, D = 4, M = 100, S = 32) for the flows
ArcSL x 2, SinhL x 2, NormalCDFL x 2 and TukeyL x 2 -- and, given the library of the parent commit, ArcSL x 2 with THAT library:
the TGP_FLOWX row kernels ArcSL runs must cost what they cost before the kinds past INV_BOXCOX existed.

Every timed block is a fresh child process of this script under its own `timeout` (a library is loaded once per process, so two
libraries need two processes), in ALTERNATING order: [ArcSL this, ArcSL parent, SinhL, NormalCDFL, TukeyL] x blocks.  A child
that fails ends the run: nothing is started after it.  HIP events around each block, the warm-up / steps convention of bench.py
(which this script does not touch).  No threshold is attached to the new kinds' numbers; for ArcSL x 2 the report says whether
this library's median lies inside the parent library's own block-to-block spread of the same run.

    python tools/bench_flow_shapes.py --parent-lib <libtgp_hip.so of the parent commit> --out profiles/flow_shapes.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
FLOWS = ("ArcSL", "SinhL", "NormalCDFL", "TukeyL")


def child(args):
    """One block: microseconds per eager step of `args.flow` x 2 with the library at `args.lib` (default: the tree's)."""
    import numpy
    import torch
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import lib as L
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
        os.environ["TGP_ALLOW_STALE_LIB"] = "1"           # another commit's binary, on purpose; the ABI (TGP_VERSION 104) is the same
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd import config as cg
    cg.set_maximum_precission()                           # float64, as main.py runs
    numpy.random.seed(11)
    spec, theta_list, _ = compile_flow(instance_flow(getattr(G, args.flow)(2)))
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow=None, S=32)
    p = {k: v.to(DEV) for k, v in prob["params"].items()}
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]).to(DEV)
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    flow = ops.FlowSpec([tuple(b) for b in spec.blocks], theta.numel(), 0, DEV)

    def step():
        return ops.elbo_step(X, Y, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], p["log_var_noise"],
                             prob["N_total"], flow=flow, theta=theta, S=32)
    for _ in range(args.warmup):
        out, _, status, _ = step()
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(status[1]) == 0 and bool(torch.isfinite(out).all())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"flow": args.flow, "lib": "parent" if args.lib else "this", "us_per_step": 1e3 * t0.elapsed_time(t1) / args.steps,
                      "elbo": float(out[0])}))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per flow and library")
    ap.add_argument("--timeout", type=int, default=120, help="seconds, per child process")
    ap.add_argument("--parent-lib", default=None, help="libtgp_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--flow", choices=FLOWS)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args(argv)
    if args.child:
        return child(args)
    order = [("ArcSL", None)] + ([("ArcSL", args.parent_lib)] if args.parent_lib else []) + [(f, None) for f in FLOWS[1:]]
    times, elbo = {}, {}
    for b in range(args.blocks):
        for flow, lib in order:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--flow", flow,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--lib", lib] if lib else [])
            r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                print("block %d, %s (%s): exit status %d -- nothing more is started" % (b, flow, lib or "this", r.returncode))
                return r.returncode
            res = json.loads(r.stdout.strip().splitlines()[-1])
            key = (flow, res["lib"])
            times.setdefault(key, []).append(res["us_per_step"])
            elbo[key] = res["elbo"]
    lines = ["# eager ELBO step, Power shape (N = 8611, D = 4, M = 100, S = 32), flow x 2, us per step: %d alternating blocks of %d "
             "steps (%d warm-up), one child process per block" % (args.blocks, args.steps, args.warmup),
             "%-12s %-7s %10s %10s %10s   blocks" % ("flow", "library", "median", "min", "max")]
    for key, v in times.items():
        lines.append("%-12s %-7s %10.2f %10.2f %10.2f   %s" % (key[0], key[1], statistics.median(v), min(v), max(v),
                                                               " ".join("%.2f" % t for t in v)))
    base = statistics.median(times[("ArcSL", "this")])
    for f in FLOWS[1:]:
        lines.append("%s x 2 / ArcSL x 2 (this library, medians): %.3f" % (f, statistics.median(times[(f, "this")]) / base))
    if args.parent_lib:
        pv = times[("ArcSL", "parent")]
        inside = min(pv) <= base <= max(pv)
        lines.append("ArcSL x 2: this library's median %.2f us, the parent library's blocks span %.2f .. %.2f us (median %.2f): %s; "
                     "the two libraries' ELBO: %s" % (base, min(pv), max(pv), statistics.median(pv),
                                                      "inside the parent's spread" if inside else
                                                      ("BELOW the parent's spread (faster)" if base < min(pv) else "ABOVE the parent's spread (slower)"),
                                                      "bit-identical" if elbo[("ArcSL", "this")] == elbo[("ArcSL", "parent")] else
                                                      "%r vs %r" % (elbo[("ArcSL", "this")], elbo[("ArcSL", "parent")])))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
