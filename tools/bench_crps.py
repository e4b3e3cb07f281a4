"""Time of the exact CRPS (model.predictive_crps: the q(f) moments + tgp_predict_crps_f64) against the only route there was
before it: sample_from_predictive_distribution(S = 100) + ops.crps_from_samples (a sort of the draws on the device).  Shapes as
tools/bench_quantiles.py: the Power test split (N = 957) and training split (N = 8611), D = 4, M = 100, SAL x 2 and tanh 3 x 2,
S = 50 and 100 quadrature nodes.  The paths are timed in ALTERNATING blocks in one process on one device (HIP events around each
block, the warm-up / calls convention of bench.py, which this script does not touch); the median of the blocks is reported.
`kernel` is ops.predict_crps alone on moments computed once -- the launch of k_pred_crps without the q(f) moments.  Prints one
JSON line per configuration; not a bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_crps.py --calls 50 --warmup 5 --blocks 5 > profiles/crps.txt
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch                                    # noqa: E402

from bench_quantiles import CONFIGS, block, build   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per path")
    ap.add_argument("--config", default=None, help="N,flow,S: this configuration only")
    args = ap.parse_args(argv)
    configs = CONFIGS
    if args.config is not None:
        n, flow, s = args.config.split(",")
        configs = [(int(n), flow, int(s))]
    if not torch.cuda.is_available():
        raise SystemExit("bench_crps.py needs the GPU: nothing is measured without one")
    from tgp.pytorch_amd import ops
    for N, flow, S in configs:
        model, X = build(N, flow, S)
        Y = model.predictive_quantiles(X, [0.4])[0, 0].reshape(-1, 1)          # targets inside the predictive
        mu, v, lvn, spec, theta, rowp = model._quantile_inputs(X, "predictive_cdf")
        model.train()
        paths = {"exact": lambda m, x: m.predictive_crps(x, Y),
                 "kernel": lambda m, x: ops.predict_crps(mu, v, lvn, Y, spec, theta, S, rowp),
                 "sampled": lambda m, x: m.predictive_crps(x, Y, samples=100)}
        for fn in paths.values():
            for _ in range(args.warmup):
                fn(model, X)
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(args.blocks):
            for k, fn in paths.items():
                times[k].append(block(fn, model, X, args.calls))
        res = {"workload": "crps_power", "N": N, "flow": flow, "S": S, "calls": args.calls, "warmup": args.warmup,
               "blocks": args.blocks}
        for k, ts in times.items():
            res[k + "_ms_per_call_median"] = sorted(ts)[len(ts) // 2]
            res[k + "_ms_per_call_blocks"] = ts
        res["sampled_over_exact"] = res["sampled_ms_per_call_median"] / res["exact_ms_per_call_median"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
