"""Step time of a warped-GP (WGP) training step: engine.ElboEngine(likelihood="warped"), SAL x 2 on the Power shape
(N = 8611, D = 4, M = 100), replayed from a HIP graph and timed with HIP events -- the warm-up / steps convention of bench.py
(`--steps K --warmup W`), which this script does not touch.  Prints one JSON line.

    python tools/bench_warped.py --steps 2000 --warmup 100
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402
from tgp.pytorch_amd.engine import ElboEngine   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--likelihood", choices=["warped", "gauss"], default="warped")
    args = ap.parse_args(argv)
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal2", S=32)
    kw = dict(flow_blocks=prob["program"], S=32, likelihood="warped")
    if args.likelihood == "gauss":
        prob["params"].pop("theta")
        kw = {}
    eng = ElboEngine(prob["X"], prob["Y"], prob["params"], float(prob["N_total"]), device="cuda:0", **kw)
    eng.capture(unroll=1)
    for _ in range(args.warmup):
        eng.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.steps):
        eng.replay()
    t1.record()
    torch.cuda.synchronize()
    eng.check_status()
    ms = t0.elapsed_time(t1) / args.steps
    elbo, ell, kl = eng.scalars()
    print(json.dumps({"workload": "wgp_power_sal2" if args.likelihood == "warped" else "svgp_power_same_script",
                      "ms_per_step": ms, "steps_per_s": 1000.0 / ms, "steps": args.steps, "warmup": args.warmup,
                      "elbo": float(elbo), "finite": bool(torch.isfinite(torch.tensor(float(elbo))))}))


if __name__ == "__main__":
    main()
