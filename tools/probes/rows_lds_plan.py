"""The flow programs rows_lds_plan.hip reads on stdin: those of bench.py's workloads (synthetic.flow_program), tanh<B>x6 for
B = 5 .. 9 (lengthened until the plan no longer fits, so that the edge of the 10-rows-per-wave kernel's range is in the table) and
every distinct program of the fixtures under tests/golden/.  One line per program:  name S P RP nblk  kind K poff flags ..."""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tgp.pytorch_amd import synthetic  # noqa: E402

PER_ROW = 4      # TGP_FLAG_PER_ROW


def nparams(kind, K):   # flow_block_params (csrc/tgp_dev.hpp)
    return {0: 2, 1: 2, 2: 4 * K, 3: 4}.get(kind, 1)


def line(name, S, blocks):
    P = max([b[2] + nparams(b[0], b[1]) for b in blocks if not b[3] & PER_ROW] + [0])
    RP = max([b[2] + nparams(b[0], b[1]) for b in blocks if b[3] & PER_ROW] + [0])
    print(name, S, P, RP, len(blocks), " ".join(str(int(t)) for b in blocks for t in b))


seen = set()
for flow in ("tanh3x2", "sal2", "idsal3", "tanh5x6", "tanh6x6", "tanh7x6", "tanh8x6", "tanh9x6"):
    blocks = tuple(tuple(int(t) for t in b) for b in synthetic.flow_program(flow)[0])
    seen.add(blocks)
    line("bench:" + flow, 32, blocks)
for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
    z = np.load(f)
    if "program" not in z.files or z["program"].shape[0] == 0:
        continue
    blocks = tuple(tuple(int(t) for t in r) for r in z["program"])
    if blocks in seen:
        continue
    seen.add(blocks)
    line("golden:" + os.path.basename(f)[:-4], int(z["xs"].size) if "xs" in z.files else 32, blocks)
