"""CPU: the arcsinh / Box-Cox / inverse Box-Cox flow kinds above the kernels -- the spec generators against the
reference's (tests/golden/flows_specs.npz, written by tools/gen_golden_flows.py from the reference's dsp/flows.py under
the same numpy seeds), the flow classes, compile_flow's program rows and theta order, and the row-kernel instantiations
of the build (skipped without the in-tree build)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

from tgp.pytorch_amd import flow as F
from tgp.pytorch_amd import flows as G
from tgp.pytorch_amd import lib as L

CHAINS = ("SAL_BCL", "SAL_InvBCL", "SAL_AL", "BCL_AL", "InvBCL_AL")
# the calls of tools/gen_golden_flows.py spec_fixture, in its order (numpy seed 100 + index)
CALLS = [("ArcSL", lambda: G.ArcSL(2)), ("ArcSL_random", lambda: G.ArcSL(2, init_random=True)),
         ("ArcSL_f0", lambda: G.ArcSL(1, add_f0=True, set_res=True)),
         ("BoxCoxL", lambda: G.BoxCoxL(2)), ("BoxCoxL_random", lambda: G.BoxCoxL(2, init_random=True)),
         ("InverseBoxCoxL", lambda: G.InverseBoxCoxL(2, add_f0=True)),
         ("InverseBoxCoxL_random", lambda: G.InverseBoxCoxL(2, init_random=True)),
         ("Affine", lambda: G.Affine(3)), ("Affine_random", lambda: G.Affine(3, init_random=True, set_res=True))]
CALLS += [(ch, lambda ch=ch: G.build_chain(ch, 2, constraint=None)) for ch in CHAINS]


def _rows(specs):
    names, values = [], []
    for kind, init in specs:
        names.append(kind)
        row = [float(np.asarray(init[k]).reshape(-1)[0]) for k in ("init_a", "init_b", "init_c", "init_d", "init_lam")
               if k in init]
        row += [float(bool(init.get(k, False))) for k in ("add_init_f0", "set_restrictions")]
        values.append(row + [np.nan] * (6 - len(row)))
    return names, np.array(values, dtype=np.float64)


@pytest.mark.parametrize("i,name", [(i, c[0]) for i, c in enumerate(CALLS)])
def test_generator_specs_equal_the_reference(i, name):
    z = np.load(os.path.join(GOLDEN, "flows_specs.npz"))
    assert int(z[name + ".seed"]) == 100 + i
    np.random.seed(100 + i)
    names, values = _rows(CALLS[i][1]())
    assert names == [str(s) for s in z[name + ".names"]]
    np.testing.assert_array_equal(values, z[name + ".values"])


def test_build_chain_reads_the_constraint_and_refuses_unknown_names():
    with pytest.raises(KeyError):
        G.build_chain("SAL_BCL", 1)
    assert len(G.build_chain("SAL_AL", 3)) == 12        # no constraint needed: no Box-Cox generator in the chain
    with pytest.raises(ValueError):
        G.build_chain("SAL_XYZ", 1, constraint=None)


def test_instance_flow_accepts_the_new_names():
    comp = F.instance_flow([("arcsinh", dict(init_a=0.1, init_b=0.2, init_c=0.3, init_d=0.4, add_init_f0=False,
                                             set_restrictions=False)),
                            ("boxcox", dict(init_lam=1.5, add_init_f0=True)),
                            ("inverseboxcox", dict(init_lam=0.7, add_init_f0=False, constraint=None)),
                            ("inverse_boxcox", dict(init_lam=np.array([1.2]), add_init_f0=False))])
    kinds = [type(f).__name__ for f in comp.flow_arr]
    assert kinds == ["ArcsinhFlow", "BoxCoxFlow", "InverseBoxCoxFlow", "InverseBoxCoxFlow"]
    names = [n for n, _ in comp.named_parameters()]
    assert names == ["flow_arr.0.a", "flow_arr.0.b", "flow_arr.0.c", "flow_arr.0.d", "flow_arr.1.lam", "flow_arr.2.lam",
                     "flow_arr.3.lam"]


def test_a_constraint_callable_is_refused():
    with pytest.raises(NotImplementedError, match="constraint"):
        F.BoxCoxFlow(1.0, False, constraint=lambda lam: 2 * torch.sigmoid(lam))
    with pytest.raises(NotImplementedError, match="constraint"):
        F.instance_flow(G.InverseBoxCoxL(1, constraint=lambda lam: lam))


def test_arcsinh_add_f0_forces_the_restriction():
    assert F.ArcsinhFlow(0.0, 1.0, 0.0, 1.0, add_init_f0=True, set_restrictions=False).set_restrictions is True


def test_compile_flow_of_mixed_chains():
    np.random.seed(3)
    comp = F.instance_flow(G.build_chain("SAL_BCL", 1, constraint=None) + G.build_chain("InvBCL_AL", 1, constraint=None)
                           + G.ArcSL(1, add_f0=True))
    spec, theta, nets = F.compile_flow(comp)
    assert nets == []
    R, A = L.FLAG_RESTRICT, L.FLAG_ADD_F0
    assert spec.blocks == [(L.FLOW_SAL, 0, 0, 0), (L.FLOW_AFFINE, 0, 2, 0), (L.FLOW_BOXCOX, 0, 4, 0), (L.FLOW_AFFINE, 0, 5, 0),
                           (L.FLOW_INV_BOXCOX, 0, 7, 0), (L.FLOW_AFFINE, 0, 8, 0), (L.FLOW_ARCSINH, 0, 10, 0),
                           (L.FLOW_AFFINE, 0, 14, 0), (L.FLOW_ARCSINH, 0, 16, R | A), (L.FLOW_AFFINE, 0, 20, 0)]
    fl = comp.flow_arr
    expect = [fl[0].a, fl[0].b, fl[1].a, fl[1].b, fl[2].lam, fl[3].a, fl[3].b, fl[4].lam, fl[5].a, fl[5].b,
              fl[6].a, fl[6].b, fl[6].c, fl[6].d, fl[7].a, fl[7].b, fl[8].a, fl[8].b, fl[8].c, fl[8].d, fl[9].a, fl[9].b]
    assert len(theta) == len(expect) == spec.P
    assert all(t is e for t, e in zip(theta, expect))


def test_constants_mirror_the_header():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    for name, val in (("ARCSINH", L.FLOW_ARCSINH), ("BOXCOX", L.FLOW_BOXCOX), ("INV_BOXCOX", L.FLOW_INV_BOXCOX)):
        assert re.search(r"#define TGP_FLOW_%s %d\b" % (name, val), hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)


# ---- the row-kernel instantiations of the build (host-side symbols of the kernels) ----
BUILD = os.path.join(REPO, "tgp", "pytorch_amd", "csrc", "build")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FLOWX = 16      # TGP_FLOWX (tgp_dev.hpp)


def _symbols(obj):
    path = os.path.join(BUILD, obj)
    if not (os.path.exists(path) and os.path.exists(READELF)):
        pytest.skip("needs the in-tree build (make -C tgp/pytorch_amd/csrc) and llvm-readelf")
    out = subprocess.check_output([READELF, "--syms", "-W", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip() and line.split()[-1].startswith("_ZN3tgp")}


def _k_rows(mt, dp, mode, rw):
    return "_ZN3tgp6k_rowsILi%dELi%dELi%dELi%dEEEvNS_7RowArgsE" % (mt, dp, mode, rw)


def _k_rows4(mt, dp, train, nw):
    return "_ZN3tgp7k_rows4ILi%dELi%dELb%dELi%dEEEvNS_7RowArgsE" % (mt, dp, int(train), nw)


@pytest.mark.parametrize("mt", range(1, 9))
def test_row_kernel_instantiations(mt):
    old, ext = _symbols("tgp_rows_mt%d.o" % mt), _symbols("tgp_rowsx_mt%d.o" % mt)
    if os.path.exists(os.path.join(BUILD, "tgp_rowsx_mt%d_dp16.o" % mt)):    # (a unit of its own: see the Makefile)
        ext |= _symbols("tgp_rowsx_mt%d_dp16.o" % mt)
    for dp in (4, 8, 16):
        # every pre-existing instantiation, under its old name
        for name in [_k_rows(mt, dp, m, 16) for m in (0, 1, 2)] + [_k_rows(mt, dp, 1, 10)] + \
                    [_k_rows4(mt, dp, True, nw) for nw in (4, 8)]:
            assert name in old, name
        # the extended-kind instantiation of every training plan (modes 1, 2, RW = 10, k_rows4 with 4 and 8 waves)
        for name in [_k_rows(mt, dp, m | FLOWX, 16) for m in (1, 2)] + [_k_rows(mt, dp, 1 | FLOWX, 10)] + \
                    [_k_rows4(mt, dp, True, nw | FLOWX) for nw in (4, 8)]:
            assert name in ext, name
        assert not any("ELi%dELi%dELi0ELi16E" % (mt, dp) in s or "ELi%dELi%dELi16ELi16E" % (mt, dp) in s for s in ext)


def test_ell_flow_instantiations():
    syms = _symbols("tgp_lik.o")
    for lpr, nbs in ((4, (8, 4, 2, 1)), (16, (4, 2, 1)), (32, (4, 2, 1))):
        for nb in nbs:
            for x in (0, FLOWX):
                for lik in ("8EllGauss", "7EllBern"):       # k_ell_quad<Lik, LPR, NB | X>: both likelihoods, both kind sets
                    assert any(s.startswith("_ZN3tgp10k_ell_quadINS_%sELi%dELi%dEEE" % (lik, lpr, nb | x)) for s in syms), \
                        (lik, lpr, nb, x)
