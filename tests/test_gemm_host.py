"""CPU: the host side of the float64 GEMM family -- which kernel and workgroup order the launcher gives a shape
(tgp_gemm_route: the launcher's own decision function, queried without a device), and what tgp_gemm_f64 / tgp_gemm_ex_f64 /
tgp_gemm_pair_ex_f64 refuse, with which code.

ROUTE_CASES is the table tests/test_gpu_gemm.py takes its routing shapes from: every GPU case there names a row, asserts the
row's route again before it launches, and so cannot drift onto another kernel when the launcher's cost model changes -- this
file fails first, and says which shape moved."""
import ctypes as C

import pytest

from tgp.pytorch_amd import lib as L
from tgp.pytorch_amd import ops

R128, PAIRED, HEAVY, TRIANGLE, R64 = (L.GEMM_ROUTE_128, L.GEMM_ROUTE_128_PAIRED, L.GEMM_ROUTE_128_HEAVY,
                                      L.GEMM_ROUTE_128_TRIANGLE, L.GEMM_ROUTE_64)
AL, AU, BL, BU, CL = ops.TRI_A_LOWER, ops.TRI_A_UPPER, ops.TRI_B_LOWER, ops.TRI_B_UPPER, ops.TRI_C_LOWER

# name -> (arguments of ops.gemm_route, route).  The 64 x 64 kernel takes products with trans_a = 0, no modifier, no split,
# at most a triangular op(B) and k % 64 == 0 where its cost model predicts 30 % less time; everything else is 128 x 128.
ROUTE_CASES = {}


def _case(name, route, m, n, k, **kw):
    assert name not in ROUTE_CASES
    ROUTE_CASES[name] = (dict(m=m, n=n, k=k, **kw), route)


for _tb in (0, 1):
    # ---- 64 x 64 tiles ----
    _case("g64_128_tb%d" % _tb, R64, 128, 128, 128, trans_b=_tb)
    # one k-block: wave group 1 idle (the cost model sends an untrimmed k = 64 to the big tiles; this one trims nothing either)
    _case("g64_k64_tb%d" % _tb, R64, 128, 128, 64, trans_b=_tb, tri=BU)
    _case("g64_k192_tb%d" % _tb, R64, 128, 256, 192, trans_b=_tb)          # 2 + 1 k-blocks over the two wave groups
    _case("g64_256_beta_tb%d" % _tb, R64, 256, 256, 256, trans_b=_tb, beta=1.0)        # tgp_qf_cov_f64 at M <= 256
    _case("g64_384_bl_tb%d" % _tb, R64, 384, 384, 384, trans_b=_tb, tri=BL)
    _case("g64_384_bu_tb%d" % _tb, R64, 384, 384, 384, trans_b=_tb, tri=BU)
    for _ta in (0, 1):
        _t = "ta%d_tb%d" % (_ta, _tb)
        # ---- 128 x 128 tiles, natural order (k % 64 != 0 keeps trans_a = 0 off the small tiles) ----
        _case("nat_" + _t, R128, 256, 384, 208, trans_a=_ta, trans_b=_tb)
        for _k in (16, 32, 48):
            _case("nat_k%d_%s" % (_k, _t), R128, 128, 256, _k, trans_a=_ta, trans_b=_tb)
        # ---- triangular op(B), unpaired: heaviest column first.  trans_a = 0 needs k % 64 != 0 again ----
        _case("heavy_bl_" + _t, HEAVY, 384, 384, 384 if _ta else 400, trans_a=_ta, trans_b=_tb, tri=BL)
        _case("heavy_bu_" + _t, HEAVY, 384, 384, 384 if _ta else 400, trans_a=_ta, trans_b=_tb, tri=BU)
        # ---- triangular op(B), paired column tiles: 171 tile rows is the smallest grid the pairing survives on ----
        _case("paired_bl_" + _t, PAIRED, 21888, 256, 256 if _ta else 272, trans_a=_ta, trans_b=_tb, tri=BL)
        _case("paired_bu_" + _t, PAIRED, 21888, 256, 256 if _ta else 272, trans_a=_ta, trans_b=_tb, tri=BU)
        # ---- TRI_C_LOWER with split-K: compact lower block triangle (6 tiles x 3 slabs = 18 workgroups) ----
        _case("triangle_" + _t, TRIANGLE, 384, 384, 208, trans_a=_ta, trans_b=_tb, tri=CL, ksplit=3)
# what else the 128 x 128 kernel is given: a modifier, a split, a triangular op(A), TRI_C_LOWER unsplit
_case("nat_mod", R128, 256, 256, 256, mod=True)                      # (without the modifier: the small tiles)
_case("nat_mod_ta", R128, 256, 256, 256, trans_a=1, mod=True)
_case("nat_epi", R128, 256, 256, 208)
_case("nat_split4", R128, 256, 256, 208, ksplit=4)
_case("nat_split8", R128, 256, 256, 208, ksplit=8)
# k = 208 is 13 stages: 4 slabs of 4, 4, 4, 1 and 8 slabs of 2 with one empty; under TRI_A_LOWER the first tile row has 8
# stages (slabs of 2, or of 1) and op(A)'s tile (0, 1) is never read
_case("nat_split4_al", R128, 256, 256, 208, ksplit=4, tri=AL)
_case("nat_split8_al", R128, 256, 256, 208, ksplit=8, tri=AL)
_case("nat_split8_al_xcd2", R128, 256, 256, 208, ksplit=8, tri=AL, xcd=2)     # the slab-major order is live at 8 slabs
_case("nat_split4_al_xcd2", R128, 256, 256, 208, ksplit=4, tri=AL, xcd=2)     # ... and falls back to the natural one at 4
_case("nat_xcd1_11rows", R128, 1408, 256, 48, xcd=1)
_case("nat_al", R128, 384, 256, 384, tri=AL)
_case("nat_au", R128, 384, 256, 384, tri=AU)
_case("nat_au_ta", R128, 384, 256, 384, trans_a=1, tri=AU)
_case("nat_al_bu", R128, 384, 384, 384, trans_b=1, tri=AL | BU)
_case("nat_au_bl", R128, 384, 384, 384, trans_a=1, tri=AU | BL)
_case("nat_cl", R128, 384, 384, 208, trans_b=1, tri=CL)
_case("g64_bl_wide", R64, 128, 384, 128, tri=BL)                     # n > k: column tiles with an empty k range
_case("heavy_bl_wide", HEAVY, 128, 384, 144, tri=BL)
_case("heavy_bl_wide_ta", HEAVY, 128, 384, 128, trans_a=1, tri=BL)


@pytest.mark.parametrize("name", sorted(ROUTE_CASES))
def test_route_of_every_routing_shape(name):
    kw, route = ROUTE_CASES[name]
    assert ops.gemm_route(**kw) == route, (name, kw)


def test_every_route_is_reached():
    assert {r for _, r in ROUTE_CASES.values()} == {R128, PAIRED, HEAVY, TRIANGLE, R64}
    # each 128-tile route by all four transpositions, the 64-tile kernel by both layouts of B
    for r in (R128, PAIRED, HEAVY, TRIANGLE):
        assert {(kw.get("trans_a", 0), kw.get("trans_b", 0)) for kw, rr in ROUTE_CASES.values() if rr == r} >= \
            {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {kw.get("trans_b", 0) for kw, rr in ROUTE_CASES.values() if rr == R64} == {0, 1}


def test_route_is_the_launchers_decision_not_the_callers():
    """xcd 3 and 4 are the launcher's own; a caller's xcd never changes the kernel; what the launcher cannot run is a code."""
    assert ops.gemm_route(384, 384, 384, tri=BL, xcd=3) == -26
    assert ops.gemm_route(384, 384, 384, trans_a=1, tri=BL, xcd=1) == HEAVY
    assert ops.gemm_route(384, 384, 208, tri=CL, ksplit=3, xcd=2) == TRIANGLE
    assert ops.gemm_route(384, 384, 208, tri=CL | AL, ksplit=3) == R128             # the compact order: TRI_C_LOWER alone
    assert ops.gemm_route(384, 256, 208, tri=CL, ksplit=3) == R128                  # ... and a square C
    assert ops.gemm_route(100, 128, 16) == -4 and ops.gemm_route(128, 130, 16) == -5 and ops.gemm_route(128, 128, 24) == -6
    assert ops.gemm_route(128, 128, 16, ksplit=0) == -24
    assert L.load().tgp_gemm_route(None) == -1


# ---- refusals, in the style of tests/test_api_refusals.py: (entry, overrides of the base call, code); nothing is launched ----
PTR = C.c_void_p(0x1000)            # non-NULL, 16-byte aligned, never dereferenced
ODD = C.c_void_p(0x1008)            # 8-byte aligned only
BASE = dict(trans_a=0, trans_b=0, tri=0, m=128, n=256, k=48, alpha=1.0, A=PTR, lda=48, B=PTR, ldb=256, beta=0.0, C=PTR, ldc=256)
PLAIN_ARGS = ("trans_a", "trans_b", "tri", "m", "n", "k", "alpha", "A", "lda", "B", "ldb", "beta", "C", "ldc")
ROWS = [
    # ---- tgp_gemm_f64: the checks it always made ----
    ("tgp_gemm_f64", dict(tri=32), -3),
    ("tgp_gemm_f64", dict(tri=-1), -3),
    ("tgp_gemm_f64", dict(m=100), -4),
    ("tgp_gemm_f64", dict(m=0), -4),
    ("tgp_gemm_f64", dict(n=200), -5),
    ("tgp_gemm_f64", dict(k=40), -6),
    ("tgp_gemm_f64", dict(k=0), -6),
    ("tgp_gemm_f64", dict(A=None), -8),
    ("tgp_gemm_f64", dict(B=None), -10),
    ("tgp_gemm_f64", dict(C=None), -13),
    # ---- ... what the launcher answered with a bare -1: the 16-byte operand loads ----
    ("tgp_gemm_f64", dict(A=ODD), -8),
    ("tgp_gemm_f64", dict(lda=49), -9),
    ("tgp_gemm_f64", dict(B=ODD), -10),
    ("tgp_gemm_f64", dict(ldb=257), -11),
    # ---- ... and what nothing checked: a leading dimension shorter than the row it strides ----
    ("tgp_gemm_f64", dict(lda=46), -9),
    ("tgp_gemm_f64", dict(trans_a=1, lda=48), -9),              # A is stored (k, m): rows of 128
    ("tgp_gemm_f64", dict(trans_a=1, lda=126), -9),
    ("tgp_gemm_f64", dict(ldb=254), -11),
    ("tgp_gemm_f64", dict(trans_b=1, ldb=46), -11),             # B is stored (n, k): rows of 48
    ("tgp_gemm_f64", dict(ldc=255), -14),
    ("tgp_gemm_f64", dict(ldc=128), -14),
    # ---- tgp_gemm_ex_f64: the same codes for the same fields ----
    ("tgp_gemm_ex_f64", dict(desc=None), -1),
    ("tgp_gemm_ex_f64", dict(tri=32), -3),
    ("tgp_gemm_ex_f64", dict(m=100), -4),
    ("tgp_gemm_ex_f64", dict(n=200), -5),
    ("tgp_gemm_ex_f64", dict(k=40), -6),
    ("tgp_gemm_ex_f64", dict(A=None), -8),
    ("tgp_gemm_ex_f64", dict(A=ODD), -8),
    ("tgp_gemm_ex_f64", dict(lda=49), -9),
    ("tgp_gemm_ex_f64", dict(lda=46), -9),
    ("tgp_gemm_ex_f64", dict(trans_a=1, lda=126), -9),
    ("tgp_gemm_ex_f64", dict(B=None), -10),
    ("tgp_gemm_ex_f64", dict(B=ODD), -10),
    ("tgp_gemm_ex_f64", dict(ldb=257), -11),
    ("tgp_gemm_ex_f64", dict(ldb=254), -11),
    ("tgp_gemm_ex_f64", dict(trans_b=1, ldb=46), -11),
    ("tgp_gemm_ex_f64", dict(C=None), -13),
    ("tgp_gemm_ex_f64", dict(ldc=254), -14),
    # ---- ... and its own fields ----
    ("tgp_gemm_ex_f64", dict(a_mul=ODD), -15),
    ("tgp_gemm_ex_f64", dict(k_scale=ODD), -16),
    ("tgp_gemm_ex_f64", dict(add=PTR, ldadd=256, beta=1.0), -17),
    ("tgp_gemm_ex_f64", dict(add=PTR, ldadd=255), -18),
    ("tgp_gemm_ex_f64", dict(rowv=PTR), -23),                   # the rank-one term needs both vectors: the missing one
    ("tgp_gemm_ex_f64", dict(colv=PTR), -22),
    ("tgp_gemm_ex_f64", dict(ksplit=0), -24),
    ("tgp_gemm_ex_f64", dict(ksplit=-3), -24),
    ("tgp_gemm_ex_f64", dict(ksplit=2, scratch=PTR, scratch_doubles=1 << 20), -24),     # the scratch route splits by itself
    ("tgp_gemm_ex_f64", dict(ksplit=2, cz=127 * 256 + 255), -25),                        # slabs that overlap
    ("tgp_gemm_ex_f64", dict(xcd=3), -26),
    ("tgp_gemm_ex_f64", dict(xcd=4), -26),
    ("tgp_gemm_ex_f64", dict(xcd=-1), -26),
    ("tgp_gemm_ex_f64", dict(scratch=C.c_void_p(0x1004)), -27),
    # ---- the pair: a's field numbers, b's plus 32; a is (0, 1), b is (0, 0) ----
    ("tgp_gemm_pair_ex_f64", dict(a=dict(desc=None)), -1),
    ("tgp_gemm_pair_ex_f64", dict(b=dict(desc=None)), -33),
    ("tgp_gemm_pair_ex_f64", dict(a=dict(lda=49)), -9),
    ("tgp_gemm_pair_ex_f64", dict(a=dict(trans_a=1, lda=128)), -1),
    ("tgp_gemm_pair_ex_f64", dict(a=dict(trans_b=0, ldb=256)), -2),
    ("tgp_gemm_pair_ex_f64", dict(a=dict(scratch=PTR, scratch_doubles=1 << 20)), -27),
    ("tgp_gemm_pair_ex_f64", dict(b=dict(ldb=254)), -43),
    ("tgp_gemm_pair_ex_f64", dict(b=dict(trans_a=1, lda=128)), -33),
    ("tgp_gemm_pair_ex_f64", dict(b=dict(trans_b=1)), -34),
    ("tgp_gemm_pair_ex_f64", dict(b=dict(ksplit=0)), -56),
    ("tgp_gemm_pair_ex_f64", dict(b=dict(scratch=PTR, scratch_doubles=1 << 20)), -59),
]


def _desc(over):
    if "desc" in over:
        return None
    d = L.TgpGemmEx()
    for k, v in dict(dict(BASE, ksplit=1), **over).items():
        setattr(d, k, v)
    return d


def call(lib, entry, over):
    if entry == "tgp_gemm_f64":
        f = dict(BASE, **over)
        return lib.tgp_gemm_f64(*[f[k] for k in PLAIN_ARGS], None)
    if entry == "tgp_gemm_ex_f64":
        return lib.tgp_gemm_ex_f64(_desc(over), None)
    a = _desc(dict(dict(trans_b=1, ldb=48), **over.get("a", {})))
    b = _desc(over.get("b", {}))
    return lib.tgp_gemm_pair_ex_f64(a, b, None)


def test_the_refusal_table_covers_what_the_entries_check():
    assert all(code < 0 for _, _, code in ROWS)
    assert len({(e, repr(sorted(o.items(), key=str))) for e, o, _ in ROWS}) == len(ROWS)      # no row twice
    assert {c for e, _, c in ROWS if e == "tgp_gemm_f64"} == {-3, -4, -5, -6, -8, -9, -10, -11, -13, -14}
    assert {c for e, _, c in ROWS if e == "tgp_gemm_ex_f64"} >= {-9, -11, -8, -10, -15, -16, -17, -24}


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: "%s-%d" % (ROWS[i][0][4:], i))
def test_refusal(row):
    entry, over, code = ROWS[row]
    assert call(L.load(), entry, over) == code, (entry, over)


def test_descriptor_layout_matches_the_header():
    """The binding's struct is the header's, field for field and in its order: the order is the meaning of a refusal's code."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "tgp_hip.h")).read()
    body = re.search(r"typedef struct tgp_gemm_ex \{(.*?)\} tgp_gemm_ex;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert names == [f for f, _ in L.TgpGemmEx._fields_]
    for number, field in ((9, "lda"), (11, "ldb"), (14, "ldc"), (17, "add"), (24, "ksplit"), (26, "xcd"), (27, "scratch")):
        assert names[number - 1] == field
