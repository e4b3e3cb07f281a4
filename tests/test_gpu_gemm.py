"""GPU (-m gpu): the float64 GEMM family (k_gemm<TA,TB,MOD,EPI>, k_gemm64<EPI>, k_gemm_pair, the slab reduction behind
gemm_mm_on) against a plain reference of the formula in tgp_gemm.hpp's header,

    x = alpha (op(A) o a_mul diag(k_scale)) op(B) + gamma add;  x *= col_scale_j row_scale_i;  x += rowv_i colv_j;  C = x + beta C

`tri` flags are applied by zeroing the reference operands.  Two kinds of case:

EXACT (structure).  Every operand, modifier and scale is an integer in [-8, 8] and alpha, beta, gamma are powers of two, so
every product and partial sum is exact in float64 whatever the order of summation (a term is at most 8^4, a sum of k <= 400 of
them times 8^2 of scales stays far below 2^53) and the result must be BIT-EQUAL to the reference: a dropped, duplicated or
misplaced element, a slab left unwritten, a k range one stage short cannot hide behind a tolerance.  The reference evaluates
the epilogue in the kernel's order (an absent term enters as its neutral element, as in the kernel), so a single launch agrees
down to the sign of a zero.  Only where slabs are added up -- by the test, or by the slab reduction -- is the SIGN OF A ZERO
set aside: alpha is then applied per slab and the sum starts from +0, so a sum that cancels can come out as +0 where
alpha * 0 is -0; there both sides are compared as x + 0.0.  A, B, a_mul, add and C are views into wider buffers -- NaN around the
operands, a sentinel around C that must come back bit-unchanged.

ROUNDING (arithmetic).  Standard-normal inputs against a numpy.longdouble reference, componentwise under the standard bound
of a sum of n = k + c correctly rounded operations in any order, gamma_n = n u / (1 - n u), u = 2^-53 -- nothing measured on
a device.  A route that accumulates in lower precision, or flushes, breaks it.

Every case names a row of test_gemm_host.ROUTE_CASES and asserts that row's route (tgp_gemm_route: the launcher's own
decision) before it launches: a case that no longer reaches its kernel fails."""
import numpy as np
import pytest
import torch

from test_gemm_host import ROUTE_CASES

pytestmark = pytest.mark.gpu

AL, AU, BL, BU, CL = 1, 2, 4, 8, 16
SENT = -777.0            # what surrounds C
U = 2.0 ** -53
# Roundings a term can meet outside the k accumulations (one fused multiply-add each), counted from the code:
#   operand modifier  sa * sm * sk                                  2   (gemm_tile, MOD)
#   k_gemm64          acc += the other wave group's accumulator     1
#   epilogue          alpha*acc, ca*ein, +, *cs, *rs, rv*cv, +, cb*ein, +           9   (-ffp-contract=off: none is fused)
C_EPI = 2 + 1 + 9
#   slab reduction    s += x[z] for at most 8 slabs, beta * c, +    10  (k_big_sum_slabs2d<0>)
C_REDUCE = 8 + 2
# the rounding cases' reference: long double where it is wider than float64 (x87: eps = 2^-63), else float64 and twice the bound
WIDE = np.finfo(np.longdouble).eps < 2e-19
REF_T, REF_SLACK = (np.longdouble, 1.0) if WIDE else (np.float64, 2.0)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _embed(a, top, left, right, fill):
    """`a` inside a wider buffer of `fill`; returns (buffer, the view's slices)."""
    r, c = a.shape
    buf = np.full((r + 2 * top, c + left + right), fill, dtype=np.float64)
    buf[top:top + r, left:left + c] = a
    return buf, (slice(top, top + r), slice(left, left + c))


def _up(buf, sl=None):
    t = torch.from_numpy(np.ascontiguousarray(buf)).to(_dev())
    return t, (t if sl is None else t[sl])


_PRODUCTS = {}     # the rounding cases' reference products, computed once per (shape, tri, seed, modifiers)


class Problem:
    """One product: operands drawn on the host, their padded device copies, and the reference."""

    def __init__(self, m, n, k, trans_a=0, trans_b=0, tri=0, alpha=1.0, beta=0.0, gamma=0.0, mods=(), epi=(), exact=True,
                 seed=0, nan_outside=False, pad=0, **_):
        rng = np.random.default_rng(seed)
        draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float64)) if exact else (lambda *s: rng.standard_normal(s))
        self.m, self.n, self.k, self.ta, self.tb, self.tri, self.exact = m, n, k, trans_a, trans_b, tri, exact
        self.alpha, self.beta, self.gamma, self.seed = alpha, beta, gamma, seed
        opA, opB = draw(m, k), draw(k, n)
        if tri & AL:
            opA = np.tril(opA)
        if tri & AU:
            opA = np.triu(opA)
        if tri & BL:
            opB = np.tril(opB)
        if tri & BU:
            opB = np.triu(opB)
        self.opA, self.opB = opA, opB
        self.mul = draw(m, k) if "a_mul" in mods else None
        self.ks = draw(k) if "k_scale" in mods else None
        self.add = draw(m, n) if "add" in epi else None
        self.cs = draw(n) if "col_scale" in epi else None
        self.rs = draw(m) if "row_scale" in epi else None
        self.rv = draw(m) if "rowcol" in epi else None
        self.cv = draw(n) if "rowcol" in epi else None
        self.C0 = draw(m, n) if beta != 0.0 else np.full((m, n), np.nan)      # beta = 0: C is never read
        self.epi = bool(epi) or beta != 0.0
        assert not (self.add is not None and beta != 0.0)

        # ---- device copies: the operands as stored, NaN all around them (lda > k, ldb > n, 16-byte aligned views) ----
        gA, gB = opA.copy(), opB.copy()
        if nan_outside:          # the trimming contract: 128-tiles wholly outside a declared triangle are never read
            for bi in range(m // 128):
                for bk in range((k + 127) // 128):
                    if (tri & AL and bk > bi) or (tri & AU and bk < bi):
                        gA[128 * bi:128 * bi + 128, 128 * bk:128 * bk + 128] = np.nan
            for bk in range((k + 127) // 128):
                for bj in range(n // 128):
                    if (tri & BL and bk < bj) or (tri & BU and bk > bj):
                        gB[128 * bk:128 * bk + 128, 128 * bj:128 * bj + 128] = np.nan
        st = lambda x, t: np.ascontiguousarray(x.T) if t else x
        bufA, sl = _embed(st(gA, trans_a), 1, 2, 4 + 2 * pad, np.nan)
        self.A = _up(bufA, sl)[1]
        bufB, slb = _embed(st(gB, trans_b), 1, 4, 2, np.nan)
        self.B = _up(bufB, slb)[1]
        self.kw = dict(trans_a=trans_a, trans_b=trans_b, tri=tri, alpha=alpha, beta=beta, gamma=gamma)
        if self.mul is not None:
            self.kw["a_mul"] = _up(_embed(st(self.mul, trans_a), 1, 2, 4 + 2 * pad, np.nan)[0], sl)[1]
        if self.add is not None:
            bufE, sle = _embed(self.add, 0, 2, 3, np.nan)                     # ldadd = n + 5
            self.kw["add"] = _up(bufE, sle)[1]
        for key, v in (("k_scale", self.ks), ("col_scale", self.cs), ("row_scale", self.rs), ("rowv", self.rv), ("colv", self.cv)):
            if v is not None:
                self.kw[key] = _up(v)[1]

    def c_buffer(self, slabs=0, init=None):
        """C as a view (odd ldc = n + 3, one sentinel row above and below, sentinel columns on both sides); `slabs`: a
        (slabs, m, n) view of NaN-filled slabs instead."""
        init = self.C0 if init is None else init
        buf, sl = _embed(init, 1, 1, 2, SENT)
        if slabs:
            buf = np.broadcast_to(buf, (slabs,) + buf.shape).copy()
            sl = (slice(None),) + sl
        t, view = _up(buf, sl)
        return buf, sl, t, view

    # ---- the reference, in dtype T ----
    def product(self, T=np.float64):
        key = (self.m, self.n, self.k, self.tri, self.seed, self.mul is not None, self.ks is not None, self.exact, T)
        if self.exact:
            return self._product(T)
        if key not in _PRODUCTS:
            _PRODUCTS[key] = self._product(T)
            _PRODUCTS[key].setflags(write=False)
        return _PRODUCTS[key]

    def _product(self, T):
        a = self.opA.astype(T)
        if self.mul is not None:
            a = a * self.mul.astype(T)
        if self.ks is not None:
            a = a * self.ks.astype(T)[None, :]
        return a @ self.opB.astype(T)

    def reference(self, T=np.float64, S=None):
        S = self.product(T) if S is None else S
        one, zero = T(1.0), T(0.0)
        if not self.epi:
            return T(self.alpha) * S
        ein = self.add.astype(T) if self.add is not None else (self.C0.astype(T) if self.beta != 0.0 else np.zeros_like(S))
        ca, cb = (T(self.gamma), zero) if self.add is not None else (zero, T(self.beta))
        cs = self.cs.astype(T)[None, :] if self.cs is not None else one
        rs = self.rs.astype(T)[:, None] if self.rs is not None else one
        rvcv = np.outer(self.rv, self.cv).astype(T) if self.rv is not None else zero * zero
        x = T(self.alpha) * S + ca * ein
        return x * cs * rs + rvcv + cb * ein

    def magnitude(self):
        """What the rounding bound multiplies: the sum of the absolute values of everything that is added up, each part on
        the scale it is added at (the product and gamma*add are scaled by col_scale_j row_scale_i, rowv_i colv_j and beta*C
        are added behind that scaling: the epilogue of the header, term by term)."""
        T = REF_T
        a = np.abs(self.opA).astype(T)
        if self.mul is not None:
            a = a * np.abs(self.mul).astype(T)
        if self.ks is not None:
            a = a * np.abs(self.ks).astype(T)[None, :]
        mag = abs(self.alpha) * (a @ np.abs(self.opB).astype(T))
        if self.add is not None:
            mag = mag + np.abs(self.gamma * self.add)
        if self.cs is not None:
            mag = mag * np.abs(self.cs)[None, :]
        if self.rs is not None:
            mag = mag * np.abs(self.rs)[:, None]
        if self.rv is not None:
            mag = mag + np.abs(np.outer(self.rv, self.cv))
        if self.beta != 0.0:
            mag = mag + np.abs(self.beta * self.C0)
        return mag


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want, what, zero_sign=True):
    """Bit for bit; zero_sign=False: but for the sign of a zero (where slabs are added up: the module's docstring)."""
    if not zero_sign:
        got, want = np.asarray(got) + 0.0, np.asarray(want) + 0.0
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, want %r" %
                             (what, len(bad), g.size, i, np.asarray(got)[i], np.asarray(want)[i]))


def _guards_untouched(buf_before, buf_after, sl, what):
    mask = np.ones(buf_before.shape, dtype=bool)
    mask[sl] = False
    _same_bits(buf_after[mask], buf_before[mask], what + ": the sentinels around C")


def _route_case(name, over=None):
    """The arguments of row `name` with the case's overrides, after asserting that the launcher still gives the row its route
    -- and gives it to the case as overridden."""
    from tgp.pytorch_amd import ops
    kw, route = ROUTE_CASES[name]
    assert ops.gemm_route(**kw) == route, "%s no longer takes route %d" % (name, route)
    kw = dict(kw, **(over or {}))
    if kw.pop("mod", False) and "mods" not in kw:
        kw["mods"] = ("k_scale",)
    q = {f: kw[f] for f in ("m", "n", "k", "trans_a", "trans_b", "tri", "beta", "ksplit", "xcd") if f in kw}
    assert ops.gemm_route(mod=bool(kw.get("mods")), **q) == route, "%s as run (%r) is not on route %d" % (name, q, route)
    return kw


def _expected_with_tri_c(p, ref, init):
    """TRI_C_LOWER: only the tiles with i_tile >= j_tile are computed, the others keep what C held."""
    if not (p.tri & CL):
        return ref
    out = ref.copy()
    for bi in range(p.m // 128):
        for bj in range(bi + 1, p.n // 128):
            out[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = init[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128]
    return out


def run_exact(name, seed=1, **over):
    """One launch of the row `name` (fields overridden by `over`), bit-compared with the reference; returns the result."""
    from tgp.pytorch_amd import ops
    kw = _route_case(name, over)
    ksplit, xcd = kw.pop("ksplit", 1), kw.pop("xcd", 0)
    p = Problem(exact=True, seed=seed, **kw)
    buf, sl, t, view = p.c_buffer(slabs=ksplit if ksplit > 1 else 0)
    ops.gemm_ex(p.A, p.B, view, ksplit=ksplit, xcd=xcd, **p.kw)
    torch.cuda.synchronize()
    after = t.cpu().numpy()
    _guards_untouched(buf, after, sl, name)
    got = after[sl]
    want = _expected_with_tri_c(p, p.reference(), p.C0)
    if ksplit > 1:
        # every slab of every computed tile is written (the slabs were NaN), and the slabs added in slab order are the product
        total = np.zeros((p.m, p.n))
        for z in range(ksplit):
            total = total + got[z]
        got = total if not (p.tri & CL) else np.where(np.isnan(want), got[0], total)
        for z in range(ksplit):
            _same_bits(np.isnan(after[sl][z]), np.isnan(want), "%s: slab %d, which entries are written" % (name, z))
    _same_bits(got, want, name, zero_sign=ksplit == 1)
    assert np.isfinite(want).all() or (p.tri & CL)
    return after[sl]


def gamma_n(nr):
    return nr * U / (1.0 - nr * U)


def within_rounding_bound(p, got, c, what):
    """|C - C_ref| <= gamma_(k + c) * magnitude, entry by entry; prints the largest ratio before it asserts."""
    assert p.m * p.n <= 6 * 128 * 128
    err = np.abs(got.astype(REF_T) - p.reference(REF_T))
    bound = REF_SLACK * gamma_n(p.k + c) * p.magnitude()
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))        # (an empty k range: 0 <= 0)
    print("%s: max |C - C_ref| / bound = %.3f" % (what, worst))
    assert np.isfinite(got).all()
    assert (err <= bound).all(), "%s: %d entries outside the rounding bound, worst %.3g x" % (what, int((err > bound).sum()), worst)


def run_rounding(name, seed=2, **over):
    from tgp.pytorch_amd import ops
    kw = _route_case(name, over)
    assert kw.pop("ksplit", 1) == 1
    p = Problem(exact=False, seed=seed, **kw)
    buf, sl, t, view = p.c_buffer()
    ops.gemm_ex(p.A, p.B, view, **p.kw)
    torch.cuda.synchronize()
    after = t.cpu().numpy()
    _guards_untouched(buf, after, sl, name)
    within_rounding_bound(p, after[sl], C_EPI, name)


def _names(route=None, prefix=""):
    return sorted(nm for nm, (_, r) in ROUTE_CASES.items() if (route is None or r == route) and nm.startswith(prefix))


SMALL = [nm for nm in _names() if not nm.startswith("paired_")]


# ------------------------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_exact_every_routing_shape(name):
    """Every row of the route table but the large paired ones: all four transpositions on each 128-tile route, both layouts of
    B on the 64-tile kernel, k = 16 (one stage: the prologue alone), 32 and 48 (both stage buffers), 208, one and three
    k-blocks on the 64-tile kernel, every tri flag and the OR-ed pairs on a square three-tile shape, op(B) lower with n > k
    (column tiles with an empty k range: zeros), split-K, the caller's xcd orders."""
    run_exact(name, alpha=-2.0)


@pytest.mark.parametrize("name", ["paired_bl_ta0_tb0", "paired_bu_ta0_tb1", "paired_bu_ta1_tb0", "paired_bl_ta1_tb1"])
def test_exact_large_paired_shape(name):
    """171 tile rows x 2 paired column tiles: the order the training step's chunk products take from ~16 384 rows on."""
    run_exact(name, alpha=0.5)


TRI_NAMES = [nm for nm in SMALL if ROUTE_CASES[nm][0].get("tri", 0) & (AL | AU | BL | BU) and ROUTE_CASES[nm][0].get("ksplit", 1) == 1]


@pytest.mark.parametrize("name", TRI_NAMES)
def test_exact_trimmed_tiles_are_never_read(name):
    """The trimming contract: operand tiles wholly outside the declared triangle hold NaN (the diagonal tiles true zeros),
    the result is finite and exact."""
    got = run_exact(name, nan_outside=True)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("name", ["nat_split4_al", "nat_split8_al", "triangle_ta0_tb1"])
def test_exact_split_k_trimmed_tiles_are_never_read(name):
    run_exact(name, nan_outside=True)


MODS = [("a_mul",), ("k_scale",), ("a_mul", "k_scale")]


@pytest.mark.parametrize("name", ["nat_mod", "nat_mod_ta"])
@pytest.mark.parametrize("mods", MODS, ids="+".join)
def test_exact_operand_modifiers(name, mods):
    """a_mul has A's layout, k_scale is loaded per k row (trans_a) or as pairs along the row (not): both layouts."""
    run_exact(name, mods=mods)
    run_exact(name, mods=mods, trans_b=1, seed=3)


EPIS = {
    "beta": dict(beta=-0.5),
    "add": dict(epi=("add",), gamma=4.0),
    "col_scale": dict(epi=("col_scale",)),
    "row_scale": dict(epi=("row_scale",)),
    "rowcol": dict(epi=("rowcol",)),
    "all_add": dict(epi=("add", "col_scale", "row_scale", "rowcol"), gamma=-0.25),
    "all_beta": dict(epi=("col_scale", "row_scale", "rowcol"), beta=2.0),
}


@pytest.mark.parametrize("name", ["nat_epi", "g64_256_beta_tb0", "g64_256_beta_tb1", "nat_ta1_tb1"])
@pytest.mark.parametrize("epi", sorted(EPIS))
def test_exact_epilogue_terms(name, epi):
    run_exact(name, alpha=2.0, **dict(dict(beta=0.0), **EPIS[epi]))


@pytest.mark.parametrize("name", ["nat_epi", "nat_mod"])
def test_exact_modifiers_and_epilogue_together(name):
    """k_gemm<.., MOD, EPI>."""
    for ta in (0, 1):
        run_exact(name, trans_a=ta, mods=("a_mul", "k_scale"), **EPIS["all_add"])


def test_exact_beta_zero_never_reads_c():
    """C pre-filled with NaN and beta = 0, through the plain store path and through the epilogue path of both tile sizes."""
    for name in ("nat_epi", "g64_256_beta_tb0"):
        for epi in ({}, dict(epi=("col_scale",))):
            got = run_exact(name, beta=0.0, **epi)
            assert np.isfinite(got).all()


def test_xcd_orders_never_change_a_result():
    """The same random-valued arguments under xcd 0, 1 and 2: bit for bit the same slabs (xcd 2 is live at 8 slabs)."""
    from tgp.pytorch_amd import ops
    for name in ("nat_split8_al", "nat_xcd1_11rows", "nat_ta1_tb0"):
        kw = _route_case(name)
        ksplit = kw.pop("ksplit", 1)
        kw.pop("xcd", None)
        p = Problem(exact=False, seed=11, **kw)
        outs = []
        for xcd in (0, 1, 2):
            buf, sl, t, view = p.c_buffer(slabs=ksplit if ksplit > 1 else 0)
            ops.gemm_ex(p.A, p.B, view, ksplit=ksplit, xcd=xcd, **p.kw)
            torch.cuda.synchronize()
            outs.append(t.cpu().numpy())
            _guards_untouched(buf, outs[-1], sl, name)
        _same_bits(outs[1], outs[0], name + " xcd 1 against 0")
        _same_bits(outs[2], outs[0], name + " xcd 2 against 0")
        assert np.isfinite(outs[0][sl]).all()


# ---- the split-K + reduction route of the step's M x M products ----
SCRATCH_CASES = {
    "plain": dict(m=256, n=256, k=256),
    "lm_t_r1": dict(m=256, n=256, k=256, trans_a=1, tri=AU | BL),
    "lq_lq_t": dict(m=256, n=256, k=256, trans_b=1, tri=AL | BU),
}


@pytest.mark.parametrize("case", sorted(SCRATCH_CASES))
@pytest.mark.parametrize("beta", [0.0, -2.0])
def test_exact_scratch_route(case, beta):
    """tgp_gemm_ex_f64 with scratch: 4 slabs (min(8, 256 / 4 tiles, k / 64)) into NaN-filled scratch, reduced into a strided
    C with beta; with scratch for 3 slabs only it must be the unsplit launch, and the same answer."""
    from tgp.pytorch_amd import ops
    kw = SCRATCH_CASES[case]
    p = Problem(exact=True, seed=5, alpha=-4.0, beta=beta, **kw)
    want = p.reference()
    for slabs in (4, 3):
        buf, sl, t, view = p.c_buffer()
        _, scratch = _up(np.full(slabs * p.m * p.n, np.nan))
        ops.gemm_ex(p.A, p.B, view, scratch=scratch, **p.kw)
        torch.cuda.synchronize()
        after = t.cpu().numpy()
        _guards_untouched(buf, after, sl, case)
        _same_bits(after[sl], want, "%s, scratch for %d slabs" % (case, slabs), zero_sign=False)
        used = int((~torch.isnan(scratch)).sum())
        assert used == (4 * p.m * p.n if slabs == 4 else 0), used      # every slab of every tile written / none touched


# ---- two products in one launch ----
def _pair(epi_a, epi_b, seed):
    """a = (256 x 128)(128 x 128)^T, b = (128 x 128)(128 x 384) with a lower-triangular op(B) (two of its three column tiles
    have no k range): no field of b equals a's."""
    a = Problem(256, 128, 128, trans_b=1, alpha=2.0, beta=0.5 if epi_a else 0.0, seed=seed)
    b = Problem(128, 384, 128, tri=BL, alpha=-0.5, beta=-1.0 if epi_b else 0.0, seed=seed + 1, pad=1)
    return a, b


@pytest.mark.parametrize("epi_a,epi_b", [(0, 0), (1, 1), (1, 0)], ids=["plain", "beta", "fallback"])
def test_exact_pair_launch(epi_a, epi_b):
    """k_gemm_pair (the second GemmArgs read from behind the first in the kernel arguments), and the two-launch fallback of a
    pair that does not qualify (one product with an epilogue, one without): bit-equal to the reference and to the two products
    launched one by one."""
    from tgp.pytorch_amd import ops
    a, b = _pair(epi_a, epi_b, 20)
    ca, cb = a.c_buffer(), b.c_buffer()
    da = ops.gemm_desc(a.A, a.B, ca[3], **a.kw)
    db = ops.gemm_desc(b.A, b.B, cb[3], **b.kw)
    for f, _ in da._fields_:
        if f not in ("trans_a", "k", "tri", "ksplit", "xcd") and getattr(da, f) not in (None, 0):
            assert getattr(da, f) != getattr(db, f), f
    ops.gemm_pair_ex(da, db)
    torch.cuda.synchronize()
    for p, (buf, sl, t, view) in ((a, ca), (b, cb)):
        after = t.cpu().numpy()
        _guards_untouched(buf, after, sl, "pair")
        _same_bits(after[sl], p.reference(), "pair against the reference")
        buf1, sl1, t1, view1 = p.c_buffer()
        ops.gemm_ex(p.A, p.B, view1, **p.kw)
        torch.cuda.synchronize()
        _same_bits(after, t1.cpu().numpy(), "pair against the single launch")


# ------------------------------------------------------------------------------------------------------------------
# rounding cases
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nat_ta0_tb0", "nat_ta0_tb1", "nat_ta1_tb0", "nat_ta1_tb1", "g64_256_beta_tb0", "g64_256_beta_tb1",
                                  "g64_bl_wide", "heavy_bl_wide_ta", "nat_al", "nat_au_ta"])
@pytest.mark.parametrize("epi", ["none", "all_add", "all_beta"])
def test_rounding_every_kernel(name, epi):
    """One case per kernel (k_gemm's four layouts, k_gemm64's two), plain and with the whole epilogue."""
    run_rounding(name, **dict(dict(beta=0.0), **(EPIS[epi] if epi != "none" else {})))


@pytest.mark.parametrize("name", ["nat_mod", "nat_mod_ta"])
@pytest.mark.parametrize("mods", MODS, ids="+".join)
@pytest.mark.parametrize("epi", ["none", "all_add"])
def test_rounding_modifiers(name, mods, epi):
    for tb in (0, 1):
        run_rounding(name, mods=mods, trans_b=tb, **(EPIS[epi] if epi != "none" else {}))


@pytest.mark.parametrize("name", ["nat_epi", "g64_256_beta_tb0"])
@pytest.mark.parametrize("epi", sorted(EPIS))
def test_rounding_epilogue_terms(name, epi):
    run_rounding(name, alpha=0.7, **dict(dict(beta=0.0), **EPIS[epi]))


@pytest.mark.parametrize("case", sorted(SCRATCH_CASES))
@pytest.mark.parametrize("beta", [0.0, -1.3])
def test_rounding_scratch_route(case, beta):
    """Split-K and the slab reduction: the reduction's additions join the count."""
    from tgp.pytorch_amd import ops
    p = Problem(exact=False, seed=7, alpha=0.7, beta=beta, **SCRATCH_CASES[case])
    buf, sl, t, view = p.c_buffer()
    _, scratch = _up(np.full(4 * p.m * p.n, np.nan))
    ops.gemm_ex(p.A, p.B, view, scratch=scratch, **p.kw)
    torch.cuda.synchronize()
    after = t.cpu().numpy()
    _guards_untouched(buf, after, sl, case)
    assert not bool(torch.isnan(scratch).any())         # the split route was taken
    within_rounding_bound(p, after[sl], C_EPI + C_REDUCE, case)
