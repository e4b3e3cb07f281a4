"""GPU (-m gpu): every copy of the Adam arithmetic against ONE extended-precision reference (tests/adam_model.py), step by step,
in units of the update: max|p - p_ref| / max|dp_ref| and the moments relative to their largest entry, the reference restarted
from the kernel's own float64 state each step.  Tolerance: 4 x what a float64 numpy restatement measures on the same inputs
(adam_model.F64, per hyper-parameter set; tests/test_adam_host.py).

Who owns which copy:
  k_adam (tgp_lik.hip)        test_standalone_entry_matches_the_reference[host-*]
  k_adam_dev (tgp_lik.hip)    test_standalone_entry_matches_the_reference[dev-*] (n > 131 072: the grid-stride loop past the cap of
                              512 workgroups), [groups-*] and test_groups_boundary (n_plain), test_captured_launch_...;
                              skip_off / skip_n: the general-M cases of test_in_step_update_matches_the_reference
  adam_elem (tgp_mm.hip)      test_in_step_update_matches_the_reference[fused-*] (Lam blocks + final role: LDS mirror on, the final
                              role's loop past 1 024 entries, MT = 1) and test_caller_owned_entries_... (mirror off)
  k_big_glam (tgp_big.hip)    test_in_step_update_matches_the_reference[general-*] (lam_off, also 0: Lam first; backward phase on its own)
  k_mlp_reduce (tgp_mlp.hip)  test_mlp_backward_adam_matches_the_reference
"""
import numpy as np
import pytest
import torch

import adam_model as am
import mlp_model as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 255, 256, 257, 131072, 131073, 300001)       # block edge; the grid cap 512 x 256, its first stride trip; > 2 trips
EDGES = (0, 254, 255, 256, 257, 131071, 131072, 131073, 262143, 262144)


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _launch(entry, p, g, m, v, hp, step, step_dev, n_plain=0):
    from tgp.pytorch_amd import lib as L
    h = L.load()
    lr, b1, b2, eps, wd, mx = hp
    head = (L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, b1, b2, eps)
    if entry == "host":
        L.check(h.tgp_adam_f64(*head, wd, int(step), mx, L.stream_ptr()), "tgp_adam_f64")
    elif entry == "dev":
        L.check(h.tgp_adam_dev_f64(*head, wd, L.ptr(step_dev), mx, L.stream_ptr()), "tgp_adam_dev_f64")
    else:
        L.check(h.tgp_adam_dev_groups_f64(*head, int(n_plain), wd, L.ptr(step_dev), mx, L.stream_ptr()), "tgp_adam_dev_groups_f64")


def _held(before, g, after, step, hp, wd, idx, what, name):
    """after == reference(before, g) in the update metric, at the indices idx, within 4 x the float64 figures of the set `name`."""
    lr, b1, b2, eps, _, mx = hp
    want = am.adam_ref(before[0][idx], g[idx], before[1][idx], before[2][idx], step, lr, b1, b2, eps, wd, mx)
    ep, em, ev = am.errors(after[0][idx], after[1][idx], after[2][idx], want)
    tp, tm, tv = am.tolerances(name)
    print("%s step %d: p %.3g (tol %.3g)  exp_avg %.3g (%.3g)  exp_avg_sq %.3g (%.3g)" % (what, step, ep, tp, em, tm, ev, tv))
    assert ep <= tp and em <= tm and ev <= tv, (what, step, ep, em, ev)


def _host(*ts):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy().copy() for t in ts)


def _walk(entry, n, name, n_plain, starts=am.STEP_STARTS, steps=5, warm=False):
    hp = am.HYPER[name]
    p0, gs, m0, v0 = am.make_inputs(n, seed=am.seed_of(n))
    idx = am.check_indices(n, EDGES + (n_plain - 1, n_plain))
    wd = hp[4] if entry != "groups" else np.where(np.arange(n) >= n_plain, hp[4], 0.0)[idx]
    p, m, v = _dev(p0), _dev(m0 if warm else np.zeros(n)), _dev(v0 if warm else np.zeros(n))
    gd = [_dev(g) for g in gs[:steps]]
    step_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
    for start in starts:
        if entry != "host" and start:
            step_dev[0] = start                        # the device counter preset: the host entry gets the same step as an argument
        for k in range(steps):
            before = _host(p, m, v)
            _launch(entry, p, gd[k], m, v, hp, start + k + 1, step_dev, n_plain)
            _held(before, gs[k], _host(p, m, v), start + k + 1, hp, wd, idx, "%s n=%d %s" % (entry, n, name), name)
            if entry != "host":
                assert step_dev.tolist() == [start + k + 1, 0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(am.HYPER))
@pytest.mark.parametrize("entry", ["host", "dev", "groups"])
def test_standalone_entry_matches_the_reference(entry, name, n):
    """tgp_adam_f64 / tgp_adam_dev_f64 / tgp_adam_dev_groups_f64 (n_plain = n // 2): five steps from zero state at steps 1-5, then
    from the state those left at 999-1003 and 99 996-100 000 (beta^t through exp_fast(t ln beta) in the device-counter copies)."""
    _walk(entry, n, name, n // 2)


@pytest.mark.parametrize("n", am.WARM_SIZES)
@pytest.mark.parametrize("name", sorted(am.HYPER))
@pytest.mark.parametrize("entry", ["host", "dev", "groups"])
def test_standalone_entry_from_a_state_it_did_not_produce(entry, name, n):
    """Steps 999-1001 from make_inputs' synthetic non-zero (exp_avg, exp_avg_sq): state no kernel of the project wrote."""
    _walk(entry, n, name, n // 2, starts=(am.WARM_START,), steps=am.WARM_STEPS, warm=True)


@pytest.mark.parametrize("n", [257, 131073])
@pytest.mark.parametrize("which", ["0", "1", "255", "256", "n-1", "n"])
def test_groups_boundary(n, which):
    """n_plain at the block edges and at both ends: weight decay 0.1 reaches exactly the elements [n_plain, n)."""
    n_plain = {"n-1": n - 1, "n": n}.get(which) if which.startswith("n") else int(which)
    _walk("groups", n, "short_memory", n_plain, starts=(0,), steps=3)


def test_captured_launch_replayed_equals_eager_launches():
    """One tgp_adam_dev_f64 launch captured in a graph (single stream) and replayed three times == three eager launches, bit for
    bit, and the device counter reads 3."""
    n, hp = 131073, am.HYPER["engine"]
    p0, gs, _, _ = am.make_inputs(n, seed=5)
    g = _dev(gs[0])

    def fresh():
        return (_dev(p0), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV),
                torch.zeros(2, dtype=torch.int32, device=DEV))
    pe, me, ve, se = fresh()
    for _ in range(3):
        _launch("dev", pe, g, me, ve, hp, 0, se)
    pg, mg, vg, sg = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        _launch("dev", pg, g, mg, vg, hp, 0, sg)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pg, pe) and torch.equal(mg, me) and torch.equal(vg, ve)
    assert sg.tolist() == [3, 0] and se.tolist() == [3, 0]


# ---- the copies inside the ELBO step ------------------------------------------------------------------------------------------
ENGINE_HP = (0.01, 0.9, 0.999, 1e-8, 0.0, 1)     # ElboEngine's: lr 0.01, no weight decay on the shared parameters, ascent


def _engine(N, D, M, flow, seed=5):
    from test_gpu_handoff import _engine as make
    return make(N, D, M, flow, seed=seed)


def _step_held(eng, call, n, what):
    fp = eng.fp
    before = _host(fp.data[:n], fp.exp_avg[:n], fp.exp_avg_sq[:n])
    t0 = int(eng.step_dev[0])
    call()
    g, = _host(fp.grad[:n])
    _held(before, g, _host(fp.data[:n], fp.exp_avg[:n], fp.exp_avg_sq[:n]), t0 + 1, ENGINE_HP, 0.0, np.arange(n), what, "engine")
    assert eng.step_dev.tolist() == [t0 + 1, 0]
    st = eng.status.cpu().tolist()
    assert st[0] == 0 and st[3] == 0 and st[4:] == [0, 0, 0, 0], st


LAM_FIRST = ("Lam", "Z", "raw_ls", "raw_os", "m", "lvn", "theta", "mean_a", "mean_b", "nn")


@pytest.mark.parametrize("path,N,D,M,flow,split,lam_first", [
    ("fused", 300, 4, 100, "sal2", False, False),       # LDS mirror on
    ("fused", 300, 13, 128, "sal2", False, False),      # more than 1 024 parameters outside Lam: the final role's loop
    ("fused", 64, 3, 5, None, False, False),            # MT = 1
    ("general", 600, 5, 150, "sal2", False, False),     # k_big_glam + the tail launch that skips Lam
    ("general", 700, 5, 300, None, False, False),
    ("general", 700, 5, 300, None, True, False),        # backward phase on its own after prepare | rows: the rotated ID_TGP unit
    # a caller layout with Lam at the head of the flat buffer: lam_off = 0 in k_big_glam, skip_off = 0 in the tail launch (every
    # index it touches is shifted), and on the fused path the final role's index map and LDS mirror with nothing in front of Lam
    ("general", 700, 5, 300, None, False, True),
    ("fused", 300, 4, 100, "sal2", False, True)])
def test_in_step_update_matches_the_reference(path, N, D, M, flow, split, lam_first, monkeypatch):
    """ElboEngine.step_adam, three steps: after each, the reference applied to (state before, the gradient buffer the call left)
    must give the state after -- every element of the flat buffer, so each copy is held on its own entries independently of the
    copies that own the others."""
    from tgp.pytorch_amd import engine
    if lam_first:
        monkeypatch.setattr(engine, "ORDER", LAM_FIRST)      # FlatParams lays the buffer out in this order
    eng = _engine(N, D, M, flow)
    assert eng.fp.offsets["Lam"] == (0 if lam_first else M * D + D + 1 + M)
    assert eng.fused_adam and (M > 128) == (path == "general")
    if path == "fused":
        assert (eng.fp.n - M * M > 1024) == (D == 13)

    def call():
        if split:
            eng.step_adam(3)
            eng.step_adam(4)
        else:
            eng.step_adam()
    for _ in range(3):
        _step_held(eng, call, eng.fp.n, "%s N=%d D=%d M=%d %s" % (path, N, D, M, flow))


def test_caller_owned_entries_after_theta_are_updated_from_the_callers_gradients():
    """tgp_elbo_step_adam_f64 on the fused path with an Adam range three entries longer than the model's parameters: the LDS
    mirror is off (the range holds entries the final role does not form), and the extra entries are stepped from the
    gradients the caller put there."""
    from tgp.pytorch_amd import synthetic
    N, D, M, extra = 300, 4, 100, 3
    prob = synthetic.synthetic_problem(N, D, M, seed=5, flow="sal2", S=32)
    eng = _engine(N, D, M, "sal2")
    fp, n = eng.fp, eng.fp.n
    for name in ("data", "exp_avg", "exp_avg_sq"):
        big = torch.zeros(n + extra, dtype=torch.float64, device=DEV)
        big[:n] = getattr(fp, name)
        setattr(fp, name, big)
    fp.grad = torch.zeros(n + extra + fp.extra, dtype=torch.float64, device=DEV)
    eng._out = torch.zeros(4, dtype=torch.float64, device=DEV)          # the scalars: not into the caller's gradient entries
    eng._abi_structs(prob["program"], 32, 1.0, "scale_rbf", 0, 1e-8)    # the model's and the gradients' pointers, into the new buffers
    eng.n_plain = n + extra
    # the final role mirrors its gradients in LDS only when the Adam range outside Lam is exactly what it forms (tgp_mm.hip,
    # bwd_final_role: npar == n_rest); here the range is three entries longer, which is what turns the mirror off
    npar = M * D + D + 1 + M + 1 + fp.sizes["theta"]
    assert n - M * M == npar and eng.n_plain - M * M == npar + extra
    fp.data[n:] = _dev(np.array([0.7, -1.3, 2.1]))
    mine = np.array([1e-9, -3.0, 0.0])
    fp.grad[n:n + extra] = _dev(mine)
    for _ in range(3):
        _step_held(eng, eng.step_adam, n + extra, "caller-owned tail")
        assert np.array_equal(fp.grad[n:n + extra].cpu().numpy(), mine)       # the call left them alone
    assert bool(torch.isfinite(eng._out[:3]).all())


# ---- the copy in the MLP weight-gradient reduction ----------------------------------------------------------------------------
def test_mlp_backward_adam_matches_the_reference():
    """tgp_mlp_backward_adam_f64 (D 4, H 50, L 2, 2 nets, N 129, weight decay 1e-5, dropout 0.25), three calls with the dropout
    step word = the Adam counter: g_W is the model's gradient under the masks of the counter's value BEFORE the call (a forward
    with that value reproduces ops.mlp_keep_mask), weights and moments are the reference's step from that g_W, the counter
    advances by one per call and the ticket word reads 0."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    h = L.load()
    case = (129, 4, 50, 2, 2, "tanh", 0.25)
    N, D, H, Lh, nnets, act, p = case
    X, W0, G = mm.make_case(case)
    spec = ops.MlpSpec(D, H, Lh, nnets, act=act, drop_p=p, seed=99)
    d = spec.struct(N, True)
    n = W0.size
    W, m, v = _dev(W0), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    gW = torch.zeros(n, dtype=torch.float64, device=DEV)
    Xd, Gd = _dev(X), _dev(G)
    ws = torch.empty(h.tgp_mlp_workspace_bytes(d) // 8 + 16, dtype=torch.float64, device=DEV)
    step_dev = torch.zeros(2, dtype=torch.int32, device=DEV)
    hp = (0.01, 0.9, 0.999, 1e-8, 1e-5, 1)
    ad = L.TgpAdamArgs(L.ptr(W), L.ptr(gW), L.ptr(m), L.ptr(v), n, hp[0], hp[1], hp[2], hp[3], L.ptr(step_dev), hp[5], 0)
    for c in range(3):
        assert step_dev.tolist() == [c, 0]
        masks = [[ops.mlp_keep_mask(99, c, k, l, N, H, p) for l in range(Lh)] for k in range(nnets)]
        before = _host(W, m, v)
        ref_out, ref_gW = mm.forward_backward(X, before[0], G, D, H, Lh, nnets, act, p, masks)
        out, = _host(ops.mlp_forward(spec, Xd, W, True, step_dev))
        assert mm.rel(out, ref_out) < mm.TOL_OUT, mm.rel(out, ref_out)
        L.check(h.tgp_mlp_backward_adam_f64(d, L.ptr(Xd), L.ptr(W), L.ptr(step_dev), L.ptr(Gd), L.ptr(gW), L.ptr(ws),
                                            ws.numel() * 8, ad, hp[4], L.stream_ptr()), "tgp_mlp_backward_adam_f64")
        g, = _host(gW)
        assert mm.rel(g, ref_gW) < mm.TOL_GW, mm.rel(g, ref_gW)
        _held(before, g, _host(W, m, v), c + 1, hp, hp[4], np.arange(n), "mlp_backward_adam", "engine")
    assert step_dev.tolist() == [3, 0]
