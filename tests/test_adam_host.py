"""Host pins of tests/adam_model.py (no GPU): the extended-precision Adam step against torch.optim.Adam, and the measurement of
how far a plain float64 restatement is from it -- the per-set constants F64 from which tests/test_gpu_adam.py takes its
tolerance."""
import numpy as np
import pytest
import torch

import adam_model as am

SIZES = (1, 255, 256, 257, 131072, 131073, 300001)


@pytest.mark.parametrize("name", sorted(am.HYPER))
@pytest.mark.parametrize("warm", [False, True])
def test_reference_matches_torch_adam(name, warm):
    """Five torch.optim.Adam steps on the CPU; after each, the reference applied to torch's own state before the step must
    give torch's state after it (restarted every step: per-step error, no drift), within the float64 restatement's measure."""
    lr, b1, b2, eps, wd, maximize = am.HYPER[name]
    n = 1000
    p0, gs, m0, v0 = am.make_inputs(n, seed=11)
    ref = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, maximize=bool(maximize))
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    t0 = 0
    if warm:        # a state torch did not produce itself: non-zero moments and a step count of 998
        ref.grad = torch.zeros(n, dtype=torch.float64)
        opt.step()
        st = opt.state[ref]
        with torch.no_grad():
            ref.copy_(torch.from_numpy(p0))
            st["exp_avg"].copy_(torch.from_numpy(m0))
            st["exp_avg_sq"].copy_(torch.from_numpy(v0))
            st["step"].fill_(998)
        m, v, t0 = m0.copy(), v0.copy(), 998
    tp, tm, tv = am.tolerances(name)
    for k, g in enumerate(gs):
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[ref]
        assert int(st["step"]) == t0 + k + 1
        want = am.adam_ref(p, g, m, v, t0 + k + 1, lr, b1, b2, eps, wd, maximize)
        p, m, v = ref.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        ep, em, ev = am.errors(p, m, v, want)
        assert ep <= tp and em <= tm and ev <= tv, (name, k, ep, em, ev)


def test_the_metric_sees_eps_inside_the_square_root():
    """The defect the GPU tests must catch, on the host: eps moved inside the square root is far outside the tolerance in the
    update metric (and invisible in the moments, which do not contain eps)."""
    lr, b1, b2, eps, wd, maximize = am.HYPER["torch_defaults"]
    p, gs, m0, v0 = am.make_inputs(257, seed=3)
    m1 = b1 * m0 + (1 - b1) * gs[0]
    v1 = b2 * v0 + (1 - b2) * gs[0] ** 2
    wrong = p - (lr / (1 - b1 ** 7)) * m1 / np.sqrt(v1 / (1 - b2 ** 7) + eps)
    ep, _, _ = am.errors(wrong, m1, v1, am.adam_ref(p, gs[0], m0, v0, 7, lr, b1, b2, eps, wd, maximize))
    assert ep > 1e3 * am.tolerances("torch_defaults")[0], ep


def _measure(n, name, warm):
    """The largest per-step errors() of the float64 step (both powers) over one walk of the GPU tests: from zero state through the
    three counter presets, or (warm) three steps from make_inputs' non-zero state at step 999; state carried in float64."""
    lr, b1, b2, eps, wd, maximize = am.HYPER[name]
    p0, gs, m0, v0 = am.make_inputs(n, seed=am.seed_of(n))
    idx = am.check_indices(n, (0, 255, 256, 257, 131071, 131072, n - 1))
    p, m, v = p0.copy(), (m0.copy() if warm else np.zeros(n)), (v0.copy() if warm else np.zeros(n))
    worst = np.zeros(3)
    for start in ((am.WARM_START,) if warm else am.STEP_STARTS):
        for k, g in enumerate(gs[:am.WARM_STEPS] if warm else gs):
            t = start + k + 1
            want = am.adam_ref(p[idx], g[idx], m[idx], v[idx], t, lr, b1, b2, eps, wd, maximize)
            outs = [am.adam_f64(p, g, m, v, t, lr, b1, b2, eps, wd, maximize, power=pw) for pw in ("pow", "exp")]
            for o in outs:
                worst = np.maximum(worst, am.errors(o[0][idx], o[1][idx], o[2][idx], want))
            p, m, v = outs[0]
    return worst


@pytest.mark.parametrize("name", sorted(am.HYPER))
def test_float64_restatement_against_the_reference(name, capsys):
    """The measurement behind the GPU tolerance: the float64 numpy step (beta^t as b**t and as exp(t ln b)) against the
    reference on the GPU tests' own inputs -- every size, both kinds of starting state, the reference restarted from the float64
    state each step.  Asserts the set's constants in adam_model.py still bound what is measured here, and are not slack (the
    measurement is above half of them)."""
    worst = np.zeros(3)
    for n in SIZES:
        worst = np.maximum(worst, _measure(n, name, False))
    for n in am.WARM_SIZES:
        worst = np.maximum(worst, _measure(n, name, True))
    with capsys.disabled():
        print("\nfloat64 Adam restatement vs reference [%s]: p %.3g  exp_avg %.3g  exp_avg_sq %.3g" % ((name,) + tuple(worst)))
    for got, const in zip(worst, am.F64[name]):
        assert 0.5 * const <= got <= const, (name, worst, am.F64[name])


def test_a_single_element_keeps_its_gradient():
    """n = 1: no planted zero (the test would hold a kernel that does nothing), and every step moves the parameter."""
    p, gs, _, _ = am.make_inputs(1, seed=am.seed_of(1))
    assert all(g[0] != 0.0 for g in gs)
    for name in sorted(am.HYPER):
        lr, b1, b2, eps, wd, maximize = am.HYPER[name]
        assert all(am.adam_ref(p, g, [0.0], [0.0], 1, lr, b1, b2, eps, wd, maximize)[3][0] != 0 for g in gs)
