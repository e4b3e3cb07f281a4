"""Flow *spec generators* with the reference's call signatures and list-of-(name, init_dict) output format
(code/dsp/flows.py: build_chain :79-112, SAL :115-136, BoxCoxL :140-165, InverseBoxCoxL :169-192, ArcSL :197-217,
Affine :223-235, StepTanhL :239-277).  Same defaults, same init values and the same numpy.random draw order, so a seeded
call returns the reference's specs.  The step generators other than StepTanhL (StepSAL, StepArcSL, StepBoxCoxL, ...) are
not provided: their step flows of mixed kinds have no HIP program.  A Box-Cox `constraint` passes through into the spec;
flow.BoxCoxFlow refuses anything but None.
SinhL, NormalCDFL, TukeyL, SALSoftplus and SALExp are this package's own: the reference has the flows (models/flow.py) but no
generator for them, so their defaults and their numpy.random draw order are defined in their docstrings."""
import numpy
import torch

from .utils import inv_softplus


def _common(options):
    return (options.get("set_res", False), options.get("add_f0", False), options.get("init_random", False),
            options.get("constraint", None))


def _input_dependent(options):
    dep = bool(options.get("input_dependent", False))
    if dep:
        assert "input_dim" in options, "You set to use input_dependent flows but the input dimension is not provided."
    cfg = {k: options[k] for k in ("batch_norm", "dropout", "hidden_dim", "hidden_activation", "num_hidden_layers",
                                   "inference") if k in options}
    return dep, options.get("input_dim", -1), cfg


def SAL(num_blocks, **kwargs):
    """[sinh_arcsinh, affine] x num_blocks; default init a=0,b=1 / a=1,b=0 is the identity map."""
    set_res, addf0, init_random, _ = _common(kwargs)
    dep, input_dim, cfg = _input_dependent(kwargs)
    blocks = []
    for _ in range(num_blocks):
        if init_random:
            a_aff, b_aff = numpy.random.randn(2)
            a_sal, b_sal = numpy.random.randn(2)
        else:
            a_aff, b_aff, a_sal, b_sal = 1.0, 0.0, 0.0, 1.0
        blocks.append(("sinh_arcsinh", {"init_a": a_sal, "init_b": b_sal, "add_init_f0": addf0,
                                        "set_restrictions": set_res, "input_dependent": dep, "input_dim": input_dim,
                                        "input_dependent_config": cfg}))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": set_res}))
    return blocks


def StepTanhL(num_blocks, num_steps, **kwargs):
    """[step_flow(num_steps x tanh), affine] x num_blocks; needs the identity initialiser (initializers.py)."""
    _, addf0, init_random, _ = _common(kwargs)
    if "set_res" in kwargs:
        assert kwargs["set_res"] is True, "In the step tanh flow set_res has to be True for num_steps > 1"
    dep, input_dim, cfg = _input_dependent(kwargs)
    blocks = []
    for _ in range(num_blocks):
        steps = []
        for _s in range(num_steps):
            e1, e2, e3, e4 = numpy.random.randn(4)
            if not init_random:
                e2 = inv_softplus(torch.abs(torch.tensor((e2 + 1.0) / float(num_steps)))).item()
                e4 = inv_softplus(torch.abs(torch.tensor((e4 + 1.0) / float(num_steps)))).item()
            steps.append(("tanh", {"init_a": e1, "init_b": e2, "init_c": e3, "init_d": e4, "add_init_f0": False,
                                   "set_restrictions": True, "input_dependent": dep, "input_dim": input_dim,
                                   "input_dependent_config": cfg}))
        a_aff, b_aff = numpy.random.randn(2) if init_random else (1.0, 0.0)
        blocks.append(("step_flow", {"flow_arr": steps, "add_init_f0": addf0}))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": False}))
    return blocks


def BoxCoxL(num_blocks, **kwargs):
    """[boxcox, affine] x num_blocks; default lam = 5 (init_random: randn(1) + 1 and no constraint)."""
    set_res, addf0, init_random, constraint = _common(kwargs)
    blocks = []
    for _ in range(num_blocks):
        if init_random:
            a_aff, b_aff = numpy.random.randn(2)
            init_lam = numpy.random.randn(1) + 1.
            constraint = None
        else:
            a_aff, b_aff = 1.0, 0.0
            init_lam = 5.0
        blocks.append(("boxcox", {"init_lam": init_lam, "add_init_f0": addf0, "constraint": constraint}))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": set_res}))
    return blocks


def InverseBoxCoxL(num_blocks, **kwargs):
    """[inverseboxcox, affine] x num_blocks; default lam = 5 (init_random: randn(1) + 1; the constraint is kept)."""
    set_res, addf0, init_random, constraint = _common(kwargs)
    blocks = []
    for _ in range(num_blocks):
        if init_random:
            a_aff, b_aff = numpy.random.randn(2)
            init_lam = numpy.random.randn(1) + 1.
        else:
            a_aff, b_aff = 1.0, 0.0
            init_lam = 5.0
        blocks.append(("inverseboxcox", {"init_lam": init_lam, "add_init_f0": addf0, "constraint": constraint}))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": set_res}))
    return blocks


def ArcSL(num_blocks, **kwargs):
    """[arcsinh, affine] x num_blocks.  randn(4) is drawn for the arcsinh parameters with or without init_random."""
    set_res, addf0, init_random, _ = _common(kwargs)
    blocks = []
    for _ in range(num_blocks):
        if init_random:
            a_aff, b_aff = numpy.random.randn(2)
            a_arc, b_arc, c_arc, d_arc = numpy.random.randn(4)
        else:
            a_aff, b_aff = 1.0, 0.0
            a_arc, b_arc, c_arc, d_arc = numpy.random.randn(4)
            b_arc += 1
            d_arc += 1
        blocks.append(("arcsinh", {"init_a": a_arc, "init_b": b_arc, "init_c": c_arc, "init_d": d_arc,
                                   "add_init_f0": addf0, "set_restrictions": set_res}))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": set_res}))
    return blocks


def _raw(value, restricted):
    """The raw parameter whose used value is `value`: inv_softplus(value) where the block puts softplus on it."""
    return inv_softplus(torch.tensor(float(value), dtype=torch.float64)).item() if restricted else float(value)


def _four_param_layers(name, num_blocks, defaults, kwargs, extra=None):
    """[name, affine] x num_blocks for a block a + b*h((f-c)/d).  This package's own generator (the reference has none for
    these flows).  numpy.random draw order, fixed here: per block, with init_random only, randn(2) for the affine block's
    (a, b), then randn(4) for the block's (a, b, c, d); without init_random nothing is drawn and (a, b, c, d) are the USED
    values of `defaults` (b and d as raw values through inv_softplus when the block is restricted)."""
    set_res, addf0, init_random, _ = _common(kwargs)
    restricted = bool(set_res or addf0)
    blocks = []
    for _ in range(num_blocks):
        if init_random:
            a_aff, b_aff = numpy.random.randn(2)
            a, b, c, d = numpy.random.randn(4)
        else:
            a_aff, b_aff = 1.0, 0.0
            a, b, c, d = defaults
            b, d = _raw(b, restricted), _raw(d, restricted)
        init = {"init_a": a, "init_b": b, "init_c": c, "init_d": d, "add_init_f0": addf0, "set_restrictions": set_res}
        init.update(extra or {})
        blocks.append((name, init))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": set_res}))
    return blocks


def SinhL(num_blocks, **kwargs):
    """[sinh, affine] x num_blocks.  Default a = c = 0, b = d = 3: 3 sinh(f/3) = f + f^3/54 + ..., near the identity on the
    range of standardised targets.  Draw order: _four_param_layers."""
    return _four_param_layers("sinh", num_blocks, (0.0, 3.0, 0.0, 3.0), kwargs)


def NormalCDFL(num_blocks, **kwargs):
    """[normalCDF, affine] x num_blocks.  Default c = 0, d = 3, b = 3 sqrt(2 pi), a = -b/2: the value 0 and the slope
    b phi(0)/d = 1 at the origin.  Draw order: _four_param_layers."""
    b = 3.0 * numpy.sqrt(2.0 * numpy.pi)
    return _four_param_layers("normalCDF", num_blocks, (-0.5 * b, b, 0.0, 3.0), kwargs, {"is_learnable": True})


def TukeyL(num_blocks, side=None, **kwargs):
    """[tukey | tukey_left | tukey_right, affine] x num_blocks (side None | "left" | "right").  This package's own generator.
    Default gamma = 0.1 (side None, "right") or -0.1 ("left") and h = softplus(h_raw) = 0.01 -- the raw values are chosen
    accordingly.  Draw order, with init_random only: per block randn(2) for the affine block's (a, b), then randn(2) for the raw
    (g, h)."""
    if side not in (None, "left", "right"):
        raise ValueError("TukeyL: side must be None, 'left' or 'right' (got {!r})".format(side))
    set_res, addf0, init_random, _ = _common(kwargs)
    if addf0:
        raise ValueError("TukeyL: add_f0 is not supported (the reference never adds f0 to a Tukey flow)")
    name = "tukey" if side is None else "tukey_" + side
    blocks = []
    for _ in range(num_blocks):
        if init_random:
            a_aff, b_aff = numpy.random.randn(2)
            g, h = numpy.random.randn(2)
        else:
            a_aff, b_aff = 1.0, 0.0
            g, h = _raw(0.1, side is not None), _raw(0.01, True)
        blocks.append((name, {"init_g": g, "init_h": h, "add_init_f0": False}))
        blocks.append(("affine", {"init_a": a_aff, "init_b": b_aff, "set_restrictions": set_res}))
    return blocks


def SALSoftplus(num_blocks, **kwargs):
    """SAL(num_blocks) followed by one softplus head: a positive-range flow (this package's own generator; SAL's draw order)."""
    return SAL(num_blocks, **kwargs) + [("softplus", {})]


def SALExp(num_blocks, **kwargs):
    """SAL(num_blocks) followed by one exp head: a positive-range flow (this package's own generator; SAL's draw order)."""
    return SAL(num_blocks, **kwargs) + [("exp", {})]


def Affine(num_blocks, **kwargs):
    """[affine] x num_blocks; default a=1, b=0."""
    set_res, _, init_random, _ = _common(kwargs)
    blocks = []
    for _ in range(num_blocks):
        a, b = numpy.random.randn(2) if init_random else (1.0, 0.0)
        blocks.append(("affine", {"init_a": a, "init_b": b, "set_restrictions": set_res}))
    return blocks


CHAINS = ("SAL_BCL", "SAL_InvBCL", "SAL_AL", "BCL_AL", "InvBCL_AL")


def build_chain(flow_combination, num_blocks, **kwargs):
    """num_blocks x the pair of generators a chain name lists, one block of each (SAL_BCL = SAL(1) + BoxCoxL(1), ...).
    The chains with a Box-Cox generator read kwargs['constraint'] (a KeyError without it, as in the reference)."""
    if flow_combination not in CHAINS:
        raise ValueError("unknown flow combination {} (one of {})".format(flow_combination, ", ".join(CHAINS)))
    blocks = []
    if flow_combination == "SAL_AL":
        for _ in range(num_blocks):
            blocks.extend(SAL(1))
            blocks.extend(ArcSL(1))
        return blocks
    constraint = kwargs["constraint"]
    for _ in range(num_blocks):
        if flow_combination == "SAL_BCL":
            blocks.extend(SAL(1))
            blocks.extend(BoxCoxL(1, constraint=constraint))
        elif flow_combination == "SAL_InvBCL":
            blocks.extend(SAL(1))
            blocks.extend(InverseBoxCoxL(1, constraint=constraint))
        elif flow_combination == "BCL_AL":
            blocks.extend(BoxCoxL(1, constraint=constraint))
            blocks.extend(ArcSL(1))
        else:
            blocks.extend(InverseBoxCoxL(1, constraint=constraint))
            blocks.extend(ArcSL(1))
    return blocks
