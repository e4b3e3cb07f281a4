"""Drop-in counterpart of the reference's code/main.py (same four flags, same hyper-parameters and call
sequence), running on the MI355X kernels:

    python -m tgp.pytorch_amd.main --model TGP --dataset power --train_test_seed_split 1 --num_inducing 100

`--dataset synthetic_power|synthetic_boston` uses seeded data of the same shape (the CSVs are the
reference's data files; point $TGP_DATA_ROOT at them for the real runs).  `--epochs` shortens the 15000-epoch
recipe for smoke runs.  `--flow_arch` (with `--num_blocks`, `--num_steps`) replaces the per-dataset flow of the recipe
by any generator of flows.py -- SAL, StepTanhL, ArcSL, BoxCoxL, InverseBoxCoxL, Affine -- or build_chain name (SAL_BCL,
SAL_InvBCL, SAL_AL, BCL_AL, InvBCL_AL); left out, each falls back to the recipe's value.
`--model WGP` trains the warped GP baseline (likelihoods.WarpedGaussianLinearMean: the same flow generators, applied to
the targets, shared parameters only: its flow is the data set's TGP recipe or --flow_arch, never ID_TGP's per-row networks,
which no flag can ask for here; with --likelihood bernoulli it is refused).
`--likelihood bernoulli` trains a binary classifier (SVGP or TGP; the Bernoulli probit likelihood) on
synthetic_heart / synthetic_banknote with the flows of the reference's classification script, and reports the test
negative log-likelihood and accuracy.
`--likelihood multiclass` trains a C-class classifier (SVGP: identity flows; TGP: one --flow_arch flow per class, default
SAL x 2) with the softmax likelihood over C latent GPs on synthetic_blobs, and reports the same two numbers:

    python -m tgp.pytorch_amd.main --model TGP --likelihood multiclass --dataset synthetic_blobs \\
        --train_test_seed_split 1 --num_inducing 20 --epochs 300

`--likelihood poisson` trains a count regression (SVGP: the log-Gaussian Poisson model; TGP: the flow, default SAL x 1, is
the learned link to the log-rate) on synthetic_counts, and reports the test negative log-likelihood (of the observed counts,
under the predictive pmf) and RMSE in counts beside those of the constant-rate baseline, a Poisson at the training mean.

`--likelihood negbinomial` is the same with the negative-binomial likelihood for over-dispersed counts (Var = mean + mean^2 / r):
the dispersion r is trained from --dispersion_init, and the run also prints the learned r.  synthetic_overdispersed is
synthetic_counts's log-mean under NB noise of r = 2:

    python -m tgp.pytorch_amd.main --model TGP --likelihood negbinomial --dataset synthetic_overdispersed \\
        --train_test_seed_split 1 --num_inducing 20 --epochs 2000

`--likelihood studentt --df 4` trains a robust regression (SVGP or TGP) with Student-t noise around G(f) on any regression
data set; synthetic_outliers has gross errors in a tenth of its training targets and a clean test split:

    python -m tgp.pytorch_amd.main --model SVGP --likelihood studentt --df 4 --dataset synthetic_outliers \\
        --train_test_seed_split 1 --num_inducing 50 --epochs 500

`--likelihood hetero` trains a regression with input-dependent Gaussian noise (SVGP or TGP): a second latent GP models the log
noise variance.  It reports the test negative log-likelihood and RMSE and, on synthetic_hetero (noise from 0.05 to 1.0 across
x0), the correlation of the learned with the true log noise level:

    python -m tgp.pytorch_amd.main --model TGP --likelihood hetero --dataset synthetic_hetero \\
        --train_test_seed_split 1 --num_inducing 50 --epochs 2000

`--likelihood ordinal` trains an ordinal regression (SVGP or TGP) on the ordered classes of synthetic_ratings: the
cumulative-probit likelihood with fixed, evenly spaced bin edges, so that the flow of a TGP (default SAL x 1) learns the spacing
of the levels.  It reports the test negative log-likelihood, the accuracy of the modal class and the mean absolute error of the
predictive median class, and the same three for the baseline that predicts the training class frequencies everywhere; with
--scores also the ranked probability score:

    python -m tgp.pytorch_amd.main --model TGP --likelihood ordinal --dataset synthetic_ratings \\
        --train_test_seed_split 1 --num_inducing 20 --epochs 2000

`--likelihood gamma` trains a Gamma regression with a log link (SVGP or TGP, default flow SAL x 1) on the positive targets of
synthetic_claims: y ~ Gamma(shape a, mean exp(G(f))), a trained from --shape_init.  It reports the test negative log-likelihood
and RMSE in raw units, the learned shape, and the same two for a constant baseline (a Gamma at the training mean with the
moment-matched shape); `--coverage exact` takes the 95 % interval from the exact quantiles of the mixture of Gammas:

    python -m tgp.pytorch_amd.main --model TGP --likelihood gamma --dataset synthetic_claims \\
        --train_test_seed_split 1 --num_inducing 20 --epochs 2000 --coverage exact

`--likelihood beta` trains a Beta regression with a logit link (SVGP or TGP, default flow SAL x 1) on the proportions of
synthetic_proportions: y ~ Beta(mu phi, (1 - mu) phi), mu = sigmoid(G(f)), the precision phi trained from --precision_init.  It
reports the test negative log-likelihood and RMSE, the learned precision, and the same two for a constant baseline (one Beta
moment-matched to the training targets); `--coverage exact` takes the 95 % interval from the exact quantiles of the mixture of
Betas:

    python -m tgp.pytorch_amd.main --model TGP --likelihood beta --dataset synthetic_proportions \\
        --train_test_seed_split 1 --num_inducing 20 --epochs 2000 --coverage exact

`--relevance` (SVGP or TGP, --likelihood gaussian) also prints, per input, the relevance on the test split -- the
root-mean-square slope of the predictive mean in that input (utils.input_relevance, from the HIP input gradients) -- beside the
inverse ARD length-scale.  synthetic_relevance has six inputs of which only the first two enter the targets:

    python -m tgp.pytorch_amd.main --model SVGP --dataset synthetic_relevance --relevance \\
        --train_test_seed_split 1 --num_inducing 20 --epochs 300

`--slope_significance` (same models) prints after everything else, per input, the share of test rows at which the posterior slope
of the latent function is significant at 95 % -- |E d_d f| > 1.96 sd(d_d f) under q(f), model.posterior_derivative -- which tells
a small relevance that is slope from one that is posterior noise.

`--suggest K` (same models) prints after everything else the K best distinct candidates for the next evaluation when the target is
to be maximised: points inside the bounding box of the (standardised) training inputs found by utils.suggest_candidates --
projected Adam ascent of model.acquisition from 64 starts, all in one batch on the GPU -- against the best training target, with
their log expected improvement (`--suggest_kind ei | pi | ucb` for another acquisition function).
"""
import argparse

import numpy
import torch

from . import config as cg
from .data import return_dataset
from .flow import instance_flow
from .flows import (CHAINS, SAL, Affine, ArcSL, BoxCoxL, InverseBoxCoxL, NormalCDFL, SALExp, SALSoftplus, SinhL, StepTanhL, TukeyL,
                    build_chain)
from .initializers import find_forward_params, find_forward_params_input_dependent_flow
from .kernels import instance_kernel
from .lib import BETA_MAX_PRECISION, BETA_MIN_PRECISION, GAMMA_MAX_SHAPE, GAMMA_MIN_SHAPE, RQ_MAX_ALPHA, RQ_MIN_ALPHA, STUDENT_MAX_DF
from .likelihoods import (Bernoulli, Beta, Gamma, GaussianLinearMean, GaussianNonLinearMean, HeteroscedasticGaussian, MulticlassCategorical,
                          NegativeBinomial, Ordinal, Poisson, StudentT, WarpedGaussianLinearMean)
from .models import sparse_MF_GP, sparse_MF_SP
from .trainers import Trainer_SP_classification, Trainer_SP_regression
from .utils import GREEDY_VARIANCE, KMEANS

# --kernel -> the instance_kernel name
KERNEL_CHOICES = {"rbf": "scale_rbf", "matern32": "scale_matern32", "matern52": "scale_matern52", "rq": "scale_rq"}

# code/exp_config.py:4-86
HYPER = {
    ("ID_TGP", "boston"): dict(arch="SAL", blocks=1, steps=None, act="tanh", layers=1, DR=0.5, BN=0, H=25),
    ("ID_TGP", "power"): dict(arch="SAL", blocks=3, steps=None, act="relu", layers=2, DR=0.25, BN=0, H=50),
    ("TGP", "boston"): dict(arch="StepTanhL", blocks=10, steps=2),
    ("TGP", "power"): dict(arch="SAL", blocks=2, steps=None),
    # bash_scripts/launch_test_uci_medium-small_classification.sh
    ("TGP", "heart"): dict(arch="SAL_InvBCL", blocks=1, steps=None),
    ("TGP", "banknote"): dict(arch="BCL_AL", blocks=5, steps=None),
    ("TGP", "blobs"): dict(arch="SAL", blocks=2, steps=None),
    ("TGP", "counts"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "overdispersed"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "outliers"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "hetero"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "relevance"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "ratings"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "claims"): dict(arch="SAL", blocks=1, steps=None),
    ("TGP", "proportions"): dict(arch="SAL", blocks=1, steps=None),
}
CLASSIFICATION_DATASETS = ("synthetic_heart", "synthetic_banknote")
MULTICLASS_DATASETS = ("synthetic_blobs",)
COUNT_DATASETS = ("synthetic_counts", "synthetic_overdispersed")
ORDINAL_DATASETS = ("synthetic_ratings",)
POSITIVE_DATASETS = ("synthetic_claims",)
PROPORTION_DATASETS = ("synthetic_proportions",)
FLOW_ARCHS = ("SAL", "StepTanhL", "ArcSL", "BoxCoxL", "InverseBoxCoxL", "Affine", "SinhL", "NormalCDFL", "TukeyL", "TukeyLeftL",
              "TukeyRightL", "SALSoftplus", "SALExp") + CHAINS
_PLAIN_GENERATORS = {"ArcSL": ArcSL, "BoxCoxL": BoxCoxL, "InverseBoxCoxL": InverseBoxCoxL, "Affine": Affine, "SinhL": SinhL,
                     "NormalCDFL": NormalCDFL, "TukeyL": TukeyL, "TukeyLeftL": lambda nb: TukeyL(nb, side="left"),
                     "TukeyRightL": lambda nb: TukeyL(nb, side="right"), "SALSoftplus": SALSoftplus, "SALExp": SALExp}


def main(argv=None):
    ap = argparse.ArgumentParser(description="TGP on MI355X")
    ap.add_argument("--model", required=True, help="ID_TGP, TGP, SVGP or WGP (warped GP: the flow acts on the targets)")
    ap.add_argument("--dataset", required=True,
                    choices=["boston", "power", "synthetic_boston", "synthetic_power", "synthetic_outliers", "synthetic_hetero",
                             "synthetic_relevance"]
                    + list(CLASSIFICATION_DATASETS)
                    + list(MULTICLASS_DATASETS) + list(COUNT_DATASETS) + list(ORDINAL_DATASETS) + list(POSITIVE_DATASETS)
                    + list(PROPORTION_DATASETS))
    ap.add_argument("--train_test_seed_split", required=True, type=int)
    ap.add_argument("--num_inducing", required=True, type=int)
    ap.add_argument("--epochs", type=int, default=15000)
    ap.add_argument("--flow_arch", choices=FLOW_ARCHS, default=None, help="flow generator (default: the recipe's)")
    ap.add_argument("--num_blocks", type=int, default=None, help="flow blocks (default: the recipe's)")
    ap.add_argument("--num_steps", type=int, default=None, help="tanh steps per StepTanhL block (default: the recipe's)")
    ap.add_argument("--whiten", type=int, choices=[0, 1], default=1,
                    help="1: whitened q(v) (the reference's main.py); 0: q(u) on the inducing values (is_whiten=False, eager loop)")
    ap.add_argument("--likelihood", choices=["gaussian", "bernoulli", "multiclass", "poisson", "negbinomial", "studentt", "hetero",
                                             "ordinal", "gamma", "beta"],
                    default="gaussian",
                    help="gaussian: regression (default); bernoulli: binary classification, probit link; multiclass: "
                         "softmax over C latent GPs; poisson: count regression, the flow of the GP is the log-rate; negbinomial: the same "
                         "for over-dispersed counts, with a trained dispersion r (Var = mean + mean^2 / r); studentt: "
                         "robust regression, Student-t noise of --df degrees of freedom around G(f); hetero: regression with "
                         "input-dependent Gaussian noise, a second latent GP for the log noise variance (SVGP or TGP); ordinal: "
                         "ordered classes, cumulative probit with fixed bin edges, the flow learns the spacing of the levels "
                         "(SVGP or TGP, synthetic_ratings); gamma: positive targets, Gamma noise with a log link and a trained "
                         "shape, Var = mean^2 / shape (SVGP or TGP, synthetic_claims); beta: proportions in (0, 1), Beta noise with a "
                         "logit link and a trained precision, Var = mean (1 - mean) / (1 + precision) (SVGP or TGP, "
                         "synthetic_proportions)")
    ap.add_argument("--df", type=float, default=4.0,
                    help="degrees of freedom of --likelihood studentt, fixed (not trained), 2 < df <= 1e4")
    ap.add_argument("--kernel", choices=list(KERNEL_CHOICES), default="rbf",
                    help="covariance function, ARD under an output scale: rbf (the reference's main.py); matern32, matern52: "
                         "Matern with nu = 3/2, 5/2; rq: rational quadratic with the fixed --rq_alpha (eager loop)")
    ap.add_argument("--rq_alpha", type=float, default=2.0,
                    help="alpha of --kernel rq, fixed (not trained), 1e-2 <= alpha <= 1e4")
    ap.add_argument("--dispersion_init", type=float, default=1.0,
                    help="the dispersion r of --likelihood negbinomial at the start (trained; supported range 1e-3 <= r <= 1e3)")
    ap.add_argument("--shape_init", type=float, default=1.0,
                    help="the shape of --likelihood gamma at the start (trained; supported range 0.1 <= shape <= 1e3)")
    ap.add_argument("--precision_init", type=float, default=10.0,
                    help="the precision of --likelihood beta at the start (trained; supported range 0.5 <= precision <= 1e3)")
    ap.add_argument("--mean", choices=["zero", "linear", "identity"], default="zero",
                    help="mean function of the GP: zero (the reference's main.py); linear m(x) = x a + b, trainable; identity "
                         "m(x) = x W, W the first principal direction of the training inputs (SVGP / TGP; gaussian, bernoulli, poisson or studentt)")
    ap.add_argument("--coverage", choices=["sampled", "exact"], default="sampled",
                    help="95 %% interval of the coverage metric (regression): sampled = order statistics of 100 predictive draws "
                         "per row (the reference); exact = the 2.5 %% / 97.5 %% quantiles of the predictive CDF")
    ap.add_argument("--qu", choices=["adam", "optimal", "natgrad"], default="adam",
                    help="q(u): adam = m and Lam trained by Adam like every other parameter (the reference); optimal = set to "
                         "their closed-form optimum before every step and evaluation, the hyper-parameters train on the "
                         "collapsed bound (SVGP and WGP, --whiten 1, data sets of one full batch); natgrad = one natural-gradient "
                         "step of q(u) per minibatch at step size --natgrad_lr, Adam on the other parameters (SVGP and TGP with "
                         "one latent GP, any of their likelihoods, --whiten 1, --mean zero)")
    ap.add_argument("--natgrad_lr", type=float, default=1.0,
                    help="step size of --qu natgrad in natural parameters, in (0, 1]: 1 on one full batch per epoch, below 1 with "
                         "several minibatches")
    ap.add_argument("--init_Z", choices=["kmeans", "greedy"], default="kmeans",
                    help="inducing inputs at the start: kmeans = centroids of k-means++ / Lloyd, best of 10 (the reference); greedy = "
                         "the training rows picked by greedy conditional-variance selection (pivoted Cholesky of K_XX) under the "
                         "kernel at its initial hyper-parameters; prints the share of tr(K_XX) they leave unexplained")
    ap.add_argument("--scores", action="store_true",
                    help="also print the test CRPS and 95 %% interval score (regression; raw units): exact where the predictive "
                         "CDF is, else the CRPS of 100 predictive draws per row and no interval score")
    ap.add_argument("--relevance", action="store_true",
                    help="also print, per input, the relevance on the test split (root-mean-square slope of the predictive mean in "
                         "that input, utils.input_relevance) beside the inverse ARD length-scale 1 / l_d (SVGP or TGP, --likelihood "
                         "gaussian)")
    ap.add_argument("--slope_significance", action="store_true",
                    help="also print, per input, the share of test rows at which the posterior slope of the latent function in that "
                         "input is further than 1.96 posterior standard deviations from zero (utils.slope_significance, from the HIP "
                         "derivative moments; SVGP or TGP, --likelihood gaussian): the error bar --relevance lacks")
    ap.add_argument("--suggest", type=int, default=0, metavar="K",
                    help="after everything else, print the K best distinct candidates for the next evaluation inside the bounding "
                         "box of the training inputs (standardised): utils.suggest_candidates, projected Adam ascent of the "
                         "acquisition from 64 starts against the best training target, maximising (SVGP or TGP, --likelihood gaussian)")
    ap.add_argument("--suggest_kind", choices=["log_ei", "ei", "pi", "ucb"], default="log_ei",
                    help="the acquisition function of --suggest: log expected improvement (default), expected improvement, "
                         "probability of improvement, or the upper confidence bound m1 + 2 sqrt(m2)")
    args = ap.parse_args(argv)
    base = args.dataset.replace("synthetic_", "")
    bern = args.likelihood == "bernoulli"
    ordn = args.likelihood == "ordinal"
    if ordn and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood ordinal: SVGP or TGP only")
    if ordn != (args.dataset in ORDINAL_DATASETS):
        ap.error("--likelihood ordinal goes with the ordinal data sets (%s), and they with it" % ", ".join(ORDINAL_DATASETS))
    gam = args.likelihood == "gamma"
    if gam and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood gamma: SVGP or TGP only")
    if gam and not (GAMMA_MIN_SHAPE <= args.shape_init <= GAMMA_MAX_SHAPE):
        ap.error("--shape_init: the shape must be in [0.1, 1e3], got %g" % args.shape_init)
    if gam != (args.dataset in POSITIVE_DATASETS):
        ap.error("--likelihood gamma goes with the positive data sets (%s), and they with it" % ", ".join(POSITIVE_DATASETS))
    beta = args.likelihood == "beta"
    if beta and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood beta: SVGP or TGP only")
    if beta and not (BETA_MIN_PRECISION <= args.precision_init <= BETA_MAX_PRECISION):
        ap.error("--precision_init: the precision must be in [0.5, 1e3], got %g" % args.precision_init)
    if beta != (args.dataset in PROPORTION_DATASETS):
        ap.error("--likelihood beta goes with the proportion data sets (%s), and they with it" % ", ".join(PROPORTION_DATASETS))
    pois = args.likelihood == "poisson"
    if pois and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood poisson: SVGP or TGP only")
    negb = args.likelihood == "negbinomial"
    if negb and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood negbinomial: SVGP or TGP only")
    if negb and not (1e-3 <= args.dispersion_init <= 1e3):
        ap.error("--dispersion_init: the dispersion must be in [1e-3, 1e3], got %g" % args.dispersion_init)
    if (pois or negb) != (args.dataset in COUNT_DATASETS):
        ap.error("--likelihood %s goes with the count data sets (%s)" % ("negbinomial" if negb else "poisson", ", ".join(COUNT_DATASETS)))
    stud = args.likelihood == "studentt"
    if stud and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood studentt: SVGP or TGP only")
    if stud and not (2.0 < args.df <= STUDENT_MAX_DF):
        ap.error("--df: the Student-t degrees of freedom must be in (2, 1e4], got %g" % args.df)
    if args.kernel == "rq" and not (RQ_MIN_ALPHA <= args.rq_alpha <= RQ_MAX_ALPHA):
        ap.error("--rq_alpha: the rational-quadratic alpha must be in [1e-2, 1e4], got %g" % args.rq_alpha)
    het = args.likelihood == "hetero"
    if het and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood hetero: SVGP or TGP only (no ID_TGP, no WGP)")
    if het and (args.dataset in CLASSIFICATION_DATASETS + MULTICLASS_DATASETS + COUNT_DATASETS):
        ap.error("--likelihood hetero goes with the regression data sets")
    if het and args.mean != "zero":
        ap.error("--likelihood hetero: --mean zero only (mean functions are not built for the two-GP model)")
    if het and args.qu == "optimal":
        ap.error("--likelihood hetero: --qu adam only (two coupled latent GPs: no closed-form optimal q(u))")
    if het and args.coverage == "exact":
        ap.error("--likelihood hetero: --coverage sampled only (the exact CDF of the double mixture is not built)")
    if het and args.init_Z == "greedy":
        ap.error("--init_Z greedy: one latent GP only (not --likelihood hetero)")
    if bern and args.model == "ID_TGP":
        ap.error("--likelihood bernoulli: SVGP or TGP only")
    if bern != (args.dataset in CLASSIFICATION_DATASETS):
        ap.error("--likelihood bernoulli goes with the classification data sets (%s), gaussian with the others"
                 % ", ".join(CLASSIFICATION_DATASETS))
    multi = args.likelihood == "multiclass"
    if multi and args.model not in ("SVGP", "TGP"):
        ap.error("--likelihood multiclass: SVGP or TGP only")
    if multi != (args.dataset in MULTICLASS_DATASETS):
        ap.error("--likelihood multiclass goes with the multi-class data sets (%s)" % ", ".join(MULTICLASS_DATASETS))
    if args.scores and (bern or multi):
        ap.error("--scores: regression only (the CRPS and the interval score are scores of a predictive distribution on the reals)")
    wgp = args.model == "WGP"
    if args.relevance and (args.likelihood != "gaussian" or args.model not in ("SVGP", "TGP")):
        ap.error("--relevance: SVGP or TGP with --likelihood gaussian only (the input gradients of the predictive moments are built "
                 "for the Gaussian and flow regression likelihoods; an ID_TGP's per-row flow parameters depend on x through the "
                 "networks, a WGP warps the targets)")
    if args.slope_significance and (args.likelihood != "gaussian" or args.model not in ("SVGP", "TGP")):
        ap.error("--slope_significance: SVGP or TGP with --likelihood gaussian only (one latent GP whose slope has the sign of the "
                 "prediction's: an ID_TGP's flow parameters depend on x through the networks, a WGP warps the targets, the other "
                 "likelihoods' models carry several latent GPs or a link of their own)")
    if args.suggest < 0:
        ap.error("--suggest: K >= 0")
    if args.suggest and (args.likelihood != "gaussian" or args.model not in ("SVGP", "TGP")):
        ap.error("--suggest: SVGP or TGP with --likelihood gaussian only (the acquisition functions are built for the Gaussian and "
                 "flow regression likelihoods; an ID_TGP's per-row flow parameters depend on x through the networks, a WGP warps "
                 "the targets)")
    if wgp and (bern or multi):
        ap.error("--model WGP is a regression model: --likelihood gaussian only")
    if wgp and args.flow_arch is None and ("TGP", base) not in HYPER:
        ap.error("--model WGP: no flow recipe for this data set, give --flow_arch / --num_blocks")
    if args.mean != "zero" and (wgp or multi or args.model == "ID_TGP"):
        ap.error("--mean %s: SVGP or TGP with the gaussian, bernoulli, poisson or studentt likelihood only" % args.mean)
    if args.qu == "optimal" and (args.model not in ("SVGP", "WGP") or args.likelihood != "gaussian" or not args.whiten):
        ap.error("--qu optimal: SVGP or WGP with the gaussian likelihood and --whiten 1 (the likelihood must be Gaussian in f)")
    if args.qu == "natgrad":
        if het:
            ap.error("--qu natgrad: not --likelihood hetero (two coupled latent GPs: the step is built for one)")
        if multi:
            ap.error("--qu natgrad: not --likelihood multiclass (C coupled latent GPs: the step is built for one)")
        if wgp:
            ap.error("--qu natgrad: not --model WGP (Gaussian in f on the warped targets: --qu optimal gives the exact optimum)")
        if args.model == "ID_TGP":
            ap.error("--qu natgrad: not --model ID_TGP (input-dependent flows: the step is built for shared flow parameters)")
        if not args.whiten:
            ap.error("--qu natgrad: --whiten 1 only (the step is built for the whitened q(u))")
        if args.mean != "zero":
            ap.error("--qu natgrad: --mean zero only (the step is built for the zero prior mean)")
        if not 0.0 < args.natgrad_lr <= 1.0:
            ap.error("--natgrad_lr: the step size must be in (0, 1], got %g" % args.natgrad_lr)
    if args.init_Z == "greedy" and args.likelihood == "multiclass":
        ap.error("--init_Z greedy: one latent GP only (not --likelihood multiclass)")
    if args.model == "ID_TGP" and args.flow_arch not in (None, "SAL"):
        ap.error("ID_TGP uses input-dependent SAL flows: --flow_arch SAL only")

    cg.device = "cuda:0"
    cg.set_maximum_precission()
    loaders, dc = return_dataset(args.dataset, 10000, use_validation=None, seed=args.train_test_seed_split,
                                 options={"shuffle_train": True})
    Dx, Dy = dc["Dx"], dc["Dy"]
    init_Z = KMEANS(dc["X_tr"], args.num_inducing, n_init=10, seed=cg.config_seed) if args.init_Z == "kmeans" else None

    flow_specs = None
    if args.model != "SVGP":
        hp = dict(HYPER[("TGP" if wgp else args.model, base)])     # WGP: the data set's TGP recipe (shared parameters only)
        for key, val in (("arch", args.flow_arch), ("blocks", args.num_blocks), ("steps", args.num_steps)):
            if val is not None:
                hp[key] = val
        if hp["arch"] == "StepTanhL" and hp["steps"] is None:
            ap.error("--flow_arch StepTanhL needs --num_steps")
        rest = {"input_dependent": args.model == "ID_TGP", "input_dim": Dx, "num_hidden_layers": hp.get("layers"),
                "batch_norm": hp.get("BN"), "dropout": hp.get("DR"), "hidden_dim": hp.get("H"),
                "hidden_activation": hp.get("act"), "inference": "MC_dropout"}
        rest = {k: v for k, v in rest.items() if v is not None}
        if hp["arch"] == "SAL":
            flow_specs = SAL(hp["blocks"], **rest)
        elif hp["arch"] in _PLAIN_GENERATORS:
            flow_specs = _PLAIN_GENERATORS[hp["arch"]](hp["blocks"])
        elif hp["arch"] in CHAINS:
            flow_specs = build_chain(hp["arch"], hp["blocks"], constraint=None)
        else:
            def random_flow_fn():
                return instance_flow(StepTanhL(hp["blocks"], hp["steps"], add_f0=True))
            Ytr = dc["Y_tr"]
            x_in = numpy.linspace(float(Ytr.min()) - 1, float(Ytr.max()) + 1, 5000)
            flow_specs, mse = find_forward_params(x_in, x_in.copy(), random_flow_fn, num_restarts=1, num_epochs=2000)
            if numpy.any(numpy.isnan(numpy.array(mse))):
                raise RuntimeError("Got MSE loss to Nan on the flow initializer.")
        if args.model == "ID_TGP":
            T_flow = instance_flow(flow_specs) if isinstance(flow_specs, list) else flow_specs
            flow_specs, _ = find_forward_params_input_dependent_flow(loaders[0], FLOW=T_flow, num_epochs=2000, noise_var=0.0)

    if multi:
        Dy = dc["num_classes"]              # one latent GP (and one flow) per class
        lik = MulticlassCategorical(Dy)
    elif bern:
        lik = Bernoulli()
    elif pois:
        lik = Poisson()
    elif negb:
        lik = NegativeBinomial(dispersion_init=args.dispersion_init)
    elif gam:
        lik = Gamma(shape_init=args.shape_init, quadrature_points=cg.quad_points)
    elif beta:
        lik = Beta(precision_init=args.precision_init, quadrature_points=cg.quad_points)
    elif ordn:
        lik = Ordinal(dc["num_classes"], quadrature_points=cg.quad_points)     # the default edges: unit spacing, centred
    elif het:
        Dy = 2                           # latent GP 0: f (with the flow), latent GP 1: h, the log noise variance (no flow)
        lik = HeteroscedasticGaussian(noise_init=0.05, quadrature_points=cg.quad_points)
    elif stud:
        lik = StudentT(out_dim=Dy, noise_init=0.05, noise_is_shared=False, quadrature_points=cg.quad_points, df=args.df)
    elif wgp:
        lik = WarpedGaussianLinearMean(out_dim=Dy, noise_init=0.05, noise_is_shared=False, flow=flow_specs,
                                       quad_points=cg.quad_points)
    elif args.model == "SVGP":
        lik = GaussianLinearMean(out_dim=Dy, noise_init=0.05, noise_is_shared=False)
    else:
        lik = GaussianNonLinearMean(out_dim=Dy, noise_init=0.05, noise_is_shared=False, quadrature_points=cg.quad_points)
    kernel_init = {"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6}
    if args.kernel == "rq":
        kernel_init["alpha"] = args.rq_alpha
    K = instance_kernel(KERNEL_CHOICES[args.kernel], ard_num_dim=Dx, num_multioutput=Dy, kernel_is_shared=False,
                        init_params=kernel_init)
    if args.init_Z == "greedy":
        init_Z, sel = GREEDY_VARIANCE(dc["X_tr"], args.num_inducing, K, return_info=True)
        print("init_Z greedy: trace[M]/trace[0] = %.6e" % float(sel["trace"][-1] / sel["trace"][0]))
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    common = dict(model_specs=[args.mean, K], X=dc["X_tr"], init_Z=init_Z, N=dc["N_tr"], likelihood=lik, num_outputs=Dy,
                  is_whiten=bool(args.whiten), K_is_shared=False, mean_is_shared=False, Z_is_shared=False, q_U_is_shared=False,
                  add_noise_inducing=0.0, init_params=ip)
    if args.model == "SVGP" or wgp:
        model = sparse_MF_GP(**common)
    else:
        # (multi-class: every class builds its own flow from the same spec list)
        model = sparse_MF_SP(flow_specs=[flow_specs] * Dy if multi else [flow_specs, [("identity", [])]] if het else [flow_specs],
                             flow_connection="single", be_fully_bayesian=False, **common)
    model.to(cg.device)

    lr = 0.01
    specs = [[]]
    if args.model == "ID_TGP":
        sched = [[lr, n] for n, _ in model.named_parameters() if "G_matrix" in n and "NNets" not in n]
        sched.append([lr, 1e-5, "NNets"])
        specs[0].extend(sched)
    Y_std = (torch.ones((Dy,)) * dc["Y_std"]).to(cg.device)
    trainer_cls = Trainer_SP_classification if (bern or multi) else Trainer_SP_regression
    trainer = trainer_cls(model=model, data_loaders=loaders, validate_each=max(args.epochs // 10, 1), plot=False,
                                    track=False, Y_std=Y_std, plot_each=-1, S_test=100, inference_in_cpu=True,
                                    coverage=args.coverage, qu=args.qu, natgrad_lr=args.natgrad_lr)
    trainer.train(epochs=args.epochs, lr_ALL=lr, opt="adam", keep_parameter_groups=True,
                  optimisation_schedule=([1.0], specs), lr_groups=None)
    res = trainer.compute_metrics()
    if bern or multi:                # (logL_train, acc_train, logL_valid, acc_valid, logL_test, acc_test)
        print("Dataset {}, num inducing points {}, model {}, Test Negative LOGL {:.3f}".format(
            args.dataset, args.num_inducing, args.model, -res[4]))
        print("Dataset {}, num inducing points {}, model {}, Test Accuracy {:.3f}".format(
            args.dataset, args.num_inducing, args.model, res[5]))
        return res
    if ordn:
        # the class of the test rows by the predictive pmf: its mode, and its median read from the CDF; beside them the baseline
        # that predicts the training class frequencies everywhere
        Kc = lik.num_classes
        y_te = dc["Y_te"].reshape(-1)
        model.set_is_training(False)
        pmf = model.predictive_pmf(dc["X_te"].to(cg.device), Kc - 1).cpu()
        acc = (pmf.argmax(1).to(y_te.dtype) == y_te).double().mean().item()
        median = (pmf.cumsum(1) < 0.5).sum(1).clamp(max=Kc - 1).to(y_te.dtype)
        mae = (median - y_te).abs().mean().item()
        freq = torch.bincount(dc["Y_tr"].reshape(-1).long(), minlength=Kc).to(y_te.dtype) / dc["Y_tr"].numel()
        base_nll = -torch.log(freq[y_te.long()]).mean().item()
        base_acc = (freq.argmax().to(y_te.dtype) == y_te).double().mean().item()
        base_mae = ((freq.cumsum(0) < 0.5).sum().clamp(max=Kc - 1).to(y_te.dtype) - y_te).abs().mean().item()
        print("Dataset {}, num inducing points {}, model {}, Test Negative LOGL {:.3f}".format(
            args.dataset, args.num_inducing, args.model, -res[6]))
        print("Dataset {}, num inducing points {}, model {}, Test Accuracy (modal class) {:.3f}".format(
            args.dataset, args.num_inducing, args.model, acc))
        print("Dataset {}, num inducing points {}, model {}, Test MAE (median class) {:.3f}".format(
            args.dataset, args.num_inducing, args.model, mae))
        print("Dataset {}, class frequencies, Test Negative LOGL {:.3f}, Test Accuracy {:.3f}, Test MAE {:.3f}".format(
            args.dataset, base_nll, base_acc, base_mae))
        if args.scores:
            rps = model.predictive_crps(dc["X_te"].to(cg.device), dc["Y_te"].to(cg.device), kmax=Kc - 1).mean().item()
            print("Dataset {}, num inducing points {}, model {}, Test ranked probability score {:.4f}".format(
                args.dataset, args.num_inducing, args.model, rps))
        return res
    if pois or negb:
        # the constant-rate baseline: a Poisson at the mean of the training counts, its NLL and RMSE on the test counts
        rate, y_te = dc["Y_tr"].mean(), dc["Y_te"].reshape(-1)
        base_nll = -(y_te * torch.log(rate) - rate - torch.lgamma(y_te + 1.0)).mean().item()
        base_rmse = ((y_te - rate) ** 2).mean().sqrt().item()
        print("Dataset {}, num inducing points {}, model {}, Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, args.num_inducing, args.model, -res[6], res[7]))
        print("Dataset {}, constant rate {:.3f}, Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, rate.item(), base_nll, base_rmse))
        if negb:
            print("Dataset {}, num inducing points {}, model {}, learned dispersion r {:.3f}{}".format(
                args.dataset, args.num_inducing, args.model, float(lik.dispersion),
                "" if "dispersion" not in dc else " (true r {:.3f})".format(dc["dispersion"])))
        if args.scores:
            print("Dataset {}, num inducing points {}, model {}, Test CRPS {:.4f} (sampled), Test interval score (95%) n/a".format(
                args.dataset, args.num_inducing, args.model, trainer.compute_scores()["test"]["crps"]))
        return res
    if gam:
        # the constant baseline: one Gamma everywhere, at the mean of the training targets with the moment-matched shape
        # mean^2 / variance; its NLL and RMSE on the test targets
        y_tr, y_te = dc["Y_tr"].reshape(-1), dc["Y_te"].reshape(-1)
        mean = y_tr.mean()
        a0 = mean ** 2 / y_tr.var(unbiased=False)
        base_nll = -(a0 * torch.log(a0 / mean) - torch.lgamma(a0) + (a0 - 1.0) * torch.log(y_te) - a0 * y_te / mean).mean().item()
        base_rmse = ((y_te - mean) ** 2).mean().sqrt().item()
        print("Dataset {}, num inducing points {}, model {}, Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, args.num_inducing, args.model, -res[6], res[7]))
        print("Dataset {}, num inducing points {}, model {}, Test coverage (95%, {}) {:.3f}".format(
            args.dataset, args.num_inducing, args.model, args.coverage, res[8]))
        print("Dataset {}, constant Gamma (mean {:.3f}, shape {:.3f}), Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, mean.item(), a0.item(), base_nll, base_rmse))
        print("Dataset {}, num inducing points {}, model {}, learned shape {:.3f}{}".format(
            args.dataset, args.num_inducing, args.model, float(lik.shape),
            "" if "shape" not in dc else " (true shape {:.3f})".format(dc["shape"])))
        if args.scores:
            print("Dataset {}, num inducing points {}, model {}, Test CRPS {:.4f} (sampled), Test interval score (95%) n/a".format(
                args.dataset, args.num_inducing, args.model, trainer.compute_scores()["test"]["crps"]))
        return res
    if beta:
        # the constant baseline: one Beta everywhere, moment-matched to the training targets (mean m, precision
        # m (1 - m) / variance - 1); its NLL and RMSE on the test targets
        y_tr, y_te = dc["Y_tr"].reshape(-1), dc["Y_te"].reshape(-1)
        mean = y_tr.mean()
        p0 = mean * (1.0 - mean) / y_tr.var(unbiased=False) - 1.0
        a0, b0 = mean * p0, (1.0 - mean) * p0
        base_nll = -(torch.lgamma(p0) - torch.lgamma(a0) - torch.lgamma(b0) + (a0 - 1.0) * torch.log(y_te)
                     + (b0 - 1.0) * torch.log1p(-y_te)).mean().item()
        base_rmse = ((y_te - mean) ** 2).mean().sqrt().item()
        print("Dataset {}, num inducing points {}, model {}, Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, args.num_inducing, args.model, -res[6], res[7]))
        print("Dataset {}, num inducing points {}, model {}, Test coverage (95%, {}) {:.3f}".format(
            args.dataset, args.num_inducing, args.model, args.coverage, res[8]))
        print("Dataset {}, constant Beta (mean {:.3f}, precision {:.3f}), Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, mean.item(), p0.item(), base_nll, base_rmse))
        print("Dataset {}, num inducing points {}, model {}, learned precision {:.3f}{}".format(
            args.dataset, args.num_inducing, args.model, float(lik.precision),
            "" if "precision" not in dc else " (true precision {:.3f})".format(dc["precision"])))
        if args.scores:
            print("Dataset {}, num inducing points {}, model {}, Test CRPS {:.4f} (sampled), Test interval score (95%) n/a".format(
                args.dataset, args.num_inducing, args.model, trainer.compute_scores()["test"]["crps"]))
        return res
    if args.model == "ID_TGP":       # the reference's result lines (main.py:309-324)
        print("Dataset {}, num inducing points {}, POINT ESTIMATE FLOW , Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, args.num_inducing, -res[6], res[7]))
    else:
        print("Dataset {}, num inducing points {}, model {}, Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, args.num_inducing, args.model, -res[6], res[7]))
    if het and "noise_std_te" in dc:
        # how well the learned noise level follows the true one: Pearson correlation of log median sigma(x*) with log sigma(x*)
        # over the test rows (invariant to the targets' standardisation)
        learned = torch.log(model.predictive_noise_std(dc["X_te"].to(cg.device), 0.5)[0]).cpu()
        corr = torch.corrcoef(torch.stack((learned, torch.log(dc["noise_std_te"]))))[0, 1].item()
        print("Dataset {}, num inducing points {}, model {}, log noise std correlation {:.3f}".format(
            args.dataset, args.num_inducing, args.model, corr))
    if args.scores:
        sc = trainer.compute_scores()["test"]
        print("Dataset {}, num inducing points {}, model {}, Test CRPS {:.4f}, Test interval score (95%) {}".format(
            args.dataset, args.num_inducing, args.model, sc["crps"],
            "n/a" if sc["interval_score"] is None else "{:.4f}".format(sc["interval_score"])))
    if args.relevance:
        rel, ils = trainer.compute_relevance()
        for d in range(rel.numel()):
            print("Dataset {}, num inducing points {}, model {}, input {} relevance {:.4f}, 1/lengthscale {:.4f}".format(
                args.dataset, args.num_inducing, args.model, d, rel[d].item(), ils[d].item()))
    if args.model == "ID_TGP":
        model.be_fully_bayesian(True)
        res = trainer.compute_metrics()
        print("Dataset {}, num inducing points {}, BAYESIAN FLOW , Test Negative LOGL {:.3f}, Test RMSE {:.3f}".format(
            args.dataset, args.num_inducing, -res[6], res[7]))
    if args.slope_significance:
        sig = trainer.compute_slope_significance()
        for d in range(sig.numel()):
            print("Dataset {}, num inducing points {}, model {}, input {} slope significant (95%) on {:.4f} of the test rows".format(
                args.dataset, args.num_inducing, args.model, d, sig[d].item()))
    if args.suggest:
        for i, (x, val) in enumerate(trainer.compute_suggestions(args.suggest, args.suggest_kind)):
            print("Dataset {}, num inducing points {}, model {}, candidate {} {} {:.6g} at x = [{}]".format(
                args.dataset, args.num_inducing, args.model, i, args.suggest_kind, val, ", ".join("%.6f" % t for t in x.tolist())))
    return res


if __name__ == "__main__":
    main()
