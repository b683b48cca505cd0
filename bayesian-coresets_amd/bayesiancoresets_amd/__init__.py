"""MI355X-native drop-in for the greedy sparse-NNLS path of ``bayesiancoresets``:

    import bayesiancoresets_amd as bc
    alg = bc.HilbertCoreset(X, projector, snnls=bc.snnls.GIGA)
    alg.build(1000); wts, pts, idcs = alg.get()

Namespace mirrors bayesiancoresets/__init__.py:1-2.  ``BatchPSVICoreset`` (the batch pseudocoreset)
runs with a ``DeviceProjector`` only: its pseudo-point gradients are device kernels (csrc/psvi.hip), and any other
projector raises NotImplementedError."""
from .coreset import Coreset, HilbertCoreset, UniformSamplingCoreset, SparseVICoreset, BatchPSVICoreset, QuasiNewtonCoreset, CoresetMCMC, ShardedHilbertCoreset
from .projector import BlackBoxProjector, Projector, DeviceProjector
from .linreg_sampler import LinregPosteriorSampler
from .laplace_sampler import LaplacePosteriorSampler
from .gaussian_sampler import GaussianPosteriorSampler
from .mcmc import DeviceHMC, log_joint_grad
from .predictive import log_predictive, PredictiveResult
from .discrepancy import energy_distance, stein_discrepancy, EnergyResult, SteinResult
from . import snnls
from . import util

__version__ = "0.1.0"
