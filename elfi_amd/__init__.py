"""elfi_amd -- the MI355X (gfx950) hot path for ELFI (elfi-dev/elfi).

One data-parallel path, built from scratch in HIP behind ELFI's own operation and
surrogate-model interfaces:

  * batched summary -> distance evaluation (elfi.Distance / elfi.AdaptiveDistance
    operations; the reference delegates to scipy.spatial.distance.cdist), and
  * the BOLFI Gaussian-process surrogate loop (the `target_model=` object of
    elfi.BOLFI; the reference delegates to GPy).

Everything else (graph compilation, samplers, storage, plotting ...) stays reference
ELFI.  The compute lives in libelfihip.so (C ABI: include/elfihip.h); this package is
the thin host-side mirror of the reference interfaces.  See DESIGN.md / INTEGRATION.md.
"""
from ._lib import (LIB_PATH, Context, ElfiHipError, default_context, device_count, load_library,  # noqa: F401
                   set_device_handover)
from .distance import (AdaptiveDistanceState, HipDiscrepancy, HipDistance, cdist_cols,  # noqa: F401
                       cdist_rows, nested_weighted_euclidean, welford_update)

from .gmix import GMDistribution  # noqa: F401
from .weighted import weighted_sample_quantile, weighted_var  # noqa: F401
from .gp import GPHandle, HipGPRegression, stochastic_optimization  # noqa: F401
from .selection import RunningBest, merge_batch, smallest_k  # noqa: F401
from .sampler import HipRejection, hip_rejection_class  # noqa: F401
from .distance import adaptive_batch, randn_rows  # noqa: F401
from .adaptive import hip_adaptive_distance_class  # noqa: F401
from .smc import HipAdaptiveDistanceSMC, HipAdaptiveThresholdSMC, HipSMC, hip_smc_class  # noqa: F401
from .summaries import autocov, gauss_distance, ma2_distance, ma2_draw_distance, ss_mean, ss_var  # noqa: F401
from .summaries import arch_summaries, lorenz_summaries, mg1_summaries  # noqa: F401
from .summaries import bignk_summaries, gnk_summaries  # noqa: F401
from .summaries import poisson, ricker_summaries  # noqa: F401
from .summaries import lotka_volterra_draws, lotka_volterra_summaries  # noqa: F401
from .summaries import daycare_distance, daycare_draws, daycare_summaries  # noqa: F401
from .fused_models import arch_model, lorenz_model, mg1_model  # noqa: F401
from .fused_models import bignk_model, gnk_model  # noqa: F401
from .fused_models import ricker_model  # noqa: F401
from .summaries import levy_stable, toad_summaries  # noqa: F401
from .fused_models import toad_model  # noqa: F401
from .summaries import levy_stable_general, sv_summaries  # noqa: F401
from .fused_models import sv_model  # noqa: F401
from .summaries import scratch_assay_draws, scratch_assay_shape, scratch_assay_summaries  # noqa: F401
from .fused_models import scratch_assay_model  # noqa: F401
from .summaries import ar1_series, bdm_clusters, bdm_draws  # noqa: F401
from .fused_models import ar1_model, ar1_rows, bdm_model, bdm_rows  # noqa: F401
from .fused_models import lotka_volterra_model, lv_summary_rows  # noqa: F401
from .fused_models import daycare_model, daycare_summary_rows  # noqa: F401
from .lcb_acquisition import HipLCBSC  # noqa: F401
from .posterior import HipBolfiPosterior, sample_posterior  # noqa: F401
from .bolfi import HipBOLFI, hip_bolfi_class  # noqa: F401
from . import chains, fused_models, multistart, priors  # noqa: F401
from .maxvar_acquisition import HipExpIntVar, HipMaxVar, HipRandMaxVar  # noqa: F401
from .synlik import (HipBSL, hip_bsl_class, log_SL_stdev, robust_likelihood, select_penalty,  # noqa: F401
                     semi_loglik, semiparametric_likelihood, slice_gamma, slice_gamma_mean, slice_gamma_variance,
                     standard_likelihood, syn_loglik, unbiased_likelihood)
from .logratio import HipLogisticRegression, hip_logistic_regression_class, log_ratio  # noqa: F401
from .bolfire import HipBOLFIRE, HipBOLFIREPosterior, hip_bolfire_class  # noqa: F401
from .twostage import (HipTwoStageSelection, hip_two_stage_selection_class, knn_entropy, mrsse,  # noqa: F401
                       subset_best)
from .adjust import HipLinearAdjustment, adjust_posterior, hip_linear_adjustment_class, linear_adjust  # noqa: F401
from .kliep import HipDensityRatioEstimation, hip_density_ratio_class, kliep_fit, kliep_ratio  # noqa: F401
from .fused_models import ma2_model  # noqa: F401
from .romc import (HipROMC, RomcProblems, hip_romc_class, hip_romc_posterior_class, romc_count, romc_objective,  # noqa: F401
                   romc_regions, romc_sample, romc_solve)



def HipAdaptiveDistance(*summaries, **kwargs):
    """elfi.AdaptiveDistance(*summaries, **kwargs) with the node's arithmetic on the GPU (elfi_amd/adaptive.py)."""
    return hip_adaptive_distance_class()(*summaries, **kwargs)


__version__ = "0.1.0"
