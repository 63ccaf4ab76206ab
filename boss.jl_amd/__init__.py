"""boss.jl_amd — MI355X-native GP-posterior + acquisition hot path for BOSS.jl.

Holds only what the path needs: csrc/ (HIP kernels + the C ABI of include/bosship.h), api.py
(ctypes twin of the Julia ccall layer) and the host-side mirror of BOSS's plugin interface
(model.py / fitter.py / maximizer.py).  The directory name contains a dot, so import it through
the repo-root shim:  `import boss_jl_amd`.
"""
from . import api  # noqa: F401
from .api import (BossError, Candidates, DomainError, GP, PosDefException, acq_ei, fit,  # noqa: F401
                  ggp_fit_batch, ggp_loglike_batch, load_library, loglike_batch, loglike_grad_batch_mean, ngp_fit_batch, ngp_loglike_batch,
                  ngp_acq_ei_grad_set, ngp_predict_grad_set, ngp_predict_set, NgpLatents, ngp_acq_ei_grad_set_lat,
                  ngp_predict_grad_set_lat, ngp_predict_set_lat, NgpWhitened)
from .problem import (BossOptions, BossProblem, Dirac, Domain, ExperimentData, ExpectedImprovement,  # noqa: F401,E402
                      LinFitness, LogNormal, MvDirac, MvLogNormal, NonlinFitness, Normal)
from .fitness import DeviceFitness  # noqa: F401,E402
from .api import FitnessProgram, acq_ei_mc, acq_ei_mc_grad, acq_ei_mc_grad_moments, acq_ei_mc_moments  # noqa: F401,E402
from .acq_program import (DeviceAcquisition, ProbabilityOfImprovement, UpperConfidenceBound, normcdf, normpdf,  # noqa: F401,E402
                          trace_acquisition)
from .api import AcqProgram, acq_prog, acq_prog_grad, acq_prog_grad_moments, acq_prog_moments  # noqa: F401,E402
from .mean import DeviceMean, trace_mean  # noqa: F401,E402
from .api import MeanProgram  # noqa: F401,E402
from .kernel import DeviceKernel, trace_kernel  # noqa: F401,E402
from .api import KernelGP, KernelProgram  # noqa: F401,E402
from .model import HipGaussianProcess, HipGPParams, average_mean  # noqa: F401,E402
from .api import WarpProgram  # noqa: F401,E402
from .transformed import (DeviceInputTransform, DeviceOutputTransform, DeviceSlicedOutputTransform,  # noqa: F401,E402
                          HipTransformedModel, HipTransformedPosterior, InputTransform, JointOutputTransform,
                          SlicedOutputTransform)
from .gradient_gp import (GradientData, HipGradientGaussianProcess, HipGradientGPParams,  # noqa: F401,E402
                          gradient_sequential_batch, join_gradient_slices)
from .nonstationary import HipNonstationaryGP, HipParametrizedGP, stack_latents  # noqa: F401,E402
from .nonstationary import (LatentActivation, constant_latent, exp_act, identity_act, latent_transform,  # noqa: F401,E402
                            softplus)
from .nonstationary import data_loglike_batch as nonstationary_data_loglike_batch  # noqa: F401,E402
from .nonstationary import data_loglike_grad_batch as nonstationary_data_loglike_grad_batch  # noqa: F401,E402
from .nonstationary import (nonstationary_acq_ei_batch, nonstationary_acq_ei_grad_batch,  # noqa: F401,E402
                            nonstationary_model_posterior_batch, nonstationary_sequential_batch)
from .fitter import HipBatchedMAP, HipGradientMAP, HipNonstationaryMAP, HipSampleOptMAP, MAPParams  # noqa: F401,E402
from .nonstationary import HipNonstationaryModel, HipNonstationaryParams  # noqa: F401,E402
from .maximizer import HipBatchAM, HipGradientAM, HipSequentialBatchAM  # noqa: F401,E402
