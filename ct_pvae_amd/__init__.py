"""ct_pvae_amd -- MI355X-native Radon forward/back-projector behind CT_PVAE's physics-decoder call signatures.

Host code is Python + PyTorch-ROCm (device memory, streams, autograd); the operators are hand-written gfx950 HIP
kernels reached through the C ABI of include/ctpvae_radon.h.  There is no CPU path.
"""
from .forward_functions import (RotatePlan, as_angle_index, num_proj_pix, pad_amounts, pad_phantom,  # noqa: F401
                                project_tf_fast, project_tf_low_mem, rotate_tables)
from .helper_functions import (calculate_log_prob_M_given_R, create_sinogram, create_sinograms,  # noqa: F401
                               gaussian_poisson_log_prob, poisson_log_prob, toy_dist)
from .create_masks import create_all_masks  # noqa: F401
from .fbp import iradon, iradon_all  # noqa: F401
from .recon import crop, evaluate_sinogram, recon, siddon_backproject  # noqa: F401
from .mcmc import HmcMarginals, hmc_marginals, hmc_sample, split_rhat  # noqa: F401
from .beta_head import beta_head, beta_head_words  # noqa: F401
from .beta_latents import beta_latent_words, beta_latents  # noqa: F401
from .output_head import head_uniforms, truncated_normal_head  # noqa: F401
from .latents import latent_draws, normal_latents  # noqa: F401
from .marginals import PixelMarginals, bin_samples, hist_distance  # noqa: F401
from .convblock import dropout, dropout_mask, dropout_pad, maxout, periodic_pad  # noqa: F401
from .conv import periodic_conv_maxout  # noqa: F401
from .conv_transpose import conv_transpose_maxout  # noqa: F401
from .merit import image_merits  # noqa: F401
from .update import FusedUpdate, adam_alpha  # noqa: F401

__version__ = "0.2.0"
