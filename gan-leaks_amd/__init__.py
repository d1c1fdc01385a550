"""gan-leaks_amd: MI355X-native implementation of the GAN-Leaks full-black-box (fbb) attack path.

Layout mirrors the part of the reference this replaces:
    attack_models/fbb.py, utils.py, eval_roc.py      drop-in entry points (same names/arguments)
    gan_models/dcgan/model_torch.py, wgangp/model.py generator classes (load_state_dict compatible)
    csrc/ + libganleaks_hip.so                       HIP kernels behind the C ABI (include/ganleaks.h)
    shard.py                                         bank sharding + RCCL min-reduce (one process per GPU)

Import as `import ganleaks_amd` (shim at the repository root; the directory name has a hyphen).
Importing the package does not load the HIP library; the first computation does and raises if the
library or the GPU is missing -- there is no CPU fallback.
"""
__version__ = "0.1.0"

from . import synth  # noqa: F401
from ._lib import Context, DeviceArray, GanLeaksError, build, device_count  # noqa: F401
from .attack import Bank, GeneratedBank, attack, ball_counts, distance_quantiles, eps_to_ssd, nearest_neighbours, pair_distance_quantiles, pair_distances, prepare_images  # noqa: F401
from .attack import ball_counts_rows, count_balls_rows, eps_to_ssd_rows, kth_distances, select_kth_rows  # noqa: F401
from .attack import count_balls_rows_f32, density_ratio_loss, density_ratio_loss_f32, eps_rows_to_bits, pair_ball_counts_rows, pair_kth_distances  # noqa: F401
from .attack import kde_coef, kde_loss, kde_scores, kde_sums  # noqa: F401
from .attack import kde_cut_bits_rows, kde_sums_f32, pair_kde_scores  # noqa: F401
from .pbb import pair_pbb_attack, pair_pbb_init_from_bank, pbb_attack, pbb_init_from_bank  # noqa: F401
from .wb import pair_grad_z, pair_wb_attack, wb_attack  # noqa: F401
from .recon import recon_attack, recon_latents  # noqa: F401
