"""MI355X-native sampling path for lbarseghyan/diffusion-models.

The directory name carries a hyphen (it is the name the build contract asks
for); import it as ``diffusion_models_amd`` through the shim at the repo root.
"""
from .spec import (  # noqa: F401
    DecoderConfig,
    EncoderConfig,
    KarrasUnetConfig,
    Unet1DConfig,
    UnetConfig,
    autoencoder_kl_param_spec,
    ddim_time_pairs,
    decoder_param_spec,
    encoder_param_spec,
    karras_unet_param_spec,
    make_schedule,
    unet1d_param_spec,
    unet_param_spec,
)
from .synth import synth_state_dict, synth_tensor  # noqa: F401
from .unet import Unet  # noqa: F401
from .diffusion import (  # noqa: F401
    DenoisingDiffusion,
    ImageConditionalDenoisingDiffusion,
    ImageConditionalLatentDiffusion,
    LatentDiffusion,
    ModelPrediction,
    TextConditionalDenoisingDiffusion,
    TextConditionalLatentDiffusion,
)
from .elucidated import (ElucidatedDiffusion, edm_dpmpp_table, edm_heun_table, edm_sigmas,  # noqa: F401
                         edm_train_table)
from .continuous import (ContinuousTimeGaussianDiffusion, VParamContinuousTimeGaussianDiffusion,  # noqa: F401
                         MonotonicLinear, alpha_cosine_log_snr, beta_linear_log_snr, ct_dpmpp_nodes, ct_dpmpp_table, ct_step_table,
                         ct_train_table, learned_noise_schedule)
from .repaint import GaussianDiffusion as RePaintGaussianDiffusion, RepaintTable, repaint_step_table  # noqa: F401
from .learned import LearnedGaussianDiffusion, lv_step_table, lv_train_table  # noqa: F401
from .weighted import WeightedObjectiveGaussianDiffusion, wo_step_table, wo_train_table  # noqa: F401
from .seq1d import DenoisingDiffusion1D, Unet1D  # noqa: F401
from .karras import KarrasUnet  # noqa: F401
from .classifier_guidance import ClassifierGuidedGaussianDiffusion, cg_step_table  # noqa: F401
from .vae import (AutoencoderKL, DiagonalGaussianDistribution, KLEncoder, VQDecoder, VQEncoder, VQModel,  # noqa: F401
                  VQModelInterface)
from .bpd import bpd_step_table, bpd_times  # noqa: F401
from .dist import bpd_global, gather_shards, sample_global, sample_sharded, shard_bounds, shared_seed  # noqa: F401
from .checkpoint import load_trainer_checkpoint, load_vae_checkpoint  # noqa: F401
from .train import EMA, diffusion_state_dict, load_checkpoint, save_checkpoint, train_step  # noqa: F401
from .inception import FIDEvaluation, InceptionScoreEvaluation, InceptionV3, calculate_frechet_distance  # noqa: F401
from .inception_spec import inception_param_spec  # noqa: F401

__all__ = [
    "Unet",
    "DenoisingDiffusion",
    "TextConditionalDenoisingDiffusion",
    "ImageConditionalDenoisingDiffusion",
    "ImageConditionalLatentDiffusion",
    "LatentDiffusion",
    "TextConditionalLatentDiffusion",
    "ElucidatedDiffusion",
    "ContinuousTimeGaussianDiffusion",
    "VParamContinuousTimeGaussianDiffusion",
    "RePaintGaussianDiffusion",
    "LearnedGaussianDiffusion",
    "WeightedObjectiveGaussianDiffusion",
    "ClassifierGuidedGaussianDiffusion",
    "Unet1D",
    "DenoisingDiffusion1D",
    "Unet1DConfig",
    "unet1d_param_spec",
    "KarrasUnet",
    "KarrasUnetConfig",
    "karras_unet_param_spec",
    "VQDecoder",
    "VQEncoder",
    "VQModel",
    "VQModelInterface",
    "AutoencoderKL",
    "KLEncoder",
    "DiagonalGaussianDistribution",
    "InceptionV3",
    "FIDEvaluation",
    "InceptionScoreEvaluation",
    "sample_sharded",
    "sample_global",
    "bpd_global",
    "gather_shards",
    "shard_bounds",
    "UnetConfig",
    "DecoderConfig",
    "unet_param_spec",
    "decoder_param_spec",
    "EncoderConfig",
    "autoencoder_kl_param_spec",
    "make_schedule",
    "ddim_time_pairs",
    "edm_sigmas",
    "edm_heun_table",
    "edm_dpmpp_table",
    "edm_train_table",
    "beta_linear_log_snr",
    "alpha_cosine_log_snr",
    "ct_step_table",
    "ct_dpmpp_table",
    "ct_dpmpp_nodes",
    "ct_train_table",
    "learned_noise_schedule",
    "MonotonicLinear",
    "repaint_step_table",
    "RepaintTable",
    "lv_step_table",
    "lv_train_table",
    "bpd_step_table",
    "bpd_times",
    "wo_step_table",
    "wo_train_table",
    "synth_state_dict",
    "synth_tensor",
]
