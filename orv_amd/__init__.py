"""orv_amd - MI355X (gfx950) native implementation of ORV's diffusion denoising hot path.

Drop-in for ``orv.models.cogvideox_control`` / ``orv.models.components`` on that path only:

    from orv_amd.cogvideox_control import CogVideoXTransformer3DModelTraj, CogVideoXImageToVideoPipelineTraj
    from orv_amd.schedulers import CogVideoXDPMScheduler, CogVideoXDDIMScheduler

or, with no edit to ORV at all, ``import orv_amd; orv_amd.install()`` ahead of the reference's own import lines.

All arithmetic runs in hand-written HIP kernels (orv_amd/csrc -> liborv_mi355.so, C ABI in include/orv_mi355.h).
There is no CPU or eager-PyTorch fallback; importing works anywhere, running needs an MI355X and the built library.
"""
__version__ = "0.1.0"


def install(verbose: bool = False):
    """Alias ORV's import paths (``orv.models.cogvideox_control``, ``orv.models.components``, the two
    ``diffusers.schedulers.scheduling_*_cogvideox`` modules, ``orv.utils.prepare_rotary_positional_embeddings``) to this package
    in ``sys.modules`` so the reference's entry points run unchanged - see ``orv_amd/dropin.py``."""
    from .dropin import install as _install
    return _install(verbose=verbose)


def __getattr__(name):
    # the optimizer surface of the train scripts, resolved on first use (importing the package stays free of torch)
    if name in ("FusedProdigy", "FusedCAME", "get_optimizer", "named_groups"):
        from . import optim
        return getattr(optim, name)
    # the weight average to sample from (orv_amd/ema.py), resolved on first use likewise
    if name == "FusedEMA":
        from .ema import FusedEMA
        return FusedEMA
    # resumable training-state checkpoints (orv_amd/train_state.py), resolved on first use likewise
    if name in ("save_state", "load_state", "latest_checkpoint", "SaveHandle"):
        from . import train_state
        return getattr(train_state, name)
    # the scoring stage of the reference's workflow (orv_amd/metrics.py), resolved on first use likewise
    if name in ("frame_metrics", "psnr_ssim", "frechet_distance"):
        from . import metrics
        return getattr(metrics, name)
    # the point-cloud front of the reconstruction stage (orv_amd/pointcloud.py), resolved on first use likewise
    if name in ("remove_statistical_outlier", "estimate_normals", "orient_normals_towards_camera_location", "preprocess_points", "nksr_inputs"):
        from . import pointcloud
        return getattr(pointcloud, name)
    # cascaded long-video rollouts (orv_amd/rollout.py), resolved on first use likewise
    # (`rollout` is the callable module itself, the one object that name ever holds: see the end of orv_amd/rollout.py)
    if name in ("rollout", "plan_slices", "stitch_ranges"):
        from importlib import import_module
        module = import_module(".rollout", __name__)
        return module if name == "rollout" else getattr(module, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
