"""HardNet / hardnetNAS / FDLNet inference and training on gfx950 HIP kernels.

The keypoint front end of FDLNet's inference and its ``Network`` (the homography ground-truth stage of the training
step) are exported here; the names resolve on first use, so importing the package imports neither torch nor the native
library."""
_DETECTOR = ("RFDet", "RFDetSO", "InvertedResidual", "channel_shuffle", "detect", "detect_and_describe",
             "select_keypoints_torch")
_NETWORK = ("Network", "warp", "gt_scale_orin", "ptCltoCr", "pair")
__all__ = list(_DETECTOR + _NETWORK)


def __getattr__(name):
    if name in _DETECTOR:
        from . import detector
        return getattr(detector, name)
    if name in _NETWORK:
        from . import network
        return getattr(network, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
