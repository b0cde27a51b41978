"""HardNet / hardnetNAS / FDLNet inference and training on gfx950 HIP kernels.

The keypoint front end of FDLNet's inference is exported here; its names resolve on first use, so importing the
package imports neither torch nor the native library."""
_DETECTOR = ("RFDet", "InvertedResidual", "channel_shuffle", "detect", "detect_and_describe",
             "select_keypoints_torch")
__all__ = list(_DETECTOR)


def __getattr__(name):
    if name in _DETECTOR:
        from . import detector
        return getattr(detector, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
