"""Table of C ABI calls that end in an argument check, for tests/test_abi_errors.py: at least one call per exported
function of hn_api_det.hip, hn_api_train.hip and hn_api_ops.hip, plus hn_param_count and the hn_forward family's
model-independent checks (hn_api.hip), each compared as (return code, hn_last_error()) with
tests/golden/abi_errors.json.  That file was recorded from the library as it was before the entry points were split
over those files:

    HN_LIB=<library built from that commit> python tests/abi_error_cases.py --record

so it pins every message, every code and, through the cases that break two rules at once (tags with "+"), the order
of the checks inside an entry point.  An entry point added since (hn_hardnet_train_layer_op and its size query) is
recorded from the library that adds it; the rows of the older ones must come out unchanged.

A case ends in HN_ERR_ARG (1), HN_ERR_WORKSPACE (4) or one of the documented early HN_OK returns (n == 0,
n_images == 0, hn_warp_score without outputs); none reaches a launch.  Device pointers are the placeholder 4096,
never dereferenced; 4096 + k where alignment is the subject.  SPEC gives every function's arguments in order with a
value that passes all its checks; a case overrides some of them, always with at least one that fails a check.

`fail(` sites no case reaches, and why:
  - hn_api_det.hip hn_det_create "hipMalloc of parameters failed", "hipMemcpy: ...", and every HIPCHK: they need a
    device; "host_params not fully consumed" there cannot happen once n_params is the state_dict's size;
  - hn_api_ops.hip hn_fpr95 "workspace too small" and hn_fpr95_workspace_bytes' success: the size comes from a
    hipCUB query (hn_fpr95_ws_bytes), which needs a device;
  - hn_det_destroy returns nothing and checks nothing;
  - hn_api.hip: hn_create past the blob's size, hn_workspace_bytes*, hn_set_profiling, hn_stage_times and the
    "workspace too small" of hn_forward, hn_forward_u8 and hn_forward_kp read an hn_model, which needs a device.
The checks of hn_forward, hn_forward_u8 and hn_forward_kp up to the pointers' alignment, and hn_det_forward's, are
covered with a placeholder model / detector: they all run before it is read.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from hardnetnas_amd import _native as N  # noqa: E402
from hardnetnas_amd import arch as A  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_errors.json")
P = 4096       # a device pointer that is never dereferenced
BIG = 1 << 40  # a workspace size that always suffices
NAN, INF = float("nan"), float("inf")


def size():
    return ctypes.byref(ctypes.c_size_t())


def table(n, hole=None):
    a = (ctypes.c_void_p * n)(*[P] * n)
    if hole is not None:
        a[hole] = None
    return a


def desc(base="wang2", **mods):
    """byref of a descriptor (wang2, "fdl", "supernet" or "hardnet") with fields (kind=7) or elements (op={2: 99}) set"""
    d = {"fdl": N.fdl_desc, "supernet": N.supernet_desc, "hardnet": N.hardnet_desc}.get(
        base, lambda: N.nas_desc(A.MODEL_ARCH["wang2"]))()
    for k, v in mods.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return ctypes.byref(d)


def n_tensors(base):
    n = ctypes.c_size_t()
    assert N.load_library().hn_nas_train_tensor_count(desc(base), ctypes.byref(n)) == 0
    return n.value


def det_params(**at):
    """A zero RFDet state_dict blob (host memory, kept alive by the caller) with some floats set."""
    n = ctypes.c_size_t()
    assert N.load_library().hn_det_param_count(ctypes.byref(n)) == 0
    a = np.zeros(n.value, np.float32)
    for i, v in at.items():
        a[int(i)] = v
    return a


def nas_tensors(base="wang2", hole=None):
    return lambda: table(n_tensors(base), hole)


T40 = lambda: table(N.DET_TRAIN_TENSORS)  # noqa: E731
T7 = lambda: table(7)  # noqa: E731
DESC = lambda: desc()  # noqa: E731
_KEEP = []  # host arrays that a call reads


def host(a):
    _KEEP.append(a)
    return a.ctypes.data


# every function's arguments in call order, with a value that passes all its checks (callables are made per call)
_IMG = [("n_images", 2), ("height", 8), ("width", 8)]
_WS = [("ws", P), ("ws_bytes", BIG)]
_SV = [("saved", P), ("saved_bytes", BIG), ("scratch", P), ("scratch_bytes", BIG)]
_KP = [("kpts", P), ("scale", P), ("ori", P), ("ratio", P), ("n", 4)]
SPEC = {
    "hn_param_count": [("desc", DESC), ("n_out", size)],
    "hn_forward": [("model", P), ("in", P), ("batch", 4), ("out", P)] + _WS + [("st", None)],
    "hn_forward_u8": [("model", P), ("in", P), ("batch", 4), ("in_hw", 64), ("resize", 1), ("normalize", 1),
                      ("mean", 0.5), ("std", 0.2), ("out", P)] + _WS + [("st", None)],
    "hn_forward_kp": [("model", P), ("images", P)] + _IMG + _KP + [("out", P)] + _WS + [("st", None)],
    # hn_api_train.hip
    "hn_hardnet_train_workspace_bytes": [("batch", 4), ("saved_out", size), ("scratch_out", size)],
    "hn_hardnet_train_forward": [("in", P), ("batch", 4), ("weights", T7), ("rmean", None), ("rvar", None),
                                 ("momentum", 0.1), ("dropout_p", 0.1), ("seed", 1), ("out", P)] + _SV + [("st", None)],
    "hn_hardnet_train_backward": [("dout", P), ("batch", 4), ("weights", T7), ("dweights", T7), ("din", P),
                                  ("dropout_p", 0.1), ("seed", 1)] + _SV + [("st", None)],
    "hn_hardnet_train_layer_op_workspace_bytes": [("bits", 17), ("row_segments", 0), ("batch", 4), ("out", size)],
    # conv_dgrad of layer 4 under bits 32 + 17: the column-GEMM form, so dgrad_chunk may be given
    "hn_hardnet_train_layer_op": [("op", 7), ("layer", 4), ("bits", 49), ("row_segments", 0), ("dgrad_chunk", 2),
                                  ("batch", 4), ("x", P), ("w", P), ("y", P), ("aux0", None), ("aux1", None),
                                  ("aux2", None), ("momentum", 0.1), ("dropout_p", 0.1), ("seed", 1), ("scratch", P),
                                  ("scratch_bytes", BIG), ("st", None)],
    "hn_nas_train_tensor_count": [("desc", DESC), ("n_out", size)],
    "hn_nas_train_workspace_bytes": [("desc", DESC), ("batch", 4), ("saved_out", size), ("scratch_out", size)],
    "hn_nas_train_forward": [("desc", DESC), ("in", P), ("batch", 4), ("tensors", nas_tensors()), ("momentum", 0.1),
                             ("soft", None), ("out", P)] + _SV + [("st", None)],
    "hn_nas_train_backward": [("desc", DESC), ("dout", P), ("in", P), ("batch", 4), ("tensors", nas_tensors()),
                              ("soft", None), ("grads", nas_tensors()), ("dsoft", None)] + _SV + [("st", None)],
    "hn_nas_train_backward_dx": [("desc", DESC), ("dout", P), ("in", P), ("batch", 4), ("tensors", nas_tensors()),
                                 ("soft", None), ("grads", nas_tensors()), ("dsoft", None), ("din", P)] + _SV +
                                [("st", None)],
    "hn_hardnet_loss_train_workspace_bytes": [("batch", 4), ("out", size)],
    "hn_hardnet_loss_train_forward": [("a", P), ("p", P), ("batch", 4), ("dim", 128), ("swap", 0), ("margin", 1.0),
                                      ("loss_type", 0), ("loss", P), ("saved", P), ("saved_bytes", BIG), ("st", None)],
    "hn_hardnet_loss_backward": [("a", P), ("p", P), ("batch", 4), ("dim", 128), ("swap", 0), ("margin", 1.0),
                                 ("loss_type", 0), ("dloss", P), ("ga", P), ("gp", P), ("saved", P),
                                 ("saved_bytes", BIG), ("st", None)],
    "hn_neimask_loss_workspace_bytes": [("batch", 4), ("out", size)],
    "hn_neimask_loss_forward": [("a", P), ("p", P), ("akp", P), ("pkp", P), ("batch", 4), ("dim", 128), ("margin", 1.0),
                                ("coo", 5.0), ("loss", P), ("pos", P), ("min_neg", P), ("saved", P),
                                ("saved_bytes", BIG), ("st", None)],
    "hn_neimask_loss_backward": [("a", P), ("p", P), ("batch", 4), ("dim", 128), ("margin", 1.0), ("dloss", P),
                                 ("ga", P), ("gp", P), ("saved", P), ("saved_bytes", BIG), ("st", None)],
    # hn_api_ops.hip
    "hn_clip_patch": [("images", P)] + _IMG + _KP + [("patches", P), ("st", None)],
    "hn_clip_patch_backward": [("dpatches", P), ("images", P)] + _IMG + _KP + [("dscale", P), ("dori", P),
        ("st", None)],
    "hn_pairdist_workspace_bytes": [("batch", 4), ("out", size)],
    "hn_pairdist_hardneg": [("a", P), ("p", P), ("batch", 4), ("dim", 128), ("swap", 0), ("pos", P), ("min_neg", P)] +
                           _WS + [("st", None)],
    "hn_pairdist_rows_workspace_bytes": [("n_rows", 2), ("batch", 4), ("out", size)],
    "hn_pairdist_rows": [("a_rows", P), ("n_rows", 2), ("row0", 0), ("p", P), ("batch", 4), ("dim", 128), ("pos", P),
                         ("row_min", P), ("col_min", P)] + _WS + [("st", None)],
    "hn_match_workspace_bytes": [("n_query", 4), ("n_db", 4), ("out", size)],
    "hn_match_nn2": [("query", P), ("n_query", 4), ("db", P), ("n_db", 4), ("dim", 128), ("metric", 0), ("dist", P),
                     ("idx", P)] + _WS + [("st", None)],
    "hn_hardnet_loss": [("pos", P), ("row_min", P), ("col_min", P), ("n", 4), ("margin", 1.0), ("loss_type", 0),
                        ("scale", 1.0), ("min_neg", P), ("loss", P), ("st", None)],
    "hn_fpr95_workspace_bytes": [("n", 4), ("out", size)],
    "hn_fpr95": [("a", P), ("p", P), ("labels", P), ("n", 4), ("dim", 128), ("dists", P), ("fpr", P)] + _WS +
                [("st", None)],
    "hn_preprocess": [("in", P), ("n", 4), ("in_hw", 64), ("resize", 1), ("normalize", 1), ("mean", 0.5), ("std", 0.2),
                      ("out", P), ("st", None)],
    # hn_api_det.hip
    "hn_det_param_count": [("n_out", size)],
    "hn_det_create": [("params", lambda: host(det_params())), ("n_params", lambda: det_params().size),
                      ("bn_eps", 1e-5), ("in_eps", 1e-5), ("out", lambda: ctypes.byref(ctypes.c_void_p()))],
    "hn_det_workspace_bytes": _IMG + [("out", size)],
    "hn_det_forward": [("det", P), ("images", P)] + _IMG + [("score", P), ("ori", P)] + _WS + [("st", None)],
    "hn_det_train_workspace_bytes": _IMG + [("saved_out", size), ("scratch_out", size)],
    "hn_det_train_forward": [("images", P)] + _IMG + [("tensors", T40), ("bn_eps", 1e-5), ("in_eps", 1e-5),
                                                      ("momentum", 0.1), ("score", P),
                                                          ("ori", P)] + _SV + [("st", None)],
    "hn_det_train_backward": [("dscore", P), ("dori", P), ("images", P)] + _IMG + [("tensors", T40), ("grads", T40)] +
                             _SV + [("st", None)],
    "hn_select_workspace_bytes": _IMG + [("topk", 16), ("out", size)],
    "hn_select_keypoints": [("score", P)] + _IMG + [("border", 1), ("nms_thresh", 0.0), ("nms_ksize", 5), ("topk", 16),
                                                    ("gauss_ksize", 5), ("gauss_sigma", 0.5), ("scale_map", P),
                                                    ("scale_value", 32.0), ("ori_map", P), ("kpts", P), ("kscore", P),
                                                    ("kscale", P), ("kori", P), ("score_proc", P), ("topk_mask", P)] +
                           _WS + [("st", None)],
    "hn_warp_score": [("score", P), ("homo", P)] + _IMG + [("border", 1), ("align_corners", 0), ("warped", P),
                                                           ("visible", P), ("st", None)],
    "hn_gt_scale_orin": [("scale", P), ("scale_value", 32.0), ("ori", P), ("homo12", P), ("homo21", P)] + _IMG +
                        [("gt_scale", P), ("gt_ori", P), ("st", None)],
    "hn_mask_keypoints": [("mask", P)] + _IMG + [("topk", 16), ("scale_map", P), ("scale_value", 32.0), ("ori_map", P),
                                                 ("kpts", P), ("kscale", P), ("kori", P), ("counts", P), ("st", None)],
    "hn_project_keypoints": [("kpts", P), ("n", 4), ("homo", P)] + _IMG + [("scale_map", P), ("scale_value", 32.0),
                                                                          ("ori_map", P), ("clamp", 1), ("kpts_r", P),
                                                                          ("scale_r", P), ("ori_r", P), ("st", None)],
}

HW31 = {"height": 1 << 16, "width": 1 << 16}  # height * width = 2^32
_GT_SHAPES = [("n_images<0", {"n_images": -1}), ("height<2", {"height": 1}), ("hw>=2^31", HW31),
              ("nhw>=2^62", {"n_images": 1 << 58}), ("n_images<0+height<2", {"n_images": -1, "height": 1})]
_CLIP_SHAPES = [("n<0", {"n": -1}), ("n_images<0", {"n_images": -1}), ("width<2", {"width": 1}),
                ("nhw>=2^63", {"n_images": 1 << 58}), ("no images", {"n_images": 0}),
                ("n<0+height<2", {"n": -1, "height": 1}), ("n==0", {"n": 0, "images": None})]
_DET_TRAIN_SHAPES = [("n_images<1", {"n_images": 0}), ("height<1", {"height": 0}), ("hw>=2^31", HW31),
                     ("n_images>2^24", {"n_images": (1 << 24) + 1}),
                     ("one pixel", {"n_images": 1, "height": 1, "width": 1}),
                     ("n_images<1+width<1", {"n_images": 0, "width": 0})]
_SELECT_SHAPES = [("n_images<0", {"n_images": -1}), ("width<1", {"width": 0}), ("hw>=2^31", HW31),
                  ("n_images>=2^31", {"n_images": 1 << 31}), ("topk<1", {"topk": 0}), ("topk>hw", {"topk": 65}),
                  ("hw>=2^31+topk<1", dict(HW31, topk=0))]
_TRAIN_WS = [("saved NULL", {"saved": None}), ("saved small", {"saved_bytes": 0}),
    ("scratch small", {"scratch_bytes": 0}),
             ("saved small+scratch small", {"saved_bytes": 0, "scratch_bytes": 0})]
_LOSS_ARGS = [("a NULL", {"a": None}), ("batch<1", {"batch": 0}), ("batch>2^22", {"batch": (1 << 22) + 1}),
              ("dim", {"dim": 64}), ("p misaligned", {"p": P + 8}), ("saved small", {"saved_bytes": 0}),
              ("saved NULL+batch<1", {"saved": None, "batch": 0}), ("batch<1+dim", {"batch": 0, "dim": 64}),
              ("a misaligned+saved small", {"a": P + 4, "saved_bytes": 0})]


def _cases():
    c = []

    def add(fn, rows):
        c.extend((fn, tag, kw) for tag, kw in rows)

    add("hn_param_count", [
        ("desc NULL", {"desc": None}), ("kind", {"desc": desc(kind=7)}), ("n_layers<1", {"desc": desc(n_layers=0)}),
        ("n_layers>8", {"desc": desc(n_layers=9)}), ("op", {"desc": desc(op={2: 99})}),
        ("chain", {"desc": desc(c_in={3: 48})}), ("stride", {"desc": desc(stride={1: 3})}),
        ("c_out%4", {"desc": desc(c_out={5: 130})}), ("c_out>256", {"desc": desc(c_out={5: 260})}),
        ("final map", {"desc": desc(stride={1: 2})}), ("fdl head", {"desc": desc("fdl", c_out={2: 64})}),
        ("fdl chain", {"desc": desc("fdl", c_in={0: 32})}), ("n_out NULL", {"n_out": None}),
        ("kind+n_out NULL", {"desc": desc(kind=7), "n_out": None}),
            ("op+stride", {"desc": desc(op={0: -1}, stride={0: 3})}),
    ])
    # a placeholder model: the checks below all run before the model is read
    add("hn_forward", [("model NULL", {"model": None}), ("batch<0", {"batch": -1}),
        ("batch==0", {"batch": 0, "in": None}),
                       ("ws NULL", {"ws": None}), ("out misaligned", {"out": P + 8}),
                       ("model NULL+batch<0", {"model": None, "batch": -1}),
                           ("in NULL+out misaligned", {"in": None, "out": P + 8})])
    add("hn_forward_u8", [("model NULL", {"model": None}), ("batch<0", {"batch": -1}), ("resize", {"resize": 3}),
                          ("in_hw", {"in_hw": 32}), ("in_hw none", {"resize": 0, "in_hw": 64}), ("std", {"std": 0.0}),
                          ("batch==0", {"batch": 0, "in": None}), ("out NULL", {"out": None}),
                              ("in misaligned", {"in": P + 4}),
                          ("batch<0+resize", {"batch": -1, "resize": 3}), ("resize+in_hw", {"resize": -1, "in_hw": 5}),
                          ("in_hw+std", {"in_hw": 32, "std": 0.0}), ("std+batch==0", {"std": 0.0, "batch": 0}),
                          ("std unused+ws NULL", {"std": 0.0, "normalize": 0, "ws": None}),
                          ("out NULL+ws misaligned", {"out": None, "ws": P + 8})])
    add("hn_forward_kp", _CLIP_SHAPES[:-1] + [("model NULL", {"model": None}),
        ("width<2+model NULL", {"width": 1, "model": None}),
                                              ("n==0", {"n": 0, "images": None}),
                                                  ("model NULL+n==0", {"model": None, "n": 0}),
                                              ("ratio NULL", {"ratio": None}),
                                                  ("ori NULL+out misaligned", {"ori": None, "out": P + 8}),
                                              ("ws NULL+out misaligned", {"ws": None, "out": P + 8})])
    add("hn_hardnet_train_workspace_bytes", [("batch<2", {"batch": 1}), ("batch>2^24", {"batch": (1 << 24) + 1}),
                                             ("saved_out NULL", {"saved_out": None})])
    add("hn_hardnet_train_forward", [("batch<2", {"batch": 1})] + _TRAIN_WS + [
        ("weights NULL", {"weights": None}), ("weights hole", {"weights": table(7, 3)}), ("in NULL", {"in": None}),
        ("rvar alone", {"rvar": table(7)}), ("dropout_p", {"dropout_p": 1.0}), ("dropout_p NaN", {"dropout_p": NAN}),
        ("scratch small+weights NULL", {"scratch_bytes": 0, "weights": None}),
        ("out NULL+dropout_p", {"out": None, "dropout_p": 1.0}),
            ("rmean alone+dropout_p", {"rmean": table(7), "dropout_p": -1.0}),
    ])
    add("hn_hardnet_train_backward", [("batch<2", {"batch": 1})] + _TRAIN_WS + [
        ("weights hole", {"weights": table(7, 6)}), ("dout NULL", {"dout": None}),
            ("dweights NULL", {"dweights": None}),
        ("dweights hole", {"dweights": table(7, 2)}), ("dropout_p", {"dropout_p": -0.1}),
        ("dout NULL+dweights NULL", {"dout": None, "dweights": None}),
    ])
    add("hn_hardnet_train_layer_op_workspace_bytes", [
        ("out NULL", {"out": None}), ("batch<2", {"batch": 1}), ("batch>2^24", {"batch": (1 << 24) + 1}),
        ("bits", {"bits": 256}), ("bits<-1", {"bits": -2}), ("row_segments", {"row_segments": 3}),
        ("out NULL+batch<2", {"out": None, "batch": 1}), ("batch<2+bits", {"batch": 1, "bits": 256}),
        ("bits+row_segments", {"bits": 256, "row_segments": 8})])
    ring = {"bits": 17, "dgrad_chunk": 0}  # the same operation as k_dgrad2: row segments, no chunks
    bn_fwd = {"op": 2, "dgrad_chunk": 0, "x": None, "w": None, "aux0": P}
    add("hn_hardnet_train_layer_op", [
        ("batch<2", {"batch": 1}), ("bits", {"bits": 256}), ("row_segments", {"row_segments": 3}),
        ("op", {"op": 9}), ("op<0", {"op": -1}), ("layer", {"layer": 7}), ("layer<0", {"layer": -1}),
        ("row_segments without a ring", {"row_segments": 2}),
        ("row_segments on bn_fwd", dict(bn_fwd, row_segments=4)),
        ("dgrad_chunk<0", {"dgrad_chunk": -1}), ("dgrad_chunk>batch", {"dgrad_chunk": 5}),
        ("dgrad_chunk on a ring", dict(ring, dgrad_chunk=2)),
        ("dgrad_chunk on conv_fwd", {"op": 1}),
        ("x NULL", {"x": None}), ("w NULL", {"w": None}), ("y NULL", {"y": None}),
        ("bn_fwd aux0 NULL", dict(bn_fwd, aux0=None)),
        ("bn_fwd rvar alone", dict(bn_fwd, aux2=P)),
        ("dropout_p", {"dropout_p": 1.0}), ("dropout_p NaN", {"dropout_p": NAN}),
        ("y misaligned", {"y": P + 8}), ("scratch misaligned", {"scratch": P + 4}),
        ("scratch NULL", {"scratch": None}), ("scratch small", {"scratch_bytes": 0}),
        ("batch<2+op", {"batch": 1, "op": 9}), ("row_segments+op", {"row_segments": 3, "op": 9}),
        ("op+layer", {"op": 9, "layer": 7}), ("layer+row_segments without a ring", {"layer": 7, "row_segments": 2}),
        ("row_segments without a ring+dgrad_chunk<0", {"row_segments": 2, "dgrad_chunk": -1}),
        ("dgrad_chunk on a ring+x NULL", dict(ring, dgrad_chunk=2, x=None)),
        ("x NULL+dropout_p", {"x": None, "dropout_p": 1.0}),
        ("bn_fwd rmean alone+dropout_p", dict(bn_fwd, aux1=P, dropout_p=-1.0)),
        ("dropout_p+w misaligned", {"dropout_p": 1.0, "w": P + 4}),
        ("x misaligned+scratch NULL", {"x": P + 8, "scratch": None}),
        ("scratch NULL+scratch small", {"scratch": None, "scratch_bytes": 0}),
    ])
    nas_desc_rows = [
        ("desc NULL", {"desc": None}), ("kind", {"desc": desc("hardnet")}), ("n_layers", {"desc": desc(n_layers=0)}),
        ("fdl input_norm", {"desc": desc("fdl", input_norm_eps=-1.0)}), ("op", {"desc": desc(op={1: 17})}),
        ("chain", {"desc": desc(c_in={3: 48})}), ("stride", {"desc": desc(stride={2: 4})}),
        ("c_out>128", {"desc": desc(c_out={5: 132})}), ("final map", {"desc": desc(stride={1: 2})}),
        ("n_layers+op", {"desc": desc(n_layers=0, op={0: 17})}),
    ]
    add("hn_nas_train_tensor_count", nas_desc_rows + [("n_out NULL", {"n_out": None}),
                                                      ("op+n_out NULL", {"desc": desc(op={1: 17}), "n_out": None})])
    add("hn_nas_train_workspace_bytes", nas_desc_rows[:2] + [
        ("batch<2", {"batch": 1}), ("batch>2^22", {"batch": (1 << 22) + 1}),
            ("scratch_out NULL", {"scratch_out": None}),
        ("kind+batch<2", {"desc": desc("hardnet"), "batch": 1})])
    sn = {"desc": desc("supernet"), "tensors": nas_tensors("supernet")()}
    sn_bwd = dict(sn, grads=nas_tensors("supernet")())
    add("hn_nas_train_forward", [("desc NULL", {"desc": None}), ("batch<2", {"batch": 1})] + _TRAIN_WS + [
        ("tensors NULL", {"tensors": None}), ("tensors hole", {"tensors": nas_tensors(hole=5)()}),
        ("supernet soft", dict(sn, soft=None)), ("in NULL", {"in": None}), ("out NULL", dict(sn, soft=P, out=None)),
        ("tensors NULL+in NULL", {"tensors": None, "in": None}), ("batch<2+saved NULL", {"batch": 1, "saved": None}),
    ])
    add("hn_nas_train_backward", [("grads NULL", {"grads": None}), ("saved small", {"saved_bytes": 0})])
    add("hn_nas_train_backward_dx", [("batch<2", {"batch": 1})] + _TRAIN_WS + [
        ("tensors hole", {"tensors": nas_tensors(hole=0)()}), ("dout NULL", {"dout": None}),
            ("grads NULL", {"grads": None}),
        ("grads hole", {"grads": nas_tensors(hole=0)()}), ("supernet soft", dict(sn_bwd, soft=None)),
        ("supernet dsoft", dict(sn_bwd, soft=P, dsoft=None)), ("din misaligned", {"din": P + 8}),
        ("in NULL+grads NULL", {"in": None, "grads": None}),
            ("grads hole+din misaligned", {"grads": nas_tensors(hole=0)(), "din": P + 8}),
    ])
    for fn in ("hn_hardnet_loss_train_workspace_bytes", "hn_neimask_loss_workspace_bytes"):
        add(fn, [("out NULL", {"out": None}), ("batch<1", {"batch": 0}), ("batch>2^22", {"batch": (1 << 22) + 1})])
    add("hn_hardnet_loss_train_forward", _LOSS_ARGS + [("loss_type", {"loss_type": 3}), ("loss NULL", {"loss": None}),
                                                       ("dim+loss_type", {"dim": 64, "loss_type": -1}),
                                                       ("saved small+loss NULL", {"saved_bytes": 0, "loss": None})])
    add("hn_hardnet_loss_backward", _LOSS_ARGS + [("loss_type", {"loss_type": 3}), ("dloss NULL", {"dloss": None}),
                                                  ("ga misaligned", {"ga": P + 4}),
                                                  ("gp NULL+ga misaligned", {"gp": None, "ga": P + 4})])
    add("hn_neimask_loss_forward", _LOSS_ARGS + [
        ("akp NULL", {"akp": None}), ("loss NULL", {"loss": None}), ("pkp misaligned", {"pkp": P + 4}),
        ("pos misaligned", {"pos": P + 2}), ("min_neg NULL", {"min_neg": None, "pos": None, "loss": P + 1}),
        ("akp misaligned+loss misaligned", {"akp": P + 4, "loss": P + 2})])
    add("hn_neimask_loss_backward", _LOSS_ARGS + [("dloss NULL", {"dloss": None}), ("gp misaligned", {"gp": P + 4}),
                                                  ("ga NULL+gp misaligned", {"ga": None, "gp": P + 4})])

    add("hn_clip_patch", _CLIP_SHAPES + [("kpts NULL", {"kpts": None}),
        ("ori NULL+patches NULL", {"ori": None, "patches": None}),
                                         ("patches misaligned", {"patches": P + 8}),
                                         ("scale NULL+patches misaligned", {"scale": None, "patches": P + 8})])
    add("hn_clip_patch_backward", _CLIP_SHAPES + [
        ("dori without ori", {"ori": None}), ("dori without ori+n==0", {"ori": None, "n": 0}),
        ("n<0+dori without ori", {"n": -1, "ori": None}), ("dpatches NULL", {"dpatches": None}),
        ("dpatches misaligned", {"dpatches": P + 4, "dscale": None}),
        ("ratio NULL+dpatches misaligned", {"ratio": None, "dpatches": P + 4})])
    add("hn_pairdist_workspace_bytes", [("out NULL", {"out": None}), ("batch<0", {"batch": -1})])
    add("hn_pairdist_hardneg", [("pos NULL", {"pos": None}), ("batch<2", {"batch": 1}),
        ("batch>2^30", {"batch": (1 << 30) + 1}),
                                ("dim", {"dim": 64}), ("ws small", {"ws_bytes": 0}),
                                    ("ws NULL+batch<2", {"ws": None, "batch": 1}),
                                ("batch<2+dim", {"batch": 1, "dim": 64}), ("dim+ws small", {"dim": 64, "ws_bytes": 0})])
    add("hn_pairdist_rows_workspace_bytes", [("out NULL", {"out": None}), ("n_rows<1", {"n_rows": 0}),
        ("batch<2", {"batch": 1, "n_rows": 1}),
                                             ("n_rows>batch", {"n_rows": 5})])
    add("hn_pairdist_rows", [("row_min NULL", {"row_min": None}), ("col_min NULL+dim", {"col_min": None, "dim": 64}),
                             ("n_rows<1", {"n_rows": 0}), ("row0<0", {"row0": -1}), ("rows outside", {"row0": 3}),
                             ("ws small", {"ws_bytes": 0}), ("a_rows misaligned", {"a_rows": P + 8}),
                             ("pos NULL+dim", {"pos": None, "dim": 64}), ("dim+n_rows<1", {"dim": 64, "n_rows": 0}),
                             ("n_rows>batch+row0<0", {"n_rows": 5, "row0": -1}),
                                 ("rows outside+ws small", {"row0": 3, "ws_bytes": 0}),
                             ("ws small+p misaligned", {"ws_bytes": 0, "p": P + 8})])
    add("hn_match_workspace_bytes", [("out NULL", {"out": None}), ("n_query<1", {"n_query": 0}),
        ("n_db>2^22", {"n_db": (1 << 22) + 1}),
                                     ("out NULL+n_query<1", {"out": None, "n_query": 0})])
    add("hn_match_nn2", [("dim", {"dim": 64}), ("metric", {"metric": 5}), ("n_query>2^22", {"n_query": (1 << 22) + 1}),
                         ("n_db<1", {"n_db": 0}), ("ws small", {"ws_bytes": 0}), ("idx NULL", {"idx": None}),
                         ("db misaligned", {"db": P + 8}), ("idx misaligned", {"idx": P + 4}),
                         ("dim+metric", {"dim": 64, "metric": 5}), ("metric+n_db<1", {"metric": 5, "n_db": 0}),
                         ("ws small+query NULL", {"ws_bytes": 0, "query": None}),
                             ("dist NULL+ws misaligned", {"dist": None, "ws": P + 8}),
                         ("query misaligned+dist misaligned", {"query": P + 8, "dist": P + 4})])
    add("hn_hardnet_loss", [("loss NULL", {"loss": None}),
        ("optional NULL+n<1", {"col_min": None, "min_neg": None, "n": 0}),
                            ("n>2^30", {"n": (1 << 30) + 1}), ("loss_type", {"loss_type": 3}),
                            ("pos NULL+n<1", {"pos": None, "n": 0}), ("n<1+loss_type", {"n": 0, "loss_type": -1})])
    add("hn_fpr95_workspace_bytes", [("out NULL", {"out": None}), ("n<1", {"n": 0}), ("n>2^30", {"n": (1 << 30) + 1})])
    add("hn_fpr95", [("labels NULL", {"labels": None}), ("dists NULL+n<1", {"dists": None, "n": 0}),
        ("dim<1", {"dim": 0}),
                     ("fpr NULL+dim<1", {"fpr": None, "dim": 0})])
    add("hn_preprocess", [("n<0", {"n": -1}), ("resize", {"resize": 7}), ("in_hw", {"in_hw": 32}),
                          ("in_hw none", {"resize": 0, "in_hw": 64}), ("n==0", {"n": 0, "in": None, "std": 0.0}),
                          ("out NULL", {"out": None}), ("in misaligned", {"in": P + 4}), ("std", {"std": 0.0}),
                          ("std unused+out NULL", {"std": 0.0, "normalize": 0, "out": None}),
                          ("n<0+resize", {"n": -1, "resize": 7}), ("resize+in_hw", {"resize": -1, "in_hw": 5}),
                          ("out misaligned+std", {"out": P + 8, "std": 0.0})])

    add("hn_det_param_count", [("n_out NULL", {"n_out": None})])
    rv = 160 + 64 + 24  # first running_var of the first block's first BatchNorm
    add("hn_det_create", [("out NULL", {"out": None}), ("params NULL", {"params": None}),
        ("n_params", {"n_params": 10}),
                          ("bn_eps", {"bn_eps": 0.0}), ("in_eps NaN", {"in_eps": NAN}),
                          ("non-finite", {"params": host(det_params(**{"7": INF}))}),
                          ("running_var", {"params": host(det_params(**{str(rv): -1.0}))}),
                          ("n_params+bn_eps", {"n_params": 10, "bn_eps": 0.0}),
                          ("bn_eps+non-finite", {"bn_eps": -1.0, "params": host(det_params(**{"7": NAN}))})])
    det_shapes = [("n_images<0", {"n_images": -1}), ("height<1", {"height": 0}),
        ("one pixel", {"height": 1, "width": 1}),
                  ("hw>=2^31", HW31), ("n_images>=2^31", {"n_images": 1 << 31}),
                  ("tiles>=2^31", {"n_images": 1 << 30, "height": 64, "width": 64}),
                  ("n_images<0+one pixel", {"n_images": -1, "height": 1, "width": 1})]
    add("hn_det_workspace_bytes", [("out NULL", {"out": None}),
        ("out NULL+height<1", {"out": None, "height": 0})] + det_shapes)
    add("hn_det_forward", det_shapes + [("det NULL", {"det": None}), ("height<1+det NULL", {"height": 0, "det": None}),
                                        ("n_images==0", {"n_images": 0, "images": None}),
                                            ("score NULL", {"score": None}),
                                        ("ori misaligned", {"ori": P + 4}), ("ws misaligned", {"ws": P + 8}),
                                        ("ws small", {"ws_bytes": 0}),
                                            ("ws NULL+ori misaligned", {"ws": None, "ori": P + 4}),
                                        ("ws misaligned+ws small", {"ws": P + 8, "ws_bytes": 0})])
    add("hn_det_train_workspace_bytes", [("saved_out NULL", {"saved_out": None}),
                                         ("scratch_out NULL+n_images<1", {"scratch_out": None, "n_images": 0})] + _DET_TRAIN_SHAPES)
    det_train = _DET_TRAIN_SHAPES + _TRAIN_WS[1:] + [
        ("images NULL", {"images": None}), ("saved misaligned", {"saved": P + 8}), ("tensors NULL", {"tensors": None}),
        ("tensors hole", {"tensors": table(40, 17)}),
            ("scratch NULL+saved misaligned", {"scratch": None, "saved": P + 8}),
        ("images misaligned+saved small", {"images": P + 4, "saved_bytes": 0}),
        ("scratch small+tensors NULL", {"scratch_bytes": 0, "tensors": None})]
    add("hn_det_train_forward", det_train + [
        ("bn_eps", {"bn_eps": 0.0}), ("momentum", {"momentum": 1.5}), ("momentum NaN", {"momentum": NAN}),
        ("score NULL", {"score": None}), ("ori misaligned", {"ori": P + 8}),
        ("tensors hole+in_eps", {"tensors": table(40, 0), "in_eps": -1.0}),
            ("in_eps+momentum", {"in_eps": 0.0, "momentum": -0.1}),
        ("momentum+ori NULL", {"momentum": 2.0, "ori": None}),
            ("ori NULL+score misaligned", {"ori": None, "score": P + 8})])
    add("hn_det_train_backward", det_train + [
        ("dori misaligned", {"dori": P + 4}), ("grads NULL", {"grads": None}), ("grads hole", {"grads": table(40, 2)}),
        ("grads statistics hole+n_images<1", {"grads": table(40, 5), "n_images": 0}),
        ("tensors hole+dscore misaligned", {"tensors": table(40, 39), "dscore": P + 8}),
        ("dscore misaligned+grads NULL", {"dscore": P + 8, "grads": None})])
    add("hn_select_workspace_bytes", [("out NULL", {"out": None}),
        ("out NULL+topk<1", {"out": None, "topk": 0})] + _SELECT_SHAPES)
    add("hn_select_keypoints", _SELECT_SHAPES + [
        ("border<0", {"border": -1}), ("border", {"border": 4}), ("nms_ksize even", {"nms_ksize": 4}),
        ("nms_ksize>15", {"nms_ksize": 17}), ("gauss_ksize<1", {"gauss_ksize": 0}),
            ("gauss_sigma<0", {"gauss_sigma": -1.0}),
        ("gauss_sigma inf", {"gauss_sigma": INF}), ("nms_thresh NaN", {"nms_thresh": NAN}),
            ("kori alone", {"ori_map": None}),
        ("ori_map alone", {"kori": None}), ("n_images==0", {"n_images": 0, "score": None}),
            ("kscore NULL", {"kscore": None}),
        ("optional NULL+ws NULL", {"scale_map": None, "ori_map": None, "kori": None, "score_proc": None, "topk_mask": None,
                                   "ws": None}),
        ("ws misaligned", {"ws": P + 8}), ("ws small", {"ws_bytes": 0}),
        ("topk<1+border<0", {"topk": 0, "border": -1}), ("border+nms_ksize", {"border": 4, "nms_ksize": 4}),
        ("nms_ksize+gauss_ksize", {"nms_ksize": 0, "gauss_ksize": 16}),
            ("gauss_ksize+gauss_sigma", {"gauss_ksize": 2, "gauss_sigma": NAN}),
        ("gauss_sigma+nms_thresh", {"gauss_sigma": -1.0, "nms_thresh": NAN}),
            ("nms_thresh+kori alone", {"nms_thresh": NAN, "ori_map": None}),
        ("kori alone+n_images==0", {"ori_map": None, "n_images": 0}),
            ("kpts NULL+ws misaligned", {"kpts": None, "ws": P + 8}),
        ("ws misaligned+ws small", {"ws": P + 8, "ws_bytes": 0})])
    add("hn_warp_score", _GT_SHAPES + [
        ("border<0", {"border": -1}), ("border", {"border": 4}), ("align_corners", {"align_corners": 2}),
        ("n_images==0", {"n_images": 0, "homo": None}), ("no outputs", {"warped": None, "visible": None, "homo": None}),
        ("homo NULL", {"homo": None}), ("score NULL", {"score": None}),
            ("visible only", {"score": None, "warped": None, "homo": None}),
        ("height<2+border", {"height": 1, "border": 4}), ("border+align_corners", {"border": 4, "align_corners": -1}),
        ("align_corners+no outputs", {"align_corners": 2, "warped": None, "visible": None})])
    add("hn_gt_scale_orin", _GT_SHAPES + [("n_images==0", {"n_images": 0, "ori": None}),
        ("homo21 NULL", {"homo21": None}),
                                          ("scale NULL+gt_ori misaligned", {"scale": None, "gt_ori": P + 4}),
                                          ("gt_scale NULL+ori misaligned", {"gt_scale": None, "ori": P + 4})])
    add("hn_mask_keypoints", _GT_SHAPES + [
        ("topk<1", {"topk": 0}), ("topk>hw", {"topk": 65}),
            ("n_images*topk", {"n_images": 1 << 59, "height": 2, "width": 2, "topk": 4}),
        ("kori alone", {"ori_map": None}), ("n_images==0", {"n_images": 0, "mask": None}),
            ("kscale NULL", {"kscale": None}),
        ("optional NULL+mask NULL", {"scale_map": None, "ori_map": None, "kori": None, "counts": None, "mask": None}),
        ("hw>=2^31+topk<1", dict(HW31, topk=0)), ("topk<1+ori_map alone", {"topk": 0, "kori": None}),
        ("ori_map alone+n_images==0", {"kori": None, "n_images": 0})])
    add("hn_project_keypoints", _GT_SHAPES + [
        ("n<0", {"n": -1}), ("no images", {"n_images": 0}), ("clamp", {"clamp": 2}), ("ori_r alone", {"ori_map": None}),
        ("n==0", {"n": 0, "kpts": None}), ("n==0 no images", {"n": 0, "n_images": 0}),
            ("scale_r NULL", {"scale_r": None}),
        ("n<0+height<2", {"n": -1, "height": 1}), ("no images+clamp", {"n_images": 0, "clamp": 2}),
        ("clamp+ori_map alone", {"clamp": -1, "ori_r": None}), ("ori_r alone+n==0", {"ori_map": None, "n": 0}),
        ("optional NULL+homo NULL", {"scale_map": None, "ori_map": None, "ori_r": None, "homo": None})])
    return c


def cases():
    """[(id, function name, argument list)]: SPEC's values with the case's overrides."""
    out, seen = [], set()
    for fn, tag, kw in _cases():
        names = [n for n, _ in SPEC[fn]]
        assert set(kw) <= set(names), (fn, tag, set(kw) - set(names))
        assert f"{fn}: {tag}" not in seen, (fn, tag)
        seen.add(f"{fn}: {tag}")
        args = [kw[n] if n in kw else (v() if callable(v) else v) for n, v in SPEC[fn]]
        out.append((f"{fn}: {tag}", fn, args))
    return out


def run(case):
    """(return code, hn_last_error()) of one case; the message only where the call failed."""
    lib = N.load_library()
    _, fn, args = case
    rc = getattr(lib, fn)(*args)
    return [rc, lib.hn_last_error().decode() if rc else ""]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [HN_LIB=<library>] python tests/abi_error_cases.py --record")
    got = {c[0]: run(c) for c in cases()}
    bad = {k: v for k, v in got.items() if v[0] not in (0, 1, 4)}
    if bad:
        sys.exit(f"cases that do not end in an argument check: {bad}")
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(got[k])}" for k in sorted(got)) + "\n}\n")
    print(f"recorded {len(got)} cases from {N.lib_path()} into {GOLDEN}")
