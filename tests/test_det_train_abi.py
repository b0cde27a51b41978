"""The C ABI's additions for the detector's training step (hn_det_train_*): header, binding and library agree, and
every argument check runs before the GPU is touched."""
import ctypes
import os

import pytest

from hardnetnas_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hn_det_train_workspace_bytes", "hn_det_train_forward", "hn_det_train_backward")
P = ctypes.c_void_p(4096)  # never dereferenced: every check runs before the GPU is touched
BIG = 1 << 40


def table(fill=4096, hole=None):
    a = (ctypes.c_void_p * N.DET_TRAIN_TENSORS)(*[fill] * N.DET_TRAIN_TENSORS)
    if hole is not None:
        a[hole] = None
    return a


def sizes(n, h, w):
    sv, sc = ctypes.c_size_t(), ctypes.c_size_t()
    rc = N.load_library().hn_det_train_workspace_bytes(n, h, w, ctypes.byref(sv), ctypes.byref(sc))
    return rc, sv.value, sc.value


def fwd(n=2, h=8, w=8, images=P, tensors=None, bn_eps=1e-5, in_eps=1e-5, mom=0.1, score=P, ori=P, saved=P,
        saved_bytes=BIG, scratch=P, scratch_bytes=BIG):
    return N.load_library().hn_det_train_forward(images, n, h, w, tensors if tensors is not None else table(), bn_eps,
                                                 in_eps, mom, score, ori, saved, saved_bytes, scratch, scratch_bytes,
                                                 None)


def bwd(n=2, h=8, w=8, dscore=P, dori=P, images=P, tensors=None, grads=None, saved=P, saved_bytes=BIG, scratch=P,
        scratch_bytes=BIG):
    return N.load_library().hn_det_train_backward(dscore, dori, images, n, h, w,
                                                  tensors if tensors is not None else table(),
                                                  grads if grads is not None else table(), saved, saved_bytes,
                                                  scratch, scratch_bytes, None)


def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    lib = N.load_library()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header and s in N.EXPORTED and hasattr(lib, s), s
        assert getattr(lib, s).restype is ctypes.c_int and getattr(lib, s).argtypes
    assert "#define HN_ABI_VERSION 2" in header and lib.hn_abi_version() == 2
    assert "#define HN_DET_TRAIN_TENSORS 40" in header and N.DET_TRAIN_TENSORS == 40


def test_workspace_sizes():
    lib = N.load_library()
    rc, sv, sc = sizes(1, 240, 320)
    assert rc == 0 and sv >= 95 * 4 * 240 * 320 and sc > 0 and sv % 4 == 0
    assert sizes(2, 33, 40)[1] > sizes(1, 33, 40)[1]
    assert sizes(1, 1, 2)[0] == 0
    for bad, msg in (((0, 8, 8), b"n_images"), ((-1, 8, 8), b"n_images"), ((1, 0, 8), b"height"),
                     ((1, 8, 0), b"width"), ((1, 1, 1), b">= 2"), ((1, 1 << 16, 1 << 16), b"2^31"),
                     (((1 << 24) + 1, 8, 8), b"2^24")):
        assert sizes(*bad)[0] == 1 and msg in lib.hn_last_error(), (bad, lib.hn_last_error())
    assert lib.hn_det_train_workspace_bytes(1, 8, 8, None, None) == 1


BAD_SHAPES = [({"n": 0}, b"n_images"), ({"h": 0}, b"height"), ({"w": -3}, b"width"),
              ({"n": 1, "h": 1, "w": 1}, b">= 2"), ({"h": 1 << 16, "w": 1 << 16}, b"2^31")]


@pytest.mark.parametrize("kw,msg", BAD_SHAPES)
def test_forward_and_backward_reject_bad_shapes(kw, msg):
    lib = N.load_library()
    assert fwd(**kw) == 1 and msg in lib.hn_last_error(), lib.hn_last_error()
    assert bwd(**kw) == 1 and msg in lib.hn_last_error(), lib.hn_last_error()


def test_forward_pointer_and_workspace_checks_without_touching_gpu():
    lib = N.load_library()
    _, sv, sc = sizes(2, 8, 8)
    assert fwd(saved_bytes=sv - 1, scratch_bytes=sc) == 4 and b"saved workspace too small" in lib.hn_last_error()
    assert fwd(saved_bytes=sv, scratch_bytes=sc - 1) == 4 and b"scratch workspace too small" in lib.hn_last_error()
    for name in ("images", "score", "ori", "saved", "scratch"):
        assert fwd(**{name: None}) == 1 and b"NULL" in lib.hn_last_error(), name
        assert fwd(**{name: ctypes.c_void_p(4096 + 8)}) == 1 and b"16-byte" in lib.hn_last_error(), name
    assert fwd(tensors=table(hole=17)) == 1 and b"NULL tensor pointer 17" in lib.hn_last_error()
    for kw in ({"bn_eps": 0.0}, {"in_eps": -1.0}, {"bn_eps": float("nan")}):
        assert fwd(**kw) == 1 and b"eps" in lib.hn_last_error(), kw
    for mom in (-0.1, 1.5, float("nan")):
        assert fwd(mom=mom) == 1 and b"momentum" in lib.hn_last_error(), mom


def test_backward_pointer_and_workspace_checks_without_touching_gpu():
    lib = N.load_library()
    _, sv, sc = sizes(2, 8, 8)
    assert bwd(saved_bytes=sv - 1, scratch_bytes=sc) == 4 and b"saved workspace too small" in lib.hn_last_error()
    assert bwd(saved_bytes=sv, scratch_bytes=sc - 1) == 4 and b"scratch workspace too small" in lib.hn_last_error()
    for name in ("images", "saved", "scratch"):
        assert bwd(**{name: None}) == 1 and b"NULL" in lib.hn_last_error(), name
    for name in ("dscore", "dori", "images", "saved", "scratch"):
        assert bwd(**{name: ctypes.c_void_p(4096 + 4)}) == 1 and b"16-byte" in lib.hn_last_error(), name
    assert bwd(tensors=table(hole=0)) == 1 and b"NULL tensor pointer 0" in lib.hn_last_error()
    # every parameter slot needs a gradient buffer; the running statistics' slots (3, 4 of features.1) do not
    assert bwd(grads=table(hole=2)) == 1 and b"d_grads[2]" in lib.hn_last_error()
    assert bwd(grads=table(hole=39)) == 1 and b"d_grads[39]" in lib.hn_last_error()
    holes = table()
    for i in (5, 6, 10, 11, 15, 16, 20, 21, 25, 26, 30, 31):
        holes[i] = None
    assert bwd(grads=holes, n=0) == 1 and b"n_images" in lib.hn_last_error()  # reaches no launch: the shape is bad
