"""The C ABI's two additions for the training step (hn_clip_patch_backward, hn_nas_train_backward_dx): header,
binding and library agree, and every argument check of the clip backward runs before the GPU is touched."""
import ctypes
import os

import pytest

from hardnetnas_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hn_clip_patch_backward", "hn_nas_train_backward_dx")


def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    lib = N.load_library()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header and s in N.EXPORTED and hasattr(lib, s), s
        assert getattr(lib, s).restype is ctypes.c_int and getattr(lib, s).argtypes
    assert len(lib.hn_nas_train_backward_dx.argtypes) == len(lib.hn_nas_train_backward.argtypes) + 1
    assert "#define HN_ABI_VERSION 2" in header and lib.hn_abi_version() == 2


GOOD = dict(n_images=2, height=8, width=8, n=4)
BAD_ARGS = [({"n": -1}, b"n must"), ({"n_images": -1}, b"n_images"), ({"height": 1}, b"height"),
            ({"width": 1}, b"width"), ({"width": 0}, b"width"),
            ({"n_images": 1 << 62, "height": 2, "width": 2}, b"2^63"), ({"n_images": 0}, b"n_images")]


@pytest.mark.parametrize("kw,name", BAD_ARGS)
def test_clip_patch_backward_rejects_what_the_forward_rejects(kw, name):
    a = dict(GOOD, **kw)
    lib = N.load_library()
    p = ctypes.c_void_p(4096)  # never dereferenced: every check runs before the GPU is touched
    rc = lib.hn_clip_patch_backward(p, p, a["n_images"], a["height"], a["width"], p, p, p, p, a["n"], p, p, None)
    assert rc == 1 and name in lib.hn_last_error(), lib.hn_last_error()


def test_clip_patch_backward_pointer_checks_without_touching_gpu():
    lib = N.load_library()
    p = ctypes.c_void_p(4096)
    # an orientation gradient without an orientation
    assert lib.hn_clip_patch_backward(p, p, 2, 8, 8, p, p, None, p, 4, p, p, None) == 1
    assert b"d_dori" in lib.hn_last_error()
    assert lib.hn_clip_patch_backward(None, None, 2, 8, 8, None, None, None, None, 0, None, p, None) == 1  # n == 0 too
    for i in (0, 1, 5, 6, 8):  # dpatches, images, kpts, scale, ratio (ori, dscale, dori may be NULL)
        args = [p, p, 2, 8, 8, p, p, p, p, 4, p, p, None]
        args[i] = None
        assert lib.hn_clip_patch_backward(*args) == 1 and b"NULL" in lib.hn_last_error(), i
    assert lib.hn_clip_patch_backward(ctypes.c_void_p(4096 + 8), p, 2, 8, 8, p, p, p, p, 4, p, p, None) == 1
    assert b"16-byte" in lib.hn_last_error()
    # n == 0 is HN_OK whatever the pointers; a bad shape is still an error
    assert lib.hn_clip_patch_backward(None, None, 0, 8, 8, None, None, None, None, 0, None, None, None) == 0
    assert lib.hn_clip_patch_backward(None, None, 0, 8, 1, None, None, None, None, 0, None, None, None) == 1
