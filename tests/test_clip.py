"""Keypoint patch extraction without a GPU: the torch formulation of hardnetnas_amd/patches.py against the
reference's recorded patches (tests/golden/clip_patch.npz, made by tests/golden/make_clip_golden.py from
FDLNet-master/latency/NASNet/utils/image_utils.py:11-158), the argument checks of the C ABI, which run before the
GPU is touched, and the host program that sweeps the kernel's address computation under the sanitizers."""
import ctypes
import os
import subprocess

import pytest
import torch

from fixtures import build_module, load
from hardnetnas_amd import _native as N
from hardnetnas_amd import patches as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hardnetnas_amd", "csrc")
NEW_SYMBOLS = ("hn_clip_patch", "hn_workspace_bytes_kp", "hn_forward_kp")


def clip_case():
    """(tensors of the fixture, fp64 evaluation, metadata); argument order of clip_patch in ``args``."""
    fx = load("clip_patch")
    t = {k: torch.from_numpy(v) for k, v in fx.items() if k != "meta"}
    t["ref64"] = t["ref32"].double() + t["ref64_minus_ref32"].double()
    t["args"] = (t["kpts"], t["scale"], t["ori"], t["im_info"], t["images"])
    return t, fx["meta"]


def test_fp32_formulation_matches_the_reference_patches():
    t, meta = clip_case()
    got = PT.clip_patch(*t["args"], 32)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(t["ref32"].shape)
    keep = ~t["excluded"]
    err = float((got - t["ref32"])[keep].abs().max())
    print(f"fp32 formulation vs reference: {err:.3e} (2 E_ref = {2 * meta['E_ref']:.3e})")
    assert err <= 2 * meta["E_ref"]


def test_fp64_formulation_matches_the_stored_evaluation():
    t, _ = clip_case()
    got = PT.clip_patch(t["kpts"], t["scale"], t["ori"], t["im_info"], t["images"].double(), 32)
    assert got.dtype == torch.float64
    assert float((got - t["ref64"]).abs().max()) <= 1e-12


def test_fixture_conditions_hold():
    t, meta = clip_case()
    assert meta["excluded_share"] <= 0.01 and meta["outside_share"] >= 0.05
    assert abs(float(t["excluded"].double().mean()) - meta["excluded_share"]) < 1e-12
    e_ref = float((t["ref32"].double() - t["ref64"])[~t["excluded"]].abs().max())
    assert abs(e_ref - meta["E_ref"]) < 1e-12 and 1e-6 < meta["E_ref"] < 1e-5  # half an fp32 ulp of a coordinate
    assert t["ref32"].numel() == 3 * 40 * 1024


def test_shuffled_keypoints_permute_the_patches():
    """Column 0 selects the image and the ratio: any keypoint order, and unequal counts per image."""
    t, _ = clip_case()
    kpts, scale, ori, im_info, images = t["args"]
    base = PT.clip_patch(*t["args"], 32)
    perm = torch.randperm(kpts.shape[0], generator=torch.Generator().manual_seed(3))[:77]  # 77: unequal counts
    got = PT.clip_patch(kpts[perm], scale[perm], ori[perm], im_info, images, 32)
    assert torch.equal(got, base[perm])


def test_no_orientation_is_the_identity_rotation():
    t, _ = clip_case()
    kpts, scale, _, im_info, images = t["args"]
    one = torch.tensor([[1.0, 0.0]]).repeat(kpts.shape[0], 1)
    assert torch.equal(PT.clip_patch(kpts, scale, None, im_info, images, 32),
                       PT.clip_patch(kpts, scale, one, im_info, images, 32))


def test_psize_16_matches_the_reference_function():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_clip_golden  # finds the reference tree as the other fixture generators do (HN_REFERENCE)
    if not os.path.exists(make_clip_golden.SOURCE):
        pytest.skip("reference tree not present")
    t, meta = clip_case()
    with torch.no_grad():
        want = make_clip_golden.reference_clip_patch()(*t["args"], 16)
    got = PT.clip_patch(*t["args"], 16)
    assert tuple(got.shape) == tuple(want.shape) == (120, 1, 16, 16)
    from clip_ref import coords64, near_lines
    xs, ys = coords64(t["kpts"], t["scale"], t["ori"], t["im_info"][:, 0], 16)
    keep = ~near_lines(xs, ys, meta["H"], meta["W"]).unsqueeze(1)
    assert float((got - want)[keep].abs().max()) <= 2 * meta["E_ref"]


def test_autograd_reaches_images_and_scale():
    t, _ = clip_case()
    kpts, scale, ori, im_info, images = (x[:5] if i < 3 else x for i, x in enumerate(t["args"]))
    images = images.clone().requires_grad_(True)
    scale = scale.clone().requires_grad_(True)
    PT.clip_patch(kpts, scale, ori, im_info, images, 32).sum().backward()
    assert images.grad is not None and float(images.grad.abs().sum()) > 0
    assert scale.grad is not None and torch.isfinite(scale.grad).all()


@pytest.mark.parametrize("name", ["hardnet", "fdl_NASNet"])
def test_describe_keypoints_is_the_composition_on_cpu(name):
    m, _, _ = build_module(name)
    t, _ = clip_case()
    args = tuple(x[:6] if i < 3 else x for i, x in enumerate(t["args"]))
    with torch.no_grad():
        want = m(PT.clip_patch(*args, 32))
        got = PT.describe_keypoints(m, *args)
    assert tuple(got.shape) == (6, 128) and torch.equal(got, want)


# ---- the C ABI's three additions, without a GPU ------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    lib = N.load_library()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header and s in N.EXPORTED and hasattr(lib, s), s
        assert getattr(lib, s).restype is ctypes.c_int and getattr(lib, s).argtypes
    assert "#define HN_ABI_VERSION 2" in header and lib.hn_abi_version() == 2


GOOD = dict(n_images=2, height=8, width=8, n=4)
BAD_ARGS = [({"n": -1}, b"n must"), ({"n_images": -1}, b"n_images"), ({"height": 1}, b"height"),
            ({"width": 1}, b"width"), ({"width": 0}, b"width"), ({"height": -5}, b"height"),
            ({"n_images": 1 << 40, "height": 1 << 12, "width": 1 << 12}, b"2^63"),
            ({"n_images": 1 << 62, "height": 2, "width": 2}, b"2^63"), ({"n_images": 0}, b"n_images")]


@pytest.mark.parametrize("kw,name", BAD_ARGS)
def test_clip_patch_rejects_bad_arguments_without_touching_gpu(kw, name):
    a = dict(GOOD, **kw)
    lib = N.load_library()
    aligned = ctypes.c_void_p(4096)  # never dereferenced: every check runs before the GPU is touched
    rc = lib.hn_clip_patch(aligned, a["n_images"], a["height"], a["width"], aligned, aligned, None, aligned, a["n"],
                           aligned, None)
    assert rc == 1 and name in lib.hn_last_error(), lib.hn_last_error()
    rc = lib.hn_forward_kp(None, aligned, a["n_images"], a["height"], a["width"], aligned, aligned, None, aligned,
                           a["n"], aligned, aligned, 1 << 40, None)
    assert rc == 1 and name in lib.hn_last_error(), lib.hn_last_error()


def test_clip_patch_pointer_checks_without_touching_gpu():
    lib = N.load_library()
    p = ctypes.c_void_p(4096)
    for i in (0, 4, 5, 7, 9):  # images, kpts, scale, ratio, patches (6 = ori may be NULL)
        args = [p, 2, 8, 8, p, p, None, p, 4, p, None]
        args[i] = None
        assert lib.hn_clip_patch(*args) == 1 and b"NULL" in lib.hn_last_error(), i
    assert lib.hn_clip_patch(p, 2, 8, 8, p, p, None, p, 4, ctypes.c_void_p(4096 + 8), None) == 1
    assert b"16-byte" in lib.hn_last_error()
    # n == 0 is HN_OK whatever the pointers; a bad shape is still an error
    assert lib.hn_clip_patch(None, 0, 8, 8, None, None, None, None, 0, None, None) == 0
    assert lib.hn_clip_patch(None, 0, 1, 8, None, None, None, None, 0, None, None) == 1


def test_forward_kp_needs_a_model_without_touching_gpu():
    lib = N.load_library()
    p = ctypes.c_void_p(4096)
    assert lib.hn_forward_kp(None, p, 2, 8, 8, p, p, None, p, 4, p, p, 1 << 40, None) == 1
    assert b"model is NULL" in lib.hn_last_error()
    sz = ctypes.c_size_t()
    assert lib.hn_workspace_bytes_kp(None, 4, ctypes.byref(sz)) == 1


def test_python_binding_validates_before_the_library():
    im = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="HIP tensor"):
        N.clip_patch(im, torch.zeros(1, 4, dtype=torch.int64), torch.ones(1), None, torch.ones(1))


# ---- the bounds guarantee on the host, before any GPU sees the kernel --------------------------
def test_host_check_of_the_address_computation_is_clean():
    """hn_clip_host_check.cpp calls hn_clip.h's functions (the kernel's own text) on adversarial keypoints, built
    with -fsanitize=address,undefined,float-cast-overflow: exit 0 and no sanitizer report."""
    r = subprocess.run(["make", "-C", CSRC, "clip_check"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "every index in bounds" in out
    assert "runtime error" not in out and "AddressSanitizer" not in out and "Sanitizer" not in out, out[-4000:]
