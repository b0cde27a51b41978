"""The homography ground-truth stage and ``Network`` without a GPU: the torch paths of ``hardnetnas_amd.network``
against the reference's fp32 outputs (tests/golden/gt.npz, tests/golden/make_gt_golden.py), the four new exports and
their argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fixtures import build_module, load
from hardnetnas_amd import _native as N
from hardnetnas_amd import network as NW
from hardnetnas_amd.detector import RFDet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hn_warp_score", "hn_gt_scale_orin", "hn_mask_keypoints", "hn_project_keypoints"]
TOL = 1e-6  # continuous outputs against the reference's fp32 ones


@pytest.fixture(scope="module")
def fx():
    return load("gt")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def maps(fx, sl=slice(None)):
    """(score [B,H,W,1], ori [B,H,W,2], scale_var [B,H,W,1], scale_const, homo12, homo21, mask [B,H,W,1])."""
    score, ori, sv = t(fx["score"][sl]).unsqueeze(-1), t(fx["ori"][sl]), t(fx["scale_var"][sl]).unsqueeze(-1)
    return (score, ori, sv, torch.full_like(sv, 32.0), t(fx["homo12"][sl]), t(fx["homo21"][sl]),
            t(fx["mask"][sl]).unsqueeze(-1))


def close(a, ref, tol=TOL):
    a, ref = a.double(), t(ref).double().reshape(a.shape)
    err = float((a - ref).abs().max())
    assert err <= tol, err


@pytest.mark.parametrize("align", [0, 1])
def test_warp_reproduces_the_reference(fx, align):
    score, _, _, _, h12, _, _ = maps(fx)
    close(NW.warp(NW.filter_border(score), h12, align_corners=bool(align)), fx[f"warped_ac{align}"])
    close(NW.warp(torch.ones_like(score), h12, align_corners=bool(align)), fx[f"visible_ac{align}"])
    for b in range(score.shape[0]):  # B = 1 slices give the same result as inside the batch
        one = NW.warp(NW.filter_border(score[b:b + 1]), h12[b:b + 1], align_corners=bool(align))
        close(one, fx[f"warped_ac{align}"][b:b + 1])
    assert float(np.abs(fx["warped_ac0"] - fx["warped_ac1"]).max()) > 0.1  # the two settings are far apart


def test_warp_default_is_the_references_behaviour(fx):
    score, _, _, _, h12, _, _ = maps(fx)
    assert torch.equal(NW.warp(score, h12), NW.warp(score, h12, align_corners=False))


@pytest.mark.parametrize("tag", ["const", "var"])
def test_gt_scale_orin_reproduces_the_reference(fx, tag):
    _, ori, sv, sc, h12, h21, _ = maps(fx)
    scale = sc if tag == "const" else sv
    gs, go = NW.gt_scale_orin(scale, ori, h12, h21)
    B, H, W, _ = scale.shape
    assert tuple(gs.shape) == (B, H, W, 1) and tuple(go.shape) == (1, B, H, W, 2)
    assert gs.dtype == torch.float32 and go.dtype == torch.float32
    close(gs, fx[f"gt_scale_{tag}"])
    close(go, fx[f"gt_ori_{tag}"])
    # the same through the [1,B,H,W,2] shape the function itself returns, and for B = 1 slices
    gs5, go5 = NW.gt_scale_orin(scale, ori.unsqueeze(0), h12, h21)
    assert torch.equal(gs5, gs) and torch.equal(go5, go)
    for b in range(B):
        g1, o1 = NW.Network.gt_scale_orin(scale[b:b + 1], ori[b:b + 1], h12[b:b + 1], h21[b:b + 1])
        assert tuple(g1.shape) == (1, H, W, 1) and tuple(o1.shape) == (1, 1, H, W, 2)
        close(g1, fx[f"gt_scale_{tag}"][b:b + 1])
        close(o1, fx[f"gt_ori_{tag}"][b:b + 1])


def test_gt_scale_orin_fp64_is_the_fixtures_fp64(fx):
    """The fp64 torch path (the GPU tests' ground truth) equals the reference's fp64 evaluation."""
    _, ori, sv, _, h12, h21, _ = maps(fx)
    gs, go = NW.gt_scale_orin(sv.double(), ori.double(), h12.double(), h21.double())
    keep = ~t(fx["gt_excluded_var"])
    assert float((gs.squeeze(-1).double() - t(fx["gt_scale64_var"]).double()).abs()[keep].max()) <= 1e-6
    ref = t(fx["gt_ori_var"]).double() + t(fx["gt_ori64_minus_32_var"]).double()
    assert float((go.squeeze(0) - ref).abs().amax(-1)[keep].max()) <= 1e-9


@pytest.mark.parametrize("clamp", [1, 0])
def test_ptCltoCr_reproduces_the_reference(fx, clamp):
    _, _, _, _, h12, _, _ = maps(fx)
    kpts = t(fx["kpts"])
    r_scale, r_ori = t(fx["gt_scale_var"]).unsqueeze(-1), t(fx["gt_ori_var"]).unsqueeze(0)
    rc, rs, ro = NW.ptCltoCr(kpts, h12, r_scale, r_ori, clamp=bool(clamp))
    assert rc.dtype == torch.int64 and torch.equal(rc, t(fx[f"proj_kpts_clamp{clamp}"]))
    assert torch.equal(rs, t(fx[f"proj_scale_clamp{clamp}"])) and torch.equal(ro, t(fx[f"proj_ori_clamp{clamp}"]))
    rc2, rs2, ro2 = NW.ptCltoCr(kpts, h12, r_scale, None, clamp=bool(clamp))
    assert ro2 is None and torch.equal(rc2, rc) and torch.equal(rs2, rs)
    # fp64 homographies: the hand projection of the fixture
    rc64, _, _ = NW.ptCltoCr(kpts, h12.double(), r_scale, None, clamp=bool(clamp))
    keep = ~t(fx["kp_excluded"])
    assert torch.equal(rc64[keep], t(fx[f"proj_kpts64_clamp{clamp}"])[keep])
    # one image alone: its own keypoints, batch index 0
    K = fx["meta"]["K"]
    one = kpts[K:2 * K].clone()
    one[:, 0] = 0
    rc1, rs1, ro1 = NW.ptCltoCr(one, h12[1:2], r_scale[1:2], r_ori[:, 1:2], clamp=bool(clamp))
    if clamp:  # unclamped, the gather index of an outside keypoint depends on the batch around it
        assert torch.equal(rs1, rs[K:]) and torch.equal(ro1, ro[K:])
    assert torch.equal(rc1[:, 1:], rc[K:, 1:])


def test_pair_reproduces_the_reference(fx):
    _, ori, sv, _, h12, _, mask = maps(fx)
    r_scale, r_ori = t(fx["gt_scale_var"]).unsqueeze(-1), t(fx["gt_ori_var"]).unsqueeze(0)
    info = torch.ones(mask.shape[0], 2)
    raw1, raw2 = t(fx["raw1"]), t(fx["raw2"])
    ppair, limc, rimc = NW.pair(mask, None, sv, ori, info, raw1, h12, r_scale, r_ori, info, raw2, 32)
    B, K = mask.shape[0], fx["meta"]["K"]
    assert tuple(ppair.shape) == (B * K, 2, 32, 32) and ppair.dtype == torch.float32
    assert torch.equal(limc, t(fx["pair_limc"])) and torch.equal(rimc, t(fx["pair_rimc"]))
    assert torch.equal(limc, t(fx["kpts"]))
    # one image alone
    p1, l1, r1 = NW.pair(mask[:1], None, sv[:1], ori[:1], info[:1], raw1[:1], h12[:1], r_scale[:1], r_ori[:, :1],
                         info[:1], raw2[:1], 32)
    assert torch.equal(l1, limc[:K]) and torch.equal(r1, rimc[:K])
    assert torch.equal(p1, ppair[:K])


def test_pair_patches_reproduce_the_reference(fx):
    """The patch pairs against the reference's, at the 1e-6 set for every continuous output: ``pair``'s torch path
    cuts them in the reference's operation order (``network._clip_patch_matmul``).  ``patches.clip_patch``'s torch
    formulation, the kernel's term-by-term order, is 6.7e-6 away on these inputs (its own bound is 2 E_ref = 1.1e-5,
    tests/test_clip.py) and would miss."""
    _, ori, sv, _, h12, _, mask = maps(fx)
    r_scale, r_ori = t(fx["gt_scale_var"]).unsqueeze(-1), t(fx["gt_ori_var"]).unsqueeze(0)
    info = torch.ones(mask.shape[0], 2)
    ppair, _, _ = NW.pair(mask, None, sv, ori, info, t(fx["raw1"]), h12, r_scale, r_ori, info, t(fx["raw2"]), 32)
    err = float((ppair[t(fx["pair_rows"])] - t(fx["pair_patches"])).abs().max())
    print(f"pair patches vs reference: {err:.3e}")
    assert err <= 1e-6, err


@pytest.fixture(scope="module")
def network_and_batch(fx):
    det_fx = load("detect")
    det = RFDet(**det_fx["meta"]["det_args"]).eval()
    sd, off = det.state_dict(), 0
    for k in det_fx["meta"]["state_dict_keys"]:
        n = sd[k].numel()
        sd[k] = t(det_fx["blob"][off:off + n]).reshape(sd[k].shape)
        off += n
    det.load_state_dict(sd)
    des, _, _ = build_module("fdl_NASNet")
    m = fx["meta"]
    net = NW.Network(det, des, m["SCORE_W"], m["PAIR_W"], 32, m["network_topk"]).eval()
    B = m["B"]
    images = t(det_fx["images"])
    im1, im2 = images[:B].contiguous(), images[1:B + 1].contiguous()
    info = torch.ones(B, 2)
    return net, (im1, info, t(fx["homo12"]), im2, info, t(fx["homo21"]), im1, im2)


def test_network_forward_and_criterion_reproduce_the_reference(fx, network_and_batch):
    net, batch = network_and_batch
    with torch.no_grad():
        end = net(batch)
        plt, det_loss, des_loss = net.criterion(end)
    ref = fx["meta"]["endpoint"]
    assert list(end) == list(ref) == list(NW.ENDPOINT_KEYS) and len(end) == 18
    for k, v in end.items():
        assert list(v.shape) == ref[k]["shape"] and str(v.dtype) == ref[k]["dtype"], k
    for k in ("im1_limc", "im1_rimcw", "im2_limc", "im2_rimcw"):
        assert torch.equal(end[k], t(fx["end_" + k])), k
    for k, v in fx["meta"]["losses"].items():
        assert abs(float(plt["scalar"][k]) - v) <= 1e-5, (k, float(plt["scalar"][k]), v)
    assert abs(float(det_loss) - fx["meta"]["det_loss"]) <= 1e-5
    assert abs(float(des_loss) - fx["meta"]["des_loss"]) <= 1e-5


def test_torch_paths_are_differentiable(fx):
    score, ori, sv, _, h12, h21, _ = maps(fx, slice(0, 1))
    score = score.clone().requires_grad_(True)
    NW.warp(score, h12).sum().backward()
    assert score.grad is not None and float(score.grad.abs().sum()) > 0
    ori = ori.clone().requires_grad_(True)
    _, go = NW.gt_scale_orin(sv, ori, h12, h21)
    (go * torch.arange(2.0)).sum().backward()
    assert ori.grad is not None and float(ori.grad.abs().sum()) > 0


# ---- C ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(hn_\w+)\s*\(", src, re.M))
    lib = N.load_library()
    for s in NEW:
        assert s in declared and s in N.EXPORTED and hasattr(lib, s), s
    assert lib.hn_abi_version() == 2


def test_argument_checks_need_no_gpu():
    lib = N.load_library()
    E = 1  # HN_ERR_ARG
    p = ctypes.c_void_p(256)  # never dereferenced: every check below fails before the GPU is touched

    def warp(h, w, border, n=1, align=0):
        return lib.hn_warp_score(p, p, n, h, w, border, align, p, p, None)

    assert warp(1, 40, 0) == E and warp(40, 1, 0) == E
    assert b"height and width" in lib.hn_last_error()
    assert warp(16, 40, 8) == E and warp(40, 16, 8) == E and warp(40, 40, -1) == E
    assert b"border" in lib.hn_last_error()
    assert warp(40, 40, 8, n=-1) == E and warp(40, 40, 8, align=2) == E
    assert warp(40, 40, 8, n=0) == 0
    assert lib.hn_gt_scale_orin(None, 32.0, p, p, p, 1, 1, 40, p, p, None) == E
    assert lib.hn_gt_scale_orin(None, 32.0, p, p, p, -1, 40, 40, p, p, None) == E
    assert lib.hn_gt_scale_orin(None, 32.0, None, p, p, 1, 40, 40, p, p, None) == E
    assert lib.hn_gt_scale_orin(None, 32.0, p, p, p, 0, 40, 40, p, p, None) == 0

    def mask(h, w, k, n=1, ori_map=None, kori=None):
        return lib.hn_mask_keypoints(p, n, h, w, k, None, 32.0, ori_map, p, p, kori, None, None)

    assert mask(1, 40, 4) == E and mask(40, 40, 0) == E and mask(4, 4, 17) == E and mask(40, 40, 4, n=-1) == E
    assert mask(40, 40, 4, ori_map=p) == E and mask(40, 40, 4, kori=p) == E
    assert b"both" in lib.hn_last_error()
    assert mask(40, 40, 4, n=0) == 0

    def proj(n, h=40, w=40, images=1, clamp=1, ori_map=None, ori_r=None):
        return lib.hn_project_keypoints(p, n, p, images, h, w, None, 32.0, ori_map, clamp, p, p, ori_r, None)

    assert proj(-1) == E and proj(4, h=1) == E and proj(4, w=1) == E and proj(4, images=-1) == E
    assert proj(4, images=0) == E and proj(4, clamp=2) == E
    assert proj(4, ori_map=p) == E and proj(4, ori_r=p) == E
    assert b"both" in lib.hn_last_error()
    assert proj(0) == 0
