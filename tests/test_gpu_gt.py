"""The homography ground-truth stage on the GPU: hn_warp_score, hn_gt_scale_orin, hn_mask_keypoints,
hn_project_keypoints, the native ``Network.forward`` and ``matching.eval_model`` (tests/golden/gt.npz and the package's
fp64 torch paths on the CPU as ground truth; the exclusion rules are tests/gt_helpers.py's)."""
import numpy as np
import pytest
import torch

import gt_helpers as G
from fixtures import build_module, load
from hardnetnas_amd import _native as N
from hardnetnas_amd import losses, matching
from hardnetnas_amd import network as NW
from hardnetnas_amd.detector import BORDER, RFDet

pytestmark = pytest.mark.gpu
SCALE_TOL = 1e-4  # a flipped truncation moves the scale by >= 0.1, rounding by about 1e-5


@pytest.fixture(scope="module")
def fx():
    return load("gt")


def t(a, dev=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(dev) if dev is not None else x


def err(a, ref, keep=None):
    d = (a.detach().cpu().double() - ref.double()).abs()
    if d.dim() > (keep.dim() if keep is not None else d.dim()):
        d = d.amax(-1)
    return float((d[keep] if keep is not None else d).max())


def check_gt(gs, go, gs64, go64, ex, e_ori, what):
    """gt scale / orientation [B,H,W] / [B,H,W,2] (GPU) against the fp64 evaluation under the exclusion mask."""
    keep = ~ex
    e_s, e_o = err(gs, gs64, keep), err(go, go64, keep)
    print(f"{what}: gt scale err {e_s:.3e} (<= {SCALE_TOL:g}), gt ori err {e_o:.3e} (4 E = {4 * e_ori:.3e})")
    assert e_s <= SCALE_TOL and e_o <= 4 * e_ori
    if bool(ex.any()):
        assert bool(torch.isfinite(gs.cpu()[ex]).all())
        assert float((go.cpu()[ex].double().norm(dim=-1) - 1).abs().max()) <= 1e-5


def check_projection(kr, sr, orr, kr64, kex, scale_map, ori_map, B, H, W, what):
    """Projected keypoints exact on the kept ones, within a pixel on the excluded; the gathers bit-equal to the maps
    at the returned coordinates (through the clamped index)."""
    kr_c = kr.cpu()
    assert torch.equal(kr_c[~kex], kr64[~kex]), what
    assert int((kr_c - kr64).abs().max()) <= 1
    idx = (kr_c[:, 0] * (H * W) + kr_c[:, 1] * W + kr_c[:, 2]).clamp(0, B * H * W - 1)
    assert torch.equal(sr.cpu(), scale_map.cpu().reshape(-1)[idx]), what
    assert torch.equal(orr.cpu(), ori_map.cpu().reshape(-1, 2)[idx]), what


def test_golden(fx, cuda_device):
    dev, m = cuda_device, fx["meta"]
    B, H, W = m["B"], m["H"], m["W"]
    score, ori, h12, h21 = t(fx["score"], dev), t(fx["ori"], dev), t(fx["homo12"], dev), t(fx["homo21"], dev)
    for a in (0, 1):
        warped, visible = N.warp_score(score, h12, border=m["border"], align_corners=bool(a))
        w64 = t(fx[f"warped_ac{a}"]).double() + t(fx[f"warped64_minus_32_ac{a}"]).double()
        v64 = t(fx[f"visible_ac{a}"]).double() + t(fx[f"visible64_minus_32_ac{a}"]).double()
        e_w, e_v = err(warped, w64), err(visible, v64)
        print(f"align_corners {a}: warp err {e_w:.3e} (4 E = {4 * m[f'E_warp_ac{a}']:.3e}), "
              f"visible err {e_v:.3e} (4 E = {4 * m[f'E_visible_ac{a}']:.3e})")
        assert e_w <= 4 * m[f"E_warp_ac{a}"] and e_v <= 4 * m[f"E_visible_ac{a}"]
    for tag in ("const", "var"):
        sm = t(fx["scale_var"], dev) if tag == "var" else None
        gs, go = N.gt_scale_orin(sm, ori, h12, h21, scale_value=32.0)
        go64 = t(fx[f"gt_ori_{tag}"]).double() + t(fx[f"gt_ori64_minus_32_{tag}"]).double()
        check_gt(gs, go, t(fx[f"gt_scale64_{tag}"]), go64, t(fx[f"gt_excluded_{tag}"]), m[f"E_gt_ori_{tag}"],
                 f"golden {tag}")
    kpts, kex = t(fx["kpts"], dev), t(fx["kp_excluded"])
    r_scale, r_ori = t(fx["gt_scale_var"], dev), t(fx["gt_ori_var"], dev)
    for clamp in (1, 0):
        kr, sr, orr = N.project_keypoints(kpts, h12, (B, H, W), scale_map=r_scale, ori_map=r_ori, clamp=bool(clamp))
        check_projection(kr, sr, orr, t(fx[f"proj_kpts64_clamp{clamp}"]), kex, r_scale, r_ori, B, H, W, f"clamp {clamp}")
        assert torch.equal(kr.cpu(), t(fx[f"proj_kpts_clamp{clamp}"]))  # and the reference's own fp32 rows
        assert torch.equal(sr.cpu(), t(fx[f"proj_scale_clamp{clamp}"]))
        assert torch.equal(orr.cpu(), t(fx[f"proj_ori_clamp{clamp}"]))


@pytest.mark.parametrize("border", [0, 8])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(17, 19), (61, 83), (130, 259)])
def test_sizes(cuda_device, H, W, B, border):
    """One pixel inside the border rule, the fixture's size, and more than one tile in both directions with odd
    sizes, against the package's fp64 torch path on the CPU; E is that path's own fp32 error on the same inputs."""
    dev = cuda_device
    c = G.case_inputs(H, W, B, 1000 + H + B)
    d64 = {k: t(v) for k, v in c.items()}
    score64, ori64, scale64 = d64["score"].unsqueeze(-1), d64["ori"], d64["scale"].unsqueeze(-1)
    h12_64, h21_64 = d64["homo12"], d64["homo21"]
    with torch.no_grad():
        ref = {}
        for dt in (torch.float64, torch.float32):
            s, o, sc, a, b_ = (x.to(dt) for x in (score64, ori64, scale64, h12_64, h21_64))
            ref[dt] = (NW.warp(NW.filter_border(s, border) if border else s, a).squeeze(-1),
                       NW.warp(torch.ones_like(s), a).squeeze(-1), *NW.gt_scale_orin(sc, o, a, b_))
    e_w, e_v = err(ref[torch.float32][0], ref[torch.float64][0]), err(ref[torch.float32][1], ref[torch.float64][1])
    ex, min_w = G.gt_exclusion(c["scale"], c["homo12"], c["homo21"])
    assert min_w > 0.5 and float(ex.mean()) <= G.GT_EXCLUDED_CAP
    ex = t(ex)
    e_o = err(ref[torch.float32][3].squeeze(0), ref[torch.float64][3].squeeze(0), ~ex)
    score, ori, scale = d64["score"].float().to(dev), ori64.float().to(dev), d64["scale"].float().to(dev)
    h12, h21 = h12_64.float().to(dev), h21_64.float().to(dev)
    warped, visible = N.warp_score(score, h12, border=border)
    g_w, g_v = err(warped, ref[torch.float64][0]), err(visible, ref[torch.float64][1])
    print(f"{H}x{W} B {B} border {border}: warp err {g_w:.3e} (4 E = {4 * e_w:.3e}), visible err {g_v:.3e} "
          f"(4 E = {4 * e_v:.3e})")
    assert g_w <= 4 * e_w and g_v <= 4 * e_v
    gs, go = N.gt_scale_orin(scale, ori, h12, h21)
    check_gt(gs, go, ref[torch.float64][2].squeeze(-1), ref[torch.float64][3].squeeze(0), ex, e_o, f"{H}x{W} B {B}")
    kp = d64["mask"].unsqueeze(-1).nonzero()
    kr64, kex, _, _ = G.project_keypoints64(kp.numpy(), c["homo12"], H, W)
    assert float(kex.mean()) <= G.KP_EXCLUDED_CAP
    kr, sr, orr = N.project_keypoints(kp.to(dev), h12, (B, H, W), scale_map=gs, ori_map=go, clamp=True)
    check_projection(kr, sr, orr, t(kr64), t(kex), gs, go, B, H, W, f"{H}x{W}")
    # and the same rows through the mask
    K = int(c["mask"][0].sum())
    kpts, ks, ko, counts = N.mask_keypoints(d64["mask"].to(dev), K, scale_map=scale, ori_map=ori, want_counts=True)
    assert torch.equal(kpts.cpu(), kp) and torch.equal(counts.cpu(), torch.full((B,), K, dtype=torch.int32))


def test_align_corners_identity(fx, cuda_device):
    dev, m = cuda_device, fx["meta"]
    score = t(fx["score"], dev)
    eye = torch.eye(3, device=dev).repeat(score.shape[0], 1, 1)
    warped, visible = N.warp_score(score, eye, border=m["border"], align_corners=True)
    want = NW.filter_border(score.unsqueeze(-1), m["border"]).squeeze(-1)
    assert err(warped, want.cpu()) <= 4 * m["E_warp_ac1"]
    assert err(visible, torch.ones_like(want).cpu()) <= 4 * m["E_visible_ac1"]
    w0, v0 = N.warp_score(score, eye, border=m["border"], align_corners=False)
    s64 = t(fx["score"]).double().unsqueeze(-1)
    with torch.no_grad():
        ref_w = NW.warp(NW.filter_border(s64, m["border"]), eye.cpu().double()).squeeze(-1)
        ref_v = NW.warp(torch.ones_like(s64), eye.cpu().double()).squeeze(-1)
    assert err(w0, ref_w) <= 4 * m["E_warp_ac0"] and err(v0, ref_v) <= 4 * m["E_visible_ac0"]
    assert err(w0, want.cpu()) > 0.1  # under 0 the identity homography is no identity warp


def test_out_of_view(fx, cuda_device):
    dev, m = cuda_device, fx["meta"]
    B, H, W = m["B"], m["H"], m["W"]
    score = t(fx["score"], dev)
    shift = torch.eye(3, device=dev).repeat(B, 1, 1)
    shift[:, 0, 2] = 2.0 * W
    warped, visible = N.warp_score(score, shift, border=m["border"])
    assert float(warped.abs().max()) == 0.0 and float(visible.abs().max()) == 0.0
    kpts = t(fx["kpts"], dev)
    kr, _, _ = N.project_keypoints(kpts, shift, (B, H, W), clamp=False)
    assert int(kr[:, 2].min()) >= W and torch.equal(kr[:, 1], kpts[:, 1]) and torch.equal(kr[:, 0], kpts[:, 0])
    kr, sr, _ = N.project_keypoints(kpts, shift, (B, H, W), clamp=True)
    assert bool((kr[:, 2] == W - 1).all()) and bool((sr == 32.0).all())


@pytest.mark.parametrize("K", [1, 48])
def test_mask_keypoints(fx, cuda_device, K):
    dev, m = cuda_device, fx["meta"]
    B, H, W = m["B"], m["H"], m["W"]
    rng = np.random.RandomState(7 + K)
    mask = G.random_mask(rng, B + 1, H, W, K, border=0)
    short = max(K - 5, 0)  # the middle image has fewer than K set pixels (none for K = 1)
    keep = np.argwhere(mask[1])[:short]
    mask[1] = 0
    mask[1][keep[:, 0], keep[:, 1]] = 255
    scale = torch.rand(B + 1, H, W, generator=torch.Generator().manual_seed(K)) * 40 + 8
    ori = t(G.unit_vectors(rng, (B + 1, H, W))).float()
    mk = t(mask)
    out = N.mask_keypoints(mk.to(dev), K, scale_map=scale.to(dev), ori_map=ori.to(dev), want_counts=True)
    kpts, ks, ko, counts = (x.cpu() for x in out)
    assert torch.equal(counts, torch.tensor([K, short, K], dtype=torch.int32))
    assert tuple(kpts.shape) == ((B + 1) * K, 4) and kpts.dtype == torch.int64
    for b in range(B + 1):
        sel = mk[b].bool()
        nz = mk[b].nonzero()
        n = nz.shape[0]
        rows = kpts[b * K:(b + 1) * K]
        assert torch.equal(rows[:n, 1:3], nz) and bool((rows[:, 0] == b).all()) and bool((rows[:, 3] == 0).all())
        assert torch.equal(ks[b * K:b * K + n], scale[b].masked_select(sel))
        assert torch.equal(ko[b * K:b * K + n], ori[b][sel])
        assert bool((rows[n:, 1:] == 0).all())
    again = N.mask_keypoints(mk.to(dev), K, scale_map=scale.to(dev), ori_map=ori.to(dev), want_counts=True)
    assert all(torch.equal(a.cpu(), b_) for a, b_ in zip(again, (kpts, ks, ko, counts)))
    # more set pixels than K: the first K in raster order; no maps: the scale value
    full = torch.ones(1, H, W, dtype=torch.uint8)
    kp, ks1, ko1, cnt = N.mask_keypoints(full.to(dev), K, scale_value=24.0, want_counts=True)
    assert ko1 is None and int(cnt[0]) == H * W and bool((ks1 == 24.0).all())
    assert torch.equal(kp.cpu()[:, 1:3], full[0].nonzero()[:K])


def guarded(x, dev):
    """``x`` in the middle of a larger allocation filled with 1e30 (255 for masks)."""
    pad = 4096
    fill = 255 if x.dtype == torch.uint8 else (1 << 40 if x.dtype == torch.int64 else 1e30)
    big = torch.full((x.numel() + 2 * pad,), fill, dtype=x.dtype, device=dev)
    big[pad:pad + x.numel()] = x.reshape(-1).to(dev)
    return big[pad:pad + x.numel()].view(x.shape)


def test_guarded_inputs(fx, cuda_device):
    """Value check on defined inputs: a horizon line through the image and NaN / Inf entries for one image of three
    leave the other two images' outputs unchanged bit for bit; every input sits between 1e30 guards."""
    dev, m = cuda_device, fx["meta"]
    H, W, K = m["H"], m["W"], m["K"]
    c = G.case_inputs(H, W, 3, 4242, K=K)
    score, ori, scale = (guarded(t(c[k]).float(), dev) for k in ("score", "ori", "scale"))
    mask = guarded(t(c["mask"]), dev)
    good12, good21 = t(c["homo12"]).float(), t(c["homo21"]).float()
    outs = {}
    for name, bad12, bad21 in (
            ("good", good12[1], good21[1]),
            ("horizon", torch.tensor([[1.0, 0, 0], [0, 1, 0], [1, 0, -W / 2]]), torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 1, -H / 2]])),
            ("nonfinite", torch.tensor([[float("nan"), 0, 0], [0, float("inf"), 0], [0, 0, 1]]),
             torch.tensor([[1.0, 0, float("-inf")], [0, 1, 0], [float("nan"), 0, 1]]))):
        h12, h21 = good12.clone(), good21.clone()
        h12[1], h21[1] = bad12, bad21
        h12, h21 = guarded(h12, dev), guarded(h21, dev)
        warped, visible = N.warp_score(score, h12, border=m["border"])
        gs, go = N.gt_scale_orin(scale, ori, h12, h21)
        kp, ks, ko, _ = N.mask_keypoints(mask, K, scale_map=scale, ori_map=ori)
        kr, sr, orr = N.project_keypoints(guarded(kp, dev), h12, (3, H, W), scale_map=scale, ori_map=ori, clamp=False)
        outs[name] = (warped, visible, gs, go, kr.view(3, K, 4), sr.view(3, K), orr.view(3, K, 2))
        finite = warped[torch.isfinite(warped)]
        assert float(finite.abs().max()) <= float(score.abs().max())
        v = visible[torch.isfinite(visible)]
        assert float(v.min()) >= 0.0 and float(v.max()) <= 1.0 + 4 * m["E_visible_ac0"]
        assert float(ks.max()) < 48.0 and float(sr.max()) < 48.0 and float(orr.abs().max()) <= 1.0  # no guard value read
    for name in ("horizon", "nonfinite"):
        for a, b_ in zip(outs["good"], outs[name]):
            assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2]), name


# ---- Network ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def network_and_batch(fx, cuda_device):
    dev = cuda_device
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
    net = NW.Network(det, des, m["SCORE_W"], m["PAIR_W"], 32, m["network_topk"]).eval().to(dev)
    B = m["B"]
    images = t(det_fx["images"], dev)
    im1, im2 = images[:B].contiguous(), images[1:B + 1].contiguous()
    info = torch.ones(B, 2, device=dev)
    return net, (im1, info, t(fx["homo12"], dev), im2, info, t(fx["homo21"], dev), im1, im2)


def test_network_forward(fx, network_and_batch):
    net, batch = network_and_batch
    im1, info, h12, im2, _, h21, _, _ = batch
    with torch.no_grad():
        assert net._native_ok(batch)
        end = net(batch)
        plt, det_loss, des_loss = net.criterion(end)
    ref = fx["meta"]["endpoint"]
    assert list(end) == list(ref)
    for k, v in end.items():
        assert list(v.shape) == ref[k]["shape"] and str(v.dtype) == ref[k]["dtype"], k
    # the composition of the separately tested calls
    det, K = net.det, int(net.det.TOPK)
    sel, sv = det._select_args(), float(det.scale_list[0])
    nm = N.NativeModel.from_module(net.des, im1.device)
    ratio = info[:, 0].contiguous()
    s1, o1 = det.forward_maps(im1)
    s2, o2 = det.forward_maps(im2)
    shape = tuple(s1.shape)
    gt = {"im1": N.gt_scale_orin(None, o2, h12, h21, scale_value=sv),
          "im2": N.gt_scale_orin(None, o1, h21, h12, scale_value=sv)}
    for tag, sl, ol, sr, orr, hlr, raw_l, raw_r, other in (("im1", s1, o1, s2, o2, h12, im1, im2, "im2"),
                                                          ("im2", s2, o2, s1, o1, h21, im2, im1, "im1")):
        warped, visible = N.warp_score(sr, hlr, border=BORDER)
        g = N.select_keypoints(warped, *sel, dense=True)
        assert torch.equal(end[tag + "_gtsc"], g["score_proc"].unsqueeze(-1))
        assert torch.equal(end[tag + "_visible"], visible.unsqueeze(-1))
        assert torch.equal(end[tag + "_score"], N.select_keypoints(sl, *sel, dense=True)["score_proc"].unsqueeze(-1))
        limc, ls, lo, _ = N.mask_keypoints(g["topk_mask"], K, scale_value=sv, ori_map=ol)
        rimcw, rs, ro = N.project_keypoints(limc, hlr, shape, scale_map=gt[other][0], ori_map=gt[other][1])
        _, ps, po = N.project_keypoints(limc, hlr, shape, scale_value=sv, ori_map=orr)
        assert torch.equal(end[tag + "_limc"], limc) and torch.equal(end[tag + "_rimcw"], rimcw)
        assert torch.equal(end[tag + "_lpdes"], nm.forward_keypoints(raw_l, limc, ls, lo, ratio))
        assert torch.equal(end[tag + "_lpreddes"], end[tag + "_lpdes"])
        assert torch.equal(end[tag + "_rpdes"], nm.forward_keypoints(raw_r, rimcw, rs, ro, ratio))
        assert torch.equal(end[tag + "_rpreddes"], nm.forward_keypoints(raw_r, rimcw, ps, po, ratio))
    e = end
    score_loss = (det.loss(e["im1_score"], e["im1_gtsc"], e["im1_visible"])
                  + det.loss(e["im2_score"], e["im2_gtsc"], e["im2_visible"])) / 2.0 * net.SCORE_W
    pair_loss = (losses.pair_distance_loss(e["im1_lpreddes"], e["im1_rpreddes"])
                 + losses.pair_distance_loss(e["im2_lpreddes"], e["im2_rpreddes"])) / 2.0 * net.PAIR_W
    hard_loss = (losses.loss_neimask(e["im1_lpdes"], e["im1_rpdes"], e["im1_limc"], e["im1_rimcw"],
                                     margin=net.des.MARGIN, C=net.des.C)
                 + losses.loss_neimask(e["im2_lpdes"], e["im2_rpdes"], e["im2_limc"], e["im2_rimcw"],
                                       margin=net.des.MARGIN, C=net.des.C)) / 2.0
    assert torch.equal(plt["scalar"]["score_loss"], score_loss) and torch.equal(plt["scalar"]["pair_loss"], pair_loss)
    assert torch.equal(plt["scalar"]["hard_loss"], hard_loss)
    assert torch.equal(det_loss, (score_loss + pair_loss).mean()) and torch.equal(des_loss, hard_loss.mean())
    print("native losses", {k: float(v) for k, v in plt["scalar"].items()}, "reference", fx["meta"]["losses"])
    with torch.no_grad():
        again = net(batch)
    assert all(torch.equal(end[k], again[k]) for k in end)


def test_eval_model(fx, network_and_batch):
    net, batch = network_and_batch
    one = tuple(x[:1].contiguous() for x in batch)
    with torch.no_grad():
        got = matching.eval_model(net, one, 1.0, 5.0)
        # the same function through the package's torch paths, on the same keypoints and descriptors
        scale1, kp1, des1, _, _, _ = net.inference(one[0], one[1], one[6])
        scale2, kp2, des2, _, _, _ = net.inference(one[3], one[4], one[7])

        class Fixed:
            calls = [(scale1.cpu(), kp1.cpu(), des1.cpu(), None, None, None),
                     (scale2.cpu(), kp2.cpu(), des2.cpu(), None, None, None)]

            def inference(self, *a):
                return self.calls.pop(0)

        want = matching.eval_model(Fixed(), tuple(x.cpu() for x in one), 1.0, 5.0)
    print("eval_model", got, want)
    assert len(got) == 6 and tuple(got) == tuple(want)


def test_graph_capture(fx, cuda_device):
    """The four calls allocate (through torch's graph pool) and synchronise nothing: captured on one side stream (a
    single-branch graph) and replayed once they give the eager result."""
    dev, m = cuda_device, fx["meta"]
    B, H, W, K = m["B"], m["H"], m["W"], m["K"]
    score, ori, scale = t(fx["score"], dev), t(fx["ori"], dev), t(fx["scale_var"], dev)
    h12, h21, mask = t(fx["homo12"], dev), t(fx["homo21"], dev), t(fx["mask"], dev)

    def run(sc):
        warped, visible = N.warp_score(sc, h12, border=m["border"])
        gs, go = N.gt_scale_orin(scale, ori, h12, h21)
        kp, ks, ko, cnt = N.mask_keypoints(mask, K, scale_map=scale, ori_map=ori, want_counts=True)
        kr, sr, orr = N.project_keypoints(kp, h12, (B, H, W), scale_map=gs, ori_map=go, clamp=True)
        return warped, visible, gs, go, kp, ks, ko, cnt, kr, sr, orr

    eager = [x.clone() for x in run(score)]
    static = torch.zeros_like(score)
    run(static)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            outs = run(static)
    static.copy_(score)
    g.replay()
    torch.cuda.synchronize()
    for a, b_ in zip(outs, eager):
        assert torch.equal(a, b_)


def test_module_functions_take_the_native_path(fx, cuda_device):
    """``network.warp`` / ``gt_scale_orin`` / ``ptCltoCr`` / ``pair`` on HIP fp32 tensors return the library's results
    bit for bit, in the reference's shapes."""
    dev, m = cuda_device, fx["meta"]
    B, H, W, K = m["B"], m["H"], m["W"], m["K"]
    score, ori, scale = t(fx["score"], dev), t(fx["ori"], dev), t(fx["scale_var"], dev)
    h12, h21, mask = t(fx["homo12"], dev), t(fx["homo21"], dev), t(fx["mask"], dev)
    with torch.no_grad():
        for a in (False, True):
            got = NW.warp(score.unsqueeze(-1), h12, align_corners=a)
            assert torch.equal(got, N.warp_score(score, h12, border=0, align_corners=a)[0].unsqueeze(-1))
        gs, go = NW.gt_scale_orin(scale.unsqueeze(-1), ori, h12, h21)
        ngs, ngo = N.gt_scale_orin(scale, ori, h12, h21)
        assert tuple(gs.shape) == (B, H, W, 1) and tuple(go.shape) == (1, B, H, W, 2)
        assert torch.equal(gs.squeeze(-1), ngs) and torch.equal(go.squeeze(0), ngo)
        kpts = t(fx["kpts"], dev)
        for clamp in (True, False):
            rc, rs, ro = NW.ptCltoCr(kpts, h12, gs, go, clamp=clamp)
            nrc, nrs, nro = N.project_keypoints(kpts, h12, (B, H, W), scale_map=ngs, ori_map=ngo, clamp=clamp)
            assert torch.equal(rc, nrc) and torch.equal(rs, nrs) and torch.equal(ro, nro)
        info = torch.ones(B, 2, device=dev)
        raw1, raw2 = t(fx["raw1"], dev), t(fx["raw2"], dev)
        ppair, limc, rimc = NW.pair(mask.unsqueeze(-1), None, scale.unsqueeze(-1), ori, info, raw1, h12, gs, go, info,
                                    raw2, 32, topk=K)
        kp, ks, ko, _ = N.mask_keypoints(mask, K, scale_map=scale, ori_map=ori)
        nrc, nrs, nro = N.project_keypoints(kp, h12, (B, H, W), scale_map=ngs, ori_map=ngo, clamp=True)
        ratio = info[:, 0].contiguous()
        want = torch.cat((N.clip_patch(raw1, kp, ks, ko, ratio), N.clip_patch(raw2, nrc, nrs, nro, ratio)), 1)
        assert torch.equal(limc, kp) and torch.equal(rimc, nrc) and torch.equal(ppair, want)
        assert torch.equal(limc.cpu(), t(fx["pair_limc"])) and torch.equal(rimc.cpu(), t(fx["pair_rimc"]))
        # without topk the row count has to be read back: nonzero() and the torch gathers, the same rows
        p2, l2, r2 = NW.pair(mask.unsqueeze(-1), None, scale.unsqueeze(-1), ori, info, raw1, h12, gs, go, info, raw2, 32)
        assert torch.equal(l2, limc) and torch.equal(r2, rimc) and torch.equal(p2, ppair)
