"""FDLNet's keypoint detector (hn_det_forward) and keypoint selection (hn_select_keypoints) on the GPU.

Tolerances.  Forward, golden: 4 E against the stored fp64 evaluation, E the reference's own fp32 error on these
inputs (E_score, E_ori from the fixture; the factor 4 is the project's margin for another fp32 evaluation order,
DESIGN section 19).  Forward, generated shapes: the same rule with E the fp32 torch module's own error against
its fp64 form on the same inputs.  Orientation pixels whose fp64 pre-division pair norm is below 0.05 are not
compared by value (the division amplifies the error there without bound); their share is asserted <= 1 %.
Selection: exact.  Against the golden arrays no cut falls inside a group of equal values (asserted by the
generator); against the torch restatement the blur is evaluated in the C ABI's own order (abi_blur), so the
blurred map is compared bit for bit too, and the tie rule (value descending, flat index ascending) decides the
rest.  Against the golden processed score, which the reference sums in another order, the bound is 1e-6."""
from functools import lru_cache

import pytest
import torch

from detect_ref import golden, golden_detector, ori_pair_norm, random_detector
from hardnetnas_amd import _native as N
from hardnetnas_amd import detector as D
from hardnetnas_amd import patches as PT
from hardnetnas_amd.model import HardNet, HardNetNeiMask

pytestmark = pytest.mark.gpu

NORM_FLOOR = 0.05


def detector_maps(det, images, dev):
    nd = N.NativeDetector(N.state_dict_blob(det.state_dict()), dev)
    score, ori = nd.forward(images.to(dev))
    return score.cpu(), ori.cpu()


def test_forward_golden(cuda_device):
    t, m = golden()
    score, ori = detector_maps(golden_detector(), t["images"], cuda_device)
    keep = ~t["ori_excluded"]
    e_s = float((score.double() - t["score64"]).abs().max())
    e_o = float((ori.double() - t["ori64"]).abs().amax(-1)[keep].max())
    print(f"golden: score error {e_s:.3e} (bound {4 * m['E_score']:.3e}), ori error {e_o:.3e} "
          f"(bound {4 * m['E_ori']:.3e})")
    assert e_s <= 4 * m["E_score"] and e_o <= 4 * m["E_ori"]
    assert bool(torch.isfinite(ori[keep]).all())
    # the module takes the same path
    det = golden_detector().to(cuda_device)
    with torch.no_grad():
        s2, sc2, o2 = det(t["images"].to(cuda_device))
    assert torch.equal(s2.squeeze(-1).cpu(), score) and torch.equal(o2.cpu(), ori)
    assert tuple(sc2.shape) == tuple(s2.shape) and float(sc2.min()) == float(sc2.max()) == m["scale"]


@pytest.mark.parametrize("shape", [(1, 17, 17), (2, 33, 40), (1, 64, 64), (2, 97, 131), (1, 240, 320)])
def test_forward_shapes(shape, cuda_device):
    B, H, W = shape
    det = random_detector(seed=H * 1000 + W)
    images = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(H * 7 + W))
    with torch.no_grad():
        s32, _, o32 = det(images)
        det64 = random_detector(seed=H * 1000 + W).double()
        s64, _, o64 = det64(images.double())
    keep = ori_pair_norm(det64, images.double()) >= NORM_FLOOR
    assert float((~keep).double().mean()) <= 0.01
    E_s = float((s32.double() - s64).abs().max())
    E_o = float((o32.double() - o64).abs().amax(-1)[keep].max())
    score, ori = detector_maps(det, images, cuda_device)
    e_s = float((score.double() - s64.squeeze(-1)).abs().max())
    e_o = float((ori.double() - o64).abs().amax(-1)[keep].max())
    print(f"{shape}: score error {e_s:.3e} (bound {4 * E_s:.3e}), ori error {e_o:.3e} (bound {4 * E_o:.3e})")
    assert e_s <= 4 * E_s and e_o <= 4 * E_o


def test_forward_batch_independence_and_graph(cuda_device):
    """An image's maps are bit-identical alone and inside a batch, call to call, and under capture and replay."""
    t, _ = golden()
    dev = cuda_device
    nd = N.NativeDetector(t["blob"].numpy(), dev)
    images = t["images"].to(dev)
    score, ori = (x.clone() for x in nd.forward(images))
    s2, o2 = nd.forward(images)
    assert torch.equal(s2, score) and torch.equal(o2, ori)
    for b in range(images.shape[0]):
        s1, o1 = nd.forward(images[b:b + 1])
        assert torch.equal(s1[0], score[b]) and torch.equal(o1[0], ori[b]), b
    rev = images.flip(0).contiguous()
    s3, o3 = nd.forward(rev)
    assert torch.equal(s3.flip(0), score) and torch.equal(o3.flip(0), ori)
    static = torch.zeros_like(images)
    out_s, out_o = torch.empty_like(score), torch.empty_like(ori)
    ws = torch.empty(nd.workspace_bytes(*score.shape), dtype=torch.uint8, device=dev)
    nd.forward(static, score=out_s, ori=out_o, workspace=ws)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            nd.forward(static, score=out_s, ori=out_o, workspace=ws)
    static.copy_(images)
    for _ in range(2):
        out_s.zero_()
        out_o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, score) and torch.equal(out_o, ori)


# ---- selection ------------------------------------------------------------------------------------------
def bits(x):
    return x.contiguous().view(torch.int32)


def check_select(dev, score, border, thresh, nk, K, gk, gs, scale_map=None, ori_map=None):
    """hn_select_keypoints against the torch restatement (C ABI blur order): everything bit for bit."""
    to = lambda x: x.to(dev) if x is not None else None  # noqa: E731
    got = N.select_keypoints(to(score), border, thresh, nk, K, gk, gs, scale_map=to(scale_map), scale_value=32.0,
                             ori_map=to(ori_map), dense=True)
    kpts, kscore, kscale, kori, q, mask, _ = D.select_keypoints_torch(score, border, thresh, nk, K, gk, gs,
                                                                      scale_map=scale_map, scale_value=32.0,
                                                                      ori_map=ori_map, abi_blur=True)
    assert tuple(got["kpts"].shape) == (score.shape[0] * K, 4)
    assert torch.equal(got["topk_mask"].cpu(), mask)
    assert torch.equal(bits(got["score_proc"].cpu()), bits(q))
    assert torch.equal(got["kpts"].cpu(), kpts)
    assert torch.equal(bits(got["kscore"].cpu()), bits(kscore)) and torch.equal(got["kscale"].cpu(), kscale)
    if ori_map is not None:
        assert torch.equal(got["kori"].cpu(), kori)
    return got, kpts


def test_select_golden(cuda_device):
    t, m = golden()
    a = m["det_args"]
    dev = cuda_device
    got = N.select_keypoints(t["score32"].to(dev), m["border"], a["nms_thresh"], a["nms_ksize"], a["topk"],
                             a["gauss_ksize"], a["gauss_sigma"], scale_value=m["scale"], ori_map=t["ori32"].to(dev),
                             dense=True)
    assert torch.equal(got["kpts"].cpu(), t["kpts"])
    assert torch.equal(got["kscore"].cpu(), t["kscore"]) and torch.equal(got["kscale"].cpu(), t["kscale"])
    assert torch.equal(got["kori"].cpu(), t["kori"]) and torch.equal(got["topk_mask"].cpu(), t["proc_mask"])
    d = float((got["score_proc"].cpu() - t["proc_score"]).abs().max())
    print(f"processed score vs the reference's: {d:.3e} (bound 1e-6)")
    assert d <= 1e-6
    # a scale map instead of the constant, no orientation
    smap = torch.rand(t["score32"].shape, generator=torch.Generator().manual_seed(3))
    g2 = N.select_keypoints(t["score32"].to(dev), m["border"], a["nms_thresh"], a["nms_ksize"], a["topk"],
                            a["gauss_ksize"], a["gauss_sigma"], scale_map=smap.to(dev))
    k = t["kpts"]
    assert g2["kori"] is None and torch.equal(g2["kscale"].cpu(), smap[k[:, 0], k[:, 1], k[:, 2]])
    # RFDet.process on a HIP tensor returns the dense outputs
    with torch.no_grad():
        p, pm, pv = golden_detector().process(t["score32"].to(dev).unsqueeze(-1))
    assert torch.equal(p.squeeze(-1), got["score_proc"]) and torch.equal(pm.squeeze(-1), got["topk_mask"])
    assert torch.equal(pv.squeeze(-1).cpu(), t["proc_value"])


def peaks_map(H=61, W=83):
    """Isolated peaks 15 apart (no pixel of a 15 x 15 blur sees two): A three distinct strong ones, B six equal,
    C six equal and weaker than A's blurred neighbours (0.135 x 0.9 > 0.05)."""
    s = torch.zeros(1, H, W)
    pos = [(y, x) for y in (10, 25, 40) for x in (10, 25, 40, 55, 70)]
    vals = [0.5, 0.05, 0.9, 0.5, 0.05, 0.05, 0.8, 0.5, 0.05, 0.5, 0.7, 0.05, 0.5, 0.05, 0.5]
    for (y, x), v in zip(pos, vals):
        s[0, y, x] = v
    return s


def test_select_fewer_than_k_survivors(cuda_device):
    got, kpts = check_select(cuda_device, peaks_map(), 8, 0.0, 5, 64, 15, 0.0)
    # sigma 0: the 15 peaks are the only positive pixels; the other 49 places go to the zeros of lowest index
    assert kpts[:49, 1:3].tolist() == [[0, x] for x in range(49)] and int((got["kscore"] > 0).sum()) == 15
    got, kpts = check_select(cuda_device, peaks_map(), 8, 0.0, 5, 64, 3, 0.1)
    # the blur reaches the 8 neighbours only: 15 x 9 = 135 positive pixels, of which the peaks and their 4-neighbours
    assert int((got["kscore"] > 0).sum()) == 15


@pytest.mark.parametrize("K", [11, 12, 13, 5])
def test_select_ties_straddling_the_cut(K, cuda_device):
    """K = 11: the first cut falls inside the six equal C peaks; K = 12: the second cut falls inside the four equal
    neighbours of the strongest peak as well; K = 13: on a group's edge; K = 5: inside the B plateau."""
    got, kpts = check_select(cuda_device, peaks_map(), 8, 0.0, 5, K, 15, 0.5)
    if K == 12:
        rows = kpts[:, 1:3].tolist()
        assert [9, 40] in rows and [10, 39] in rows and [10, 41] in rows and [11, 40] not in rows


def test_select_plateaus_and_duplicates(cuda_device):
    """2 x 2 and 1 x 3 plateaus survive NMS whole (t >= max); duplicated values elsewhere; sigma 0 keeps the maps
    apart from the blur, 0.5 adds it (overlapping windows: the blurred map is still compared bit for bit)."""
    s = torch.zeros(2, 40, 50)
    s[0, 10:12, 10:12] = 0.6
    s[0, 20, 20:23] = 0.6
    s[0, 30, 30] = s[0, 30, 40] = s[1, 9, 9] = s[1, 30, 41] = 0.6
    s[1, 15:17, 15:17] = 0.25
    s[1, 25, 25] = 0.7
    for K in (1, 3, 5, 8, 10):
        check_select(cuda_device, s, 8, 0.0, 5, K, 15, 0.0)
        check_select(cuda_device, s, 8, 0.0, 5, K, 15, 0.5)
        check_select(cuda_device, s, 8, 0.0, 3, K, 5, 1.0)


def test_select_first_interior_row_and_column(cuda_device):
    s = torch.zeros(1, 33, 40)
    s[0, 8, 8], s[0, 7, 20], s[0, 24, 31], s[0, 20, 7], s[0, 8, 30] = 0.9, 1.0, 0.8, 1.0, 0.3
    got, kpts = check_select(cuda_device, s, 8, 0.0, 5, 3, 15, 0.5)
    assert kpts[:, 1:3].tolist() == [[8, 8], [8, 30], [24, 31]]  # border pixels never count


@pytest.mark.parametrize("K", [1, 17 * 19])
def test_select_k_extremes(K, cuda_device):
    s = torch.rand(2, 17, 19, generator=torch.Generator().manual_seed(K))
    got, kpts = check_select(cuda_device, s, 8, 0.0, 5, K, 15, 0.5)
    if K == 17 * 19:
        assert torch.equal(kpts[:K, 1] * 19 + kpts[:K, 2], torch.arange(K))


def test_select_nan_threshold_and_negative_scores(cuda_device):
    g = torch.Generator().manual_seed(9)
    s = torch.rand(3, 33, 40, generator=g)
    s[torch.rand(s.shape, generator=g) < 0.05] = float("nan")
    s[0, 16, 20] = float("nan")
    ori = torch.rand(3, 33, 40, 2, generator=g)
    smap = torch.rand(3, 33, 40, generator=g)
    check_select(cuda_device, s, 8, 0.0, 5, 40, 15, 0.5, scale_map=smap, ori_map=ori)
    check_select(cuda_device, s, 8, 0.6, 5, 40, 7, 0.8, ori_map=ori)      # a threshold that removes most of the map
    check_select(cuda_device, s - 0.5, 8, -0.2, 3, 40, 3, 0.5)             # negative scores and threshold
    check_select(cuda_device, s, 0, 0.0, 15, 40, 15, 2.0)                  # no border, the widest windows


def test_select_stress(cuda_device):
    g = torch.Generator().manual_seed(21)
    s = torch.rand(8, 97, 131, generator=g)
    ori = torch.rand(8, 97, 131, 2, generator=g)
    check_select(cuda_device, s, 8, 0.0, 5, 512, 15, 0.5, ori_map=ori)


def test_select_memory_safety(cuda_device):
    """Canaries around every output and the workspace; a workspace poisoned with NaN gives the same results (no
    byte of it is read before it is written)."""
    dev = cuda_device
    lib = N.load_library()
    B, H, W, K = 3, 61, 83, 48
    t, m = golden()
    a = m["det_args"]
    score, ori = t["score32"].to(dev), t["ori32"].to(dev)
    need = N.select_workspace_bytes(B, H, W, K)
    pad = 4096
    canary = 0x5A

    def guarded(nbytes, fill):
        buf = torch.full((nbytes + 2 * pad,), canary, dtype=torch.uint8, device=dev)
        buf[pad:pad + nbytes] = fill
        return buf

    sizes = {"kpts": B * K * 32, "kscore": B * K * 4, "kscale": B * K * 4, "kori": B * K * 8, "proc": B * H * W * 4,
             "mask": B * H * W, "ws": need}
    results = []
    for poison in (0x00, 0xFF):  # 0xFF bytes are NaN as floats
        bufs = {k: guarded(n, poison if k == "ws" else 0) for k, n in sizes.items()}
        p = {k: b.data_ptr() + pad for k, b in bufs.items()}
        assert p["ws"] % 16 == 0
        rc = lib.hn_select_keypoints(score.data_ptr(), B, H, W, m["border"], a["nms_thresh"], a["nms_ksize"], K,
                                     a["gauss_ksize"], a["gauss_sigma"], None, m["scale"], ori.data_ptr(), p["kpts"],
                                     p["kscore"], p["kscale"], p["kori"], p["proc"], p["mask"], p["ws"], need,
                                     torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, lib.hn_last_error()
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert bool((b[:pad] == canary).all()) and bool((b[pad + sizes[k]:] == canary).all()), k
        results.append({k: b[pad:pad + sizes[k]].clone() for k, b in bufs.items() if k != "ws"})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    assert torch.equal(results[0]["kpts"].view(torch.int64).view(B * K, 4).cpu(), t["kpts"])
    # a short workspace is refused
    rc = lib.hn_select_keypoints(score.data_ptr(), B, H, W, 8, 0.0, 5, K, 15, 0.5, None, 32.0, None, p["kpts"],
                                 p["kscore"], p["kscale"], None, None, None, p["ws"], need - 1, None)
    assert rc == 4 and b"workspace" in lib.hn_last_error()


# ---- pipeline -------------------------------------------------------------------------------------------
def test_detect_is_forward_plus_select(cuda_device):
    t, m = golden()
    dev = cuda_device
    a = m["det_args"]
    det = golden_detector().to(dev)
    images = t["images"].to(dev)
    with torch.no_grad():
        kpts, kscale, kori, kscore, im_scale = D.detect(det, images)
    nd = N.NativeDetector(t["blob"].numpy(), dev)
    score, ori = nd.forward(images)
    got = N.select_keypoints(score, m["border"], a["nms_thresh"], a["nms_ksize"], a["topk"], a["gauss_ksize"],
                             a["gauss_sigma"], scale_value=m["scale"], ori_map=ori)
    assert torch.equal(kpts, got["kpts"]) and torch.equal(kscore, got["kscore"])
    assert torch.equal(kscale, got["kscale"]) and torch.equal(kori, got["kori"])
    assert tuple(im_scale.shape) == (m["B"], m["H"], m["W"], 1) and float(im_scale.min()) == m["scale"]
    # every stable reference keypoint is among the returned ones
    have = {tuple(r) for r in kpts[:, :3].cpu().tolist()}
    stable = t["kpts"][t["stable"]][:, :3].tolist()
    missing = [r for r in stable if tuple(r) not in have]
    print(f"stable reference keypoints: {len(stable)} of {t['kpts'].shape[0]}, missing {len(missing)}")
    assert not missing


@lru_cache(maxsize=None)
def _descriptor(name):
    torch.manual_seed(5)
    return (HardNetNeiMask("NASNet") if name == "fdl_NASNet" else HardNet()).eval()


@pytest.mark.parametrize("name", ["fdl_NASNet", "hardnet"])
def test_detect_and_describe(name, cuda_device):
    t, m = golden()
    dev = cuda_device
    det = golden_detector().to(dev)
    des = _descriptor(name).to(dev)
    images = t["images"].to(dev)
    im_info = torch.ones(m["B"], 2, device=dev)
    with torch.no_grad():
        im_scale, kpts, im_des, scale, ori, score = D.detect_and_describe(det, des, images, im_info, images)
        k2, s2, o2, sc2, _ = D.detect(det, images)
        want = PT.describe_keypoints(des, k2, s2, o2, im_info, images)
    assert tuple(im_des.shape) == (m["B"] * m["K"], 128) and bool(torch.isfinite(im_des).all())
    assert torch.equal(kpts, k2) and torch.equal(scale, s2) and torch.equal(ori, o2) and torch.equal(score, sc2)
    assert torch.equal(im_des, want)
