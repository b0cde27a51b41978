"""RF-Net's ten-scale detector on the MI355X: hn_rfdet_forward (hn_rfdet.hip) through ``NativeRFDetector`` and the
``RFDetSO`` module against the reference fixture tests/golden/rfdet.npz and against the torch module in fp64; its
chain into keypoint selection and the descriptors; ``RFDes`` on the HardNet kernels; ``Network``'s guard.

The comparison rule everywhere: |GPU - fp64| <= 4 E, where E is the error of an fp32 evaluation by torch on the CPU
against the same fp64 (the fixture's E_score / E_scale / E_ori for its images; computed here per shape for the
others) and 4 the project's margin for another fp32 evaluation order.  Orientations are compared where none of the
ten per-level pre-division norms nor the final one is below 0.05 in fp64 (the division amplifies any error without
bound there); that excluded share is asserted <= 1 %.  Every figure is printed before it is asserted."""
import copy

import numpy as np
import pytest
import torch

import rfdet_ref as R
from fixtures import build_module, golden_inputs
from hardnetnas_amd import _native as N
from hardnetnas_amd import detector as D
from hardnetnas_amd.model import HardNetNeiMask, RFDes
from hardnetnas_amd.network import ENDPOINT_KEYS, Network
from hardnetnas_amd.patches import describe_keypoints

pytestmark = pytest.mark.gpu
M = R.MARGIN
_FX = {}


def fixture():
    if not _FX:
        _FX["fx"] = R.load_fixture()
    return _FX["fx"]


def native(det, dev):
    return N.NativeRFDetector(N.state_dict_blob(det.state_dict()), det.scale_list.numpy(), dev,
                              in_eps=det.insnorm1.eps, score_com_strength=det.score_com_strength,
                              scale_com_strength=det.scale_com_strength)


def errors(tag, got, s64, c64, o64, excluded):
    """max |GPU - fp64| of the three maps (orientation on the non-excluded pixels), printed."""
    score, scale, ori = (t.double().cpu() for t in got)
    keep = ~excluded
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(scale).all())
    assert bool(torch.isfinite(ori[keep]).all())
    d = ((score - s64).abs().max().item(), (scale - c64).abs().max().item(),
         (ori - o64).abs().amax(dim=-1)[keep].max().item())
    print(f"{tag}: |gpu - fp64| score {d[0]:.3e} scale {d[1]:.3e} ori {d[2]:.3e}; "
          f"excluded {excluded.double().mean().item():.4%}")
    return d


def test_golden(cuda_device):
    """The fixture's images: the three maps within 4 E of the stored fp64; the module on the device returns the
    same bits as NativeRFDetector, in the reference's shapes."""
    fx, dev = fixture(), cuda_device
    m = fx["meta"]
    det = R.fixture_detector(fx)
    images = torch.from_numpy(fx["images"])
    nd = native(det, dev)
    got = nd.forward(images.to(dev))
    s64 = torch.from_numpy(fx["score32"].astype(np.float64) + fx["score64_minus_score32"])
    c64 = torch.from_numpy(fx["scale32"].astype(np.float64) + fx["scale64_minus_scale32"])
    o64 = torch.from_numpy(fx["ori32"].astype(np.float64) + fx["ori64_minus_ori32"])
    d = errors("golden", got, s64, c64, o64, torch.from_numpy(fx["ori_excluded"]))
    print(f"golden: E_score {m['E_score']:.3e} E_scale {m['E_scale']:.3e} E_ori {m['E_ori']:.3e}")
    assert d[0] <= M * m["E_score"] and d[1] <= M * m["E_scale"] and d[2] <= M * m["E_ori"]
    det = det.to(dev)
    with torch.no_grad():
        score, scale, ori = det(images.to(dev))
    B, H, W = m["B"], m["H"], m["W"]
    assert tuple(score.shape) == (B, H, W, 1) and tuple(scale.shape) == (B, H, W, 1)
    assert tuple(ori.shape) == (B, H, W, 1, 2)
    assert torch.equal(score.squeeze(-1), got[0]) and torch.equal(scale.squeeze(-1), got[1])
    assert torch.equal(ori.squeeze(-2), got[2])
    assert got[1].std().item() > 0.5  # a real scale map


T, T2 = 16, 32  # the layer kernels' tile and the tail kernel's
SHAPES = [(2, 1, 2), (1, 5, 7), (1, 17, 17), (1, 240, 320),
          (2, T - 1, T + 1), (1, T, T), (2, 2 * T + 1, 3 * T - 1), (2, 97, 131),
          (2, T2 - 1, T2 + 1), (1, T2, T2), (2, 2 * T2 + 1, 3 * T2 - 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_shapes(cuda_device, shape):
    """Seeded weights and uniform-noise images at the smallest legal image, images smaller than the tail's halo and
    the border, the training shape, and one below / at / several times the tile of the layer kernels (16) and of the
    tail kernel (32): 4 E with E the fp32 torch module's own error against its fp64 form on those inputs."""
    B, H, W = shape
    seed = 100 + 7 * H + W
    det = R.random_rfdet(seed)
    images = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(seed + 1))
    s64, c64, o64, excluded, e_score, e_scale, e_ori = R.reference_errors(det, images)
    print(f"{shape}: E_score {e_score:.3e} E_scale {e_scale:.3e} E_ori {e_ori:.3e}")
    assert excluded.double().mean().item() <= 0.01
    got = native(det, cuda_device).forward(images.to(cuda_device))
    d = errors(str(shape), got, s64, c64, o64, excluded)
    assert d[0] <= M * e_score and d[1] <= M * e_scale and d[2] <= M * e_ori


def test_forward_batch_independence_and_graph(cuda_device):
    """An image's maps are bit-identical alone and inside a batch, call to call, and under capture and replay."""
    fx, dev = fixture(), cuda_device
    nd = native(R.fixture_detector(fx), dev)
    images = torch.from_numpy(fx["images"]).to(dev)
    ref = [x.clone() for x in nd.forward(images)]
    assert all(torch.equal(a, b) for a, b in zip(nd.forward(images), ref))
    for b in range(images.shape[0]):
        one = nd.forward(images[b:b + 1])
        assert all(torch.equal(a[0], r[b]) for a, r in zip(one, ref)), b
    rev = nd.forward(images.flip(0).contiguous())
    assert all(torch.equal(a.flip(0), r) for a, r in zip(rev, ref))
    static = torch.zeros_like(images)
    outs = [torch.empty_like(r) for r in ref]
    ws = torch.empty(nd.workspace_bytes(*ref[0].shape), dtype=torch.uint8, device=dev)
    nd.forward(static, *outs, workspace=ws)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            nd.forward(static, *outs, workspace=ws)
    static.copy_(images)
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, r) for a, r in zip(outs, ref))


def test_memory_safety(cuda_device):
    """Canaries around the three outputs and the workspace survive; a workspace poisoned with 0x00 and with 0xFF
    gives identical outputs (no byte is read before the call writes it); workspace_bytes - 1 is refused."""
    fx, dev = fixture(), cuda_device
    nd = native(R.fixture_detector(fx), dev)
    images = torch.from_numpy(fx["images"]).to(dev)
    B, _, H, W = images.shape
    ref = [x.clone() for x in nd.forward(images)]
    need = nd.workspace_bytes(B, H, W)
    PAD = 4096
    outs = []
    for fill in (0x00, 0xFF):
        raw = [torch.full((PAD + r.numel() * 4 + PAD,), 0xA5, dtype=torch.uint8, device=dev) for r in ref]
        views = [b[PAD:PAD + r.numel() * 4].view(torch.float32).view(r.shape) for b, r in zip(raw, ref)]
        wsb = torch.full((PAD + need + PAD,), 0xA5, dtype=torch.uint8, device=dev)
        wsb[PAD:PAD + need] = fill
        nd.forward(images, *views, workspace=wsb[PAD:PAD + need])
        torch.cuda.synchronize()
        for b, r in zip(raw + [wsb], ref + [None]):
            n = need if r is None else r.numel() * 4
            assert bool((b[:PAD] == 0xA5).all()) and bool((b[PAD + n:] == 0xA5).all())
        assert all(torch.equal(v, r) for v, r in zip(views, ref)), fill
        outs.append(views)
    short = torch.empty(need - 1 + 16, dtype=torch.uint8, device=dev)[:need - 1]
    with pytest.raises(RuntimeError, match="workspace too small"):
        nd.forward(images, workspace=short)


@pytest.mark.parametrize("value", [0.0, 0.5])
def test_constant_image(cuda_device, value):
    """A constant image: level 1's InstanceNorm sees zero variance in all 16 channels for the zero image (pre_1 is
    the bias everywhere) and the deeper ones only what the zero padding at the border puts in.  Rule: the GPU maps
    are finite wherever the fp32 torch module's are, and at every pixel where the fp32 torch module itself agrees
    with its fp64 form within E (the fixture's E_score / E_scale / E_ori: the reference's error on ordinary images)
    the GPU agrees with the fp64 form within 4 E.  The share of compared pixels is printed and must be >= 50 %."""
    m = fixture()["meta"]
    det = R.random_rfdet(77)
    images = torch.full((1, 1, 40, 52), value)
    det64 = copy.deepcopy(det).double()
    det64.scale_list = det64.scale_list.double()
    with torch.no_grad():
        t32 = [t.reshape(1, 40, 52, -1) for t in det(images)]
        t64 = [t.reshape(1, 40, 52, -1) for t in det64(images.double())]
        excluded = R.ori_min_norm(det64, images.double()) < R.NORM_FLOOR
    got = [t.reshape(1, 40, 52, -1).cpu() for t in native(det, cuda_device).forward(images.to(cuda_device))]
    for name, g, a, b, e in zip(("score", "scale", "ori"), got, t32, t64, (m["E_score"], m["E_scale"], m["E_ori"])):
        fin = torch.isfinite(a).all(dim=-1)
        assert bool(torch.isfinite(g)[fin].all()), name
        agree = ((a.double() - b).abs().amax(dim=-1) <= e) & fin
        if name == "ori":
            agree &= ~excluded
        d = (g.double() - b).abs().amax(dim=-1)
        worst = d[agree].max().item() if agree.any() else 0.0
        print(f"constant {value} {name}: compared {agree.double().mean().item():.2%} of the pixels, "
              f"max |gpu - fp64| {worst:.3e} (4 E = {M * e:.3e})")
        assert agree.double().mean().item() >= 0.5 and worst <= M * e, name


def test_detect_is_forward_plus_select(cuda_device):
    fx, dev = fixture(), cuda_device
    det = R.fixture_detector(fx).to(dev)
    images = torch.from_numpy(fx["images"]).to(dev)
    with torch.no_grad():
        kpts, kscale, kori, kscore, im_scale = D.detect(det, images)
    score, scale, ori = native(R.fixture_detector(fx), dev).forward(images)
    out = N.select_keypoints(score, *det._select_args(), scale_map=scale, ori_map=ori)
    assert torch.equal(kpts, out["kpts"]) and torch.equal(kscale, out["kscale"])
    assert torch.equal(kori, out["kori"]) and torch.equal(kscore, out["kscore"])
    assert torch.equal(im_scale.squeeze(-1), scale)
    b, y, x = kpts[:, 0], kpts[:, 1], kpts[:, 2]
    assert torch.equal(kscale, scale[b, y, x]) and torch.equal(kori, ori[b, y, x])
    assert kscale.unique().numel() >= 5  # a constant-scale bug cannot pass
    got = {tuple(r) for r in kpts[:, :3].tolist()}
    stable = fx["kpts"][fx["stable"], :3].tolist()
    assert len(stable) >= 0.9 * len(fx["kpts"]) and all(tuple(r) in got for r in stable)


@pytest.mark.parametrize("which", ["RFDes", "HardNetNeiMask"])
def test_detect_and_describe(cuda_device, which):
    fx, dev = fixture(), cuda_device
    det = R.fixture_detector(fx).to(dev)
    torch.manual_seed(11)
    des = (RFDes(1.0, 1.0) if which == "RFDes" else HardNetNeiMask(1.0, 1.0, "NASNet")).eval().to(dev)
    images = torch.from_numpy(fx["images"]).to(dev)
    info = torch.ones(images.shape[0], 2, device=dev)
    with torch.no_grad():
        im_scale, kpts, im_des, kscale, kori, kscore = D.detect_and_describe(det, des, images, info, images)
        k2, s2, o2, c2, _ = D.detect(det, images)
        want = describe_keypoints(des, k2, s2, o2, info, images)
    n = fx["meta"]["B"] * fx["meta"]["K"]
    assert tuple(im_des.shape) == (n, 128) and bool(torch.isfinite(im_des).all())
    assert torch.equal(kpts, k2) and torch.equal(kscale, s2) and torch.equal(kori, o2) and torch.equal(kscore, c2)
    assert torch.equal(im_des, want)
    assert tuple(im_scale.shape) == (*images.shape[:1], *images.shape[2:], 1)


def test_rfdes_native(cuda_device):
    """RFDes in eval mode runs the stock HardNet kernels (hardnet_desc(1e-8, 0.0)): 256 synthetic patches against
    its torch layers in fp64, max abs <= 1e-4 (the HardNet bar)."""
    hn, hfx, _ = build_module("hardnet")
    des = RFDes(1.0, 1.0)
    des.load_state_dict(dict(zip(des.state_dict(), hn.state_dict().values())), strict=True)
    des = des.eval()
    x = torch.from_numpy(golden_inputs(hfx)[:256])
    with torch.no_grad():
        ref = copy.deepcopy(des).double()(x.double())
        got = des.to(cuda_device)(x.to(cuda_device))
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"RFDes native vs fp64 torch layers: max abs {err:.3e}")
    assert tuple(got.shape) == (256, 128) and err <= 1e-4
    assert N._BY_ID[des._native_handle(x.to(cuda_device))].desc.l2_eps == 0.0


def test_network_guard(cuda_device):
    """Network with RFDetSO never takes the native path (its ground-truth stage passes one constant scale); forward
    takes the reference-order path, which carries the scale and orientation maps."""
    dev = cuda_device
    torch.manual_seed(5)
    net = Network(R.random_rfdet(5), RFDes(1.0, 1.0), 1.0, 1.0, 32, R.K).eval().to(dev)
    img = torch.rand(1, 1, 61, 83, generator=torch.Generator().manual_seed(6)).to(dev)
    info = torch.ones(1, 2, device=dev)
    eye = torch.eye(3, device=dev).unsqueeze(0)
    batch = (img, info, eye, img.clone(), info, eye.clone(), img, img.clone())
    assert net._native_ok(batch) is False
    with torch.no_grad():
        end = net(batch)
    assert sorted(end) == sorted(ENDPOINT_KEYS)
    for k in ENDPOINT_KEYS:
        v = end[k]
        assert not v.is_floating_point() or bool(torch.isfinite(v).all()), k
