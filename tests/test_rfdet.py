"""RF-Net's detector without a GPU: the fixture tests/golden/rfdet.npz (made from the reference by
tests/golden/make_rfdet_golden.py) and its conditions, the torch ``RFDetSO`` and ``RFDes`` against it, the extension
header include/hardnet_mi355x_rfdet.h against the binding's table, and every argument check of the five functions.

The host-side sweep of the kernels' address arithmetic is ``make -C hardnetnas_amd/csrc rfdet_check`` (built with the
address and undefined-behaviour sanitizers; about a minute); it is not a pytest test."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rfdet_ref as R
from hardnetnas_amd import _native as N
from hardnetnas_amd import detector as D
from hardnetnas_amd.model import HardNet, RFDes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu_only = pytest.mark.skipif(torch.cuda.is_available(),
                                 reason="placeholder device pointers: runs on machines without a GPU only")


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


# ---- the fixture ----------------------------------------------------------------------------------------------
def test_fixture_conditions(fx):
    m = fx["meta"]
    B, H, W, K = m["B"], m["H"], m["W"], m["K"]
    assert (B, H, W) == (3, 61, 83) and fx["images"].shape == (B, 1, H, W)
    assert fx["blob"].shape == (N.RFDET_PARAM_FLOATS,) and len(m["state_dict_keys"]) == 100
    assert 0 < m["E_score"] < 1e-4 and 0 < m["E_scale"] < 1e-2 and 0 < m["E_ori"] < 1e-3
    e_score = np.abs(fx["score64_minus_score32"]).max()
    e_scale = np.abs(fx["scale64_minus_scale32"]).max()
    assert abs(e_score - m["E_score"]) < 1e-9 and abs(e_scale - m["E_scale"]) < 1e-8
    ex = fx["ori_excluded"]
    assert ex.shape == (B, H, W) and ex.mean() <= 0.01 and abs(ex.mean() - m["ori_excluded_share"]) < 1e-12
    d = np.abs(fx["ori64_minus_ori32"]).max(axis=-1)
    assert abs(d[~ex].max() - m["E_ori"]) < 1e-9
    assert min(m["nms_survivors"]) >= K and all((fx["proc_value"][b] > 0).sum() >= K for b in range(B))
    assert m["kth_gap_first"] > 1e-5 and m["kth_gap_second"] > 1e-5
    assert fx["kpts"].shape == (B * K, 4) and fx["kpts"].dtype == np.int64
    assert len(np.unique(fx["kscale"])) >= 5 and m["distinct_keypoint_scales"] == len(np.unique(fx["kscale"]))
    assert m["stable_share"] >= 0.9 and fx["stable"].mean() >= 0.9
    # a real scale map: it spans the levels
    assert fx["scale32"].min() >= 3.0 and fx["scale32"].max() <= 21.0 and fx["scale32"].std() > 0.5
    # the keypoints' scale, orientation and score are the maps' values at them
    b, y, x = fx["kpts"][:, 0], fx["kpts"][:, 1], fx["kpts"][:, 2]
    assert np.array_equal(fx["kscale"], fx["scale32"][b, y, x]) and np.array_equal(fx["kori"], fx["ori32"][b, y, x])
    assert np.array_equal(fx["kscore"], fx["score32"][b, y, x])


# ---- the torch RFDetSO ----------------------------------------------------------------------------------------
def test_state_dict_is_the_references(fx):
    det = D.RFDetSO(**fx["meta"]["det_args"])
    assert list(det.state_dict()) == fx["meta"]["state_dict_keys"]
    assert N.state_dict_blob(R.fixture_detector(fx).state_dict()).tobytes() == fx["blob"].tobytes()
    assert det.scale_list.tolist() == R.SCALE_LIST and "scale_list" not in det.state_dict()
    for name in ("score_com_strength", "scale_com_strength", "NMS_THRESH", "NMS_KSIZE", "TOPK", "GAUSSIAN_KSIZE",
                 "GAUSSIAN_SIGMA"):
        assert hasattr(det, name)
    # shared with RFDet, not copied
    for name in ("process", "loss", "weights_init", "convO_init", "_select_args"):
        assert getattr(D.RFDetSO, name) is getattr(D.RFDet, name)


def test_torch_forward_fp32_within_2E_of_the_reference(fx):
    m = fx["meta"]
    det = R.fixture_detector(fx)
    with torch.no_grad():
        score, scale, ori = det(torch.from_numpy(fx["images"]))
    B, H, W = m["B"], m["H"], m["W"]
    assert tuple(score.shape) == (B, H, W, 1) and tuple(scale.shape) == (B, H, W, 1)
    assert tuple(ori.shape) == (B, H, W, 1, 2)
    assert np.abs(score.squeeze(-1).numpy() - fx["score32"]).max() <= 2 * m["E_score"]
    assert np.abs(scale.squeeze(-1).numpy() - fx["scale32"]).max() <= 2 * m["E_scale"]
    d = np.abs(ori.squeeze(-2).numpy() - fx["ori32"]).max(axis=-1)
    assert d[~fx["ori_excluded"]].max() <= 2 * m["E_ori"]


def test_torch_forward_fp64_is_the_stored_fp64(fx):
    det = R.fixture_detector(fx, torch.float64)
    x = torch.from_numpy(fx["images"]).double()
    with torch.no_grad():
        score, scale, ori = det(x)
        mn = R.ori_min_norm(det, x)
    s64 = fx["score32"].astype(np.float64) + fx["score64_minus_score32"]
    c64 = fx["scale32"].astype(np.float64) + fx["scale64_minus_scale32"]
    o64 = fx["ori32"].astype(np.float64) + fx["ori64_minus_ori32"]
    # the stored differences are rounded to fp32: 2^-24 of their size (the generator asserts the round trip)
    assert np.abs(score.squeeze(-1).numpy() - s64).max() < 1e-10
    assert np.abs(scale.squeeze(-1).numpy() - c64).max() < 1e-10
    d = np.abs(ori.squeeze(-2).numpy() - o64).max(axis=-1)
    assert d[~fx["ori_excluded"]].max() < 1e-10
    assert np.array_equal((mn < R.NORM_FLOOR).numpy(), fx["ori_excluded"])


def test_process_and_detect_on_the_cpu(fx):
    m = fx["meta"]
    det = R.fixture_detector(fx)
    with torch.no_grad():
        proc, mask, value = det.process(torch.from_numpy(fx["score32"]).unsqueeze(-1))
        kpts, kscale, kori, kscore, im_scale = D.detect(det, torch.from_numpy(fx["images"]))
    assert np.array_equal(mask.squeeze(-1).numpy(), fx["proc_mask"])
    assert np.array_equal(value.squeeze(-1).numpy(), fx["proc_value"])
    assert np.abs(proc.squeeze(-1).numpy() - fx["proc_score"]).max() < 1e-6
    got = {tuple(r) for r in kpts[:, :3].tolist()}
    assert all(tuple(r) in got for r in fx["kpts"][fx["stable"], :3].tolist())
    assert tuple(kpts.shape) == (m["B"] * m["K"], 4) and tuple(kori.shape) == (m["B"] * m["K"], 2)
    assert torch.equal(kscale, im_scale.squeeze(-1)[kpts[:, 0], kpts[:, 1], kpts[:, 2]])
    assert kscale.unique().numel() >= 5


def test_random_rfdet_is_seeded():
    a, b, c = R.random_rfdet(7), R.random_rfdet(7), R.random_rfdet(8)
    sa, sb, sc = (N.state_dict_blob(d.state_dict()) for d in (a, b, c))
    assert sa.tobytes() == sb.tobytes() and sa.tobytes() != sc.tobytes() and not a.training


# ---- RFDes ----------------------------------------------------------------------------------------------------
def test_rfdes_keys_and_forward(fx):
    des = RFDes(1.0, 1.0)
    assert list(des.state_dict()) == fx["meta"]["rfdes_state_dict_keys"]
    convs = [i for i, l in enumerate(des.features) if isinstance(l, torch.nn.Conv2d)]
    assert convs == [0, 3, 6, 9, 12, 15, 18] and des.input_norm_eps == 1e-8 and des.l2_eps == 0.0
    assert not any(isinstance(l, torch.nn.Dropout) for l in des.features)
    # HardNet's forward on the same weights, once eps and Dropout (identity in eval) are accounted for
    torch.manual_seed(3)
    hn = HardNet().eval()
    with torch.no_grad():
        for m in hn.features:
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    src = [v for k, v in hn.state_dict().items()]
    des.load_state_dict(dict(zip(des.state_dict(), src)), strict=True)
    des = des.eval()
    assert N.state_dict_blob(des.state_dict()).tobytes() == N.state_dict_blob(hn.state_dict()).tobytes()
    hn.input_norm_eps, hn.l2_eps = 1e-8, 0.0
    x = torch.rand(5, 1, 32, 32)
    with torch.no_grad():
        a, b = des(x), hn(x)
    assert float((a - b).abs().max()) <= 2e-7  # torch.norm against sqrt(sum(x * x) + 0): one rounding apart
    d = N.desc_for_module(des)
    assert d.kind == N.HN_KIND_HARDNET and d.input_norm_eps == np.float32(1e-8) and d.l2_eps == 0.0
    assert des.train().training and des(x).shape == (5, 128)


# ---- the extension header and the binding ---------------------------------------------------------------------
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _header():
    src = open(os.path.join(ROOT, "include", "hardnet_mi355x_rfdet.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_prototypes_agree_with_the_extension_header():
    decl, rets = {}, {}
    for ret, name, args in re.findall(r"^\s*(int|void)\s+(hn_\w+)\s*\(([^)]*)\)\s*;", _header(), re.M):
        params = [" ".join(a.split()) for a in args.split(",")]
        decl[name] = ["pointer" if "*" in a else SCALARS[a.replace("const ", "").split()[0]] for a in params]
        rets[name] = ret
    assert sorted(decl) == sorted(N.EXPORTED_RFDET) and len(decl) == 5
    assert not set(decl) & set(N.EXPORTED) and not set(decl) & set(N.EXPORTED_LOSS_REDUCE)
    main = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    assert '#include "hardnet_mi355x_rfdet.h"' in main  # one include gives a C caller the whole ABI
    lib = N.load_library()
    for name, params in decl.items():
        fn = getattr(lib, name)
        got = ["pointer" if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else t for t in fn.argtypes]
        assert got == params, name
        assert fn.restype is (ctypes.c_int if rets[name] == "int" else None), name
    assert rets == {**{n: "int" for n in decl}, "hn_rfdet_destroy": "void"}


P = 4096       # a device pointer that is never dereferenced
BIG = 1 << 50  # a workspace size that always suffices
ARG, WORKSPACE = 1, 4
FWD = dict(d=P, images=P, n=2, h=61, w=83, score=P, scale=P, ori=P, ws=P, ws_bytes=BIG, stream=None)


def _call(name, *args):
    lib = N.load_library()
    rc = getattr(lib, name)(*args)
    return rc, lib.hn_last_error().decode()


def _need(n, h, w):
    out = ctypes.c_size_t()
    assert N.load_library().hn_rfdet_workspace_bytes(n, h, w, ctypes.byref(out)) == 0
    return out.value


@no_gpu_only
def test_param_count_and_workspace_bytes():
    n = ctypes.c_size_t()
    assert _call("hn_rfdet_param_count", ctypes.byref(n))[0] == 0 and n.value == 21890 == N.RFDET_PARAM_FLOATS
    rc, msg = _call("hn_rfdet_param_count", None)
    assert rc == ARG and "n_out is NULL" in msg
    rc, msg = _call("hn_rfdet_workspace_bytes", 1, 8, 8, None)
    assert rc == ARG and "bytes_out is NULL" in msg
    for bad, text in (((-1, 8, 8), "n_images must be >= 0"), ((1, 1, 1), "at least 2 pixels"),
                      ((1, 0, 8), "at least 2 pixels"), ((1, 8, -1), "at least 2 pixels"),
                      ((1, 1 << 16, 1 << 16), "below 2^31"), ((1 << 31, 8, 8), "n_images * tiles")):
        rc, msg = _call("hn_rfdet_workspace_bytes", *bad, ctypes.byref(n))
        assert rc == ARG and text in msg, (bad, msg)
    # intermediates: two pre and two feat buffers of 16 channels, ten raw scores and ten unit orientations per pixel
    assert _need(1, 240, 320) >= 240 * 320 * 4 * (4 * 16 + 10 + 20)
    assert _need(1, 240, 320) <= 240 * 320 * 4 * (4 * 16 + 10 + 20) + (1 << 20)
    assert _need(0, 8, 8) % 16 == 0 and _need(3, 1, 2) > 0 and _need(2, 61, 83) < 2 * _need(1, 61, 83) + 64


@no_gpu_only
def test_create_checks():
    blob = np.zeros(21890, np.float32)
    scales = np.asarray(R.SCALE_LIST, np.float32)
    h = ctypes.c_void_p()

    def create(b=blob, n=None, s=scales, eps=1e-5, c1=100.0, c2=100.0, out=h):
        return _call("hn_rfdet_create", b.ctypes.data if b is not None else None, b.size if n is None else n,
                     s.ctypes.data if s is not None else None, eps, c1, c2, ctypes.byref(out) if out is not None else None)

    for kw in (dict(b=None, n=21890), dict(s=None), dict(out=None)):
        rc, msg = create(**kw)
        assert rc == ARG and "NULL argument" in msg
    for n in (21889, 21891):
        rc, msg = create(n=n)
        assert rc == ARG and f"host_params has {n} floats, expected 21890" in msg
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = create(eps=eps)
        assert rc == ARG and "in_eps must be > 0" in msg
    rc, msg = create(c1=float("inf"))
    assert rc == ARG and "must be finite" in msg
    bad = blob.copy()
    bad[21889] = np.nan
    rc, msg = create(b=bad)
    assert rc == ARG and "host_params holds a non-finite value" in msg
    bad_s = scales.copy()
    bad_s[9] = np.inf
    rc, msg = create(s=bad_s)
    assert rc == ARG and "scale_list holds a non-finite value" in msg
    assert not h.value
    N.load_library().hn_rfdet_destroy(None)  # NULL is a no-op


FORWARD_CHECKS = [
    ("n negative", dict(n=-1), ARG, "n_images must be >= 0"),
    ("one pixel", dict(h=1, w=1), ARG, "at least 2 pixels"),
    ("height 0", dict(h=0), ARG, "at least 2 pixels"),
    ("too many pixels", dict(h=1 << 16, w=1 << 16), ARG, "height * width must be below 2^31"),
    ("too many tiles", dict(n=1 << 31), ARG, "n_images * tiles must be below 2^31"),
    ("detector NULL", dict(d=None), ARG, "detector is NULL"),
    ("images NULL", dict(images=None), ARG, "NULL device pointer"),
    ("score NULL", dict(score=None), ARG, "NULL device pointer"),
    ("scale NULL", dict(scale=None), ARG, "NULL device pointer"),
    ("ori NULL", dict(ori=None), ARG, "NULL device pointer"),
    ("workspace NULL", dict(ws=None), ARG, "NULL device pointer"),
    ("ori misaligned", dict(ori=P + 4), ARG, "d_ori must be 8-byte and d_workspace 16-byte aligned"),
    ("workspace misaligned", dict(ws=P + 8), ARG, "d_ori must be 8-byte and d_workspace 16-byte aligned"),
    ("workspace short", dict(ws_bytes=None), WORKSPACE, "workspace too small: need "),
    ("workspace 0", dict(ws_bytes=0), WORKSPACE, "workspace too small: need "),
]


@no_gpu_only
@pytest.mark.parametrize("tag,mods,code,text", FORWARD_CHECKS, ids=[c[0] for c in FORWARD_CHECKS])
def test_forward_argument_checks(tag, mods, code, text):
    a = {**FWD, **mods}
    if a["ws_bytes"] is None:  # one byte short of the size query's answer
        a["ws_bytes"] = _need(a["n"], a["h"], a["w"]) - 1
    rc, msg = _call("hn_rfdet_forward", *a.values())
    assert rc == code and text in msg, (rc, msg)
    if tag == "workspace short":
        assert msg.endswith(f"need {_need(a['n'], a['h'], a['w'])} bytes")


@no_gpu_only
def test_forward_of_no_images_is_ok():
    # n_images == 0 returns HN_OK before any pointer is looked at (but after the shape checks and the handle's)
    assert _call("hn_rfdet_forward", *{**FWD, "n": 0, "images": None, "ws": None, "ws_bytes": 0}.values())[0] == 0
    rc, msg = _call("hn_rfdet_forward", *{**FWD, "n": 0, "d": None}.values())
    assert rc == ARG and "detector is NULL" in msg
    rc, msg = _call("hn_rfdet_forward", *{**FWD, "n": 0, "h": 1, "w": 1}.values())
    assert rc == ARG and "at least 2 pixels" in msg


def test_network_guard_on_the_cpu(monkeypatch):
    """A detector with more than one scale never takes Network's native path, whose ground-truth stage passes the
    one constant scale.  The detector's own check is stubbed to True, so the guard is what answers."""
    from hardnetnas_amd import network as NW
    calls = []

    def yes(self, photos):
        calls.append(type(self).__name__)
        return True
    monkeypatch.setattr(D.RFDetSO, "_native_ok", yes)
    monkeypatch.setattr(D.RFDet, "_native_ok", yes)
    img, info, eye = torch.rand(1, 1, 61, 83), torch.ones(1, 2), torch.eye(3).unsqueeze(0)
    batch = (img, info, eye, img, info, eye, img, img)
    assert NW.Network(R.random_rfdet(5), RFDes(1.0, 1.0), 1.0, 1.0, 32, R.K)._native_ok(batch) is False
    assert calls == []  # refused before the detector was asked
    # the one-scale detector gets past the guard: its own check is consulted (the CPU tensors refuse it later)
    one = NW.Network(D.RFDet(100.0, 100.0, 0.0, 5, R.K, 15, 0.5), RFDes(1.0, 1.0), 1.0, 1.0, 32, R.K)
    assert one._native_ok(batch) is False and calls == ["RFDet", "RFDet"]
