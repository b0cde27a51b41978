"""FDLNet's keypoint detector and keypoint selection without a GPU: the torch module and the torch selection of
hardnetnas_amd/detector.py against the reference's recorded outputs (tests/golden/detect.npz), and the C ABI's
argument checks, which all run before the GPU is touched.

Tolerances.  The torch module in fp32 is another fp32 evaluation of the reference's expression: within 2 E of the
reference's fp32 maps, E the reference's own fp32 error on these inputs (read from the fixture); in fp64 it must
reproduce the stored fp64 evaluation to 1e-10 (the relation clip_patch's torch formulation is held to).  The
selection is exact: the generator asserts that no top-K cut of the fixture falls inside a group of equal values,
where alone the tie rule could differ from torch.sort."""
import ctypes
import os

import pytest
import torch

from detect_ref import golden, golden_detector, state_dict_from_blob
from hardnetnas_amd import _native as N
from hardnetnas_amd import detector as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hn_det_param_count", "hn_det_create", "hn_det_workspace_bytes", "hn_det_forward",
               "hn_select_workspace_bytes", "hn_select_keypoints")


def test_fixture_conditions():
    t, m = golden()
    assert 0 < m["E_score"] < 1e-4 and m["ori_excluded_share"] <= 0.01 and m["stable_share"] >= 0.9
    assert min(m["nms_survivors"]) >= m["K"] and m["kth_gap_first"] > 1e-5 and m["kth_gap_second"] > 1e-5
    assert tuple(t["kpts"].shape) == (m["B"] * m["K"], 4) and len(m["state_dict_keys"]) == 40


def test_torch_module_loads_strict_and_reproduces_the_reference():
    t, m = golden()
    det = golden_detector()
    assert [k for k in det.state_dict() if not k.endswith("num_batches_tracked")] == m["state_dict_keys"]
    assert torch.equal(N_blob(det), t["blob"])
    keep = ~t["ori_excluded"]
    with torch.no_grad():
        score, scale, ori = det(t["images"])
        assert tuple(score.shape) == (m["B"], m["H"], m["W"], 1) and tuple(ori.shape) == (m["B"], m["H"], m["W"], 2)
        assert torch.equal(scale, torch.full_like(score, m["scale"]))
        e_s = float((score.squeeze(-1) - t["score32"]).abs().max())
        e_o = float((ori - t["ori32"]).abs().amax(-1)[keep].max())
        det64 = golden_detector().double()
        s64, sc64, o64 = det64(t["images"].double())
        d_s = float((s64.squeeze(-1) - t["score64"]).abs().max())
        d_o = float((o64 - t["ori64"]).abs().amax(-1)[keep].max())
    print(f"fp32 vs reference fp32: score {e_s:.3e} (2E {2 * m['E_score']:.3e}), ori {e_o:.3e} "
          f"(2E {2 * m['E_ori']:.3e}); fp64 vs stored fp64: score {d_s:.3e}, ori {d_o:.3e}")
    assert e_s <= 2 * m["E_score"] and e_o <= 2 * m["E_ori"]
    assert d_s <= 1e-10 and d_o <= 1e-10
    assert float((sc64 - m["scale"]).abs().max()) < 1e-6  # exp(0) / (1 + 1e-8) in fp64


def N_blob(det):
    return torch.from_numpy(N.state_dict_blob(det.state_dict()))


def test_torch_selection_returns_the_reference_keypoints():
    t, m = golden()
    a = m["det_args"]
    kpts, kscore, kscale, kori, q, mask, v = D.select_keypoints_torch(
        t["score32"], m["border"], a["nms_thresh"], a["nms_ksize"], a["topk"], a["gauss_ksize"], a["gauss_sigma"],
        scale_value=m["scale"], ori_map=t["ori32"])
    assert torch.equal(kpts, t["kpts"])
    assert torch.equal(mask, t["proc_mask"]) and torch.equal(v, t["proc_value"])
    assert torch.equal(kscore, t["kscore"]) and torch.equal(kscale, t["kscale"]) and torch.equal(kori, t["kori"])
    assert float((q - t["proc_score"]).abs().max()) <= 1e-6
    # the module's process and the helpers take the same path
    det = golden_detector()
    with torch.no_grad():
        p, pm, pv = det.process(t["score32"].unsqueeze(-1))
        assert torch.equal(p.squeeze(-1), q) and torch.equal(pm.squeeze(-1), mask) and torch.equal(pv.squeeze(-1), v)
        k2, s2, o2, sc2, im_scale = D.detect(det, t["images"])
    stable = t["stable"]
    got = {tuple(r) for r in k2[:, :3].tolist()}
    assert all(tuple(r) in got for r in t["kpts"][stable][:, :3].tolist())
    assert tuple(im_scale.shape) == (m["B"], m["H"], m["W"], 1)


def test_tie_rule_of_the_torch_selection():
    """Equal values are taken by lowest flat index at both steps; fewer than K positives are filled with zeros."""
    s = torch.zeros(1, 17, 19)
    s[0, 8, 8] = s[0, 8, 10] = 0.5   # NMS ksize 1: no suppression; two equal peaks, K = 1
    kpts, *_ , q, mask, v = D.select_keypoints_torch(s, 8, 0.0, 1, 1, 1, 0.0)
    assert kpts.tolist() == [[0, 8, 8, 0]] and int(mask.sum()) == 1 and mask[0, 8, 8] == 1
    kpts, *_ = D.select_keypoints_torch(s, 8, 0.0, 1, 4, 1, 0.0)
    assert kpts.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 8, 8, 0], [0, 8, 10, 0]]
    s[0, 8, 9] = float("nan")
    kpts, kscore, *_ = D.select_keypoints_torch(s, 8, 0.0, 1, 2, 1, 0.0)
    assert kpts.tolist() == [[0, 8, 8, 0], [0, 8, 10, 0]]


def test_exports_and_header():
    header = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    lib = N.load_library()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header and s in N.EXPORTED and hasattr(lib, s), s
        assert getattr(lib, s).restype is ctypes.c_int and getattr(lib, s).argtypes
    assert "void hn_det_destroy(" in header and "hn_det_destroy" in N.EXPORTED and lib.hn_det_destroy.restype is None
    assert "#define HN_ABI_VERSION 2" in header and lib.hn_abi_version() == 2
    import hardnetnas_amd as P
    for name in ("RFDet", "detect", "detect_and_describe", "select_keypoints_torch"):
        assert getattr(P, name) is getattr(D, name) and name in P.__all__
    assert hasattr(N, "NativeDetector") and hasattr(N, "select_keypoints")


def test_param_count_is_the_blob_length():
    t, _ = golden()
    n = ctypes.c_size_t()
    lib = N.load_library()
    assert lib.hn_det_param_count(ctypes.byref(n)) == 0 and n.value == t["blob"].numel() == 1193
    assert lib.hn_det_param_count(None) == 1 and b"NULL" in lib.hn_last_error()
    det = golden_detector()
    assert sum(v.numel() for k, v in det.state_dict().items() if not k.endswith("num_batches_tracked")) == n.value
    assert set(state_dict_from_blob(det, t["blob"])) == set(det.state_dict())


PTR = ctypes.c_void_p(4096)  # never dereferenced: every check runs before the GPU is touched
SEL_GOOD = dict(n_images=2, height=61, width=83, border=8, nms_thresh=0.0, nms_ksize=5, topk=64, gauss_ksize=15,
                gauss_sigma=0.5)


def _select(lib, **kw):
    a = dict(SEL_GOOD, **kw)
    kori = a.pop("kori", None)
    ori_map = a.pop("ori_map", None)
    return lib.hn_select_keypoints(PTR, a["n_images"], a["height"], a["width"], a["border"], a["nms_thresh"],
                                   a["nms_ksize"], a["topk"], a["gauss_ksize"], a["gauss_sigma"], None, 32.0, ori_map,
                                   PTR, PTR, PTR, kori, None, None, a.get("ws", PTR), a.get("ws_bytes", 1 << 40), None)


@pytest.mark.parametrize("kw,word", [
    (dict(topk=0), b"topk"), (dict(topk=61 * 83 + 1), b"topk"), (dict(n_images=-1), b"n_images"),
    (dict(height=16), b"border"), (dict(width=16), b"border"), (dict(border=-1), b"border"),
    (dict(height=0), b"height"), (dict(nms_ksize=4), b"nms_ksize"), (dict(nms_ksize=17), b"nms_ksize"),
    (dict(nms_ksize=0), b"nms_ksize"), (dict(gauss_ksize=6), b"gauss_ksize"), (dict(gauss_ksize=17), b"gauss_ksize"),
    (dict(gauss_sigma=-1.0), b"gauss_sigma"), (dict(gauss_sigma=float("nan")), b"gauss_sigma"),
    (dict(nms_thresh=float("nan")), b"nms_thresh"), (dict(kori=PTR), b"d_kori"), (dict(ori_map=PTR), b"d_kori"),
    (dict(ws=None), b"NULL"), (dict(ws=ctypes.c_void_p(4096 + 8)), b"16-byte"),
])
def test_select_rejects_bad_arguments_without_touching_gpu(kw, word):
    lib = N.load_library()
    assert _select(lib, **kw) == 1 and word in lib.hn_last_error(), lib.hn_last_error()


def test_select_workspace_and_empty_batch_without_touching_gpu():
    lib = N.load_library()
    n = ctypes.c_size_t()
    assert lib.hn_select_workspace_bytes(2, 61, 83, 64, ctypes.byref(n)) == 0 and n.value >= 3 * 2 * 61 * 83 * 4
    assert _select(lib, ws_bytes=n.value - 1) == 4 and b"workspace too small" in lib.hn_last_error()
    assert lib.hn_select_workspace_bytes(2, 61, 83, 0, ctypes.byref(n)) == 1 and b"topk" in lib.hn_last_error()
    assert lib.hn_select_workspace_bytes(2, 61, 83, 64, None) == 1
    assert lib.hn_select_workspace_bytes(2, 46341, 46341, 64, ctypes.byref(n)) == 1 and b"2^31" in lib.hn_last_error()
    # an empty batch is HN_OK whatever the pointers; a bad shape is still an error
    assert lib.hn_select_keypoints(None, 0, 61, 83, 8, 0.0, 5, 64, 15, 0.5, None, 32.0, None, None, None, None, None,
                                   None, None, None, 0, None) == 0
    assert lib.hn_select_keypoints(None, 0, 61, 83, 8, 0.0, 4, 64, 15, 0.5, None, 32.0, None, None, None, None, None,
                                   None, None, None, 0, None) == 1


def test_detector_rejects_bad_arguments_without_touching_gpu():
    lib = N.load_library()
    n = ctypes.c_size_t()
    assert lib.hn_det_workspace_bytes(2, 61, 83, ctypes.byref(n)) == 0 and n.value >= 3 * 2 * 61 * 83 * 4
    for args, word in (((-1, 61, 83), b"n_images"), ((2, 0, 83), b"height"), ((2, 1, 1), b"2 pixels"),
                       ((2, 46341, 46341), b"2^31"), ((1 << 40, 61, 83), b"2^31")):
        assert lib.hn_det_workspace_bytes(*args, ctypes.byref(n)) == 1 and word in lib.hn_last_error(), args
        assert lib.hn_det_forward(PTR, PTR, *args, PTR, PTR, PTR, 1 << 40, None) == 1 and word in lib.hn_last_error()
    assert lib.hn_det_workspace_bytes(2, 61, 83, None) == 1
    assert lib.hn_det_forward(None, PTR, 2, 61, 83, PTR, PTR, PTR, 1 << 40, None) == 1
    assert b"detector is NULL" in lib.hn_last_error()
    # hn_det_create's checks precede its allocation
    t, _ = golden()
    blob = t["blob"].numpy().copy()
    h = ctypes.c_void_p()
    assert lib.hn_det_create(blob.ctypes.data, blob.size - 1, 1e-5, 1e-5, ctypes.byref(h)) == 1
    assert b"expected 1193" in lib.hn_last_error() and not h.value
    assert lib.hn_det_create(None, blob.size, 1e-5, 1e-5, ctypes.byref(h)) == 1
    assert lib.hn_det_create(blob.ctypes.data, blob.size, 0.0, 1e-5, ctypes.byref(h)) == 1
    assert b"bn_eps" in lib.hn_last_error()
    bad = blob.copy()
    bad[200] = float("nan")
    assert lib.hn_det_create(bad.ctypes.data, bad.size, 1e-5, 1e-5, ctypes.byref(h)) == 1
    assert b"non-finite" in lib.hn_last_error()
    lib.hn_det_destroy(None)
