"""Generate tests/golden/gt.npz from the REFERENCE homography ground-truth stage and Network.forward.

Run from the repo root:  python tests/golden/make_gt_golden.py
Needs the reference tree (HN_REFERENCE, as make_golden.py; read-only, never copied).  The definitions are
AST-extracted at run time and executed on the CPU with ``torch`` in scope:
  warp, filtbordmask, filter_border, clip_patch (utils/image_utils.py); imgBatchXYZ, transXYZ_2_to_1
  (utils/common_utils.py); MSD, L2Norm, ptCltoCr, distance_matrix_vector, pairwise_distances (utils/math_utils.py);
  pair (utils/net_utils.py); Network.forward / gtscore / gt_scale_orin / criterion (model/network.py), called with a
  stand-in ``self``; HardNetNeiMask.loss (model/des.py); RFDet and what it needs (make_detect_golden.py's namespace).
For ``align_corners=True`` the namespace's ``torch.nn.functional.grid_sample`` is bound to
``functools.partial(F.grid_sample, align_corners=True)`` while warp runs; the function text stays the reference's.
The end-to-end part runs the reference detector on the weights of detect.npz; its descriptor is this package's
``HardNetNeiMask`` torch module on the weights of fdl_NASNet.npz (verified against the reference module by that
fixture) with the reference's ``loss`` bound to it.  The stand-in detector returns the reference detector's
orientation map as a contiguous tensor (the same values): the reference's ptCltoCr ``.view(-1)``s a chunk of it, which
on the detector's permuted view works for B = 1 only.

Only data is written: the inputs, the reference's fp32 outputs, an fp64 evaluation of each (fp64 inputs and
homographies; stored as fp32 differences as detect.npz does; ptCltoCr casts to fp32 internally, so its fp64 twin is a
hand projection), the reference's own error E = max |fp32 - fp64| of every continuous output, the exclusion masks of
tests/gt_helpers.py and JSON metadata.  The conditions asserted here are recorded in the metadata.
"""
from __future__ import annotations

import ast
import functools
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import gt_helpers as G  # noqa: E402
import make_detect_golden as D  # noqa: E402

SEED = 2041
B, H, W, K = 2, 61, 83, 48
BORDER = 8
PATCH_ROWS = 8  # patch pairs stored per image (the first rows)
WANTED = {
    "utils/image_utils.py": ("warp",),
    "utils/common_utils.py": ("imgBatchXYZ", "transXYZ_2_to_1"),
    "utils/math_utils.py": ("MSD", "ptCltoCr", "distance_matrix_vector", "pairwise_distances"),
    "utils/net_utils.py": ("pair",),
}


def reference_namespace():
    ns = D.reference_namespace()  # RFDet, filter_border, clip_patch, L2Norm, ...
    ns["np"] = np
    for rel, names in WANTED.items():
        tree = ast.parse(open(os.path.join(D.BASE, rel)).read())
        keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert len(keep) == len(names), (rel, [n.name for n in keep])
        exec(ast.unparse(ast.Module(body=keep, type_ignores=[])), ns)
    for rel, cls_name, methods in (("model/network.py", "Network", ("forward", "gtscore", "gt_scale_orin", "criterion")),
                                   ("model/des.py", "HardNetNeiMask", ("loss",))):
        tree = ast.parse(open(os.path.join(D.BASE, rel)).read())
        cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name]
        fns = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name in methods]
        assert len(cls) == 1 and len(fns) == len(methods)
        for f in fns:
            f.decorator_list = []
            f.name = cls_name + "_" + f.name
        exec(ast.unparse(ast.Module(body=fns, type_ignores=[])), ns)
    return ns


def warp_ref(ns, im, homo, align):
    """The reference's warp; with ``align`` its grid_sample call gets align_corners=True."""
    if not align:
        return ns["warp"](im, homo)
    fake_torch = types.SimpleNamespace(**{k: getattr(torch, k) for k in ("meshgrid", "arange", "cat", "matmul")})
    fake_torch.nn = types.SimpleNamespace(functional=types.SimpleNamespace(
        grid_sample=functools.partial(F.grid_sample, align_corners=True)))
    saved = ns["torch"]
    ns["torch"] = fake_torch
    try:
        return ns["warp"](im, homo)
    finally:
        ns["torch"] = saved


def diff32(x64, x32):
    d = (x64.double() - x32.double()).float()
    assert float((x32.double() + d.double() - x64.double()).abs().max()) < 1e-10
    return d.numpy()


def main():
    ns = reference_namespace()
    rng = np.random.RandomState(SEED)
    score64 = torch.from_numpy(rng.uniform(0.0, 1.0, (B, H, W, 1)))
    ori64 = torch.from_numpy(G.unit_vectors(rng, (B, H, W)))
    scale_var64 = torch.from_numpy(rng.uniform(8.0, 48.0, (B, H, W, 1)))
    scale_const64 = torch.full((B, H, W, 1), 32.0, dtype=torch.float64)
    h12_np, h21_np = G.homographies(H, W, G.FIXTURE_MOTIONS)
    h12_64, h21_64 = torch.from_numpy(h12_np), torch.from_numpy(h21_np)
    mask = G.random_mask(rng, B, H, W, K, BORDER)
    score32, ori32, scale_var32 = score64.float(), ori64.float(), scale_var64.float()
    h12_32, h21_32 = h12_64.float(), h21_64.float()
    # the fp64 evaluation sees the fp32 inputs' values: the difference is the arithmetic's alone
    score64, ori64, scale_var64, h12_64, h21_64 = (t.double() for t in (score32, ori32, scale_var32, h12_32, h21_32))
    h12_np, h21_np = h12_64.numpy(), h21_64.numpy()

    out, meta = {}, {}
    out.update(score=score32.squeeze(-1).numpy(), ori=ori32.numpy(), scale_var=scale_var32.squeeze(-1).numpy(),
               homo12=h12_32.numpy(), homo21=h21_32.numpy(), mask=mask)
    min_w = np.inf
    with torch.no_grad():
        # ---- warp + visible, both align_corners ----
        for align in (0, 1):
            w32 = warp_ref(ns, ns["filter_border"](score32), h12_32, align)
            w64 = warp_ref(ns, ns["filter_border"](score64), h12_64, align)
            v32 = warp_ref(ns, torch.ones_like(score32), h12_32, align)
            v64 = warp_ref(ns, torch.ones_like(score64), h12_64, align)
            e_w, e_v = float((w32.double() - w64).abs().max()), float((v32.double() - v64).abs().max())
            assert 0 < e_w < 1e-4 and 0 < e_v < 1e-4, (e_w, e_v)
            partial = float(((v64 > 0) & (v64 < 1)).double().mean())
            out[f"warped_ac{align}"], out[f"visible_ac{align}"] = w32.squeeze(-1).numpy(), v32.squeeze(-1).numpy()
            out[f"warped64_minus_32_ac{align}"] = diff32(w64, w32).squeeze(-1)
            out[f"visible64_minus_32_ac{align}"] = diff32(v64, v32).squeeze(-1)
            meta[f"E_warp_ac{align}"], meta[f"E_visible_ac{align}"] = e_w, e_v
            meta[f"visible_partial_share_ac{align}"] = partial
        # the installed torch's default is align_corners=False (the reference's own output, ac0); how far True is
        meta["warp_ac0_vs_ac1_max_diff"] = float(np.abs(out["warped_ac0"] - out["warped_ac1"]).max())
        # ---- gt_scale_orin, constant and varying scale ----
        for tag, s32, s64 in (("const", scale_const64.float(), scale_const64), ("var", scale_var32, scale_var64)):
            gs32, go32 = ns["Network_gt_scale_orin"](s32, ori32, h12_32, h21_32)
            gs64, go64 = ns["Network_gt_scale_orin"](s64, ori64, h12_64, h21_64)
            assert tuple(gs32.shape) == (B, H, W, 1) and tuple(go32.shape) == (1, B, H, W, 2)
            ex, mw = G.gt_exclusion(s64.squeeze(-1).numpy(), h12_np, h21_np)
            min_w = min(min_w, mw)
            share = float(ex.mean())
            assert share <= G.GT_EXCLUDED_CAP, share
            keep = torch.from_numpy(~ex)
            ds = (gs32.double() - gs64.double()).abs().squeeze(-1)
            assert float(ds[keep].max()) <= 1e-4, float(ds[keep].max())
            do = (go32.double() - go64).abs().amax(-1).squeeze(0)
            e_o = float(do[keep].max())
            assert 0 < e_o < 1e-4, e_o
            out[f"gt_scale_{tag}"], out[f"gt_ori_{tag}"] = gs32.squeeze(-1).numpy(), go32.squeeze(0).numpy()
            out[f"gt_scale64_{tag}"] = gs64.float().squeeze(-1).numpy()
            out[f"gt_ori64_minus_32_{tag}"] = diff32(go64, go32).squeeze(0)
            out[f"gt_excluded_{tag}"] = ex
            meta[f"E_gt_ori_{tag}"], meta[f"gt_excluded_share_{tag}"] = e_o, share
            meta[f"gt_scale_identical_{tag}"] = bool(torch.equal(gs32.double(), gs64.double()))
        # ---- ptCltoCr on the mask's keypoints: maps of the varying-scale ground truth ----
        topk = torch.from_numpy(mask).unsqueeze(-1)
        kpts = topk.nonzero()
        r_scale = torch.from_numpy(out["gt_scale_var"]).unsqueeze(-1)
        r_ori = torch.from_numpy(out["gt_ori_var"]).unsqueeze(0)
        for clamp in (1, 0):
            rc, rs, ro = ns["ptCltoCr"](kpts, h12_32, r_scale, r_ori, clamp=bool(clamp))
            rc64, kex, closest, mw = G.project_keypoints64(kpts.numpy(), h12_np, H, W, clamp=bool(clamp))
            min_w = min(min_w, mw)
            assert float(kex.mean()) <= G.KP_EXCLUDED_CAP
            assert np.array_equal(rc.numpy()[~kex], rc64[~kex])
            out[f"proj_kpts_clamp{clamp}"], out[f"proj_scale_clamp{clamp}"] = rc.numpy(), rs.numpy()
            out[f"proj_ori_clamp{clamp}"], out[f"proj_kpts64_clamp{clamp}"] = ro.numpy(), rc64
        out["kpts"], out["kp_excluded"] = kpts.numpy(), kex
        meta["kp_excluded_share"], meta["kp_closest_to_half"] = float(kex.mean()), closest
        # ---- pair ----
        info = torch.ones(B, 2)
        raw1 = torch.from_numpy(rng.uniform(0.0, 1.0, (B, 1, H, W))).float()
        raw2 = torch.from_numpy(rng.uniform(0.0, 1.0, (B, 1, H, W))).float()
        ppair, limc, rimc = ns["pair"](topk, None, scale_var32, ori32, info, raw1, h12_32, r_scale, r_ori, info, raw2, 32)
        assert tuple(ppair.shape) == (B * K, 2, 32, 32)
        rows = np.concatenate([np.arange(b * K, b * K + PATCH_ROWS) for b in range(B)])
        out.update(raw1=raw1.numpy(), raw2=raw2.numpy(), pair_rows=rows, pair_patches=ppair.numpy()[rows],
                   pair_limc=limc.numpy(), pair_rimc=rimc.numpy())
        # ---- Network.forward + criterion ----
        det_fx = np.load(os.path.join(HERE, "detect.npz"))
        det_meta = json.loads(str(det_fx["meta"]))
        det = ns["RFDet"](**det_meta["det_args"]).eval()
        sd, off = det.state_dict(), 0
        for k in det_meta["state_dict_keys"]:
            n = sd[k].numel()
            sd[k] = torch.from_numpy(det_fx["blob"][off:off + n].reshape(tuple(sd[k].shape)))
            off += n
        assert off == det_fx["blob"].size
        det.load_state_dict(sd)
        from fixtures import build_module
        des_module, _, _ = build_module("fdl_NASNet")

        class Des:
            MARGIN, C = float(des_module.MARGIN), float(des_module.C)

            def __call__(self, p):
                return des_module(p)

            def loss(self, *a):
                return ns["HardNetNeiMask_loss"](self, *a)

        images = torch.from_numpy(det_fx["images"])
        im1, im2 = images[:B].contiguous(), images[1:B + 1].contiguous()
        def det_c(x):  # the detector's orientation map made contiguous (see the docstring)
            sc, scale, ori = det(x)
            return sc, scale, ori.contiguous()
        det_c.process, det_c.loss = det.process, det.loss
        net = types.SimpleNamespace(det=det_c, des=Des(), PSIZE=32, TOPK=det_meta["K"], SCORE_W=1000.0, PAIR_W=1.0)
        net.gt_scale_orin = ns["Network_gt_scale_orin"]
        net.gtscore = lambda s, h: ns["Network_gtscore"](net, s, h)
        batch = (im1, info, h12_32, im2, info, h21_32, im1, im2)
        end = ns["Network_forward"](net, batch)
        plt, det_loss, des_loss = ns["Network_criterion"](net, end)
        for s, h in ((det(im2)[0], h12_32), (det(im1)[0], h21_32)):  # no top-K cut inside a group of equal values
            _, _, value, _ = net.gtscore(s, h)
            assert min(int((value[b] > 0).sum()) for b in range(B)) >= net.TOPK
            assert D.kth_gap(value, net.TOPK) > 1e-5
        meta["endpoint"] = {k: {"shape": list(v.shape), "dtype": str(v.dtype)} for k, v in end.items()}
        meta["losses"] = {k: float(v) for k, v in plt["scalar"].items()}
        meta["det_loss"], meta["des_loss"] = float(det_loss), float(des_loss)
        for k in ("im1_limc", "im1_rimcw", "im2_limc", "im2_rimcw"):
            out["end_" + k] = end[k].numpy()
    assert min_w > 0.5, min_w
    meta.update(source="FDLNet-master/latency/NASNet model/network.py, utils/{image,common,math,net}_utils.py; fp32 and "
                       "fp64 on the CPU", seed=SEED, B=B, H=H, W=W, K=K, border=BORDER, eps=G.EPS, min_abs_w=min_w,
                motions=[list(m) for m in G.FIXTURE_MOTIONS], SCORE_W=net.SCORE_W, PAIR_W=net.PAIR_W,
                network_topk=net.TOPK, torch=torch.__version__)
    out["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "gt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps({k: v for k, v in meta.items() if k != "endpoint"}, indent=1))


if __name__ == "__main__":
    main()
