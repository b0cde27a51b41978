"""Keypoint detector and keypoint selection: the kernels (NativeDetector.forward = hn_det_forward,
_native.select_keypoints = hn_select_keypoints) against this package's torch formulation of the same two steps
(RFDet.forward_torch, select_keypoints_torch) on the same device, timed with hipEvents after warm-up, median of
--reps, at FDLNet's own size (2 images of 240 x 320, K = 512) and at 8 images of 480 x 640.  Images are uniform
noise; the detector's weights are seeded.  Run it on an otherwise idle GPU.  Prints one JSON line.

"share_of_detect_and_describe" is (detector + selection) / a whole detect_and_describe call with
HardNetNeiMask("NASNet") as the descriptor, all three timed the same way."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd import _native  # noqa: E402
from hardnetnas_amd import detector as D  # noqa: E402
from hardnetnas_amd.model import HardNetNeiMask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2x240x320,8x480x640", help="images x height x width")
ap.add_argument("--topk", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


torch.manual_seed(1)
det = D.RFDet(100.0, 100.0, 0.0, 5, args.topk, 15, 0.5).eval().to(dev)
des = HardNetNeiMask("NASNet").eval().to(dev)
sel = det._select_args()
out = {"config": "hn_det_forward + hn_select_keypoints vs the torch formulation on the same GPU",
       "topk": args.topk, "reps": args.reps, "sizes": {}}
with torch.no_grad():
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        images = torch.rand(B, 1, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(B * H))
        im_info = torch.ones(B, 2, device=dev)
        nd = det.native_detector(dev)
        score, ori = nd.forward(images)
        ws = torch.empty(_native.select_workspace_bytes(B, H, W, args.topk), dtype=torch.uint8, device=dev)
        det_ms = timed(lambda: nd.forward(images, score=score, ori=ori))
        sel_ms = timed(lambda: _native.select_keypoints(score, *sel, ori_map=ori, workspace=ws))
        both_ms = timed(lambda: D.detect(det, images))
        t_score, t_scale, t_ori = det.forward_torch(images)
        tdet_ms = timed(lambda: det.forward_torch(images))
        tsel_ms = timed(lambda: D.select_keypoints_torch(t_score.squeeze(-1), *sel, scale_map=t_scale.squeeze(-1),
                                                         ori_map=t_ori))
        whole_ms = timed(lambda: D.detect_and_describe(det, des, images, im_info, images))
        k_native = D.detect(det, images)[0]
        k_torch = D.select_keypoints_torch(t_score.squeeze(-1), *sel)[0]
        common = len({tuple(r) for r in k_native.tolist()} & {tuple(r) for r in k_torch.tolist()})
        out["sizes"][size] = {
            "detector_ms": round(det_ms, 4), "select_ms": round(sel_ms, 4), "detect_ms": round(both_ms, 4),
            "torch_detector_ms": round(tdet_ms, 4), "torch_select_ms": round(tsel_ms, 4),
            "speedup_detector": round(tdet_ms / det_ms, 1), "speedup_select": round(tsel_ms / sel_ms, 1),
            "speedup": round((tdet_ms + tsel_ms) / (det_ms + sel_ms), 1),
            "detect_and_describe_ms": round(whole_ms, 4),
            "share_of_detect_and_describe": round((det_ms + sel_ms) / whole_ms, 4),
            "max_abs_score_diff_vs_torch": float((score - t_score.squeeze(-1)).abs().max()),
            "keypoints_shared_with_torch": common, "keypoints": int(k_native.shape[0])}
print(json.dumps(out))
