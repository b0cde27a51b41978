"""RF-Net's ten-scale detector: hn_rfdet_forward (NativeRFDetector.forward) against the same module's torch layers
(RFDetSO.forward_torch) on the same GPU in the same process, timed with events on the stream after warm-up, median
of --reps (>= 10), at 1 x 240 x 320 and 8 x 480 x 640; and detect / detect_and_describe at K = --topk against their
torch formulations (forward_torch + select_keypoints_torch, then clip_patch + the descriptor's torch layers).
Images are uniform noise; the weights are seeded.  Run it on an otherwise idle GPU.  Prints one JSON line and, with
--out, writes it to that file.

"hbm_bytes" is the traffic the kernels are built to move -- per pixel: the image once, and per level one write and
one 18 x 18 / 16 x 16 windowed read of pre and of feat (64 B each), the raw score (4 B) and unit orientation (8 B)
written once and read by the tail (the score twice more with halo, from L2) -- and "achieved_gbps" that figure over
the measured time, against the 8 TB/s HBM figure the other benchmarks use."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hardnetnas_amd import detector as D  # noqa: E402
from hardnetnas_amd.model import RFDes  # noqa: E402
from hardnetnas_amd.patches import _clip_patch_torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1x240x320,8x480x640", help="images x height x width")
ap.add_argument("--topk", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--native-only", action="store_true", help="time hn_rfdet_forward alone (for a kernel trace)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.reps >= 10
dev = torch.device("cuda:0")
HBM_GBPS = 8000.0


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


def designed_bytes(B, H, W):
    win = (18 * 18) / (16 * 16)  # a layer workgroup reads its tile with halo 1
    per_pixel = 4 + 64  # image read, pre_1 written
    per_pixel += 9 * (64 * win + 64 * win + 64 + 64 + 12)  # steps 1..9 (feat is not read at step 1 nor written at 9)
    per_pixel -= 64 * win + 64
    per_pixel += 64 + 12  # step 10
    per_pixel += 10 * 12 + 12 + 4  # the tail: ten scores and orientations in, three maps out
    return B * H * W * per_pixel


torch.manual_seed(1)
# rfnet/config.py's values
det = D.randomise_rfdet_(D.RFDetSO(100.0, 100.0, 0.0, 5, args.topk, 15, 0.5, 3, 1, 1,
                                   [3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0, 17.0, 19.0, 21.0]), 1).to(dev)
des = RFDes(1.0, 1.0).eval().to(dev)
sel = det._select_args()
out = {"config": "hn_rfdet_forward vs RFDetSO.forward_torch on the same GPU; detect and detect_and_describe at K",
       "topk": args.topk, "reps": args.reps, "hbm_gbps_reference": HBM_GBPS, "sizes": {}}
with torch.no_grad():
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        images = torch.rand(B, 1, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(B * H))
        im_info = torch.ones(B, 2, device=dev)
        nd = det.native_detector(dev)
        score, scale, ori = nd.forward(images)
        fwd_ms = timed(lambda: nd.forward(images, score=score, scale=scale, ori=ori))
        row = {"forward_ms": round(fwd_ms, 4), "workspace_bytes": nd.workspace_bytes(B, H, W),
               "hbm_bytes": int(designed_bytes(B, H, W)),
               "achieved_gbps": round(designed_bytes(B, H, W) / (fwd_ms * 1e-3) / 1e9, 1)}
        row["share_of_hbm"] = round(row["achieved_gbps"] / HBM_GBPS, 4)
        if not args.native_only:
            t_score, t_scale, t_ori = det.forward_torch(images)
            tfwd_ms = timed(lambda: det.forward_torch(images))
            detect_ms = timed(lambda: D.detect(det, images))
            whole_ms = timed(lambda: D.detect_and_describe(det, des, images, im_info, images))

            def torch_detect():
                s, c, o = det.forward_torch(images)
                return D.select_keypoints_torch(s.squeeze(-1), *sel, scale_map=c.squeeze(-1),
                                                ori_map=o.reshape(B, H, W, 2))

            def torch_whole():
                kpts, _, kscale, kori, _, _, _ = torch_detect()
                x = _clip_patch_torch(kpts, kscale, kori, im_info, images, 32)
                f = des.features(des.input_norm(x)).view(x.shape[0], -1)
                return f / torch.norm(f, p=2, dim=-1, keepdim=True)

            tdetect_ms = timed(torch_detect)
            twhole_ms = timed(torch_whole)
            k_native = D.detect(det, images)[0]
            k_torch = torch_detect()[0]
            common = len({tuple(r) for r in k_native.tolist()} & {tuple(r) for r in k_torch.tolist()})
            row.update({
                "torch_forward_ms": round(tfwd_ms, 4), "speedup_forward": round(tfwd_ms / fwd_ms, 2),
                "detect_ms": round(detect_ms, 4), "torch_detect_ms": round(tdetect_ms, 4),
                "speedup_detect": round(tdetect_ms / detect_ms, 2),
                "detect_and_describe_ms": round(whole_ms, 4), "torch_detect_and_describe_ms": round(twhole_ms, 4),
                "speedup_detect_and_describe": round(twhole_ms / whole_ms, 2),
                "max_abs_score_diff_vs_torch": float((score - t_score.squeeze(-1)).abs().max()),
                "max_abs_scale_diff_vs_torch": float((scale - t_scale.squeeze(-1)).abs().max()),
                "keypoints_shared_with_torch": common, "keypoints": int(k_native.shape[0])})
        out["sizes"][size] = row
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
