"""Generate tests/golden/clip_patch.npz from the REFERENCE keypoint patch extraction.

Run from the repo root:  python tests/golden/make_clip_golden.py
Needs the reference tree (HN_REFERENCE, as make_golden.py; read-only, never copied): ``clip_patch`` of
FDLNet-master/latency/NASNet/utils/image_utils.py:11-158 is AST-extracted (the file imports skimage, which is
not needed for this one function) and executed with ``torch`` in scope on seeded inputs; only data (the inputs,
the reference's fp32 patches, an fp64 evaluation, the mask of excluded pixels, JSON metadata) is written.

Inputs: B = 3 images of 61 x 83 uniform noise in [0, 1) (the worst case for interpolation error),
im_info[:, 0] = (1, 0.5, 1/3), 40 keypoints per image in batch order (where the reference's two ways of finding
a keypoint's image agree), integer (y, x) uniform over the whole rescaled image with its borders, scale uniform
in [2, 40] x ratio, random angles; every 8th keypoint is axis-aligned (cos 1, sin 0) with an even-integer scale
in raw pixels, so that its corner columns land on integer coordinates.

The function is discontinuous only where a sample coordinate crosses 0 or W - 1 (H - 1); pixels whose fp64
coordinate lies within 1e-3 of one of those lines are excluded from value comparisons (tests/clip_ref.py).  The
generator asserts that the excluded share is <= 1 % and that at least 5 % of the samples fall outside the image.
E_ref = max |reference fp32 - fp64| over the kept pixels is what the tests scale their tolerances by.
"""
from __future__ import annotations

import ast
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_ref  # noqa: E402

REF = os.environ.get("HN_REFERENCE", "/root/reference")
SOURCE = os.path.join(REF, "FDLNet-master", "latency", "NASNet", "utils", "image_utils.py")

SEED = 2025
B, H, W = 3, 61, 83
PER_IMAGE = 40
RATIOS = (1.0, 0.5, 1.0 / 3.0)
PSIZE = 32


def reference_clip_patch():
    tree = ast.parse(open(SOURCE).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "clip_patch"]
    assert len(keep) == 1, SOURCE
    ns = {"torch": torch}
    exec(ast.unparse(ast.Module(body=keep, type_ignores=[])), ns)
    return ns["clip_patch"]


def inputs():
    g = torch.Generator().manual_seed(SEED)
    images = torch.rand(B, 1, H, W, generator=g)
    ratio = torch.tensor(RATIOS, dtype=torch.float32)
    im_info = torch.stack([ratio, ratio], dim=1)
    n = B * PER_IMAGE
    kpts = torch.zeros(n, 4, dtype=torch.int64)
    scale = torch.empty(n)
    ori = torch.empty(n, 2)
    for b in range(B):
        r = float(ratio[b])
        rows = slice(b * PER_IMAGE, (b + 1) * PER_IMAGE)
        kpts[rows, 0] = b
        kpts[rows, 1] = torch.randint(0, int((H - 1) * r) + 1, (PER_IMAGE,), generator=g)
        kpts[rows, 2] = torch.randint(0, int((W - 1) * r) + 1, (PER_IMAGE,), generator=g)
        scale[rows] = (2.0 + 38.0 * torch.rand(PER_IMAGE, generator=g)) * ratio[b]
        ang = 2.0 * math.pi * torch.rand(PER_IMAGE, generator=g)
        ori[rows, 0], ori[rows, 1] = torch.cos(ang), torch.sin(ang)
    even = 2.0 * torch.randint(1, 21, (n,), generator=g).float()  # raw-pixel scales 2, 4, .. 40
    for i in range(0, n, 8):
        scale[i] = even[i] * ratio[kpts[i, 0]]
        ori[i, 0], ori[i, 1] = 1.0, 0.0
    return kpts, scale, ori, im_info, images


def main():
    ref_fn = reference_clip_patch()
    kpts, scale, ori, im_info, images = inputs()
    with torch.no_grad():
        ref32 = ref_fn(kpts, scale, ori, im_info, images, PSIZE)
    assert ref32.dtype == torch.float32 and tuple(ref32.shape) == (kpts.shape[0], 1, PSIZE, PSIZE)
    ratio = im_info[:, 0].contiguous()
    ref64 = clip_ref.eval64(kpts, scale, ori, ratio, images, PSIZE)
    xs, ys = clip_ref.coords64(kpts, scale, ori, ratio, PSIZE)
    excluded = clip_ref.near_lines(xs, ys, H, W).unsqueeze(1)
    outside = ((xs < 0) | (xs > W - 1) | (ys < 0) | (ys > H - 1)).unsqueeze(1)
    excluded_share = float(excluded.double().mean())
    outside_share = float(outside.double().mean())
    assert excluded_share <= 0.01, excluded_share
    assert outside_share >= 0.05, outside_share
    e_ref = float((ref32.double() - ref64)[~excluded].abs().max())
    assert 0.0 < e_ref < 1e-4, e_ref
    outside_max = float(ref32[outside & ~excluded].abs().max())
    # the fp64 evaluation is stored as its difference from the reference's fp32 patches, in fp32: |difference|
    # <= E_ref, so the sum ref32 + difference (in fp64) restores it to E_ref x 2^-24 < 1e-12 at half the bytes
    delta = (ref64 - ref32.double()).float()
    assert float((ref32.double() + delta.double() - ref64).abs().max()) < 2.5e-13
    meta = {"source": "FDLNet-master/latency/NASNet/utils/image_utils.py:11-158, fp32 on the CPU",
            "seed": SEED, "B": B, "H": H, "W": W, "per_image": PER_IMAGE, "PSIZE": PSIZE,
            "exclude_eps": clip_ref.EXCLUDE_EPS, "E_ref": e_ref, "excluded_share": excluded_share,
            "outside_share": outside_share, "outside_max_abs": outside_max}
    out = {"images": images.numpy(), "kpts": kpts.numpy(), "scale": scale.numpy(), "ori": ori.numpy(),
           "im_info": im_info.numpy(), "ref32": ref32.numpy(), "ref64_minus_ref32": delta.numpy(),
           "excluded": excluded.numpy(), "meta": json.dumps(meta)}
    path = os.path.join(HERE, "clip_patch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
