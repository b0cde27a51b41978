"""Shared helpers of the keypoint patch extraction tests (test_clip.py, test_gpu_clip.py) and of
tests/golden/make_clip_golden.py: an fp64 evaluation of clip_patch written sample by sample, independent of
hardnetnas_amd/patches.py, with the side of each discontinuity selectable, and the exclusion rule.

clip_patch is discontinuous only where a sample coordinate crosses 0 or W - 1 (H - 1): inside [0, W - 1) it
interpolates, outside it is (nearly) 0.  Pixels whose fp64 coordinate lies within EXCLUDE_EPS of one of those four
lines are left out of value comparisons; on them a result must equal one of the one-sided evaluations."""
import itertools

import torch

EXCLUDE_EPS = 1e-3


RATIOS = (1.0, 0.5, 1.0 / 3.0)


def random_case(n, B, H, W, seed, images=None):
    """Seeded CPU inputs in the golden fixture's style: (kpts [n,4] int64, scale [n], ori [n,2], ratio [B],
    images [B,1,H,W]) -- a random image per keypoint (unequal counts, no order), integer (y, x) over the whole
    rescaled image with its borders, scale uniform in [2, 40] x ratio, random angles."""
    g = torch.Generator().manual_seed(seed)
    if images is None:
        images = torch.rand(B, 1, H, W, generator=g)
    ratio = torch.tensor([RATIOS[b % 3] for b in range(B)], dtype=torch.float32)
    kpts = torch.zeros(n, 4, dtype=torch.int64)
    kpts[:, 0] = torch.randint(0, B, (n,), generator=g)
    r = ratio[kpts[:, 0]].double()
    u = torch.rand(n, 2, generator=g, dtype=torch.float64)
    kpts[:, 1] = (u[:, 0] * (((H - 1) * r).floor() + 1)).floor().long()
    kpts[:, 2] = (u[:, 1] * (((W - 1) * r).floor() + 1)).floor().long()
    scale = ((2.0 + 38.0 * torch.rand(n, generator=g)) * ratio[kpts[:, 0]]).float()
    ang = 2.0 * 3.141592653589793 * torch.rand(n, generator=g)
    ori = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1)
    return kpts, scale, ori, ratio, images


def coords64(kpts, scale, ori, ratio, P=32):
    """fp64 sample coordinates (xs, ys) [N,P,P] from the fp32 inputs (grid values: the fp32 linspace values);
    ratio [B] is indexed by the keypoint's column 0."""
    g = torch.linspace(-1, 1, P, dtype=torch.float32).double()
    n = kpts.shape[0]
    r = ratio.double()[kpts[:, 0]]
    s = (scale.double().view(-1) / r / 2.0).view(n, 1, 1)
    c = ori[:, 0].double().view(n, 1, 1) if ori is not None else 1.0
    sn = ori[:, 1].double().view(n, 1, 1) if ori is not None else 0.0
    gx, gy = g.view(1, 1, P), g.view(1, P, 1)
    xs = s * c * gx - s * sn * gy + (kpts[:, 2].double() / r).view(n, 1, 1)
    ys = s * sn * gx + s * c * gy + (kpts[:, 1].double() / r).view(n, 1, 1)
    return xs, ys


def near_lines(xs, ys, H, W, eps=EXCLUDE_EPS):
    """The excluded pixels: a coordinate within eps of x = 0, x = W - 1, y = 0 or y = H - 1."""
    return ((xs.abs() < eps) | ((xs - (W - 1)).abs() < eps) | (ys.abs() < eps) | ((ys - (H - 1)).abs() < eps))


def _corners(v, hi, flip):
    """(v0, v1) clamped corners of fp64 coordinates v; with flip, pixels within EXCLUDE_EPS of the line 0 or hi
    take the corners of the other side of that line."""
    f = v.floor()
    if flip:
        lo_line, hi_line = v.abs() < EXCLUDE_EPS, (v - hi).abs() < EXCLUDE_EPS
        f = torch.where(lo_line, torch.where(v >= 0, f - 1, f + 1), f)   # [0, 1) <-> [-1, 0)
        f = torch.where(hi_line, torch.where(v >= hi, f - 1, f + 1), f)  # [hi - 1, hi) <-> [hi, hi + 1)
    return f.clamp(0, hi), (f + 1).clamp(0, hi)


def eval64(kpts, scale, ori, ratio, images, P=32, flip_x=False, flip_y=False):
    """clip_patch in fp64 [N,1,P,P] on CPU tensors; flip_x / flip_y evaluate the pixels near a discontinuity
    line with the other side's corners (at the same coordinate), all other pixels as they are."""
    B, _, H, W = images.shape
    xs, ys = coords64(kpts, scale, ori, ratio, P)
    x0, x1 = _corners(xs, W - 1, flip_x)
    y0, y1 = _corners(ys, H - 1, flip_y)
    im = images.double().reshape(-1)
    base = (kpts[:, 0] * (H * W)).view(-1, 1, 1)

    def px(yv, xv):
        return im[base + yv.long() * W + xv.long()]

    out = ((x1 - xs) * (y1 - ys) * px(y0, x0) + (x1 - xs) * (ys - y0) * px(y1, x0)
           + (xs - x0) * (y1 - ys) * px(y0, x1) + (xs - x0) * (ys - y0) * px(y1, x1))
    return out.unsqueeze(1)


def one_sided(kpts, scale, ori, ratio, images, P=32):
    """The four evaluations (natural, x flipped, y flipped, both) a pixel near a line may equal."""
    return [eval64(kpts, scale, ori, ratio, images, P, fx, fy) for fx, fy in itertools.product((False, True), repeat=2)]


def check_against_fp64(got, kpts, scale, ori, ratio, images, tol, want=None):
    """Assert the comparison of the issue: on the kept pixels ``got`` is within tol of the fp64 evaluation
    (``want`` if given, else eval64), on the excluded ones within tol of one of the one-sided evaluations.  All CPU
    tensors.  Returns (worst kept error, excluded share)."""
    B, _, H, W = images.shape
    xs, ys = coords64(kpts, scale, ori, ratio, got.shape[-1])
    excl = near_lines(xs, ys, H, W).unsqueeze(1)
    want = eval64(kpts, scale, ori, ratio, images, got.shape[-1]) if want is None else want
    err = (got.double() - want).abs()
    worst = float(err[~excl].max()) if (~excl).any() else 0.0
    share = float(excl.double().mean())
    print(f"clip: worst kept error {worst:.3e} (tol {tol:.3e}), excluded share {share:.4%}")
    assert worst <= tol, (worst, tol)
    if excl.any():  # only the keypoints that own an excluded pixel are evaluated again
        rows = excl.flatten(1).any(dim=1)
        sides = one_sided(kpts[rows], scale[rows], ori[rows] if ori is not None else None, ratio, images, got.shape[-1])
        best = torch.stack([(got[rows].double() - s).abs() for s in sides]).min(dim=0).values
        assert float(best[excl[rows]].max()) <= tol, (float(best[excl[rows]].max()), tol)
    return worst, share
