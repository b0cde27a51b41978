"""Shared by tests/golden/make_gt_golden.py, tests/test_gt.py and tests/test_gpu_gt.py: the homographies the
homography ground-truth tests draw, fp64 hand projections and the exclusion rules of the comparisons.

Exclusion (EPS = 2e-4, about six times the few-ulp error of an fp32 coordinate below 128, so a pixel outside the band
cannot flip): ``gt_scale_orin`` truncates ten projected coordinates per output pixel and rounds two, so an output pixel
is excluded from value comparison if, in fp64, any of the ten truncated coordinates at its q lies within EPS of an
integer or either coordinate of proj(homo12, p) lies within EPS of a half-integer.  A keypoint is excluded if either of
its fp64 projected coordinates lies within EPS of a half-integer."""
import numpy as np

EPS = 2e-4
GT_EXCLUDED_CAP = 0.01
KP_EXCLUDED_CAP = 0.02
# (a, s, tx, ty, p1, p2) of the fixture's two images
FIXTURE_MOTIONS = ((0.21, 1.07, 3.3, -2.6, 4e-4, -3e-4), (-0.13, 0.91, -4.7, 1.9, -5e-4, 2e-4))


def homography_pair(H, W, motion):
    """(homo12, homo21) fp64 [3,3]: translate-to-centre . [[s cos a, -s sin a, tx], [s sin a, s cos a, ty],
    [p1, p2, 1]] . translate-back, and its fp64 inverse."""
    a, s, tx, ty, p1, p2 = motion
    cx, cy = W / 2.0, H / 2.0
    to_c = np.array([[1.0, 0.0, cx], [0.0, 1.0, cy], [0.0, 0.0, 1.0]])
    back = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]])
    m = np.array([[s * np.cos(a), -s * np.sin(a), tx], [s * np.sin(a), s * np.cos(a), ty], [p1, p2, 1.0]])
    h12 = to_c @ m @ back
    return h12, np.linalg.inv(h12)


def homographies(H, W, motions):
    """(homo12, homo21) fp64 [B,3,3] for a list of motions."""
    pairs = [homography_pair(H, W, m) for m in motions]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def drawn_motions(B, seed):
    """B motions in the fixture's range (rotation, scale, shift, perspective), seeded."""
    r = np.random.RandomState(seed)
    return [(r.uniform(-0.25, 0.25), r.uniform(0.9, 1.1), r.uniform(-5, 5), r.uniform(-3, 3), r.uniform(-5e-4, 5e-4),
             r.uniform(-5e-4, 5e-4)) for _ in range(B)]


def project64(h, x, y):
    """fp64 (px, py, w) of the [3,3] homography applied to (x, y, 1)."""
    u = h[0, 0] * x + h[0, 1] * y + h[0, 2]
    v = h[1, 0] * x + h[1, 1] * y + h[1, 2]
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    return u / (w + 1e-8), v / (w + 1e-8), w


def _near_integer(c):
    return np.abs(c - np.rint(c)) < EPS


def _near_half(c):
    return np.abs(c - np.floor(c) - 0.5) < EPS


def gt_exclusion(scale, homo12, homo21):
    """(excluded [B,H,W] bool, min |w|) for ``gt_scale_orin`` on the fp64 scale map [B,H,W] (see the module's
    docstring); min |w| runs over every projection the exclusion looks at."""
    B, H, W = scale.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((B, H, W), bool)
    min_w = np.inf
    for b in range(B):
        px, py, w = project64(homo12[b], xs, ys)
        min_w = min(min_w, float(np.abs(w).min()))
        ex = _near_half(px) | _near_half(py)
        qx = np.clip(np.rint(px), 0, W - 1)
        qy = np.clip(np.rint(py), 0, H - 1)
        hs = np.floor(scale[b][qy.astype(int), qx.astype(int)] / 2.0)
        for dx, dy in ((0, 0), (0, -1), (1, 0), (0, 1), (-1, 0)):
            cx, cy, w = project64(homo21[b], qx + dx * hs, qy + dy * hs)
            min_w = min(min_w, float(np.abs(w).min()))
            ex |= _near_integer(cx) | _near_integer(cy)
        out[b] = ex
    return out, min_w


def project_keypoints64(kpts, homo, H, W, clamp=True):
    """fp64 hand projection of int64 [N,4] rows (b, y, x, .): (rows (b, y', x', 0) int64, excluded [N] bool,
    distance of the nearest coordinate to a half-integer, min |w|)."""
    b = kpts[:, 0]
    h = homo[b]
    x, y = kpts[:, 2].astype(np.float64), kpts[:, 1].astype(np.float64)
    u = h[:, 0, 0] * x + h[:, 0, 1] * y + h[:, 0, 2]
    v = h[:, 1, 0] * x + h[:, 1, 1] * y + h[:, 1, 2]
    w = h[:, 2, 0] * x + h[:, 2, 1] * y + h[:, 2, 2]
    px, py = u / (w + 1e-8), v / (w + 1e-8)
    ex = _near_half(px) | _near_half(py)
    closest = float(min(np.abs(px - np.floor(px) - 0.5).min(), np.abs(py - np.floor(py) - 0.5).min()))
    xr, yr = np.rint(px).astype(np.int64), np.rint(py).astype(np.int64)
    if clamp:
        xr, yr = np.clip(xr, 0, W - 1), np.clip(yr, 0, H - 1)
    return np.stack((b, yr, xr, np.zeros_like(b)), 1), ex, closest, float(np.abs(w).min())


def unit_vectors(rng, shape):
    """Random unit (cos, sin) pairs [..., 2] fp64."""
    a = rng.uniform(0.0, 2.0 * np.pi, shape)
    return np.stack((np.cos(a), np.sin(a)), -1)


def random_mask(rng, B, H, W, K, border=8):
    """uint8 [B,H,W] with exactly K set pixels per image, all inside the border."""
    m = np.zeros((B, H, W), np.uint8)
    inner = [(y, x) for y in range(border, H - border) for x in range(border, W - border)]
    for b in range(B):
        for i in rng.choice(len(inner), K, replace=False):
            m[b, inner[i][0], inner[i][1]] = 1
    return m


def case_inputs(H, W, B, seed, K=48):
    """Seeded inputs of one (H, W, B) case, fp32-representable fp64 arrays: score [B,H,W], ori [B,H,W,2], scale
    [B,H,W] uniform in [8, 48), homo12 / homo21 [B,3,3] drawn as the fixture's, mask [B,H,W] with min(K, H W / 4) set
    pixels per image anywhere."""
    rng = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    h12, h21 = homographies(H, W, drawn_motions(B, seed + 1))
    return {"score": f(rng.uniform(0.0, 1.0, (B, H, W))), "ori": f(unit_vectors(rng, (B, H, W))),
            "scale": f(rng.uniform(8.0, 48.0, (B, H, W))), "homo12": f(h12), "homo21": f(h21),
            "mask": random_mask(rng, B, H, W, min(K, H * W // 4), border=0)}
