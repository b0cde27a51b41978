"""Shared by tests/test_hardnet_layer_ref.py (CPU) and tests/test_gpu_hardnet_layers.py (GPU): the stock HardNet train
step one layer operation at a time (hn_hardnet_train_layer_op) -- cases, seeded inputs, the fp64 / fp32 CPU references,
the bars and the mutants that justify them.

A case is (op, layer, B).  Its inputs come from ``synth.normal`` under a seed derived from the case: a pre-activation
``z`` of the previous layer (the kernel applies the ReLU where the step does; layer 0 reads it as the normalised
patch), weights scaled by 1 / sqrt(Cin k k), and an upstream gradient.  Everything here is NCHW on the CPU;
``to_cnhw`` / ``from_cnhw`` convert to the kernels' layout.

References.  ``ref64`` is torch.nn.functional.conv2d and autograd in fp64 (BatchNorm's train-mode statistics, the L2
normalisation and input_norm written out in fp64); ``ref32`` is the same operation in fp32 on the CPU: its distance
E32 from ref64 is what a correct fp32 evaluation costs on that input.

Metrics: the L2-relative error, and the largest absolute error over the largest |ref64|.

The bar: each metric against 16 x its own E32, with a floor of 2^-22 (a few ulps of one fp32 rounding).  16 = the
project's 4 for another fp32 evaluation order x 4 for chain length: the kernels accumulate up to
K = 1,152 terms in one fp32 chain where the CPU's vectorised convolution splits the chain at least 16 ways, and
sqrt(16) = 4 (a plain sequential fp32 chain on the CPU measured up to 2.7 x torch's E32).  The stride-1 data gradients
on the bf16x3 eval kernels (and the forwards of layers 1..5 on the same kernels, HN_TRAIN_F32 bit 0 off: the same
arithmetic, so the same rule) get 2 E_split + 16 E32, E_split from a CPU emulation of the split on the case's inputs
(hi = bf16(v), lo = bf16(v - hi), hi.hi + hi.lo + lo.hi summed in fp64): tests/test_gpu_match.py's rule.  Running
statistics keep the project's 1e-5 relative bar.

Mutants (``mutants``) are deliberately wrong fp64 evaluations of the same operation -- the structural errors these
kernels can have.  tests/test_hardnet_layer_ref.py asserts that every one misses the case's bar by a factor of 10 or
more in at least one metric: that is what allows the 16 x margin.  The seeds were chosen on the CPU references alone
(the plain crc32 of the case: no case needed another)."""
import zlib
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from hardnetnas_amd import synth

# cin, cout, hin, ks, stride, pad (csrc/hn_train.hip kHardnetTrainLayers)
LAYERS = [(1, 32, 32, 3, 1, 1), (32, 32, 32, 3, 1, 1), (32, 64, 32, 3, 2, 1), (64, 64, 16, 3, 1, 1),
          (64, 128, 16, 3, 2, 1), (128, 128, 8, 3, 1, 1), (128, 128, 8, 8, 1, 0)]
CONV_OPS = ("conv_fwd", "conv_wgrad", "conv_dgrad")
BATCHES = (3, 5, 37)
FLOOR = 2.0 ** -22
FACTOR = 16.0
RUNNING_BAR = 1e-5
BN_EPS, IN_EPS, L2_EPS, MOMENTUM = 1e-5, 1e-7, 1e-10, 0.1
DROP_P, DROP_SEED = 0.3, 20240607

CONV_CASES = [(op, l, b) for op in CONV_OPS for l in range(7) for b in BATCHES]
# layers 5 / 6 read 128 channels of 8x8: two statistics slices from B = 65 (L = 4,480 at B = 70); 32 channels at
# B = 37: ten slices
BN_SHAPES = [(l, 5) for l in range(7)] + [(4, 70), (5, 70), (1, 37)]
BN_CASES = [(op, l, b) for op in ("bn_fwd", "bn_bwd") for l, b in BN_SHAPES]
PATCH_CASES = [(op, 0, b) for op in ("input_norm", "l2_fwd", "l2_bwd", "input_norm_bwd") for b in BATCHES]
DROPOUT_CASES = [("conv_fwd+drop", 6, 5), ("conv_wgrad+drop", 6, 5), ("bn_bwd+drop", 5, 5)]
ALL_CASES = CONV_CASES + BN_CASES + PATCH_CASES + DROPOUT_CASES


def case_id(case):
    return f"{case[0]}-l{case[1]}-B{case[2]}"


def hout(l):
    cin, cout, h, k, s, p = LAYERS[l]
    return (h + 2 * p - k) // s + 1


def normal(case, name, shape):
    """fp32 N(0, 1) of ``shape`` for tensor ``name`` of a case."""
    seed = zlib.crc32(f"hardnet-layer:{case_id(case)}:{name}".encode())
    n = int(np.prod(shape))
    return torch.from_numpy(synth.normal(seed, n).astype(np.float32).reshape(shape))


def to_cnhw(t):
    return t.transpose(0, 1).contiguous()


def from_cnhw(t):
    return t.transpose(0, 1).contiguous()


def bn_slices(c, length):
    """csrc/hn_train_kernels.h bn_slices and the slice length of bn_part_body / k_bn_bwd_part."""
    ns = max(1, min(64, (2048 + c - 1) // c, (length + 4095) // 4096))
    per = (length + ns - 1) // ns
    if length % 4 == 0:
        per = (per + 3) & ~3
    return ns, per


def dropout_mask(seed, p, b):
    """csrc/hn_train_kernels.h drop_scale (tests/test_gpu_train.py _dropout_mask's restatement): the mask of
    relu(z5), CNHW index [128][B][8][8], as NCHW [B,128,8,8] fp32."""
    e = np.arange(128 * b * 64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (e * np.uint64(0x9E3779B97F4A7C15))
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    m = np.where(u < np.float32(p), np.float32(0.0), scale).astype(np.float32)
    return torch.from_numpy(m.reshape(128, b, 8, 8).transpose(1, 0, 2, 3).copy())


def metrics(got, ref):
    """(L2-relative error, largest absolute error / largest |ref|), in fp64."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


def bar_of(e32, e_split=None):
    """The bar of each metric from its own E32 (and E_split for the bf16x3 form)."""
    if e_split is None:
        return tuple(max(FACTOR * e, FLOOR) for e in e32)
    return tuple(max(2.0 * s + FACTOR * e, FLOOR) for e, s in zip(e32, e_split))


# ------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------
def conv_inputs(case):
    """{z [B,cin,h,h], w [cout,cin,k,k], dy [B,cout,ho,ho], mask or None}, fp32."""
    op, l, b = case
    cin, cout, h, k, s, p = LAYERS[l]
    ho = hout(l)
    base = (op.split("+")[0], l, b)
    return {"z": normal(base, "z", (b, cin, h, h)),
            "w": normal(base, "w", (cout, cin, k, k)) / float(np.sqrt(cin * k * k)),
            "dy": normal(base, "dy", (b, cout, ho, ho)),
            "mask": dropout_mask(DROP_SEED, DROP_P, b) if op.endswith("+drop") else None}


def conv_eval(op, l, z, w, dy, mask=None, relu=True):
    """The operation in the dtype of its arguments: conv2d over act(z) (act: ReLU from layer 1 on, x mask), its
    weight gradient, or its gradient w.r.t. act(z), for the upstream gradient dy."""
    cin, cout, h, k, s, p = LAYERS[l]
    a = z if (l == 0 or not relu) else z.clamp_min(0)
    if mask is not None:
        a = a * mask.to(a.dtype)
    if op == "conv_fwd":
        return F.conv2d(a, w, stride=s, padding=p)
    w, a = w.detach().clone().requires_grad_(op == "conv_wgrad"), a.detach().clone().requires_grad_(op == "conv_dgrad")
    (F.conv2d(a, w, stride=s, padding=p) * dy).sum().backward()
    return w.grad if op == "conv_wgrad" else a.grad


def _bf16_split(v):
    hi = v.float().bfloat16().double()
    lo = (v.double() - hi).float().bfloat16().double()
    return hi, lo


@lru_cache(maxsize=None)
def conv_case(case):
    """{inputs (fp32), ref64, ref32, e32, bar; for the stride-1 data gradients also e_split, bar_bf16x3}."""
    op, l, b = case
    kind = op.split("+")[0]
    x = conv_inputs(case)
    d = {k: (v.double() if v is not None else None) for k, v in x.items()}
    ref64 = conv_eval(kind, l, d["z"], d["w"], d["dy"], d["mask"])
    ref32 = conv_eval(kind, l, x["z"], x["w"], x["dy"], x["mask"])
    e32 = metrics(ref32, ref64)
    out = {"x": x, "ref64": ref64, "ref32": ref32, "e32": e32, "bar": bar_of(e32)}
    if kind == "conv_dgrad" and l in (1, 3, 5):
        (wh, wl), (gh, gl) = _bf16_split(x["w"]), _bf16_split(x["dy"])
        split = sum(conv_eval(kind, l, d["z"], ww, gg) for ww, gg in ((wh, gh), (wh, gl), (wl, gh)))
    elif kind == "conv_fwd" and 1 <= l <= 5 and x["mask"] is None:
        # HN_TRAIN_F32 bit 0 off runs the forward on the same bf16x3 kernels: the same rule, on relu(z) and w
        (wh, wl), (ah, al) = _bf16_split(x["w"]), _bf16_split(x["z"].clamp_min(0))
        split = sum(conv_eval(kind, l, aa, ww, None, relu=False) for ww, aa in ((wh, ah), (wh, al), (wl, ah)))
    else:
        return out
    out["e_split"] = metrics(split, ref64)
    out["bar_bf16x3"] = bar_of(e32, out["e_split"])
    return out


def conv_mutants(case):
    """{name: wrong fp64 result} of a convolution case."""
    op, l, b = case
    kind = op.split("+")[0]
    cin, cout, h, k, s, p = LAYERS[l]
    c = conv_case(case)
    z, w, dy = (c["x"][n].double() for n in ("z", "w", "dy"))
    mask = c["x"]["mask"].double() if c["x"]["mask"] is not None else None
    ref = c["ref64"]
    ev = lambda **kw: conv_eval(kind, l, kw.get("z", z), kw.get("w", w), kw.get("dy", dy), mask,  # noqa: E731
                                kw.get("relu", True))
    m = {}
    # the last patch dropped (a ragged last workgroup that returns early)
    if kind == "conv_wgrad":
        m["last patch dropped"] = conv_eval(kind, l, z[:-1], w, dy[:-1], mask[:-1] if mask is not None else None)
    else:
        m["last patch dropped"] = ref.clone()
        m["last patch dropped"][-1] = 0
    rows = ref.shape[2] if kind != "conv_wgrad" else hout(l)  # the rows the segments split
    if 1 <= l <= 5:
        for ns in (2, 4):
            # the last row segment of the last patch dropped
            r0 = rows - rows // ns
            if kind == "conv_wgrad":
                only = torch.zeros_like(dy)
                only[-1, :, r0:] = dy[-1, :, r0:]
                m[f"last segment dropped NS={ns}"] = ref - ev(dy=only)
            else:
                m[f"last segment dropped NS={ns}"] = ref.clone()
                m[f"last segment dropped NS={ns}"][-1, :, r0:] = 0
        # the first row of the second segment (NS = 2) of the last patch without the tap row above it; k_dgrad2's
        # ring runs the other way: the last cell row of the first segment without the dY row below it
        ys = hout(l) // 2 if (kind != "conv_dgrad" or s == 2) else h // 2
        ky = 0 if (kind != "conv_dgrad" or s == 2) else 2
        wk = torch.zeros_like(w)
        wk[:, :, ky] = w[:, :, ky]
        if kind == "conv_wgrad":
            only = torch.zeros_like(dy)
            only[-1, :, ys] = dy[-1, :, ys]
            part = ev(dy=only)
            m["halo row missing"] = ref.clone()
            m["halo row missing"][:, :, 0] -= part[:, :, 0]
        else:
            row = ys if kind == "conv_fwd" or s == 1 else 2 * ys - 1
            part = ev(w=wk)
            m["halo row missing"] = ref.clone()
            m["halo row missing"][-1, :, row] -= part[-1, :, row]
    # the x = -1 pad column reading the previous row's last element (the flat neighbour) instead of zero
    if p == 1 and (kind != "conv_dgrad" or s == 1 and l >= 1):
        if kind == "conv_dgrad":
            src, wf = dy, w.flip(2, 3).transpose(0, 1)  # din = conv2d(dy, wf, padding 1)
        else:
            src = z if l == 0 else z.clamp_min(0)
            wf = w
        prev = torch.zeros(src.shape[0], src.shape[1], src.shape[2], 1, dtype=src.dtype)
        prev[:, :, 1:, 0] = src[:, :, :-1, -1]
        st = (s, 1) if kind != "conv_dgrad" else (1, 1)
        if kind == "conv_wgrad":
            wk = wf[:, :, :, 0:1].clone().requires_grad_()
            (F.conv2d(prev, wk, stride=st, padding=(1, 0)) * dy[:, :, :, 0:1]).sum().backward()
            extra = wk.grad
        else:
            extra = F.conv2d(prev, wf[:, :, :, 0:1], stride=st, padding=(1, 0))
        m["pad column reads its flat neighbour"] = ref.clone()
        m["pad column reads its flat neighbour"][:, :, :, 0:1] += extra
    if kind != "conv_dgrad" and l >= 1:
        m["input ReLU left out"] = ev(relu=False)
    m["ky and kx swapped"] = ref.transpose(2, 3) if kind == "conv_wgrad" else ev(w=w.transpose(2, 3))
    if kind == "conv_dgrad":
        m["unflipped weights"] = ev(w=w.flip(2, 3))
        if s == 2:
            idx = torch.arange(h) ^ 1
            m["parity classes swapped"] = ref[:, :, idx][:, :, :, idx]
        if (s == 2 or k == 8) and b >= 4:  # chunks of 2 patches: the second one written at offset 0
            m["second chunk at offset 0"] = ref.clone()
            m["second chunk at offset 0"][0:2] = ref[2:4]
            m["second chunk at offset 0"][2:4] = 0
    return m


# ------------------------------------------------------------------------------------------
# BatchNorm (train mode, affine=False), forward and backward
# ------------------------------------------------------------------------------------------
def bn_inputs(case):
    """bn_fwd: {y, rmean, rvar}; bn_bwd: {z, rstd, da, mask or None}; fp32, NCHW."""
    op, l, b = case
    c, ho = LAYERS[l][1], hout(l)
    base = (op.split("+")[0], l, b)
    y = normal(base, "y", (b, c, ho, ho)) * (0.5 + normal(base, "scale", (1, c, 1, 1)).abs()) \
        + 0.5 * normal(base, "shift", (1, c, 1, 1))
    if op == "bn_fwd":
        return {"y": y, "rmean": 0.1 * normal(base, "rmean", (c,)), "rvar": 1.0 + 0.2 * normal(base, "rvar", (c,)).abs()}
    y = y.double()
    var = y.var((0, 2, 3), unbiased=False, keepdim=True)
    z = ((y - y.mean((0, 2, 3), keepdim=True)) / (var + BN_EPS).sqrt()).float()  # a BN output, as the step saves it
    return {"z": z, "rstd": (1.0 / (var.flatten() + BN_EPS).sqrt()).float(), "da": normal(base, "da", (b, c, ho, ho)),
            "mask": dropout_mask(DROP_SEED, DROP_P, b) if op.endswith("+drop") else None}


def bn_fwd_eval(y, rmean, rvar, count=None):
    """(z, rstd, running_mean, running_var) in y's dtype; ``count``: statistics from the first ``count`` positions of
    every channel's CNHW row only (the mutant)."""
    b, c = y.shape[:2]
    rows = y.transpose(0, 1).reshape(c, -1)
    n = rows.shape[1]
    used = rows if count is None else rows[:, :count]
    mean = used.sum(1) / n
    var = ((used * used).sum(1) / n - mean * mean).clamp_min(0) if count is not None else rows.var(1, unbiased=False)
    rstd = 1.0 / (var + BN_EPS).sqrt()
    z = (y - mean.view(1, c, 1, 1)) * rstd.view(1, c, 1, 1)
    return (z, rstd, (1 - MOMENTUM) * rmean + MOMENTUM * mean, (1 - MOMENTUM) * rvar + MOMENTUM * var * n / (n - 1))


def bn_bwd_eval(l, z, rstd, da, mask=None, relu=True, count=None):
    """dy = rstd (g - mean(g) - z mean(g z)), g = da relu'(z) [x mask]; ReLU for layers 0..5."""
    b, c = z.shape[:2]
    g = da * (z > 0).to(da.dtype) if (l < 6 and relu) else da
    if mask is not None:
        g = g * mask.to(g.dtype)
    rows = lambda t: t.transpose(0, 1).reshape(c, -1)  # noqa: E731
    n = rows(g).shape[1]
    cut = slice(None) if count is None else slice(0, count)
    m1 = (rows(g)[:, cut].sum(1) / n).view(1, c, 1, 1)
    m2 = (rows(g * z)[:, cut].sum(1) / n).view(1, c, 1, 1)
    return rstd.view(1, c, 1, 1) * (g - m1 - z * m2)


@lru_cache(maxsize=None)
def bn_case(case):
    """bn_fwd: ref64 / ref32 are (z, rstd, rmean, rvar), e32 / bar per output for z and rstd; bn_bwd: one tensor."""
    op, l, b = case
    x = bn_inputs(case)
    d = {k: (v.double() if v is not None else None) for k, v in x.items()}
    if op == "bn_fwd":
        ref64 = bn_fwd_eval(d["y"], d["rmean"], d["rvar"])
        rm, rv = x["rmean"].clone(), x["rvar"].clone()
        z32 = F.batch_norm(x["y"], rm, rv, training=True, momentum=MOMENTUM, eps=BN_EPS)
        rstd32 = 1.0 / (x["y"].transpose(0, 1).reshape(z32.shape[1], -1).var(1, unbiased=False) + BN_EPS).sqrt()
        ref32 = (z32, rstd32, rm, rv)
        e32 = [metrics(ref32[i], ref64[i]) for i in range(2)]
        return {"x": x, "ref64": ref64, "ref32": ref32, "e32": e32, "bar": [bar_of(e) for e in e32]}
    ref64 = bn_bwd_eval(l, d["z"], d["rstd"], d["da"], d["mask"])
    ref32 = bn_bwd_eval(l, x["z"], x["rstd"], x["da"], x["mask"])
    e32 = metrics(ref32, ref64)
    return {"x": x, "ref64": ref64, "ref32": ref32, "e32": e32, "bar": bar_of(e32)}


def bn_mutants(case):
    """{name: wrong fp64 result (bn_fwd: of z)}."""
    op, l, b = case
    c = bn_case(case)
    d = {k: (v.double() if v is not None else None) for k, v in c["x"].items()}
    ns, per = bn_slices(LAYERS[l][1], b * hout(l) ** 2)
    count = (ns - 1) * per if ns > 1 else None
    m = {}
    if op == "bn_fwd":
        m["last patch left as it was"] = c["ref64"][0].clone()
        m["last patch left as it was"][-1] = d["y"][-1]
        if count:
            m["statistics without the last slice"] = bn_fwd_eval(d["y"], d["rmean"], d["rvar"], count)[0]
        return m
    m["last patch left as it was"] = c["ref64"].clone()
    m["last patch left as it was"][-1] = d["da"][-1]
    if l < 6:
        m["ReLU mask left out"] = bn_bwd_eval(l, d["z"], d["rstd"], d["da"], d["mask"], relu=False)
    if count:
        m["statistics without the last slice"] = bn_bwd_eval(l, d["z"], d["rstd"], d["da"], d["mask"], count=count)
    return m


# ------------------------------------------------------------------------------------------
# the per-patch kernels: input_norm, L2Norm forward / backward, input_norm's backward
# ------------------------------------------------------------------------------------------
def patch_inputs(case):
    op, _, b = case
    if op == "input_norm":
        seed = zlib.crc32(f"hardnet-layer:{case_id(case)}".encode()) & 0xFFFF
        return {"x": torch.from_numpy(synth.synth_patches(b, seed=seed)).reshape(b, 1024)}
    if op == "input_norm_bwd":
        return {"g": normal(case, "g", (b, 1024)), "inv_sd": 1.0 / (0.5 + normal(case, "sd", (b,)).abs())}
    x = {"z": normal(case, "z", (b, 128))}  # z6 as [B][128]; the kernels read it as [128][B]
    if op == "l2_bwd":
        x["dout"] = normal(case, "dout", (b, 128))
    return x


def patch_eval(op, x):
    """The operation's outputs (a tuple) in the dtype of its inputs."""
    if op == "input_norm":
        v = x["x"]
        sd = v.std(1, unbiased=True, keepdim=True) + IN_EPS
        return ((v - v.mean(1, keepdim=True)) / sd, (1.0 / sd).flatten())
    if op == "input_norm_bwd":
        return (x["g"] * x["inv_sd"].view(-1, 1),)
    z = x["z"]
    n = ((z * z).sum(1, keepdim=True) + L2_EPS).sqrt()
    if op == "l2_fwd":
        return (z / n,)
    y = z / n
    return ((x["dout"] - y * (y * x["dout"]).sum(1, keepdim=True)) / n,)


@lru_cache(maxsize=None)
def patch_case(case):
    x = patch_inputs(case)
    ref64 = patch_eval(case[0], {k: v.double() for k, v in x.items()})
    ref32 = patch_eval(case[0], x)
    e32 = [metrics(a, r) for a, r in zip(ref32, ref64)]
    return {"x": x, "ref64": ref64, "ref32": ref32, "e32": e32, "bar": [bar_of(e) for e in e32]}


def patch_mutants(case):
    m = patch_case(case)["ref64"][0].clone()
    m[-1] = 0
    return {"last patch dropped": m}


# ------------------------------------------------------------------------------------------
def family(case):
    op = case[0].split("+")[0]
    return "conv" if op in CONV_OPS else "bn" if op.startswith("bn_") else "patch"


def case_of(case):
    return {"conv": conv_case, "bn": bn_case, "patch": patch_case}[family(case)](case)


def mutants_of(case):
    return {"conv": conv_mutants, "bn": bn_mutants, "patch": patch_mutants}[family(case)](case)


def first_output(case):
    """(ref64, e32, the case's widest bar) of the output the mutants are compared on."""
    c = case_of(case)
    if family(case) == "conv":
        return c["ref64"], c["e32"], c.get("bar_bf16x3", c["bar"])
    if case[0] == "bn_fwd" or family(case) == "patch":
        return c["ref64"][0], c["e32"][0], c["bar"][0]
    return c["ref64"], c["e32"], c["bar"]


def check(label, got, ref64, bar, e32=None):
    """Print both metrics of ``got`` next to their bars; True when both hold."""
    l2, mx = metrics(got.detach().cpu(), ref64)
    e = f"  E32 {e32[0]:.2e}/{e32[1]:.2e}" if e32 is not None else ""
    print(f"[hardnet-layer] {label}: L2 {l2:.3e} (bar {bar[0]:.3e})  max {mx:.3e} (bar {bar[1]:.3e}){e}")
    return l2 <= bar[0] and mx <= bar[1]


def check_running(label, got, ref64):
    err = float((got.detach().cpu().double() - ref64).abs().max() / max(1.0, float(ref64.abs().max())))
    print(f"[hardnet-layer] {label}: running statistic error {err:.3e} (bar {RUNNING_BAR:.0e})")
    return err <= RUNNING_BAR
