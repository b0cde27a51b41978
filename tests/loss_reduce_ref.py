"""References for loss_HardNet's 'average' and 'random' reductions (hardnet/Losses.py:87-154), shared by
test_loss_reduce_ref.py (CPU) and test_gpu_loss_reduce.py:

  formulation(...)  the reference's formulation restated in torch, in the dtype of its inputs (fp64 for the
                    reference, fp32 for the error the formulation itself carries), differentiable by autograd;
                    'random' takes its index list explicitly (the reference draws torch.randperm(B));
  closed_form(...)  the closed form the kernels implement (loss and both gradients, fp64, no autograd), pinned to
                    the formulation's autograd by test_loss_reduce_ref.py;
  reference(...)    fp64 loss and gradients of a case, with the fp32 formulation's own errors beside them;
  the case builders (ragged sizes, the exact tie, the masked near-duplicate and the zero positive distance).
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from fixtures import GOLDEN, load

REDUCES = ("average", "random")
LOSS_TYPES = ("triplet_margin", "softmax", "contrastive")
RAGGED_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 130)
# the kernels' walk over the other side is split over workgroups (hn_loss_dense.hip, dense_split): one split up to
# 64 rows, one 64-row tile per split up to 1,024 rows, two or more tiles per split beyond
SPLIT_SIZES = (1024, 1025)


def fixture():
    """loss_reduce.npz with the gradients of its three side files merged in, and a, p of loss_modes.npz."""
    fx = load("loss_reduce")
    for k in range(fx["meta"]["grad_files"]):
        z = np.load(os.path.join(GOLDEN, f"loss_reduce_grads_{k}.npz"), allow_pickle=False)
        fx.update({name: z[name] for name in z.files})
    src = load("loss_modes")
    fx["a"], fx["p"] = src["a"], src["p"]
    return fx


def case_name(reduce, swap, loss_type, margin):
    return f"{reduce}_{int(swap)}_{loss_type}_m{margin:g}"


def parse_case(name):
    reduce, swap, rest = name.split("_", 2)
    loss_type, margin = rest.rsplit("_m", 1)
    return reduce, bool(int(swap)), loss_type, float(margin)


def _terms(pos, mn, margin, loss_type):
    if loss_type == "triplet_margin":
        return torch.clamp(margin + pos - mn, min=0.0)
    if loss_type == "softmax":
        e_pos = torch.exp(2.0 - pos)
        return -torch.log(e_pos / (e_pos + torch.exp(2.0 - mn) + 1e-8))
    return torch.clamp(margin - mn, min=0.0) + pos


def formulation(a, p, swap, margin, reduce, loss_type, idx=None):
    """loss_HardNet (Losses.py:87-154) with batch_reduce 'average' or 'random', as the reference writes it."""
    b = a.size(0)
    d1 = torch.sum(a * a, dim=1).unsqueeze(-1)
    d2 = torch.sum(p * p, dim=1).unsqueeze(-1)
    d = torch.sqrt((d1.repeat(1, b) + torch.t(d2.repeat(1, b))) - 2.0 * (a @ p.t()) + 1e-6) + 1e-8
    eye = torch.eye(b, dtype=d.dtype)
    pos1 = torch.diag(d)
    dn = d + eye * 10
    mask = (dn.ge(0.008).to(dn.dtype) - 1.0) * -1
    dn = dn + mask * 10
    if reduce == "average":
        pos = pos1.repeat(b).view(-1, 1).squeeze(0)
        mn = dn.view(-1, 1)
        if swap:
            mn = torch.min(mn, torch.t(dn).contiguous().view(-1, 1))
        mn = mn.squeeze(0)
    else:
        idxs = idx.long()
        mn = dn.gather(1, idxs.view(-1, 1))
        if swap:
            mn = torch.min(mn, torch.t(dn).gather(1, idxs.view(-1, 1)))
        mn = torch.t(mn).squeeze(0)
        pos = pos1
    if reduce == "average":
        pos, mn = pos.reshape(-1), mn.reshape(-1)
    return torch.mean(_terms(pos, mn, margin, loss_type))


def _partials(pos, mn, margin, loss_type):
    """(f, df/dpos, df/dmn) elementwise, autograd's forms (clamp passes its gradient at >= 0)."""
    if loss_type == "triplet_margin":
        t = margin + pos - mn
        on = (t >= 0).to(t.dtype)
        return t.clamp(min=0.0), on, -on
    if loss_type == "softmax":
        ep, en = torch.exp(2.0 - pos), torch.exp(2.0 - mn)
        den = ep + en + 1e-8
        return -torch.log(ep / den), (en + 1e-8) / den, -en / den
    t = margin - mn
    return t.clamp(min=0.0) + pos, torch.ones_like(t), -(t >= 0).to(t.dtype)


def closed_form(a, p, swap, margin, reduce, loss_type, idx=None):
    """(loss, grad_a, grad_p) in fp64 by the closed form of the kernels: the coefficient C_ij the loss puts on
    u_ij = |a_i|^2 + |p_j|^2 - 2 a_i.p_j, then W = C / (2 sqrt(u + 1e-6)),
    grad_a = 2 rowsum(W) a - 2 W p, grad_p = 2 colsum(W) p - 2 W^T a."""
    a, p = a.double(), p.double()
    b = a.size(0)
    u = ((a * a).sum(1)[:, None] + (p * p).sum(1)[None, :]) - 2.0 * (a @ p.t())
    d = torch.sqrt(u + 1e-6) + 1e-8
    dn = d + 10.0 * torch.eye(b, dtype=d.dtype)
    dn = dn + 10.0 * (dn < 0.008).to(d.dtype)
    pos = torch.diag(d)
    s = (dn < dn.t()).to(d.dtype) + 0.5 * (dn == dn.t()).to(d.dtype)  # torch.minimum's backward
    if reduce == "average":
        m = torch.minimum(dn, dn.t()) if swap else dn
        f, dp, dm = _partials(pos[None, :].expand(b, b), m, margin, loss_type)
        g = 1.0 / (b * b)
        c = g * (s * (dm + dm.t()) if swap else dm)
        c = c + torch.diag(g * dp.sum(0))  # the positives' entries (i, i)
        loss = f.mean()
    else:
        r, t = torch.arange(b), idx.long()
        m = torch.minimum(dn[r, t], dn[t, r]) if swap else dn[r, t]
        f, dp, dm = _partials(pos, m, margin, loss_type)
        g = 1.0 / b
        fr = s[r, t] if swap else torch.ones(b, dtype=d.dtype)
        c = torch.zeros(b, b, dtype=d.dtype)
        c.index_put_((r, r), g * dp, accumulate=True)
        c.index_put_((r, t), g * dm * fr, accumulate=True)
        c.index_put_((t, r), g * dm * (1.0 - fr), accumulate=True)
        loss = f.mean()
    w = c / (2.0 * torch.sqrt(u + 1e-6))
    ga = 2.0 * w.sum(1)[:, None] * a - 2.0 * (w @ p)
    gp = 2.0 * w.sum(0)[:, None] * p - 2.0 * (w.t() @ a)
    return loss, ga, gp


def autograd_step(a, p, swap, margin, reduce, loss_type, idx, dtype):
    """(loss, [grad_a; grad_p] as fp64) of the formulation in ``dtype`` on the CPU."""
    x, y = a.to(dtype).clone().requires_grad_(True), p.to(dtype).clone().requires_grad_(True)
    loss = formulation(x, y, swap, margin, reduce, loss_type, idx)
    loss.backward()
    return float(loss.detach()), torch.cat([x.grad, y.grad]).double()


def reference(a, p, swap, margin, reduce, loss_type, idx=None):
    """fp64 loss and gradients of a case, and the fp32 formulation's own error on each."""
    l64, g64 = autograd_step(a, p, swap, margin, reduce, loss_type, idx, torch.float64)
    l32, g32 = autograd_step(a, p, swap, margin, reduce, loss_type, idx, torch.float32)
    g32err = float((g32 - g64).norm() / g64.norm()) if float(g64.norm()) > 0 else 0.0
    return SimpleNamespace(loss=l64, grad=g64, loss32=l32, g32err=g32err)


# ----------------------------------------------------------------------------------
# case builders
# ----------------------------------------------------------------------------------
def ragged_case(b, seed=0, scale=True):
    """(a, p, idx): b pairs, with ``scale`` rows scaled by factors in [0.5, 2] (nothing may assume unit norm), a
    seeded permutation for 'random'."""
    rs = np.random.RandomState(1000 + 7 * b + seed)
    a = rs.randn(b, 128)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    p = a + 0.08 * rs.randn(b, 128)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    if scale:
        a *= rs.uniform(0.5, 2.0, (b, 1))
        p *= rs.uniform(0.5, 2.0, (b, 1))
    idx = torch.from_numpy(rs.permutation(b).astype(np.int64))
    return torch.from_numpy(a.astype(np.float32)), torch.from_numpy(p.astype(np.float32)), idx


def tie_case():
    """B = 2, a = p, rows e0 and (e0 + e1) / 2: u_01 = u_10 = 0.5 exactly in fp32 and fp64, so dn_01 = dn_10 and
    torch.minimum's backward halves across the tie."""
    a = torch.zeros(2, 128)
    a[0, 0] = 1.0
    a[1, 0] = a[1, 1] = 0.5
    return a, a.clone(), torch.tensor([1, 0])


def masking_case(b, dup_row, dup_col, zero_row):
    """Unit rows (as a network's descriptors: the expanded u of an exact duplicate then stays far above -1e-6 in
    fp32) with a masked near-duplicate negative (p[dup_col] = a[dup_row]) and a zero positive distance
    (p[zero_row] = a[zero_row])."""
    a, p, idx = ragged_case(b, seed=3, scale=False)
    p[dup_col] = a[dup_row]
    p[zero_row] = a[zero_row]
    return a, p, idx
