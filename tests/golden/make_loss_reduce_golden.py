"""Generate tests/golden/loss_reduce.npz and loss_reduce_grads_{0,1,2}.npz from the REFERENCE losses.

The reference's own functions (hardnet/Losses.py: distance_matrix_vector, distance_vectors_pairwise, loss_HardNet,
loss_random_sampling, global_orthogonal_regularization; hardnet/HardNet.py: CorrelationPenaltyLoss) are
AST-extracted and exec'd on the CPU, as make_golden.py does.  Inputs: the anchors and positives of loss_modes.npz
(B = 129, with its masked near-duplicate and its zero positive distance; read, not stored again); 'random' draws
its permutation after torch.manual_seed(23), and the permutation is stored.

Cases: batch_reduce 'average' and 'random' x anchor_swap x the three loss types at margin 1.0, and triplet_margin
and contrastive at a second margin each (at margin 1.0 the contrastive clamp passes no entry of this fixture and
the triplet's nearly all).  Each stored case records the share of its entries whose clamp argument is positive
(``active_<case>``); a second-margin case outside [0.1, 0.9] is refused.  Per case: the fp64 loss, the fp64
gradients (anchors then positives, stored fp32), the reference's own fp32 loss and ``g32err``, the L2-relative
error of its fp32 gradients.  One value and gradient each of loss_random_sampling, global_orthogonal_regularization
and CorrelationPenaltyLoss on a third descriptor set (seed 23) are stored beside them.

The gradients are spread over three files so that every file stays below 1 MiB.

Run from the repository root with the reference checkout at $HN_REFERENCE (default /root/reference):
    python tests/golden/make_loss_reduce_golden.py
"""
import ast
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("HN_REFERENCE", "/root/reference")
SEED = 23
LOSS_TYPES = ("triplet_margin", "softmax", "contrastive")
GRAD_FILES = 3


def _extract(path, names):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert {n.name for n in keep} == set(names), (path, names)
    return ast.unparse(ast.Module(body=keep, type_ignores=[]))


def case_name(reduce, swap, loss_type, margin):
    return f"{reduce}_{int(swap)}_{loss_type}_m{margin:g}"


def active_share(a, p, idx, reduce, swap, loss_type, margin):
    """The share of the case's entries whose clamp argument is positive (fp64; softmax has no clamp: 1)."""
    a, p = a.double(), p.double()
    d = torch.cdist(a, p).pow(2).add(1e-6).sqrt() + 1e-8
    dn = d + 10.0 * torch.eye(len(a), dtype=d.dtype)
    dn = dn + 10.0 * (dn < 0.008)
    if reduce == "average":
        mn = torch.minimum(dn, dn.t()) if swap else dn
        pos = d.diag()[None, :].expand_as(mn)
    else:
        mn = dn[torch.arange(len(a)), idx]
        if swap:
            mn = torch.minimum(mn, dn[idx, torch.arange(len(a))])
        pos = d.diag()
    if loss_type == "triplet_margin":
        return float((margin + pos - mn > 0).double().mean())
    if loss_type == "contrastive":
        return float((margin - mn > 0).double().mean())
    return 1.0


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: the fixture can only be regenerated beside the reference checkout")
    ns = {"torch": torch, "nn": nn, "sys": sys}
    exec(_extract(os.path.join(REF, "hardnet/Losses.py"),
                  ["distance_matrix_vector", "distance_vectors_pairwise", "loss_HardNet", "loss_random_sampling",
                   "global_orthogonal_regularization"]), ns)
    exec(_extract(os.path.join(REF, "hardnet/HardNet.py"), ["CorrelationPenaltyLoss"]), ns)
    torch.Tensor.cuda = lambda self, *a, **k: self  # CPU-only fixture generation
    src = np.load(os.path.join(HERE, "loss_modes.npz"))
    a, p = torch.from_numpy(src["a"]), torch.from_numpy(src["p"])
    b = len(a)
    torch.manual_seed(SEED)
    idx = torch.randperm(b).long()  # what loss_HardNet draws after the same seed

    def run(reduce, swap, loss_type, margin, dtype):
        ag, pg = a.to(dtype).clone().requires_grad_(True), p.to(dtype).clone().requires_grad_(True)
        torch.manual_seed(SEED)
        loss = ns["loss_HardNet"](ag, pg, anchor_swap=swap, margin=margin, batch_reduce=reduce, loss_type=loss_type)
        loss.backward()
        return loss.item(), torch.cat([ag.grad, pg.grad]).double()

    def second_margin(loss_type, candidates):
        for m in candidates:
            shares = [active_share(a, p, idx, r, s, loss_type, m) for r in ("average", "random") for s in (0, 1)]
            if all(0.1 <= x <= 0.9 for x in shares):
                return m
        sys.exit(f"no second margin of {loss_type} keeps every case's active share in [0.1, 0.9]")

    margins = {"triplet_margin": second_margin("triplet_margin", [0.2, 0.25, 0.3, 0.15, 0.1]),
               "contrastive": second_margin("contrastive", [1.4, 1.35, 1.45, 1.3])}
    cases = [(r, s, lt, 1.0) for r in ("average", "random") for s in (False, True) for lt in LOSS_TYPES]
    cases += [(r, s, lt, m) for lt, m in margins.items() for r in ("average", "random") for s in (False, True)]
    out = {"idx": idx.numpy()}
    grads = [{} for _ in range(GRAD_FILES)]
    names = []
    for k, (reduce, swap, lt, margin) in enumerate(cases):
        name = case_name(reduce, swap, lt, margin)
        share = active_share(a, p, idx, reduce, swap, lt, margin)
        if margin != 1.0 and not 0.1 <= share <= 0.9:
            sys.exit(f"{name}: active share {share:.3f} outside [0.1, 0.9]")
        l64, g64 = run(reduce, swap, lt, margin, torch.float64)
        l32, g32 = run(reduce, swap, lt, margin, torch.float32)
        out[f"loss64_{name}"], out[f"loss32_{name}"] = np.float64(l64), np.float64(l32)
        out[f"g32err_{name}"] = np.float64((g32 - g64).norm() / g64.norm())
        out[f"active_{name}"] = np.float64(share)
        grads[k % GRAD_FILES][f"g_{name}"] = g64.numpy().astype(np.float32)
        names.append(name)
        print(name, l64, "active", round(share, 3), "g32err", float(out[f"g32err_{name}"]))

    # the losses beside loss_HardNet (HardNet.py:399-419) on a third descriptor set
    rs = np.random.RandomState(SEED)
    n = torch.from_numpy(rs.randn(b, 128).astype(np.float32))
    n = n / n.norm(dim=1, keepdim=True)
    out["n"] = n.numpy()

    def aux(tag, fn, *tensors):
        ts = [t.double().clone().requires_grad_(True) for t in tensors]
        v = fn(*ts)
        v.backward()
        out[f"{tag}_value"] = np.float64(v.item())
        out[f"{tag}_grad"] = torch.cat([t.grad for t in ts]).numpy().astype(np.float32)
        print(tag, v.item())

    aux("random_sampling", lambda x, y, z: ns["loss_random_sampling"](x, y, z, anchor_swap=True, margin=1.0,
                                                                      loss_type="triplet_margin"), a, p, n)
    aux("gor", ns["global_orthogonal_regularization"], a, n)
    aux("decor", ns["CorrelationPenaltyLoss"](), a)
    out["meta"] = json.dumps({"b": b, "seed": SEED, "cases": names, "grad_files": GRAD_FILES,
                              "second_margins": margins, "inputs": "loss_modes.npz a, p",
                              "source": "hardnet/Losses.py, hardnet/HardNet.py (AST-extracted, torch %s CPU)"
                                        % torch.__version__})
    np.savez_compressed(os.path.join(HERE, "loss_reduce.npz"), **out)
    for k, g in enumerate(grads):
        np.savez_compressed(os.path.join(HERE, f"loss_reduce_grads_{k}.npz"), **g)
    for f in ["loss_reduce.npz"] + [f"loss_reduce_grads_{k}.npz" for k in range(GRAD_FILES)]:
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size)
        assert size < (1 << 20), f


if __name__ == "__main__":
    main()
