"""Shared by the NAS / FDLNet train-path shape tests (tests/test_gpu_nas_train_shapes.py, tests/test_nas_train_ref.py)
and tests/test_gpu_des_input_grad.py: the cases, the step, its fp64 / fp32 CPU references, the bars, and the C ABI
calls with guarded workspaces.

A case is (model, B): ``model`` is "op:<name>" (HardNetNAS([name] * 6) with splitmix64 weights and fresh BatchNorm
buffers), one of the golden architectures of tests/fixtures.py (cov_b, wang2, wang3, fdl_NASNet, fdl_NASNet_01) or
"supernet" (fixtures.supernet_start, soft weights from the fixture's recorded Gumbel noise as in
fixtures.supernet_step).  The step is one train() call on ``synth.synth_patches(B, seed)`` and the backward of the
smooth objective ``(y * c).sum()`` with c = synth.normal (loss_HardNet's hardest-negative mining has ties and kinks
of its own).  A result is a dict: y [B,128], grads {name: tensor}, stats {name: running statistic after the step},
nbt (by how much every num_batches_tracked rose), dx (the input gradient or None), thetas (the supernet's stacked
thetas gradient or None), node (y's grad_fn name); everything fp64 on the CPU.

The references are the module's own torch layers, deep-copied to fp64 (``ref64``, the truth) and to fp32 (``ref32``,
the yardstick: its distance from ref64 is what a correct fp32 implementation costs on that input) on the CPU.

The bars (``check_step``) are nas_grad_check's rule (tests/fixtures.py) restated for full tensors:
  descriptors max abs error <= max(1e-4, 3 E32_y); running statistics 1e-5 relative to max(1, the tensor's largest
  magnitude); all parameter gradients together L2-relative <= max(5e-3, 3 E32_all); every single tensor (and the
  input gradient) <= max(2e-2, 3 E32_k); a tensor whose fp64 norm is below 1e-9 of the largest is held in absolute
  terms to 1e-6 of that largest norm.
``ref_conditions`` are what keeps the 3 E32 terms from hiding a failure; tests/test_nas_train_ref.py asserts them
for every case without a GPU.  The seeds below were chosen on the CPU references alone so that they hold."""
import copy
import ctypes
from functools import lru_cache

import numpy as np
import torch

from fixtures import build_module, load, supernet_start
from hardnetnas_amd import arch as A
from hardnetnas_amd import synth
from hardnetnas_amd.model import HardNetNAS

FDL = ["fdl_NASNet", "fdl_NASNet_01"]
SHIPPED = ["cov_b", "wang3", "wang2"] + FDL
OP_BATCH = 5
RAGGED = [3, 6, 37]
OP_WEIGHT_SEED = 4321
C_SEED = 77
TINY = 1e-9

# the patch seed of every case: 300 + B unless listed here.  Chosen on the CPU references alone so that
# ref_conditions holds: at seed 305 the fp32 CPU layers of ir_k5_e3_se land on the other side of a ReLU kink from
# fp64 (E32_all 1.7e-3, stages.4.pw.bn.bias 6e-3); 306 is the next seed and measures 6.5e-6.
SEEDS = {("op:ir_k5_e3_se", 5): 306}

OP_CASES = [(f"op:{op}", OP_BATCH) for op in A.CANDIDATE_BLOCKS]
RAGGED_CASES = [(name, b) for name in SHIPPED for b in RAGGED]
B2_CASES = [("cov_b", 2), ("fdl_NASNet", 2)]
SUPERNET_CASE = ("supernet", 5)
FULL_CASES = OP_CASES + RAGGED_CASES + [SUPERNET_CASE]
ALL_CASES = FULL_CASES + B2_CASES


def case_id(case):
    return f"{case[0].replace('op:', '')}-B{case[1]}"


def case_seed(model, b):
    return SEEDS.get((model, b), 300 + b)


def make_module(model):
    """The case's module in train() on the CPU in fp32 at its starting point."""
    if model == "supernet":
        return supernet_start()[0].train()
    if model.startswith("op:"):
        m = HardNetNAS([model[3:]] * 6)
        sd = m.state_dict()
        tmpl = {k: tuple(v.shape) for k, v in sd.items()}
        sd.update({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(tmpl, OP_WEIGHT_SEED).items()})
        m.load_state_dict(sd)
        return m.train()
    return build_module(model)[0].train()


def case_inputs(model, b):
    """(x [B,1,32,32], c [B,128]) fp32 on the CPU."""
    x = torch.from_numpy(synth.synth_patches(b, seed=case_seed(model, b)))
    c = torch.from_numpy(synth.normal(C_SEED + b, b * 128).reshape(b, 128).astype(np.float32))
    return x, c


def supernet_soft(m, dev, dtype):
    """softmax((thetas + g) / T) with the fixture's recorded noise for outs_X (fixtures.supernet_step)."""
    fx = load("train_nas")
    g = torch.from_numpy(fx["super/noise"][:6]).to(dev, dtype)
    thetas = torch.stack([st.thetas for st in m.stages_to_search])
    return ((thetas + g) / fx["meta"]["supernet"]["temperature"]).softmax(-1)


def run_step(model, m, x, c, need_dx=False, soft=None):
    """One step of ``m`` (already on x's device in x's dtype, in train()): see the module docstring.  ``soft``
    replaces the supernet's noise-derived soft weights."""
    nbt0 = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    xi = x.clone().requires_grad_(need_dx)
    if model == "supernet":
        if soft is None:
            soft = supernet_soft(m, x.device, x.dtype)
        lat0 = torch.zeros((1, 1), device=x.device, dtype=x.dtype, requires_grad=True)
        temperature = load("train_nas")["meta"]["supernet"]["temperature"]
        y = m(xi, temperature, lat0, soft_weights=soft)[0]
    else:
        y = m(xi)
    (y * c).sum().backward()
    f = lambda t: t.detach().double().cpu()  # noqa: E731
    sd = m.state_dict()
    thetas = [p.grad for k, p in m.named_parameters() if k.endswith(".thetas")]
    return {"node": type(y.grad_fn).__name__, "y": f(y),
            "grads": {k: f(p.grad) for k, p in m.named_parameters() if not k.endswith(".thetas")},
            "stats": {k: f(v) for k, v in sd.items() if "running" in k},
            "nbt": {k: int(sd[k]) - n for k, n in nbt0.items()},
            "dx": f(xi.grad) if need_dx else None,
            "thetas": f(torch.stack(thetas)) if thetas and thetas[0] is not None else None}


def needs_dx(model):
    return model in FDL


@lru_cache(maxsize=None)
def cpu_refs(model, b):
    """(ref64, ref32) of a case; computed once per process and never modified."""
    x, c = case_inputs(model, b)
    ref64 = run_step(model, make_module(model).double(), x.double(), c.double(), needs_dx(model))
    ref32 = run_step(model, make_module(model), x, c, needs_dx(model))
    return ref64, ref32


def gpu_step(model, b, dev, soft=None):
    """The case's step on the native path."""
    x, c = case_inputs(model, b)
    m = make_module(model).to(dev)
    return run_step(model, m, x.to(dev), c.to(dev), needs_dx(model), soft)


def _norm(t):
    return float(t.norm())


def grad_errors(grads, g64):
    """(global, per, tiny, scale) of a {name: gradient} against the fp64 one: ``global`` the L2-relative error of
    all tensors taken together, ``per`` {name: L2-relative error}, ``tiny`` {name: ||g|| / scale} for the tensors
    whose fp64 norm is below 1e-9 of ``scale``, the largest fp64 norm (they enter neither of the other two)."""
    scale = max(_norm(g) for g in g64.values())
    per, tiny, num, den = {}, {}, 0.0, 0.0
    for k, ref in g64.items():
        n = _norm(ref)
        if n < TINY * scale:
            tiny[k] = _norm(grads[k]) / scale
            continue
        e = _norm(grads[k] - ref)
        per[k] = e / n
        num += e * e
        den += n * n
    return float(np.sqrt(num / den)), per, tiny, scale


def stat_error(stats, s64):
    return max(float((stats[k] - ref).abs().max()) / max(1.0, float(ref.abs().max())) for k, ref in s64.items())


def rel(a, ref):
    return _norm(a - ref) / _norm(ref)


def figures(res, ref64):
    """Every error figure of a result against the fp64 reference."""
    glob, per, tiny, scale = grad_errors(res["grads"], ref64["grads"])
    out = {"y": float((res["y"] - ref64["y"]).abs().max()), "stat": stat_error(res["stats"], ref64["stats"]),
           "all": glob, "per": per, "tiny": tiny, "scale": scale}
    if ref64["dx"] is not None:
        out["dx"] = rel(res["dx"], ref64["dx"])
    if ref64["thetas"] is not None:
        out["thetas"] = rel(res["thetas"], ref64["thetas"])
    return out


def ref_conditions(model, b):
    """The figures of ref32 against ref64 and the list of the conditions they miss (empty: the bars of check_step
    mean what they say for this case)."""
    ref64, ref32 = cpu_refs(model, b)
    e = figures(ref32, ref64)
    over = [k for k, v in e["per"].items() if 3.0 * v > 2e-2]
    bad = []
    if e["y"] > 3e-5:
        bad.append(f"E32_y {e['y']:.2e} > 3e-5")
    if b >= 3:  # B = 2 holds its gradients in absolute terms: no 3 E32 bar to protect
        if e["all"] > 1.6e-3:
            bad.append(f"E32_all {e['all']:.2e} > 1.6e-3")
        if 10 * len(over) > len(e["per"]):
            bad.append(f"{len(over)} of {len(e['per'])} tensors have 3 E32_k > 2e-2: {over[:4]}")
        if e.get("thetas", 0.0) > 1.6e-3:
            bad.append(f"E32_thetas {e['thetas']:.2e} > 1.6e-3")
    return e, bad


def check_step(res, model, b, label=None):
    """Print the native step's errors beside ref32's and hold them to the bars (module docstring)."""
    ref64, ref32 = cpu_refs(model, b)
    label = label or case_id((model, b))
    e, e32 = figures(res, ref64), figures(ref32, ref64)
    worst = max(e["per"], key=lambda k: e["per"][k] / max(2e-2, 3.0 * e32["per"][k]))
    line = (f"{label}: descriptors {e['y']:.2e} (fp32 CPU {e32['y']:.2e}); running statistics {e['stat']:.2e} "
            f"({e32['stat']:.2e}); gradients, all {e['all']:.2e} ({e32['all']:.2e}), worst tensor "
            f"{e['per'][worst]:.2e} ({e32['per'][worst]:.2e}) at {worst}")
    for k in ("dx", "thetas"):
        if k in e:
            line += f"; {k} {e[k]:.2e} ({e32[k]:.2e})"
    if e["tiny"]:
        line += f"; {len(e['tiny'])} cancelled tensors, largest {max(e['tiny'].values()):.2e} of the scale"
    print(line)
    assert set(res["grads"]) == set(ref64["grads"])
    assert e["y"] <= max(1e-4, 3.0 * e32["y"]), ("descriptors", e["y"], e32["y"])
    assert e["stat"] <= 1e-5, ("running statistics", e["stat"])
    assert all(v == 1 for v in res["nbt"].values()) and len(res["nbt"]) == len(ref64["nbt"]), res["nbt"]
    assert e["all"] <= max(5e-3, 3.0 * e32["all"]), ("all gradients", e["all"], e32["all"])
    for k, v in e["per"].items():
        assert v <= max(2e-2, 3.0 * e32["per"][k]), (k, v, e32["per"][k])
    for k, v in e["tiny"].items():
        assert v <= 1e-6, (k, v)
    if "dx" in e:
        assert e["dx"] <= max(2e-2, 3.0 * e32["dx"]), ("input gradient", e["dx"], e32["dx"])
    if "thetas" in e:
        assert e["thetas"] <= max(5e-3, 3.0 * e32["all"]), ("thetas", e["thetas"], e32["thetas"])
    return e, e32


def check_step_b2(res, model):
    """B = 2: descriptors and running statistics to the bars; every gradient in absolute terms,
    ||g - g64|| <= max(3 ||g32 - g64||, 1e-6 x the B = 3 case's largest gradient norm) -- with two samples the head
    BatchNorm's z is +-d / sqrt(d^2 + eps), its backward cancels to the eps / (d^2 + eps) that is left (rounding
    noise in fp32 wherever the two samples differ by more than sqrt(eps)), so a relative bar would mean nothing."""
    ref64, ref32 = cpu_refs(model, 2)
    scale3 = max(_norm(g) for g in cpu_refs(model, 3)[0]["grads"].values())
    e_y, e32_y = float((res["y"] - ref64["y"]).abs().max()), float((ref32["y"] - ref64["y"]).abs().max())
    e_s = stat_error(res["stats"], ref64["stats"])
    todo = [(k, res["grads"][k], ref64["grads"][k], ref32["grads"][k]) for k in ref64["grads"]]
    if ref64["dx"] is not None:
        todo.append(("input", res["dx"], ref64["dx"], ref32["dx"]))
    errs = {k: (_norm(g - g64), _norm(g32 - g64)) for k, g, g64, g32 in todo}
    worst = max(errs, key=lambda k: errs[k][0] / max(3.0 * errs[k][1], 1e-6 * scale3))
    print(f"{model}-B2: descriptors {e_y:.2e} (fp32 CPU {e32_y:.2e}); running statistics {e_s:.2e}; gradients in "
          f"absolute terms, floor {1e-6 * scale3:.2e}: worst {errs[worst][0]:.2e} ({errs[worst][1]:.2e}) at {worst}; "
          f"largest fp64 gradient norm {max(_norm(g) for g in ref64['grads'].values()):.2e}, at B = 3 {scale3:.2e}")
    assert e_y <= max(1e-4, 3.0 * e32_y), ("descriptors", e_y, e32_y)
    assert e_s <= 1e-5, ("running statistics", e_s)
    assert all(v == 1 for v in res["nbt"].values()), res["nbt"]
    for k, (e, e32) in errs.items():
        assert e <= max(3.0 * e32, 1e-6 * scale3), (k, e, e32)


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def raw_step(m, x, v, entry, din=None):
    """One hn_nas_train_forward + backward through the C ABI on clones of the module's tensors: ``entry`` is
    "hn_nas_train_backward" or "hn_nas_train_backward_dx" (with ``din``, a tensor or None).  Returns the
    gradient buffers of every tensor slot."""
    from hardnetnas_amd import _native as N
    lib = N.load_library()
    dev, b = x.device, x.shape[0]
    desc = N.desc_for_module(m)
    ts = [t.detach().clone() for t in N.train_tensors(m)[1]]
    sv, sc = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.hn_nas_train_workspace_bytes(ctypes.byref(desc), b, ctypes.byref(sv), ctypes.byref(sc)) == 0
    saved = torch.empty(sv.value, device=dev, dtype=torch.uint8)
    scratch = torch.empty(sc.value, device=dev, dtype=torch.uint8)
    out = torch.empty((b, 128), device=dev)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rc = lib.hn_nas_train_forward(ctypes.byref(desc), x.data_ptr(), b, ptrs, 0.1, None, out.data_ptr(),
                                  saved.data_ptr(), saved.numel(), scratch.data_ptr(), scratch.numel(), None)
    assert rc == 0, lib.hn_last_error()
    grads = [torch.zeros_like(t) for t in ts]
    gp = (ctypes.c_void_p * len(ts))(*[g.data_ptr() for g in grads])
    head = (ctypes.byref(desc), v.data_ptr(), x.data_ptr(), b, ptrs, None, gp, None)
    tail = (saved.data_ptr(), saved.numel(), scratch.data_ptr(), scratch.numel(), None)
    if entry == "hn_nas_train_backward":
        rc = lib.hn_nas_train_backward(*head, *tail)
    else:
        rc = lib.hn_nas_train_backward_dx(*head, din.data_ptr() if din is not None else None, *tail)
    assert rc == 0, lib.hn_last_error()
    torch.cuda.synchronize()
    return grads


CANARY, GUARD = 0xA5, 256


def guarded(nbytes, dev, fill):
    """A uint8 tensor of ``nbytes`` (rounded up to 16) filled with ``fill`` inside a larger allocation with 256
    canary bytes either side: (whole, view)."""
    n = (nbytes + 15) // 16 * 16
    whole = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    whole[GUARD:GUARD + n] = fill
    return whole, whole[GUARD:GUARD + n]


def intact(whole):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all())


def abi_step(m, x, v, soft=None, need_din=False, fill=None):
    """hn_nas_train_forward + hn_nas_train_backward_dx through the C ABI on clones of the module's tensors, with a
    scratch region of its own for the backward (nothing is carried over from the forward except ``saved``).
    ``soft`` ([6, 17]): the supernet, with d_dsoft.  ``fill`` None: plain torch.empty buffers; a byte value:
    saved, both scratch regions, the output, every gradient buffer, d_din and d_dsoft each sit between canaries and
    are pre-filled with that byte.  Returns {"out", "grads" (None for the running statistics' slots), "tensors"
    (the clones, running statistics updated), "din", "dsoft", "holders" (the guarded allocations)}."""
    from hardnetnas_amd import _native as N
    lib = N.load_library()
    dev, b = x.device, x.shape[0]
    desc = N.supernet_desc() if soft is not None else N.desc_for_module(m)
    names, ts = N.train_tensors(m)
    ts = [t.detach().clone() for t in ts]
    holders = []

    def buf(nbytes):
        if fill is None:
            return torch.empty((nbytes + 15) // 16 * 16, device=dev, dtype=torch.uint8)
        whole, view = guarded(nbytes, dev, fill)
        holders.append(whole)
        return view

    def floats(shape):
        n = int(np.prod(shape))
        return buf(4 * n).view(torch.float32)[:n].view(shape)

    sv, sc = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.hn_nas_train_workspace_bytes(ctypes.byref(desc), b, ctypes.byref(sv), ctypes.byref(sc)) == 0
    saved, scratch_f, scratch_b = buf(sv.value), buf(sc.value), buf(sc.value)
    out = floats((b, 128))
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    soft_p = soft.data_ptr() if soft is not None else None
    rc = lib.hn_nas_train_forward(ctypes.byref(desc), x.data_ptr(), b, ptrs, 0.1, soft_p, out.data_ptr(),
                                  saved.data_ptr(), sv.value, scratch_f.data_ptr(), sc.value, None)
    assert rc == 0, lib.hn_last_error()
    grads = [None if "running" in k else floats(tuple(t.shape)) for k, t in zip(names, ts)]
    gp = (ctypes.c_void_p * len(ts))(*[g.data_ptr() if g is not None else None for g in grads])
    din = floats((b, 1, 32, 32)) if need_din else None
    dsoft = floats((6, 17)) if soft is not None else None
    rc = lib.hn_nas_train_backward_dx(ctypes.byref(desc), v.data_ptr(), x.data_ptr(), b, ptrs, soft_p, gp,
                                      dsoft.data_ptr() if dsoft is not None else None,
                                      din.data_ptr() if din is not None else None, saved.data_ptr(), sv.value,
                                      scratch_b.data_ptr(), sc.value, None)
    assert rc == 0, lib.hn_last_error()
    torch.cuda.synchronize()
    return {"out": out, "grads": grads, "tensors": ts, "names": names, "din": din, "dsoft": dsoft,
            "holders": holders}
