"""The NAS / FDLNet train path (hn_nas_train_*: the sampled hardnetNAS nets, the supernet, FDLNet's HardNetNeiMask)
per op and at ragged batches, against the same module's torch layers in fp64 on the CPU (tests/nas_train_ref.py).

tests/test_gpu_nas_train.py and tests/test_gpu_des_input_grad.py check batches that are multiples of 32, where every
row length L = B hw^2 is a multiple of the GEMM's 128-column tile and of its 32-deep K step, every BatchNorm slice is
exact and no four-patch workgroup is partial.  Here:
  B = 5 for each of the 17 CANDIDATE_BLOCKS at all six layers (head L = 5: the scalar BatchNorm branch; SE GEMMs with
  N = K = 5; partial last workgroup of the four-per-workgroup kernels; L = 5120 at 32x32: two BatchNorm slices with
  an inexact ``per``) and for the supernet's batched launches;
  B = 3, 6, 37 on the shipped architectures (N = 48 / 96: one partial tile; N = 592: four tiles and one of 80 columns;
  K = 48 and 592: a ragged last K step and split-K slice; ten BatchNorm slices; five k_wgrad0 slice groups);
  B = 2, the smallest native batch; one-hot soft weights (the supernet's batched kernels against the sampled path's
  single ones, bit for bit); guarded and pre-filled workspaces; determinism.

The bars are nas_train_ref.check_step's: the project's own (fixtures.nas_grad_check) on full tensors, with ``3 x`` the
fp32 CPU layers' own error as the only other term; tests/test_nas_train_ref.py proves without a GPU that this term
stays below the fixed bars (global 5e-3, descriptors 1e-4) in every case.  Every test prints the HIP error and the
fp32 CPU error side by side."""
import pytest
import torch

import nas_train_ref as R
from fixtures import load
from hardnetnas_amd import _native as N
from hardnetnas_amd import arch as A
from hardnetnas_amd.model import HardNetNAS

pytestmark = pytest.mark.gpu
NODE = "NasTrainFunction"


@pytest.mark.parametrize("case", R.OP_CASES, ids=R.case_id)
def test_every_op_at_every_layer_sampled_path(case, cuda_device):
    """HardNetNAS([op] * 6) at B = 5: the op at all six (C_in, C_out, stride) entries of SEARCH_SPACE2 on the sampled
    path's own launch sequence; ["skip"] * 6 is SKIP_MP, SKIP_ID and SKIP_MPCONV.  The per-tensor bar names the layer."""
    res = R.gpu_step(*case, cuda_device)
    assert NODE in res["node"]
    R.check_step(res, *case)


@pytest.mark.parametrize("case", R.RAGGED_CASES, ids=R.case_id)
def test_ragged_batches_on_the_shipped_architectures(case, cuda_device):
    """cov_b, wang3, wang2 and the two FDLNet descriptors at B = 3 (the smallest batch whose head BatchNorm backward
    is not identically zero), 6 (even, no multiple of 4) and 37; the FDLNet models with the input requiring grad
    (k_dgrad0's per-patch launch at an odd batch), the input gradient held to the single-tensor bar.  Measured:
    everything at 1e-6 .. 7e-5 except wang2 at 37 (all gradients 1.8e-3, stages.3.pw.bn.bias 1.0e-2): one ReLU
    pre-activation of stages.3.pw is -1.0e-7 in fp64 and the kernels' fp32 value lands on the other side; flipping
    it in the fp64 CPU module reproduces both figures."""
    res = R.gpu_step(*case, cuda_device)
    assert NODE in res["node"]
    assert (res["dx"] is not None) == (case[0] in R.FDL)
    R.check_step(res, *case)


@pytest.mark.parametrize("case", R.B2_CASES, ids=R.case_id)
def test_smallest_native_batch(case, cuda_device):
    """B = 2: descriptors and running statistics to the bars, every gradient in absolute terms
    (nas_train_ref.check_step_b2)."""
    res = R.gpu_step(*case, cuda_device)
    assert NODE in res["node"]
    R.check_step_b2(res, case[0])


def test_supernet_at_an_odd_batch(cuda_device):
    """The batched path (BnBatcher, PwBatcher, k_dw_fwd_multi, k_dot_part) at B = 5: all 17 ops x 6 layers, soft
    weights from the fixture's recorded noise, every parameter's gradient and the thetas' (through the native soft-weight
    gradient and the softmax) against the fp64 CPU module."""
    res = R.gpu_step(*R.SUPERNET_CASE, cuda_device)
    assert NODE in res["node"] and res["thetas"] is not None
    R.check_step(res, *R.SUPERNET_CASE)


def cov_b_ops():
    return list(load("nas_cov_b")["meta"]["ops"])


def with_skips():
    """cov_b's ops with ``skip`` at layers 0 (SKIP_MP), 3 (SKIP_ID) and 4 (SKIP_MPCONV)."""
    ops = cov_b_ops()
    for i in (0, 3, 4):
        ops[i] = "skip"
    return ops


@pytest.mark.parametrize("pattern", [cov_b_ops, with_skips], ids=["cov_b", "with_skips"])
def test_one_hot_soft_weights_give_the_sampled_path_bit_for_bit(pattern, cuda_device):
    """Soft weights exactly one-hot on op j_i at layer i: the mix is 1 * a plus fmaf(0, v, .) terms and the batched
    kernels (k_bn_part_multi, k_dw_fwd_multi, k_gemm_pw_batch) claim the single kernels' bits, so the supernet and a
    HardNetNAS of that arch with the chosen ops' weights agree bit for bit in descriptors, the chosen ops' running
    statistics and parameter gradients at B = 6; every gradient of an op with weight 0 is exactly zero (anything else
    is a leak from one op into another)."""
    dev, b, ops = cuda_device, 6, pattern()
    idx = [A.CANDIDATE_BLOCKS.index(op) for op in ops]
    sup = R.make_module("supernet")
    nas = HardNetNAS(ops)
    nas.load_supernet_state_dict(sup.state_dict())
    x, c = R.case_inputs("one-hot", b)
    soft = torch.zeros(6, 17)
    soft[torch.arange(6), torch.tensor(idx)] = 1.0
    rs = R.run_step("supernet", sup.to(dev), x.to(dev), c.to(dev), soft=soft.to(dev))
    rn = R.run_step("nas", nas.train().to(dev), x.to(dev), c.to(dev))
    assert NODE in rs["node"] and NODE in rn["node"]

    def sup_key(k):
        p = k.split(".")
        return ".".join(["stages_to_search", p[1], "ops", str(idx[int(p[1])])] + p[2:]) if p[0] == "stages" else k

    e_y = float((rs["y"] - rn["y"]).abs().max())
    diff = [k for k, g in rn["grads"].items() if not torch.equal(g, rs["grads"][sup_key(k)])]
    sdiff = [k for k, s in rn["stats"].items() if not torch.equal(s, rs["stats"][sup_key(k)])]
    chosen = {sup_key(k) for k in rn["grads"]}
    leaks = [k for k, g in rs["grads"].items() if k not in chosen and not bool((g == 0).all())]
    worst = max([R.rel(rs["grads"][sup_key(k)], rn["grads"][k]) for k in diff], default=0.0)
    print(f"one-hot {ops}: descriptors differ by {e_y:.2e}; {len(diff)} of {len(rn['grads'])} gradients differ (worst "
          f"L2-rel {worst:.2e}) {diff[:4]}; {len(sdiff)} running statistics differ {sdiff[:4]}; "
          f"{len(leaks)} of {len(rs['grads']) - len(chosen)} unchosen gradients nonzero {leaks[:4]}")
    assert not leaks
    assert torch.equal(rs["y"], rn["y"])
    assert not sdiff and not diff
    assert max(float(g.abs().max()) for g in rn["grads"].values()) > 0


GUARD_MODELS = ["cov_b", "wang3", "fdl_NASNet", "supernet"]
_plain = {}


def abi_case(model, dev, fill):
    m = R.make_module(model).to(dev)
    x, v = R.case_inputs(model, 5)
    soft = R.supernet_soft(m, dev, torch.float32).detach().contiguous() if model == "supernet" else None
    return R.abi_step(m, x.to(dev), v.to(dev), soft, need_din=model in R.FDL, fill=fill)


@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["zeros", "nans"])
@pytest.mark.parametrize("model", GUARD_MODELS)
def test_workspace_guards_and_prefill(model, fill, cuda_device):
    """hn_nas_train_forward / _backward_dx through the C ABI at B = 5 with ``saved``, the forward's and the backward's
    own ``scratch``, the output, every gradient buffer, d_din (FDLNet) and d_dsoft (the supernet) each between 256
    canary bytes and pre-filled with 0x00 or 0xFF (every float a NaN): the canaries stay intact and the descriptors,
    gradients and updated running statistics are the plain call's bit for bit -- every byte that is read was written
    by the same call, also by the kernels that accumulate into their output."""
    if model not in _plain:
        _plain[model] = abi_case(model, cuda_device, None)
    want, got = _plain[model], abi_case(model, cuda_device, fill)
    assert got["holders"] and all(R.intact(w) for w in got["holders"])
    assert bool(torch.isfinite(want["out"]).all()) and torch.equal(got["out"], want["out"])
    for k, g, gw, t, tw in zip(got["names"], got["grads"], want["grads"], got["tensors"], want["tensors"]):
        assert (g is None) == ("running" in k)
        assert torch.equal(t, tw), k
        if g is not None:
            assert torch.equal(g, gw), k
    for k in ("din", "dsoft"):
        assert (got[k] is None) == (want[k] is None)
        if got[k] is not None:
            assert bool(torch.isfinite(want[k]).all()) and float(want[k].abs().max()) > 0
            assert torch.equal(got[k], want[k]), k
    assert (got["din"] is not None) == (model in R.FDL) and (got["dsoft"] is not None) == (model == "supernet")
    start = dict(zip(*N.train_tensors(R.make_module(model))))
    for k, t in zip(want["names"], want["tensors"]):  # the running statistics were updated, nothing else was
        assert torch.equal(t.cpu(), start[k]) == ("running" not in k), k


@pytest.mark.parametrize("case", [("cov_b", 37), R.SUPERNET_CASE], ids=R.case_id)
def test_two_steps_from_one_start_are_bit_identical(case, cuda_device):
    """No atomics, every reduction in a fixed order: descriptors, gradients, running statistics and the thetas'
    gradient of two steps from the same start are the same bits."""
    a, b = R.gpu_step(*case, cuda_device), R.gpu_step(*case, cuda_device)
    assert NODE in a["node"] and torch.equal(a["y"], b["y"])
    for part in ("grads", "stats"):
        assert a[part].keys() == b[part].keys()
        for k, t in a[part].items():
            assert torch.equal(t, b[part][k]), k
    if a["thetas"] is not None:
        assert torch.equal(a["thetas"], b["thetas"])
