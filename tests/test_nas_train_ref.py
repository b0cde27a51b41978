"""The references of tests/test_gpu_nas_train_shapes.py, without a GPU: for every case of that file the fp32 CPU
layers' own error against the fp64 ones (tests/nas_train_ref.py) is small enough that the ``3 x E32`` terms of the
bars cannot hide a failure -- E32_all <= 1.6e-3 (so the global gradient bar is 5e-3), at most one tensor in ten with
3 E32_k > 2e-2, E32_y <= 3e-5 (so the descriptor bar is 1e-4) -- and the references are what they claim to be."""
import pytest
import torch

import nas_train_ref as R


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_reference_conditions(case):
    model, b = case
    e, bad = R.ref_conditions(model, b)
    print(f"{R.case_id(case)}: E32_y {e['y']:.2e}, E32_all {e['all']:.2e}, largest E32_k {max(e['per'].values()):.2e}, "
          f"{len(e['tiny'])} cancelled of {len(e['per']) + len(e['tiny'])} tensors")
    assert not bad, bad
    # the fp32 layers meet the running-statistics bar themselves, and their cancelled tensors the absolute one
    assert e["stat"] <= 1e-5
    assert all(v <= 1e-6 for v in e["tiny"].values()), e["tiny"]


def test_cases_are_the_issue_s():
    """17 ops at B = 5; five shipped architectures at 3, 6 and 37; B = 2; the supernet at 5; nothing above 37."""
    from hardnetnas_amd import arch as A
    assert [m for m, _ in R.OP_CASES] == ["op:" + op for op in A.CANDIDATE_BLOCKS] and {b for _, b in R.OP_CASES} == {5}
    assert sorted(R.RAGGED_CASES) == sorted((n, b) for n in ("cov_b", "wang3", "wang2", "fdl_NASNet", "fdl_NASNet_01")
                                            for b in (3, 6, 37))
    assert R.B2_CASES == [("cov_b", 2), ("fdl_NASNet", 2)] and R.SUPERNET_CASE == ("supernet", 5)
    assert max(b for _, b in R.ALL_CASES) == 37 and len(set(R.ALL_CASES)) == len(R.ALL_CASES)


def test_references_are_fp64_and_fp32_runs_of_the_torch_layers():
    """ref64 and ref32 come from the module's torch layers (no native node), differ (two precisions), carry every
    parameter's gradient, the input gradient for the FDLNet models and the thetas' for the supernet; the skip arch
    has SKIP_MP, SKIP_ID and SKIP_MPCONV (no parameters at layers 0, 1, 3, 5; a 1x1 ConvBNRelu at 2 and 4)."""
    for model, b in (("op:skip", 5), ("fdl_NASNet", 3), R.SUPERNET_CASE):
        ref64, ref32 = R.cpu_refs(model, b)
        m = R.make_module(model)
        want = {k for k, _ in m.named_parameters() if not k.endswith(".thetas")}
        for ref in (ref64, ref32):
            assert "NasTrainFunction" not in ref["node"]
            assert set(ref["grads"]) == want and tuple(ref["y"].shape) == (b, 128)
            assert all(v == 1 for v in ref["nbt"].values()) and ref["nbt"]
            assert (ref["dx"] is not None) == (model in R.FDL) and (ref["thetas"] is not None) == (model == "supernet")
        assert not torch.equal(ref64["y"], ref32["y"]) and float((ref64["y"] - ref32["y"]).abs().max()) < 1e-4
    stages = {k.split(".")[1] for k in R.cpu_refs("op:skip", 5)[0]["grads"] if k.startswith("stages.")}
    assert stages == {"2", "4"}
    assert tuple(R.cpu_refs("supernet", 5)[0]["thetas"].shape) == (6, 17)


def test_the_bars_catch_a_dropped_contribution():
    """check_step on a result that is ref32 with one weight gradient's last row zeroed, or one descriptor row
    perturbed by 1e-3, fails; on ref32 itself it passes."""
    model, b = "cov_b", 6
    _, ref32 = R.cpu_refs(model, b)
    R.check_step(ref32, model, b, "ref32 as the result")
    broken = dict(ref32, grads=dict(ref32["grads"]))
    g = ref32["grads"]["stages.5.pwl.conv.weight"].clone()
    g[-1] = 0
    broken["grads"]["stages.5.pwl.conv.weight"] = g
    with pytest.raises(AssertionError):
        R.check_step(broken, model, b, "last row dropped")
    y = ref32["y"].clone()
    y[-1] += 1e-3
    with pytest.raises(AssertionError):
        R.check_step(dict(ref32, y=y), model, b, "descriptor moved")
