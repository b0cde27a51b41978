"""The package's torch layers (``RFDet.forward_torch`` in train()) reproduce the reference's training step of
tests/golden/det_train.npz on the CPU: this pins the ground truth the GPU tests of the native step lean on."""
import numpy as np
import torch

from det_train_ref import golden, golden_detector, run_step


def test_fixture_records_its_conditions():
    _, meta, ref64, ref32 = golden()
    assert 0.0 < meta["E_score"] < 1e-4 and 0.0 < meta["E_ori"] < 1e-3 and meta["ori_excluded_share"] <= 0.01
    assert meta["grad_rel_fp32_vs_fp64"] < 1e-3 and meta["cancellation_err_over_G"] <= 1e-5
    assert {"conv.bias", "conv_ori.bias", "features.1.banch2.4.bias", "features.2.banch2.4.bias",
            "insnorm.bias"} <= set(meta["cancellation_set"])
    assert len(meta["state_dict_keys"]) == 40 and len(meta["param_names"]) == 28 and len(meta["stat_names"]) == 12
    G = float(np.sqrt(sum(float(v.norm()) ** 2 for v in ref64["grads"].values())))
    assert abs(G - meta["grad_norm_G"]) <= 1e-9 * G
    assert [k for k, v in ref64["grads"].items() if float(v.norm()) < 1e-3 * G] == meta["cancellation_set"]


def test_forward_torch_reproduces_the_reference_step():
    t, meta, ref64, _ = golden()
    det = golden_detector()
    res = run_step(det, t["images"], t["Gs"], t["Go"], det.forward_torch)
    assert list(res["grads"]) == meta["param_names"] and list(res["stats"]) == meta["stat_names"]
    assert res["nbt"] == [1] * 6
    keep = ~t["ori_excluded"]
    e_s = float((res["score"] - ref64["score"]).abs().max())
    e_o = float((res["ori"] - ref64["ori"]).abs().amax(dim=-1)[keep].max())
    G = meta["grad_norm_G"]
    e_g = float(np.sqrt(sum(float((res["grads"][k] - v).norm()) ** 2 for k, v in ref64["grads"].items()))) / G
    e_r = max(float(((res["stats"][k] - v).abs() / v.abs()).max()) for k, v in ref64["stats"].items())
    print(f"score {e_s:.3e} (E {meta['E_score']:.3e})  ori {e_o:.3e} (E {meta['E_ori']:.3e})  grads {e_g:.3e}  "
          f"running statistics {e_r:.3e}")
    assert e_s <= 4.0 * meta["E_score"] and e_o <= 4.0 * meta["E_ori"]
    assert e_g <= 1e-3
    assert e_r <= 1e-5
    assert torch.equal(det.scale_list, torch.tensor([32.0]))
