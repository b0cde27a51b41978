"""Descriptor matching without a GPU: the torch formulation of hardnetnas_amd/matching.py against the
reference's recorded results (tests/golden/fdl_match.npz, made by tests/golden/make_match_golden.py from
FDLNet-master/latency/NASNet/utils/eval_utils.py:112-197), and the argument checks of the matcher's C ABI,
which run before the GPU is touched."""
import ctypes

import pytest
import torch

from fixtures import load
from hardnetnas_amd import _native as N
from hardnetnas_amd import matching as MT

COUNT_KEYS = ("TPNN", "PNN", "TPNNT", "PNNT", "TPNNDR", "PNNDR")


def match_case(case: str):
    """(inputs as torch tensors, recorded results, metadata) of the fixture's database ``case``:
    "" = copies at noise 0.3 (every nearest distance above DES_THRSH), "close/" = copies at noise 0.05."""
    fx = load("fdl_match")
    meta = fx["meta"]
    t = {k: torch.from_numpy(fx[k]) for k in ("des1", "kp1w", "kp2", "visible")}
    t["des2"] = torch.from_numpy(fx[case + "des2"])
    ref = {k: torch.from_numpy(fx[case + k]) for k in ("nn_value", "nn_idx", "Da", "Db", "Ia", "predict_label")}
    return t, ref, dict(meta, **(meta["close"] if case else {}))


def six_counts(t, meta):
    a = (t["des1"], t["des2"], t["kp1w"], t["kp2"], t["visible"])
    return (MT.nearest_neighbor_match_score(*a, meta["COO_THRSH"])
            + MT.nearest_neighbor_threshold_match_score(*a, meta["DES_THRSH"], meta["COO_THRSH"])
            + MT.nearest_neighbor_distance_ratio_match_score(*a, meta["COO_THRSH"]))


@pytest.mark.parametrize("case", ["", "close/"])
def test_cpu_formulation_reproduces_the_reference(case):
    t, ref, meta = match_case(case)
    nn_value, nn_idx = MT._nearest(t["des1"], t["des2"])
    da, db, ia = MT._nearest2(t["des1"], t["des2"])
    assert torch.equal(nn_idx, ref["nn_idx"]) and torch.equal(ia, ref["Ia"])
    for got, want in ((nn_value, ref["nn_value"]), (da, ref["Da"]), (db, ref["Db"])):
        assert (got - want).abs().max().item() <= 1e-6
    label, nn_kp2 = MT.nearest_neighbor_distance_ratio_match(t["des1"], t["des2"], t["kp2"], meta["ratio_threshold"])
    assert torch.equal(label, ref["predict_label"]) and torch.equal(nn_kp2, t["kp2"][ref["Ia"]])
    assert six_counts(t, meta) == tuple(meta["counts"][k] for k in COUNT_KEYS)


def test_distance_matrix_vector_is_the_fdl_form():
    t, ref, _ = match_case("")
    a, b = t["des1"].double(), t["des2"].double()
    want = (2 - 2 * a @ b.t()).clamp(1e-8, 4.0).sqrt()
    assert (MT.distance_matrix_vector(a, b) - want).abs().max().item() < 1e-12
    same = MT.distance_matrix_vector(a[:3], a[:3])  # 2 - 2 a.a is inside the clamp: sqrt(1e-8)
    assert (same.diag() - 1e-4).abs().max().item() < 1e-6


def _ws(n, m):
    sz = ctypes.c_size_t()
    assert N.load_library().hn_match_workspace_bytes(n, m, ctypes.byref(sz)) == 0
    return sz.value


def test_workspace_bytes_monotone_and_covers_the_planes():
    sizes = [1, 2, 63, 64, 65, 257, 1000, 70001, 1 << 22]
    for n in sizes:
        prev = 0
        for m in sizes:
            w = _ws(n, m)
            assert w >= m * 128 * 2 * 2 and w >= prev
            prev = w
    for m in sizes:
        got = [_ws(n, m) for n in sizes]
        assert got == sorted(got)
    assert N.match_workspace_bytes(300, 257) == _ws(300, 257)
    sz = ctypes.c_size_t()
    lib = N.load_library()
    assert lib.hn_match_workspace_bytes(0, 5, ctypes.byref(sz)) == 1 and b"n_query" in lib.hn_last_error()
    assert lib.hn_match_workspace_bytes(5, (1 << 22) + 1, ctypes.byref(sz)) == 1 and b"n_db" in lib.hn_last_error()


@pytest.mark.parametrize("kw,name", [({"dim": 64}, b"dim"), ({"metric": 7}, b"metric"), ({"n_db": 0}, b"n_db"),
                                     ({"n_query": 0}, b"n_query"), ({"n_query": (1 << 22) + 1}, b"n_query")])
def test_match_nn2_rejects_bad_arguments_without_touching_gpu(kw, name):
    a = dict(n_query=8, n_db=8, dim=128, metric=0)
    a.update(kw)
    lib = N.load_library()
    rc = lib.hn_match_nn2(None, a["n_query"], None, a["n_db"], a["dim"], a["metric"], None, None, None, 1 << 30, None)
    assert rc == 1 and name in lib.hn_last_error(), lib.hn_last_error()


def test_match_nn2_rejects_a_short_workspace_without_touching_gpu():
    lib = N.load_library()
    assert lib.hn_match_nn2(None, 8, None, 8, 128, 0, None, None, None, 0, None) == 4
    assert b"workspace" in lib.hn_last_error()
    assert lib.hn_match_nn2(None, 8, None, 8, 128, 1, None, None, None, _ws(8, 8) - 1, None) == 4
    assert lib.hn_match_nn2(None, 8, None, 8, 128, 1, None, None, None, _ws(8, 8), None) == 1  # then the pointers
    assert b"NULL" in lib.hn_last_error()
