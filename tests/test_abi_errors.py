"""Every argument check of the model-less C ABI (hn_api_det.hip, hn_api_train.hip, hn_api_ops.hip) and of
hn_param_count: return code, message and the order of the checks, against what the library answered before the entry
points were split over those files (tests/abi_error_cases.py, tests/golden/abi_errors.json).  No case reaches a
launch, so none needs a GPU; with one present the module skips, because the placeholder pointers of the table must
never be able to reach a device."""
import json

import pytest
import torch

import abi_error_cases as C

if torch.cuda.is_available():
    pytest.skip("placeholder device pointers: runs on machines without a GPU only", allow_module_level=True)

CASES = C.cases()
with open(C.GOLDEN) as f:
    GOLDEN = json.load(f)


def test_table_and_golden_file_cover_each_other():
    assert sorted(c[0] for c in CASES) == sorted(GOLDEN)
    fns = {c[1] for c in CASES}
    assert fns == set(C.SPEC) and fns <= set(C.N.EXPORTED)
    assert any("+" in c[0] for c in CASES if c[1] == "hn_select_keypoints")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_check(case):
    rc, msg = C.run(case)
    assert rc in (0, 1, 4), (rc, msg)  # HN_OK, HN_ERR_ARG, HN_ERR_WORKSPACE: anything else went past the checks
    assert [rc, msg] == GOLDEN[case[0]]
