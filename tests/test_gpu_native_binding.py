"""The binding's call helpers where only a GPU call shows them (``_native._workspace``'s three policies for a
supplied buffer one byte short, ``_aligned16`` in front of a launch, the function name in ``_call``'s error), at
the smallest shapes.  Every wrapper's values are pinned elsewhere; here results are compared bit for bit with the
same wrapper's plain call."""
import pytest
import torch

from detect_ref import random_detector
from fixtures import build_module, golden_inputs
from hardnetnas_amd import _native as N

pytestmark = pytest.mark.gpu

H, W = 1, 2  # the smallest image the detector accepts (test_gpu_det_train.SHAPES)


@pytest.mark.parametrize("b", [1, 3])
def test_forward_replaces_a_short_workspace(b, cuda_device):
    """Replace: a workspace one byte short is left alone and a fresh one used; the result is the plain call's."""
    m, fx, _ = build_module("hardnet")
    nm = N.NativeModel.from_module(m, cuda_device)
    x = torch.from_numpy(golden_inputs(fx)[:b]).to(cuda_device)
    short = torch.full((nm.workspace_bytes(b) - 1,), 0xA5, dtype=torch.uint8, device=cuda_device)
    got = nm.forward(x, workspace=short)
    want = nm.forward(x)
    torch.cuda.synchronize(cuda_device)
    assert got.shape == (b, 128) and torch.equal(got, want)
    assert bool((short == 0xA5).all())


def test_det_train_forward_raises_on_a_short_scratch(cuda_device):
    """Raise: a scratch one byte short is a ValueError naming the byte count, before anything is launched -- the
    outputs and the running statistics keep what they held."""
    dev = cuda_device
    det = random_detector(7).train().to(dev)
    tensors = [t.detach() for t in N.det_train_tensors(det)]
    before = [t.clone() for t in tensors]
    images = torch.rand(1, 1, H, W, device=dev)
    n_sv, n_sc = N.det_train_workspace_bytes(1, H, W)
    score, ori = torch.full((1, H, W), 7.0, device=dev), torch.full((1, H, W, 2), 7.0, device=dev)
    saved = torch.zeros(n_sv, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=f"scratch must be .* at least {n_sc} bytes"):
        N.det_train_forward(images, tensors, 1e-5, 1e-5, 0.1, score, ori, saved,
                            torch.empty(n_sc - 1, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize(dev)
    assert bool((score == 7.0).all()) and bool((ori == 7.0).all()) and not bool(saved.any())
    assert all(torch.equal(a, b) for a, b in zip(tensors, before))
    # the exact size passes
    N.det_train_forward(images, tensors, 1e-5, 1e-5, 0.1, score, ori, saved,
                        torch.empty(n_sc, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize(dev)
    assert not bool((score == 7.0).all())


def test_detector_forward_passes_a_short_workspace_to_the_c_abi(cuda_device):
    """Pass-through: Python does not size-check a supplied detector workspace; the C ABI's HN_ERR_WORKSPACE, an
    argument error returned before any launch, arrives as a RuntimeError with hn_last_error's message."""
    dev = cuda_device
    nd = N.NativeDetector(N.state_dict_blob(random_detector(7).state_dict()), dev)
    images = torch.rand(1, 1, H, W, device=dev)
    need = nd.workspace_bytes(1, H, W)
    with pytest.raises(RuntimeError, match=r"^hn_det_forward failed \(status 4\): .*workspace"):
        nd.forward(images, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    score, ori = nd.forward(images, workspace=torch.empty(need, dtype=torch.uint8, device=dev))
    want_s, want_o = nd.forward(images)
    assert torch.equal(score, want_s) and torch.equal(ori, want_o)


def test_match_nn2_copies_a_misaligned_query(cuda_device):
    dev = cuda_device
    g = torch.Generator().manual_seed(11)
    base = torch.nn.functional.normalize(torch.randn(3 * 128 + 1, generator=g).to(dev), dim=0)
    query = base[1:].view(3, 128)  # contiguous, one float past the allocation's start
    assert query.is_contiguous() and query.data_ptr() % 16 == 4
    db = torch.nn.functional.normalize(torch.randn(5, 128, generator=g), dim=1).to(dev)
    dist, idx = N.match_nn2(query, db)
    want_d, want_i = N.match_nn2(query.clone(), db)
    assert torch.equal(dist, want_d) and torch.equal(idx, want_i)
    assert idx.shape == (3, 2) and bool((idx[:, 0] != idx[:, 1]).all())


def test_error_message_names_the_function(cuda_device):
    """An input Python accepts and the C ABI rejects (an even nms_ksize): the message starts with the name of the
    function that failed, not with that of the size query before it."""
    score = torch.rand(1, 16, 16, device=cuda_device)
    with pytest.raises(RuntimeError, match=r"^hn_select_keypoints failed \(status 1\): "):
        N.select_keypoints(score, border=0, nms_thresh=0.0, nms_ksize=2, topk=4, gauss_ksize=1, gauss_sigma=0.0)
