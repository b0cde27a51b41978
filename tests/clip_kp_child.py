"""Child process of tests/test_gpu_clip.py::test_forward_keypoints_across_chunks (not a test module).

Started with HN_CHUNK / HN_SUBCHUNK in its environment (hn_create reads them), so that the keypoints of one call
span two chunks of the forward: runs NativeModel.forward_keypoints of the models named on the command line on
the parent's seeded inputs, checks it against forward(clip_patch(...)) under the same knobs, and saves the
descriptors for the parent to compare with its own, made at the default chunk size.
usage: clip_kp_child.py OUT.pt N MODEL [MODEL ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kp_inputs(n, dev):
    """The keypoint inputs of the forward_keypoints tests on the golden fixture's images, on ``dev``."""
    import torch
    from clip_ref import random_case
    from fixtures import load
    images = torch.from_numpy(load("clip_patch")["images"])
    B, _, H, W = images.shape
    kpts, scale, ori, ratio, images = random_case(n, B, H, W, seed=100 + n, images=images)
    return tuple(t.to(dev) for t in (images, kpts, scale, ori, ratio))


def main() -> int:
    import torch
    from fixtures import build_module
    from hardnetnas_amd import _native
    out_path, n, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    args = kp_inputs(n, dev)
    res = {}
    for name in names:
        m, _, _ = build_module(name)
        nm = _native.NativeModel.from_module(m, dev)
        y = nm.forward_keypoints(*args)
        torch.cuda.synchronize()
        assert torch.equal(y, nm.forward(_native.clip_patch(*args))), name
        res[name] = y.cpu()
    torch.save(res, out_path)
    print(f"CLIP_KP_OK chunk={os.environ.get('HN_CHUNK')} n={n} models={','.join(names)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
