"""The clip_patch backward's per-sample arithmetic on the host, before any GPU sees the kernel that uses it:
hn_clip.h's sample_grad / accumulate_grad / keypoint_grad (the kernel's own text) over the adversarial keypoints of
the forward's sweep and a grid of ordinary ones (hardnetnas_amd/csrc/hn_clip_grad_host_check.cpp)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hardnetnas_amd", "csrc")


def test_host_sweep_of_the_gradient_function_is_clean():
    """Built with -fsanitize=address,undefined,float-cast-overflow: exit 0, every index inside the exactly sized
    images whatever the keypoint data (NaN / +-Inf / 1e30 scales, orientations and ratios, coordinates and batch
    indices far outside), every ordinary keypoint's (a, b) equal to the closed form in double at the same cells,
    no sanitizer report."""
    r = subprocess.run(["make", "-C", CSRC, "clip_grad_check"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "clip_grad_check:" in out and "every index in bounds" in out and "equal the closed form" in out
    assert "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
