"""The homography ground-truth stage's conversions and address computations on the host, before any GPU sees a kernel
that uses them: hn_homo.h's functions (the kernels' own text) swept over adversarial homographies, keypoints, maps and
masks (hardnetnas_amd/csrc/hn_homo_host_check.cpp)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hardnetnas_amd", "csrc")


def test_host_sweep_of_the_address_computations_is_clean():
    """Built with -fsanitize=address,undefined,float-cast-overflow: exit 0, every index inside its array, no sanitizer
    report.  The sweep: horizon lines through the image (w ~ 0), NaN / +-Inf / 1e38 entries, singular and all-zero
    matrices, keypoints and batch indices far outside, masks with 0 and with H W set pixels."""
    r = subprocess.run(["make", "-C", CSRC, "homo_check"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "every index in bounds" in out
    assert "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
