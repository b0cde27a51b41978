"""The dynamic tile-claiming protocol on the host, before any GPU sees a kernel that uses it: both wave roles of
every workgroup walk hn_tiles.h's functions (the kernels' own text) against a mocked counter pair in seeded
interleavings (hardnetnas_amd/csrc/hn_tiles_host_check.cpp)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hardnetnas_amd", "csrc")


def test_host_model_of_the_claim_protocol_is_clean():
    """Built with -fsanitize=address,undefined: exit 0, every invariant held, no sanitizer report.  The invariants:
    both roles of a workgroup see one tile sequence and stop behind the same barrier, what is staged for a stage
    is what is computed at it, every tile runs exactly once, the counters end at zero."""
    r = subprocess.run(["make", "-C", CSRC, "tiles_check"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "all invariants held" in out
    assert "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
