"""The weight packers of hn_create on the host (hardnetnas_amd/csrc/hn_pack.h): every packer at every shape the
model builders pass it, under the sanitizers, against digests recorded before the packers left hn_api.hip
(hardnetnas_amd/csrc/hn_pack_host_check.cpp, tests/golden/pack_digests.txt)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hardnetnas_amd", "csrc")


def test_packers_write_inside_their_outputs_and_keep_their_layouts():
    """Built with -fsanitize=address,undefined,float-cast-overflow: exit 0, no sanitizer report, every output has
    the size its layout states with the write cursor at its end, and every digest equals the recorded one."""
    r = subprocess.run(["make", "-C", CSRC, "pack_check"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sizes and digests match" in out
    assert "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
