"""The batch scratch is laid out in one place (carve, hkv_batch.hip): its size and every array's offset, for
cap in {1, 250, 2048, 2^20} and entry sizes 64 and 320, equal what the two hand-kept listings gave."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_size_and_offsets_unchanged(tmp_path):
    exe = str(tmp_path / "scratch_layout_check")
    lib = os.path.join(ROOT, "hermes_amd")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-I", os.path.join(lib, "csrc"),
                    os.path.join(ROOT, "tools", "scratch_layout_check.cpp"), "-L", lib, "-lhermeskv",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "scratch layout: OK" in r.stdout, r.stdout + r.stderr
