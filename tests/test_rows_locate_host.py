"""k_unique_rows' batch search (kary_last_le and rows_window_batch, hkv_batch_dev.h) on the host: a stand-alone
program (tools/rows_locate_check.cpp) compiled for the host alone under AddressSanitizer and
UndefinedBehaviorSanitizer checks it against batch_of's binary search -- all batches empty but one, runs of more
than a window of empty batches, first and last batch empty, one batch, offsets equal to i and to i +- 1, batch
counts that are no power of two up to 2^18 (and 2^20, where the narrowing takes a third step). It runs as a child
process with nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_locate_matches_binary_search(tmp_path):
    exe = str(tmp_path / "rows_locate_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-g", "--cuda-host-only",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "hermes_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-x", "hip", os.path.join(ROOT, "tools", "rows_locate_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rows locate: OK" in r.stdout, r.stdout + r.stderr
