"""The plain parts of the mirror's shared header (libear_amd/host/ear/hip_batch.hpp) on the host, under ASan and UBSan
(tests/cpp/test_mirror_batch.cpp): the carver of the device batches over malloc'ed memory with the array lists of the five batch
sites at n = 1, 3 and 67 (alignment, order, no overlap, the size computed from the same list and not above what the site asked
for before), a mis-ordered list refused, the layout binding's scatter and the zone conversion.  The program links no library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carver_scatter_and_zone_conversion_on_the_host_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "test_mirror_batch")
    res = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-static-libasan", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "libear_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_mirror_batch.cpp"),
                          "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    m = re.search(r"^(\d+) passed, 0 failed$", res.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 328, res.stdout
