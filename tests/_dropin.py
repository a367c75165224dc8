"""Helpers for the drop-in tests: build one tests/cpp program against the mirror headers and libearhip.so, and run it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, program, wextra=True, libs=()):
    """tests/cpp/<program>.cpp -> an executable under tmp_path, as C++14 with -Wall [-Wextra] -Werror"""
    from libear_amd import build as build_lib
    build_lib()
    exe = str(tmp_path / program)
    libdir = os.path.join(ROOT, "libear_amd", "lib")
    cmd = ["g++", "-std=c++14", "-Wall"] + (["-Wextra"] if wextra else []) + ["-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "libear_amd", "host"), os.path.join(ROOT, "tests", "cpp", program + ".cpp"),
           "-L" + libdir, "-learhip"] + ["-l" + lib for lib in libs] + ["-Wl,-rpath," + libdir, "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


def run(exe, *args, timeout=None):
    """the completed process, its stderr folded into stdout"""
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
