"""The handle of a device buffer (ansel_amd/csrc/dev_buf.h) on the host: tests/native/dev_buf_host.cpp, a program of its own
with counting stubs for the runtime's allocator, compiled with the host compiler and run as a child process.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_buf_releases_every_owned_block_exactly_once(tmp_path):
    exe = str(tmp_path / "dev_buf_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ansel_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "dev_buf_host.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "dev_buf_host ok" in r.stdout
