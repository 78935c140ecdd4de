"""csrc/hrx_host_split.hpp: how an AUTO hrx_witness_batch_host call divides a batch between the device and the host cores.  Built with the host
compiler and run here; the GPU side is tests/test_host_routes_gpu.py::test_auto_route_small_batches_of_long_strings."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_parts_cover_the_batch_and_small_batches_are_not_split(tmp_path):
    """B in {1, 2, 32, 63, 64, 65, 127, 128, 129, ..., 16384, 2^32} x device shares at and past both clamps (0, 1/16, 15/16, 1, NaN): the device part is at most
    B, the host part is B minus it, both are at least 64 strings; batches under 128 strings are not split (B = 32 once made the host part wrap around)."""
    exe = str(tmp_path / "hrx_test_host_split")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host_cpp", "test_host_split.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "host split: ok" in out.stdout, out.stdout + out.stderr
