"""csrc/xp_launch.hpp without a GPU: tests/launch_check.hip (a program of its own, host code only) holds the dispatchers
to "one call, with the value asked for, and the last choice for any other value" and the launch geometry to its block counts."""
import os
import subprocess

from xarray_parcel_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


def test_dispatchers_and_geometry_of_the_launch_header(tmp_path):
    exe = str(tmp_path / 'launch_check')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    build = subprocess.run([hipcc, '-O1', '-std=c++17', '--offload-arch=gfx950', '--cuda-host-only', '-Wall', '-Werror', '-I', _lib.SRC_DIR,
                            os.path.join(HERE, 'launch_check.hip'), '-o', exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and 'all checks passed' in run.stdout, run.stdout[-3000:] + run.stderr[-1000:]
