"""examples/c_consumer.c: the C-ABI from plain C99 (what a GDExtension / P/Invoke shim does).  CPU: it builds with
-pedantic -Werror against include/ocean_waves.h and fails loudly without a device.  GPU: its output equals the Python
mirror driving the same schedule (update + one cascade per frame + asynchronous hand-off + surface sampling)."""
import subprocess

import pytest
from checks import check_against_mirror
from cpu_builds import build_example


def test_builds_as_pedantic_c99_and_fails_loudly_without_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by the gpu test")
    r = subprocess.run([build_example(tmp_path, "c_consumer")], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stderr and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_c_program_and_python_mirror_agree(tmp_path):
    n, frames = 256, 12
    r = subprocess.run([build_example(tmp_path, "c_consumer"), str(n), str(frames)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    check_against_mirror(r.stdout, n, frames)
    assert "spectra_generated=3" in r.stdout
