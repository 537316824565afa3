"""Index arithmetic of the Winograd path (csrc/winograd_index.hpp) on the host: tools/winograd_index_check.cpp, a stand-alone program,
walks every offset the input and output transforms form for the GPU test shapes and for 8 x 512 x 97 x 97 at dilation 4, touching
real arrays of the tensors' exact sizes for the small ones.  Built with AddressSanitizer and UBSan (host code only, its own
`main`; no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and (shutil.which(c) or os.path.isfile(c)):
            return c
    return None


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")
def test_every_offset_of_the_winograd_transforms_lies_inside_its_tensor(tmp_path):
    exe = tmp_path / "winograd_index_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "da-sac_amd", "csrc"), os.path.join(ROOT, "tools", "winograd_index_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    assert "winograd index check: 0 bad" in out.stdout
    assert "8 C=512 M=512 97x97 d=4: 49 x 49 tiles per image, T=19208" in out.stdout
