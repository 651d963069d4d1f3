"""Builds the host programs of tests/lockstep (xm_kernels.hip compiled as plain C++ through the shim, under ASan + UBSan), once per
pytest session and program: tests/test_lockstep_place_cpu.py and tests/test_lockstep_kernels_cpu.py share this."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H

# what every run of such a program gets: a sanitizer report ends it, and leaks count
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
_BUILT = {}


def host_clangxx():
    """ROCm's host clang++ (g++ has no ext_vector_type), found from hipcc as xenomapper_amd/build.py finds that."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))] if os.path.exists(hipcc) else []
    roots += [os.environ.get("ROCM_PATH", ""), "/opt/rocm"]
    for root in roots:
        for rel in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
            exe = os.path.join(root, rel)
            if root and os.path.exists(exe):
                return exe
    return None


def host_program(tmp_path_factory, name):
    """The path of tests/<name>.cpp built as a stand-alone program; skips when ROCm's host clang++ is not there."""
    if name in _BUILT:
        return _BUILT[name]
    cxx = host_clangxx()
    if cxx is None:
        pytest.skip("ROCm's host clang++ not found: the lockstep build of xm_kernels.hip needs it")
    path = str(tmp_path_factory.mktemp("lockstep") / name)
    # use-after-return detection off: it gives every lane context a fake stack of its own, mapped and unmapped per workgroup
    subprocess.check_call([cxx, "-x", "c++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fsanitize-address-use-after-return=never", "-Wall", "-Wextra", "-Wno-pass-failed",
                           "-I", os.path.join(H.REPO, "tests", "lockstep"),
                           os.path.join(H.REPO, "tests", name + ".cpp"), "-o", path, "-lpthread"])
    _BUILT[name] = path
    return path
