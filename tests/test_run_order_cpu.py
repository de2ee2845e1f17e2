"""The run flow's ordering pieces (csrc/run_order.hpp: the POS chain, the in-order sequencer, the
whole-region split) as a stand-alone host program under the thread sanitizer: tests/native/
run_order_main.cpp includes the header alone, is built with the ROCm clang++ and run as a child."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rocm_clang():
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    for r in roots:
        if r and os.path.exists(os.path.join(r, "lib", "llvm", "bin", "clang++")):
            return os.path.join(r, "lib", "llvm", "bin", "clang++")
    hipcc = shutil.which("hipcc")
    if hipcc:
        c = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
        if os.path.exists(c):
            return c
    return None


def test_ordering_pieces_under_the_thread_sanitizer(tmp_path):
    cxx = rocm_clang()
    assert cxx is not None, "the ROCm clang++ was not found"
    exe = str(tmp_path / "run_order_main")
    src = os.path.join(ROOT, "tests", "native", "run_order_main.cpp")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", src, "-o", exe, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stdout + r.stderr
    assert "run_order: ok" in r.stdout
