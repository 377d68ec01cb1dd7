"""corsair_amd/csrc/exact_div.h (the division-free centroid of k_ransac_hyp) against the IEEE division on the CPU: builds
tools/div_sweep.cpp with the host compiler and runs a reduced sweep -- every adversarial operand (significands of all ones,
powers of two, quotients next to rounding midpoints, zeros, subnormals, non-finite values; n = 3 .. 64) and 2e7 random ones.
The full run (1.2e9 operands, the default of the program) and the -fsanitize=address,undefined build are run by hand:
profiles/front_div_sweep.txt holds the output of both."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_div_equals_ieee_division(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler on PATH (the project cannot be built without one)"
    exe = str(tmp_path / "div_sweep")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "corsair_amd", "csrc"),
                           os.path.join(ROOT, "tools", "div_sweep.cpp"), "-o", exe])
    out = subprocess.run([exe, "20000000", "4"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
    assert int(out.stdout.split()[1]) > 9e7
