"""The plan of a batch upload (rpvg_amd/csrc/batch_forms.hpp: the forms a host batch arrives in, decided once) under the
sanitizers.  No GPU; what the device makes of every form is tests/test_hip_kernels.py's."""
import os
import subprocess


def test_batch_forms_under_the_sanitizers():
    """tests/cpp/batch_forms_check.cpp: every form, the argument errors as worded, the copied bytes against the upload's former
    formula and the reads of unvalidated offsets, as a program of its own built against the header alone with AddressSanitizer and
    UBSan; every array in a heap block of exactly its length."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "batch_forms_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: no order of libraries to keep
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "batch_forms_check.cpp"), "-o", binary])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"
