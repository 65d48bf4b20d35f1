"""The plan of the BGZF text (rpvg_amd/csrc/text_deflate_plan.hpp) checked without a GPU: tests/cpp/text_deflate_plan_check.cpp holds
the chunk ranges at their edges, CRC-32 and the operators that join slices to zlib's, every length and distance code to RFC 1951's
tables, code lengths under the 15- and 7-bit limits to the Kraft sum and to within one percent of the unlimited Huffman cost, the
canonical codes to the RFC's example, and whole members — the host's framing and the model of the device's member, over texts from
one byte to three chunks — to zlib's inflate.  Built against the plan header alone, with the address and undefined-behaviour
sanitizers, as a program of its own."""
import os
import subprocess


def _text_deflate_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "text_deflate_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "text_deflate_plan_check.cpp"),
                           "-o", binary, "-lz"])
    return binary


def test_codes_lengths_crc_and_members_hold_to_zlib_and_the_rfc():
    done = subprocess.run([_text_deflate_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", (done.stdout + done.stderr)[-2000:]
