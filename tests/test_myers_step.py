"""The shared Myers column step (floxer_amd/csrc/flx_myers.hpp) on the host: no GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_column_step_truth_tables_and_symbol_patch(tmp_path):
    """the header's step, written on 32-bit halves with three-input operations, against the plain u64 formula: every carry-in pair on
    structured words (single bits at 0 / 31 / 32 / 63, runs that end at bit 31 and bit 63), a million random triples and 250 000
    chained columns; each truth-table constant against its expression on all eight input combinations; the symbol patch for every
    count of in-window columns; tests/myers_step_check.cpp"""
    exe = str(tmp_path / "myers_step_check")
    src = os.path.join(ROOT, "tests", "myers_step_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
