"""The bucket rule of the pruned strategy's score histogram (seekstorm_amd/csrc/bm25_hist.h: bucket of a score, edge of a bucket, both on
float BIT patterns) on the CPU: a stand-alone program (tests/hist_threshold_check.cpp, its own main) is compiled with g++ under
AddressSanitizer and UBSan and checks, for a range of (lo, hi) pairs -- lo = hi, lo one ulp below hi, ranges that need shift 0 and 1, a
seedless range (lo = the fixed share of hi), hi in the next binade, ten binades, the whole range of normal floats, random pairs --:

  * `shift` is the smallest with (bits(hi) - bits(lo)) >> shift < B;
  * bucket() is monotone in the score;
  * edge(bucket(s)) <= s -- as bit patterns and as floats -- for s at every bucket edge +- 1 ulp and at a few thousand random scores
    (this is what makes a published edge a valid lower bound of the k-th best score);
  * scores >= hi land in no bucket below hi's own and in bucket B - 1 once the clamp is reached (the last edge, FLT_MAX);
  * scores < lo are not counted."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_and_edge_on_bit_patterns(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "hist_threshold_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "hist_threshold_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hist_threshold ok:" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
