"""CPU-side (-m "not gpu"): the C ABI spans several translation units (csrc/ss_api.hip and csrc/api_*.hip); an entry point left
static, dropped or pulled into a namespace there still compiles and links.  The library's dynamic symbol table is compared with
include/seekstorm_hip.h, by name only: every prototyped ss_* function is exported once and unmangled, nothing unmangled named ss_* is
exported beside them, and no ssi_* function that one file expects of another is left undefined."""
import collections
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nm(lib, which):
    out = subprocess.run(["nm", "-D", which, lib], check=True, capture_output=True, text=True).stdout
    return [ln.split() for ln in out.splitlines() if ln.strip()]


def test_exports_are_the_header_prototypes():
    from seekstorm_amd.build import build
    lib = build()  # (incremental: nothing to do on a built tree)
    hdr = open(os.path.join(ROOT, "include", "seekstorm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 100
    defined = _nm(lib, "--defined-only")  # [address, type, name]
    exported = collections.Counter(f[-1] for f in defined if f[-2] in "TW" and re.fullmatch(r"ss_[a-z0-9_]+", f[-1]))
    assert sorted(declared - set(exported)) == [], "prototyped in seekstorm_hip.h, not exported unmangled"
    assert sorted(set(exported) - declared) == [], "exported as ss_*, not prototyped in seekstorm_hip.h"
    assert [n for n, c in exported.items() if c != 1] == []
    undefined = [f[-1] for f in _nm(lib, "--undefined-only") if "ssi_" in f[-1]]
    assert undefined == [], "declared in a header of csrc/, defined nowhere"
