#!/usr/bin/env python
"""Generates tests/golden/ref_calls.npz: every call tests/test_oracle_pinned.py makes into the compiled reference (oracle/_ref)
with what it returned, so that those tests run the same comparisons where oracle/_ref is not built (tests/ref_replay.py).
Needs oracle/_ref (built by __graft_entry__.build() where the reference tree is present):
    python tests/golden/make_ref_calls.py"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "ref_calls.npz")

if __name__ == "__main__":
    env = dict(os.environ, XIVO_REF_RECORD=OUT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_oracle_pinned.py")], cwd=ROOT, env=env)
    sys.exit(r.returncode)
