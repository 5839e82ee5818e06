#!/usr/bin/env python3
"""Golden digests for tests/test_dev_sort_cpu.py: the reference's own radix sort (ksort.h, KRADIX_SORT_INIT as the fork
instantiates it for mm128_t) compiled from its header where it lies (tests/csrc/sort_ref.c) and run on the test's seeded cases.
Authoring container only (needs /root/reference); what is committed is data: per case, n, the SHA-256 of the input keys and
the SHA-256 of the sorted (key, original index) pairs, both as little-endian uint64.

    python tests/golden/make_ksort_digests.py
"""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dev_sort_cpu import KSORT_GOLDEN, _cases, _pairs, _sha  # noqa: E402


def main():
    hdr = glob.glob("/root/reference/**/minimap2-master_remapping/ksort.h", recursive=True)
    so = os.path.join(tempfile.mkdtemp(prefix="al_ksort_"), "libsort_ref.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", '-DREF_KSORT_H="%s"' % hdr[0], os.path.join(ROOT, "tests", "csrc", "sort_ref.c"), "-o", so])
    R = C.CDLL(so); R.ref_sort128.argtypes = [C.c_void_p, C.c_int]
    lines = ["# case\tn\tsha256(keys)\tsha256(sorted pairs): the reference's radix_sort on tests/test_dev_sort_cpu.py::_cases (make_ksort_digests.py)"]
    for i, x in enumerate(_cases()):
        b = _pairs(x)
        R.ref_sort128(b.ctypes.data, len(x))
        lines.append("%d\t%d\t%s\t%s" % (i, len(x), _sha(x), _sha(b)))
    with open(KSORT_GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
