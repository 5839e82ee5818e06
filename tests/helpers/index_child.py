"""The in-process GPU steps of tests/test_gpu_index.py, in a process of its own so that the test can run them under a time limit: the taps of `bam-index`
(al_dbg_bai against al_dbg_bai_host against the rules of tests/index_cases.py) over the case lists and the piece sizes, the refusals through the taps, and the C
ABI (al_index_bam without its host flag).

usage: index_child.py taps|refusals|abi WORKDIR
An assertion that fails ends the process with its traceback; otherwise the last line printed is "ok <what ran>"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import index_cases as ic  # noqa: E402
import merge_cases as mc  # noqa: E402
from select_cases import bgzf  # noqa: E402
from airlift_amd import capi  # noqa: E402

TAP_PIECES = (0, 1000, 4096, 97)


def taps(L, d):
    """every case at every piece size: the device tap equals the host tap and Python"""
    n = 0
    for name, (recs, layout) in sorted(ic.self_check().items()):
        blob = ic.stream(recs); data = ic.compress(blob, layout); mem = ic.members(data)
        want = ic.expected_bai(ic.REFS, recs, mem)
        for piece in TAP_PIECES:
            host, dev = ic.tap(L, blob, mem, len(data), piece), ic.tap(L, blob, mem, len(data), piece, dev=0)
            assert host == want, (name, piece)
            assert dev == host, (name, piece)
            n += 1
    return "%d runs" % n


def refusals(L, d):
    """what the twin refuses through the device tap: refused alike, and the process goes on"""
    n = 0
    for name, (recs, say) in sorted(ic.refusals().items()):
        blob = ic.stream(recs); data = bgzf(blob, 700); mem = ic.members(data)
        for q in (0, 1000, 97):
            ic.tap(L, blob, mem, len(data), q, expect=-2); ic.tap(L, blob, mem, len(data), q, dev=0, expect=-2); n += 1
    for p in ic.PIECES:
        recs, off = ic.boundary_descent(ic.H0 + p)
        blob = ic.stream(recs); data = bgzf(blob, 700); mem = ic.members(data)
        ic.tap(L, blob, mem, len(data), p, expect=-2); ic.tap(L, blob, mem, len(data), p, dev=0, expect=-2); n += 1
    for name, (first, blob, say) in sorted(mc.malformed().items()):
        data = bgzf(blob, 700); mem = ic.members(data)
        for q in (0, 1000):
            ic.tap(L, blob, mem, len(data), q, expect=-2); ic.tap(L, blob, mem, len(data), q, dev=0, expect=-2); n += 1
    recs, layout = ic.all_cases()["basics@700"]
    blob = ic.stream(recs); data = ic.compress(blob, layout); mem = ic.members(data)
    assert ic.tap(L, blob, mem, len(data), 1000, dev=0) == ic.expected_bai(ic.REFS, recs, mem)          # the device is as it was
    return "%d refusals" % n


def abi(L, d):
    """al_index_bam on the device and with its host flag: the same file, no device memory held"""
    recs, layout = ic.all_cases()["basics@700"]
    bam = os.path.join(d, "abi.bam"); data = ic.compress(ic.stream(recs), layout); open(bam, "wb").write(data)
    want = ic.expected_bai(ic.REFS, recs, ic.members(data))
    for flags in (0, capi.BAI_HOST):
        if os.path.exists(bam + ".bai"):
            os.unlink(bam + ".bai")
        st = capi.index_bam(bam, flags=flags, piece_bytes=200)
        assert st.held == 0 and st.on_device == (0 if flags else 1) and st.records == len(recs) and st.unplaced == 3 and st.pieces > 1 and st.bai_bytes == len(want)
        assert open(bam + ".bai", "rb").read() == want
    return "2 forms"


def main():
    what, d = sys.argv[1], sys.argv[2]
    L = capi.load()
    print("ok", what, {"taps": taps, "refusals": refusals, "abi": abi}[what](L, d))


if __name__ == "__main__":
    main()
