"""The in-process GPU steps of tests/test_gpu_merge.py, in a process of its own so that the test can run them under a time limit: the taps of `merge`
(al_dbg_merge against al_dbg_merge_host against the rules of tests/merge_cases.py) with one round and with the round loop, the refusals through the taps, and
the C ABI (al_merge_bams without its host flag).

usage: merge_child.py taps|loop|refusals|abi WORKDIR
An assertion that fails ends the process with its traceback; otherwise the last line printed is "ok <what ran>"."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lift_cases as lc  # noqa: E402
import lift_sort_cases as ls  # noqa: E402
import merge_cases as mc  # noqa: E402
from merge_tap import tap  # noqa: E402
from select_cases import bgzf  # noqa: E402
from airlift_amd import capi  # noqa: E402


def taps(L, T, d):
    """one round with every input at eof: device tags, keys and packed bytes equal the host tap's and Python's on every set of tiles, ties and refs"""
    all_ = mc.self_check(T); n = 0
    for lname in ("tiles", "ties", "refs"):
        for name, inputs in sorted(all_[lname].items()):
            host, dev = tap(L, inputs, 0), tap(L, inputs, 0, dev=0)
            assert dev == host, (lname, name)
            e = mc.expected(inputs)
            assert host["rounds"] == 1 and host["tags"] == [i << 28 | x for i, x, _ in e] and host["keys"] == [mc.key(o) for _, _, o in e], (lname, name)
            assert host["packed"] == b"".join(lc.rec_bytes(o) for _, _, o in e), (lname, name)
            n += 1
    return "%d sets" % n


def loop(L, T, d):
    """the round loop over the windows sets at pieces of 1000 and 4096 bytes: device equals host equals Python, for K = 2, 3 and 8"""
    all_ = mc.self_check(T); n = 0; ks = set()
    for p in mc.PIECES:
        for name, inputs in sorted(all_["windows%d" % p].items()):
            host, dev = tap(L, inputs, p), tap(L, inputs, p, dev=0)
            assert dev == host, (p, name)
            e = mc.expected(inputs)
            assert host["rounds"] > 1 and [t >> 28 for t in host["tags"]] == [i for i, _, _ in e] and host["keys"] == [mc.key(o) for _, _, o in e], (p, name)
            assert host["packed"] == b"".join(lc.rec_bytes(o) for _, _, o in e), (p, name)
            n += 1; ks.add(len(inputs))
    assert {2, 3, 8} <= ks
    return "%d sets" % n


def refusals(L, T, d):
    """unsorted and malformed streams and a refID beyond the list through the device tap: refused as by the twin, and the process goes on"""
    n = 0
    for p in mc.PIECES:
        for name, (inputs, idx) in sorted(mc.unsorted(mc.ENDS["tap", p]).items()):
            for q in (0, p):
                tap(L, inputs, q, expect=-2); tap(L, inputs, q, dev=0, expect=-2); n += 1
    for name, (first, blob, say) in sorted(mc.malformed().items()):
        for q in (0, 1000):
            tap(L, [first, blob], q, expect=-2); tap(L, [first, blob], q, dev=0, expect=-2); n += 1
    for name in ("refid_beyond", "next_refid_beyond"):
        inputs = mc.refs_refusals()[name][0]
        tap(L, inputs, 0, expect=-2); tap(L, inputs, 0, dev=0, expect=-2); n += 1
    good = mc.ties(T)["equal_diff_len"]
    assert tap(L, good, 0, dev=0) == tap(L, good, 0)                       # the device is as it was
    return "%d refusals" % n


def abi(L, T, d):
    """al_merge_bams on the device, alone and with the device compressor: the records of the host call, no device memory held"""
    inputs = mc.self_check(T)["windows1000"]["k3"]
    bams = []
    for i, x in enumerate(inputs):
        bams.append(os.path.join(d, "abi%d.bam" % i)); open(bams[-1], "wb").write(bgzf(mc.stream(x), 700))
    out = os.path.join(d, "abi_out.bam")
    for flags in (0, capi.MERGE_GPU_DEFLATE, capi.MERGE_HOST):
        st = capi.merge_bams(bams, out, flags=flags, piece_bytes=1000)
        assert st.held == 0 and st.on_device == (0 if flags & capi.MERGE_HOST else 1) and st.rounds > 3 and list(st.records_in[:3]) == [len(i[2]) for i in inputs]
        assert ls.inflate(out) == mc.expected_stream(inputs)
    return "3 forms"


def main():
    what, d = sys.argv[1], sys.argv[2]
    L = capi.load()
    print("ok", what, {"taps": taps, "loop": loop, "refusals": refusals, "abi": abi}[what](L, L.al_dbg_merge_tile(), d))


if __name__ == "__main__":
    main()
