"""The in-process GPU steps of tests/test_gpu_lift.py, in a process of its own so that the test can run them under a time limit: the taps of lift
(al_dbg_lift against al_dbg_lift_host against the rules of tests/lift_cases.py) and the C ABI (al_lift_bam).

usage: lift_child.py kernels|ends|malformed|abi WORKDIR
An assertion that fails ends the process with its traceback; otherwise the last line printed is "ok <what ran>"."""
import ctypes as C
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lift_cases as lc  # noqa: E402
from select_cases import bgzf  # noqa: E402
from airlift_amd import capi  # noqa: E402


def tap(L, fn, blob, chain, *dev):
    n_cap = len(blob) // 36 + 2; cap = len(blob) + 8 * n_cap + 64
    rec_off = (C.c_uint32 * n_cap)(); verdict = (C.c_uint32 * n_cap)(); out4 = (C.c_uint64 * 4)()
    packed = C.create_string_buffer(cap); arena = C.create_string_buffer(cap); packed_n, arena_n, held = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = fn(*dev, blob, len(blob), chain.encode(), rec_off, verdict, n_cap, out4, packed, cap, C.byref(packed_n), arena, cap, C.byref(arena_n), *([C.byref(held)] if dev else []))
    assert rc == 0, rc
    assert held.value == 0
    n = out4[0]
    return dict(rec_off=list(rec_off[:n]), verdict=list(verdict[:n]), consumed=out4[1], first_bad=out4[2], code=out4[3], packed=packed.raw[:packed_n.value], arena=arena.raw[:arena_n.value])


def both(L, blob, chain):
    return tap(L, L.al_dbg_lift_host, blob, chain), tap(L, L.al_dbg_lift, blob, chain, 0)


def rows_of_arena(arena, refs):
    out, p = [], 0
    while p < len(arena):
        name_len, n_cig, mf, ref, s, _, e = struct.unpack_from("<IIIiiiq", arena, p)
        name = arena[p + 32:p + 32 + name_len].decode(); cg = struct.unpack_from("<%dI" % n_cig, arena, p + 32 + name_len)
        flag = mf >> 8
        out.append("%s\t%d\t%d\t%s\t%d\t%s" % (refs[ref][0], s, e, name + (".1" if flag & 64 else ".2" if flag & 128 else ""), mf & 255, "".join("%d%s" % (c >> 4, lc.CIG[c & 15]) for c in cg) or "*"))
        p += 32 + ((name_len + 4 * n_cig + 7) & ~7)
    return out


def offsets(recs):
    offs, o = [], len(lc.header_bytes(lc.HEADER, lc.REFS))
    for r in recs:
        offs.append(o); o += len(lc.rec_bytes(r))
    return offs


def kernels(L, chain, W, d):
    """al_dbg_lift equals al_dbg_lift_host equals the Python rules on every directed set and window shape: rec_off, verdicts, packed bytes, arena"""
    assert W >= 1024 and W & (W - 1) == 0
    sets = [("d%d" % n, lc.directed(n)) for n in lc.SIZES] + sorted(lc.walk_sets(W).items())
    for name, recs in sets:
        blob = lc.bam_bytes(lc.HEADER, lc.REFS, recs)
        host, dev = both(L, blob, chain)
        assert dev == host, name
        offs = offsets(recs)
        v, kept, rows = lc.lift_all(lc.CHAIN, lc.REFS, recs)
        assert host["rec_off"] == offs and host["consumed"] == len(blob) and host["first_bad"] == 2 ** 64 - 1 and host["verdict"] == v, name
        assert host["packed"] == b"".join(lc.rec_bytes(k) for k in kept) and rows_of_arena(host["arena"], lc.REFS) == rows, name
        if name.startswith("cut"):
            c = int(name[3:]); k = offs.index(2 * W - c)                  # the record whose block_size field the window's edge cuts after c bytes
            assert 0 < k < len(offs) - 1 and offs[k] - offs[k - 1] > W
        if name == "long":
            assert max(b - a for a, b in zip(offs, offs[1:])) > 5 * W
    return "%d sets" % len(sets)


def ends(L, chain, W, d):
    """the end of a piece: inside a block_size field after 1, 2 and 3 bytes, inside a record, and a text with no complete record"""
    recs = lc.walk_sets(W)["cut2"]; blob = lc.bam_bytes(lc.HEADER, lc.REFS, recs)
    offs = offsets(recs); h = offs[0]
    cuts = [(offs[k] + c, k) for k in (1, 20, 21, 40) for c in (0, 1, 2, 3, 4, 30)] + [(h, 0), (h + 3, 0), (h + 40, 0), (offs[21] - 1, 20), (2 * W, 21), (2 * W + 1, 21)]
    for end, k in cuts:
        host, dev = both(L, blob[:end], chain)
        assert dev == host, end
        assert host["rec_off"] == offs[:k] and host["consumed"] == offs[k] and host["first_bad"] == 2 ** 64 - 1, (end, k)
    return "%d ends" % len(cuts)


def malformed(L, chain, W, d):
    """the malformed streams: both backends name the same record and the same code"""
    bad = lc.malformed()
    for name, (blob, say) in sorted(bad.items()):
        host, dev = both(L, blob, chain)
        for k in ("rec_off", "consumed", "first_bad", "code"):
            assert dev[k] == host[k], (name, k)
        if name.startswith("cut_"):
            assert host["first_bad"] == 2 ** 64 - 1 and host["consumed"] < len(blob), name
        else:
            assert host["first_bad"] == 7 and host["code"] >= 3, name
    return "%d streams" % len(bad)


def abi(L, chain, W, d):
    """al_lift_bam: the counts, the output, and no device memory held at return, on the device, with the device compressor and on the twin"""
    from test_lift_cpu import check
    recs = lc.directed(257) + lc.walk_sets(W)["long"]
    bam = os.path.join(d, "abi.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 700))
    v = lc.lift_all(lc.CHAIN, lc.REFS, recs)[0]
    out, bed = os.path.join(d, "abi_out.bam"), os.path.join(d, "abi_out.bed")
    for flags in (0, capi.LIFT_GPU_DEFLATE, capi.LIFT_HOST):
        st = capi.lift_bam(bam, chain, out, bed, flags=flags, piece_bytes=4096)
        assert (st.kept, st.unlifted, st.unmapped_kept) == (v.count(lc.KEPT), v.count(lc.UNLIFTED), v.count(lc.UNMAPPED))
        assert st.held == 0 and st.on_device == (0 if flags == capi.LIFT_HOST else 1) and st.pieces > 3
        check(type("R", (), dict(returncode=0, stderr=b""))(), out, bed, lc.HEADER, lc.REFS, recs)
    return "3 forms"


def main():
    what, d = sys.argv[1], sys.argv[2]
    L = capi.load()
    chain = os.path.join(d, "child.chain"); open(chain, "w").write(lc.CHAIN)
    print("ok", what, {"kernels": kernels, "ends": ends, "malformed": malformed, "abi": abi}[what](L, chain, L.al_dbg_lift_window(), d))


if __name__ == "__main__":
    main()
