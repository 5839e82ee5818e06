"""The in-process GPU steps of tests/test_gpu_lift_sorted.py, in a process of its own so that the test can run them under a time limit: the taps of
lift --sorted (al_dbg_lift_sorted against al_dbg_lift_sorted_host against the rules of tests/lift_sort_cases.py), the order made on the host when the sort's
temporaries are refused, and the C ABI (al_lift_bam with capi.LIFT_SORTED).

usage: lift_sort_child.py taps|fallback|abi WORKDIR
An assertion that fails ends the process with its traceback; otherwise the last line printed is "ok <what ran>"."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lift_cases as lc  # noqa: E402
import lift_sort_cases as ls  # noqa: E402
from select_cases import bgzf  # noqa: E402
from airlift_amd import capi  # noqa: E402
from lift_child import rows_of_arena, tap  # noqa: E402


def tap_sorted(L, blob, chain, dev=None, tap_flags=0):
    n_cap = len(blob) // 36 + 2; cap = len(blob) + 8 * n_cap + 64
    rec_off = (C.c_uint32 * n_cap)(); verdict = (C.c_uint32 * n_cap)(); perm = (C.c_uint32 * n_cap)(); out4 = (C.c_uint64 * 4)(); sort3 = (C.c_uint64 * 3)()
    packed = C.create_string_buffer(cap); arena = C.create_string_buffer(cap); packed_n, arena_n, held = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    if dev is None:
        rc = L.al_dbg_lift_sorted_host(blob, len(blob), chain.encode(), rec_off, verdict, n_cap, out4, packed, cap, C.byref(packed_n), arena, cap, C.byref(arena_n), perm, sort3)
    else:
        rc = L.al_dbg_lift_sorted(dev, blob, len(blob), chain.encode(), rec_off, verdict, n_cap, out4, packed, cap, C.byref(packed_n), arena, cap, C.byref(arena_n), perm, sort3, tap_flags, C.byref(held))
    assert rc == 0, rc
    assert held.value == 0
    n = out4[0]
    return dict(rec_off=list(rec_off[:n]), verdict=list(verdict[:n]), consumed=out4[1], first_bad=out4[2], code=out4[3], packed=packed.raw[:packed_n.value], arena=arena.raw[:arena_n.value],
                perm=list(perm[:sort3[0]]), descents=sort3[1], sort_launched=sort3[2])


def cases(W, d):
    chains = {}
    for i, text in enumerate((lc.CHAIN, ls.BIG_CHAIN)):
        chains[text] = os.path.join(d, "sort_child%d.chain" % i); open(chains[text], "w").write(text)
    return sorted(ls.self_check(W).items()), chains


def taps(L, W, d):
    """device tap == host tap == Python on every set: perm, packed bytes, descents, sort_launched, arena, verdicts; a piece in order launches no sort and its
    packed bytes are the flagless tap's"""
    sets, chains = cases(W, d)
    n_sorted = n_in_order = 0
    for name, (chain_text, recs) in sets:
        blob = lc.bam_bytes(lc.HEADER, lc.REFS, recs); chain = chains[chain_text]
        host, dev = tap_sorted(L, blob, chain), tap_sorted(L, blob, chain, 0)
        assert dev == host, name
        t = ls.truth(chain_text, lc.REFS, recs)
        assert host["verdict"] == t["v"] and host["consumed"] == len(blob) and host["first_bad"] == 2 ** 64 - 1, name
        assert host["perm"] == t["perm"] and host["packed"] == t["packed"] and host["descents"] == t["descents"] and host["sort_launched"] == (1 if t["descents"] else 0), name
        assert rows_of_arena(host["arena"], lc.REFS) == t["rows"], name
        plain = tap(L, L.al_dbg_lift, blob, chain, 0)
        assert plain["arena"] == dev["arena"] and plain["packed"] == t["unsorted"], name
        if t["descents"] == 0:
            assert dev["sort_launched"] == 0 and dev["packed"] == plain["packed"], name
            n_in_order += 1
        else:
            n_sorted += 1
    assert n_in_order >= 6 and n_sorted >= 20
    return "%d sets" % len(sets)


def fallback(L, W, d):
    """the sort's temporaries refused: the order is made on the host from the keys, no sort is launched, and the result is the same"""
    sets, chains = cases(W, d)
    n = 0
    for name, (chain_text, recs) in sets:
        if name not in ("kept2", "kept65", "kept257", "one_descent299", "equal_desc", "big_pos", "walk_long", "in_order65"):
            continue
        blob = lc.bam_bytes(lc.HEADER, lc.REFS, recs); t = ls.truth(chain_text, lc.REFS, recs)
        dev = tap_sorted(L, blob, chains[chain_text], 0, tap_flags=1)
        assert dev["perm"] == t["perm"] and dev["packed"] == t["packed"] and dev["descents"] == t["descents"] and dev["sort_launched"] == 0, name
        n += 1
    assert n == 8
    return "%d sets" % n


def abi(L, W, d):
    """al_lift_bam with the sorted flag, alone and with the device compressor: the counts of the flagless call, no device memory held, more than three pieces"""
    recs = lc.directed(257) + lc.walk_sets(W)["long"]
    bam = os.path.join(d, "sabi.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 700))
    chain = os.path.join(d, "sabi.chain"); open(chain, "w").write(lc.CHAIN)
    t = ls.truth(lc.CHAIN, lc.REFS, recs); v = t["v"]
    out, bed = os.path.join(d, "sabi_out.bam"), os.path.join(d, "sabi_out.bed")
    st0 = capi.lift_bam(bam, chain, out, bed, flags=0, piece_bytes=4096)
    bed0 = open(bed, "rb").read()
    for flags in (capi.LIFT_SORTED, capi.LIFT_SORTED | capi.LIFT_GPU_DEFLATE, capi.LIFT_SORTED | capi.LIFT_HOST):
        st = capi.lift_bam(bam, chain, out, bed, flags=flags, piece_bytes=4096)
        assert (st.kept, st.unlifted, st.unmapped_kept) == (st0.kept, st0.unlifted, st0.unmapped_kept) == (v.count(lc.KEPT), v.count(lc.UNLIFTED), v.count(lc.UNMAPPED))
        assert st.held == 0 and st.on_device == (0 if flags & capi.LIFT_HOST else 1) and st.pieces > 3 and st.pieces == st0.pieces
        assert b"".join(ls.split_records(ls.inflate(out))) == t["packed"] and open(bed, "rb").read() == bed0
    return "3 forms"


def main():
    what, d = sys.argv[1], sys.argv[2]
    L = capi.load()
    print("ok", what, {"taps": taps, "fallback": fallback, "abi": abi}[what](L, L.al_dbg_lift_window(), d))


if __name__ == "__main__":
    main()
