"""Helpers of the BGZF inflater's tests: the taps of airlift_amd/capi.py as bytes in, (rc, bytes, statuses) out."""
import ctypes as C
import struct

from airlift_amd import capi


def _room(data):
    """(members, output bytes) an upper bound of what the BSIZE chain of `data` can reach: BSIZE at the BC subfield's usual place where the magic is there"""
    o, n, out = 0, 0, 0
    while o + 18 <= len(data) and data[o:o + 2] == b"\x1f\x8b":
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        ex = data[o + 12:o + 12 + xlen]; k = ex.find(b"BC\x02\x00")
        if k < 0 or k + 6 > len(ex):
            break
        size = struct.unpack_from("<H", ex, k + 4)[0] + 1
        n += 1; out += 65536; o += size
    return n + 2, out + 65536


def _run(fn, data, head=()):
    n_status, cap = _room(data)
    dst = C.create_string_buffer(cap); on = C.c_size_t(0); nm = C.c_size_t(0); st = (C.c_uint32 * n_status)()
    rc = fn(*head, data, len(data), dst, cap, C.byref(on), st, n_status, C.byref(nm))
    return rc, dst.raw[:on.value], list(st[:nm.value])


def inflate_host(data):
    """the host twin over every member of `data`"""
    return _run(capi.load().al_dbg_bgzf_inflate_host, data)


def inflate_device(data, device=0, guard=False):
    """k_inflate over the whole member list in one launch (guard: between two poisoned ranges, rc -7 when one was written)"""
    L = capi.load()
    return _run(L.al_dbg_bgzf_inflate_guard if guard else L.al_dbg_bgzf_inflate, data, (device,))
