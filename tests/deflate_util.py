"""Helpers of the BGZF compressor's tests: the taps of airlift_amd/capi.py as bytes in, bytes out, and a BGZF member walker."""
import ctypes as C
import struct
import zlib

from airlift_amd import capi

BLOCK = 0xff00
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _cap(n):
    return n + 64 * (n // BLOCK + 2) + 1024


def deflate_host(data, level=5):
    """(members, stored blocks) from the host twin"""
    L = capi.load()
    dst = C.create_string_buffer(_cap(len(data))); on = C.c_size_t(0); ns = C.c_size_t(0)
    rc = L.al_dbg_bgzf_deflate_host(data, len(data), level, dst, len(dst), C.byref(on), C.byref(ns))
    assert rc == 0, rc
    return dst.raw[:on.value], ns.value


def deflate_device(data, level=5, device=0):
    """(members, stored blocks) from the kernel, through the device backend"""
    L = capi.load()
    dst = C.create_string_buffer(_cap(len(data))); on = C.c_size_t(0); ns = C.c_size_t(0)
    rc = L.al_dbg_bgzf_deflate(device, data, len(data), level, dst, len(dst), C.byref(on), C.byref(ns))
    assert rc == 0, rc
    return dst.raw[:on.value], ns.value


def stream_device(data, piece, level=5, device=0):
    """a whole BGZF file from AlBgzf with the device backend, written in calls of `piece` bytes"""
    L = capi.load()
    dst = C.create_string_buffer(_cap(len(data)) + 28); on = C.c_size_t(0)
    rc = L.al_dbg_bgzf_stream(device, data, len(data), piece, level, dst, len(dst), C.byref(on))
    assert rc == 0, rc
    return dst.raw[:on.value]


def members(z):
    """[(member bytes, inflated bytes)] of a BGZF byte string: BC field and BSIZE checked, raw deflate inflated, CRC32 and ISIZE checked"""
    out, o = [], 0
    while o < len(z):
        assert z[o:o + 4] == b"\x1f\x8b\x08\x04" and z[o + 10:o + 16] == b"\x06\x00BC\x02\x00", "no BGZF header at %d" % o
        size = struct.unpack_from("<H", z, o + 16)[0] + 1
        assert o + size <= len(z) and size <= 65536
        m = z[o:o + size]
        d = zlib.decompressobj(-15)
        raw = d.decompress(m[18:-8])
        assert d.eof and d.unused_data == b"", "the deflate stream does not end where BSIZE says"
        crc, isize = struct.unpack("<II", m[-8:])
        assert isize == len(raw) and crc == zlib.crc32(raw)
        out.append((m, raw))
        o += size
    return out


def is_stored(member):
    return member[18] & 7 == 1


def stream_device_resident(data, piece, mix=False, ring=1 << 16, level=5, device=0):
    """the same file with every call's bytes lying in device memory (AlBgzf::write_device, the stream driver's --bam --gpu-deflate path: the carry goes
    up into the seam buffer, the members leave through two page-locked buffers of `ring` bytes); mix: every second call from the host instead"""
    L = capi.load()
    dst = C.create_string_buffer(_cap(len(data)) + 28); on = C.c_size_t(0)
    rc = L.al_dbg_bgzf_stream_dev(device, data, len(data), piece, 1 if mix else 0, ring, level, dst, len(dst), C.byref(on))
    assert rc == 0, rc
    return dst.raw[:on.value]
