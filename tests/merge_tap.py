"""The test taps of `merge` (al_dbg_merge_host, al_dbg_merge of include/airlift.h) behind one Python call."""
import ctypes as C

import merge_cases as mc


def tap(L, inputs, piece, dev=None, expect=0):
    """k inputs (merge_cases) as uncompressed streams through the round loop of the host twin (dev None) or of the kernels: piece 0 makes one round with every
    input at eof.  -> dict(tags, keys, packed, rounds); the return code must be `expect`"""
    blobs = [mc.stream(x) if not isinstance(x, bytes) else x for x in inputs]; k = len(blobs)
    arr = (C.c_char_p * k)(*blobs); ns = (C.c_size_t * k)(*[len(b) for b in blobs])
    n_cap = sum(len(b) for b in blobs) // 36 + 2; cap = sum(len(b) for b in blobs) + 64
    tags = (C.c_uint32 * n_cap)(); keys = (C.c_uint64 * n_cap)(); packed = C.create_string_buffer(cap)
    n_out, packed_n, held, rounds = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
    if dev is None:
        rc = L.al_dbg_merge_host(arr, ns, k, piece, tags, keys, n_cap, C.byref(n_out), packed, cap, C.byref(packed_n), C.byref(rounds))
    else:
        rc = L.al_dbg_merge(dev, arr, ns, k, piece, tags, keys, n_cap, C.byref(n_out), packed, cap, C.byref(packed_n), C.byref(rounds), C.byref(held))
    assert rc == expect, rc
    assert held.value == 0
    return dict(tags=list(tags[:n_out.value]), keys=list(keys[:n_out.value]), packed=packed.raw[:packed_n.value], rounds=rounds.value)
