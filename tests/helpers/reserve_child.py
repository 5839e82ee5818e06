"""The child process of tests/test_gpu_reserve.py (one device memory reserve per process, and the environment switches are read once): a
reserve of 500 MB in chunks of 125 MB, then the index of a golden set built on the device and the set mapped through al_map_file_frag,
every device range of both coming from al_dev_malloc (airlift_amd/csrc/al_devmem.cpp).

usage: reserve_child.py <unpacked golden set> <output SAM>     (the environment may carry AL_TEST_POISON / AL_TEST_GUARD)
Prints one JSON line: the return codes, al_device_reserve_peak() and the line of al_device_reserve_report()."""
import ctypes as C
import json
import os
import sys

os.environ["AL_POOL_CHUNK_GB"] = "0.125"                                    # (before the library's first look at the environment)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    d, out_path = sys.argv[1], sys.argv[2]
    import airlift_amd as A
    L = A.load()
    m = json.load(open(os.path.join(d, "meta.json")))
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    res = {"rc_reserve": L.al_device_reserve(0, 500_000_000)}            # four chunks; the filler does not ask for a remainder below 64 MiB
    idx = A.Index(fasta=os.path.join(d, m["ref"]), on_device=0)
    fp = libc.fopen(out_path.encode(), b"wb")
    fns = (C.c_char_p * len(m["reads"]))(*[os.path.join(d, f).encode() for f in m["reads"]])
    res["rc_map"] = L.al_map_file_frag(idx.h, len(m["reads"]), fns, C.byref(idx.mo), 4, fp, m["rg"].encode() if m.get("rg") else None, 0)
    libc.fclose(fp)
    res["peak"] = L.al_device_reserve_peak()
    idx.close()
    fp = libc.fopen((out_path + ".report").encode(), b"wb")
    L.al_device_reserve_report(fp)
    libc.fclose(fp)
    res["report"] = open(out_path + ".report").read()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
