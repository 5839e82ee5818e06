"""The BAM record formatter the GPU runs (al_dev_bam.h: k_bam_len / k_bam_write / k_bam_bulk of al_stream.hip), compiled for the CPU and pinned
against the host writer al_write_bam_rec (al_bam.cpp), which tests/test_gpu_sam.py pins against the reference's SAM text.  No GPU needed."""
import struct

import pytest


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_device_bam_formatter_equals_host_writer(seed):
    """8000 random fragments: hits with inline and arena CIGARs, supplementary and secondary records, flipped mates, unmapped reads with and
    without a mapped mate, -Y, MD / cs, a read group, reads of 1 .. 4 bases, odd and even lengths, reads without quality, IUPAC / lowercase / U /
    bytes >= 128 in SEQ, names around 254 bytes; a third of them in the coordinate-sorted form (unmapped records left out, sort keys).  Bytes of
    every record, the length pass, record counts, keys, offsets and lengths must be the host writer's."""
    import airlift_amd as A
    L = A.load()
    assert L.al_dbg_bam_selftest(seed, 8000) == 0


def test_de_float_is_the_float_of_the_four_digit_text():
    """de:f is stored as (float)atof("%.4f" text) by the host writer; the formatter gets the text's digits q from al_fmt_f4 and must give the same
    float for every q the tag can take (0 <= q / 10000 <= 1)."""
    import airlift_amd as A
    L = A.load()
    bad = [q for q in range(10001) if struct.pack("<I", L.al_dbg_bam_de_bits(q)) != struct.pack("<f", float("%.4f" % (q / 10000)))]
    assert not bad, bad[:10]
