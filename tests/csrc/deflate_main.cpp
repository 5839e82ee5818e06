// deflate_main.cpp -- the BGZF compressor's host twin (al_dev_deflate.h) as a stand-alone program for AddressSanitizer + UBSan (`make san-deflate`):
// every file named on the command line is cut into BGZF blocks from a heap buffer of exactly its size (so a read past the end is seen), each block is
// compressed at the given level into a buffer of exactly 65536 bytes, checked (header, BSIZE, CRC32, ISIZE, the n + 31 bound) and inflated with zlib.
// usage: san_deflate LEVEL FILE...   exit status 0 when every block came back.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <vector>
#include "al_dev_deflate.h"

static int check_block(const uint8_t *in, uint32_t n, int level, const char *fn, size_t off)
{
	uint8_t *src = (uint8_t *)malloc(n), *dst = (uint8_t *)malloc(AL_DFL_SLOT), *back = (uint8_t *)malloc(n);
	memcpy(src, in, n);
	int stored = -1, bad = 0;
	const uint32_t total = al_deflate_block_host(src, n, level, dst, &stored);
	if (total > AL_DFL_SLOT || total > n + 31 || total < 28) bad = 1;
	if (!bad && (dst[0] != 0x1f || dst[1] != 0x8b || dst[12] != 'B' || dst[13] != 'C' || (uint32_t)(dst[16] | dst[17] << 8) != total - 1)) bad = 2;
	if (!bad && level == 0 && !stored) bad = 3;
	if (!bad) {
		z_stream zs; memset(&zs, 0, sizeof(zs));
		if (inflateInit2(&zs, -15) != Z_OK) bad = 4;
		else {
			zs.next_in = dst + 18; zs.avail_in = total - 26; zs.next_out = back; zs.avail_out = n;
			if (inflate(&zs, Z_FINISH) != Z_STREAM_END || zs.total_out != n || zs.avail_in != 0 || memcmp(back, src, n) != 0) bad = 5;
			inflateEnd(&zs);
		}
	}
	if (!bad) {
		uint32_t crc, isz; memcpy(&crc, dst + total - 8, 4); memcpy(&isz, dst + total - 4, 4);
		if (crc != (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, n) || isz != n) bad = 6;
	}
	if (bad) fprintf(stderr, "%s: block at %zu (%u bytes, level %d): check %d failed\n", fn, off, n, level, bad);
	free(src); free(dst); free(back);
	return bad;
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: %s LEVEL FILE...\n", argv[0]); return 2; }
	const int level = atoi(argv[1]);
	size_t blocks = 0;
	for (int a = 2; a < argc; ++a) {
		FILE *f = fopen(argv[a], "rb");
		if (!f) { perror(argv[a]); return 2; }
		std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t k;
		while ((k = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + k);
		fclose(f);
		for (size_t o = 0; o < buf.size(); o += AL_DFL_BLOCK, ++blocks) {
			const uint32_t n = (uint32_t)(buf.size() - o < AL_DFL_BLOCK ? buf.size() - o : AL_DFL_BLOCK);
			if (check_block(buf.data() + o, n, level, argv[a], o)) return 1;
		}
	}
	printf("san_deflate: %zu blocks at level %d\n", blocks, level);
	return 0;
}
