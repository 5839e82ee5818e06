// al_bgzf_take.h -- BGZF FASTQ input of the stream driver (--gpu-inflate on the mapping commands), host side: the compressed bytes of one file as they
// arrive in pieces, and the function that takes whole members off their front for one launch of the inflater.  Host code only, no HIP include, so that
// tests/csrc/bgzf_take_main.cpp can run it stand-alone under the sanitizers.
//
// AlBgzfFeed is a window buf[beg, end) over the file's compressed bytes: the caller reads the next piece to al_bgzf_feed_room() and says how much came
// (al_bgzf_feed_add); a member cut by a piece's end simply stays in the window until the next piece completes it (the carry).  al_bgzf_take walks the
// BSIZE chain from the window's front and lists whole members -- ISIZE from each trailer -- until `want_out` inflated bytes are covered, the window has
// no whole member left, or one launch's limits (staging bytes, members) are reached.  What it lists is taken: the window's front moves behind it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <vector>
#include "al_dev_inflate.h"

struct AlBgzfFeed {
	uint8_t *buf = nullptr; size_t cap = 0, beg = 0, end = 0;     // the caller's buffer (page-locked in the driver); cap >= piece + 65536 keeps room for a piece behind a cut member
	uint64_t file_off = 0, out_off = 0;                            // file offset of buf[beg]; offset in the inflated stream of the next member's first byte
};
// room for the next piece: the window is moved to the buffer's front; *room bytes may be written at the returned address
static inline uint8_t *al_bgzf_feed_room(AlBgzfFeed &f, size_t *room)
{
	if (f.beg) { memmove(f.buf, f.buf + f.beg, f.end - f.beg); f.end -= f.beg; f.beg = 0; }
	*room = f.cap - f.end;
	return f.buf + f.end;
}
static inline void al_bgzf_feed_add(AlBgzfFeed &f, size_t n) { f.end += n; }
static inline size_t al_bgzf_feed_left(const AlBgzfFeed &f) { return f.end - f.beg; }

enum { AL_BGZF_COVERED = 0, AL_BGZF_MORE = 1, AL_BGZF_FULL = 2, AL_BGZF_BROKEN = -1 };
// One launch's members off the front of the window.  mem: cleared, then an entry per member taken, in_off relative to *bytes, out_off relative to the
// launch's output (the prefix sum of ISIZE from 0); *n_in / *n_out: their compressed / inflated bytes; *file_off_at: the file offset of (*bytes)[0].
//   AL_BGZF_COVERED  *n_out >= want_out (members are taken while the sum is still short of it: the last one may overshoot by up to 65 535 bytes)
//   AL_BGZF_MORE     the window holds no further whole member: feed the next piece (at the end of the file: bytes left in the window are a cut member)
//   AL_BGZF_FULL     max_in compressed bytes or max_mem members reached: launch these and call again
//   AL_BGZF_BROKEN   the bytes at the window's front (file offset f.file_off) are no BGZF member; what was listed before them is still taken
static inline int al_bgzf_take(AlBgzfFeed &f, uint64_t want_out, uint64_t max_in, size_t max_mem, std::vector<AlInfMember> &mem, const uint8_t **bytes, uint64_t *n_in, uint64_t *n_out, uint64_t *file_off_at)
{
	mem.clear();
	*bytes = f.buf + f.beg; *n_in = 0; *n_out = 0; *file_off_at = f.file_off;
	int rc = AL_BGZF_COVERED;
	while (*n_out < want_out) {
		const uint64_t left = (uint64_t)(f.end - f.beg);
		if (left == 0) { rc = AL_BGZF_MORE; break; }
		uint32_t msize = 0, hdr = 0;
		const int r = al_inf_parse_header(f.buf + f.beg, left, &msize, &hdr);
		if (r > 0) { rc = AL_BGZF_BROKEN; break; }
		if (r < 0 || msize > left) { rc = AL_BGZF_MORE; break; }
		const uint32_t isize = al_inf_le32(f.buf + f.beg + msize - 4);
		if (isize > AL_INF_MAX_ISIZE) { rc = AL_BGZF_BROKEN; break; }
		if (mem.size() >= max_mem || *n_in + msize > max_in) { rc = AL_BGZF_FULL; break; }
		mem.push_back(AlInfMember{*n_in, *n_out, msize, isize});
		*n_in += msize; *n_out += isize;
		f.beg += msize; f.file_off += msize; f.out_off += isize;
	}
	return rc;
}
// inflated / compressed bytes of the whole members at the window's front (nothing is taken): what the driver scales its file-size estimates by
static inline double al_bgzf_ratio(const AlBgzfFeed &f)
{
	uint64_t in = 0, out = 0; size_t p = f.beg;
	while (p < f.end) {
		uint32_t msize = 0, hdr = 0;
		if (al_inf_parse_header(f.buf + p, f.end - p, &msize, &hdr) != 0 || msize > f.end - p) break;
		in += msize; out += al_inf_le32(f.buf + p + msize - 4); p += msize;
	}
	return in && out ? (double)out / (double)in : 1.0;
}

// Where the pieces of a driver that walks a BGZF file come from (al_select.h, al_lift.h): compressed pieces by pread into the feed's window, whole members
// taken off its front and inflated into a slot's text by the driver's backend.  Backend: append_bgzf(), host_buffer(), host_buffer_free(); Source: the
// driver's source interface (read / push / pending, read_s, Timer).  tag: the option or command the messages name.  open(): the piece of compressed bytes,
// and where the first member lies in the file and in the inflated stream.
template <class Backend, class Source> struct AlBgzfPieceSource : Source {
	int fd = -1; uint64_t fpos = 0; Backend *B = nullptr; const char *tag = ""; AlBgzfFeed feed; size_t piece = 0, want_out[2] = {0, 0}; bool eof_file = false, own = false; const char *fn = "";
	size_t max_in = 0, max_mem = 0; std::vector<AlInfMember> mem;
	~AlBgzfPieceSource() { if (feed.buf) { if (own) free(feed.buf); else B->host_buffer_free(feed.buf); } }
	int open(size_t piece_bytes, uint64_t file_off = 0, uint64_t out_off = 0)
	{
		piece = piece_bytes; feed.cap = 2 * piece + 65536; fpos = file_off; feed.file_off = file_off; feed.out_off = out_off;
		feed.buf = (uint8_t *)B->host_buffer(feed.cap);
		if (!feed.buf) { feed.buf = (uint8_t *)malloc(feed.cap); own = true; }
		if (!feed.buf) { fprintf(stderr, "[ERROR] airlift: %s: no host memory for the BGZF window of '%s'\n", tag, fn); return -1; }
		max_in = feed.cap; max_mem = feed.cap / 28 + 16;           // (a member is at least 28 bytes)
		return 0;
	}
	int read_piece()
	{
		size_t room = 0; uint8_t *dst = al_bgzf_feed_room(feed, &room);
		size_t want = std::min(piece, room);
		typename Source::Timer tm(this->read_s);
		while (want) {
			const ssize_t g = pread(fd, dst, want, (off_t)fpos);
			if (g < 0) { fprintf(stderr, "[ERROR] airlift: %s: reading '%s' failed\n", tag, fn); return -1; }
			if (g == 0) { eof_file = true; break; }
			al_bgzf_feed_add(feed, (size_t)g); dst += g; fpos += (uint64_t)g; want -= (size_t)g;
		}
		return 0;
	}
	int read(int slot, size_t want) override { want_out[slot] = want; return 0; }
	size_t pending(int slot) const override { return want_out[slot] + 65536; }
	int push(Backend &Bk, int slot, bool *eof) override
	{
		uint64_t got = 0; *eof = false;
		while (got < want_out[slot]) {
			const uint8_t *bytes = nullptr; uint64_t n_in = 0, n_out = 0, at = 0;
			const int r = al_bgzf_take(feed, want_out[slot] - got, max_in, max_mem, mem, &bytes, &n_in, &n_out, &at);
			if (!mem.empty()) {
				size_t bad = 0; uint32_t bst = 0;
				const int ar = Bk.append_bgzf(slot, bytes, (size_t)n_in, mem.data(), mem.size(), n_out, &bad, &bst);
				if (ar > 0) fprintf(stderr, "[ERROR] airlift: %s: '%s': BGZF member at file offset %llu: status %u (%s)\n", tag, fn, (unsigned long long)(at + mem[bad].in_off), bst, al_inf_strerror((int)bst));
				if (ar) return -1;
				got += n_out;
			}
			if (r == AL_BGZF_BROKEN) { fprintf(stderr, "[ERROR] airlift: %s: '%s': no BGZF member at file offset %llu\n", tag, fn, (unsigned long long)feed.file_off); return -1; }
			if (r == AL_BGZF_MORE) {
				if (eof_file) {
					if (al_bgzf_feed_left(feed)) { fprintf(stderr, "[ERROR] airlift: %s: '%s': truncated BGZF member at file offset %llu\n", tag, fn, (unsigned long long)feed.file_off); return -1; }
					*eof = true; break;
				}
				if (read_piece()) return -1;
			}
		}
		return 0;
	}
};

