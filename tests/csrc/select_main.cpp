// select_main.cpp -- the selector of --gpu-select on the host, stand-alone under AddressSanitizer + UBSan (`make san-select`): the name table's builder and
// the kernels' twin (al_dev_select.h) and the piece / carry / hand-over loop (al_select.h), host code only.
//
//   san_select LIST     LIST: one case per line, "<fastq file> <names file>" (names: one per line)
//
// Every case is walked at every piece size from 64 bytes to 256, then at sizes growing by 1/16 up to the text's length (every size of a text of at most
// 4096 bytes), each from exactly sized heap buffers.  What the walk selects, followed by what the default reader (AlSeqReader) selects from the hand-over
// offset on, must be what the default reader selects from the whole file.  One line per case, then "san_select: N files".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <string>
#include <unordered_set>
#include <vector>
#include "al_select.h"
#include "al_seqio.h"

struct Rec { std::string name, seq, qual; bool operator==(const Rec &o) const { return name == o.name && seq == o.seq && qual == o.qual; } };

static bool default_reader(const char *fn, const std::unordered_set<std::string> &want, long long from, std::vector<Rec> &out, uint64_t *walked)
{
	AlSeqReader rd;
	if (!rd.open(fn)) return false;
	if (from > 0 && !rd.seek(from)) return false;
	AlChunk c;
	for (;;) {
		c.text.clear(); c.recs.clear();
		if (!rd.read(c)) break;
		++*walked;
		const AlRec &r = c.recs[0];
		const char *nm = c.text.data() + r.name;
		if (!want.count(nm)) continue;
		Rec q; q.name = nm; q.seq.assign(c.text.data() + r.seq, r.len); if (r.qual != ~0u) q.qual.assign(c.text.data() + r.qual, r.len);
		out.push_back(q);
	}
	return true;
}

// the file's bytes from memory, every piece in a heap buffer of exactly its size (an overrun of a piece is an overrun of an allocation)
struct MemSource : AlSelSource {
	const std::vector<uint8_t> *text = nullptr; size_t pos = 0; uint8_t *buf[2] = {nullptr, nullptr}; size_t n[2] = {0, 0}; bool at_eof[2] = {false, false};
	~MemSource() { free(buf[0]); free(buf[1]); }
	int read(int slot, size_t want) override
	{
		free(buf[slot]); buf[slot] = nullptr;
		n[slot] = std::min(want, text->size() - pos); at_eof[slot] = n[slot] < want;
		if (n[slot]) { buf[slot] = (uint8_t *)malloc(n[slot]); memcpy(buf[slot], text->data() + pos, n[slot]); pos += n[slot]; }
		return 0;
	}
	int push(AlSelBackend &B, int slot, bool *eof) override { *eof = at_eof[slot]; return n[slot] ? B.append(slot, buf[slot], n[slot]) : 0; }
	size_t pending(int slot) const override { return n[slot]; }
};

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: san_select LIST\n"); return 2; }
	std::ifstream lst(argv[1]); std::string fq, nm; int n_files = 0;
	while (lst >> fq >> nm) {
		std::vector<uint8_t> text;
		{ std::ifstream f(fq, std::ios::binary); text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
		std::unordered_set<std::string> want;
		{ std::ifstream f(nm); std::string l; while (std::getline(f, l)) want.insert(l); }
		AlSelNames N;
		if (al_sel_build(want, N)) { fprintf(stderr, "%s: al_sel_build failed\n", fq.c_str()); return 1; }
		// the table answers for every name of the list, and for none of a few that are not in it
		const AlSelTable T = N.table();
		for (const std::string &s : want) if (!al_sel_probe(T, (const uint8_t *)s.data(), (uint32_t)s.size())) { fprintf(stderr, "%s: '%s' not found in its table\n", fq.c_str(), s.c_str()); return 1; }
		for (const std::string &s : want) { const std::string x = s + "#"; if (!want.count(x) && al_sel_probe(T, (const uint8_t *)x.data(), (uint32_t)x.size())) { fprintf(stderr, "%s: '%s' found\n", fq.c_str(), x.c_str()); return 1; } }
		std::vector<Rec> ref; uint64_t ref_walked = 0;
		if (!default_reader(fq.c_str(), want, -1, ref, &ref_walked)) { fprintf(stderr, "%s: cannot be read\n", fq.c_str()); return 1; }
		std::vector<Rec> rest; uint64_t rest_walked = 0, rest_at = ~0ull;      // what the default reader selects from the hand-over offset on
		size_t sizes = 0; uint64_t tested_full = 0, handed_full = 0, hand_full = ~0ull;
		const size_t len = text.size() < 64 ? 64 : text.size();
		for (size_t piece = 64; ; ) {
			std::vector<Rec> got; uint64_t handover = ~0ull; AlSelStat st;
			AlSelHostBackend B(T); MemSource src; src.text = &text;
			const int rc = al_select_file(B, src, piece, [&](const uint8_t *arena, const AlSelDesc *d, size_t n) -> int {
				for (size_t k = 0; k < n; ++k) { const char *p = (const char *)arena + d[k].off; got.push_back(Rec{std::string(p, d[k].name_len), std::string(p + d[k].name_len, d[k].len), std::string(p + d[k].name_len + d[k].len, d[k].len)}); }
				return 0;
			}, &handover, st);
			if (rc) { fprintf(stderr, "%s: piece %zu: al_select_file failed\n", fq.c_str(), piece); return 1; }
			uint64_t handed = 0;
			if (handover != ~0ull) {                                       // (the reader's 5 MB of buffers are set up once per offset, not once per piece size)
				if (handover != rest_at) { rest.clear(); rest_walked = 0; rest_at = handover; if (!default_reader(fq.c_str(), want, (long long)handover, rest, &rest_walked)) { fprintf(stderr, "%s: piece %zu: hand-over at %llu failed\n", fq.c_str(), piece, (unsigned long long)handover); return 1; } }
				got.insert(got.end(), rest.begin(), rest.end()); handed = rest_walked;
			}
			if (!(got == ref)) { fprintf(stderr, "%s: piece %zu: %zu records, the default reader selects %zu (or they differ)\n", fq.c_str(), piece, got.size(), ref.size()); return 1; }
			if (st.tested + handed != ref_walked) { fprintf(stderr, "%s: piece %zu: %llu tested + %llu handed over, the default reader walks %llu\n", fq.c_str(), piece, (unsigned long long)st.tested, (unsigned long long)handed, (unsigned long long)ref_walked); return 1; }
			if (sizes && (handover != hand_full || st.tested != tested_full)) { fprintf(stderr, "%s: piece %zu: hand-over %llu after %llu records, before it %llu after %llu\n", fq.c_str(), piece, (unsigned long long)handover, (unsigned long long)st.tested, (unsigned long long)hand_full, (unsigned long long)tested_full); return 1; }
			hand_full = handover; tested_full = st.tested; handed_full = handed; ++sizes;
			if (piece >= len) break;
			const size_t next = (piece < 256 || len <= 4096) ? piece + 1 : piece + piece / 16;
			piece = next > len ? len : next;
		}
		printf("case %d sizes=%zu selected=%zu tested=%llu handed=%llu handover=%lld\n", n_files, sizes, ref.size(), (unsigned long long)tested_full, (unsigned long long)handed_full, hand_full == ~0ull ? -1LL : (long long)hand_full);
		++n_files;
	}
	printf("san_select: %d files\n", n_files);
	return 0;
}
