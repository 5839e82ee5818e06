// al_dev_bam.h -- the BAM alignment record (SAM specification 4.2) of one hit as one routine over a byte sink: the twin of al_dev_sam.h,
// compiled for the device (k_bam_len / k_bam_write, al_stream.hip) and, with AL_SAM_HOST, for the CPU (al_dbg_bam_selftest pins it byte
// for byte against al_write_bam_rec, al_bam.cpp, which tests/test_gpu_sam.py pins against the reference's SAM text).
//
// Same inputs as the SAM formatter: the device's own records in mapping orientation, un-flipped through al_sam_view.  Records are not
// 4-byte aligned in the stream, so a sink takes every multi-byte field as u16 / u32 and stores it as bytes.
#pragma once
#include "al_dev_sam.h"
#ifdef AL_SAM_HOST
#define AL_SHD static inline
#else
#define AL_SHD __host__ __device__ __forceinline__
#endif

// 4-bit code of a base: "=ACMGRSVTWYHKDBN", case-insensitive, anything else 15 (the table seq16 of al_bam.cpp; the slot's device table is filled from this)
AL_SHD uint8_t al_bam_code16(uint8_t c)
{
	if (c == '=') return 0;
	const uint8_t l = c | 0x20;                          // (a letter of either case, or not a letter at all: setting bit 5 maps nothing else into a-z)
	switch (l) {
	case 'a': return 1; case 'c': return 2; case 'm': return 3; case 'g': return 4; case 'r': return 5; case 's': return 6; case 'v': return 7; case 't': return 8;
	case 'w': return 9; case 'y': return 10; case 'h': return 11; case 'k': return 12; case 'd': return 13; case 'b': return 14;
	default: return 15;
	}
}
// de:f as the host stores it, (float)atof("%.4f" text): q = the text's digits (al_fmt_f4).  The double division is correctly rounded, which
// is what atof gives for a decimal of so few digits; a float division would round twice.
AL_SD float al_bam_de(bool neg, uint64_t q) { const double d = (double)q / 10000.0; return (float)(neg ? -d : d); }
AL_SD int al_bam_reg2bin(int64_t beg, int64_t end)
{   // SAM specification 5.3
	--end;
	if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}
// the name as stored: without a trailing /1 /2 in paired mode (bseq.h:31-36).  More than 254 bytes do not fit l_read_name: the sink is told.
template <class S>
AL_SD uint32_t al_bam_name_len(S &o, const AlSamRead &me, int n_seg)
{
	uint32_t l = me.name_len;
	if (n_seg > 1 && l >= 3) { const char c1 = o.peek(me.name + l - 1), c2 = o.peek(me.name + l - 2); if (c1 >= '0' && c1 <= '9' && c2 == '/') l -= 2; }
	if (l > 254) o.name_too_long();
	return l;
}
template <class S> AL_SD void al_bam_tag(S &o, const char *t, char type) { o.u8((uint8_t)t[0]); o.u8((uint8_t)t[1]); o.u8((uint8_t)type); }
template <class S> AL_SD void al_bam_tag_i(S &o, const char *t, int32_t x) { al_bam_tag(o, t, 'i'); o.u32((uint32_t)x); }

// One record, block_size included.  reg_idx < 0: the unmapped record of a read without hits.  Sink: u8 / u16 / u32 (little-endian), ch / num / cname
// (the text of SA:Z), txt(off, len) (bytes of the read's text), mem(p, len), seq4(off, len, rev) (len bases as (len + 1) / 2 bytes of 4-bit codes,
// reverse-complemented if rev), qual(off, len, rev) (len bytes - 33), fill(byte, len), tag(k), begin_record() (by the caller) and end_record(key), which
// patches block_size and takes the coordinate-sort key refID << 32 | pos (~0 without a position).
template <class S>
AL_SD void al_bam_record(S &o, const AlSamCfg &C, const AlSamRead &me, const AlSamRead *mate, int seg_idx, int n_seg, int reg_idx, int rep_len)
{
	const AlReg *regs = me.regs; const int n_regs = me.n_regs;
	const AlReg *r = n_regs > 0 && reg_idx >= 0 && reg_idx < n_regs ? &regs[reg_idx] : nullptr;
	const AlReg *r_next = nullptr; AlSamView vn{0, 0, 0};
	if (n_seg > 1 && mate) { const int p = al_sam_pri_idx(mate->regs, mate->n_regs); if (p >= 0) { r_next = &mate->regs[p]; vn = al_sam_view(*r_next, mate->qlen, mate->flip); } }
	const AlReg *r_prev = r_next;
	AlSamView v{0, 0, 0}; if (r) v = al_sam_view(*r, me.qlen, me.flip);
	const int l_seq = me.qlen;
	int this_rid = -1, this_pos = -1, flag, mapq = 0;
	flag = n_seg > 1 ? 0x1 : 0x0;
	if (!r) flag |= 0x4;
	else { if (v.rev) flag |= 0x10; if (r->parent != r->id) flag |= 0x100; else if (!(r->flags & ALR_SAM_PRI)) flag |= 0x800; }
	if (n_seg > 1) {
		if (r && (r->flags & ALR_PROPER)) flag |= 0x2;
		if (seg_idx == 0) flag |= 0x40; else if (seg_idx == n_seg - 1) flag |= 0x80;
		if (!r_next) flag |= 0x8; else if (vn.rev) flag |= 0x20;
	}
	const uint32_t n_cig = r ? al_sam_ncig(*r) : 0u;
	const uint32_t *cig = r && n_cig ? al_sam_cig(*r, me.arena) : nullptr;
	uint32_t clip_op = 4; int c0 = 0, c1 = 0;
	if (!r) { if (r_prev) { this_rid = r_prev->rid; this_pos = r_prev->rs; } }     // an unmapped read takes its mate's position
	else {
		this_rid = r->rid; this_pos = r->rs; mapq = (int)(r->mapq & 0xff);
		if (n_cig) { clip_op = (flag & 0x800) && !C.softclip ? 5 : 4; c0 = v.rev ? l_seq - v.qe : v.qs; c1 = v.rev ? v.qs : l_seq - v.qe; }
	}
	const uint32_t n_cig_out = n_cig ? n_cig + (c0 ? 1u : 0u) + (c1 ? 1u : 0u) : 0u;
	int next_rid = -1, next_pos = -1, tlen = 0;
	if (n_seg > 1) {
		if (this_rid >= 0 && r_next) {
			if (this_rid == r_next->rid && r) { const int a5 = v.rev ? r->re - 1 : this_pos, b5 = vn.rev ? r_next->re - 1 : r_next->rs; tlen = b5 - a5; }
			next_rid = r_next->rid; next_pos = r_next->rs;
		} else if (r_next) { next_rid = r_next->rid; next_pos = r_next->rs; }
		else if (this_rid >= 0) { next_rid = this_rid; next_pos = this_pos; }
		if (tlen > 0) ++tlen; else if (tlen < 0) --tlen;
	}
	// SEQ / QUAL as printed (format.c:480-503): the whole read; nothing on a secondary record; [qs, qe) on a hard-clipped supplementary one
	uint32_t sq = me.seq, ql = me.qual; int sl = l_seq, rev = 0;
	if (r) {
		if ((flag & 0x900) == 0 || C.softclip) rev = v.rev;
		else if (flag & 0x100) sl = 0;
		else { sq = me.seq + (uint32_t)v.qs; ql = me.qual + (uint32_t)v.qs; sl = v.qe - v.qs; rev = v.rev; }
	}
	int64_t ref_end = (int64_t)this_pos + 1;
	if (n_cig) {
		int64_t e = this_pos;
		for (uint32_t k = 0; k < n_cig; ++k) { const uint32_t op = cig[k] & 0xf; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) e += cig[k] >> 4; }
		ref_end = e > this_pos ? e : (int64_t)this_pos + 1;
	}
	const uint32_t nl = al_bam_name_len(o, me, n_seg);
	o.u32(0);                                                              // block_size: end_record() patches it
	o.u32((uint32_t)this_rid); o.u32((uint32_t)this_pos);                   // 0-based pos; -1 when absent
	o.u8((uint8_t)(nl + 1)); o.u8((uint8_t)mapq); o.u16((uint16_t)al_bam_reg2bin(this_pos < 0 ? -1 : this_pos, this_pos < 0 ? 0 : ref_end));
	o.u16((uint16_t)n_cig_out); o.u16((uint16_t)flag); o.u32((uint32_t)sl);
	o.u32((uint32_t)next_rid); o.u32((uint32_t)next_pos); o.u32((uint32_t)tlen);
	o.txt(me.name, nl); o.u8(0);
	if (n_cig) {
		if (c0) o.u32((uint32_t)c0 << 4 | clip_op);
		for (uint32_t k = 0; k < n_cig; ++k) o.u32(cig[k]);
		if (c1) o.u32((uint32_t)c1 << 4 | clip_op);
	}
	o.seq4(sq, sl, rev);
	if (me.qual != ~0u) o.qual(ql, sl, rev); else o.fill(0xff, sl);
	if (C.rg_len > 0) { al_bam_tag(o, "RG", 'Z'); o.mem(C.rg_id, C.rg_len); o.u8(0); }
	if (r) {
		const char type = r->id == r->parent ? 'P' : 'S';                   // inversions do not occur on this path (inv = 0)
		if (n_cig) { al_bam_tag_i(o, "NM", r->blen - r->mlen + (int)r->n_ambi); al_bam_tag_i(o, "ms", r->dp_max); al_bam_tag_i(o, "AS", r->dp_score); al_bam_tag_i(o, "nn", (int)r->n_ambi); }
		al_bam_tag(o, "tp", 'A'); o.u8((uint8_t)type); al_bam_tag_i(o, "cm", r->cnt); al_bam_tag_i(o, "s1", r->score);
		if (r->parent == r->id) al_bam_tag_i(o, "s2", r->subsc);
		if (n_cig) {
			int n_gapo = 0, n_gap = 0;
			for (uint32_t i = 0; i < n_cig; ++i) { const int op = cig[i] & 0xf, len = (int)(cig[i] >> 4); if (op == 1 || op == 2) ++n_gapo, n_gap += len; }
			const double div = 1.0 - (double)r->mlen / (double)(r->blen - n_gap + n_gapo);
			float de = 0.0f;
			if (div != 0.0) { bool neg; uint64_t q; al_fmt_f4(div, &neg, &q); de = al_bam_de(neg, q); }
			uint32_t u; __builtin_memcpy(&u, &de, 4);
			al_bam_tag(o, "de", 'f'); o.u32(u);
		}
		if (r->flags & 3u) al_bam_tag_i(o, "zd", (int)(r->flags & 3u));
		if (r->parent == r->id && n_cig && n_regs > 1) {
			int n_sa = 0;
			for (int i = 0; i < n_regs; ++i) if (i != reg_idx && regs[i].parent == regs[i].id && al_sam_ncig(regs[i])) ++n_sa;
			if (n_sa > 0) {
				al_bam_tag(o, "SA", 'Z');
				for (int i = 0; i < n_regs; ++i) {
					const AlReg *q = &regs[i]; int l_M, l_I = 0, l_D = 0;
					if (i == reg_idx || q->parent != q->id || al_sam_ncig(*q) == 0) continue;
					const AlSamView vq = al_sam_view(*q, me.qlen, me.flip);
					if (vq.qe - vq.qs < q->re - q->rs) l_M = vq.qe - vq.qs, l_D = (q->re - q->rs) - l_M;
					else l_M = q->re - q->rs, l_I = (vq.qe - vq.qs) - l_M;
					const int clip5 = vq.rev ? l_seq - vq.qe : vq.qs, clip3 = vq.rev ? vq.qs : l_seq - vq.qe;
					o.cname(q->rid); o.ch(','); o.num(q->rs + 1); o.ch(','); o.ch("+-"[vq.rev]); o.ch(',');
					if (clip5) { o.num(clip5); o.ch('S'); }
					if (l_M) { o.num(l_M); o.ch('M'); }
					if (l_I) { o.num(l_I); o.ch('I'); }
					if (l_D) { o.num(l_D); o.ch('D'); }
					if (clip3) { o.num(clip3); o.ch('S'); }
					o.ch(','); o.num((int)(q->mapq & 0xff)); o.ch(','); o.num(q->blen - q->mlen + (int)q->n_ambi); o.ch(';');
				}
				o.u8(0);
			}
		}
		if (C.tag_kind && n_cig) { al_bam_tag(o, C.tag_kind == 1 ? "MD" : "cs", 'Z'); o.tag((uint64_t)(r - C.tag_reg0)); o.u8(0); }
	}
	if (rep_len >= 0) al_bam_tag_i(o, "rl", rep_len);
	o.end_record(this_rid < 0 ? ~0ULL : ((uint64_t)(uint32_t)this_rid << 32 | (uint32_t)(this_pos < 0 ? 0 : this_pos)));
}

// All records of one read, in the order al_sam_read_records prints them.  sorted: the coordinate-sorted output keeps mapped records only
// (`samtools view -F4`): the unmapped record (flag 0x4) is skipped -- its name is still checked, as the host writer checks it before it drops
// the record.  Returns the number of records.
template <class S>
AL_SD int al_bam_read_records(S &o, const AlSamCfg &C, const AlSamRead &me, const AlSamRead *mate, int seg_idx, int n_seg, int rep_len, int sorted)
{
	int n = 0;
	if (me.n_regs > 0) {
		for (int k = 0; k < me.n_regs; ++k) {
			const AlReg *r = &me.regs[k];
			if (C.no_print_2nd && r->id != r->parent) continue;
			o.begin_record(); al_bam_record(o, C, me, mate, seg_idx, n_seg, k, rep_len); ++n;
		}
	} else if (!C.hit_only) {
		if (sorted) (void)al_bam_name_len(o, me, n_seg);
		else { o.begin_record(); al_bam_record(o, C, me, mate, seg_idx, n_seg, -1, rep_len); ++n; }
	}
	return n;
}

struct AlBamCountSink {               // pass 1: bytes only (and the reads whose name cannot be stored)
	const AlSamCfg *C; const char *text; uint64_t n = 0; uint32_t bad_name = 0;
	AL_SM char peek(uint32_t off) const { return text[off]; }
	AL_SM void name_too_long() { ++bad_name; }
	AL_SM void begin_record() {}
	AL_SM void end_record(uint64_t) {}
	AL_SM void u8(uint8_t) { ++n; }
	AL_SM void u16(uint16_t) { n += 2; }
	AL_SM void u32(uint32_t) { n += 4; }
	AL_SM void ch(char) { ++n; }
	AL_SM void num(long long v) { n += (uint64_t)al_num_len(v); }
	AL_SM void txt(uint32_t, uint32_t len) { n += len; }
	AL_SM void mem(const char *, int len) { n += (uint64_t)len; }
	AL_SM void cname(int rid) { n += C->name_off[rid + 1] - C->name_off[rid]; }
	AL_SM void seq4(uint32_t, int len, int) { if (len > 0) n += (uint64_t)(len + 1) / 2; }
	AL_SM void qual(uint32_t, int len, int) { if (len > 0) n += (uint64_t)len; }
	AL_SM void fill(uint8_t, int len) { if (len > 0) n += (uint64_t)len; }
	const uint64_t *tag_off = nullptr;
	AL_SM void tag(uint64_t k) { n += tag_off[k + 1] - tag_off[k]; }
};
