// al_dev_paf.h -- PAF record text (mm_write_paf3, format.c:304-330; write_tags :276-302) as one routine over a byte sink, the twin of
// al_dev_sam.h: compiled for the device (k_paf_len / k_paf_write, al_stream.hip) and, with AL_SAM_HOST, for the CPU (al_dbg_paf_selftest
// pins it against al_write_paf, which the golden PAF files pin against the reference).
//
// Same inputs as the SAM formatter: the device's own records in mapping orientation, mate 2 un-flipped on the fly (map.c:486-497).  A PAF
// line has no SEQ / QUAL and does not look at the mate, so the sink needs no seqfld().
#pragma once
#include "al_dev_sam.h"

// One line.  reg_idx < 0: the line of a read without hits (--paf-no-hit, format.c:307-311).  The name is printed whole (t->name: PAF keeps /1 /2).
template <class S>
AL_SD void al_paf_record(S &o, const AlSamCfg &C, const AlSamRead &me, int reg_idx, int rep_len)
{
	const AlReg *r = reg_idx >= 0 && reg_idx < me.n_regs ? &me.regs[reg_idx] : nullptr;
	o.txt(me.name, me.name_len); o.ch('\t'); o.num(me.qlen);
	if (!r) {
		o.lit("\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0");
		if (rep_len >= 0) { o.lit("\trl:i:"); o.num(rep_len); }
		o.ch('\n');
		return;
	}
	const AlSamView v = al_sam_view(*r, me.qlen, me.flip);
	o.ch('\t'); o.num(v.qs); o.ch('\t'); o.num(v.qe); o.ch('\t'); o.ch("+-"[v.rev]); o.ch('\t'); o.cname(r->rid);
	o.ch('\t'); o.num((long long)C.ctg_len[r->rid]); o.ch('\t'); o.num(r->rs); o.ch('\t'); o.num(r->re);
	o.ch('\t'); o.num(r->mlen); o.ch('\t'); o.num(r->blen); o.ch('\t'); o.num((int)(r->mapq & 0xff));
	const uint32_t n_cig = al_sam_ncig(*r);
	const uint32_t *cig = n_cig ? al_sam_cig(*r, me.arena) : nullptr;
	al_sam_write_tags(o, *r, cig, n_cig);
	if (rep_len >= 0) { o.lit("\trl:i:"); o.num(rep_len); }
	if (n_cig && C.out_cg) {
		o.lit("\tcg:Z:");
		for (uint32_t k = 0; k < n_cig; ++k) { o.num((int)(cig[k] >> 4)); o.ch("MIDNSHP=XB"[cig[k] & 0xf]); }
	}
	if (n_cig && C.tag_kind) { o.lit(C.tag_kind == 1 ? "\tMD:Z:" : "\tcs:Z:"); o.tag((uint64_t)(r - C.tag_reg0)); }   // format.c:327-328
	o.ch('\n');
}

// All lines of one read, in the order the reference prints them (map.c:617-633): every hit (secondaries unless NO_PRINT_2ND), or the
// no-hit line under PAF_NO_HIT.  Returns the number of lines.
template <class S>
AL_SD int al_paf_read_records(S &o, const AlSamCfg &C, const AlSamRead &me, int rep_len)
{
	int n = 0;
	if (me.n_regs > 0) {
		for (int k = 0; k < me.n_regs; ++k) {
			const AlReg *r = &me.regs[k];
			if (C.no_print_2nd && r->id != r->parent) continue;
			al_paf_record(o, C, me, k, rep_len); ++n;
		}
	} else if (C.paf_no_hit) { al_paf_record(o, C, me, -1, rep_len); ++n; }
	return n;
}
