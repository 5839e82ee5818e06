// airlift-align -- drop-in command line for the aligner invocations in AirLift's stage scripts.
//
// Accepted argv shapes:
//   B1/B2  airlift-align mem [-R RG] [-t N] REF.fa R_1.fastq [R_2.fastq]        (src/0-align_reads.sh:13, 0-align_singletons.sh:12)
//   B3     airlift-align aln [-n X] [-t N] REF.fa GAPS.fa > X.sai               (src/3-align_gaps/align_gaps.sh:14; writes a stub .sai)
//          airlift-align samse REF.fa X.sai GAPS.fa                              (align_gaps.sh:15; does the actual single-end mapping)
//          airlift-align index REF.fa                                             (accepted, no-op: the index is built on the GPU per run)
//   mm2    airlift-align -ax sr [-t N] [-R RG] [-K NUM] [--sam-hit-only] REF.fa R1 [R2]   (fork README usage; main.c:113-273)
//   8e     airlift-align ... --devices 0-7 [-o out.sam]      reads sharded over several GPUs of the node (index built once, copied
//                                                                   device to device; with a regular output file every lane pwrite()s its block)
//   N3     airlift-align ... --bam | --sorted-bam [-l LEVEL]       BAM on stdout; sorted = mapped records in coordinate order,
//                                                                   i.e. the result of `| samtools view -h -F4 | samtools sort -l5`
//   N2     airlift-align tokens --read-size R --skip S [-t N] REF.fa GAPS.fa      gaps_to_fasta.py GAPS.fa R tokens.fa S ; samse REF x tokens.fa
//          airlift-align tokens --read-size R --skip S [--regions-bed FILE] [--merged-bed FILE] REF.fa GAPS.fa   the merged regions of that SAM instead of it
//                                                                   (extract_regions.sh + run_pipeline.sh:62): BED per gap sequence / across all of them, merged on the GPU
//          airlift-align tokens --read-size R --skip S --gaps-bed GAPS.bed [--regions-bed FILE] [--merged-bed FILE] REF.fa   the gap sequences are the BED's rows of
//                                                                   REF.fa itself (extract_fasta_regions_with_bedfile.sh): no GAPS.fa, the tokens are cut from the index on the GPU
//          airlift-align tokens --read-size R --skip S --chain CHAIN --max-errors E [--gaps-out FILE] [--regions-bed F] [--merged-bed F] [--retired-bed F] [--constant-bed F] REF.fa
//                                                                   the gaps BED is made from the chain file on the GPU (2_get_updated_regions_bed.py, run_pipeline.sh:32), and the
//                                                                   retired / constant regions come from the same process (get_retired_regions.py :68, get_constant_regions.py :79)
//          airlift-align chain-beds --read-size R [--max-errors E] [--gaps-out FILE] [--constant-bed FILE] [--merged-in MERGED.bed --retired-bed FILE] [--host] [--device D] CHAIN
//                                                                   the three scripts alone, file for file
//          airlift-align chain-exact verify|build [--min-region 100] [--host] [--device D] [-o FILE] OLD.fa NEW.fa CHAIN
//                                                                   run/1_build_exact_chain_file.py: the exact chain file those scripts assume, verified or built on the GPU
//          airlift-align lift --chain CHAIN -o OUT.bam --unmapped-bed FILE [--sorted [--sort-mem BYTES]] [--write-index] [--host] [--gpu-deflate] [-l LEVEL] [-t N] [--device D] [--piece BYTES] IN.bam
//                                                                   run_pipeline.sh:92-95 (FastRemap): the constant-region reads moved across the chain file on the GPU
//          airlift-align merge -o OUT.bam [--write-index] [--host] [--gpu-deflate] [-l LEVEL] [-t N] [--device D] [--piece BYTES] IN1.bam IN2.bam [IN3.bam ...]
//                 run_pipeline.sh:116 and :119 (samtools merge): 2 to 8 coordinate-sorted BAMs merged into one on the GPU
//          airlift-align bam-index [--host] [-t N] [--device D] [--piece BYTES] IN.bam [OUT.bai]
//                 run_pipeline.sh:9, :95 and :119 (samtools index): the BAI of a coordinate-sorted BAM built on the GPU; merge and lift --sorted take --write-index
//                 (`index` stays the accepted no-op of `bwa index REF`)
//   PAF    airlift-align -x sr --paf [-c] [--cs] [--paf-no-hit] [--secondary=yes] REF.fa R1 [R2]   PAF instead of SAM; without -c / --cs no base-level alignment (the fork's -x sr without -a)
//   a8     airlift-align -ax sr --count-candidates REF.fa READS     the as-shipped fork's observable: seed-cluster count on stderr
// SAM goes to stdout; exit status 0 on success, non-zero on failure (so the caller's pipe fails).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <string>
#include <vector>
#include "../../include/airlift.h"
#include "al_env.h"

// numbers with k/m/g suffixes, as the fork's command line reads -K, -r, -g, -F (mm_parse_num, main.c:87-96)
static long long parse_num(const char *str, const char *opt)
{
	char *p; double x = strtod(str, &p);
	if (*p == 'G' || *p == 'g') x *= 1e9, ++p;
	else if (*p == 'M' || *p == 'm') x *= 1e6, ++p;
	else if (*p == 'K' || *p == 'k') x *= 1e3, ++p;
	if (*p) fprintf(stderr, "[WARNING] airlift-align: trailing characters in the value of %s: '%s'\n", opt, str);
	return (long long)(x + .499);
}

// output options of the fork's command line (main.c:158, 164, 207, 210-233) and --paf: 1 if `a` was one of them.  The fork writes PAF unless -a
// is given; here SAM stays the default (every existing invocation keeps its output) and --paf selects PAF, whatever else (-a, -ax) was said.
// As in the fork, PAF comes without base-level alignment unless -c or --cs asks for it (--MD alone does not, and then prints nothing).
struct OutSel { bool paf = false, aln = false; };
static int parse_out_opt(const char *a, al_mapopt_t &mo, OutSel &sel)
{
	if (!strcmp(a, "--MD")) mo.flag |= AL_F_OUT_MD;
	else if (!strcmp(a, "--eqx")) mo.flag |= AL_F_EQX;
	else if (!strcmp(a, "-Y")) mo.flag |= AL_F_SOFTCLIP;
	else if (!strcmp(a, "--paf")) sel.paf = true;
	else if (!strcmp(a, "-c")) { mo.flag |= AL_F_OUT_CG; sel.aln = true; }
	else if (!strcmp(a, "--paf-no-hit")) mo.flag |= AL_F_PAF_NO_HIT;
	else if (!strncmp(a, "--secondary=", 12)) {                        // main.c:213-222 (yes_or_no)
		if (!strcmp(a + 12, "yes") || !strcmp(a + 12, "y")) mo.flag &= ~(int64_t)AL_F_NO_PRINT_2ND;
		else if (!strcmp(a + 12, "no") || !strcmp(a + 12, "n")) mo.flag |= AL_F_NO_PRINT_2ND;
		else fprintf(stderr, "[WARNING]\033[1;31m option '--secondary' only accepts 'yes' or 'no'.\033[0m\n");
	}
	else if (!strcmp(a, "--cs") || !strncmp(a, "--cs=", 5)) {
		const char *v = a[4] == '=' ? a + 5 : nullptr;
		mo.flag |= AL_F_OUT_CS | AL_F_CIGAR; sel.aln = true;
		if (!v || !strcmp(v, "short")) mo.flag &= ~(int64_t)AL_F_OUT_CS_LONG;
		else if (!strcmp(v, "long")) mo.flag |= AL_F_OUT_CS_LONG;
		else if (!strcmp(v, "none")) mo.flag &= ~(int64_t)AL_F_OUT_CS;
		else fprintf(stderr, "[WARNING]\033[1;31m --cs only takes 'short' or 'long'. Invalid values are assumed to be 'short'.\033[0m\n");
	} else return 0;
	return 1;
}
// after the command line is read: --paf replaces SAM, and the alignment stays on only where -c / --cs asked for it
static void apply_out_sel(al_mapopt_t &mo, const OutSel &sel)
{
	if (!sel.paf) return;
	mo.flag = (mo.flag & ~(int64_t)(AL_F_OUT_SAM | AL_F_CIGAR)) | AL_F_OUT_PAF;
	if (sel.aln) mo.flag |= AL_F_CIGAR;
}

static int usage()
{
	fprintf(stderr, "Usage: airlift-align mem [-R RG] [-t N] ref.fa reads_1.fq [reads_2.fq]\n"
	                "       airlift-align aln [-n X] [-t N] ref.fa reads.fa > x.sai ; airlift-align samse ref.fa x.sai reads.fa\n"
	                "       airlift-align -ax sr [-t N] [-R RG] ref.fa reads_1.fq [reads_2.fq]\n"
	                "output options (every mode that writes alignments): --MD (MD:Z tag), --cs[=short|long|none] (cs:Z tag; --MD wins),\n"
	                "       --eqx (=/X CIGAR operations instead of M), -Y (soft clips and full SEQ/QUAL on supplementary records),\n"
	                "       --secondary=yes|no (secondary alignments; the sr preset leaves them out)\n"
	                "PAF:   --paf (PAF instead of SAM: chaining and MAPQ only, no base-level alignment, unless -c or --cs is given), -c (cg:Z CIGAR),\n"
	                "       --paf-no-hit (a line for reads without hits); not with mem / samse / aln / tokens, --bam, --sorted-bam, --count-candidates\n"
	                "BAM:   --bam | --sorted-bam [-l LEVEL] [--sort-mem BYTES]; --gpu-deflate (BGZF blocks deflated on the GPU: one compressor for every -l above 0,\n"
	                "       -l 0 stores; one device, one process: not with --devices of several lanes, --world, --rank, --ranked)\n"
	                "input: --gpu-inflate (BGZF-compressed FASTQ files -- bgzip, bcl-convert, DRAGEN -- stay with the GPU's input parser: their members are\n"
	                "       inflated on the GPU; decided per file; another gzip file, '-', or --world / --rank take the host reader as without the option)\n"
	                "tokens: airlift-align tokens --read-size R --skip S [--regions-bed FILE] [--merged-bed FILE] ref.fa gaps.fa  (without the two options: SAM of the tokens;\n"
	                "       with either: no SAM, the intervals of the mapped records sorted and merged on the GPU as sort-bed | mergeBed do -- --regions-bed within each gap\n"
	                "       sequence, the gaps in file order, --merged-bed across all; FILE '-' is stdout (for one of them); one device, one process, not with --paf, --bam,\n"
	                "       --sorted-bam, --count-candidates; --MD / --cs / --eqx / -Y change nothing there)\n"
	                "       airlift-align tokens --read-size R --skip S --gaps-bed FILE [--regions-bed FILE] [--merged-bed FILE] ref.fa  (no gaps.fa: a row 'name a b' of the\n"
	                "       gaps BED is the sequence `samtools faidx ref.fa name:a-b` prints, named name:a-b -- the bases [max(a,1)-1, min(b, contig length)) -- and its tokens\n"
	                "       are cut from the indexed reference on the GPU; SEQ of the SAM is therefore upper-case ACGTN where the FASTA run prints the file's own letters,\n"
	                "       every other column and both BED files are the same; the group of --regions-bed is the BED row; refused like the two options above)\n"
	                "       airlift-align tokens --read-size R --skip S --chain CHAIN --max-errors E [--gaps-out FILE] [--regions-bed FILE] [--merged-bed FILE] [--retired-bed FILE]\n"
	                "       [--constant-bed FILE] ref.fa  (no gaps BED either: the rows 2_get_updated_regions_bed.py CHAIN R E writes -- the gaps between the chain file's blocks padded\n"
	                "       by R + E, clamped to tSize and merged -- are computed on the GPU and tiled as --gaps-bed tiles them; --gaps-out writes them; --retired-bed: what\n"
	                "       get_retired_regions.py R MERGED CHAIN makes of the run's merged regions, taken where they lie on the GPU; --constant-bed: get_constant_regions.py's rows;\n"
	                "       --retired-bed / --constant-bed put the run in regions mode like --merged-bed: no SAM; refused like --gaps-bed, and beside it or a gaps.fa)\n"
	                "chain-beds: airlift-align chain-beds --read-size R [--max-errors E] [--gaps-out FILE] [--constant-bed FILE] [--merged-in MERGED.bed --retired-bed FILE] [--host]\n"
	                "       [--device D] chain  (the three scripts alone; at least one output, '-' is stdout for one of them; --gaps-out needs --max-errors, --retired-bed needs\n"
	                "       --merged-in; --host: the kernels' host twin, no device is opened; malformed input is refused as FILE:LINE: reason)\n"
	                "chain-exact: airlift-align chain-exact verify|build [--min-region 100] [--host] [--device D] [-o FILE] old.fa new.fa chain  (1_build_exact_chain_file.py: the two\n"
	                "       references compared over every block of the chain file on the GPU; verify prints the mismatch lines or PASS VERIFICATION, build the exact chain file)\n"
	                "lift:  airlift-align lift --chain CHAIN -o OUT.bam --unmapped-bed FILE [--sorted [--sort-mem BYTES]] [--write-index] [--host] [--gpu-deflate] [-l LEVEL=5] [-t N] [--device D] [--piece BYTES] in.bam\n"
	                "       (the reads in constant regions moved across the chain file on the GPU; the reads that do not lift leave as the rows extract-reads writes;\n"
	                "       --sorted: OUT.bam in coordinate order, what samtools sort makes of it)\n"
	                "merge: airlift-align merge -o OUT.bam [--write-index] [--host] [--gpu-deflate] [-l LEVEL=5] [-t N] [--device D] [--piece BYTES] in1.bam in2.bam [in3.bam ...]\n"
	                "       (2 to 8 coordinate-sorted BGZF BAMs merged into one on the GPU, what samtools merge does at the end of run_pipeline.sh; equal positions: the\n"
	                "       earlier input first; --write-index: OUT.bam.bai as bam-index writes it)\n"
	                "bam-index: airlift-align bam-index [--host] [-t N] [--device D] [--piece BYTES] in.bam [out.bai]\n"
	                "       (the BAI of a coordinate-sorted BGZF BAM built on the GPU, out.bai by default in.bam.bai; lift --sorted and merge take --write-index)\n"
	                "       airlift-align extract-sequence [--gpu-select[=host]] [--gpu-inflate] [--select-piece BYTES] [--device D] [-t N] reads_1.fq reads_2.fq rows.bed outdir\n"
	                "       airlift-align remap ... --gpu-select[=host] (the selected names are tested against both FASTQ files on the GPU; =host: by the kernels' host twin)\n");
	return 1;
}

int main(int argc, char **argv)
{
	al_idxopt_t io; al_mapopt_t mo;
	struct timespec tsm; clock_gettime(CLOCK_MONOTONIC, &tsm);
	std::vector<const char *> pos; const char *rg = nullptr; int n_threads = 3, device = -1; std::vector<int> devices; bool count_only = false; int bam_mode = 0, bam_level = 5; bool gpu_deflate = false;
	enum { MODE_MEM, MODE_ALN, MODE_SAMSE, MODE_MM2, MODE_TOKENS } mode = MODE_MM2; int tok_size = 0, tok_skip = 1;
	bool prefilter = false; int pf[4] = {3, 3, 5, 3};          // adjacency e, GreedySnake e, k-mer size, rounds
	const char *dump_fn = nullptr, *regions_fn = nullptr, *merged_fn = nullptr, *gaps_bed_fn = nullptr;
	const char *chain_fn = nullptr, *retired_fn = nullptr, *constant_fn = nullptr, *gaps_out_fn = nullptr; int max_errors = -1;
	OutSel sel;
	int i = 1; bool k_given = false; int rank = -1, world = 0; const char *rendezvous = nullptr, *out_path = nullptr;
	if (argc < 2) return usage();
	for (int j = 2; j < argc; ++j)                                      // (decided before any mode reads its arguments)
		if ((!strcmp(argv[j], "--regions-bed") || !strcmp(argv[j], "--merged-bed")) && strcmp(argv[1], "tokens") != 0) {
			fprintf(stderr, "[ERROR] %s writes the merged regions of a tokens run (airlift-align tokens --read-size R --skip S %s FILE ref.fa gaps.fa): it cannot be combined with another mode\n", argv[j], argv[j]);
			return 1;
		}
	for (int j = 2; j < argc; ++j)
		if (!strcmp(argv[j], "--gaps-bed") && strcmp(argv[1], "tokens") != 0) {
			fprintf(stderr, "[ERROR] --gaps-bed names the gap regions of a tokens run (airlift-align tokens --read-size R --skip S --gaps-bed GAPS.bed ref.fa): it cannot be combined with another mode\n");
			return 1;
		}
	for (int j = 2; j < argc; ++j)
		if (!strcmp(argv[j], "--chain") && strcmp(argv[1], "tokens") != 0 && strcmp(argv[1], "lift") != 0) {
			fprintf(stderr, "[ERROR] --chain names the chain file of a tokens run (airlift-align tokens --read-size R --skip S --chain CHAIN --max-errors E ref.fa; the scripts alone: airlift-align chain-beds): it cannot be combined with another mode\n");
			return 1;
		}
	if (!strcmp(argv[1], "lift")) {                // run_pipeline.sh:92-95 (FastRemap): the constant-region reads moved across the chain file, the rest to a BED
		int dev = -1, nt = 3, level = 5; unsigned lf = 0; size_t piece = 0; const char *c_fn = nullptr, *o_fn = nullptr, *b_fn = nullptr; std::vector<const char *> p;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "--chain") && j + 1 < argc) c_fn = argv[++j];
			else if (!strcmp(argv[j], "-o") && j + 1 < argc) o_fn = argv[++j];
			else if (!strcmp(argv[j], "--unmapped-bed") && j + 1 < argc) b_fn = argv[++j];
			else if (!strcmp(argv[j], "--host")) lf |= AL_LIFT_HOST;
			else if (!strcmp(argv[j], "--gpu-deflate")) lf |= AL_LIFT_GPU_DEFLATE;
			else if (!strcmp(argv[j], "--sorted")) lf |= AL_LIFT_SORTED;
			else if (!strcmp(argv[j], "--write-index")) lf |= AL_LIFT_WRITE_INDEX;
			else if (!strcmp(argv[j], "--sort-mem") && j + 1 < argc) setenv("AL_SORT_MEM", std::to_string(parse_num(argv[++j], "--sort-mem")).c_str(), 1);   // --sorted: bytes held before the held runs are merged into a file
			else if (!strcmp(argv[j], "-l") && j + 1 < argc) level = atoi(argv[++j]);
			else if (!strcmp(argv[j], "-t") && j + 1 < argc) nt = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--piece") && j + 1 < argc) piece = (size_t)strtoull(argv[++j], nullptr, 10);
			else p.push_back(argv[j]);
		}
		if (p.size() != 1 || !c_fn || !o_fn || !b_fn || level < 0 || level > 9) {
			fprintf(stderr, "Usage: airlift-align lift --chain CHAIN -o OUT.bam --unmapped-bed FILE [--sorted [--sort-mem BYTES]] [--write-index] [--host] [--gpu-deflate] [-l LEVEL=5] [-t N] [--device D] [--piece BYTES] in.bam\n"
			                "       (every record of in.bam, a BGZF file, through the chain file on the GPU: a mapped read that lies wholly and uniquely inside one block of a '+' chain\n"
			                "       gets its new contig, position and bin and stays in OUT.bam, in input order and unsorted; one that does not becomes a row of FILE -- chrom start end\n"
			                "       name[.1|.2] MAPQ CIGAR, what extract-reads writes -- and is re-aligned; unmapped reads are kept; --host: the kernels' host twin, no device is opened;\n"
			                "       --gpu-deflate: OUT.bam's blocks are deflated on the GPU; -t: host threads of the compressor; --piece: inflated bytes per piece;\n"
			                "       --sorted: OUT.bam holds the same records in coordinate order -- by new contig and position, records without a contig last, equal positions in\n"
			                "       input order -- and its header says SO:coordinate: each piece is put in order on the GPU, the pieces are merged on the host; --sort-mem BYTES:\n"
			                "       bytes held before the merged runs go to a temporary file in TMPDIR, default 16 GB, 0: never)\n");
			return 1;
		}
		if ((lf & AL_LIFT_HOST) && (lf & AL_LIFT_GPU_DEFLATE)) { fprintf(stderr, "[ERROR] lift: --host opens no device: it cannot be combined with --gpu-deflate\n"); return 1; }
		if ((lf & AL_LIFT_WRITE_INDEX) && !(lf & AL_LIFT_SORTED)) { fprintf(stderr, "[ERROR] lift: an index needs a BAM in coordinate order: --write-index goes with --sorted\n"); return 1; }
		const int rc2 = al_lift_bam(p[0], c_fn, o_fn, b_fn, lf, dev, nt, level, piece, nullptr) == 0 ? 0 : 1;
		fflush(stderr);
		_exit(rc2);
	}
	if (!strcmp(argv[1], "merge")) {               // run_pipeline.sh:116 and :119 (samtools merge -l5 -f OUT.bam A.bam B.bam): coordinate-sorted BAMs merged into one
		int dev = -1, nt = 3, level = 5; unsigned mf = 0; size_t piece = 0; const char *o_fn = nullptr; std::vector<const char *> p;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "-o") && j + 1 < argc) o_fn = argv[++j];
			else if (!strcmp(argv[j], "--host")) mf |= AL_MERGE_HOST;
			else if (!strcmp(argv[j], "--gpu-deflate")) mf |= AL_MERGE_GPU_DEFLATE;
			else if (!strcmp(argv[j], "--write-index")) mf |= AL_MERGE_WRITE_INDEX;
			else if (!strcmp(argv[j], "-l") && j + 1 < argc) level = atoi(argv[++j]);
			else if (!strcmp(argv[j], "-t") && j + 1 < argc) nt = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--piece") && j + 1 < argc) piece = (size_t)strtoull(argv[++j], nullptr, 10);
			else p.push_back(argv[j]);
		}
		if (p.empty() || !o_fn || level < 0 || level > 9) {
			fprintf(stderr, "Usage: airlift-align merge -o OUT.bam [--write-index] [--host] [--gpu-deflate] [-l LEVEL=5] [-t N] [--device D] [--piece BYTES] in1.bam in2.bam [in3.bam ...]\n"
			                "       (2 to 8 BGZF BAMs, each in coordinate order, merged into OUT.bam on the GPU: the records in order of contig and position, records without a\n"
			                "       contig last, equal positions with the earlier input first and in input order within one input; OUT.bam's reference list is in1.bam's with the\n"
			                "       contigs only later inputs name appended, and the later inputs' refIDs are translated; its header text is in1.bam's with SO:coordinate and the\n"
			                "       later inputs' other lines (a colliding @PG ID gets the suffix .K of input K; a colliding @RG ID is refused); an input that is not in order is\n"
			                "       refused, nothing is sorted here; --host: the kernels' host twin, no device is opened; --gpu-deflate: OUT.bam's blocks are deflated on the GPU;\n"
			                "       -t: host threads of the compressor; --piece: inflated bytes per refill of an input's window)\n");
			return 1;
		}
		if (p.size() < 2 || p.size() > 8) { fprintf(stderr, "[ERROR] merge takes 2 to 8 input BAMs, not %zu\n", p.size()); return 1; }
		for (const char *f : p) if (!strcmp(f, o_fn)) { fprintf(stderr, "[ERROR] merge: the input '%s' is also the output (-o)\n", f); return 1; }
		if ((mf & AL_MERGE_HOST) && (mf & AL_MERGE_GPU_DEFLATE)) { fprintf(stderr, "[ERROR] merge: --host opens no device: it cannot be combined with --gpu-deflate\n"); return 1; }
		const int rc2 = al_merge_bams(p.data(), (int)p.size(), o_fn, mf, dev, nt, level, piece, nullptr) == 0 ? 0 : 1;
		fflush(stderr);
		_exit(rc2);
	}
	if (!strcmp(argv[1], "bam-index")) {           // run_pipeline.sh:9, :95 and :119 (samtools index IN.bam): the BAI of a coordinate-sorted BAM
		int dev = -1, nt = 3; unsigned xf = 0; size_t piece = 0; std::vector<const char *> p;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "--host")) xf |= AL_BAI_HOST;
			else if (!strcmp(argv[j], "-t") && j + 1 < argc) nt = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--piece") && j + 1 < argc) piece = (size_t)strtoull(argv[++j], nullptr, 10);
			else p.push_back(argv[j]);
		}
		if (p.size() < 1 || p.size() > 2 || p[0][0] == '-') {
			fprintf(stderr, "Usage: airlift-align bam-index [--host] [-t N] [--device D] [--piece BYTES] in.bam [out.bai]\n"
			                "       (the index of in.bam, a BGZF BAM in coordinate order, built on the GPU and written to out.bai, by default in.bam.bai: the members are inflated and\n"
			                "       the records walked in pieces; a record's bin is reg2bin of its own interval, a run of records of one bin is one chunk, bins are not folded into\n"
			                "       their parents; the linear index, pseudo-bin 37450 and n_no_coor are written; contigs end at 2^29, CSI is not built; a BAM that is not in order\n"
			                "       is refused, nothing is sorted here; --host: the kernels' host twin, no device is opened; -t: host threads of the twin's inflater; --piece:\n"
			                "       inflated bytes per piece)\n");
			return 1;
		}
		const int rc2 = al_index_bam(p[0], p.size() > 1 ? p[1] : nullptr, xf, dev, nt, piece, nullptr) == 0 ? 0 : 1;
		fflush(stderr);
		_exit(rc2);
	}
	if (!strcmp(argv[1], "chain-beds")) {          // 2_get_updated_regions_bed.py + get_constant_regions.py + get_retired_regions.py
		int R = 0, E = -1, dev = -1; unsigned cf = 0; const char *g_fn = nullptr, *c_fn = nullptr, *r_fn = nullptr, *m_fn = nullptr; std::vector<const char *> p;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "--read-size") && j + 1 < argc) R = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--max-errors") && j + 1 < argc) E = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--gaps-out") && j + 1 < argc) g_fn = argv[++j];
			else if (!strcmp(argv[j], "--constant-bed") && j + 1 < argc) c_fn = argv[++j];
			else if (!strcmp(argv[j], "--retired-bed") && j + 1 < argc) r_fn = argv[++j];
			else if (!strcmp(argv[j], "--merged-in") && j + 1 < argc) m_fn = argv[++j];
			else if (!strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--host")) cf |= AL_CHAIN_HOST;
			else p.push_back(argv[j]);
		}
		const int n_stdout = (g_fn && !strcmp(g_fn, "-")) + (c_fn && !strcmp(c_fn, "-")) + (r_fn && !strcmp(r_fn, "-"));
		const char *why = p.size() != 1 || R <= 0 ? "" : (!g_fn && !c_fn && !r_fn) ? "at least one of --gaps-out, --constant-bed, --retired-bed is required" : (g_fn && E < 0) ? "--gaps-out needs --max-errors E (0 or more)"
		                : (r_fn && !m_fn) ? "--retired-bed needs --merged-in MERGED.bed" : n_stdout > 1 ? "at most one output may be '-' (stdout)" : nullptr;
		if (why && !*why) { fprintf(stderr, "Usage: airlift-align chain-beds --read-size R [--max-errors E] [--gaps-out FILE] [--constant-bed FILE] [--merged-in MERGED.bed --retired-bed FILE] [--host] [--device D] chain\n"); return 1; }
		if (why) { fprintf(stderr, "[ERROR] chain-beds: %s\n", why); return 1; }
		// the outputs are buffered and opened only once the rows exist: a refused input writes nothing
		FILE *tg = g_fn ? tmpfile() : nullptr, *tc = c_fn ? tmpfile() : nullptr, *tr = r_fn ? tmpfile() : nullptr;
		if ((g_fn && !tg) || (c_fn && !tc) || (r_fn && !tr)) { perror("[ERROR] chain-beds: tmpfile"); return 1; }
		int rc2 = al_chain_beds(p[0], R, E, m_fn, tg, tc, tr, cf, dev) == 0 ? 0 : 1;
		auto copy_out = [&](FILE *t, const char *fn) {
			if (!t || rc2) return;
			FILE *o = strcmp(fn, "-") ? fopen(fn, "wb") : stdout;
			if (!o) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", fn); rc2 = 1; return; }
			char buf[1 << 16]; size_t k; rewind(t);
			while ((k = fread(buf, 1, sizeof(buf), t)) > 0) if (fwrite(buf, 1, k, o) != k) { rc2 = 1; break; }
			if ((o == stdout ? fflush(o) : fclose(o)) == EOF) rc2 = 1;
		};
		copy_out(tg, g_fn); copy_out(tc, c_fn); copy_out(tr, r_fn);
		fflush(stderr);
		_exit(rc2);
	}
	if (!strcmp(argv[1], "chain-exact")) {         // run/1_build_exact_chain_file.py verify|build old.fa new.fa chain
		int M = 100, dev = -1; unsigned cf = 0; const char *o_fn = nullptr; std::vector<const char *> p;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "--min-region") && j + 1 < argc) M = atoi(argv[++j]);
			else if (!strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else if (!strcmp(argv[j], "-o") && j + 1 < argc) o_fn = argv[++j];
			else if (!strcmp(argv[j], "--host")) cf |= AL_CHAIN_HOST;
			else p.push_back(argv[j]);
		}
		const int mode = p.size() == 4 && !strcmp(p[0], "verify") ? AL_CEX_VERIFY : p.size() == 4 && !strcmp(p[0], "build") ? AL_CEX_BUILD : -1;
		if (mode < 0) { fprintf(stderr, "Usage: airlift-align chain-exact verify|build [--min-region 100] [--host] [--device D] [-o FILE] old.fa new.fa chain\n"); return 1; }
		if (M < 1) { fprintf(stderr, "[ERROR] chain-exact: --min-region must be positive\n"); return 1; }
		// the output is buffered and opened only once the text exists: a refused input writes nothing
		FILE *t = tmpfile();
		if (!t) { perror("[ERROR] chain-exact: tmpfile"); return 1; }
		int rc2 = al_chain_exact(p[1], p[2], p[3], mode, M, t, cf, dev) == 0 ? 0 : 1;
		if (!rc2) {
			FILE *o = o_fn && strcmp(o_fn, "-") ? fopen(o_fn, "wb") : stdout;
			if (!o) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", o_fn); rc2 = 1; }
			else {
				char buf[1 << 16]; size_t k; rewind(t);
				while ((k = fread(buf, 1, sizeof(buf), t)) > 0) if (fwrite(buf, 1, k, o) != k) { rc2 = 1; break; }
				if ((o == stdout ? fflush(o) : fclose(o)) == EOF) rc2 = 1;
			}
		}
		fflush(stderr);
		_exit(rc2);
	}
	al_set_opt(0, &io, &mo);
	al_set_opt("sr", &io, &mo);
	mo.flag |= AL_F_OUT_SAM | AL_F_CIGAR;
	if (!strcmp(argv[1], "extract-reads")) {       // N1: airlift-align extract-reads [--noprune] READS.bam REGIONS.bed READSIZE > rows   (extract_reads.sh BINDIR BAM BED READSIZE)
		int prune = 1, nt = 3, dev = -1; unsigned xf = 0; std::vector<const char *> p;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "--noprune")) prune = 0;
			else if (!strcmp(argv[j], "--gpu-inflate")) xf |= AL_EXTRACT_GPU_INFLATE;      // the BAM's BGZF members are inflated on the GPU (-t: host threads of the fallback)
			else if (xf && !strcmp(argv[j], "-t") && j + 1 < argc) nt = atoi(argv[++j]);
			else if (xf && !strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else p.push_back(argv[j]);
		}
		if (p.size() < 2 || (prune && p.size() < 3)) { fprintf(stderr, "Usage: airlift-align extract-reads [--noprune] [--gpu-inflate [-t N] [--device D]] reads.bam regions.bed [readsize]\n"); return 1; }
		const int64_t n = xf ? al_extract_reads_ex(p[0], p[1], p.size() > 2 ? atoi(p[2]) : 0, prune, stdout, xf, dev, nt) : al_extract_reads(p[0], p[1], p.size() > 2 ? atoi(p[2]) : 0, prune, stdout);
		return n < 0 || fflush(stdout) == EOF ? 1 : 0;
	}
	if (!strcmp(argv[1], "extract-sequence")) {    // N1: airlift-align extract-sequence FQ1 FQ2 ROWS OUTDIR   (extract_sequence.sh BINDIR FQ1 FQ2 BED THREAD OUTPUT)
		// options first: --gpu-select[=host] (the names tested on the GPU, or by the kernels' host twin), --gpu-inflate (BGZF FASTQ inflated there too), --select-piece BYTES, --device D, -t N
		unsigned xf = 0; int dev = -1, nt = 3, j = 2; size_t piece = 0;
		for (; j < argc; ++j) {
			if (!strcmp(argv[j], "--gpu-select")) xf |= AL_EXTRACT_GPU_SELECT;
			else if (!strcmp(argv[j], "--gpu-select=host")) xf |= AL_EXTRACT_GPU_SELECT | AL_EXTRACT_SELECT_HOST;
			else if (!strcmp(argv[j], "--gpu-inflate")) xf |= AL_EXTRACT_GPU_INFLATE;
			else if (!strcmp(argv[j], "--select-piece") && j + 1 < argc) piece = (size_t)strtoull(argv[++j], nullptr, 10);
			else if (!strcmp(argv[j], "--device") && j + 1 < argc) dev = atoi(argv[++j]);
			else if (!strcmp(argv[j], "-t") && j + 1 < argc) nt = atoi(argv[++j]);
			else break;
		}
		if (argc - j < 4) { fprintf(stderr, "Usage: airlift-align extract-sequence [--gpu-select[=host]] [--gpu-inflate] [--select-piece BYTES] [--device D] [-t N] reads_1.fq reads_2.fq rows.bed outdir\n"); return 1; }
		int64_t np = 0, ns = 0;
		const int rc = xf ? al_extract_sequence_ex(argv[j], argv[j + 1], argv[j + 2], argv[j + 3], &np, &ns, xf, dev, nt, piece) : al_extract_sequence(argv[j], argv[j + 1], argv[j + 2], argv[j + 3], &np, &ns);
		if (rc == 0) fprintf(stderr, "[airlift] extract-sequence: %lld pairs, %lld singletons\n", (long long)np, (long long)ns);
		return rc == 0 ? 0 : 1;
	}
	if (!strcmp(argv[1], "remap")) {
		// N1 fused with the re-alignment: airlift-align remap [-t N] [-R RG] [--noprune] [--readsize R] -o PAIRS.sam [--singletons SINGLE.sam] REF.fa READS.bam REGIONS.bed FQ1 FQ2
		// = extract_reads.sh + extract_sequence.sh + 0-align_reads.sh + 0-align_singletons.sh (run_pipeline.sh:58,103-113) without the rows file, the
		// three FASTQ files and the tool processes in between: the selected reads stay in memory files that the stream driver hands to the GPU.
		int prune = 1, read_size = 0, n_threads = 3; const char *rg = nullptr, *out_p = nullptr, *out_s = nullptr; std::vector<const char *> p; unsigned xf = 0;
		for (int j = 2; j < argc; ++j) {
			if (!strcmp(argv[j], "--noprune")) prune = 0;
			else if (!strcmp(argv[j], "--gpu-inflate")) xf |= AL_EXTRACT_GPU_INFLATE;      // READS.bam is inflated on the run's device; the reader's buffers are gone before the mapper sizes its own
			else if (!strcmp(argv[j], "--gpu-select")) xf |= AL_EXTRACT_GPU_SELECT;        // the names of both FASTQ files are tested on the run's device; the selector's buffers are gone before the index is built
			else if (!strcmp(argv[j], "--gpu-select=host")) xf |= AL_EXTRACT_GPU_SELECT | AL_EXTRACT_SELECT_HOST;
			else if (!strcmp(argv[j], "--readsize") && j + 1 < argc) read_size = atoi(argv[++j]);
			else if (!strcmp(argv[j], "-t") && j + 1 < argc) n_threads = atoi(argv[++j]);
			else if (!strcmp(argv[j], "-R") && j + 1 < argc) rg = argv[++j];
			else if (!strcmp(argv[j], "-o") && j + 1 < argc) out_p = argv[++j];
			else if (!strcmp(argv[j], "--singletons") && j + 1 < argc) out_s = argv[++j];
			else if (parse_out_opt(argv[j], mo, sel)) {}
			else p.push_back(argv[j]);
		}
		apply_out_sel(mo, sel);
		if (p.size() != 5 || !out_p || (prune && read_size <= 0)) { fprintf(stderr, "Usage: airlift-align remap [-t N] [-R RG] [--noprune | --readsize R] [--gpu-inflate] [--gpu-select[=host]] -o pairs.sam [--singletons single.sam] ref.fa reads.bam regions.bed reads_1.fq reads_2.fq\n"); return 1; }
		if (!al_env().pg_plain) al_set_program_line(AL_MM_VERSION, argc, argv);
		if (!k_given) setenv("AL_AUTO_BATCH", "1", 0);
		int fds[3]; int64_t np = 0, ns = 0;
		if (al_extract_to_memory_ex(p[1], p[2], read_size, prune, p[3], p[4], fds, &np, &ns, xf, -1, n_threads) != 0) return 1;
		fprintf(stderr, "[airlift] remap: %lld pairs, %lld singletons selected\n", (long long)np, (long long)ns);
		if (al_check_opt(&io, &mo) < 0) return 1;
		al_idx_t *mi = al_idx_build_device(p[0], &io, -1);
		if (!mi) return 1;
		int rc = 0;
		const std::string f1 = "/proc/self/fd/" + std::to_string(fds[0]), f2 = "/proc/self/fd/" + std::to_string(fds[1]), f3 = "/proc/self/fd/" + std::to_string(fds[2]);
		{ FILE *o = fopen(out_p, "wb"); const char *fn[2] = {f1.c_str(), f2.c_str()};
		  if (!o) { perror(out_p); rc = 1; } else { if (al_map_file_frag(mi, 2, fn, &mo, n_threads, o, rg, -1) != 0) rc = 1; if (fclose(o) == EOF) rc = 1; } }
		if (out_s && rc == 0) { FILE *o = fopen(out_s, "wb"); const char *fn[1] = {f3.c_str()};
		  if (!o) { perror(out_s); rc = 1; } else { if (al_map_file_frag(mi, 1, fn, &mo, n_threads, o, rg, -1) != 0) rc = 1; if (fclose(o) == EOF) rc = 1; } }
		for (int j = 0; j < 3; ++j) if (fds[j] >= 0) close(fds[j]);
		al_idx_destroy(mi);
		return rc;
	}
	// @PG as main.c:369 writes it (VN = the fork's MM_VERSION, main.c:16: the version whose records this path reproduces;
	// CL = this process's argv).  AL_PG_PLAIN=1 leaves the bare line (the tests' goldens come from a driver without argv).
	if (!al_env().pg_plain) al_set_program_line(AL_MM_VERSION, argc, argv);
	if (!strcmp(argv[1], "mem")) mode = MODE_MEM, i = 2;
	else if (!strcmp(argv[1], "aln")) mode = MODE_ALN, i = 2;
	else if (!strcmp(argv[1], "samse")) mode = MODE_SAMSE, i = 2;
	else if (!strcmp(argv[1], "tokens")) mode = MODE_TOKENS, i = 2;
	else if (!strcmp(argv[1], "index")) return 0;        // `bwa index REF`: nothing to precompute, the minimizer index is built on the GPU at start-up
	for (; i < argc; ++i) {
		const char *a = argv[i];
		if (a[0] != '-' || !strcmp(a, "-")) { pos.push_back(a); continue; }
		if (!strcmp(a, "-R") && i + 1 < argc) rg = argv[++i];
		else if (!strcmp(a, "-t") && i + 1 < argc) n_threads = atoi(argv[++i]);
		else if (!strcmp(a, "-x") && i + 1 < argc) { if (al_set_opt(argv[++i], &io, &mo) < 0) { fprintf(stderr, "[ERROR] unknown preset '%s'\n", argv[i]); return 1; } }
		else if (!strcmp(a, "-ax") && i + 1 < argc) { if (al_set_opt(argv[++i], &io, &mo) < 0) { fprintf(stderr, "[ERROR] unknown preset '%s'\n", argv[i]); return 1; } }
		else if (!strcmp(a, "-a")) mo.flag |= AL_F_OUT_SAM | AL_F_CIGAR;
		else if (!strcmp(a, "-d") && i + 1 < argc) dump_fn = argv[++i];                       // main.c:150: dump the index to FILE (mm_idx_dump's format)
		else if (!strcmp(a, "-k") && i + 1 < argc) io.k = atoi(argv[++i]);
		else if (!strcmp(a, "-w") && i + 1 < argc) io.w = atoi(argv[++i]);
		else if (!strcmp(a, "-K") && i + 1 < argc) { mo.mini_batch_size = (int)parse_num(argv[++i], "-K"); k_given = true; }
		else if (!strcmp(a, "-n") && i + 1 < argc) { if (mode == MODE_ALN) ++i; else mo.min_cnt = atoi(argv[++i]); }   // bwa aln -n X: accepted, no analogue; minimap2 -n: main.c:165
		// numeric options of the fork's command line (main.c:144-230), same letters and meaning
		else if (!strcmp(a, "-g") && i + 1 < argc) mo.max_gap = (int)parse_num(argv[++i], "-g");
		else if (!strcmp(a, "-F") && i + 1 < argc) mo.max_frag_len = (int)parse_num(argv[++i], "-F");
		else if (!strcmp(a, "-r") && i + 1 < argc) mo.bw = (int)parse_num(argv[++i], "-r");
		else if (!strcmp(a, "-N") && i + 1 < argc) mo.best_n = atoi(argv[++i]);
		else if (!strcmp(a, "-p") && i + 1 < argc) mo.pri_ratio = (float)atof(argv[++i]);
		else if (!strcmp(a, "-M") && i + 1 < argc) mo.mask_level = (float)atof(argv[++i]);
		else if (!strcmp(a, "-m") && i + 1 < argc) mo.min_chain_score = atoi(argv[++i]);
		else if (!strcmp(a, "-A") && i + 1 < argc) mo.a = atoi(argv[++i]);
		else if (!strcmp(a, "-B") && i + 1 < argc) mo.b = atoi(argv[++i]);
		else if (!strcmp(a, "-s") && i + 1 < argc) mo.min_dp_max = atoi(argv[++i]);
		else if (!strcmp(a, "-O") && i + 1 < argc) { char *e; mo.q = mo.q2 = (int)strtol(argv[++i], &e, 10); if (*e == ',') mo.q2 = (int)strtol(e + 1, &e, 10); }
		else if (!strcmp(a, "-E") && i + 1 < argc) { char *e; mo.e = mo.e2 = (int)strtol(argv[++i], &e, 10); if (*e == ',') mo.e2 = (int)strtol(e + 1, &e, 10); }
		else if (!strcmp(a, "-z") && i + 1 < argc) { char *e; mo.zdrop = mo.zdrop_inv = (int)strtol(argv[++i], &e, 10); if (*e == ',') mo.zdrop_inv = (int)strtol(e + 1, &e, 10); }
		else if (!strcmp(a, "--end-bonus") && i + 1 < argc) mo.end_bonus = atoi(argv[++i]);
		else if (!strcmp(a, "--max-chain-skip") && i + 1 < argc) mo.max_chain_skip = atoi(argv[++i]);
		else if (!strcmp(a, "--score-N") && i + 1 < argc) mo.sc_ambi = atoi(argv[++i]);
		else if (!strcmp(a, "--seed") && i + 1 < argc) mo.seed = atoi(argv[++i]);
		else if (!strcmp(a, "--sam-hit-only")) mo.flag |= AL_F_SAM_HIT_ONLY;
		else if (parse_out_opt(a, mo, sel)) {}
		else if (!strcmp(a, "--count-candidates")) count_only = true;
		else if (!strcmp(a, "--prefilter") && i + 1 < argc) {   // N4: --prefilter ADJ_E[,SNAKE_E[,SNAKE_K[,SNAKE_ITER]]] with --count-candidates
			prefilter = true; char *e; const char *v = argv[++i];
			pf[0] = (int)strtol(v, &e, 10); if (*e == ',') { pf[1] = (int)strtol(e + 1, &e, 10); if (*e == ',') { pf[2] = (int)strtol(e + 1, &e, 10); if (*e == ',') pf[3] = (int)strtol(e + 1, &e, 10); } } else pf[1] = pf[0];
		}
		else if (!strcmp(a, "--read-size") && i + 1 < argc) tok_size = atoi(argv[++i]);
		else if (!strcmp(a, "--skip") && i + 1 < argc) tok_skip = atoi(argv[++i]);
		else if (!strcmp(a, "--regions-bed") && i + 1 < argc) regions_fn = argv[++i];         // tokens: the merged regions per gap sequence instead of SAM
		else if (!strcmp(a, "--merged-bed") && i + 1 < argc) merged_fn = argv[++i];          // tokens: ... merged across all gap sequences
		else if (!strcmp(a, "--gaps-bed") && i + 1 < argc) gaps_bed_fn = argv[++i];            // tokens: the gap sequences are these regions of the reference itself
		else if (!strcmp(a, "--chain") && i + 1 < argc) chain_fn = argv[++i];                  // tokens: the gap regions are made from this chain file, on the GPU
		else if (!strcmp(a, "--max-errors") && i + 1 < argc) max_errors = atoi(argv[++i]);
		else if (!strcmp(a, "--gaps-out") && i + 1 < argc) gaps_out_fn = argv[++i];            // tokens --chain: the gaps rows, as 2_get_updated_regions_bed.py writes them
		else if (!strcmp(a, "--retired-bed") && i + 1 < argc) retired_fn = argv[++i];          // tokens --chain: the retired regions instead of SAM
		else if (!strcmp(a, "--constant-bed") && i + 1 < argc) constant_fn = argv[++i];        // tokens --chain: the constant regions instead of SAM
		else if (!strcmp(a, "--bam")) bam_mode = 1;
		else if (!strcmp(a, "--sorted-bam")) bam_mode = 2;
		else if (!strcmp(a, "-l") && i + 1 < argc) bam_level = atoi(argv[++i]);
		else if (!strcmp(a, "--gpu-deflate")) gpu_deflate = true;
		else if (!strcmp(a, "--gpu-inflate")) mo.flag |= AL_F_IN_GPU_INFLATE;              // BGZF-compressed FASTQ input stays with the stream driver, inflated on the GPU
		else if (!strcmp(a, "--sort-mem") && i + 1 < argc) setenv("AL_SORT_MEM", std::to_string(parse_num(argv[++i], "--sort-mem")).c_str(), 1);   // --sorted-bam: bytes held before a sorted run is spilled (samtools sort -m)
		else if (!strcmp(a, "--device") && i + 1 < argc) device = atoi(argv[++i]);
		else if (!strcmp(a, "--rank") && i + 1 < argc) rank = atoi(argv[++i]);             // one process per GPU: --rank r --world R -o OUT (al_map_file_frag_ranked)
		else if (!strcmp(a, "--world") && i + 1 < argc) world = atoi(argv[++i]);
		else if (!strcmp(a, "--ranked")) {                                                 // ... with rank and world from the launcher's environment (torchrun: RANK, WORLD_SIZE; the GPU is LOCAL_RANK)
			if (!al_env_rank() || !al_env_world_size()) { fprintf(stderr, "[ERROR] --ranked needs RANK and WORLD_SIZE in the environment\n"); return 1; }
			rank = *al_env_rank(); world = *al_env_world_size();
		}
		else if (!strcmp(a, "--rendezvous") && i + 1 < argc) rendezvous = argv[++i];
		else if (!strcmp(a, "--devices") && i + 1 < argc) {   // "0-7", "0,1,2", "0,0" (two lanes on one GPU): reads of every mini-batch sharded over the lanes
			const char *p = argv[++i];
			while (*p) {
				char *e; const long v0 = strtol(p, &e, 10); long v1 = v0;
				if (e == p) { fprintf(stderr, "[ERROR] --devices expects a list like 0-7 or 0,1,2\n"); return 1; }
				if (*e == '-') { p = e + 1; v1 = strtol(p, &e, 10); }
				for (long v = v0; v <= v1 && devices.size() < 64; ++v) devices.push_back((int)v);
				p = *e == ',' ? e + 1 : e;
				if (*e && *e != ',') { fprintf(stderr, "[ERROR] --devices expects a list like 0-7 or 0,1,2\n"); return 1; }
			}
		}
		else if (!strcmp(a, "-o") && i + 1 < argc) out_path = argv[++i];                   // opened below, once it is known whether this is one of several processes (which open the merged file themselves)
		else if (!strcmp(a, "--version")) { puts(al_version()); return 0; }
		else { fprintf(stderr, "[WARNING] airlift-align: option '%s' ignored\n", a); }
	}
	if (!chain_fn && (retired_fn || constant_fn || gaps_out_fn)) {
		fprintf(stderr, "[ERROR] %s writes rows made from the chain file of a tokens run: it needs --chain CHAIN (airlift-align tokens --read-size R --skip S --chain CHAIN --max-errors E ref.fa)\n", retired_fn ? "--retired-bed" : constant_fn ? "--constant-bed" : "--gaps-out");
		return 1;
	}
	if (chain_fn) {                                                     // (decided before the reference is read or a device opened)
		const bool ranked = world > 1 || rank >= 0;
		const char *outs[5] = {regions_fn, merged_fn, retired_fn, constant_fn, gaps_out_fn}; int n_stdout = 0;
		for (const char *o : outs) n_stdout += o && !strcmp(o, "-");
		const bool bed_mode = regions_fn || merged_fn || retired_fn || constant_fn;
		const char *why = sel.paf ? "--paf" : bam_mode == 2 ? "--sorted-bam" : bam_mode ? "--bam" : count_only ? "--count-candidates" : devices.size() > 1 ? "--devices of more than one lane" : ranked ? "--world / --rank / --ranked" : nullptr;
		if (why) { fprintf(stderr, "[ERROR] --chain makes the gap regions of a tokens run from the chain file on one device, in one process, for SAM or the merged regions: it cannot be combined with %s\n", why); return 1; }
		if (gaps_bed_fn) { fprintf(stderr, "[ERROR] --chain takes the place of --gaps-bed (the gaps BED is made from the chain file): give one of them, not both\n"); return 1; }
		if (pos.size() > 1) { fprintf(stderr, "[ERROR] --chain takes the place of the gap FASTA: give the reference alone (airlift-align tokens --read-size R --skip S --chain CHAIN --max-errors E ref.fa), not '%s' as well\n", pos[1]); return 1; }
		if (max_errors < 0) { fprintf(stderr, "[ERROR] --chain needs --max-errors E (0 or more): the gaps are padded by the read size plus E\n"); return 1; }
		if (n_stdout > (bed_mode ? 1 : 0)) { fprintf(stderr, "[ERROR] --chain: %s\n", bed_mode ? "at most one of the BED outputs may be '-' (stdout)" : "--gaps-out cannot be '-' beside the SAM on stdout"); return 1; }
	}
	if (gaps_bed_fn) {                                                  // (decided before the reference is read or a device opened)
		const bool ranked = world > 1 || rank >= 0;
		const char *why = sel.paf ? "--paf" : bam_mode == 2 ? "--sorted-bam" : bam_mode ? "--bam" : count_only ? "--count-candidates" : devices.size() > 1 ? "--devices of more than one lane" : ranked ? "--world / --rank / --ranked" : nullptr;
		if (why) { fprintf(stderr, "[ERROR] --gaps-bed cuts the tokens of a tokens run from the indexed reference on one device, in one process, for SAM or the merged regions: it cannot be combined with %s\n", why); return 1; }
		if (pos.size() > 1) { fprintf(stderr, "[ERROR] --gaps-bed takes the place of the gap FASTA: give the reference alone (airlift-align tokens --read-size R --skip S --gaps-bed GAPS.bed ref.fa), not '%s' as well\n", pos[1]); return 1; }
	}
	if (regions_fn || merged_fn) {                                      // (decided before any device is opened)
		const bool ranked = world > 1 || rank >= 0;
		const char *why = sel.paf ? "--paf" : bam_mode == 2 ? "--sorted-bam" : bam_mode ? "--bam" : count_only ? "--count-candidates" : devices.size() > 1 ? "--devices of more than one lane" : ranked ? "--world / --rank / --ranked" : nullptr;
		if (why) { fprintf(stderr, "[ERROR] --regions-bed / --merged-bed write the merged regions of a tokens run from one device, in one process: they cannot be combined with %s\n", why); return 1; }
		if (regions_fn && merged_fn && !strcmp(regions_fn, "-") && !strcmp(merged_fn, "-")) { fprintf(stderr, "[ERROR] --regions-bed and --merged-bed cannot both be written to stdout: at most one of them may be '-'\n"); return 1; }
	}
	if (sel.paf && (mode != MODE_MM2 || bam_mode || count_only)) {     // (decided before any device is opened)
		fprintf(stderr, "[ERROR] --paf writes PAF text from the -x sr mapping of reads: it cannot be combined with %s\n",
		        mode == MODE_MEM ? "mem" : mode == MODE_ALN ? "aln" : mode == MODE_SAMSE ? "samse" : mode == MODE_TOKENS ? "tokens" : bam_mode == 2 ? "--sorted-bam" : bam_mode ? "--bam" : "--count-candidates");
		return 1;
	}
	apply_out_sel(mo, sel);
	if (gpu_deflate) {                                                  // (decided before any device is opened)
		const bool ranked = world > 1 || rank >= 0;
		const char *why = !bam_mode ? "it needs --bam or --sorted-bam" : devices.size() > 1 ? "it cannot be combined with --devices of more than one lane" : ranked ? "it cannot be combined with --world / --rank / --ranked" : nullptr;
		if (why) { fprintf(stderr, "[ERROR] --gpu-deflate deflates the one BGZF stream of a BAM on one device, in one process: %s\n", why); return 1; }
		if (bam_level < 0 || bam_level > 9) bam_level = 5;
		fprintf(stderr, "[airlift] --gpu-deflate: BGZF blocks are %s\n", bam_level == 0 ? "stored (-l 0)" : "deflated on the device; there is one device compressor, whatever -l above 0 says");
		bam_level |= AL_BAM_DEFLATE_DEVICE;
	}
	// one process per GPU?  (--world, or --rank / --ranked with the launcher's WORLD_SIZE.)  Anything else -- also WORLD_SIZE = 1, or WORLD_SIZE set
	// without --rank / --ranked -- is a single process and writes -o FILE itself (main.c:183-190).
	if (world <= 0 && rank >= 0 && al_env_world_size()) world = *al_env_world_size();
	if (world <= 1 && out_path && strcmp(out_path, "-") != 0 && !freopen(out_path, "wb", stdout)) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", out_path); return 1; }
	// -K given: an upper bound of the bases per device batch.  Not given: the stream driver (plain FASTQ in, SAM out) sizes its batches
	// from the free device memory (al_stream_pipe.cpp); the host driver keeps the preset's 50 Mbases, as the reference.
	if (!k_given) setenv("AL_AUTO_BATCH", "1", 0);
	if (al_check_opt(&io, &mo) < 0) return 1;
	const char *ref = nullptr; std::vector<const char *> reads;
	if (mode == MODE_ALN) {          // the real work happens in samse; emit a small marker so `> x.sai` is non-empty
		if (pos.size() < 2) return usage();
		fputs("AIRLIFT-SAI-STUB\n", stdout);
		return 0;
	} else if (mode == MODE_SAMSE) {
		if (pos.size() < 3) return usage();
		ref = pos[0]; reads.push_back(pos[2]);
	} else if (gaps_bed_fn || chain_fn) {        // tokens --gaps-bed / --chain: the reference alone
		if (pos.size() != 1) return usage();
		ref = pos[0];
	} else {
		if ((pos.size() < 2 && !(dump_fn && pos.size() == 1)) || pos.size() > 3) return usage();   // (-d FILE ref.fa: index only, main.c:374-376)
		ref = pos[0]; for (size_t j = 1; j < pos.size(); ++j) reads.push_back(pos[j]);
	}
	struct timespec ts0, ts1; clock_gettime(CLOCK_MONOTONIC, &ts0);
	if (!devices.empty()) device = devices[0];
	// plain FASTQ files in, SAM out, one GPU: the run's device memory is obtained by a background thread while the reference is loaded and indexed
	const bool ref_is_idx = al_idx_is_idx(ref) > 0;                              // index.c:585-600: a prebuilt index (the fork's -d file, or this program's) instead of a FASTA
	if (devices.size() <= 1 && world <= 1 && !bam_mode && !count_only && mode != MODE_TOKENS && !al_env().host_index && !al_env().host_io && !ref_is_idx && !reads.empty()) {
		const int64_t rb = al_device_reserve_for_run(device, ref, (int)reads.size(), reads.data());
		if (rb > 0 && al_env().timing) fprintf(stderr, "[airlift] device memory reserve of %.1f GB started\n", rb / 1e9);
	}
	al_idx_t *mi = ref_is_idx ? al_idx_load(ref) : al_env().host_index ? al_idx_build(ref, &io, n_threads) : al_idx_build_device(ref, &io, device);
	if (mi && ref_is_idx && (al_idx_k(mi) != io.k || al_idx_w(mi) != io.w)) fprintf(stderr, "[WARNING]\033[1;31m Indexing parameters (-k, -w or -H) overridden by parameters used in the prebuilt index.\033[0m\n");   // main.c:378-380
	clock_gettime(CLOCK_MONOTONIC, &ts1);
	if (al_env().timing) fprintf(stderr, "[airlift] index build %.3f s\n", (ts1.tv_sec - ts0.tv_sec) + 1e-9 * (ts1.tv_nsec - ts0.tv_nsec));
	if (!mi) { fprintf(stderr, "[ERROR] failed to open file '%s'\n", ref); return 1; }
	if (dump_fn && !ref_is_idx && al_idx_dump(dump_fn, mi) != 0) { al_idx_destroy(mi); return 1; }
	if (reads.empty() && !gaps_bed_fn && !chain_fn) { al_idx_destroy(mi); fflush(stderr); _exit(0); }       // (index only)
	if (mode == MODE_TOKENS && chain_fn) {   // the gap regions from the chain file; SAM, or the BED outputs instead of it
		FILE *f[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; const char *fn[5] = {regions_fn, merged_fn, retired_fn, constant_fn, gaps_out_fn}; int rc2 = 0;
		for (int j = 0; j < 5 && rc2 == 0; ++j) if (fn[j]) { f[j] = strcmp(fn[j], "-") ? fopen(fn[j], "wb") : stdout; if (!f[j]) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", fn[j]); rc2 = 1; } }
		if (rc2 == 0) rc2 = (regions_fn || merged_fn || retired_fn || constant_fn) ? al_map_tokens_chain_regions(mi, chain_fn, max_errors, tok_size, tok_skip, &mo, n_threads, f[0], f[1], device, f[2], f[3], f[4])
		                                                                           : al_map_tokens_chain_file(mi, chain_fn, max_errors, tok_size, tok_skip, &mo, n_threads, stdout, rg, device, f[4]);
		al_idx_destroy(mi);
		for (FILE *o : f) if (o && (o == stdout ? fflush(o) : fclose(o)) == EOF) rc2 = 1;
		if (fflush(stdout) == EOF) rc2 = 1;
		fflush(stderr);
		_exit(rc2 == 0 ? 0 : 1);
	}
	if (mode == MODE_TOKENS && (regions_fn || merged_fn)) {   // ... and the regions of the tokens' alignments instead of their SAM
		FILE *fr = nullptr, *fm = nullptr; int rc2 = 0;
		auto open_out = [&](const char *fn, FILE *&f) { if (!fn) return; f = strcmp(fn, "-") ? fopen(fn, "wb") : stdout; if (!f) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", fn); rc2 = 1; } };
		open_out(regions_fn, fr); open_out(merged_fn, fm);
		if (rc2 == 0) rc2 = gaps_bed_fn ? al_map_tokens_bed_regions(mi, gaps_bed_fn, tok_size, tok_skip, &mo, n_threads, fr, fm, device)
		                                : al_map_tokens_regions(mi, reads[0], tok_size, tok_skip, &mo, n_threads, fr, fm, device);
		al_idx_destroy(mi);
		for (FILE *f : {fr, fm}) if (f && (f == stdout ? fflush(f) : fclose(f)) == EOF) rc2 = 1;
		fflush(stderr);
		_exit(rc2 == 0 ? 0 : 1);
	}
	if (mode == MODE_TOKENS) {   // gaps_to_fasta.py + single-end alignment of the tokens in one step (tokens are cut on the GPU)
		const int rc2 = gaps_bed_fn ? al_map_tokens_bed_file(mi, gaps_bed_fn, tok_size, tok_skip, &mo, n_threads, stdout, rg, device)
		                            : al_map_tokens_file(mi, reads[0], tok_size, tok_skip, &mo, n_threads, stdout, rg, device);
		al_idx_destroy(mi);
		if (fflush(stdout) == EOF) return 1;
		fflush(stderr);
		_exit(rc2 == 0 ? 0 : 1);
	}
	if (count_only) {   // what the as-shipped fork prints instead of alignments (main.c:384-391, 417)
		int64_t total = 0, o4[4] = {0, 0, 0, 0};
		const int rc2 = prefilter ? al_count_candidates_file_filtered(mi, reads[0], &mo, n_threads, device, pf[0], pf[1], pf[2] > 0 ? pf[2] : 5, pf[3], o4)
		                          : al_count_candidates_file(mi, reads[0], &mo, n_threads, device, &total);
		al_idx_destroy(mi);
		if (rc2 != 0) return 1;
		if (prefilter) total = o4[0];
		fprintf(stderr, "\nTotal No. of Mappings before alignment (verification): %d\n", (int)total);
		if (prefilter) fprintf(stderr, "Candidates kept by the adjacency filter (at most %d absent seeds): %lld\nCandidates kept by GreedySnake (e = %d, k-mer %d, %d rounds): %lld\nCandidates kept by both: %lld\n", pf[0], (long long)o4[1], pf[1], pf[2], pf[3], (long long)o4[2], (long long)o4[3]);
		fflush(stderr);
		_exit(0);
	}
	if (world > 1) {   // one process per GPU
		if (rank < 0 && al_env_rank()) rank = *al_env_rank();
		if (rank < 0 || rank >= world || !out_path || bam_mode == 2) { fprintf(stderr, "[ERROR] a multi-process run needs --rank r (or RANK) below --world, -o FILE after --world, and SAM or unsorted BAM output\n"); return 1; }
		const int rc2 = bam_mode ? al_map_file_frag_ranked_bam(mi, (int)reads.size(), reads.data(), &mo, n_threads, out_path, rg, device, rank, world, rendezvous, 0.0, bam_level)
		                         : al_map_file_frag_ranked(mi, (int)reads.size(), reads.data(), &mo, n_threads, out_path, rg, device, rank, world, rendezvous, 0.0);
		al_idx_destroy(mi);
		fflush(stderr);
		_exit(rc2 == 0 ? 0 : 1);
	}
	int rc = devices.size() > 1 ? al_map_file_frag_multi(mi, (int)reads.size(), reads.data(), &mo, n_threads, stdout, rg, devices.data(), (int)devices.size(), bam_mode, bam_level)
	       : bam_mode ? al_map_file_frag_bam(mi, (int)reads.size(), reads.data(), &mo, n_threads, stdout, rg, device, bam_mode == 2, bam_level)
	                  : al_map_file_frag(mi, (int)reads.size(), reads.data(), &mo, n_threads, stdout, rg, device);
	clock_gettime(CLOCK_MONOTONIC, &ts0);
	al_idx_destroy(mi);
	clock_gettime(CLOCK_MONOTONIC, &ts1);
	if (al_env().timing) fprintf(stderr, "[airlift] index release %.3f s\n", (ts1.tv_sec - ts0.tv_sec) + 1e-9 * (ts1.tv_nsec - ts0.tv_nsec));
	if (fflush(stdout) == EOF) { perror("[ERROR] failed to write the results"); return 1; }
	clock_gettime(CLOCK_MONOTONIC, &ts1);
	if (al_env().timing) { fprintf(stderr, "[airlift] main() %.3f s\n", (ts1.tv_sec - tsm.tv_sec) + 1e-9 * (ts1.tv_nsec - tsm.tv_nsec)); al_device_reserve_report(stderr); }
	// results are flushed and every device object is released: skip the HIP runtime's static teardown (0.3 s)
	fflush(stderr);
	if (al_env().no_fast_exit) return rc == 0 ? 0 : 1;          // (profilers flush their traces from exit handlers)
	_exit(rc == 0 ? 0 : 1);
}
