/*
 * locityper_hip.h — C ABI of liblocityper_hip.so
 *
 * MI355X (gfx950) implementation of ONE hot path of Locityper: read -> haplotype
 * likelihood scoring and genotype pre-filtering / assignment of `locityper genotype`.
 * Every entry point below names the reference interface it replaces
 * (paths relative to the reference crate root, tprodanov/locityper v1.7.2).
 *
 * Conventions
 *   - all functions return int32 status (LCTY_OK == 0); the message of the last
 *     failure on the calling thread is available from lcty_last_error();
 *     codes mirror the error categories of src/err.rs:11-30;
 *   - handles are opaque and owned by the library; input buffers are caller-owned
 *     host memory, only read during the call; output buffers are caller-allocated;
 *   - distinct handles may be used from distinct threads concurrently;
 *   - nothing in here falls back to the CPU: without a usable HIP device every
 *     compute entry point fails with LCTY_ERR_RUNTIME.
 */
#ifndef LOCITYPER_HIP_H
#define LOCITYPER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (src/err.rs:11-30) ---------------------------------- */
#define LCTY_OK                0
#define LCTY_ERR_INVALID_INPUT 1   /* Error::InvalidInput */
#define LCTY_ERR_INVALID_DATA  2   /* Error::InvalidData  */
#define LCTY_ERR_RUNTIME       3   /* Error::RuntimeError */
#define LCTY_ERR_SOLVER        4   /* Error::Solver       */
#define LCTY_ERR_UNSUPPORTED   5   /* shape outside what this build handles (fails loudly, never silently) */
/* Results the library allocates (the locus-file stages from "locus database build" down: an out struct with arrays, or out pointers
 * with their lengths): ON ANY NON-ZERO STATUS THE OUT STRUCT IS ALL ZERO, EVERY OUT POINTER IS NULL AND ITS LENGTH 0, AND NOTHING IS
 * LEAKED. The arrays appear in the caller's struct only when the call can no longer fail; the *_free of the struct (lcty_io_free for
 * a lone pointer) takes a zeroed one as well. */

/* ---- constants of the path -------------------------------------------- */
#define LCTY_GC_BINS        101    /* src/bg/depth.rs:42 */
#define LCTY_DEPTH_CACHE    256    /* src/model/distr_cache.rs:14 */
#define LCTY_MAX_ALT_CN     15     /* src/math/distr/bayes.rs:4,16 (alternatives.len() < 16) */
#define LCTY_MAX_USED_ALNS  10     /* src/model/locs.rs:743 */
#define LCTY_MAX_UNUSED_ALNS 2     /* src/model/locs.rs:740 */
#define LCTY_NONE_U32       0xFFFFFFFFu

/* sequencing technology (src/bg/mod.rs:182-268) */
#define LCTY_TECH_ILLUMINA 0
#define LCTY_TECH_HIFI     1
#define LCTY_TECH_PACBIO   2
#define LCTY_TECH_NANOPORE 3

/* edit-distance threshold kind (src/bg/err_prof.rs:365-399) */
#define LCTY_EDIT_FRACTION 0
#define LCTY_EDIT_PVALUE   1

/* read status after AllAlignments::load (src/model/locs.rs:1116-1150, 1255-1286) */
#define LCTY_READ_GOOD          0  /* goes to AllAlignments::reads */
#define LCTY_READ_POORLY_MAPPED 1
#define LCTY_READ_OUT_OF_BOUNDS 2
#define LCTY_READ_FEW_KMERS     3  /* goes to AllAlignments::unused_reads */

/* alignment record flags: BAM flag bits, plus MATE2 assigned by the loader
 * (src/model/locs.rs:1119-1131: first primary-led group = ReadEnd::First). */
#define LCTY_FLAG_UNMAPPED  0x0004u
#define LCTY_FLAG_REVERSE   0x0010u
#define LCTY_FLAG_MATE2     0x0080u
#define LCTY_FLAG_SECONDARY 0x0100u
#define LCTY_FLAG_SUPPL     0x0800u

/* raw BAM CIGAR op codes accepted on the path (src/seq/cigar.rs:116-129) */
#define LCTY_CIGAR_M 0u  /* rejected: the path requires --eqx (src/seq/aln.rs:311) */
#define LCTY_CIGAR_I 1u
#define LCTY_CIGAR_D 2u
#define LCTY_CIGAR_S 4u
#define LCTY_CIGAR_H 5u
#define LCTY_CIGAR_EQ 7u
#define LCTY_CIGAR_X 8u

/* ---- plain-data structs crossing the boundary -------------------------- */

/* model::Params (src/model/mod.rs:64-135) — the fields the path consumes. */
typedef struct lcty_params {
    uint32_t boundary_size;      /* 200 */
    int32_t  tweak;              /* -1 = auto (set_tweak_size, model/mod.rs:179-197) */
    double   lik_skew;           /* 0.85 */
    double   prob_diff;          /* NaN = auto: |unmapped_penalty| + ln 10 (command/genotype.rs:1294-1296) */
    double   unmapped_penalty;   /* NaN = auto by technology (model/mod.rs:55-60) */
    double   poor_compl;         /* 0.5 */
    double   poor_compl_edit;    /* 0.7 */
    double   compl_weight_bp;    /* 0.5; <= 0 disables the calculator (None) */
    double   compl_weight_pow;   /* 4 */
    double   kmers_weight_bp;    /* 0.2; <= 0 disables */
    double   kmers_weight_pow;   /* 4 */
    double   min_weight;         /* 0.001 */
    double   filt_diff;          /* ln 1e100 */
    double   prob_thresh;        /* ln 1e-4 */
    double   alt_cn[LCTY_MAX_ALT_CN]; /* 0.3,2,3,4,5 */
    uint32_t n_alt_cn;           /* 5 */
    uint16_t kmer_soft_thresh;   /* 5 */
    uint16_t kmer_hard_thresh;   /* 1 */
    uint8_t  complexity_k;       /* 5 */
    uint8_t  dont_skip;          /* 0 */
    uint8_t  strict_subset;      /* locs.rs:490: BAM header has fewer contigs than the contig set */
    uint8_t  _pad0;
    uint32_t threads;            /* reference `-@` (only enters truncate_ixs / discard thresholds) */
} lcty_params;

/* bg::BgDistr as loaded from distr.gz (src/bg/mod.rs:147-177) */
typedef struct lcty_bg {
    double   op_lnprobs[5];      /* matches, mismatches, insertions, deletions, clipping (bg/err_prof.rs:321-329) */
    double   edit_alpha;         /* BetaBinomial(alpha, beta) of the error profile */
    double   edit_beta;
    double   ins_n;              /* insert-size NBinom(n,p); ignored when !is_paired (bg/insertsz.rs:195-208) */
    double   ins_p;
    double   depth_n[LCTY_GC_BINS]; /* bg_depth NBinom per GC bin (bg/depth.rs:400-412) */
    double   depth_p[LCTY_GC_BINS];
    double   edit_p1;            /* EditThresh params: Fraction(.03,.06) / PValue(.99,.999) (bg/err_prof.rs:394-399) */
    double   edit_p2;
    uint32_t window;             /* bg_depth.window */
    uint32_t neighb;             /* bg_depth.neighb */
    int32_t  is_paired;          /* insert_distr defined */
    int32_t  technology;         /* LCTY_TECH_* */
    int32_t  edit_kind;          /* LCTY_EDIT_* */
    uint32_t _pad0;
} lcty_bg;

/* One BAM record of OUT/loci/<locus>/aln.bam reduced to what the path reads
 * (src/seq/aln.rs:147-157, src/seq/cigar.rs:203-208). 16 bytes. */
typedef struct lcty_aln_rec {
    uint32_t pos;        /* 0-based leftmost reference position (record.pos()) */
    uint16_t contig;     /* ContigId of the allele */
    uint16_t flags;      /* LCTY_FLAG_* */
    uint32_t n_cigar;    /* number of raw CIGAR words */
    uint32_t cigar_rel;  /* offset of the first CIGAR word relative to the pair's cigar_off */
} lcty_aln_rec;

/* Host view of a chunk of read pairs (or single reads) with all their records, in
 * the input-order contract of locs.rs:1116-1150: per pair
 *   mate-1 primary, mate-1 secondaries..., mate-2 primary, mate-2 secondaries...
 * Sequences are the primary record's SEQ (BAM orientation), 2-bit packed
 * (A=0,C=1,G=2,T=3; src/seq/kmers.rs:179-183) with a 1-bit/base "not ACGT" side
 * channel because kmers() emits UNDEF for such windows (kmers.rs:184-190). */
typedef struct lcty_reads_host {
    uint64_t n_pairs;
    const uint32_t*     mate_len;   /* [2*n_pairs]; 0 = mate absent (single-end data: every odd entry 0) */
    const uint64_t*     mate_off;   /* [2*n_pairs+1] base offsets, each a multiple of 32 */
    const uint32_t*     bases2;     /* 16 bases per word, base i of a mate at bit 2*(i%16) of word (off+i)/16 */
    const uint32_t*     nmask;      /* 32 bases per word, bit set = base is not A/C/G/T */
    const uint64_t*     aln_off;    /* [n_pairs+1] record offsets */
    const lcty_aln_rec* recs;
    const uint64_t*     cigar_off;  /* [n_pairs+1] CIGAR word offsets */
    const uint32_t*     cigar;      /* raw BAM CIGAR words: len<<4 | op */
} lcty_reads_host;

/* One alignment with its operations already counted — the 16-byte alignment-table entry of SURVEY.md section 8(d). It holds what
 * Alignment::count_region_operations_fast (src/seq/aln.rs:301-317) with limited_clipping (288-296) leaves of a record: the caller
 * (who walks raw_cigar() anyway and knows the contig length) counts, the device computes edit_distance (bg/err_prof.rs:73-79),
 * ErrorProfile::ln_prob (212-221) and everything behind. Counts are 16-bit: reads of up to 65 535 bases; longer reads, hard-clipped
 * primaries and the other checks of the record path (seq/aln.rs:311, model/locs.rs:526) stay with the caller, as does alignment
 * recovery (lcty_recover_alignments needs the CIGARs and refuses a counted batch). */
#define LCTY_CF_REVERSE     (1u << 28)
#define LCTY_CF_NOT_PRIMARY (1u << 29)   /* secondary or supplementary record */
#define LCTY_CF_UNMAPPED    (1u << 30)
typedef struct lcty_aln_counted {
    uint32_t pos_flags;   /* 0-based leftmost position (28 bits) | LCTY_CF_* */
    uint16_t contig;      /* ContigId of the allele */
    uint16_t matches, mismatches, insertions, deletions, clipping;   /* OperCounts (bg/err_prof.rs:25-45), clipping already limited */
} lcty_aln_counted;

/* PairAlignment (src/model/locs.rs:668-676); LCTY_NONE_U32 encodes Option::None. */
typedef struct lcty_pair_aln {
    double   ln_prob;    /* already multiplied by the read weight (locs.rs:861-863) */
    uint32_t ix1;        /* record index inside the pair, or NONE */
    uint32_t mid1;       /* Interval::middle of the mate-1 alignment, or NONE */
    uint32_t ix2;
    uint32_t mid2;
    uint16_t contig;
    uint16_t _pad[3];
} lcty_pair_aln;

/* Solver of one stage (src/solvers/stoch.rs): Greedy (36-145) or SimAnneal (151-266) with their parameters
 * (`-S greedy:x0=..,s=..,p=..` / `-S anneal:n=..,p=..,P=..`, SetParams 128-139, 249-260). */
#define LCTY_SOLVER_GREEDY 0
#define LCTY_SOLVER_ANNEAL 1
/* The exact solver in the place of the reference's ILP back ends (HiGHS: src/solvers/highs.rs:38-134, Gurobi: gurobi.rs:15-83;
 * registered at solve.rs:152-171, `-S highs` / `-S gurobi`): the same model — one binary per (non-trivial read, location), one-hot
 * depth variables per window, coupling rows, objective = ReadAssignment::likelihood — built on the device by the stage's
 * initialisation and solved by branch and bound ON THE HOST: the models of a stage's chains are copied to the host, solved by a pool
 * of host threads, one model per thread at a time (as the reference runs one model per worker, solve.rs:1052-1062;
 * lcty_ctx_set_knob "exact_threads", default: the machine's hardware threads, at most 64), and the assignments are written back
 * into the chains' device records. `node_limit` nodes without an answer -> LCTY_ERR_SOLVER, as a non-optimal solver status is
 * upstream (highs.rs:113-116). Every attempt starts from the best location of every read; with tweak = 0 the attempts of a genotype
 * share one model, which is solved once.
 * `init_prob` is this kind's relative gap g: the search stops when nothing left can beat the incumbent by more than g x |incumbent|.
 * Default 1e-4 = HiGHS' default mip_rel_gap, at which the reference's runs report "optimal" (highs.rs:103-110 changes no option);
 * 0 asks for a proof of optimality (reaches ~1 000 read pairs; larger loci end in LCTY_ERR_SOLVER). The bound is the relaxation of
 * that programme without cuts (~0.45 above the optimum HiGHS proves at its root node): at the default gap every genotype of a locus of
 * 10 000 read pairs x 8 alleles is answered within 3e-5 of HiGHS' optimum (tests/test_exact_highs.py), models of a few thousand read
 * pairs and fewer may end in LCTY_ERR_SOLVER. */
#define LCTY_SOLVER_EXACT 2
typedef struct lcty_solver {
    int32_t  kind;          /* LCTY_SOLVER_* */
    int32_t  best_start;    /* greedy: 1 = start from the best location of every read (default), 0 = random */
    uint32_t sample_size;   /* greedy: 10 */
    uint32_t plato_size;    /* greedy: 100; anneal: 10000 */
    uint32_t anneal_steps;  /* anneal: 20000 */
    uint32_t node_limit;    /* exact: branch-and-bound nodes per attempt before LCTY_ERR_SOLVER (default 20 000 000) */
    double   init_prob;     /* anneal: 0.5; exact: relative gap at which the search stops and the answer counts as optimal = HiGHS'
                             * mip_rel_gap, default 1e-4 as the reference's runs (highs.rs:103-110 leaves the option alone); 0 = a proof */
} lcty_solver;

typedef struct lcty_ctx   lcty_ctx;
typedef struct lcty_locus lcty_locus;
typedef struct lcty_reads lcty_reads;

/* ---- library / context -------------------------------------------------- */
const char* lcty_last_error(void);
const char* lcty_version(void);
/* number of HIP devices visible; 0 when there is none (never an error) */
int32_t lcty_device_count(void);
int32_t lcty_ctx_create(int32_t device_id, lcty_ctx** out);
void    lcty_ctx_destroy(lcty_ctx* ctx);
int32_t lcty_ctx_synchronize(lcty_ctx* ctx);
/* Limits of the retry / batching machinery of this context and choices between equivalent kernel forms, for tests that must reach
 * those paths with small inputs (no environment variable changes what the library computes):
 *   "transfer_levels", "transfer_scratch_mb", "transfer_waves", "transfer_cap_new", "transfer_arena"   lcty_recover_alignments: scratch
 *       levels, arenas;
 *   "depth_table_start"   first width of the extended depth table;   "solve_budget_mb"   device memory for the per-chain state of a
 *       solver stage;   "solve_extra_start"   first size of a chain's run of locations beyond the second;
 *   "solve_chains_per_wave"   1, 2, 4, 5, 6 chains of the greedy loop per wavefront;   "solve_lds_weights"   0: the greedy loop gathers
 *       the window weights, 1 (default where the locus has the weight tables): table indices + tables in LDS;
 *   "anneal_lds_weights"   0 gathered, 1 in LDS as they are, 2 (default where possible) table indices + tables in LDS;
 *   "contig_info_slide"   0 / 1: lcty_locus_create counts its neighbourhoods position by position / with sliding windows (default:
 *       sliding from 1 024 bases on);   "solve_stats"   1: per-stage iteration counts on stderr;   "queue_trace"   1: wall-clock marks of the phases of every locus of
 *       lcty_solve / lcty_solve_queue on stderr;   "gather_chunk_mb"   staging size of lcty_solve_stage_read_sharded;
 *   "prefilter_gram"   0: always the f64 tile kernel, 1: the integer Gram contraction on the matrix cores whenever it applies
 *       (default: from 512 alleles on);   "arena_cap_pct"   p: batches created afterwards (lcty_reads_create) get p % of the bound on their PairAlignment arena (two per
 *       record; one per (pair, allele) is the rule — an arena that is too small fails loudly);   "score_lean"   0: counted batches go through the general scoring kernel only (default 1: the lean kernel first, the general
 *       one on the pairs it leaves);   "score_lean_keep"   0: the lean kernel scores a saved record again in its last pass instead of
 *       keeping the first pass' products in LDS (what loci of more than 309 alleles get anyway);   "score_timing"   1: the lean kernel's
 *       timed build, shader-clock ticks per phase on stderr;   "comm_fail_at"   k: the k-th status agreement of a multi-GPU call fails on this rank (tests of
 *       the error path of the exchanges);   "prefilter_gram_cols"   room for that many level columns per read (default 6; too few: the
 *       f64 kernel takes the batch);   "queue_early_head"   0: lcty_solve_queue makes the head of a locus after the chains of the locus before (default 1:
 *       beside them);   "prefilter_gram_levels"   levels of a row the contraction takes (<= 16; rows with more go
 *       through the f64 kernel);   "db_chunk_cols"   columns of the bit matrix per pass of lcty_db_divergences (default: what fits 1/8 of
 *       the free device memory, 256 MB at most);   "basis_batch_words"   CIGAR words per batch of lcty_basis_windows (default: what fits a
 *       quarter of the free device memory; an entry with more words travels alone);   "align_batch_pairs"   pairs per batch of
 *       lcty_align_haplotypes (default: sized from the free device memory);   "align_match_budget"   bytes for the k-mer matches of such
 *       a batch, 20 a match (default: a quarter of the free device memory, at least 64 MB; a batch with more is cut to its longest
 *       prefix of pairs that fits, a single pair always runs);   "align_hash_bits"   bits kept of a backbone window's hash
 *       (default 64; fewer: collisions, which the comparison of the bases must reject);   "align_dp_cells"   cells of the largest
 *       stretch the exact aligner takes (default 2^26; a larger stretch is dropped to align_simple and counted in n_dropped — this one
 *       changes CIGARs, as the limit itself does);   "align_cigar_store_mb"   megabytes of device memory for the finished CIGARs of
 *       lcty_align_haplotypes_transitive (default: an eighth of the free device memory, at least 64; a call whose CIGARs outgrow it is
 *       LCTY_ERR_UNSUPPORTED naming this knob — it never takes another route);   "pafvcf_hash_bits"   bits kept of the hash of an
 *       allele's bytes in lcty_pafvcf_table (default 64; fewer: collisions, which the comparison of the bytes must reject);
 *       "pafvcf_table_mb"   megabytes the resident allele table (n_ranges x n_seqs x 4 bytes) of lcty_pafvcf_table / lcty_paf_to_vcf may
 *       take (default: a quarter of the free device memory; a larger table is LCTY_ERR_UNSUPPORTED naming this knob);
 *       "genome_max_bases"   positions (bases + one separator per contig) a resident genome may reach (default 2^32; lcty_genome_append
 *       refuses a piece that reaches it with LCTY_ERR_UNSUPPORTED before it uploads anything);
 *       "sample_bam_hash_bits"   bits kept of the hash of a read name in lcty_sample_bam_fetch (default 64; fewer: collisions, which the
 *       comparison of the names must resolve);   "sample_bam_max_slice_bytes"   inflated bytes one lcty_sample_bam_fetch may take
 *       (default 2^33; a larger slice is LCTY_ERR_UNSUPPORTED naming this knob, before anything is uploaded);
 *       "sample_bam_inflate"   0 (default): lcty_sample_bam_fetch inflates its BGZF blocks with zlib on the host, 1: on the device
 *       (lcty_bgzf_inflate's kernel, straight into the buffer the record kernel reads; any other value is LCTY_ERR_INVALID_INPUT).
 *       "bgzf_deflate"   0 (default): lcty_write_bam deflates its BGZF blocks with zlib on the host as the records come, 1: it keeps the
 *       stream and deflates it on the device when the file is closed (lcty_bgzf_deflate; the inflated bytes of the BAM and what its
 *       index points at are the same, the deflate bytes differ); any other value, a negative one included, is refused by this call with
 *       LCTY_ERR_INVALID_INPUT naming the knob;   "bgzf_deflate_max_bytes"   input bytes one slice of lcty_bgzf_deflate takes to the
 *       device (default 256 MB; the output does not depend on it; below 0xff00, one block, lcty_bgzf_deflate is LCTY_ERR_INVALID_INPUT).
 *       "aln_bam_max_slice_bytes"   inflated bytes lcty_bam_read_device may take (default 2^33; a larger file is LCTY_ERR_UNSUPPORTED
 *       naming this knob, before anything is allocated); its inflate follows "sample_bam_inflate".
 *       "vcf_max_slice_bytes"   inflated bytes one lcty_vcf_indexed_fetch may take (default 2^33; a larger window is LCTY_ERR_UNSUPPORTED
 *       naming this knob, before the slice is allocated or uploaded); its inflate follows "sample_bam_inflate".
 *       "fastx_window_bytes"   bytes of text lcty_fastx_device_open's reader takes per file and window (default 2^28, at least 64: less is
 *       LCTY_ERR_INVALID_INPUT; the records do not depend on it); a window without a complete record is doubled, up to
 *       "fastx_window_limit"   (default and most 2^31 - 64: offsets inside a window are 32-bit; a record beyond it is LCTY_ERR_UNSUPPORTED).
 *       "recruit_blocks"   the most workgroups either launch of lcty_recruit starts (default: 16 per CU for read pairs and single reads
 *       of up to 256 bases, 8 per CU for longer single reads; 0 counts as 1): with few workgroups each one takes many chunks of 64 pairs,
 *       or many long reads, in turn; the loci of a read do not depend on it.
 *       "recruited_init_units"   32-base units the device arrays of a locus of an lcty_recruited set hold when they are first made
 *       (default 4 096: 128 kb of bases, 48 KB; room for an eighth as many pairs beside them; 0 counts as 1); they double until an add fits,
 *       device to device; the contents do not depend on it.   "recruited_max_bytes"   bytes the contents of an lcty_recruited set may
 *       reach over all loci, 12 per unit and 32 per pair (default 2^36; an add beyond it is LCTY_ERR_UNSUPPORTED naming this knob,
 *       before anything is copied; the capacity behind the contents is at most twice as large).
 *       "bam_stream_window_bytes"   inflated bytes, the carried tail included, at which a window of lcty_bam_stream_next stops taking
 *       BGZF blocks (default 2^28, at least 1: 0 is LCTY_ERR_INVALID_INPUT at lcty_bam_stream_open; the reads do not depend on it); a
 *       window that completes no record is doubled, up to   "bam_stream_window_limit"   (default 2^33; a record beyond it is
 *       LCTY_ERR_UNSUPPORTED naming this knob).
 * value < 0 restores the default; an unknown name is LCTY_ERR_INVALID_INPUT. None of them changes a result beyond the last bits of
 * an f64 sum (the order in which a chain's likelihood or a genotype's score is added up). */
int32_t lcty_ctx_set_knob(lcty_ctx* ctx, const char* name, int64_t value);
/* Files a developer asks the library to write (no environment variable is read anywhere in the library): name "exact_dump" = the
 * model of the first chain of an exact-solver stage as text, written when that stage runs; path NULL or "" switches it off.
 * No counterpart upstream (HiGHS' own `write_model` is not called by highs.rs). */
int32_t lcty_ctx_set_path(lcty_ctx* ctx, const char* name, const char* path);
/* The solver stages keep their per-chain device state (32 B per chain and good read pair: ~150 GB for the 5 000 greedy chains of
 * the default scheme at 1 M read pairs; batches of chains when the device has less) with the context between stages and loci;
 * this releases it (the next stage allocates again). So does alignment recovery with its lane scratch and the arenas of the
 * transferred alignments (up to half of what is free on the device when lcty_recover_alignments first runs; long reads need tens of MB
 * per wavefront): kept between calls, handed back when a solver stage sizes its workspace, and by this call. */
int32_t lcty_ctx_trim(lcty_ctx* ctx);
/* Page-locked host memory for the chunks handed to lcty_reads_append / lcty_reads_append_counted / lcty_recruit_*: the copies of
 * a chunk that lies in such memory go over PCIe at link rate (a pageable chunk is staged through the driver's bounce buffers at
 * about half of it). The reference reads its records into ordinary Vecs (locs.rs:1116-1150); a binding would fill these
 * buffers instead. Release with lcty_host_free. */
int32_t lcty_host_alloc(lcty_ctx* ctx, uint64_t bytes, void** out);
void    lcty_host_free(void* p);

/* defaults of model::Params::default (model/mod.rs:108-135) */
void    lcty_params_default(lcty_params* out);
/* Resolves the "auto" fields exactly as command/genotype.rs:1282-1296 does:
 * tweak (model/mod.rs:179-197), unmapped_penalty (55-60), prob_diff. */
int32_t lcty_params_resolve(lcty_params* params, const lcty_bg* bg);

/* ---- locus: ContigSet + KmerCounts + ContigInfos + UniqueKmers + LUTs ----
 * Replaces ContigSet::load_with_kmer_counts (src/seq/contigs.rs:295),
 * ContigInfos::new (src/model/windows.rs:584-615), UniqueKmers::new
 * (src/model/locs.rs:930-963), InsertDistr::load (src/bg/insertsz.rs:195-208),
 * EditDistCache::new (src/bg/err_prof.rs:422-428), DistrCache::new
 * (src/model/distr_cache.rs:61-75).
 *   seqs       ASCII allele sequences, concatenated; seq_off[n_alleles+1]
 *   offtarget  off-target k-mer counts (first KmerCounts block), cnt_off[n_alleles+1],
 *              cnt_off[a+1]-cnt_off[a] == len(a)+1-k
 *   k          2 <= k <= 63 as in the reference (u128 k-mers, src/seq/kmers.rs:8-26; locs.rs:919). k <= 31 (the default of
 *              `locityper add` is 25): 64-bit keys, the set built on the device, the reads' k-mers taken from registers;
 *              32 <= k <= 63: 128-bit keys in a table of {lo, hi} pairs built on the host, the reads' k-mers from memory          */
int32_t lcty_locus_create(lcty_ctx* ctx, uint32_t n_alleles,
                          const uint8_t* seqs, const uint64_t* seq_off,
                          const uint16_t* offtarget, const uint64_t* cnt_off, uint32_t k,
                          const lcty_bg* bg, const lcty_params* params, lcty_locus** out);
void    lcty_locus_destroy(lcty_locus* locus);
/* KmerCounts::load (src/seq/counts.rs:127-150) on the decompressed bytes of `kmers.bin.br` / `.lz4` (command/paths.rs:4-5): parses
 * the FIRST block, which holds the off-target counts (command/add.rs:647-650; contigs.rs:301-303), into the arrays
 * lcty_locus_create takes. Values are clamped to min(65535, 2^(8 * counter bytes) - 1). Two calls: with cnt_off = counts = NULL it
 * only reports k, the number of contigs and (in *consumed) the bytes of the block; the total number of values is then
 * cnt_off[n_contigs] of the second call, for which cap_counts may be the remaining length of the buffer (a value takes at least
 * one byte). Truncated data / overlong varints / a counter length > 8: LCTY_ERR_INVALID_DATA. Host code. */
int32_t lcty_kmer_counts_parse(const uint8_t* buf, uint64_t len, uint32_t* k, uint32_t* n_contigs, uint64_t* cnt_off /* [n_contigs+1] */,
                               uint64_t cap_contigs, uint16_t* counts, uint64_t cap_counts, uint64_t* consumed);
/* number of locus-unique canonical k-mers (the count logged at locs.rs:953) */
int32_t lcty_locus_n_unique_kmers(const lcty_locus* locus, uint64_t* out);
/* ContigInfo::new products per allele (windows.rs:386-407): position count = len-neighb+1.
 * Any output pointer may be NULL. uniq counts / complexity counts are the integer
 * numerators, the f64 values of the reference are count*mult with
 *   uniq_kmer_frac = uniq * (1/(neighb+1-k)),  complexity = distinct * (1/min(neighb+1-ck, 4^ck)). */
int32_t lcty_locus_contig_info(const lcty_locus* locus, uint32_t allele,
                               uint8_t* gc, uint32_t* uniq_cnt, uint16_t* compl_cnt,
                               uint32_t* n_windows, uint32_t* reg_start);
/* EditDistCache::get (bg/err_prof.rs:434-448) */
int32_t lcty_locus_edit_thresholds(const lcty_locus* locus, uint32_t read_len, uint32_t* good, uint32_t* passable);
/* InsertDistr::ln_prob / insert_penalty (bg/insertsz.rs:153-175) */
int32_t lcty_locus_insert_lnprob(const lcty_locus* locus, uint32_t n, const uint32_t* sizes, double* out, double* insert_penalty);
/* DistrCache: ln P(depth) for gc bin, depth in 0..LCTY_DEPTH_CACHE (distr_cache.rs:61-75; bayes.rs:27-35) */
int32_t lcty_locus_depth_lut(const lcty_locus* locus, double* out /* [101*256] */);
/* ContigInfo::neighb_info weight (windows.rs:439-445) of every moving-window position, alleles concatenated
 * (sum over alleles of len - neighb + 1 values) */
int32_t lcty_locus_window_weights(const lcty_locus* locus, double* out);
/* The depth table of the solver stages: DistrCache (src/model/distr_cache.rs:61-92) past the 256 entries of the reference's
 * LinearCache, the same BayesCalc::ln_pmf (src/math/distr/bayes.rs:27-35) evaluated on the device. *width_io is rounded up to a
 * power of two >= 256; out (may be NULL to ask for the width) receives [101][width]. */
int32_t lcty_locus_depth_table(lcty_locus* locus, uint32_t* width_io, double* out);

/* Explicit region weights (`locityper genotype --reg-weights`): replaces load_explicit_weights (src/model/windows.rs:257-317)
 * minus the text parsing — the lines of the BED file in file order as (allele index, start, end, value); an index >= n_alleles
 * stands for a contig name the locus does not have (the line is skipped, 269-272). Errors as upstream: value outside [0, 1],
 * an allele not covered from its first base on without gaps, missing, or covered to a different length -> LCTY_ERR_INVALID_DATA
 * (Error::ParsingError); an interval beyond the end of its allele -> LCTY_ERR_INVALID_INPUT (seq/interv.rs:112-116).
 * Effects, both on the device: every window weight gets the window's average as its last factor (ExplicitWeights::average,
 * 236-238; ContigInfo::new 409-413; neighb_info 441-443), and lcty_score_reads multiplies a read pair's weight by
 * ContigInfos::explicit_read_weight over its PairAlignments (683-693, read_end_weight 493-503; locs.rs:860, 903).
 * A NaN value is rejected as out of range (upstream's `val < 0.0 || val > 1.0` lets it through and every weight turns NaN).
 * Call it after lcty_locus_create and before the reads of the locus are scored; a second call replaces the first.
 * (ContigInfos::weighted_aln_prob / average_read_weight, windows.rs:506-643, have no caller upstream and are not built.) */
int32_t lcty_locus_set_explicit_weights(lcty_locus* locus, uint32_t n_lines, const uint32_t* allele, const uint32_t* start,
                                        const uint32_t* end, const double* value);

/* ---- reads: device-resident batch -----------------------------------------
 * Capacity is fixed at creation so a batch larger than host memory can be
 * appended chunk by chunk (each append is one set of H2D copies).             */
int32_t lcty_reads_create(lcty_locus* locus, uint64_t cap_pairs, uint64_t cap_bases,
                          uint64_t cap_recs, uint64_t cap_cigar, lcty_reads** out);
/* A batch larger than HBM (1 M ONT reads x 256 alleles carry 600 GB of CIGAR words): the records, CIGAR words and bases of ONE
 * chunk are on the device at a time, the products of every scored chunk stay (status, weights, k-mer counts, matrix rows,
 * PairAlignments: about 9 KB per read at 256 alleles). Use:  create_streaming; { lcty_reads_append (one or more chunks that fit
 * the chunk capacities); lcty_score_reads } ...; then prefilter / solver stages / read-backs as for any batch — they see all
 * pairs appended so far, in order, and the results are those of one resident batch (AllAlignments::load is a loop over reads,
 * locs.rs:1119-1185). An append after a score drops the records of the scored chunk. cap_pair_alns = room for that many
 * PairAlignments in total (0: three per (pair, allele)); overflow fails loudly. With alignment recovery the loop body is
 * { append; lcty_score_reads; lcty_recover_alignments; lcty_score_reads }: recovery works on the chunk whose records are resident. */
int32_t lcty_reads_create_streaming(lcty_locus* locus, uint64_t cap_pairs, uint64_t chunk_pairs, uint64_t chunk_bases,
                                    uint64_t chunk_recs, uint64_t chunk_cigar, uint64_t cap_pair_alns, lcty_reads** out);
int32_t lcty_reads_append(lcty_reads* reads, const lcty_reads_host* chunk);
/* The same chunk with its records counted by the caller: alns[aln_off[n_pairs]] in the record order of the chunk; chunk->recs,
 * cigar_off and cigar are not read. A batch holds records or counted alignments, never both. lcty_score_reads, the prefilter and
 * the solver stages see no difference; results equal the record path's bit for bit (tests/test_gpu_counted.py). */
int32_t lcty_reads_append_counted(lcty_reads* reads, const lcty_reads_host* chunk, const lcty_aln_counted* alns);
/* An empty batch again, bound to `locus` (same context, not more alleles than the locus it was created for): every buffer stays.
 * For queues of loci that rotate over a few batch objects — allocating or releasing tens of GB per locus would wait for every
 * stream of the device. Nothing of the batch may be in use (see lcty_solve_queue_fed's release). */
int32_t lcty_reads_reset(lcty_reads* reads, lcty_locus* locus);
void    lcty_reads_destroy(lcty_reads* reads);
int32_t lcty_reads_n_pairs(const lcty_reads* reads, uint64_t* out);

/* AllAlignments::load without alignment recovery (src/model/locs.rs:1085-1185,
 * 1237-1288 with opt_hap_alns == None): K2 unique k-mers + read weight (968-1002),
 * K4 op counts + ErrorProfile::ln_prob (aln.rs:301-317, err_prof.rs:212-221),
 * K5 thresholds / 128-bp dedupe (502-567, 298-344), K7 pairing (746-868 / 873-911)
 * and K8 the dense row of best_aln_matrix (1203-1212) — one fused launch.
 * Asynchronous on the context's stream.                                         */
int32_t lcty_score_reads(lcty_reads* reads);

/* Which scoring kernel took which pair in the last lcty_score_reads launch of the batch. A counted batch goes
 * through the lean kernel (every (contig, read end) group holds at most one saved alignment), what it leaves through its two-slot
 * form (a second saved alignment in a group, at most 64 such groups in a pair) and what that leaves through the general kernel;
 * every other batch through the general kernel alone. n_lean + n_two + n_general == n_pairs, the pairs of that launch (of a
 * streaming batch: the chunk on the device). route: NULL, or n_pairs bytes of the caller's, one LCTY_ROUTE_* per pair in input
 * order (set it before the call; 0 pairs scored so far: untouched). Read-only; synchronises the context's stream. */
#define LCTY_ROUTE_LEAN    0
#define LCTY_ROUTE_TWO     1
#define LCTY_ROUTE_GENERAL 2
#define LCTY_LEAN_FORM_NONE  0   /* the lean kernel did not run: n_general == n_pairs */
#define LCTY_LEAN_FORM_INDEX 1   /* pass 1 leaves the record's index, pass 3 scores the record again (more than 309 alleles) */
#define LCTY_LEAN_FORM_KEEP  2   /* pass 1's products stay in LDS */
typedef struct lcty_score_routes {
    uint64_t n_pairs, n_lean, n_two, n_general;
    int32_t  lean_form;      /* LCTY_LEAN_FORM_* */
    int32_t  two_ran;        /* 1: the two-slot form ran between the lean and the general kernel */
    uint8_t* route;          /* in: NULL or [n_pairs] */
} lcty_score_routes;
int32_t lcty_reads_score_routes(lcty_reads* reads, lcty_score_routes* out);

/* per-pair products of load(): any pointer may be NULL */
int32_t lcty_reads_get_status(lcty_reads* reads, uint8_t* status, double* weight,
                              double* unmapped_prob, uint16_t* uniq_kmers /* [2*n_pairs] */);
/* number of LCTY_READ_GOOD pairs (AllAlignments::reads().len()) */
int32_t lcty_reads_n_good(lcty_reads* reads, uint64_t* out);
/* AllAlignments::best_aln_matrix (locs.rs:1203-1212): out[a*n_good + j], j over GOOD
 * pairs in input order (the order produced with threads == 1, locs.rs:1149). */
int32_t lcty_best_aln_matrix(lcty_reads* reads, double* out);
/* GrouppedAlignments::aln_pairs of every GOOD and FEW_KMERS pair, CSR over all input
 * pairs: off[n_pairs+1]; entries contig-ascending, ln_prob-descending inside a contig
 * (locs.rs:819-851). Call with out == NULL to obtain only the offsets / total. */
int32_t lcty_reads_get_pair_alns(lcty_reads* reads, uint64_t* off, lcty_pair_aln* out, uint64_t cap);
/* The record table as the batch holds it now: after lcty_recover_alignments the caller's records with the transferred alignments
 * behind the original records of their read end (secondary records, CIGAR offsets relative to the pair's block as everywhere) — the
 * `table` lcty_write_bam needs then. aln_off / cigar_off [n_pairs + 1]; recs = cigar = NULL: the sizes only (aln_off[n_pairs],
 * cigar_off[n_pairs]). Not for counted or streaming batches. */
int32_t lcty_reads_get_records(lcty_reads* reads, uint64_t* aln_off, lcty_aln_rec* recs, uint64_t cap_recs, uint64_t* cigar_off, uint32_t* cigar,
                               uint64_t cap_cigar);

/* run_filter (src/solvers/solve.rs:87-122): scores[g] = prior[g] + sum_r max_{a in g} M[a][r].
 * genotypes == NULL: all multisets of size `ploidy` in the order of
 * gen_combinations_with_repl (src/ext/vec.rs:298-339), n_genotypes is then checked
 * against count_combinations_with_repl. priors == NULL: all 0.0.                     */
int32_t lcty_prefilter(lcty_reads* reads, const uint16_t* genotypes, uint64_t n_genotypes,
                       uint32_t ploidy, const double* priors, double* scores);
/* device-only variant used by the timed path: leaves the scores in HBM */
int32_t lcty_prefilter_async(lcty_reads* reads, uint32_t ploidy);
int32_t lcty_prefilter_scores(lcty_reads* reads, double* scores, uint64_t n);

/* truncate_ixs (src/solvers/solve.rs:52-84). ixs: in = candidate indices, out = kept,
 * sorted by (score desc, index asc); returns the kept count in *n_keep.              */
int32_t lcty_truncate(const double* scores, uint64_t* ixs, uint64_t n, double filt_diff,
                      uint64_t min_size, uint64_t threads, uint64_t* n_keep);

/* The same on the scores the last prefilter call left on the device (lcty_prefilter_async / lcty_prefilter /
 * lcty_prefilter_allreduce), all genotypes as candidates: a stable device radix sort of (score descending, index ascending) and the
 * prefix truncate_ixs keeps; only the kept indices come to the host (at 4 096 alleles the scores are 67 MB). ixs = NULL: *n_keep only. */
int32_t lcty_prefilter_truncate(lcty_reads* reads, double filt_diff, uint64_t min_size, uint64_t threads, uint64_t* ixs, uint64_t cap,
                                uint64_t* n_keep);
/* scores[g] = priors[g] + scores[g] on the device (run_filter, solve.rs:114: `--priors`), between lcty_prefilter_async (or the
 * all-reduce) and lcty_prefilter_truncate; n = the number of genotypes of the last prefilter call. */
int32_t lcty_prefilter_add_priors(lcty_reads* reads, const double* priors, uint64_t n);

/* generate_genotypes without priors (src/command/genotype.rs:1120-1126) */
uint64_t lcty_count_genotypes(uint32_t n_alleles, uint32_t ploidy);
int32_t  lcty_generate_genotypes(uint32_t n_alleles, uint32_t ploidy, uint16_t* out, uint64_t cap);

/* Per-read posteriors: assignment counts of a genotype's attempts (lcty_assignment_counts) -> probability and mapping quality of
 * every (read, location), as the output BAMs carry them in the `pr` tag / MAPQ — count_to_prob (src/model/bam.rs:56-67):
 * 0 -> (0, 0); all attempts -> (1, 60); otherwise count / attempts in f32 and min(60, round(-10 log10(1 - p))). */
int32_t lcty_counts_to_posteriors(const uint16_t* counts, uint64_t n, uint16_t attempts, float* prob, uint8_t* mapq);

/* ---- one locus over several GPUs: the exchange step -----------------------------------------------------------
 * run_filter's score of a genotype is a sum over reads (solve.rs:105-119): with the reads of a locus sharded over ranks (one process
 * per GPU), every rank runs lcty_score_reads + lcty_prefilter_async on its shard and lcty_prefilter_allreduce sums the G-long f64
 * vectors in place on the devices (RCCL all-reduce over xGMI); lcty_prefilter_scores then returns the scores of the whole batch on
 * every rank and truncate_ixs proceeds identically everywhere. Priors are added afterwards (they are not per-read).
 * lcty_comm_unique_id: ncclGetUniqueId on rank 0; the launcher hands the 128 bytes to the other ranks. n_ranks == 1 is allowed. */
#define LCTY_COMM_ID_BYTES 128
typedef struct lcty_comm lcty_comm;
int32_t lcty_comm_unique_id(uint8_t* id);
int32_t lcty_comm_create(lcty_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t* id, lcty_comm** out);
void    lcty_comm_destroy(lcty_comm* comm);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank): the launcher's proof of how many ranks an
 * exchange really spans (bench.py prints it) */
int32_t lcty_comm_ranks(const lcty_comm* comm, int32_t* n_ranks, int32_t* rank);
/* Every exchange below: whatever a rank does on its own between two collectives (checks, allocations, launches) runs behind a
 * status agreement — a three-word MAX all-reduce every rank joins unconditionally — so that a failure on one rank makes ALL ranks
 * return an error (the failing rank its own status, the others "another rank failed") instead of leaving them inside RCCL; the
 * same agreement carries the sizes the next collective depends on and refuses ranks that disagree about them.
 * (Test hook: lcty_ctx_set_knob "comm_fail_at" = k fails the k-th agreement of a call on this rank.) */
int32_t lcty_prefilter_allreduce(lcty_reads* reads, lcty_comm* comm);
/* One solver stage with its (genotype, attempt) chains dealt to the ranks of `comm` (SURVEY.md 8e level 3; the reference deals
 * the genotypes of a stage to its worker threads, solve.rs:1052-1062): every rank passes the SAME arguments and holds the same
 * scored reads; rank r runs the r-th contiguous block of the genotype list, the per-chain likelihoods are all-gathered on the
 * devices (RCCL) and every rank returns mean / variance / likelihoods of ALL n_gt genotypes — bit for bit what lcty_solve_stage
 * returns on one GPU, for any number of ranks. */
int32_t lcty_solve_stage_sharded(lcty_reads* reads, lcty_comm* comm, const uint16_t* genotypes, uint64_t n_gt, uint32_t ploidy,
                                 const double* priors, const lcty_solver* solver, uint32_t attempts, const uint64_t* chain_seeds,
                                 double* lik_mean, double* lik_var, double* liks_out /* [n_gt][attempts] or NULL */);
/* One solver stage of a locus whose READS are sharded over the ranks (SURVEY.md 8e level 2 carried through the solver; BASELINE
 * configs[4]): rank r scored the r-th contiguous block of the locus' read list into `shard`. GenotypeAlignments::new walks every
 * read of the locus (assgn.rs:41-84), so the ranks exchange what a stage needs of it: the location-table rows of the alleles
 * of the stage's genotypes — 32 B per (allele, good read pair) plus the runs of further pair-alignments — packed, all-gathered
 * in chunks of rows (RCCL) and laid side by side in rank order. The chains are then dealt to the ranks as in
 * lcty_solve_stage_sharded and their likelihoods all-gathered. Every rank passes the same stage arguments and gets the results of
 * all n_gt genotypes — bit for bit what lcty_solve_stage returns on the unsharded batch. Device memory: alleles-of-the-stage x
 * good read pairs of the locus x 32 B per rank (LCTY_ERR_RUNTIME when that does not fit).
 * lcty_count_unexplained of a sharded locus: the sum of the ranks' counts. */
int32_t lcty_solve_stage_read_sharded(lcty_reads* shard, lcty_comm* comm, const uint16_t* genotypes, uint64_t n_gt, uint32_t ploidy,
                                      const double* priors, const lcty_solver* solver, uint32_t attempts, const uint64_t* chain_seeds,
                                      double* lik_mean, double* lik_var, double* liks_out /* [n_gt][attempts] or NULL */);
/* The same with every shard on ONE device and no exchange: `shards` in read order, all of one locus and one context. The packing
 * and the side-by-side layout are the code lcty_solve_stage_read_sharded runs between its collectives. Scratch lives on shards[0]. */
int32_t lcty_solve_stage_from_shards(lcty_reads* const* shards, uint32_t n_shards, const uint16_t* genotypes, uint64_t n_gt,
                                     uint32_t ploidy, const double* priors, const lcty_solver* solver, uint32_t attempts,
                                     const uint64_t* chain_seeds, double* lik_mean, double* lik_var, double* liks_out);

/* ---- alignment recovery (AllAlignments::load with opt_hap_alns = Some; src/seq/transfer.rs, src/seq/cigar.rs:1085-1384,
 * src/seq/wfa.rs) ------------------------------------------------------------------------------------------------------
 * lcty_locus_set_hap_alns: the pairwise haplotype alignments of `haplotypes.paf` as HapAlns::add takes them (transfer.rs:41-62):
 * entry t aligns contig id1[t] (query) to contig id2[t] (target) over their full lengths on the forward strand
 * (PafEntry::full_positive_alignment), CIGAR = raw BAM words cigar[cigar_off[t] .. cigar_off[t+1]) with =, X, I, D;
 * n_matches / aln_len as in the PAF columns (divergence filter: (aln_len - n_matches) / aln_len <= max_div, paf.rs:201-208).
 * The first entry of a pair of contigs wins; targets of a contig are tried in order of decreasing n_matches.
 * lcty_recover_alignments: transfer_alignments (transfer.rs:70-140) for every read pair of the batch that reaches
 * recover_and_group_alignments with weight >= min_weight (locs.rs:1255-1260). Call order:
 *     lcty_score_reads -> lcty_recover_alignments -> lcty_score_reads.
 * Transferred alignments become records of the batch (after the original records of their read end); nothing can be appended
 * to the batch afterwards. The aligner is an exact gap-affine dynamic programme (WFA2-lib computes the same optimum). Lanes
 * hold stretches between anchors of up to 255 bases; a read pair with a transfer that needs more is repeated with larger lane
 * scratch (2 047, then 16 383 bases; transferred CIGARs of up to 16 x the level-0 capacity) and LCTY_ERR_UNSUPPORTED beyond.
 * lcty_recover_stats: level_pairs[3] = read pairs the last lcty_recover_alignments took at each of the three levels. */
int32_t lcty_locus_set_hap_alns(lcty_locus* locus, uint32_t n_entries, const uint32_t* id1, const uint32_t* id2, const uint64_t* cigar_off,
                                const uint32_t* cigar, const uint32_t* n_matches, const uint32_t* aln_len, uint32_t transfer_fails,
                                double max_div);
int32_t lcty_recover_alignments(lcty_reads* reads, uint64_t* n_recovered);
int32_t lcty_recover_stats(lcty_reads* reads, uint64_t* level_pairs);
/* cells of the gap-affine aligner's matrices (the stand-in for WFA2, src/seq/wfa.rs:162-365) filled by the last
 * lcty_recover_alignments on this batch: cells / kernel time = the GCUPS figure of SURVEY.md section 8(d) */
int32_t lcty_recover_dp_cells(lcty_reads* reads, uint64_t* cells);

/* ---- minimizer read recruitment: the step of `locityper genotype` immediately before the path (SURVEY.md §8f rank 1;
 * src/seq/recruit.rs, src/seq/kmers.rs:71-340, src/math/frac.rs) ----------------------------------------------------------------
 * lcty_recruit_params_default: DEFAULT_MINIM_KW = (15, 10), match length 2000, k-mer threshold 50 (genotype.rs:136-139) and
 *   Technology::default_match_frac (bg/mod.rs:245-252).
 * lcty_targets_create / _add_locus / _finalize: recruit::Params::new (recruit.rs:65-105), TargetBuilder::add (688-738: canonical
 *   minimizers of every allele, rare = off-target count of the k-mer around the minimizer < thresh_kmer_count) and ::finalize.
 *   counts / cnt_off / base_k as in lcty_locus_create. Loci are numbered in the order they are added.
 * lcty_recruit: Targets::recruit_read_pair (883-929) for every pair of the chunk when `paired`, otherwise recruit_short_read
 *   (848-879) for single reads of up to 500 bases and recruit_long_read (938-996) beyond, as upstream dispatches (589-595).
 *   Mates of a pair: up to 256 bases; loci per read: up to 8 (16 for single reads beyond 256 bases); anything else is
 *   LCTY_ERR_UNSUPPORTED, never a different answer. Only the sequence fields of the chunk are read. Output: out_cnt[i] loci of
 *   pair i in out_loci[i * max_out ...], increasing (the reference writes the read to the files of exactly these loci). */
typedef struct lcty_recruit_params {
    double   match_frac;
    uint32_t match_length;
    uint16_t thresh_kmer_count;
    uint8_t  minimizer_k, minimizer_w;
} lcty_recruit_params;
typedef struct lcty_targets lcty_targets;
int32_t lcty_recruit_params_default(lcty_recruit_params* p, int32_t technology, int32_t is_paired);
int32_t lcty_targets_create(lcty_ctx* ctx, const lcty_recruit_params* params, lcty_targets** out);
void    lcty_targets_destroy(lcty_targets* targets);
int32_t lcty_targets_add_locus(lcty_targets* targets, uint32_t n_alleles, const uint8_t* seqs, const uint64_t* seq_off,
                               const uint16_t* counts, const uint64_t* cnt_off, uint32_t base_k, uint32_t* locus_ix);
int32_t lcty_targets_finalize(lcty_targets* targets, uint64_t* n_minimizers);
int32_t lcty_recruit(lcty_targets* targets, const lcty_reads_host* chunk, int32_t paired, uint32_t max_out, uint32_t* out_cnt,
                     uint32_t* out_loci);

/* ---- the readers and writers around recruitment (host; src/seq/fastx.rs, src/seq/recruit.rs:1000-1030) -------------------------
 * lcty_fastx_open: Reader::from_path (fastx.rs:296-312) on one FASTA / FASTQ file (plain or gzip), PairedEndInterleaved (444-466)
 *   with `interleaved`, PairedEndReaders (473-511) with a second file. lcty_fastx_next: up to max_records records (read pairs when
 *   paired) as the sequence fields of a chunk — what lcty_recruit reads; every byte but A, C, G, T is "not ACGT" (seq/kmers.rs:178-190)
 *   —; the arrays belong to the handle until the next call; *n = 0 at the end of the input. A record's name is its header up to the
 *   first blank (fastx.rs:417-419). Errors as upstream, LCTY_ERR_INVALID_DATA with the reference's messages: "Fastq record .. is
 *   incomplete" / "has incorrect format" / "has non-matching sequence and qualities", "Fasta record .. has an empty sequence.", "Odd
 *   number of records in an interleaved input file(s)", "non matching first and second mate(s)", "Different number of records in
 *   paired-end input files".
 * lcty_fastx_writers_open / lcty_fastx_write_recruited / _close: the per-locus read files of recruit_single_thread's loop
 *   (recruit.rs:1017-1021: `record.write_to(writers.get(locus_ix))` for every locus of the answer): record i of the LAST chunk goes
 *   to the writers out_loci[i * max_out .. + out_cnt[i]] as lcty_recruit filled them, as write_fastq / write_fasta leave it
 *   (fastx.rs:46-75) and both mates of a pair one after the other (141-150) — the `reads.fq` the mapper is given WITHOUT
 *   --interleaved. A path that ends in .gz is gzip-compressed. */
typedef struct lcty_fastx lcty_fastx;
typedef struct lcty_fastx_writers lcty_fastx_writers;
int32_t lcty_fastx_open(const char* path1, const char* path2, int32_t interleaved, lcty_fastx** out);
void    lcty_fastx_close(lcty_fastx* f);
int32_t lcty_fastx_is_paired(const lcty_fastx* f, int32_t* paired);
int32_t lcty_fastx_next(lcty_fastx* f, uint64_t max_records, lcty_reads_host* view, uint64_t* n);
int32_t lcty_fastx_writers_open(const char* const* paths, uint32_t n, lcty_fastx_writers** out);
int32_t lcty_fastx_write_recruited(lcty_fastx* f, lcty_fastx_writers* writers, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci,
                                   uint64_t* n_written);
int32_t lcty_fastx_writers_close(lcty_fastx_writers* writers);

/* ---- the same input parsed on the device ---------------------------------------------------------------------------
 * The route beside lcty_fastx_open for `locityper genotype -i reads_1.fq.gz reads_2.fq.gz`: the host reads windows of text (knob
 * "fastx_window_bytes" per file) into a page-locked slice — plain files by pread, BGZF files block by block through the inflate of
 * lcty_sample_bam_fetch (knob "sample_bam_inflate" 1: on the device), any other gzip through zlib —, kernels find lines and records,
 * lay the mates out and pack them, and recruitment reads them where they lie. Records, layout, packed words, status and message
 * are those of lcty_fastx_next for the same files, with one exception: a file that mixes FASTA and FASTQ records (fastx.rs:410-414
 * decides per record) is LCTY_ERR_UNSUPPORTED naming the record. The first offending record in input order decides.
 * lcty_fastx_device_open: Reader::from_path (fastx.rs:298-317), PairedEndInterleaved (423-453), PairedEndReaders (461-498) as
 *   lcty_fastx_open; nothing is read yet. .lz4 / .br: LCTY_ERR_UNSUPPORTED. lcty_fastx_device_is_paired: as lcty_fastx_is_paired.
 * lcty_fastx_device_next: read_next (fastx.rs:396-415, 437-453, 480-498) for up to max_records records (pairs, when paired) of the
 *   current window, resident on the device; *n = 0 at the end of the input; records of the window beyond max_records are carried
 *   to the next call. Records in front of a refused one are handed out; the call that would begin with it fails. A record
 *   that no window of "fastx_window_limit" bytes holds is LCTY_ERR_UNSUPPORTED naming knob "fastx_window_bytes". stats (may be
 *   NULL): sums since the handle was opened.
 * lcty_fastx_device_view: the chunk as lcty_fastx_next gives it, downloaded on first use; the arrays belong to the handle until
 *   the next call of lcty_fastx_device_next.
 * lcty_fastx_device_recruit: lcty_recruit (recruit.rs:1000-1030) on the chunk, from the device-resident arrays. The handle's
 *   context must be the targets', else LCTY_ERR_INVALID_INPUT.
 * lcty_fastx_device_write_recruited: write_fastq / write_fasta (fastx.rs:46-75, 262-272), the bytes lcty_fastx_write_recruited
 *   writes for the chunk: the text comes from the page-locked slice and the downloaded rows, a FASTA sequence on one line. */
typedef struct lcty_fastx_device lcty_fastx_device;
typedef struct lcty_fastx_device_stats {
    uint64_t bytes_read, bytes_inflated;          /* bytes read from the files; text that came out of a compressed container */
    uint64_t windows, windows_enlarged, records;  /* windows parsed (both files); of them: doubled for want of a complete record; records handed out */
    double   ms_read, ms_inflate;                 /* host: pread; zlib, or with "sample_bam_inflate" 1 upload + inflate kernel + copy back */
    double   ms_upload, ms_lines, ms_records, ms_pack;   /* device, wall clock around each stage with its synchronisation */
    double   ms_total;                            /* inside lcty_fastx_device_next */
} lcty_fastx_device_stats;
int32_t lcty_fastx_device_open(lcty_ctx* ctx, const char* path1, const char* path2, int32_t interleaved, lcty_fastx_device** out);
void    lcty_fastx_device_close(lcty_fastx_device* f);
int32_t lcty_fastx_device_is_paired(const lcty_fastx_device* f, int32_t* paired);
int32_t lcty_fastx_device_next(lcty_fastx_device* f, uint64_t max_records, uint64_t* n, lcty_fastx_device_stats* stats);
int32_t lcty_fastx_device_view(lcty_fastx_device* f, lcty_reads_host* view);
int32_t lcty_fastx_device_recruit(lcty_targets* targets, lcty_fastx_device* f, uint32_t max_out, uint32_t* out_cnt, uint32_t* out_loci);
int32_t lcty_fastx_device_write_recruited(lcty_fastx_device* f, lcty_fastx_writers* writers, uint32_t max_out, const uint32_t* out_cnt,
                                          const uint32_t* out_loci, uint64_t* n_written);

/* ---- a sample's reads from a coordinate-sorted, indexed BAM file: `locityper genotype -a sample.bam` ---------------
 * recruit_to_targets (command/genotype.rs:872-907) -> create_fetch_targets / postprocess_targets (776-854) -> IndexedBamReader +
 * PairedBamReader (seq/fastx.rs:577-874) -> Targets::recruit. The index, the file access and the inflation of the selected BGZF
 * blocks are host code (the inflation runs on the device with lcty_ctx_set_knob "sample_bam_inflate" 1); the fetched slice becomes recruitable read pairs on the device (record filter, name pairing, unpacking
 * with strand restore) and is recruited from there. The rules are restated index-free in tests/pyref_sample_bam.py.
 * lcty_sample_bam_open: bam::IndexedReader::from_path / from_path_and_index (genotype.rs:886-890): the header, and the BAI index
 *   at index_path, or else at path + ".bai", or else at path with ".bam" replaced by ".bai". A CSI index or a CRAM file is
 *   LCTY_ERR_UNSUPPORTED, no index LCTY_ERR_INVALID_INPUT. Host code. lcty_sample_bam_contigs: ContigNames::from_bam_header (892):
 *   name i = names + name_off[i], 0-terminated; the arrays belong to the handle.
 * lcty_sample_bam_is_paired: identify_pairedness (857-867): flag 0x1 of the first record; a file without records is
 *   LCTY_ERR_INVALID_DATA "Input BAM/CRAM file is empty".
 * lcty_recruit_fetch_regions: postprocess_targets (776-797), host code: every interval padded (Interval::add_padding,
 *   seq/interv.rs:74-77: start - padding saturating at 0, end + padding at most the contig's length), every contig SHORTER than
 *   alt_contig_len appended whole, sorted by (tid, start, end), merged (Interval::merge, 232-247: the next interval joins the last
 *   when last.end + merge_distance >= next.start). The reference uses merge_distance 1000, alt_contig_len 10 000 000 and padding =
 *   min(ceil(quantile 0.999 of the insert size distribution), 10 000) + 100, or 1000 without one (genotype.rs:848-852); the padding
 *   is the caller's. The out arrays hold n_in + n_contigs entries. tid >= n_contigs, start >= end: LCTY_ERR_INVALID_INPUT.
 * lcty_sample_bam_plan: the chunks of virtual offsets a fetch of these regions reads, host code: reg2bins, chunks that end at or
 *   before the linear index's offset of the region's first 16 kb window dropped, sorted, and chunks that touch, overlap or meet
 *   in one BGZF block merged over all regions of the call; with_unmapped adds [largest chunk end of the index, end of file).
 *   Up to chunk_cap chunks are written, *n_chunks is their number; *blocks_total (may be NULL) the BGZF blocks they span, read
 *   from the file. Regions are (tid, start, end), sorted, strictly increasing and disjoint as postprocess_targets leaves them:
 *   anything else is LCTY_ERR_INVALID_INPUT (the reference asserts, fastx.rs:770).
 * lcty_sample_bam_fetch: IndexedBamReader (732-803) [+ PairedBamReader (805-874) with paired = 1; paired = -1 asks the file],
 *   one call per sample. Region i gives the records with tid == tid_i, pos < end_i, endpos > start_i (endpos = pos + reference
 *   length of the CIGAR, 0 for a record with flag 0x4, 0 counting as 1) in file order; one is kept iff (flag & 0x900) == 0 and
 *   pos >= end_(i-1) when region i - 1 is on the same contig (587-611, 762-783). with_unmapped: then the primaries without
 *   coordinate (tid < 0). whole_file != 0 (n_regions == 0, with_unmapped == 0): DirectBamReader (692-729), every primary of the
 *   file, single-end only (paired: LCTY_ERR_UNSUPPORTED). A record's sequence is reversed and complemented when flag 0x10 is set;
 *   every BAM code but A, C, G, T is "not ACGT". Pairs: per record of that stream as read_next (829-869) — a record without
 *   0x40 / 0x80 is LCTY_ERR_INVALID_DATA "Expected paired-end reads, but read .. is unpaired"; a waiting record of the same name
 *   with the same first-in-template flag is LCTY_ERR_INVALID_DATA "Found two primary alignments for .. for the same read end",
 *   otherwise the two are a pair (mate 1 the one with 0x40), in the order of the records that complete them; a record nobody waits
 *   for waits iff (tid as u32, pos as u64) <= (mtid as u32, mpos as u64), else it is discarded, as is whatever waits at the end.
 *   A kept record without sequence: LCTY_ERR_INVALID_DATA "Primary alignment for read .. has no sequence". The first offending
 *   record in file order decides. Beyond the reference: a record that leaves the fetched slice or is shorter than its fields, and
 *   (tid, pos) running backwards inside the slice: LCTY_ERR_INVALID_DATA; a primary mapped record whose CIGAR is the `kSmN`
 *   placeholder of a CG tag: LCTY_ERR_UNSUPPORTED with the read's name; an inflated slice above lcty_ctx_set_knob
 *   "sample_bam_max_slice_bytes" (default 2^33): LCTY_ERR_UNSUPPORTED before anything is uploaded; 2^31 records or more:
 *   LCTY_ERR_UNSUPPORTED. "sample_bam_hash_bits" (default 64) keeps that many bits of the hash of a read name: names are always
 *   compared in full, the hash only brings candidates together. stats may be NULL.
 * lcty_sample_reads_view: the reads as the sequence fields of a chunk, what lcty_fastx_next gives (single-end: every odd mate
 *   absent), and per mate the ordinal of its record in the fetched stream (0xFFFFFFFF: absent); downloaded on first use, the
 *   arrays belong to the handle. lcty_sample_reads_recruit: lcty_recruit on that view, from the device-resident arrays (paired as
 *   fetched). lcty_sample_reads_write_recruited: BamRecord::write_to (633-668) to the writers of exactly the loci of the answer, both
 *   mates one after the other: FASTA when the qualities are absent or start with 255, else FASTQ with q + 33, reversed for reverse
 *   records. Not built: CRAM, CSI, several files, subsampling. */
typedef struct lcty_sample_bam lcty_sample_bam;
typedef struct lcty_sample_reads lcty_sample_reads;
typedef struct lcty_sample_bam_stats {
    uint64_t n_regions, n_chunks;                 /* as given; after merging */
    uint64_t file_bytes, bytes_read;              /* size of the BAM file; compressed bytes read from it */
    uint64_t blocks_inflated, bytes_inflated;     /* BGZF blocks of the chunks; their inflated size */
    uint64_t records_walked, records_primary, records_kept;
    uint64_t n_pairs, n_discarded;                /* paired: pairs made, kept records without a pair; single-end: reads, 0 */
    double   ms_read, ms_inflate, ms_walk;        /* host: pread, inflate (at most 16 threads), the chain of record lengths */
    double   ms_upload, ms_record, ms_pair, ms_unpack;   /* device, wall clock around each stage with its synchronisation */
    /* with knob "sample_bam_inflate" 1: ms_inflate = upload of the compressed bytes + the inflate kernel + the copy of the slice back
     * to the host, and ms_upload = what is still uploaded afterwards (record offsets, regions; the slice is on the device already) */
    double   ms_total;
} lcty_sample_bam_stats;
int32_t lcty_sample_bam_open(const char* path, const char* index_path, lcty_sample_bam** out);
void    lcty_sample_bam_close(lcty_sample_bam* bam);
int32_t lcty_sample_bam_contigs(const lcty_sample_bam* bam, uint32_t* n, const char** names, const uint64_t** name_off, const uint32_t** lengths);
int32_t lcty_sample_bam_is_paired(lcty_sample_bam* bam, int32_t* paired);
int32_t lcty_recruit_fetch_regions(uint32_t n_in, const uint32_t* tid, const uint32_t* start, const uint32_t* end, uint32_t n_contigs,
                                   const uint32_t* contig_len, uint32_t padding, uint32_t alt_contig_len, uint32_t merge_distance,
                                   uint32_t* out_tid, uint32_t* out_start, uint32_t* out_end, uint32_t* n_out);
int32_t lcty_sample_bam_plan(lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start, const uint32_t* end,
                             int32_t with_unmapped, uint64_t chunk_cap, uint64_t* n_chunks, uint64_t* chunk_beg, uint64_t* chunk_end,
                             uint64_t* blocks_total);
int32_t lcty_sample_bam_fetch(lcty_ctx* ctx, lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start,
                              const uint32_t* end, int32_t with_unmapped, int32_t whole_file, int32_t paired, lcty_sample_reads** reads,
                              lcty_sample_bam_stats* stats);
int32_t lcty_sample_reads_view(lcty_sample_reads* reads, lcty_reads_host* view, const uint32_t** src_record, int32_t* paired);
int32_t lcty_sample_reads_recruit(lcty_targets* targets, lcty_sample_reads* reads, uint32_t max_out, uint32_t* out_cnt, uint32_t* out_loci);
int32_t lcty_sample_reads_write_recruited(lcty_sample_reads* reads, lcty_fastx_writers* writers, uint32_t max_out, const uint32_t* out_cnt,
                                          const uint32_t* out_loci, uint64_t* n_written);
void    lcty_sample_reads_free(lcty_sample_reads* reads);

/* ---- Whole BAM files without an index, streamed through the device in windows --------------------------------------
 * `locityper genotype|recruit -a reads.bam [-a ...] --no-index [-^]`: process_readers! (src/seq/fastx.rs:1029-1043) -> DirectBamReader
 * (692-729), under PairedEndInterleaved (423-453) with -^. How unaligned BAM files (PacBio HiFi, ONT), name-collated paired files and
 * several files given as one input arrive. The rules are restated in tests/pyref_bam_stream.py.
 * lcty_bam_stream_open: DirectBamReader::new: every file is opened and its header read now; no index is looked for, the contigs are
 *   ignored. n_paths == 0 or a null argument: LCTY_ERR_INVALID_INPUT; a path that cannot be opened: LCTY_ERR_INVALID_INPUT; a CRAM
 *   file: LCTY_ERR_UNSUPPORTED; bytes that are not BGZF or not BAM (an empty file included): LCTY_ERR_INVALID_DATA "... is not a BAM
 *   file"; a truncated header: LCTY_ERR_INVALID_DATA. Host code.
 * lcty_bam_stream_next: one chunk per call, all reads of one window: whole BGZF blocks of the current file until the inflated bytes,
 *   the tail carried from the last window included, reach knob "bam_stream_window_bytes" or the file ends (inflated on the host, or
 *   with knob "sample_bam_inflate" 1 on the device); the chain of record lengths is walked on the host, everything else runs on the
 *   device. The stream is the records of file 0, then file 1, ...; a record is kept iff (flag & 0x900) == 0, nothing else of it
 *   matters; its sequence is reversed and complemented with flag 0x10, every code but A, C, G, T is "not ACGT". interleaved == 0: every
 *   kept record is a read (mate 2 absent). interleaved: kept records 2 i and 2 i + 1 of the whole stream are mates 1 and 2 of pair i,
 *   whatever their flags, any number of other records apart and in different files; their names a, b (without the NUL) must satisfy
 *   len(a) == len(b) && (len(a) <= 3 || a[len - 3] == b[len - 3]) (equal_names_fast).
 *   *n: the reads, or pairs, of the chunk; 0 only at the end of the last file (a window that completes no read makes the call go on
 *   to the next window). *reads belongs to the stream: it is valid until the next lcty_bam_stream_next or lcty_bam_stream_close and is
 *   NEVER passed to lcty_sample_reads_free. lcty_sample_reads_view, _recruit, _write_recruited and lcty_recruited_add_sample work on it
 *   unchanged; src_record of the view is the ordinal among the kept records of the chunk's window, stats.first_kept + src_record the
 *   ordinal among the kept records of the whole input.
 *   Errors, LCTY_ERR_INVALID_DATA: a kept record without sequence ("Primary alignment for read <name> has no sequence"); a name
 *   mismatch ("Interleaved input file(s) <paths> contains non matching first and second mate (<a> and <b>)"); a kept record left alone
 *   at the end of the last file ("Odd number of records in an interleaved input file(s) <paths>"); a record shorter than its fields, or
 *   one that leaves the end of its file (a record never continues in the next file), naming the file. LCTY_ERR_UNSUPPORTED: a window of
 *   2^31 - 16 records or more; a record beyond knob "bam_stream_window_limit". The first offending record in input order decides (for a
 *   mismatch the second mate): reads completed in front of it are handed out, by a call that returns LCTY_OK; the call that would begin
 *   with the offending record fails, and so does every call after it. What was handed out does not depend on the window knob.
 *   stats (may be NULL): sums since lcty_bam_stream_open, every record counted once, whatever the window (a window that ends in an
 *   error counts the records in front of it); first_kept belongs to this chunk. */
typedef struct lcty_bam_stream lcty_bam_stream;
typedef struct lcty_bam_stream_stats {
    uint64_t files, file_bytes, bytes_read, blocks_inflated, bytes_inflated;   /* sums since open */
    uint64_t windows, windows_enlarged, bytes_carried;
    uint64_t records_walked, records_primary, records_kept, bases_kept;        /* every record counted once, whatever the window */
    uint64_t reads;            /* reads, or pairs, handed out */
    uint64_t first_kept;       /* of THIS chunk: ordinal in the whole input of record 0 of its window's kept stream */
    double   ms_read, ms_inflate, ms_walk, ms_upload, ms_record, ms_pair, ms_unpack, ms_total;
} lcty_bam_stream_stats;
int32_t lcty_bam_stream_open(lcty_ctx* ctx, const char* const* paths, uint32_t n_paths, int32_t interleaved, lcty_bam_stream** out);
void    lcty_bam_stream_close(lcty_bam_stream* s);
int32_t lcty_bam_stream_next(lcty_bam_stream* s, lcty_sample_reads** reads, uint64_t* n, lcty_bam_stream_stats* stats);

/* ---- BGZF blocks inflated on the device ------------------------------------------------------------------------------
 * BGZF is the SAM specification's section 4.1: gzip members (RFC 1952) of at most 64 KB each, whose extra field holds the block's
 * size and whose payload is a raw DEFLATE stream (RFC 1951) followed by CRC32 and ISIZE. No counterpart upstream: the reference reads
 * BGZF through htslib, which inflates on the host.
 * lcty_bgzf_inflate: comp holds whole BGZF blocks back to back (host memory); they are split as lcty_sample_bam_fetch splits them,
 *   uploaded, inflated one wavefront per block, checked against their CRC32 and ISIZE on the device, and downloaded to out in
 *   order. *out_len = the sum of the ISIZE fields, written whenever the headers parse; out == NULL only sizes. Blocks of ISIZE 0
 *   (the end-of-file marker) are skipped. The decoder accepts exactly what zlib's inflate accepts (locityper_amd/csrc/
 *   lcty_inflate.hpp states the rules; tests/test_bgzf_inflate_host.py holds it to zlib on the CPU). Bytes that are not a BGZF block at
 *   some offset, or a block that says it inflates to more than 65 536 bytes: LCTY_ERR_INVALID_DATA naming the offset; out_cap below
 *   *out_len: LCTY_ERR_INVALID_INPUT; a block the decoder refuses: LCTY_ERR_INVALID_DATA "corrupt BGZF block at offset N (class)",
 *   the first one in input order. A block whose gzip FLG byte is not exactly 4 (FEXTRA alone, what every BAM writer sets) sends
 *   the whole call through zlib on the host (ms_upload, ms_kernel, ms_download stay 0). stats may be NULL. */
typedef struct lcty_bgzf_stats {
    uint64_t n_blocks, bytes_in, bytes_out;       /* blocks, the EOF marker included; compressed bytes; inflated bytes */
    double   ms_upload, ms_kernel, ms_download;   /* wall clock around each stage with its synchronisation */
    double   ms_total;
} lcty_bgzf_stats;
int32_t lcty_bgzf_inflate(lcty_ctx* ctx, const uint8_t* comp, uint64_t n_comp, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                          lcty_bgzf_stats* stats);

/* ---- BGZF blocks deflated on the device -------------------------------------------------------------------------------
 * The writing half of the section above. No counterpart upstream: htslib deflates on the host (bam::Writer, bgzf::Writer).
 * lcty_bgzf_deflate: data (host memory) is cut every 0xff00 bytes, where lcty_io_write_bgzf and lcty_write_bam cut it, uploaded,
 *   deflated one wavefront per block (locityper_amd/csrc/lcty_deflate.hpp: hash matches in groups of 64 positions, a greedy parse, and
 *   the smallest of the stored, fixed and dynamic forms; tests/test_bgzf_deflate_host.py holds the same text to zlib's inflate on the
 *   CPU), given the 18-byte header (FLG 4, the BC subfield) and the CRC32 / ISIZE trailer, packed back to back on the device and
 *   downloaded to out. with_eof appends the 28-byte end-of-file marker. *out_len = the bytes written. block_off: NULL, or
 *   ceil(len / 0xff00) + 1 offsets in out: the start of every data block, and the end of the last. The bytes depend on `data` alone,
 *   not on the device, the grid or knob "bgzf_deflate_max_bytes" (the slice an input above it is processed in). len == 0 gives the
 *   marker alone, or nothing. They are not zlib's bytes: any inflater gives `data` back.
 *   out_cap is asked for up front, the exact size not being known: below lcty_bgzf_deflate_bound (a stored block takes n + 31 bytes)
 *   the call is LCTY_ERR_INVALID_INPUT, as are null arguments and a slice knob below one block. stats may be NULL.
 * lcty_io_write_bgzf_device: lcty_io_write_bgzf through lcty_bgzf_deflate: the same blocks of inflated bytes and the marker. */
typedef struct lcty_bgzf_deflate_stats {
    uint64_t n_blocks, bytes_in, bytes_out;      /* data blocks (EOF marker not counted); raw bytes; file bytes */
    uint64_t n_stored, n_fixed, n_dynamic;       /* blocks by the form chosen */
    double   ms_upload, ms_kernel, ms_download, ms_total;
} lcty_bgzf_deflate_stats;
uint64_t lcty_bgzf_deflate_bound(uint64_t len, int32_t with_eof);   /* len + 31 * ceil(len / 0xff00) + 28 * with_eof */
int32_t  lcty_bgzf_deflate(lcty_ctx* ctx, const uint8_t* data, uint64_t len, int32_t with_eof, uint8_t* out, uint64_t out_cap,
                           uint64_t* out_len, uint64_t* block_off /* NULL or ceil(len/0xff00)+1 compressed offsets */,
                           lcty_bgzf_deflate_stats* stats);
int32_t  lcty_io_write_bgzf_device(lcty_ctx* ctx, const char* path, const uint8_t* data, uint64_t len, lcty_bgzf_deflate_stats* stats);

/* ---- candidate generation inside a locus (first slice) ----------------------------------------------------
 * The reference runs an external mapper per locus — strobealign -k 15 -N/-M min(25000, 4 x alleles) -S 0.5 --eqx for short
 * reads (src/command/genotype.rs:962-1005), piped through samtools view -e "[AS] >= 50 || flag & 2304 == 0" (1055-1094), on the
 * basis haplotypes when --basis is given (1007-1052) — and reads the resulting aln.bam. No mapper source is in the reference
 * tree; the algorithm of this slice is this build's own (locityper_amd/csrc/lcty_map.hip states it, tests/pyref_map.py restates
 * it): k-mer seeds every `stride` bases -> votes for (basis allele, strand, diagonal) -> per (allele, strand) the diagonal with
 * the most votes -> extension without gaps (+match / -mismatch per base, end_bonus per read end reached; the best-scoring stretch,
 * the rest soft-clipped), and for a clipped candidate a gap-affine alignment in a band around its diagonal that replaces it when it
 * scores higher -> the best candidate of a read end is its primary record, the others with score >= min_score secondary
 * records, a read end without candidates an unmapped record. Record order, flags, =/X/S CIGARs and SEQ orientation are those of
 * the BAM the reference reads, so the result is a chunk for lcty_reads_append; the alleles outside the basis are reached with
 * lcty_recover_alignments. Limits of this SHORT route: read ends of up to 256 bases, up to 32 basis alleles, seed length 8..31, at
 * most 64 seeds per read end and 1 024 votes (the first ones in seed order).
 * The LONG route (locityper_amd/csrc/lcty_map_long.hip states it, tests/pyref_map_long.py restates it) takes what the short one
 * refuses — the reference's long-read case, minimap2 -x map-ont / map-hifi --eqx (genotype.rs:990-1002): read ends of up to 2^20 - 1
 * bases on up to 256 basis alleles. Seeds as above (any number of them) -> every (seed, place) is an anchor (q, t) of its (basis allele,
 * strand), t on the allele in the read's orientation -> per (allele, strand) one chain: an anchor follows one of the `chain_back`
 * anchors of its group before it, at most `chain_gap` bases on in both sequences, at most `chain_skew` diagonals apart, gaining
 * min(dq, dt, k) - (0 if on the same diagonal else 2 + skew) -> the (allele, strand)s whose best chain has >= min_votes anchors and
 * >= half the score of the read end's best one are aligned along their chain: gap-affine (gaps open from any state) from node to
 * node, in a band of min(0, d) - band .. max(0, d) + band diagonals between two anchors d diagonals apart, and +- band beyond the first
 * and last anchor, where the alignment may stop (soft clip; end_bonus when the read end is reached) -> records as above, = / X / I / D / S
 * CIGARs. route: LCTY_MAP_ROUTE_AUTO takes the short route when the chunk and the index fit it.
 * lcty_locus_build_map_index: the k-mers of the basis alleles (hash table built on the device, once per locus).
 * lcty_map_reads: only the sequence fields of `chunk` are read. aln_off / cigar_off [n_pairs + 1] are always written; with
 *   recs == NULL the call only sizes. bases2_out / nmask_out: the chunk's bases in BAM orientation (same offsets). */
typedef struct lcty_map_params {
    uint32_t k, stride, min_votes;
    uint32_t max_occ;            /* seeds with more places in the index do not vote; 0: four per basis allele */
    int32_t  match, mismatch, end_bonus, min_score;
    uint32_t band;               /* diagonals on either side in the alignment with gaps of a clipped candidate (<= 16); 0: none */
    int32_t  gap_open, gap_extend;   /* a gap of n bases costs gap_open + (n - 1) * gap_extend */
    uint32_t route;              /* LCTY_MAP_ROUTE_* */
    uint32_t chain_gap;          /* long route: bases between two chained anchors, in either sequence (<= 8 192) */
    uint32_t chain_skew;         /* long route: diagonals between two chained anchors (<= 1 024) */
    uint32_t chain_back;         /* long route: anchors of its group an anchor looks back at (1..64) */
} lcty_map_params;
#define LCTY_MAP_ROUTE_AUTO  0u
#define LCTY_MAP_ROUTE_SHORT 1u
#define LCTY_MAP_ROUTE_LONG  2u
int32_t lcty_map_params_default(lcty_map_params* p);       /* strobealign's scores (short reads) */
int32_t lcty_map_params_default_long(lcty_map_params* p);  /* minimap2's (map-ont): seeds 16 bases apart, 2 / 4 / gap 4 + 2 n, every record kept */
int32_t lcty_locus_build_map_index(lcty_locus* locus, const uint16_t* basis, uint32_t n_basis, uint32_t k);
int32_t lcty_map_reads(lcty_locus* locus, const lcty_reads_host* chunk, const lcty_map_params* params, uint64_t* aln_off,
                       lcty_aln_rec* recs, uint64_t cap_recs, uint64_t* cigar_off, uint32_t* cigar, uint64_t cap_cigar,
                       uint32_t* bases2_out, uint32_t* nmask_out);
/* The same with the records going straight into a batch of the locus (as lcty_reads_append of the mapped chunk would put them):
 * records, CIGAR words and re-oriented bases are copied device to device, only the offsets visit the host. The device buffers of the
 * mapping (arenas and kernel scratch: tens of GB for long reads on many alleles) stay with the context from chunk to chunk; the solver
 * stages release them before they size their workspace, and so does lcty_ctx_trim. One mapping call at a time per context. */
int32_t lcty_reads_map_append(lcty_reads* reads, const lcty_reads_host* chunk, const lcty_map_params* params);

/* ---- the recruited reads of every locus, resident on the device, and the mapper fed from them ----------------------
 * The reference writes the reads of a locus to `reads.fq`, runs an external mapper on that file and reads its `aln.bam`
 * (command/genotype.rs:872-907, 962-1094). Here the recruited reads stay on the device in the layout the mapper reads, so that
 * recruitment and mapping meet without a file and without the host: SURVEY.md 8(f) rank 2.
 * lcty_recruited_create: an empty set over the loci of finalized targets (not finalized: LCTY_ERR_INVALID_INPUT); the targets outlive
 *   the set. keep_names != 0: the name of every added pair is kept per locus, on the host. Qualities are not kept.
 * lcty_recruited_add / _add_fastx / _add_sample: pair i of the chunk goes to exactly the loci out_loci[i * max_out .. + out_cnt[i]], the
 *   host arrays lcty_recruit / lcty_fastx_device_recruit / lcty_sample_reads_recruit filled, with the meaning they have in
 *   *_write_recruited. _add uploads a host chunk (only its sequence fields are read; `paired` is accepted for symmetry with lcty_recruit:
 *   an absent mate has length 0 either way), _add_fastx takes the chunk of the last lcty_fastx_device_next and _add_sample the fetched
 *   reads from where they lie on the device. Within a locus the pairs stand in input order — add after add, inside an add by i —, the
 *   order of the records of the reads.fq the writers produce for the same calls. Every pair carries a source ordinal: its index i plus
 *   the pairs of every earlier add of the set, recruited or not. The contents depend on the chunks and the answers alone (no atomics, no
 *   dependence on the grid): two runs give the same bytes. The set, the source handle and the targets share one context, else
 *   LCTY_ERR_INVALID_INPUT, as are out_cnt[i] > max_out and a locus beyond the targets'. 2^32 or more (locus, pair) entries or 2^31 or
 *   more 32-base units in one add: LCTY_ERR_UNSUPPORTED. The contents of the whole set after the add — 12 bytes per 32-base unit and
 *   32 bytes per pair, over all loci — above knob "recruited_max_bytes": LCTY_ERR_UNSUPPORTED naming the knob. All of this is decided
 *   before anything is copied: a failed add leaves the set as it was. A locus's arrays grow geometrically from knob
 *   "recruited_init_units", device to device.
 * lcty_recruited_sizes: the pairs of a locus and the bases its units span (32 per unit). locus_ix beyond the targets' loci is
 *   LCTY_ERR_INVALID_INPUT here and in every call below.
 * lcty_recruited_view: the reads of a locus as the sequence fields of one chunk, bit for bit what selecting those pairs from the source
 *   views (lcty_fastx_next / lcty_fastx_device_view / lcty_sample_reads_view) gives: the mates on consecutive 32-base units in the
 *   source's order, padding bits as they were, an absent mate with mate_len 0 and no unit; aln_off / cigar_off are zeros.
 *   src_ordinal (may be NULL): the ordinal of every pair. Downloaded on first use; the arrays belong to the set and hold until the
 *   next add that reaches the locus.
 * lcty_recruited_names: name i = names[name_off[i] .. name_off[i + 1]), one behind the other without terminators, as lcty_write_bam
 *   takes them: a FASTA / FASTQ header up to the first blank, a BAM record's read name (the first read end's). LCTY_ERR_INVALID_INPUT without keep_names, and once lcty_recruited_add,
 *   which has no names, has added a read.
 * lcty_reads_map_append_recruited: lcty_reads_map_append on pairs [first_pair, first_pair + n_pairs) of the locus, read where they lie
 *   (either route): same records, same bytes in the batch as for the host chunk of those pairs. A range that does not start at pair 0
 *   takes the bases in place as well; only its offsets are rebased, on the host. n_pairs == 0 does nothing; a range past the locus's
 *   pairs is LCTY_ERR_INVALID_INPUT, as is a batch of another context. */
typedef struct lcty_recruited lcty_recruited;
int32_t lcty_recruited_create(lcty_targets* targets, int32_t keep_names, lcty_recruited** out);
void    lcty_recruited_destroy(lcty_recruited* set);
int32_t lcty_recruited_add(lcty_recruited* set, const lcty_reads_host* chunk, int32_t paired, uint32_t max_out, const uint32_t* out_cnt,
                           const uint32_t* out_loci);
int32_t lcty_recruited_add_fastx(lcty_recruited* set, lcty_fastx_device* f, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci);
int32_t lcty_recruited_add_sample(lcty_recruited* set, lcty_sample_reads* reads, uint32_t max_out, const uint32_t* out_cnt,
                                  const uint32_t* out_loci);
int32_t lcty_recruited_sizes(lcty_recruited* set, uint32_t locus_ix, uint64_t* n_pairs, uint64_t* n_bases);
int32_t lcty_recruited_view(lcty_recruited* set, uint32_t locus_ix, lcty_reads_host* view, const uint64_t** src_ordinal);
int32_t lcty_recruited_names(lcty_recruited* set, uint32_t locus_ix, const uint64_t** name_off, const char** names);
int32_t lcty_reads_map_append_recruited(lcty_reads* reads, lcty_recruited* set, uint32_t locus_ix, uint64_t first_pair, uint64_t n_pairs,
                                        const lcty_map_params* params);

/* ---- solver stages (src/solvers/solve.rs:789-850, src/solvers/stoch.rs, src/model/assgn.rs) ----------------
 * The reference drives these stages from one Xoshiro256++ through rand ^0.10 adaptors that are not in its tree and
 * whose results already depend on --threads (solve.rs:1017, 1051). Here every (genotype, attempt) chain gets its
 * own 64-bit seed (lcty_chain_seeds draws them from seed_from_u64(master)); DESIGN.md §2 lists the adaptors. */
int32_t lcty_solver_default(lcty_solver* out, int32_t kind);                 /* Greedy::default / SimAnneal::default */
int32_t lcty_chain_seeds(uint64_t master_seed, uint64_t n, uint64_t* out);
/* One stage over genotypes[n_gt][ploidy] (the body of the stage loop, solve.rs:816-843): per genotype `attempts` x
 * (apply_tweak -> Solver::solve -> prior + likelihood), then mean_variance_or_nan. chain_seeds[n_gt*attempts];
 * liks_out (optional) [n_gt*attempts]. Device solver: ploidy <= 4. */
int32_t lcty_solve_stage(lcty_reads* reads, const uint16_t* genotypes, uint64_t n_gt, uint32_t ploidy, const double* priors,
                         const lcty_solver* solver, uint32_t attempts, const uint64_t* chain_seeds,
                         double* lik_mean, double* lik_var, double* liks_out);

/* ---- `trait Solver` on the caller's own object (src/solvers/mod.rs:49-75) ------------------------------------------------
 * The reference calls a solver as `gt_alns.apply_tweak(rng, ..); stage.solver.solve(&gt_alns, rng)` (solve.rs:824-826): the
 * solver is handed a GenotypeAlignments (model/assgn.rs:16-36) the CALLER built and tweaked, and returns a ReadAssignment
 * (assgn.rs:171-186) borrowing it. lcty_gt_alns_view is that object as plain arrays, lcty_solve_given is `Solver::solve` on it:
 * ONE chain of `solver` (Greedy, stoch.rs:81-120; SimAnneal, 195-245; the exact model of highs.rs:38-134) on the device, over
 * exactly the locations, windows and window distributions given — nothing is re-derived from a read batch and no tweak is drawn.
 *   read_ixs[n_reads + 1]   assgn.rs:29-33; read pair i has the locations read_ixs[i] .. read_ixs[i + 1] (at least one, best first)
 *   ln_prob[n_alns]         ReadGtAlns::ln_prob (windows.rs:83-92)
 *   windows[2 * n_alns]     ReadGtAlns::windows after define_windows_determ / _random (windows.rs:112-136)
 *   window_gc / _weight[n_windows]   depth_distrs (assgn.rs:21, 140-150): WindowDistr::weight, 0 = WindowDistr::TRIVIAL
 *                           (distr_cache.rs:28-31); the GC bin selects the cached distribution of `locus` (DistrCache,
 *                           distr_cache.rs:61-92); windows 0 and 1 are the two trivial ones (assgn.rs:72-77)
 *   depth_contrib, aln_contrib   assgn.rs:24-25, 80-81
 *   wshifts[n_contigs + 1]  GenotypeWindows::wshifts (windows.rs:709-739), optional (n_contigs 0): only the exact solver looks
 *                           at it, for the order of its search
 * rng_state: the four words of the caller's XoshiroRng (xoshiro256++, ext/rand.rs:3). With non-trivial reads the call draws ONE
 * next_u64 from it — the chain's seed, as lcty_solve_stage takes one seed per chain; the chain is then that of lcty_solve_stage for
 * this seed (DESIGN.md §2 lists the adaptors) — and leaves the state advanced by that draw. A genotype without non-trivial reads has
 * one assignment (Solver::solve, mod.rs:64-66): the generator is not touched (rng_state may be NULL).
 * Outputs: read_assgn[n_reads] (ReadAssignment::read_assgn), lik_parts = {aln_lik, depth_lik} (optional), *likelihood =
 * depth_contrib * depth_lik + aln_contrib * aln_lik (ReadAssignment::likelihood, assgn.rs:235-237; optional).
 * Re-entrant: any number of host threads may call it at once on one locus (the Solver contract: `&self` shared by the worker
 * threads, solve.rs:254-257, 1010-1017); every call in flight has its own stream and chain state. Limits of the device solver:
 * < 2^24 read pairs, <= 255 locations per read pair (LCTY_ERR_UNSUPPORTED beyond; the reference asserts <= 65 535, assgn.rs:58).
 * LCTY_ERR_SOLVER as `Error::Solver` (err.rs:14): the exact solver without a proof inside its node limit (highs.rs:113-116). */
typedef struct lcty_gt_alns_view {
    uint64_t n_reads;
    const uint64_t* read_ixs;
    const double*   ln_prob;
    const uint32_t* windows;
    uint32_t n_windows;
    uint32_t n_contigs;
    const uint8_t*  window_gc;
    const double*   window_weight;
    const uint32_t* wshifts;
    double depth_contrib, aln_contrib;
} lcty_gt_alns_view;
int32_t lcty_solve_given(lcty_locus* locus, const lcty_gt_alns_view* gt_alns, const lcty_solver* solver, uint64_t* rng_state,
                         uint16_t* read_assgn, double* lik_parts, double* likelihood);
/* The same call for a caller that holds the window distributions itself and no lcty_locus — which is what `Solver::solve` is
 * handed: the WindowDistr of every window carries its cached distribution (Arc<LinearCache<BayesCalc<..>>>, distr_cache.rs:17-25), at
 * most one per GC bin. `tables`: values[n_rows][width] = DiscretePmf::ln_pmf(depth) of row's distribution for depth 0 .. width - 1
 * (LinearCache::ln_pmf, lincache.rs:41-48: cached below 256, evaluated beyond); window_gc[w] then names the ROW of window w. width
 * must exceed what lcty_gt_alns_deepest reports for the object: the number of locations that name the fullest window with a
 * distribution (no assignment can make a window deeper). id != 0: a table the slot already holds under this id, width and row count
 * is not uploaded again (the rows of a locus do not change between the attempts of its genotypes). n_rows <= 128. */
typedef struct lcty_depth_tables {
    uint32_t n_rows, width;
    const double* values;
    uint64_t id;
} lcty_depth_tables;
int32_t lcty_gt_alns_deepest(const lcty_gt_alns_view* gt_alns, uint32_t* deepest);
int32_t lcty_solve_given_tables(lcty_ctx* ctx, const lcty_gt_alns_view* gt_alns, const lcty_depth_tables* tables, const lcty_solver* solver,
                                uint64_t* rng_state, uint16_t* read_assgn, double* lik_parts, double* likelihood);
/* XoshiroRng::seed_from_u64 (ext/rand.rs:3-22) into four words / next_u64 on them: for a caller whose generator keeps its state
 * private (rand_xoshiro without serde): `lcty_rng_seed_from_u64(rng.next_u64(), state)` starts a stream for the solver calls */
int32_t lcty_rng_seed_from_u64(uint64_t seed, uint64_t* state);
int32_t lcty_rng_next_u64(uint64_t* state, uint64_t* out);
/* Per-read assignment counts of ONE genotype over `attempts` chains — the "per-read posteriors" behind the output BAMs
 * (GenotypeAlignments::create_counts + ReadAssignment::update_counts, assgn.rs:94-96, 374-378; solve.rs:821-836;
 * model/bam.rs divides by `attempts`). read_off[n_good + 1]: first count of every good read pair, its possible
 * locations on the genotype in extend_read_gt_alns order (windows.rs:762-797); counts[read_off[n_good]] (u16 as in the
 * reference). counts == NULL: only read_off / *n_counts are produced. The chains are the ones lcty_solve_stage runs
 * for the same genotype, solver and seeds. */
int32_t lcty_assignment_counts(lcty_reads* reads, const uint16_t* genotype, uint32_t ploidy, const lcty_solver* solver,
                               uint32_t attempts, const uint64_t* chain_seeds, uint64_t* read_off, uint16_t* counts, uint64_t cap,
                               uint64_t* n_counts);
/* Genotyping::count_unexplained_reads (solve.rs:718-729): good read pairs whose best alignment on the alleles of the
 * called genotype is no better than "both mates unmapped" (+1e-8). */
int32_t lcty_count_unexplained(lcty_reads* reads, const uint16_t* genotype, uint32_t ploidy, uint32_t* out);
/* Genotyping::{find_weighted_dist, check_first_prob, check_num_of_reads} (solve.rs:621-675). genotypes[n][ploidy] and
 * ln_probs[n] as produced by lcty_produce_result (best first); dist: optional n_alleles x n_alleles matrix of contig distances
 * (symmetric, LCTY_NONE_U32 = unknown; `contig_distances`, solve.rs:974-976). distances_out[n] (LCTY_NONE_U32 = None),
 * *weighted_dist (NaN = None), *warnings = LCTY_WARN_* bits. Host only. */
#define LCTY_WARN_NO_PROBABLE_GENOTYPE 1u
#define LCTY_WARN_FEW_READS            2u
int32_t lcty_call_checks(const uint16_t* genotypes, uint64_t n, uint32_t ploidy, const double* ln_probs, uint32_t n_reads,
                         const uint32_t* dist, uint32_t n_alleles, uint32_t* distances_out, double* weighted_dist, uint32_t* warnings);
/* ---- the whole genotyping of one locus: solve::solve (src/solvers/solve.rs:926-981) ---------------------------------
 * Scheme = list of stages (Stage, solve.rs:138-171; default "-S greedy:i=5k,a=1 -S anneal:i=20,a=20", 211-230). The call:
 * all genotypes of `ploidy` (generate_genotypes) with optional priors -> run_filter + truncate_ixs when the first stage
 * takes fewer genotypes than there are (or dont_skip) -> every stage (skipped when the survivors already fit the next
 * stage, 805-809) + discard_improbable_genotypes -> produce_result -> count_unexplained_reads / check_first_prob /
 * check_num_of_reads. Chain seeds of stage s: lcty_chain_seeds(master_seed + (s + 1) * 0x9e3779b97f4a7c15, n * attempts).
 * lik_mean / lik_var / attempts_out (optional, [G]): NaN / 0 for genotypes that were never solved. */
typedef struct lcty_stage {
    lcty_solver solver;
    uint64_t in_size;       /* genotypes this stage takes (Stage::in_size) */
    uint32_t attempts;      /* chains per genotype */
    uint32_t _pad0;
} lcty_stage;
#define LCTY_MAX_RESULT 50  /* MAX_GENOTYPES of produce_result (solve.rs:485) */
typedef struct lcty_call {
    uint64_t n_out;                       /* genotypes reported, best first */
    uint64_t ixs[LCTY_MAX_RESULT];        /* indices into generate_genotypes order */
    double   ln_probs[LCTY_MAX_RESULT];
    double   quality;                     /* Phred of "the call is wrong", capped at 1e9 */
    uint32_t unexpl_reads;                /* count_unexplained_reads of the call */
    uint32_t warnings;                    /* LCTY_WARN_* */
    uint64_t n_good;                      /* read pairs used */
    uint64_t kept_after_filter;           /* genotypes after run_filter (= all when it was skipped) */
} lcty_call;
int32_t lcty_stages_default(lcty_stage* stages /* [2] */, uint32_t* n_stages);
int32_t lcty_solve(lcty_reads* reads, uint32_t ploidy, const lcty_stage* stages, uint32_t n_stages, uint64_t master_seed,
                   const double* priors, lcty_call* out, double* lik_mean, double* lik_var, uint32_t* attempts_out);
/* The loop of `locityper genotype` over its loci (analyze_locus one after the other, command/genotype.rs:1331-1351) as a queue on one
 * GPU: for every entry lcty_score_reads + lcty_solve. Loci are independent, so the last stage of entry i (by default the annealing
 * attempts: a few hundred long serial chains on a few per cent of the device) runs on a second stream of the context, from a second
 * host thread, while entry i + 1 is greedily solved — and what comes before the chains of entry i + 2 (its scores, run_filter, the cut,
 * the location table) is issued on a third stream, by a third host thread, as soon as the last stage of entry i has ended, beside the
 * greedy chains of entry i + 1 (knob "queue_early_head" 0: on the main stream after those chains).
 * out[i] equals what lcty_solve gives for entry i alone.
 * All batches share one context; neighbours in the queue are different batches of different lcty_locus objects (a batch may come
 * again later in the queue: it is scored again). master_seeds[n_batches]; priors NULL or [n_batches] pointers (NULL = no priors). */
int32_t lcty_solve_queue(lcty_reads* const* batches, uint32_t n_batches, uint32_t ploidy, const lcty_stage* stages, uint32_t n_stages,
                         const uint64_t* master_seeds, const double* const* priors, lcty_call* out);
/* The same queue fed one batch at a time, for loci that are not all resident: `acquire(user, i)` is called right before position i is
 * scored and returns its batch (NULL: the queue ends with LCTY_ERR_INVALID_INPUT) — typically filled by another host thread, with
 * lcty_reads_append* on page-locked chunks (their copies have a stream of their own), while position i - 1 is being solved;
 * `release(user, i)` (may be NULL) when the last stage of position i is done and nothing of its batch is in use: lcty_reads_reset can
 * then bind the object to the locus of a later position. Position i is released before position i + 3 is acquired, so three batch
 * objects carry a queue of any length. `acquire(user, i)` for i > 0 comes from a thread of the library, while position i - 1 is in its
 * chains and once the last stage of position i - 2 has ended (the head of position i is made there: lcty_solve_queue), and may run at
 * the same time as a `release` on the caller's thread; with knob "queue_early_head" 0 both come from the caller's thread, `acquire(i)`
 * after the chains of position i - 1 and after `release(i - 2)`. On an error every position that was acquired and not yet released is
 * released before the call returns, with nothing of the queue left in flight on the device. The loading of locus i + 1 next to
 * analyze_locus of locus i (genotype.rs:1331-1351). */
typedef lcty_reads* (*lcty_queue_acquire_fn)(void* user, uint32_t position);
typedef void (*lcty_queue_release_fn)(void* user, uint32_t position);
int32_t lcty_solve_queue_fed(uint32_t n_loci, lcty_queue_acquire_fn acquire, lcty_queue_release_fn release, void* user, uint32_t ploidy,
                             const lcty_stage* stages, uint32_t n_stages, const uint64_t* master_seeds, const double* const* priors,
                             lcty_call* out);

/* Diagnostics of the last lcty_solve_stage on this batch: chains run, solver iterations (greedy iterations /
 * annealing moves) and accepted moves summed over the chains (stoch.rs has no counterpart; used by bench.py). */
int32_t lcty_solve_stats(const lcty_reads* reads, uint64_t* chains, uint64_t* iterations, uint64_t* accepted);
/* Predictions::discard_improbable_genotypes (solve.rs:425-480): ixs in/out */
int32_t lcty_discard_improbable(const double* lik_mean, const double* lik_var, const uint32_t* attempts, uint64_t* ixs, uint64_t n,
                                double prob_thresh, uint64_t out_size, uint64_t threads, uint64_t* n_keep);
/* Predictions::produce_result (solve.rs:482-535): out arrays sized >= min(n, 50) */
int32_t lcty_produce_result(const double* lik_mean, const double* lik_var, const uint32_t* attempts, const uint64_t* ixs, uint64_t n,
                            double prob_thresh, uint64_t out_bams, uint64_t* out_ixs, double* out_ln_probs, uint64_t* n_out,
                            double* quality);

/* ---- measurement hooks (bench.py) -----------------------------------------
 * HIP-event timing of the launches issued between begin/end on the context's
 * stream; kernel ids LCTY_K_*.                                                 */
#define LCTY_K_SCORE     0
#define LCTY_K_PREFILTER 1
#define LCTY_K_SOLVE     2   /* greedy_loop_kernel: the Greedy chains */
#define LCTY_K_SOLVE_INIT  3 /* solve_init_tile_kernel / solve_init_kernel: apply_tweak + ReadAssignment::try_new of every chain of a greedy (or exact) stage, its records */
#define LCTY_K_SOLVE_TABLE 4 /* build_loc_table_kernel: allele-major location table of a scored batch */
#define LCTY_K_TRANSFER  5   /* transfer_kernel: alignment recovery */
#define LCTY_K_RECRUIT   6   /* recruit_kernel: minimizer read recruitment */
#define LCTY_K_ANNEAL    7   /* anneal_loop_kernel: the SimAnneal chains */
#define LCTY_K_MAP       8   /* map_kernel: candidate generation on the basis alleles */
#define LCTY_K_SOLVE_INIT_ANNEAL 9 /* the same for the chains of an annealing stage (a few hundred: a launch of its own size, timed apart) */
#define LCTY_K_COUNT     10
/* Timing is opt-in: nothing is recorded before the first lcty_timing_reset on a context (a production run that never reads
 * timings creates no events); afterwards every launch is bracketed by two events, at most 256 pairs per kernel id kept. */
int32_t lcty_timing_reset(lcty_ctx* ctx);
int32_t lcty_timing_get(lcty_ctx* ctx, int32_t kernel, uint64_t* launches, double* total_ms);

/* ---- file formats at the edges of the path (host code, no device) --------------------------------------------
 * lcty_io_read_file: the whole file with its container removed, chosen by the extension as ext::sys::open does: .gz / .bgz / .bam
 *   gzip members (zlib), .lz4 LZ4 frames, .br brotli streams one after the other (src/ext/sys/brotli.rs:18-86; needs the system's
 *   libbrotlidec.so.1, LCTY_ERR_UNSUPPORTED without it), anything else as it is. *data is released with lcty_io_free.
 *   `kmers.bin.br` / `.lz4` (command/paths.rs:4-5) -> lcty_io_read_file -> lcty_kmer_counts_parse.
 * lcty_io_write_gz: ext::sys::create_gzip + write.
 * lcty_io_write_br: the brotli writer behind `sol.csv.br`, `reads.csv.br` and the other --debug tables (solvers/solve.rs:937-938,
 *   model/locs.rs:1062-1065): a brotli stream (RFC 7932) of `data` — compressed at `quality` 0..11 by the system's libbrotlienc.so.1
 *   (looked up at run time), or, without that library or with quality < 0, STORED in uncompressed meta-blocks (a valid stream any
 *   brotli reader takes, the reference's included; *stored = 1 then).
 * lcty_bg_from_json: BgDistr::load (src/bg/mod.rs:159-177) on the text of PREPROC/distr.gz: seq_info (349-364), insert_distr
 *   ({} = single-end, bg/insertsz.rs:195-208), error_profile (bg/err_prof.rs:321-329), bg_depth (bg/depth.rs:400-412; required, as
 *   `locityper genotype` requires it); edit thresholds = EditThresh::default_for (err_prof.rs:394-399). Missing keys / wrong types
 *   -> LCTY_ERR_INVALID_DATA (Error::JsonLoad).
 * lcty_res_to_json: Genotyping::to_json (src/solvers/solve.rs:732-773) in the layout of write_pretty(.., 4) (genotype.rs:1256):
 *   total_reads, quality, [dist_type, weight_dist], unexpl_reads, genotype, options[{genotype, lik_mean, lik_sd, prob, log10_prob,
 *   [dist_to_primary]}], [warnings]; lik_sd is the log10-scaled VARIANCE, as upstream (solve.rs:755). genotypes[n_out][ploidy],
 *   lik_mean / lik_var[n_out] in the order of call->ixs. Two calls: out = NULL sizes it (*needed includes the final 0). */
int32_t lcty_io_read_file(const char* path, uint8_t** data, uint64_t* len);
void    lcty_io_free(void* p);
int32_t lcty_io_write_gz(const char* path, const uint8_t* data, uint64_t len);
int32_t lcty_io_write_br(const char* path, const uint8_t* data, uint64_t len, int32_t quality, int32_t* stored);
int32_t lcty_bg_from_json(const char* json, uint64_t len, lcty_bg* bg, double* read_len);
int32_t lcty_res_to_json(const lcty_call* call, const uint16_t* genotypes, uint32_t ploidy, const char* const* names, uint32_t n_alleles,
                         const double* lik_mean, const double* lik_var, const uint32_t* distances, int32_t true_edit_distances,
                         double weighted_dist, char* out, uint64_t cap, uint64_t* needed);
/* write_bam (src/model/bam.rs:356-413): the alignments of the batch's read pairs to the contigs of ONE genotype as a coordinate-sorted
 * BAM file (path) and its BAI index (path + ".bai"). For every used read pair (status GOOD) the locations of the pair on the genotype
 * (extend_read_gt_alns, model/windows.rs:762-797) are folded by (alignment of mate 1, alignment of mate 2) with their assignment counts
 * (count_alignments, bam.rs:144-176) — read_off / counts exactly as lcty_assignment_counts returned them for THIS genotype and
 * `attempts` —, one record (pair) per fold: MAPQ and pr from the counts (count_to_prob, 56-67), the fold with most counts primary,
 * the others secondary; read pairs with few unique k-mers (status FEW_KMERS) follow with us:F (268-298, 328-353). Tags NM, il, al, uk,
 * pr, us as bam.rs:123-141; flags, mate fields and insert sizes as connect_pair / calc_insert_size (69-86, 178-221).
 *   table        the caller's copy of what was appended to the batch (records, CIGARs, packed sequences)
 *   name_off     [n_pairs + 1] into names; qual_off [2 * n_pairs + 1] into quals (NULL: qualities 255), both as in the primary
 *                record of each mate (lcty_bam_table_view hands them out for an aln.bam)
 * Not after lcty_recover_alignments (the transferred alignments are not in the caller's table) and not for counted batches:
 * LCTY_ERR_UNSUPPORTED. *n_records (may be NULL): records written. */
int32_t lcty_write_bam(const char* path, lcty_reads* reads, const lcty_reads_host* table, const uint64_t* name_off, const char* names,
                       const uint64_t* qual_off, const uint8_t* quals, const char* const* allele_names, const uint16_t* genotype,
                       uint32_t ploidy, uint16_t attempts, const uint64_t* read_off, const uint16_t* counts, uint64_t* n_records);

/* OUT/loci/<locus>/aln.bam -> the flat table of lcty_reads_append, grouped as AllAlignments::load walks the records
 * (src/model/locs.rs:405-461, 502-567, 1116-1150): a group = a primary record + the non-primary records behind it; the first group
 * of a read is its first end, with paired != 0 the next group (same name, else LCTY_ERR_INVALID_DATA as ReadData::set_name,
 * 147-155) its second. Reference names map to allele indices through names[n_alleles] (construct_tid_to_contig_map, 388-401).
 * lcty_bam_table_view: the table (valid while the handle lives), read names (name_off[n_pairs + 1] into name_blob) and the number
 * of reference sequences of the header (fewer than alleles: set lcty_params.strict_subset, locs.rs:486). */
typedef struct lcty_bam_table lcty_bam_table;
int32_t lcty_bam_read(const char* path, const char* const* names, uint32_t n_alleles, int32_t paired, lcty_bam_table** out);
int32_t lcty_bam_table_view(const lcty_bam_table* t, lcty_reads_host* view, const uint64_t** name_off, const char** name_blob, uint32_t* n_refs);
void    lcty_bam_table_free(lcty_bam_table* t);
/* The same file read on the device (src/model/locs.rs:405-461, 502-567, 1116-1150, as lcty_bam_read): the file is inflated into one
 * slice (host pool, or the device with knob "sample_bam_inflate" 1), the header is parsed and the record lengths are walked on the
 * host, everything else — fields, grouping, offsets, CIGAR words, names, qualities, bases — is made by kernels and stays resident on
 * ctx's device with the handle. host_copy != 0: everything is downloaded once and lcty_bam_table_view gives the view lcty_bam_read
 * gives for the file, word for word. host_copy == 0: only the per-pair arrays (mate_len, mate_off, aln_off, cigar_off, names) come
 * back; lcty_bam_table_view then fails with LCTY_ERR_INVALID_INPUT. Errors: status and text of lcty_bam_read for the same file.
 * A slice above knob "aln_bam_max_slice_bytes" (default 2^33), or 2^31 - 16 or more records, CIGAR words or 32-base units:
 * LCTY_ERR_UNSUPPORTED. stats (may be NULL): sizes and the milliseconds of every stage. */
typedef struct lcty_aln_bam_stats {
    uint64_t bytes_read, bytes_inflated, blocks, records, pairs, bases, cigar_words;
    double ms_read, ms_inflate, ms_walk, ms_record, ms_gather, ms_unpack, ms_download, ms_total;
} lcty_aln_bam_stats;
int32_t lcty_bam_read_device(lcty_ctx* ctx, const char* path, const char* const* names, uint32_t n_alleles, int32_t paired,
                             int32_t host_copy, lcty_bam_table** out, lcty_aln_bam_stats* stats);
/* What lcty_reads_create needs for the table of either reader (locs.rs:1116-1150): pairs, bases (mate_off[2 n_pairs]), records,
 * CIGAR words, and the reference sequences of the header. Every output may be NULL. */
int32_t lcty_bam_table_sizes(const lcty_bam_table* t, uint64_t* n_pairs, uint64_t* n_bases, uint64_t* n_recs, uint64_t* n_cigar,
                             uint32_t* n_refs);
/* What the handle of either reader holds and the view does not show (locs.rs:1116-1150 reads neither): qual_off[2 n_pairs + 1] into
 * quals, the qualities of every mate as its primary record stores them (0xFF: absent), and mapq[n_recs]. A device handle needs
 * host_copy: LCTY_ERR_INVALID_INPUT otherwise. Every output may be NULL. */
int32_t lcty_bam_table_quals(const lcty_bam_table* t, const uint64_t** qual_off, const uint8_t** quals, const uint8_t** mapq);
/* Pairs [first_pair, first_pair + n_pairs) of a handle of lcty_bam_read_device appended to a batch of the same context, as
 * lcty_reads_append of the host view's sub-chunk would (locs.rs:502-567, 1116-1150): records, CIGAR words, bases and nmask go device to
 * device, the host builds the rebased offsets of the range only. Another context, a handle of lcty_bam_read or a range outside the
 * table: LCTY_ERR_INVALID_INPUT. */
int32_t lcty_reads_append_bam(lcty_reads* reads, const lcty_bam_table* t, uint64_t first_pair, uint64_t n_pairs);
/* DB/loci/<locus>/haplotypes.fa[.gz] (ContigSet::load, src/seq/contigs.rs:295-306): names up to the first blank (0-separated in
 * `names`), upper-cased sequences concatenated, seq_off[n_seqs + 1]. Called twice: with names = seqs = seq_off = NULL it returns the sizes. */
int32_t lcty_fasta_read(const char* path, uint32_t* n_seqs, char* names, uint64_t* names_len, uint8_t* seqs, uint64_t* seqs_len, uint64_t* seq_off);
/* DB/loci/<locus>/haplotypes.paf[.gz|.br|.lz4] as process_paf reads it (src/command/genotype.rs:1131-1160; PafFile::next and
 * PafEntry::parse, src/seq/paf.rs:31-56, 103-144): the entries lcty_locus_set_hap_alns takes, in file order. names[n_alleles]: the
 * contig names of the locus (their order gives the ids). Left out, as there: empty and '#' lines, lines naming a contig the locus
 * does not have, self-alignments, entries without a cg:Z: tag, entries that do not cover both sequences on the forward strand
 * (HapAlns::add, src/seq/transfer.rs:48-52). Malformed lines are errors, as there. Called twice: id1 = NULL sizes it
 * (*n_entries, *n_cigar); with buffers, *n_entries / *n_cigar carry their capacities in. cigar_off[n_entries + 1]. */
int32_t lcty_paf_read(const char* path, const char* const* names, uint32_t n_alleles, uint64_t* n_entries, uint32_t* id1, uint32_t* id2,
                      uint32_t* n_matches, uint32_t* aln_len, uint64_t* cigar_off, uint32_t* cigar, uint64_t* n_cigar,
                      uint32_t* dist /* NULL or [n_alleles x n_alleles]: contig_distances (genotype.rs:1139-1150), the edit distance
                                        aln_len - n_matches of every entry with a CIGAR between two different contigs of the locus,
                                        symmetric, LCTY_NONE_U32 where the file has none: the `dist` of lcty_call_checks, "edit" */);
/* DB/loci/<locus>/distances.bin (load_divergences_and_convert, src/seq/minim_div.rs:126-149; read when there is no PAF,
 * genotype.rs:1229-1237): u8 k, u8 w, varint n (= n_alleles or LCTY_ERR_INVALID_DATA), then the non-shared minimizers of the pairs
 * i < j row by row. dist[n_alleles x n_alleles]: symmetric, LCTY_NONE_U32 on the diagonal: the `dist` of lcty_call_checks, "minim-div". */
int32_t lcty_distances_parse(const uint8_t* buf, uint64_t len, uint32_t n_alleles, uint32_t* k, uint32_t* w, uint32_t* dist);

/* ---- background distributions of a sample (locityper preproc, existing alignments + a background region) ------------------------
 * estimate_bg_distrs (src/command/preproc.rs:1157-1192) with `-a`: the alignments of ONE background interval [start, end) of one
 * contig, read sequentially from a BAM file that holds them (a slice of the sample's BAM) or fetched through the index of the
 * sample's whole BAM file (lcty_bg_reads_fetch; no CRAM), the reference
 * sequence of the interval +- 50 kb (BgRegion::new, preproc.rs:1357-1385) and the k-mer counts of that padded sequence (what
 * `jellyfish query` returns for it; the caller runs jellyfish). Out of scope: mapping reads (run_mapping, 918), --similar-dataset
 * (estimate_like, 1293), input subsampling (only the rate enters the depth fit), the region-less OpCounter::Unbounded path.
 *
 * lcty_bg_reads_load: IndexedReader::fetch (records of `contig` overlapping [start, end), file order) + load_alns (preproc.rs:988-1028):
 *   flags & 3844 == 0, MAPQ >= min_mapq, clipping_rate <= max_clipping (seq/cigar.rs:944-966; first and last op that consume no
 *   reference, a one-op CIGAR twice, over SEQ length); records whose extended CIGAR cannot be inferred from the padded sequence (an
 *   M run starting before it or ending at or past its end, cigar.rs:446-448) are dropped and counted. Mates by read name
 *   (group_mates, bg/insertsz.rs:25-37). Errors (LCTY_ERR_INVALID_DATA): paired and unpaired records mixed, no records, a read with
 *   two first (second) mates, SEQ length != CIGAR query length (the reference panics), an op other than M I D S = X (H, N, P: the
 *   reference panics in count_region_operations). Paired-end data with a technology other than Illumina -> LCTY_ERR_INVALID_INPUT.
 * lcty_bg_reads_fetch: the same records and the same answer from the sample's whole, coordinate-sorted, indexed BAM file
 *   (lcty_sample_bam_open): IndexedReader::fetch (preproc.rs:1174-1192) through the BAI index, load_alns (988-1028) and group_mates
 *   (bg/insertsz.rs:25-37) on the device. The records read are those of lcty_sample_bam_fetch's front half for the one region
 *   (tid of contig, start, end) without the unmapped tail: the chunks of the index, pread, the BGZF split, the inflate (knob
 *   "sample_bam_inflate"), the host walk of record lengths. The view of the handle equals, field for field and word for word, the
 *   one lcty_bg_reads_load gives for a file of the same records, and so do the status and the read an error names (the first
 *   offending record in file order; a mapped record without a CIGAR is named here too). Beyond lcty_bg_reads_load, as
 *   lcty_sample_bam_fetch: a record that leaves the fetched slice or is shorter than its fields, and (tid, pos) running backwards
 *   inside the slice: LCTY_ERR_INVALID_DATA; a slice above "sample_bam_max_slice_bytes", 2^31 records or CIGAR operations or more:
 *   LCTY_ERR_UNSUPPORTED. A contig that is not in the header, an interval outside the padded sequence: LCTY_ERR_INVALID_INPUT.
 *   "sample_bam_hash_bits" keeps that many bits of the hash of a read name (names are always compared in full). The arrays of the
 *   view are downloaded once and belong to the handle, which also keeps them on the device of `ctx`: lcty_bg_estimate on the same
 *   context reads them there (no upload; the results are bit-identical either way). The handle must be freed before its context.
 *   stats (may be NULL) as lcty_sample_bam_fetch fills it: ms_record the record stage with its scans, ms_pair the mates, ms_unpack
 *   the CIGAR gather, the base unpack and the downloads; records_kept = n_records, n_pairs the full pairs, n_discarded 0.
 * lcty_bg_estimate: estimate_bg_from_paired / _unpaired (preproc.rs:1065-1155) -> lcty_bg + the mean read length (read_len_from_alns,
 *   1031-1037; SequencingInfo::new 304-322: out of the technology's range -> LCTY_ERR_INVALID_INPUT unless explicit_technology).
 *   padded_seq: upper-case A/C/G/T only (JfKmerGetter::fetch refuses Ns, seq/counts.rs:326-327: LCTY_ERR_INVALID_INPUT);
 *   kmer_counts[padded_len + 1 - k]: the counts of every k-mer of padded_seq, already clamped (KmerCounts::subregion, 234-246 takes
 *   the interval's part). Errors as the reference: < 1000 pairs / FF-RR orientation / match probability <= 0.5 -> INVALID_DATA,
 *   zero kept windows -> RUNTIME. Integer work on the device; fits on the host (what is exact, what is a tolerance).
 * lcty_bg_diag: the --debug intermediates. lcty_bg_diag_sizes gives n_windows, n_records, n_pairs; hist_* need n_pairs entries,
 *   edit_* n_records (upper bounds: n_hist / n_edit say how many were written). Any array may be NULL.
 * lcty_bg_to_json: BgDistr::save (bg/mod.rs:147-158) as text, total_reads / file_size null; doubles in the shortest form that reads
 *   back bit-exact; `ploidy` is bg_depth.ploidy (lcty_bg does not carry it). Two calls: out = NULL sizes it (*needed includes the final 0). */
typedef struct lcty_bg_params {
    int32_t  technology;          /* LCTY_TECH_* */
    int32_t  explicit_technology; /* 1: a read length outside the technology's range is a warning, not an error (bg/mod.rs:304-322) */
    uint32_t min_mapq;            /* 30 (preproc.rs:275) */
    uint32_t ploidy;              /* 2 (bg/depth.rs:172) */
    double   max_clipping;        /* 0.02 (preproc.rs:294) */
    double   insert_pval;         /* 0.001 (bg/mod.rs:39-46) */
    double   edit_pval;           /* 0.01 */
    uint32_t window_size;         /* 0 = auto: clamp(round(2/3 read length), 20, 5000) (bg/windows.rs:103-109) */
    uint32_t boundary_size;       /* 1000 */
    double   uniq_kmer_perc;      /* 90 */
    double   frac_windows;        /* 0.5 */
    uint32_t min_tail_obs;        /* 100 */
    uint32_t _pad0;
    double   tail_var_mult;       /* 0.02 */
    double   subsampling_rate;    /* 1.0 */
} lcty_bg_params;

typedef struct lcty_bg_reads lcty_bg_reads;
#define LCTY_BG_REVERSE 1u          /* lcty_bg_reads_view.flags */
#define LCTY_BG_SECOND  2u          /* ReadEnd::Second (BAM flag 0x80) */
typedef struct lcty_bg_reads_view {
    uint64_t n_records;           /* kept records (file order) */
    uint64_t n_ignored;           /* failed flags / MAPQ / clipping */
    uint64_t n_wo_cigar;          /* no extended CIGAR (outside the padded sequence) */
    int32_t  paired;
    uint32_t _pad0;
    double   read_len;            /* mean query length of the first 10 000 kept records */
    const uint32_t* pos;          /* [n] 0-based start */
    const uint32_t* end;          /* [n] start + reference length */
    const uint32_t* qlen;         /* [n] query length */
    const uint8_t*  flags;        /* [n] LCTY_BG_* */
    const uint32_t* mate;         /* [n] index of the other end of a full pair, LCTY_NONE_U32 without one */
    const uint64_t* cigar_off;    /* [n + 1] */
    const uint32_t* cigar;        /* raw BAM CIGAR words */
    const uint64_t* seq_off;      /* [n + 1] base offsets, multiples of 32; bases2 / nmask as lcty_reads_host */
    const uint32_t* bases2;
    const uint32_t* nmask;
} lcty_bg_reads_view;

typedef struct lcty_bg_diag {
    uint64_t n_windows, n_records, n_pairs, n_hist, n_edit;   /* n_hist / n_edit: written by lcty_bg_estimate */
    /* per window [n_windows] (filter_windows, bg/windows.rs:44-101; count_reads, depth.rs:27-39) */
    uint32_t* win_start; double* win_gc; double* win_kmer_frac; uint8_t* win_keep; uint32_t* win_depth /* [2 n_windows] */;
    /* per record [n_records] (count_region_operations, seq/aln.rs:241-281; edit_distance, err_prof.rs:73-79) */
    uint32_t* rec_counts /* [5 n_records] =, X, I, D, S */; uint32_t* rec_edit; uint32_t* rec_read_len; uint32_t* rec_middle;
    uint32_t* rec_window /* LCTY_NONE_U32 outside */;
    /* per pair [n_pairs]: the pairs in order of their first end, insert size and FF/RR (seq/aln.rs:223-233) */
    uint32_t* pair_first; uint32_t* pair_second; uint32_t* pair_insert; uint8_t* pair_same_strand;
    /* insert sizes (InsertDistr::estimate, insertsz.rs:67-143) */
    uint32_t* hist_size; uint32_t* hist_count;               /* [n_hist] ascending size, inserts < 500 000 */
    uint64_t orient[2];                                      /* FR/RF, FF/RR */
    double   ins_limit, ins_mean, ins_var;                   /* 3 x q0.99, mean / variance of the inserts <= limit */
    uint32_t ci_low, ci_high;                                /* confidence_interval(1 - insert_pval) */
    /* error profile (ErrorProfile::estimate, err_prof.rs:152-197) */
    uint64_t op_totals[5];
    uint32_t* edit_edit; uint32_t* edit_len; uint64_t* edit_count;   /* [n_edit] ascending (edit, read_len) */
    double   unif_coef;
    /* records / pairs entering each stage: 0 loaded records, 1 pairs, 2 pairs in the histogram, 3 error-profile records,
     * 4 of them in kept windows, 5 depth records (edit-filtered) */
    uint64_t n_stage[6];
    /* depth (ReadDepth::estimate, depth.rs:300-345) per GC bin */
    uint32_t gc_nwin[LCTY_GC_BINS];
    double   loess_mean[LCTY_GC_BINS], loess_var[LCTY_GC_BINS], blur_mean[LCTY_GC_BINS], blur_var[LCTY_GC_BINS];
    double   nb_n[LCTY_GC_BINS], nb_p[LCTY_GC_BINS];
    double   depth_mean, depth_var;                          /* technologies without GC bias: the one mean / variance */
    /* timing of this call: device time of windows / counts / pairs / depth kernels (events), host fits, whole call (ms) */
    double   kernel_ms[4], fit_ms, total_ms;
} lcty_bg_diag;

void    lcty_bg_params_default(lcty_bg_params* params);
int32_t lcty_bg_reads_load(const char* path, const char* contig, uint32_t start, uint32_t end, uint32_t padded_start, uint32_t padded_len,
                           const lcty_bg_params* params, lcty_bg_reads** out);
int32_t lcty_bg_reads_fetch(lcty_ctx* ctx, lcty_sample_bam* bam, const char* contig, uint32_t start, uint32_t end,
                            uint32_t padded_start, uint32_t padded_len, const lcty_bg_params* params,
                            lcty_bg_reads** out, lcty_sample_bam_stats* stats /* may be NULL */);
int32_t lcty_bg_reads_view_get(const lcty_bg_reads* reads, lcty_bg_reads_view* view);
void    lcty_bg_reads_free(lcty_bg_reads* reads);
int32_t lcty_bg_diag_sizes(const lcty_bg_reads* reads, uint32_t region_start, uint32_t region_end, const lcty_bg_params* params,
                           uint64_t* n_windows, uint64_t* n_records, uint64_t* n_pairs);
int32_t lcty_bg_estimate(lcty_ctx* ctx, const lcty_bg_reads* reads, const uint8_t* padded_seq, uint32_t padded_start, uint32_t padded_len,
                         const uint16_t* kmer_counts, uint32_t k, uint32_t region_start, uint32_t region_end, const lcty_bg_params* params,
                         lcty_bg* out, double* read_len, lcty_bg_diag* diag /* may be NULL */);
int32_t lcty_bg_to_json(const lcty_bg* bg, double read_len, uint32_t ploidy, char* out, uint64_t cap, uint64_t* needed);

/* ---- locus database build (locityper target: the files of DB/loci/<locus>/) -----------------------------------------------------
 * process_alleles (src/command/add.rs:585-652) and what it calls, on buffers: the haplotype sequences of one locus, the reference
 * sequence of the locus and the k-mer counts `jellyfish query` returned for all of them (the caller runs Jellyfish, exactly as the
 * caller runs the mapper for aln.bam). Out of scope: lock and `success` files, augment. (From a pangenome VCF — reconstruction, locus
 * expansion, ref.bed: lcty_db_locus_from_vcf; haplotypes.paf.gz: lcty_align_haplotypes; prune: lcty_db_prune_locus, all further down.)
 * Integer work throughout: every output equals the reference's bit for bit (the f64 divergence is one IEEE division of two u32).
 *
 * A HAPLOTYPE SET (n_seqs, seqs, seq_off), here and in every section below: the sequences back to back in seqs, sequence a at
 *   [seq_off[a], seq_off[a + 1]). seq_off[0] MUST BE 0 and the offsets ascend; seqs may be NULL only when no sequence has a base.
 *   Anything else is LCTY_ERR_INVALID_INPUT, as is a count below what the call needs. A sequence too long for the stage's kernels, or
 *   too many sequences, is LCTY_ERR_UNSUPPORTED: below 2^31 bases here, below 2^28 for the aligner, below 0x7FFFFFF0 and at most
 *   65 535 haplotypes for paf-vcf; prune has no bound. The offsets are checked before a base is read or sent to the device.
 *
 * lcty_db_minimizers: kmers::minimizers::<u64, _, NON_CANONICAL> + sort_unstable per sequence (src/seq/kmers.rs:265-331,
 *   src/seq/minim_div.rs:53-61): the sorted HASHES (fast_hash, kmers.rs:93-103) of the minimizers, one per minimizer position, so
 *   a list is a multiset. 1 <= k <= 32: the reference asserts k <= 31 in debug builds only; at 32 the mask is the whole word (the
 *   form the comment at kmers.rs:49 gives). 1 <= w <= 63: add.rs:101 lets 64 through, but the circular array of kmers.rs:205-236
 *   holds 64 hashes and the loop asserts w < 64 (kmers.rs:270), so 64 is LCTY_ERR_INVALID_INPUT. Sequences of ACGT take a parallel
 *   kernel (stats->n_fast); a sequence with any other byte — N, lower case: the reference matches the four capitals only — takes a
 *   one-lane walk that restates the loop with its first_kmer / first_window rules (stats->n_walk). min_off[n_seqs + 1];
 *   *hashes is released with lcty_io_free.
 * lcty_db_divergences: minimizer_divergences over all pairs (minim_div.rs:45-72; jaccard_distance, 16-40) in the order of
 *   TriangleMatrix::indices (src/ext/trimat.rs:15-17: rows i, then j > i): uniq[n (n - 1) / 2] the non-shared minimizers (what
 *   distances.bin holds), diverg (may be NULL) uniq / union as f64, NaN where both lists are empty, as the reference's 0 / 0.
 *   *check (may be NULL) is check_divergencies (add.rs:521-543): pairs with diverg >= 0.2, the highest value and its pair.
 *   Fewer than two sequences: LCTY_ERR_INVALID_DATA (add.rs:656-658). lcty_ctx_set_knob "db_chunk_cols" = columns of the bit
 *   matrix per pass (default: 1/8 of the free device memory, 256 MB at most); "host_threads" sorts lists longer than 8 192.
 * lcty_db_off_target: KmerCounts::off_target_counts (src/seq/counts.rs:180-230) with the preparation of add.rs:626-644: runs of
 *   N of ref_seq (n_runs, seq/mod.rs:57-74) count as A and the counts of the k-mers over them as 0. counts / cnt_off: the counts
 *   of the sequences' k-mers (cnt_off[a + 1] - cnt_off[a] == len(a) + 1 - k, and n_ref_counts == ref_len + 1 - k, else
 *   LCTY_ERR_INVALID_DATA as KmerCounts::validate, 159-172); counter_bytes (1..8) gives max_value = min(65535, 2^(8 bytes) - 1)
 *   (KmerCounts::load, 133). 2 <= k <= 63: 64-bit keys on the device up to 31, the 128-bit table on the host from 32.
 *   out[cnt_off[n_seqs]]. *warn_bits (may be NULL): LCTY_DB_WARN_*.
 * lcty_db_discard_identical: discard_identical (add.rs:546-582): the first of equal sequences is kept, order kept. names: n_seqs
 *   0-terminated names one after the other. kept[n_seqs] (the first *n_kept filled), owner[n_seqs] = input index of the kept
 *   haplotype an input equals (itself when kept); text = discarded_haplotypes.txt as lines 567-578 write it, *needed its length
 *   (0: nothing was discarded and the reference writes no file). kept, owner, text may be NULL.
 * lcty_kmer_counts_write: KmerCounts::save (counts.rs:108-124): u8 k, u8 counter bytes, varint contigs, per contig varint length
 *   + its counts as varints. A count above the counter's maximum: LCTY_ERR_INVALID_DATA. `kmers.bin.br` = the off-target block
 *   and the block of the counts as given, back to back (add.rs:648-650), through lcty_io_write_br.
 * lcty_distances_write: write_divergences (minim_div.rs:113-127): u8 k, u8 w, varint n, the triangle as varints. Not compressed.
 * lcty_fasta_write_text: write_multiline_fasta (src/seq/fastx.rs:27-43) per sequence: ">name", lines of 120 bases;
 *   `haplotypes.fa.gz` = this text through lcty_io_write_gz.
 *   The three writers are called twice: out = NULL sizes (*needed), then cap >= *needed.
 * lcty_db_build_locus: the sequence of process_alleles: discard_identical, FASTA text, [--calc-div: divergences -> distances.bin],
 *   off-target counts -> the two blocks of kmers.bin. counts / cnt_off[n_seqs + 2]: one block of n_seqs + 1 contigs, the reference
 *   sequence LAST (the order of add.rs:633-636). The reference counts k-mers after discard_identical; here the table covers every
 *   input haplotype: the blocks of discarded haplotypes are dropped. only_seqs (add.rs:606-609): counts, ref_seq may be NULL.
 *   The payloads come back uncompressed (the containers are the writers' business); release with lcty_db_files_free. */
#define LCTY_DB_WARN_NEGATIVES_SEEN 1u   /* have_negatives (counts.rs:203): a k-mer occurs more often in ref_seq than its count says */
#define LCTY_DB_WARN_REF_MISMATCH   2u   /* ... and ref_seq has no N runs: the error the reference logs at counts.rs:208-211 */
typedef struct lcty_db_params {
    uint32_t div_k, div_w;        /* 15, 15 (add.rs:77-78) */
    int32_t  calc_div;            /* 0 (add.rs:76): 1 = --calc-div, distances.bin is made */
    int32_t  only_seqs;           /* 0: 1 = --only-seqs, the FASTA text alone */
} lcty_db_params;
typedef struct lcty_db_check {
    uint64_t n_high;              /* pairs with diverg >= 0.2 */
    double   highest;             /* 0 when n_high == 0 */
    uint32_t highest_i, highest_j;
} lcty_db_check;
typedef struct lcty_db_stats {
    uint64_t n_minimizers, n_columns, n_chunks;    /* list entries; distinct (hash, copy) columns; passes over the bit matrix */
    uint64_t n_fast, n_walk, n_sorted_host;        /* sequences per minimizer path; lists sorted on the host */
    uint64_t bytes_h2d, bytes_d2h, bitmat_bytes;
    /* wall time per stage with the stream drained at its end: minimizers (upload included), LDS sort, host sort, column index,
     * bit matrix + Gram tiles (download included), off-target (transfers included), host work, whole call */
    double   minim_ms, sort_ms, sort_host_ms, index_ms, tiles_ms, offt_ms, host_ms, total_ms;
} lcty_db_stats;
typedef struct lcty_db_files {
    uint8_t* fasta;     uint64_t fasta_len;        /* text of haplotypes.fa */
    uint8_t* kmers;     uint64_t kmers_len;        /* kmers.bin: off-target block, then the counts as given (empty with only_seqs) */
    uint8_t* distances; uint64_t distances_len;    /* distances.bin (empty without calc_div) */
    uint8_t* discarded; uint64_t discarded_len;    /* discarded_haplotypes.txt (empty: no file) */
    uint32_t* kept;     uint32_t n_kept;           /* input indices of the haplotypes written */
    uint32_t warn_bits;
    lcty_db_check check;
    lcty_db_stats stats;
} lcty_db_files;

void    lcty_db_params_default(lcty_db_params* params);
int32_t lcty_db_minimizers(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t k, uint32_t w,
                           uint64_t* min_off, uint64_t** hashes, lcty_db_stats* stats);
int32_t lcty_db_divergences(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t k, uint32_t w,
                            uint32_t* uniq, double* diverg, lcty_db_check* check, lcty_db_stats* stats);
int32_t lcty_db_off_target(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, const uint16_t* counts,
                           const uint64_t* cnt_off, uint32_t k, uint32_t counter_bytes, const uint8_t* ref_seq, uint64_t ref_len,
                           const uint16_t* ref_counts, uint64_t n_ref_counts, uint16_t* out, uint32_t* warn_bits, lcty_db_stats* stats);
int32_t lcty_db_discard_identical(uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, const char* names, uint32_t* kept,
                                  uint32_t* n_kept, uint32_t* owner, char* text, uint64_t cap, uint64_t* needed);
int32_t lcty_kmer_counts_write(uint32_t k, uint32_t counter_bytes, uint32_t n_contigs, const uint64_t* cnt_off, const uint16_t* counts,
                               uint8_t* out, uint64_t cap, uint64_t* needed);
int32_t lcty_distances_write(uint32_t k, uint32_t w, uint32_t n_alleles, const uint32_t* uniq, uint8_t* out, uint64_t cap, uint64_t* needed);
int32_t lcty_fasta_write_text(uint32_t n_seqs, const char* names, const uint8_t* seqs, const uint64_t* seq_off, char* out, uint64_t cap,
                              uint64_t* needed);
int32_t lcty_db_build_locus(lcty_ctx* ctx, uint32_t n_seqs, const char* names, const uint8_t* seqs, const uint64_t* seq_off,
                            const uint8_t* ref_seq, uint64_t ref_len, const uint16_t* counts, const uint64_t* cnt_off, uint32_t k,
                            uint32_t counter_bytes, const lcty_db_params* params, lcty_db_files* out);
void    lcty_db_files_free(lcty_db_files* files);

/* ---- a locus from a pangenome VCF (locityper target -v: expansion, reconstruction, ref.bed; lcty_panvcf.hip) --------------------------
 * What add_locus does with a VCF before process_alleles (src/command/add.rs:733-782): the boundaries of the locus move onto a quiet,
 * unique piece of the reference, every phased haplotype of the VCF is rebuilt over the new interval, and the sequences go to
 * lcty_db_build_locus unchanged. Integer and byte work, and one short f64 recipe that is followed to the bit. Positions are 0-based.
 *
 * lcty_vcf_open / _view_get / _region / _free (host): a text VCF — plain, gzip or BGZF, told by its first bytes; read whole, no BCF (a
 *   `.bcf` path is LCTY_ERR_UNSUPPORTED). open reads the sample names of the #CHROM line and the ploidies of the FIRST record
 *   (HaplotypeNames::new, panvcf.rs:85-91); a file without records is LCTY_ERR_INVALID_DATA as there. region returns the records htslib's
 *   fetch(start, end) returns — same contig, pos < end, pos + len(REF) > start, in file order; INFO/END is NOT looked at, a stated
 *   difference for symbolic alleles — as flat arrays: pos, ref_len = len(REF), the alleles verbatim (REF first; no case folding) in
 *   allele_bytes with rec_allele[n_recs + 1] indexing allele_off[n_alleles + 1], gt[n_recs][n_haps] the allele indices of every sample's
 *   GT one after the other (hap_off of the view; -1 for '.'), phased[n_recs][n_samples] = the separator before the sample's last allele
 *   is '|' (a haploid call has none: 1). sample_used (NULL: all) [n_samples]: for these samples a GT whose allele count differs from the
 *   first record's ploidy ("has ploidy ... (expected ...)", panvcf.rs:161-164) and a sample of ploidy > 1 whose last separator is '/'
 *   ("is unphased", 167-171) are LCTY_ERR_INVALID_DATA. A contig the file does not name gives no records.
 * lcty_vcf_indexed_open / _view_get / _plan / _fetch / _close: the same records through the file's tabix index, what add_locus does with
 *   its bcf::IndexedReader (add.rs:802): it fetches the two flanks of a locus (add.rs:496-499) and reconstruct_sequences the interval
 *   (panvcf.rs, filter_variants), never the whole file. The file must be BGZF (a plain or plain-gzip file is LCTY_ERR_INVALID_INPUT: an
 *   indexed file must be BGZF); the index is `.tbi` (index_path NULL: path + ".tbi"): a `.csi` index and a `.bcf` file are
 *   LCTY_ERR_UNSUPPORTED, no index LCTY_ERR_INVALID_INPUT, an index whose format is not 2 (VCF), whose counts are negative or reach
 *   beyond its bytes, whose names lack their terminators or one of whose chunks begins behind its end LCTY_ERR_INVALID_DATA naming the
 *   index file. open (host) reads the index and only the head of the file — BGZF blocks from offset 0 until the #CHROM line and the
 *   first record are complete — and fills the view of lcty_vcf_open (samples, the ploidies of the first record of the FILE, hap_off)
 *   with n_records = 0: the file is not walked. Its errors (no #CHROM line, a record before it, no records) are lcty_vcf_open's.
 *   plan (host): the chunks of [start, end) on contig by the rule of lcty_sample_bam_plan — the bins of the region without the chunks
 *   that end at or before the linear index's offset of its first 16 kb window, sorted, merged where they touch, overlap or meet in one
 *   BGZF block; chunk_cap / n_chunks / blocks_total as there. fetch (device; add.rs:496-499, panvcf.rs filter_variants): exactly the
 *   arrays lcty_vcf_region returns for the same file and arguments (the same fetch rule; INFO/END is still not looked at; a contig
 *   the index does not know gives no records), released with lcty_vcf_records_free. Only the chunks are read and inflated (knob
 *   "sample_bam_inflate": 0 the host's zlib pool, 1 the device); line starts, record heads, the allele pool and the records x samples
 *   GT matrix are made by kernels on the inflated text (lcty_vcf_fetch.hip). The first offending line in file order —
 *   a record of the window with a wrong column count, no GT, an unparsable genotype, a ploidy mismatch or an unphased call of a used
 *   sample, an allele index above 32767, or any line of the chunks that names the contig with a bad position — is handed to the line
 *   functions of lcty_vcf_open / lcty_vcf_region: status and text are theirs. LCTY_ERR_UNSUPPORTED: a slice above knob
 *   "vcf_max_slice_bytes" (default 2^33), 2^31 - 16 lines or more, a line of 2^32 bytes or more. Without a device (ctx NULL, none
 *   visible) fetch is LCTY_ERR_RUNTIME: there is no CPU fallback. stats (may be NULL): chunks, bytes read and inflated, lines walked,
 *   records kept, the milliseconds of each stage.
 * lcty_panvcf_names (host): HaplotypeNames::new (panvcf.rs:65-135) on samples (n_samples 0-terminated names) and their ploidies: the
 *   retained columns in order (shift_ix), the reference first (col_sample = LCTY_NONE_U32) unless leave_out (n_leave_out 0-terminated
 *   names) holds ref_name; a haplotype is `sample` for ploidy 1, else `sample.<hap_ix + 1>`; leave_out matches a sample or a haplotype.
 *   LCTY_ERR_INVALID_DATA: duplicate name, ploidy 0, ploidy > 255, no sample left ("Loaded zero haplotypes"). Called twice: col_sample =
 *   col_hap = names = NULL sizes it (*n_cols, *names_len). *n_left_out (may be NULL): haplotypes left out.
 * lcty_panvcf_filter (device): filter_variants' has_variation (panvcf.rs:173-181): kept[v] = some column of gt[n_recs][n_cols] (the
 *   matrix restricted to the retained columns; a kept reference is a column of zeros) has allele >= 1.
 * lcty_panvcf_reconstruct (device): filter_variants (149-184), reconstruct_sequences (223-321) and the has_n filter of add_locus
 *   (add.rs:775-780) over [ref_start, ref_end) with its reference bytes ref_seq. A record is kept iff some column has allele >= 1; a
 *   kept record with var_end <= ref_start is skipped, one with ref_end <= var_start ends the walk, one that straddles either end is
 *   LCTY_ERR_INVALID_INPUT ("overlaps the boundary of the region"). Per column a non-reference allele is taken iff var_start >=
 *   prev_end, else it counts in total_overlaps — or, with overlaps_allowed == 0, is LCTY_ERR_INVALID_DATA naming the first such
 *   (record, haplotype) in record-major order ("Overlapping variants forbidden (contig:pos for name)"). A missing allele adds ref_len
 *   to the column's unknown_nts and uses the reference. ALT bytes are appended verbatim. A column is dropped when f64(unknown) >
 *   unknown_frac * f64(len) (LCTY_PANVCF_UNKNOWN), and then when its sequence holds b'N' (LCTY_PANVCF_HAS_N). names: n_cols
 *   0-terminated names. Out: the surviving sequences concatenated with seq_off[n_seqs + 1] and their names, in the layout
 *   lcty_db_build_locus takes, kept_cols[n_seqs] their columns; per column col_unknown, col_len, col_reason. An allele index the
 *   record does not have, or a broken allele table, is LCTY_ERR_INVALID_DATA. Kernels: a row reduction with the transposed copy of
 *   the matrix, one wavefront per column for the accept rule, scans for the offsets, a tiled gather, a compaction;
 *   no host loop over records and no host copy per haplotype. Release with lcty_panvcf_out_free.
 * lcty_db_find_boundary (device): find_best_boundary::<LEFT> (add.rs:371-435) over [start, end): counts[n_counts] the k-mer counts of
 *   the side's sequence, n_counts == (end - start) + moving_window - k; the records (pos, ref_len) sorted by position (else
 *   LCTY_ERR_INVALID_DATA), applied to every position IN RECORD ORDER: covered positions 0, the nine to the left scaled by
 *   (9 - i) / 10, the nine to the right by (i + 1) / 10; then w -= (w * (0.2 / allowed_expansion)) * i with i the distance from the
 *   locus side; left != 0: the LAST maximum, else the FIRST; a maximum of 0.0 is *found = 0; start == end as lines 381-387.
 *   weights (may be NULL) [end - start]: the final weights, equal to the reference's to the bit.
 * lcty_db_expand_locus: expand_locus (438-518) and the retry loop of add_locus (733-755). win_seq / win_counts: the reference bytes
 *   and the k-mer counts (n_win_counts == win_len + 1 - k) of ONE window [win_start, win_start + win_len) that holds the flanks of
 *   every attempt, [inner_start - E, min(inner_end + E, contig_len)); the counts of a flank are a slice of it. pos / ref_len: the
 *   KEPT records of the window (lcty_panvcf_filter) in file order. expansions: strictly increasing, 0 only alone; moving_window is
 *   raised to k (add.rs:812). Per attempt: the flank ranges of 459-466, the crop at the last / first N (an N inside the locus side:
 *   LCTY_ERR_INVALID_INPUT "Unknown sequence at the locus"), the records of [left_start, inner_start + 1) and [inner_end - 1,
 *   right_end) by the fetch rule, two boundary searches. A locus shorter than the moving window: LCTY_ERR_INVALID_INPUT; no attempt
 *   succeeds: LCTY_ERR_RUNTIME "Cannot expand locus ...".
 * lcty_db_locus_from_vcf: the whole step: lcty_panvcf_filter over the window's records, lcty_db_expand_locus (unless the only
 *   allowed expansion is 0), lcty_panvcf_reconstruct over the new interval, check_sequences without a reference (add.rs:655-690:
 *   fewer than two haplotypes LCTY_ERR_INVALID_DATA; a sequence shorter than the 5-base affix LCTY_ERR_INVALID_INPUT; the warnings
 *   as LCTY_LOCUS_WARN_* bits), lcty_db_build_locus. hap_counts / hap_cnt_off: the k-mer counts of the SURVIVING haplotypes and the
 *   new reference interval as lcty_db_build_locus takes them — known only once the sequences are, so a first call with
 *   params->only_seqs = 1 gives the sequences to count. ref_bed: the line of ref.bed, "contig\tstart\tend\tname\n". files.kept
 *   indexes the reconstructed haplotypes, hap_cols[n_hap_cols] their columns. Lock files, `success`, Jellyfish and the rerun modes
 *   stay with the caller. Release with lcty_locus_vcf_out_free. */
#define LCTY_PANVCF_KEPT    0u
#define LCTY_PANVCF_UNKNOWN 1u   /* too many unknown bases (discard_unknown, panvcf.rs:196-219) */
#define LCTY_PANVCF_HAS_N   2u   /* the sequence holds N (add.rs:776) */
#define LCTY_LOCUS_WARN_VERY_SHORT       1u   /* shortest haplotype < 1 000 (add.rs:660-662) */
#define LCTY_LOCUS_WARN_SHORT            2u   /* ... < 10 000 (663-664) */
#define LCTY_LOCUS_WARN_BOUNDARY_DIFFERS 4u   /* the haplotypes differ in their first or last 5 bases (684-688) */
typedef struct lcty_vcf lcty_vcf;
typedef struct lcty_vcf_view {
    uint32_t n_samples, n_haps;                    /* n_haps = sum of the ploidies */
    uint64_t n_records;                            /* records in the file */
    const char* samples; uint64_t samples_len;     /* 0-terminated names */
    const uint32_t* ploidy;                        /* [n_samples], from the first record */
    const uint32_t* hap_off;                       /* [n_samples + 1] columns of gt */
} lcty_vcf_view;
typedef struct lcty_vcf_records {
    uint32_t n_recs, n_haps, n_samples, _pad0;
    uint64_t n_alleles, pool_len;
    uint32_t* pos; uint32_t* ref_len; uint32_t* rec_allele;
    uint64_t* allele_off; uint8_t* allele_bytes;
    int16_t* gt; uint8_t* phased;
} lcty_vcf_records;
typedef struct lcty_panvcf_stats {
    uint64_t bytes_h2d, bytes_d2h, n_segments, out_bytes;
    /* wall time per stage with the stream drained at its end: uploads, row reduction + transpose, chain, scans + segment lists, gather,
     * compaction + download, whole call */
    double   upload_ms, rows_ms, chain_ms, scan_ms, gather_ms, compact_ms, total_ms;
} lcty_panvcf_stats;
typedef struct lcty_panvcf_out {
    uint8_t* seqs; uint64_t* seq_off;              /* the surviving haplotypes, seq_off[n_seqs + 1] */
    char* names; uint64_t names_len;               /* their names, 0-terminated */
    uint32_t* kept_cols;                           /* [n_seqs] their columns */
    uint32_t* col_unknown; uint32_t* col_len; uint8_t* col_reason;   /* [n_cols] unknown_nts, reconstructed length, LCTY_PANVCF_* */
    uint32_t n_seqs, n_cols, n_unknown, n_with_n;
    uint64_t total_overlaps, n_kept_records;       /* ignored alleles; records that passed the variation filter */
    lcty_panvcf_stats stats;
} lcty_panvcf_out;
typedef struct lcty_expand_out {
    uint32_t start, end;                           /* the new interval */
    int32_t  attempt;                              /* index of the allowed expansion that succeeded */
    uint32_t allowed_expansion, n_attempts;
    uint32_t crop_bits;                            /* 1: the left flank was cropped at an N, 2: the right one */
    double   total_ms;
} lcty_expand_out;
typedef struct lcty_locus_vcf_in {
    const char* locus; const char* contig;
    uint32_t inner_start, inner_end, contig_len, win_start;
    const uint8_t* win_seq; uint64_t win_len;
    const uint16_t* win_counts; uint64_t n_win_counts;      /* may be NULL when the only allowed expansion is 0 */
    uint32_t k, counter_bytes;
    uint32_t n_recs, n_cols;                                /* the records of the window (lcty_vcf_region) and the retained columns */
    const uint32_t* pos; const uint32_t* ref_len; const uint32_t* rec_allele;
    const uint64_t* allele_off; const uint8_t* allele_bytes;
    const int16_t* gt; const char* names;
    const uint32_t* expansions; uint32_t n_expansions, moving_window;   /* 20 000, 50 000, 200 000; 500 (add.rs:72-73) */
    double   unknown_frac;                                  /* 0.0001 (add.rs:79) */
    int32_t  overlaps_allowed, _pad0;
    const uint16_t* hap_counts; const uint64_t* hap_cnt_off; /* NULL with params->only_seqs */
} lcty_locus_vcf_in;
typedef struct lcty_locus_vcf_stats {
    uint32_t start, end;                           /* the interval of ref.bed */
    int32_t  attempt; uint32_t allowed_expansion, crop_bits, warn_bits;
    uint32_t n_cols, n_haplotypes, n_unknown, n_with_n, n_identical, n_records;   /* columns in; reconstructed and passed; dropped for unknown / N / identity */
    uint64_t n_kept_records, total_overlaps, shortest;
    double   filter_ms, expand_ms, reconstruct_ms, build_ms, total_ms;
    lcty_panvcf_stats recon;
} lcty_locus_vcf_stats;
typedef struct lcty_locus_vcf_out {
    lcty_db_files files;
    char* ref_bed; uint64_t ref_bed_len;
    uint32_t* hap_cols; uint32_t n_hap_cols, _pad0;
    lcty_locus_vcf_stats stats;
} lcty_locus_vcf_out;

int32_t lcty_vcf_open(const char* path, lcty_vcf** out);
int32_t lcty_vcf_view_get(const lcty_vcf* vcf, lcty_vcf_view* view);
int32_t lcty_vcf_region(const lcty_vcf* vcf, const char* contig, uint32_t start, uint32_t end, const uint8_t* sample_used, lcty_vcf_records* out);
void    lcty_vcf_records_free(lcty_vcf_records* records);
void    lcty_vcf_free(lcty_vcf* vcf);
/* the indexed reader (add.rs:496-499, 802; panvcf.rs filter_variants) */
typedef struct lcty_vcf_indexed lcty_vcf_indexed;
typedef struct lcty_vcf_fetch_stats {
    uint64_t n_chunks, file_bytes, bytes_read, blocks_inflated, bytes_inflated;
    uint64_t lines_walked, records_kept;
    double ms_read, ms_inflate, ms_upload, ms_lines, ms_heads, ms_alleles, ms_gt, ms_download, ms_total;
} lcty_vcf_fetch_stats;
/* host; index_path NULL: path + ".tbi". The view's n_records is 0: the file is not walked (add.rs:802) */
int32_t lcty_vcf_indexed_open(const char* path, const char* index_path, lcty_vcf_indexed** out);
int32_t lcty_vcf_indexed_view_get(const lcty_vcf_indexed* vcf, lcty_vcf_view* view);
/* host: the contigs of the file in the order of their indices (htslib's get_tid, extra/into_vcf.py:170): the ##contig lines of the head in
 * file order with their length= (0: none given), then the names of the tabix index that no line declares, length 0, as htslib adds them.
 * names: n_contigs 0-terminated names. The arrays are the reader's and live until lcty_vcf_indexed_close. */
typedef struct lcty_vcf_contigs {
    uint32_t n_contigs, _pad0;
    const char* names; uint64_t names_len;
    const uint64_t* length;
} lcty_vcf_contigs;
int32_t lcty_vcf_indexed_contigs(const lcty_vcf_indexed* vcf, lcty_vcf_contigs* out);
/* host: the merged chunks of a window (add.rs:496-499: the flanks; panvcf.rs filter_variants: the interval) */
int32_t lcty_vcf_indexed_plan(lcty_vcf_indexed* vcf, const char* contig, uint32_t start, uint32_t end, uint64_t chunk_cap,
                              uint64_t* n_chunks, uint64_t* chunk_beg, uint64_t* chunk_end, uint64_t* blocks_total);
/* device: the records of a window, the arrays of lcty_vcf_region (add.rs:496-499, panvcf.rs filter_variants) */
int32_t lcty_vcf_indexed_fetch(lcty_ctx* ctx, lcty_vcf_indexed* vcf, const char* contig, uint32_t start, uint32_t end,
                               const uint8_t* sample_used, lcty_vcf_records* out, lcty_vcf_fetch_stats* stats);
void    lcty_vcf_indexed_close(lcty_vcf_indexed* vcf);
int32_t lcty_panvcf_names(uint32_t n_samples, const char* samples, const uint32_t* ploidy, const char* ref_name, uint32_t n_leave_out,
                          const char* leave_out, uint32_t cap_cols, uint32_t* n_cols, uint32_t* col_sample, uint32_t* col_hap, char* names,
                          uint64_t cap_names, uint64_t* names_len, uint32_t* n_left_out);
int32_t lcty_panvcf_filter(lcty_ctx* ctx, uint32_t n_recs, uint32_t n_cols, const int16_t* gt, uint8_t* kept, uint64_t* n_kept);
int32_t lcty_panvcf_reconstruct(lcty_ctx* ctx, const char* contig, uint32_t ref_start, uint32_t ref_end, const uint8_t* ref_seq,
                                uint32_t n_recs, const uint32_t* pos, const uint32_t* ref_len, const uint32_t* rec_allele,
                                const uint64_t* allele_off, const uint8_t* allele_bytes, uint32_t n_cols, const int16_t* gt, const char* names,
                                double unknown_frac, int32_t overlaps_allowed, lcty_panvcf_out* out);
void    lcty_panvcf_out_free(lcty_panvcf_out* out);
int32_t lcty_db_find_boundary(lcty_ctx* ctx, uint32_t start, uint32_t end, uint32_t n_recs, const uint32_t* pos, const uint32_t* ref_len,
                              uint32_t k, const uint16_t* counts, uint64_t n_counts, uint32_t allowed_expansion, uint32_t moving_window,
                              int32_t left, int32_t* found, uint32_t* position, double* weights);
int32_t lcty_db_expand_locus(lcty_ctx* ctx, const char* locus, uint32_t inner_start, uint32_t inner_end, uint32_t contig_len,
                             uint32_t win_start, const uint8_t* win_seq, uint64_t win_len, uint32_t k, const uint16_t* win_counts,
                             uint64_t n_win_counts, uint32_t n_recs, const uint32_t* pos, const uint32_t* ref_len, uint32_t n_expansions,
                             const uint32_t* expansions, uint32_t moving_window, lcty_expand_out* out);
int32_t lcty_db_locus_from_vcf(lcty_ctx* ctx, const lcty_locus_vcf_in* in, const lcty_db_params* params, lcty_locus_vcf_out* out);
void    lcty_locus_vcf_out_free(lcty_locus_vcf_out* out);

/* ---- a locus's haplotypes as a VCF (locityper paf-vcf, src/command/paf_vcf.rs; lcty_pafvcf.hip) ----------------------------------------
 * The inverse of the section above: haplotypes.fa.gz + haplotypes.paf.gz (what lcty_align_haplotypes writes) -> haplotypes.vcf.gz.
 * Integer and byte work. Positions are 0-based inside the reference haplotype; the text adds shift + 1. A variant is the four numbers
 * (ref_start, ref_end, hap_start, hap_end) of VarRange (202-208). Every device entry point fills the parts of one lcty_pafvcf_out it
 * makes (the others stay NULL / 0) and the out is released with lcty_pafvcf_out_free.
 *
 * lcty_pafvcf_samples (host): group_haplotypes (569-621) over names (n_seqs 0-terminated contig names) and the text of
 *   discarded_haplotypes.txt (NULL / 0: none; DiscardedHaplotypes::load, src/seq/contigs.rs:488-528, with its chaining through left-hand
 *   names the FASTA does not have; a line with fewer than 3 columns is LCTY_ERR_INVALID_INPUT). A name must match
 *   ^([0-9A-Za-z][0-9A-Za-z+._|~=@^-]*?)([._][1-9])?$ (577), else LCTY_ERR_INVALID_DATA (Error::ParsingError): with a suffix sample =
 *   prefix, slot = digit - 1 and the sample has at least 2 slots, without one slot 0; a later writer of a slot replaces an earlier one;
 *   every contig under its own name, then under every discarded name listed behind it ('=' and '~' lines alike). The name equal to
 *   ref_hap gives *ref_id and is no sample — unless it has a suffix: then it stays one and LCTY_PAFVCF_WARN_REF_SUFFIX is set (588-590).
 *   ref_hap not found: LCTY_ERR_INVALID_INPUT (612-616). A '~' line sets LCTY_PAFVCF_WARN_PRUNED (convert_to_vcf 633-635). Out: the
 *   samples sorted bytewise (618-619) as 0-terminated names, slot_off[n_samples + 1], slot_hap[n_slots] (contig index or LCTY_NONE_U32).
 *   Called twice: sample_names = slot_off = slot_hap = NULL sizes it (*n_samples, *names_len, *n_slots).
 * lcty_pafvcf_variants (device): process_paf (362-415), process_haplotype (276-332) and move_all_left (242-271, gap_move_left 231-239)
 *   for all haplotypes at once, on the arrays of lcty_paf_read (id1 = query, id2 = target, CIGAR words length << 4 | BAM operation).
 *   Only entries with the reference on one side count; with the reference as the query the items are inverted (I, S -> D; D -> I;
 *   cigar.rs:147-158); an entry whose CIGAR lengths differ from the two sequences is skipped and counted (n_bad_len, 403-407); of the
 *   others the LAST in file order is the haplotype's (408) — a stated difference: the reference also walks the entries it then replaces,
 *   so an M in a replaced entry fails there and not here. A haplotype without an entry is missing (has_aln 0, counted in n_missing, 410);
 *   the reference haplotype has an entry and no variant (371). An M or H item is LCTY_ERR_RUNTIME (293-295), a last variant that reaches
 *   past a sequence too (325-329). Items merge as 300-310, a new variant takes one of the three forms of 313-319 — reproduced as
 *   written, the right-padded form's quirk included (`5I1D1=` on `GG` gives (0, 1, 0, 6)). n_shifted: variants the shift moved. A stated
 *   difference: every '=' run is compared with the bases it covers, and a run over different bases is LCTY_ERR_INVALID_DATA (the
 *   reference writes a VCF that does not describe the haplotype). Out: var_off[n_seqs + 1], ref_start / ref_end / hap_start / hap_end
 *   [n_variants] after the shift, has_aln[n_seqs].
 * lcty_pafvcf_ranges (device): combine_variants (535-555) on the (ref_start, ref_end) of all variants: unique_* the sorted, deduplicated
 *   ranges, merged_* those with every run of OVERLAPPING ranges joined (prev_end > start; ranges that touch stay apart).
 * lcty_pafvcf_table (device): get_hap_ranges (420-460, the bisections of src/algo/bisect.rs:45-83) and the allele part of write_vcf
 *   (473-494) for a list of ranges: allele_ix[n_ranges][n_seqs] — -1 for None: a missing haplotype, a range that starts or ends inside
 *   one of the haplotype's variants, a slice with an N —, 0 the reference's slice, k >= 1 the k-th other allele in the order of its
 *   first carrier in contig order. n_alleles[n_ranges] (the reference's included), and for the alleles from 1 on allele_off[n_ranges + 1]
 *   into allele_hap (the first carrier) / allele_start / allele_len (the slice inside that haplotype). Equality is decided by the
 *   bytes; lcty_ctx_set_knob "pafvcf_hash_bits" only narrows the hash that picks the candidates. A slice that lies outside its
 *   haplotype (where the reference panics: the quirk above) is LCTY_ERR_RUNTIME. The variants of a haplotype must be ordered
 *   (LCTY_ERR_INVALID_INPUT).
 * lcty_pafvcf_text (device): the record lines of write_vcf (495-517) from a table: a range with one allele gives no line; else
 *   chrom \t start + shift + 1 \t . \t REF \t ALT[,ALT..] \t60\t.\t.\tGT and per sample \t and its slots joined by '|', '.' for an empty
 *   slot or a None cell. Out: merged / merged_len (no header).
 * lcty_paf_to_vcf (device): convert_to_vcf (623-657) on buffers: the samples, the variants, the ranges, and for the merged ranges —
 *   with_separate != 0: also for the unique ones (separate) — the table and the text behind the header of 349-357. chrom NULL: the
 *   records are named ref_hap with shift 0; else [region_start, region_end) must be as long as the reference haplotype
 *   (LCTY_ERR_INVALID_DATA, 639-642) and shift = region_start. Kernels: a wavefront per entry and per haplotype, a lane
 *   per variant, a radix sort, scans and compactions, a lane per cell, a workgroup per line; no host loop over haplotypes, variants,
 *   ranges or cells and no host copy per haplotype — but for the checks of the caller's offset arrays (seq_off, cigar_off, slot_off;
 *   in the part-wise entry points also var_off, the variants' order and the ranges), which keep the kernels inside their buffers.
 * Limits (LCTY_ERR_UNSUPPORTED): more than 65 535 haplotypes, a haplotype of 2^31 bases, 2^31 variants / ranges / alleles, a line of
 *   2^32 bytes, an allele table beyond knob "pafvcf_table_mb". */
#define LCTY_PAFVCF_WARN_REF_SUFFIX 1u   /* the reference haplotype's name has a haplotype suffix and stays in the VCF (588-590) */
#define LCTY_PAFVCF_WARN_PRUNED     2u   /* "Haplotypes were previously pruned (~ for some lines), VCF will be inaccurate" (633-635) */
typedef struct lcty_pafvcf_stats {
    uint64_t n_variants, n_unique, n_merged, n_shifted, n_lines_merged, n_lines_separate, merged_bytes, separate_bytes;
    uint32_t n_missing, n_bad_len, warn_bits, n_samples;
    /* wall time per stage with the stream drained at its end: uploads, variants (entries, walk, shift), ranges, tables, texts (with
     * their download), whole call */
    double   upload_ms, variants_ms, ranges_ms, table_ms, text_ms, total_ms;
} lcty_pafvcf_stats;
typedef struct lcty_pafvcf_out {
    uint32_t n_seqs, _pad0;
    uint64_t n_variants, n_unique, n_merged, n_ranges;
    uint64_t* var_off; uint32_t* ref_start; uint32_t* ref_end; uint32_t* hap_start; uint32_t* hap_end; uint8_t* has_aln;      /* variants */
    uint32_t* unique_start; uint32_t* unique_end; uint32_t* merged_start; uint32_t* merged_end;                                /* ranges */
    int32_t* allele_ix; uint32_t* n_alleles; uint64_t* allele_off; uint32_t* allele_hap; uint32_t* allele_start; uint32_t* allele_len;   /* table */
    char* merged; uint64_t merged_len; char* separate; uint64_t separate_len;                                                  /* text */
    lcty_pafvcf_stats stats;
} lcty_pafvcf_out;

int32_t lcty_pafvcf_samples(uint32_t n_seqs, const char* names, const char* discarded, uint64_t discarded_len, const char* ref_hap, uint32_t cap_samples,
                            uint32_t* n_samples, char* sample_names, uint64_t cap_names, uint64_t* names_len, uint32_t* slot_off, uint32_t cap_slots,
                            uint32_t* n_slots, uint32_t* slot_hap, uint32_t* ref_id, uint32_t* warn_bits);
int32_t lcty_pafvcf_variants(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, uint64_t n_entries,
                             const uint32_t* id1, const uint32_t* id2, const uint64_t* cigar_off, const uint32_t* cigar, lcty_pafvcf_out* out);
int32_t lcty_pafvcf_ranges(lcty_ctx* ctx, uint64_t n_variants, const uint32_t* ref_start, const uint32_t* ref_end, lcty_pafvcf_out* out);
int32_t lcty_pafvcf_table(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, const uint64_t* var_off,
                          const uint32_t* ref_start, const uint32_t* ref_end, const uint32_t* hap_start, const uint32_t* hap_end, const uint8_t* has_aln,
                          uint64_t n_ranges, const uint32_t* range_start, const uint32_t* range_end, lcty_pafvcf_out* out);
int32_t lcty_pafvcf_text(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, uint64_t n_ranges,
                         const uint32_t* range_start, const uint32_t* range_end, const int32_t* allele_ix, const uint32_t* n_alleles,
                         const uint64_t* allele_off, const uint32_t* allele_hap, const uint32_t* allele_start, const uint32_t* allele_len,
                         uint32_t n_samples, const uint32_t* slot_off, const uint32_t* slot_hap, const char* chrom, uint32_t shift, lcty_pafvcf_out* out);
int32_t lcty_paf_to_vcf(lcty_ctx* ctx, uint32_t n_seqs, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const char* discarded,
                        uint64_t discarded_len, const char* ref_hap, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2,
                        const uint64_t* cigar_off, const uint32_t* cigar, const char* chrom, uint32_t region_start, uint32_t region_end,
                        int32_t with_separate, lcty_pafvcf_out* out);
void    lcty_pafvcf_out_free(lcty_pafvcf_out* out);
/* A buffer as a BGZF file (SAM specification 4.1; what htslib::bgzf::Writer gives create_vcf_writer, 341-344): blocks of at most 0xff00
 * input bytes and the empty end-of-file block. The deflate bytes are zlib's at level 6; the inflated bytes are `data`. Host code; the
 * writer is the one behind lcty_write_bam. */
int32_t lcty_io_write_bgzf(const char* path, const uint8_t* data, uint64_t len);

/* ---- a cohort's genotypes as a phased VCF (extra/into_vcf.py, extra/into_csv.py) ----------------------------------------
 * For every locus into_vcf.py takes the records of the locus's interval from a phased variants file and, for every sample, copies the
 * GT of the predicted haplotypes into a phased call (process_locus, into_vcf.py:117-144). Here the window is the arrays of an
 * lcty_vcf_records (lcty_vcf_region, lcty_vcf_indexed_fetch), the predictions are columns of its GT matrix, and the text of the file is
 * made on the device. lcty_gtvcf_merge is merge_vcfs (167-196); the table between the two scripts is lcty_res_summary_read and
 * lcty_predictions_csv_write / _read (into_csv.py:65-100, 125; load_predictions, into_vcf.py:18-44).
 *
 * lcty_res_summary_read (host): the top level of one res.json.gz as process_sample reads it (into_csv.py:73-96), through the JSON reader
 *   of lcty_bg_from_json. state: LCTY_RES_MISSING when the file does not exist (the caller's `?` row, 74-77), LCTY_RES_NO_GENOTYPE when
 *   it has no `genotype` key (`*`, 85-87), else LCTY_RES_CALLED with genotype = the comma-joined allele names (90), qual10 =
 *   floor(10 quality) in double arithmetic as line 91 computes it (a call without a numeric quality is LCTY_ERR_INVALID_DATA, as
 *   float(None) raises there), reads / unexpl = total_reads / unexpl_reads, which must be whole numbers, wdist5 = weight_dist as `:.5f`
 *   rounds it (96: the text of %.5f, read back digit by digit), LCTY_GTVCF_ABSENT for an absent, null or NaN value (get_or_nan, 60-62),
 *   warnings = the texts joined by `;`, `*` without the key (95). A file that is no gzip or no JSON object: LCTY_ERR_INVALID_DATA.
 *   The two strings are released with lcty_res_summary_free. In every other state they are NULL and the numbers absent. A call that
 *   fails leaves state LCTY_RES_UNKNOWN, which lcty_predictions_csv_write refuses: a corrupt file never becomes a `?` row.
 * lcty_predictions_csv_write (host): the table of into_csv.py:125 and one row per (sample[i], locus[i], rows[i]) in the order given (96;
 *   `?` and `*` rows end behind the genotype column as upstream's do): quality with one decimal and weight_dist with five
 *   (lcty_gtvcf_fixed_print with pad; absent: `nan`), the counts as integers (absent: `nan`, what Python prints for get_or_nan's value).
 *   A name or text with a tab or a newline: LCTY_ERR_INVALID_INPUT. A path that ends in .gz is written as gzip.
 * lcty_predictions_csv_read (host): load_predictions (into_vcf.py:18-44) and common.read_csv: lines that start with `#` before the
 *   column line are skipped, the columns are found by name (sample, locus, genotype required; quality, total_reads, unexpl_reads,
 *   weight_dist, warnings optional: absent for every row), a row may end early (csv.DictReader gives None: absent). Per row, in file
 *   order: the offsets of its sample, locus, genotype (`*` or `?`: no prediction, 26-27) and warnings in `text`, a pool of 0-terminated
 *   strings, and the four numbers in fixed point, parsed from the decimal text by lcty_gtvcf_fixed_parse's rule and never through a
 *   double (the counts with 0 decimals). samples_off[n_samples]: the distinct sample names, sorted bytewise (44). A sample and locus that
 *   appear twice keep the later row upstream (42); here both rows are returned and the caller takes the last. Released with
 *   lcty_predictions_free.
 * lcty_gtvcf_columns (host): copy_genotype's rule (into_vcf.py:99-114), applied once per predicted allele and not once per record.
 *   names: n_names 0-terminated allele names; cols[n_names]: the column of view's GT matrix each one reads. A name longer than 2 bytes
 *   whose second-to-last byte is `.` or `_` (102): sample = the name without its last two bytes, haplotype = the last byte as a digit
 *   (103-104), column = hap_off[sample] + digit - 1 (106). A name equal to genome_name (107): LCTY_GTVCF_REF, allele 0 in every record
 *   (108). Any other name: a sample, which must have ploidy 1 (110-112), column hap_off[sample]. LCTY_ERR_INVALID_DATA naming the allele:
 *   a sample the view does not have (upstream: KeyError), a last byte that is no digit, a digit above the sample's ploidy, a name without
 *   suffix of a sample with ploidy above 1 (the assertion of 112), and the digit 0 — a stated difference: Python would index from the end.
 * lcty_gtvcf_fixed_print / _parse (host): the numbers of the FORMAT fields are fixed point, value x 10^decimals as an integer (decimals
 *   <= 18; quality: 1, floor(10 q) as into_csv.py:91; weight_dist: 5, as `:.5f` of line 96), LCTY_GTVCF_ABSENT for an absent or NaN
 *   value. print, integer arithmetic only: the integer part, then the fraction without trailing zeros, no point when nothing follows
 *   (273 tenths: 27.3, 270: 27, 123 units of 1e-5: 0.00123), absent `.`; with pad != 0 all the decimals as `:.1f` / `:.5f` write them
 *   (into_csv.py:96), absent `nan`. A stated difference: htslib prints FORMAT floats with %g and loses digits. Called for the size
 *   (out NULL) and then with a buffer; no terminator is written. parse: [+-]digits[.digits], digit by digit and never through a double;
 *   digits behind the last decimal are dropped towards minus infinity; `nan` in any case and `NA` (parse_float, into_vcf.py:14-15) are
 *   absent; anything else, or a value of more than 18 digits, is LCTY_ERR_INVALID_DATA.
 * lcty_gtvcf_header (host): create_vcf_header (into_vcf.py:76-96) as pysam writes it: ##fileformat=VCFv4.2, the PASS filter htslib
 *   gives every new header, one ##contig per contig (79-83; contig_len NULL or an entry 0: no length=), the seven ##FORMAT lines in
 *   upstream's order and wording (84-93; GQ is declared and never written, as upstream never sets it), the #CHROM line with the samples
 *   (94-95). contigs, samples: 0-terminated names. Called for the size and then with a buffer.
 * lcty_tbi_write (host): the tabix index of a BGZF VCF, what pysam.tabix_index(preset='vcf') leaves beside it (into_vcf.py:143, 196);
 *   the library's first index writer. contigs: n_contigs 0-terminated names, all listed in the index; per record contig_ix, pos
 *   (0-based) and ref_len = len(REF), sorted by (contig_ix, pos), else LCTY_ERR_INVALID_INPUT; line_off[n_records + 1]: the offset of
 *   every record line in the inflated text and of what follows the last (lcty_gtvcf_add_locus gives them); block_off[n_blocks + 1]: the
 *   array of lcty_bgzf_deflate over that text. The virtual offset of text offset u is block_off[u / 0xff00] << 16 | u % 0xff00. Header:
 *   format 2, columns 1 / 2 / 0, meta `#`, skip 0. A record lies in bin reg2bin(pos, pos + max(len(REF), 1)); the chunks of a bin that
 *   touch are one; the linear index has a 16-kb window per entry, a window without a record takes the offset before it; the pseudo-bin
 *   37450 holds the reference's file range and record count as htslib writes them; n_no_coor 0. The file itself is BGZF
 *   (lcty_io_write_bgzf). A record that ends beyond 2^29 needs a CSI index: LCTY_ERR_UNSUPPORTED. BCF and CSI are not written.
 * lcty_gtvcf_create: a set for the loci of one cohort, on ctx, which outlives it. samples: n_samples 0-terminated names in the order of
 *   the output columns (load_predictions sorts them bytewise, into_vcf.py:44; the order is the caller's). field_mask: the features that
 *   follow GT, LCTY_GTVCF_QUAL .. _WARN. LCTY_GTVCF_ALL is the default. Upstream's load_predictions tests `'qual' in row` and `'warn' in
 *   row` (31, 39) against a table whose columns are `quality` and `warnings`, and so writes reads:unexpl:wdist alone: that is
 *   LCTY_GTVCF_UPSTREAM. Bits beyond LCTY_GTVCF_ALL, a name that is empty or holds a tab or a newline: LCTY_ERR_INVALID_INPUT. More than
 *   65 535 x 256 samples: LCTY_ERR_UNSUPPORTED. The set
 *   keeps the names, the FORMAT key, the device scratch of its calls and, on the device, what lcty_gtvcf_merge needs of every locus
 *   added: its records, 2 bytes per (record, predicted allele) and the feature text of every sample.
 * lcty_gtvcf_add_locus (device): the file of one locus (process_locus, 117-144), header and one line per record:
 *     chrom \t pos + 1 \t ID \t REF \t ALT[,ALT..] \t . \t . \t . \t FORMAT, then one field per sample (127-142).
 *   in: the locus's name (one locus per name, else LCTY_ERR_INVALID_INPUT), the contig's index in the variants file (get_tid, 170)
 *   and the interval [start, end) of ref.bed, which only the merge reads; chrom and the contig's length (0: unknown; 123-124; two loci
 *   of one contig index with different names or lengths: LCTY_ERR_INVALID_INPUT); the arrays of an lcty_vcf_records with n_haps columns, gt negative = missing;
 *   id_off[n_recs + 1] / id_bytes, the ID column (131) — NULL or an empty ID gives `.`; the fetch of lcty_vcf_indexed_fetch and
 *   lcty_vcf_region do not keep that column, so a caller that has only their arrays writes `.`; pred_off[n_samples + 1] / pred_col[]:
 *   per output sample the columns of its predicted alleles from lcty_gtvcf_columns (134-138), an empty range = no prediction (`*`, `?`
 *   or a sample the table does not have for this locus: 135-136); qual10, reads, unexpl, wdist5 [n_samples]: the features in fixed
 *   point, LCTY_GTVCF_ABSENT = absent (any of the four arrays NULL: absent for every sample); warn_off[n_samples + 1] / warn: the warning
 *   texts (NULL or an empty text: absent). A record with one allele has ALT `.`. A sample with a prediction: its alleles joined by `|`
 *   (139), `.` for a missing one (106, 113), then `:` and the value of every feature of field_mask, `.` for an absent one; a sample
 *   without: the one byte `.`. Features of samples without a prediction are not read.
 *   Kernels (lcty_gtvcf.hip), no host loop over records, samples or cells behind the check of the arguments: one lane per (record, slot)
 *   gathers call = pred_col == LCTY_GTVCF_REF ? 0 : gt[rec][pred_col] into calls[n_recs][n_slots], consecutive lanes on consecutive
 *   slots of one record; one lane per sample sizes and writes the feature text, which is the same in every record; a workgroup per
 *   record sums the line's length, a 64-bit scan places the lines, and a workgroup per line writes it with a scan of the field widths
 *   per 256 samples (the helpers of lcty_pafvcf.hip's text stage, lcty_text.hpp). The text is downloaded once.
 *   out: text = header + lines, line_off[n_lines + 1] the offset of every record line in text and text_len behind the last (what a
 *   tabix writer needs), calls[n_recs][n_slots] with in->want_calls (else NULL). Released with lcty_gtvcf_out_free.
 *   LCTY_ERR_INVALID_INPUT: null arguments, offsets that decrease, a record without an allele, a column beyond n_haps.
 *   LCTY_ERR_INVALID_DATA: a call that names an allele its record does not have; a warning text with a tab, a space, a newline or `:`
 *   (naming the sample). LCTY_ERR_UNSUPPORTED: a line of 2^32 bytes or more, more than 255 predicted alleles in one sample, a warning
 *   text above 65 535 bytes, more than 65 535 x 256 predicted alleles over all samples, 2^31 records, feature texts that may reach
 *   2^31 bytes over all samples (94 bytes per predicted sample plus the warning texts). A failed call
 *   leaves *out zeroed and the set as it was.
 * lcty_gtvcf_merge (device): merge_vcfs (167-196) over all loci added so far: one file with every record once. The loci are taken in
 *   the order (contig index, start, end) (176), whatever the order they were added in; a record's key is (contig index, pos, the tuple
 *   of its allele strings) (181); the lines come out in the order of the keys (192), tuples compared as Python compares them: element
 *   by element, bytewise, a proper prefix first. The header lists the contigs of the loci in index order with their lengths (169-172,
 *   189). Records of one key are joined (merge_vars, 153-164). Upstream cannot execute that branch — it reads GQ, which is never set,
 *   and qual, which its table never gives — so the rule is this library's own: per sample, the first record in the order of the loci
 *   keeps its field; a later record replaces it iff the sample has a prediction there and either had none so far, or the GTs differ
 *   and the later locus's quality in whole units (floor) is strictly larger; an absent quality is the lowest. ID, REF and ALT are the
 *   first record's (upstream asserts equal IDs, 154). Kernels: a stable radix sort (lcty_sort.hpp) of contig << 32 | pos over all
 *   records; one wavefront per run of equal (contig, pos), a lane per record, which ranks the run by allele bytes and marks the records
 *   that open a key; one lane per (line, sample) for the join; the text kernels of lcty_gtvcf_add_locus, each sample's field read from
 *   the record the join chose. out: text, line_off as above; the n_contigs names of the header (contigs, 0-terminated) and per line
 *   line_contig, line_pos, line_ref_len. line_contig[i] is the place of the line's contig among `contigs` (0 .. n_contigs - 1), NOT
 *   the index in the variants file, which may be sparse (loci on contigs 0, 6 and 21 give 0, 1, 2): contigs, line_contig, line_pos,
 *   line_ref_len and line_off go to lcty_tbi_write as they are. contig_ix[n_contigs]: the variants file's index of every header
 *   contig. stats: the sort, the runs and the join are merge_ms; n_joined: the records joined to another, upstream's "Merged N variants" (184, 187). A run of more than 64
 *   records at one position: LCTY_ERR_UNSUPPORTED naming it. The set stays as it was; more loci may be added and merged again. */
#define LCTY_GTVCF_REF      0xFFFFFFFFu   /* a column of lcty_gtvcf_columns: the reference genome itself, allele 0 everywhere */
#define LCTY_GTVCF_ABSENT   INT64_MIN     /* a fixed-point feature that is absent or NaN */
#define LCTY_GTVCF_QUAL     1u
#define LCTY_GTVCF_READS    2u
#define LCTY_GTVCF_UNEXPL   4u
#define LCTY_GTVCF_WDIST    8u
#define LCTY_GTVCF_WARN     16u
#define LCTY_GTVCF_ALL      31u
#define LCTY_GTVCF_UPSTREAM 14u           /* reads:unexpl:wdist, what into_vcf.py writes */
typedef struct lcty_gtvcf lcty_gtvcf;
typedef struct lcty_gtvcf_locus_in {
    const char* locus; const char* chrom; uint64_t contig_len;
    uint32_t contig_ix, start, end, _pad0;
    uint32_t n_recs, n_haps;
    const uint32_t* pos; const uint32_t* ref_len; const uint32_t* rec_allele; const uint64_t* allele_off; const uint8_t* allele_bytes; const int16_t* gt;
    const uint64_t* id_off; const uint8_t* id_bytes;
    const uint32_t* pred_off; const uint32_t* pred_col;
    const int64_t* qual10; const int64_t* reads; const int64_t* unexpl; const int64_t* wdist5;
    const uint64_t* warn_off; const char* warn;
    int32_t want_calls, _pad1;
} lcty_gtvcf_locus_in;
typedef struct lcty_gtvcf_stats {
    uint64_t n_records, n_samples, n_slots, n_predicted, header_bytes, text_bytes, bytes_h2d, bytes_d2h;
    /* wall time per stage with the stream drained at its end */
    double   upload_ms, cells_ms, merge_ms, widths_ms, write_ms, download_ms, total_ms;
} lcty_gtvcf_stats;
typedef struct lcty_gtvcf_out {
    char* text; uint64_t text_len;
    uint64_t* line_off; uint64_t n_lines;
    int16_t* calls; uint64_t n_slots;                               /* lcty_gtvcf_add_locus with want_calls */
    /* lcty_gtvcf_merge: per line the contig's index, pos and len(REF); the records joined to another; the contigs of the header */
    uint32_t* line_contig; uint32_t* line_pos; uint32_t* line_ref_len; uint64_t n_joined;
    char* contigs; uint64_t contigs_len; uint32_t n_contigs, _pad0;
    uint32_t* contig_ix;
    lcty_gtvcf_stats stats;
} lcty_gtvcf_out;
#define LCTY_RES_CALLED      0
#define LCTY_RES_NO_GENOTYPE 1             /* the `*` row */
#define LCTY_RES_MISSING     2             /* the `?` row */
#define LCTY_RES_UNKNOWN     (-1)          /* what a failed lcty_res_summary_read leaves: no row may be written from it */
typedef struct lcty_res_summary {
    char* genotype; char* warnings;
    int64_t qual10, reads, unexpl, wdist5;
    int32_t state, _pad0;
} lcty_res_summary;
typedef struct lcty_predictions {
    uint64_t n_rows;
    char* text; uint64_t text_len;
    uint64_t* sample_off; uint64_t* locus_off; uint64_t* genotype_off; uint64_t* warn_off;
    int64_t* qual10; int64_t* reads; int64_t* unexpl; int64_t* wdist5;
    uint64_t* samples_off; uint64_t n_samples;
} lcty_predictions;
int32_t lcty_res_summary_read(const char* path, lcty_res_summary* out);
void    lcty_res_summary_free(lcty_res_summary* out);
int32_t lcty_predictions_csv_write(const char* path, uint64_t n_rows, const char* const* sample, const char* const* locus, const lcty_res_summary* rows);
int32_t lcty_predictions_csv_read(const char* path, lcty_predictions* out);
void    lcty_predictions_free(lcty_predictions* out);
int32_t lcty_gtvcf_columns(const lcty_vcf_view* view, const char* genome_name, uint32_t n_names, const char* names, uint32_t* cols);
int32_t lcty_gtvcf_fixed_print(int64_t value, uint32_t decimals, int32_t pad, char* out, uint64_t cap, uint64_t* len);
int32_t lcty_gtvcf_fixed_parse(const char* text, uint32_t decimals, int64_t* value);
int32_t lcty_gtvcf_header(uint32_t n_contigs, const char* contigs, const uint64_t* contig_len, uint32_t n_samples, const char* samples,
                          char* out, uint64_t cap, uint64_t* len);
int32_t lcty_tbi_write(const char* path, uint32_t n_contigs, const char* contigs, uint64_t n_records, const uint32_t* contig_ix,
                       const uint32_t* pos, const uint32_t* ref_len, const uint64_t* line_off, const uint64_t* block_off, uint64_t n_blocks);
int32_t lcty_gtvcf_create(lcty_ctx* ctx, const char* samples, uint32_t n_samples, uint32_t field_mask, lcty_gtvcf** out);
void    lcty_gtvcf_destroy(lcty_gtvcf* set);
int32_t lcty_gtvcf_add_locus(lcty_gtvcf* set, const lcty_gtvcf_locus_in* in, lcty_gtvcf_out* out);
int32_t lcty_gtvcf_merge(lcty_gtvcf* set, lcty_gtvcf_out* out);
void    lcty_gtvcf_out_free(lcty_gtvcf_out* out);

/* ---- basis haplotypes (locityper augment, the basis step: DB/loci/<locus>/haplotypes-basis[.TAG].fa.gz) ------------------------------
 * construct_dominant_set -> inner_construct_dominant_set -> Cigar::locally_similar -> find_dominating_set (src/command/augment.rs:258-396,
 * src/seq/cigar.rs:656-751, src/algo/dom_set.rs) on buffers: the pairwise haplotype alignments as lcty_paf_read returns them (the
 * arguments of lcty_locus_set_hap_alns) and the haplotype lengths. The ids a basis holds are what lcty_locus_build_map_index takes.
 * Out of scope: lock files and rerun modes of augment. (The PAF itself: lcty_align_haplotypes; prune: lcty_db_prune_locus, both below.)
 * Integer work: the bit rows equal the reference's bit for bit. Differences, on purpose: a contig not longer than the window has ONE
 * window (the reference's `l - window`, augment.rs:323, underflows there); the entries are those lcty_paf_read keeps (full length, forward
 * strand); the reference solves the covering problem with SCIP, so only the SIZE of the optimum can be compared, not which optimum.
 *
 * lcty_basis_windows: for every entry (query id1, target id2, id1 != id2, with a CIGAR of M = X I D) and both of its sides — IN_QUERY
 *   on contig id1, the reference form on contig id2 — the windows [s, s + window), s = t * step, whose edit count is at most
 *   floor(window * divergence), and the last window at len - window (index ceil((len - window) / step)): bit `other` of row
 *   (contig, window). A side not longer than the window counts for window 0 iff (aln_len - n_matches) / aln_len <= divergence (1.0 when
 *   aln_len == 0): update_bitarray, augment.rs:291-312. Every row starts with its own contig's bit. lengths[n_alleles];
 *   leave_out (may be NULL) [n_alleles]: != 0 = --basis-lo, the contig has no rows, entries that name it are skipped, ids stay those of
 *   the full set. win_off[n_alleles + 1]: first row of every contig; *rows [win_off[n_alleles]][ceil(n_alleles / 32)] 32-bit words, bit
 *   i of a row at word i / 32, bit i % 32; released with lcty_io_free. One wavefront per (entry, side); the entries stream through the
 *   device in batches (a quarter of the free device memory; lcty_ctx_set_knob "basis_batch_words" = CIGAR words per batch).
 *   A CIGAR with another operation, or one that does not cover its contig's length: LCTY_ERR_INVALID_DATA.
 * lcty_basis_constraints: the distinct rows (the HashSet of augment.rs:341-344) in a fixed order — by number of bits, then by content —
 *   and with minimal != 0 only the rows that contain no other row (a presolve of ours: a row that contains another is implied by it).
 *   *out [*n_out][ceil(n_alleles / 32)], released with lcty_io_free.
 * lcty_basis_select: find_dominating_set: the fewest haplotypes that hit every row, by a host branch and bound (no device is used).
 *   ids[n_alleles] (the first *n_ids filled, ascending), *bound = a proven lower bound of the size, *optimal = 1 when *n_ids == *bound.
 *   node_limit (0 = 2 000 000) reached: the best cover found, *optimal = 0 — the reference, too, only logs a status other than optimal
 *   and takes the best solution (dom_set.rs:26-30). The same input gives the same ids. A row without a bit: LCTY_ERR_INVALID_INPUT.
 * lcty_basis_build: the three in one call, the rows staying on the device between the first two.
 * lcty_basis_tag: construct_basis_tag (augment.rs:259-279): "x" fmt_signif(divergence, 5), "-global" for window == UINT32_MAX, else
 *   "-w" window ["-s" step when step != 0] as PrettyU32 prints them (1000 -> 1k), "-lo" names joined by commas (leave_out: n_leave_out
 *   0-terminated names one after the other). 128 characters or more: LCTY_ERR_RUNTIME, as there. */
typedef struct lcty_basis_params {
    double   divergence;          /* 0.01 (augment.rs:59) */
    uint32_t window;              /* 250 (augment.rs:60); UINT32_MAX = global */
    uint32_t step;                /* 0 = not given: max(window >> 1, 1) (augment.rs:320) */
    uint32_t minimal;             /* 1: lcty_basis_build reduces the rows to the minimal ones before the search; 0: the distinct rows as they are */
    uint32_t _pad0;
    uint64_t node_limit;          /* 2 000 000 nodes of the search */
} lcty_basis_params;
typedef struct lcty_basis_stats {
    uint64_t n_entries, n_walks, n_batches;                /* entries taken; (entry, side) walks; batches they travelled in */
    uint64_t n_rows_raw, n_rows_unique, n_rows_minimal;    /* rows per stage (minimal == unique where the presolve is off) */
    uint64_t n_forced, n_nodes;                            /* haplotypes fixed by rows of one bit; nodes of the search */
    uint64_t bytes_h2d, bytes_d2h;
    /* wall time per stage with the stream drained at its end (transfers included) */
    double   windows_ms, dedup_ms, subsume_ms, search_ms, total_ms;
} lcty_basis_stats;

void    lcty_basis_params_default(lcty_basis_params* params);
int32_t lcty_basis_windows(lcty_ctx* ctx, uint32_t n_alleles, const uint32_t* lengths, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2,
                           const uint32_t* n_matches, const uint32_t* aln_len, const uint64_t* cigar_off, const uint32_t* cigar,
                           const uint8_t* leave_out, const lcty_basis_params* params, uint64_t* win_off, uint32_t** rows, lcty_basis_stats* stats);
int32_t lcty_basis_constraints(lcty_ctx* ctx, uint32_t n_alleles, uint64_t n_rows, const uint32_t* rows, int32_t minimal, uint64_t* n_out,
                               uint32_t** out, lcty_basis_stats* stats);
int32_t lcty_basis_select(uint32_t n_alleles, uint64_t n_rows, const uint32_t* rows, uint64_t node_limit, uint32_t* ids, uint32_t* n_ids,
                          uint32_t* bound, int32_t* optimal, uint64_t* nodes);
int32_t lcty_basis_build(lcty_ctx* ctx, uint32_t n_alleles, const uint32_t* lengths, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2,
                         const uint32_t* n_matches, const uint32_t* aln_len, const uint64_t* cigar_off, const uint32_t* cigar,
                         const uint8_t* leave_out, const lcty_basis_params* params, uint32_t* ids, uint32_t* n_ids, uint32_t* bound,
                         int32_t* optimal, lcty_basis_stats* stats);
int32_t lcty_basis_tag(const lcty_basis_params* params, const char* leave_out, uint32_t n_leave_out, char* out, uint64_t cap);

/* ---- pairwise haplotype alignments (locityper align --transitive 0: DB/loci/<locus>/haplotypes.paf.gz) ---------------------------------
 * The backbone strategy of src/seq/align.rs on buffers. For a requested pair the reference is sequence ref_id (entry1) and the query
 * sequence query_id (entry2): process_pair, 627-679.
 *   divergence  um / md = jaccard_distance of the two minimizer lists = lcty_db_divergences (unless skip_div). The pair is aligned iff
 *               md <= thresh_div, or <= against_div when either sequence carries the `against` flag (646-648); a pair that is not
 *               still has its PAF line (`0 0 255`). thresh_div == 0 means "never align" (Params::validate, 67-89: the ks are
 *               cleared); a pair that passes all the same — skip_div, or an `against` pair under against_div — is LCTY_ERR_RUNTIME
 *               "No alignment found", as align_multik ends there (316).
 *   stage A     backbone matches (precompute_kmers, get_kmer_matches; 102-120, 202-224): every (pos1, pos2) whose non-canonical k-mers
 *               are equal, sorted. 5 <= k <= LCTY_ALIGN_MAX_K = 127 = U256::MAX_KMER_SIZE (kmers.rs:43: BITS / 2 - 1). Exact: windows
 *               are found by a 64-bit hash, and every candidate is compared base by base before it counts. More than 2^24 matches of
 *               one pair and k: LCTY_ERR_UNSUPPORTED (nothing is truncated).
 *   stage B     LCSk++ (bio::alignment::sparse::lcskpp, called at 255; Pavetic, Zuzic, Sikic 2014): over the matches m = (i, j),
 *               dp(m) = max of k; dp(m') + 1 where m' = (i - 1, j - 1) is a match; k + max dp(m'') over the matches with i'' + k <= i
 *               and j'' + k <= j. The chain score is max dp, the path the predecessors back from the argmax. The SCORE is the
 *               reference's; which optimal path comes back is fixed here: the lowest match index wherever values tie.
 *   stage C     the walk of align_from_backbone (262-286) with smart_align (wfa.rs:280-321; threshold max_gap): an empty side is a
 *               plain I or D, a side longer than max_gap takes align_simple, equal lengths <= 3 are compared base by base, anything
 *               else takes the exact gap-affine aligner — accuracy level 9 puts no step limit on WFA. Here that is the Gotoh recurrence
 *               of alignment recovery with its tie rule. A stretch beyond its largest scratch level (16 383 bases a side or 2^26 cells;
 *               knob align_dp_cells) takes align_simple, as the reference does when WFA drops an alignment (wfa.rs:234-237), and is
 *               counted in stats.n_dropped: never an error.
 *   per pair    align_multik (294-318): the best score over backbone_ks, the first k on a tie; n_matches, aln_len, NM, AS as 652-664.
 * Differences, on purpose: (1) no transitive acceleration: every aligned pair has its backbone alignment; (2) a window with a byte
 * outside ACGT is not a backbone k-mer (the reference makes all such windows equal to each other, UNDEF); (3) in the gap fill any byte
 * outside ACGT is N and N equals N; (4) a sequence shorter than k has no k-mers and the pair is one stretch (the reference indexes an
 * empty buffer, 109); (5) which optimal chain and which co-optimal alignment of a stretch: the fixed tie rules above; (6) accuracy
 * levels below 9 and penalties other than 4 / 6 / 1 are not offered (LCTY_ERR_UNSUPPORTED); (7) equal neighbouring CIGAR operations
 * are merged (the reference's push_unchecked can write `5=25=`): the same alignment and score.
 *
 * lcty_align_haplotypes: pairs are taken and returned in input order; they stream through the device in batches sized from the free
 *   memory (knob align_batch_pairs), the k-mer index is built once per call. against: u8[n_seqs] or NULL. out: per pair aligned,
 *   n_matches, aln_len, nerrs, score (AS), best_k, um, md (0 with skip_div), cigar_off[n_pairs + 1] and cigar — raw BAM words with
 *   = X I D, what lcty_locus_set_hap_alns and lcty_basis_build take (id1 = query_id, id2 = ref_id). Released with lcty_align_out_free.
 *   ref_id == query_id, a pair given twice (in either order), an id out of range: LCTY_ERR_INVALID_INPUT.
 * lcty_align_all_pairs: the order of TriangleMatrix::indices — rows i, then j > i, i the reference: load_pairs with --all
 *   (command/align.rs:264-266). ref_id, query_id [n (n - 1) / 2].
 * lcty_align_backbone: one pair and one k, every stage's output: matches [2 n_matches] (pos1, pos2), the chain score, the path as
 *   match indices, the CIGAR and its score. Released with lcty_align_backbone_out_free.
 * lcty_paf_write_text (host): the header line of command/align.rs:385-387 (accuracy=9) and one line per pair as process_pair 639-677
 *   writes it; qv is `inf` when dv is 0. names: n_seqs 0-terminated names one after the other. Called twice: out = NULL sizes
 *   (*needed), then cap >= *needed. `haplotypes.paf.gz` = this text through lcty_io_write_gz. */
#define LCTY_ALIGN_MAX_K 127u
typedef struct lcty_align_params {
    uint32_t div_k, div_w;            /* 15, 15 */
    int32_t  skip_div;                /* 0 */
    uint32_t n_backbone_ks;           /* 3 */
    double   thresh_div, against_div; /* 1.0, 1.0 */
    uint32_t backbone_ks[8];          /* 25, 51, 101 */
    uint32_t max_gap;                 /* 10000 */
    int32_t  mismatch, gap_open, gap_extend;   /* 4, 6, 1 (Penalties::default, wfa.rs:30-38); anything else: LCTY_ERR_UNSUPPORTED */
} lcty_align_params;
typedef struct lcty_align_out {
    uint64_t  n_pairs;
    uint8_t*  aligned;                /* [n_pairs] 0: skipped by its divergence */
    uint32_t* n_matches; uint32_t* aln_len; uint32_t* nerrs;
    int32_t*  score;
    uint32_t* best_k;
    uint32_t* um; double* md;
    uint64_t* cigar_off; uint32_t* cigar;
} lcty_align_out;
typedef struct lcty_align_backbone_out {
    uint64_t  n_matches; uint32_t* matches;
    uint32_t  chain_score, path_len; uint32_t* path;
    uint32_t  n_cigar; int32_t score; uint32_t* cigar;
    uint32_t  n_dropped, _pad0;
} lcty_align_backbone_out;
typedef struct lcty_align_stats {
    uint64_t n_aligned, n_skipped, n_dropped;      /* pairs aligned / skipped by divergence; stretches dropped to align_simple */
    uint64_t n_kmer_matches, n_chain_points;       /* over all (pair, k) */
    uint64_t n_trivial, n_simple, n_small_dp, n_general_dp;   /* stretches by route; small / general DP are SIZE classes (both sides <= 7, or not) of one aligner */
    uint64_t dp_cells, n_batches, n_level[3];      /* cells of the exact aligner; batches; (pair, k) tasks per scratch level */
    uint64_t bytes_h2d, bytes_d2h;
    /* wall time per stage with the stream drained at its end: divergences, k-mer index, matches, chains, gap fill, best k + download */
    double   div_ms, index_ms, match_ms, chain_ms, fill_ms, select_ms, total_ms;
} lcty_align_stats;

void    lcty_align_params_default(lcty_align_params* params);
int32_t lcty_align_all_pairs(uint32_t n_seqs, uint32_t* ref_id, uint32_t* query_id);
int32_t lcty_align_haplotypes(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref_id,
                              const uint32_t* query_id, const uint8_t* against, const lcty_align_params* params, lcty_align_out* out,
                              lcty_align_stats* stats);
void    lcty_align_out_free(lcty_align_out* out);
int32_t lcty_align_backbone(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref, uint32_t query, uint32_t k,
                            const lcty_align_params* params, lcty_align_backbone_out* out, lcty_align_stats* stats);
void    lcty_align_backbone_out_free(lcty_align_backbone_out* out);
int32_t lcty_paf_write_text(const lcty_align_params* params, uint32_t n_seqs, const char* names, const uint64_t* seq_off, uint64_t n_pairs,
                            const uint32_t* ref_id, const uint32_t* query_id, const lcty_align_out* res, char* out, uint64_t cap, uint64_t* needed);

/* ---- transitive haplotype alignments (locityper align --tr-div D, D > 0: the default route of the tool, D = 0.01) ---------------------
 * lcty_align_haplotypes_transitive = lcty_align_haplotypes with the single-thread TransitiveStrategy of src/seq/align.rs:452-514 run
 * over the pairs in input order (the multi-thread form is racy by its own comment, 581-583, and defines nothing). State: closest[q] =
 * (reference id, that pair's CIGAR, its dv), and the finished CIGARs with their direction (DirectedCigar, 428-450). For the pair
 * (k = ref, i = query):
 *   route 2     closest[k] = (j, ..) exists and {i, j} is aligned: i-k is composed of i-j and j-k through j (first clause, 481-484);
 *   route 3     else closest[i] = (j, ..) exists and {k, j} is aligned: the same through that j (second clause, 485-488);
 *   route 1     else the backbone alignment, exactly as lcty_align_haplotypes makes it;
 *   save        dv = nerrs / aln_len in f64 (process_pair 652-665); the CIGAR is kept; if dv <= transitive_div and closest[i] is empty
 *               or has a strictly greater dv, closest[i] = (k, CIGAR, dv) (save_cigar, 504-513).
 * A pair skipped by its minimizer divergence (route 0) reads and writes nothing. transitive_div <= 0, or fewer than 16 pairs in the
 * call (align.rs:784): every pair goes the backbone route and the result is lcty_align_haplotypes' bit for bit (n_rounds 0).
 * The composed CIGAR is Cigar::find_transitive_alignment (cigar.rs:1389-1414) = transfer_alignment::<true> (1248-1368) as written: both
 * full_sequence_match shortcuts (they return before optimize), the four direction combinations, anchors of transitive_anchor equal
 * bases with ANCHOR_MARGIN 5, smart_align with max_gap for every stretch between anchors and for the tail, Cigar::optimize(1000, 51)
 * at the end. Its score is calculate_score of the CIGAR (wfa.rs:87-99), its best_k 0. Aligner, tie rules, N handling and the merging of
 * equal neighbouring operations are those of the section above (differences 2-7); merging is applied throughout: the CIGARs the walk
 * reads are the merged ones this library returns, and optimize looks for its anchors in the merged walk. A stretch beyond the largest
 * scratch level takes align_simple and counts in n_dropped, as there. Of the four direction combinations three can occur: the CIGAR of
 * closest[k] always has k as its query, so "j-k with k the reference" meets "i-j with i the reference" in neither clause (the kernels take it all the same; no test reaches
 * that path on the device).
 * Schedule: rounds. A round is the longest prefix of the remaining pairs in which no pair reads a cell an earlier pair of the prefix
 * writes — read: closest[k], closest[i] and the CIGAR cells its clause tests; written: its own CIGAR cell and closest[i] (whatever dv
 * turns out to be). With lcty_align_all_pairs a round is one row of the triangle. The host decides a round from its mirror of closest
 * (id, dv) and of which cells exist; the round's backbone pairs go through the usual batches, its transitive pairs through the
 * transitive kernels (one lane per pair: plan, fill per scratch level, optimize, counts; the walk and optimize write into per-round
 * temporaries sized by the plan's bounds, which are not part of the store's budget); finished CIGARs are gathered into one store on the
 * device (knob align_cigar_store_mb), only the counts of a round come back, the store is downloaded once at the end.
 * out: as lcty_align_haplotypes. tr_out: per pair route (0 skipped, 1 backbone, 2 first clause, 3 second clause) and via (j, or
 * UINT32_MAX); released with lcty_align_tr_out_free. Input errors are those of lcty_align_haplotypes; transitive_div > 1 or NaN and
 * transitive_anchor 0 are LCTY_ERR_INVALID_INPUT. */
typedef struct lcty_align_tr_params { double transitive_div; uint32_t transitive_anchor; uint32_t _pad0; } lcty_align_tr_params;  /* 0.01, 101 */
typedef struct lcty_align_tr_out   { uint8_t* route; uint32_t* via; } lcty_align_tr_out;
typedef struct lcty_align_tr_stats {
    uint64_t n_rounds, n_accelerated, n_shortcut, n_tr_stretches, tr_dp_cells, store_bytes;   /* shortcut: a full_sequence_match copy; stretches, cells: of the transitive kernels */
    double   plan_ms, tr_fill_ms, optimize_ms, count_ms;   /* wall time with the stream drained: both planning passes, the walk, optimize, counts + gather into the store */
} lcty_align_tr_stats;
void    lcty_align_tr_params_default(lcty_align_tr_params* params);
int32_t lcty_align_haplotypes_transitive(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs,
                                         const uint32_t* ref_id, const uint32_t* query_id, const uint8_t* against, const lcty_align_params* params,
                                         const lcty_align_tr_params* tr_params, lcty_align_out* out, lcty_align_tr_out* tr_out,
                                         lcty_align_stats* stats, lcty_align_tr_stats* tr_stats);
void    lcty_align_tr_out_free(lcty_align_tr_out* out);

/* ---- pruning similar haplotypes (locityper prune: DB/loci/<locus>/ -> a thinned DB/loci/<locus>/, all_haplotypes.nwk.gz) ----------------
 * process_locus + prune_files (src/command/prune.rs:471-582) on buffers, for one locus. Out of scope: *.bed copies, `success` and lock
 * files, rerun modes, --subset-loci and the loop over loci.
 *
 * lcty_paf_divergences (host): load_divergences (prune.rs:159-230) on the decompressed text of haplotypes.paf (lcty_io_read_file gives
 *   it). Lines end at '\n'; white space at the end of a line is dropped before it is split at tabs. Per line: columns 1 and 6 are the
 *   two names; the first column from the 13th on that starts with `<field>:` is the tag, its value is what follows the two type
 *   characters (`dv:f:0.01` -> 0.01), parsed as Rust's str::parse::<f64> does (decimal, exponent, inf / infinity / nan in any case,
 *   an optional sign; no white space, no hexadecimal). Skipped, as there: a line naming a contig the locus does not have (checked
 *   column 1 first, so '#' lines and empty lines fall here), self pairs, lines without the tag, negative values (n_negative), a
 *   second DIFFERENT value for a pair (n_conflicting; the first stays). A tag whose value does not parse: LCTY_ERR_INVALID_DATA; so
 *   is a line of a known contig with fewer than 6 columns, or of two known contigs with fewer than 12 (the reference indexes past the
 *   end there). Pairs without a value become repl_missing (n_missing; missing_i < missing_j is the LAST such pair in triangle order,
 *   the one the reference names in its warning; UINT32_MAX without one); the caller passes 10 x threshold, or +inf with n_clusters
 *   (process_locus:537). All pairs missing (n < 2 included): LCTY_ERR_INVALID_INPUT. field NULL = "dv"; a field with ':' is
 *   LCTY_ERR_INVALID_INPUT (Args::validate, 63). tri[n (n - 1) / 2]: TriangleMatrix's linear order (src/ext/trimat.rs:43-46: rows
 *   i, then j > i). A caller that has lcty_align_haplotypes' result passes nerrs / aln_len per pair instead and never makes the text.
 * lcty_prune_multiplicities (host): DiscardedHaplotypes::load (src/seq/contigs.rs:488-528) on the text of the locus's old
 *   discarded_haplotypes.txt, as far as pruning uses it: mult[n] = 1 + the number of names listed for the contig (add_identical,
 *   prune.rs:251-260, counts `~` entries as well). A line with fewer than 3 columns: LCTY_ERR_INVALID_INPUT. text NULL / len 0: all 1.
 *   *all_identical (may be NULL): 0 when a line has `~` (the reference then warns that the tree will be inaccurate).
 * lcty_prune_linkage (device): complete-linkage clustering of the triangle — what the reference asks of kodama::linkage(..,
 *   Method::Complete) (prune.rs:375). THE CONTRACT, which is this library's own definition: leaves carry the labels 0 .. n - 1, step
 *   s creates label n + s; at every step, among the active clusters, the pair (a, b), a < b BY LABEL, with the smallest dissimilarity
 *   is merged, on equal dissimilarities the smallest a, then the smallest b; the new cluster's dissimilarity to every other cluster x
 *   is max(D[a][x], D[b][x]). steps[n - 1] = {cluster1 < cluster2, dissimilarity, size}. Every dissimilarity is one of the input
 *   values, bit for bit; +inf is a legal input, NaN is LCTY_ERR_INVALID_INPUT; the steps come out in non-decreasing order. Where all
 *   input values are distinct the dendrogram is unique (and is SciPy's linkage(.., 'complete'), whose output kodama documents as its
 *   own); under ties equality with the reference is NOT claimed: kodama is not in the reference tree.
 *   n = 1: zero steps. n > LCTY_PRUNE_MAX_N: LCTY_ERR_UNSUPPORTED, before anything is read or allocated.
 *   The full symmetric matrix lives in device memory (8 n^2 bytes: 512 MB at n = 8 192), built from the triangle by a kernel of
 *   many workgroups; per matrix row the minimum and its partner of smallest label are cached; the n - 1 merges run in ONE launch of
 *   ONE workgroup (no cross-workgroup wait of any kind): argmin over the cached rows, new row and column as the elementwise maximum,
 *   rescan of the rows whose cached partner was merged (one wavefront per row).
 * lcty_prune_cluster (device): cluster_haplotypes (prune.rs:350-427) without its texts: linkage, the cut, the clusters and their
 *   representatives. Cut: with n_clusters != 0 the threshold is steps[n - n_clusters - 1].dissimilarity, 0 when n <= n_clusters
 *   (select_cut_threshold, 327-347); a step is above the cut iff dissimilarity > threshold. Clusters in the order the reference's
 *   loop meets them (by step, child 1 before child 2, the root last when no step exceeded the cut), members in merge_and_clear order
 *   (the first child's, then the second's). Representatives: select_representative (276-304), one workgroup per cluster of more
 *   than one member, one thread per member x accumulating over y in member order exactly as buf[x] is fed there: epsilon =
 *   max(1e-6 min(tri), 1e-12) (1e-12 when n = 1), div = epsilon + D, PowerMean::update_mult (src/math/mod.rs:288-295) with powi as
 *   compiler-rt's __powidf2 and nothing fused: the accumulators equal the reference's bit for bit for min, max and every non-zero
 *   power; power 0 uses the device's log (no bit equality claimed). The representative is the first minimum of the accumulators,
 *   the first maximum for negative powers (src/ext/vec.rs:223-232). mult[n] (NULL: all 1). power: -128 .. 127, LCTY_PRUNE_POWER_MIN
 *   or LCTY_PRUNE_POWER_MAX. threshold < 0 or NaN: LCTY_ERR_INVALID_INPUT. Released with lcty_prune_out_free.
 * lcty_prune_texts (host): the Newick text (Cluster::new / add_identical / merge_and_clear, 243-274: a leaf is its name, with old
 *   discarded names `(name:0,other:0,...)`, a merge `(A:{:.8},B:{:.8})` with branch 0.5 (div - child.div), the root + ";\n") and the
 *   new discarded_haplotypes.txt: the old text, then `repr ~ a, b, c\n` per cluster of more than one member (write_discarded_haplotypes,
 *   306-323). names: n 0-terminated names one after the other. *newick, *discarded released with lcty_io_free; *discarded_len 0: no file.
 * lcty_db_prune_locus: process_locus + prune_files on the DECOMPRESSED contents of the locus directory: paf (required), kmers (both
 *   KmerCounts blocks of kmers.bin.*; NULL: none), distances (distances.bin; NULL: none), discarded (the old discarded_haplotypes.txt;
 *   NULL: none; not read with skip_tree, as there, so its lines are not carried over then). Out: newick (unless skip_tree); with
 *   only_tree nothing else; discarded (old + new lines; empty: no file), keep (sorted ids). If every haplotype is kept, unchanged = 1
 *   and the caller copies its files as they are (copy_output_files). Otherwise fasta (the kept haplotypes in id order, one line per
 *   sequence: fastx::write_fasta), kmers (both blocks thinned, KmerCounts::thin_out + save; empty with LCTY_PRUNE_WARN_KMERS when the
 *   blocks do not match the haplotypes, as prune.rs:494-503), distances (TriangleMatrix::thin_out + write_divergences) and paf
 *   (prune_paf, src/seq/paf.rs:237-267: '#' lines kept, a line kept iff both names are kept, fewer than 7 columns LCTY_ERR_INVALID_DATA).
 *   The containers (.gz, .br) are the writers' business. Released with lcty_prune_files_free.
 * lcty_prune_thin (host): that second half alone, for ids the caller has: fasta, kmers, distances, paf of `keep` (ascending) into *out. */
#define LCTY_PRUNE_MAX_N      16384u
#define LCTY_PRUNE_POWER_MIN  INT32_MIN          /* PowerMean::Min */
#define LCTY_PRUNE_POWER_MAX  INT32_MAX          /* PowerMean::Max */
#define LCTY_PRUNE_WARN_KMERS 1u                 /* the k-mer counts do not match the haplotypes: no kmers output */
typedef struct lcty_paf_div_stats {
    uint64_t n_missing, n_negative, n_conflicting;
    uint32_t missing_i, missing_j;
} lcty_paf_div_stats;
typedef struct lcty_prune_step {
    uint32_t cluster1, cluster2;      /* labels, cluster1 < cluster2 */
    double   dissimilarity;
    uint32_t size, _pad0;
} lcty_prune_step;
typedef struct lcty_prune_params {
    double   threshold;               /* 0.0002 (prune.rs:49) */
    uint32_t n_clusters;              /* 0 = none: cut at threshold */
    int32_t  power;                   /* 2 (prune.rs:51) */
    int32_t  only_tree, skip_tree;    /* 0, 0: lcty_db_prune_locus only */
} lcty_prune_params;
typedef struct lcty_prune_stats {
    uint64_t n_rescans, n_rep_pairs;  /* rows scanned again by the merge loop; pair terms of the representatives kernel */
    uint64_t bytes_h2d, bytes_d2h, matrix_bytes;
    /* wall time per stage with the stream drained at its end: matrix + row caches, the merge loop, representatives, host work, whole call */
    double   build_ms, merge_ms, repr_ms, host_ms, total_ms;
} lcty_prune_stats;
typedef struct lcty_prune_out {
    uint32_t  n, n_clusters;          /* n_clusters: clusters found (= haplotypes kept) */
    double    threshold, epsilon;     /* the cut used; the epsilon of the representatives */
    lcty_prune_step* steps;           /* [n - 1] */
    uint32_t* keep_ids;               /* [n_clusters] ascending */
    uint32_t* cluster_off;            /* [n_clusters + 1] into members / acc */
    uint32_t* members;                /* [n] */
    uint32_t* repr;                   /* [n_clusters] */
    double*   acc;                    /* [n] the accumulators, beside members (0 for clusters of one) */
    lcty_prune_stats stats;
} lcty_prune_out;
typedef struct lcty_prune_files {
    uint8_t* newick;    uint64_t newick_len;       /* text of all_haplotypes.nwk (empty with skip_tree) */
    uint8_t* discarded; uint64_t discarded_len;    /* discarded_haplotypes.txt (empty: no file) */
    uint8_t* fasta;     uint64_t fasta_len;        /* text of haplotypes.fa */
    uint8_t* kmers;     uint64_t kmers_len;        /* kmers.bin: both blocks */
    uint8_t* distances; uint64_t distances_len;    /* distances.bin (empty: there was none) */
    uint8_t* paf;       uint64_t paf_len;          /* text of haplotypes.paf */
    uint32_t* keep;     uint32_t n_keep;
    int32_t  unchanged;                            /* every haplotype kept: fasta, kmers, distances, paf are empty, the inputs stand */
    uint32_t warn_bits, _pad0;
    double   threshold;
    lcty_paf_div_stats div;
    lcty_prune_stats stats;
} lcty_prune_files;

void    lcty_prune_params_default(lcty_prune_params* params);
int32_t lcty_paf_divergences(const uint8_t* text, uint64_t len, const char* const* names, uint32_t n, const char* field, double repl_missing,
                             double* tri, lcty_paf_div_stats* stats);
int32_t lcty_prune_multiplicities(const char* text, uint64_t len, const char* const* names, uint32_t n, uint32_t* mult, int32_t* all_identical);
int32_t lcty_prune_linkage(lcty_ctx* ctx, uint32_t n, const double* tri, lcty_prune_step* steps, lcty_prune_stats* stats);
int32_t lcty_prune_cluster(lcty_ctx* ctx, uint32_t n, const double* tri, const uint32_t* mult, const lcty_prune_params* params, lcty_prune_out* out);
void    lcty_prune_out_free(lcty_prune_out* out);
int32_t lcty_prune_texts(uint32_t n, const char* names, const char* old_discarded, uint64_t old_len, const lcty_prune_out* res,
                         uint8_t** newick, uint64_t* newick_len, uint8_t** discarded, uint64_t* discarded_len);
int32_t lcty_db_prune_locus(lcty_ctx* ctx, uint32_t n, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const uint8_t* paf,
                            uint64_t paf_len, const uint8_t* kmers, uint64_t kmers_len, const uint8_t* distances, uint64_t distances_len,
                            const char* discarded, uint64_t discarded_len, const char* field, const lcty_prune_params* params,
                            lcty_prune_files* out);
int32_t lcty_prune_thin(uint32_t n, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const uint8_t* paf, uint64_t paf_len,
                        const uint8_t* kmers, uint64_t kmers_len, const uint8_t* distances, uint64_t distances_len, const uint32_t* keep,
                        uint32_t n_keep, lcty_prune_files* out);
void    lcty_prune_files_free(lcty_prune_files* files);

/* ---- a resident genome: its k-mer counts for a locus and its reference windows (lcty_genome.hip) ------------------
 * Replaces JfKmerGetter::new / fetch (src/seq/counts.rs:258-369: `jellyfish query` against a whole-genome database, called for the
 * flanks of expand_locus, command/add.rs:502; every haplotype plus the reference sequence, add.rs:633-636; the background region,
 * command/preproc.rs:1373; the locus sequences of recruit, command/recruit.rs:540) and seq::fetch_seq + standardize
 * (src/seq/mod.rs:26-38, 149). No database of every k-mer is built: a call counts the k-mers of ITS sequences in one pass over the
 * genome, which stays on the device packed at 3 bits a base. Parity with the jellyfish binary is not pinned (there is none to run);
 * the definition is the one below, restated in tests/pyref_kmer_count.py.
 *   Genome: named contigs. A C G T a c g t are the bases (case folded); every other letter seq::standardize accepts (N and the IUPAC
 *   codes, either case) is "not a base"; any other byte is LCTY_ERR_INVALID_DATA naming contig, position and byte, and the genome
 *   is unusable from then on. A k-mer occurrence is k consecutive bases of one contig. count(x) = occurrences whose canonical form
 *   (src/seq/kmers.rs:163-202) equals canonical(x).
 * lcty_genome_append: one contig (continues == 0: `name` is its name), or the next piece of the contig that is open (continues != 0,
 *   name ignored). Pieces of any length give the same genome as one piece. ASCII is uploaded as it is (at link rate from
 *   lcty_host_alloc memory) and packed by a kernel. All positions, one separator per contig included, stay below 2^32 (32-bit
 *   counters cannot wrap): more is LCTY_ERR_UNSUPPORTED before anything is uploaded (knob "genome_max_bases").
 * lcty_genome_load_fasta: a FASTA file, plain or gzip / BGZF, multi-line, \n or \r\n; the name is the header up to the first blank
 *   (src/seq/fastx.rs:417-419). Empty lines are skipped; sequence before the first header is LCTY_ERR_INVALID_DATA.
 * lcty_genome_info / _contig: the contigs in order; name_buf (may be NULL) takes the 0-terminated name, cap its size.
 * lcty_genome_fetch: out[end - start] = the window [start, end) of the contig (0-based) as fetch_seq + standardize leave it: capitals
 *   A C G T, N for everything else. start >= end, end beyond the contig, an unknown name: LCTY_ERR_INVALID_INPUT.
 * lcty_genome_kmer_counts: JfKmerGetter::fetch. Sequence i (seq_off[n_seqs + 1] into seqs, upper-case A C G T only) gets
 *   max(len_i + 1 - k, 0) values at counts[cnt_off[i]..cnt_off[i + 1]); cnt_off[n_seqs + 1] is written, counts is the caller's
 *   (cnt_off[n_seqs] values: sized from the lengths). A value is max(min(count, max_value), 1) with max_value = 65 535 for
 *   counter_bytes >= 2, else 255 (counts.rs:297-303; the floor of 1: 354-355). A sequence with N: LCTY_ERR_RUNTIME "Cannot count
 *   k-mers for sequence with Ns" (326-328); any other byte outside the four capitals: LCTY_ERR_INVALID_INPUT. k even:
 *   LCTY_ERR_INVALID_DATA with the message of 284-286; 1 <= k <= 31 runs; 33 <= k <= 63: LCTY_ERR_UNSUPPORTED. counter_bytes outside
 *   1..8: LCTY_ERR_INVALID_INPUT (292-295). Kernels, on the context's stream, workspace per call: byte check; the distinct canonical
 *   k-mers of the query into an open-addressing table (load <= 0.5); the scan (a thread per LCTY_GENOME_SCAN_RUN k-mer starts of the
 *   packed genome); the gather. Every count is exact. The genome is only read: calls on one genome come from one thread at a time. */
#define LCTY_GENOME_SCAN_RUN 128u
typedef struct lcty_genome lcty_genome;
typedef struct lcty_genome_count_stats {
    uint64_t n_query_kmers, n_distinct, table_slots;   /* values returned; distinct canonical k-mers among them; slots of the table */
    uint64_t n_scanned, n_hits;                        /* genome positions (separators included) the scan went over; lookups that hit */
    uint32_t scan_run, _pad0;                          /* LCTY_GENOME_SCAN_RUN */
    double   table_ms, scan_ms, gather_ms, total_ms;   /* device events: check + table, scan, gather + download; host clock: the call */
} lcty_genome_count_stats;
int32_t lcty_genome_create(lcty_ctx* ctx, lcty_genome** out);
void    lcty_genome_destroy(lcty_genome* genome);
int32_t lcty_genome_append(lcty_genome* genome, const char* name, const uint8_t* bases, uint64_t len, int32_t continues);
int32_t lcty_genome_load_fasta(lcty_ctx* ctx, const char* path, lcty_genome** out);
int32_t lcty_genome_info(const lcty_genome* genome, uint32_t* n_contigs, uint64_t* n_bases);
int32_t lcty_genome_contig(const lcty_genome* genome, uint32_t i, char* name_buf, uint64_t cap, uint64_t* len);
int32_t lcty_genome_fetch(const lcty_genome* genome, const char* contig_name, uint64_t start, uint64_t end, uint8_t* out);
int32_t lcty_genome_kmer_counts(const lcty_genome* genome, uint32_t k, uint32_t counter_bytes, uint32_t n_seqs, const uint8_t* seqs,
                                const uint64_t* seq_off, uint16_t* counts, uint64_t* cnt_off, lcty_genome_count_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* LOCITYPER_HIP_H */
