"""ctypes mirrors of the plain-data structs in include/locityper_hip.h.

Shared by the product binding (api.py), the synthetic-workload generator (synth.py)
and — in tests only — the oracle binding. Field order and types must match the header.
"""
import ctypes as C

import numpy as np

GC_BINS = 101
DEPTH_CACHE = 256
MAX_ALT_CN = 15
NONE_U32 = 0xFFFFFFFF

OK, ERR_INVALID_INPUT, ERR_INVALID_DATA, ERR_RUNTIME, ERR_SOLVER, ERR_UNSUPPORTED = range(6)
TECH_ILLUMINA, TECH_HIFI, TECH_PACBIO, TECH_NANOPORE = range(4)
EDIT_FRACTION, EDIT_PVALUE = 0, 1
READ_GOOD, READ_POORLY_MAPPED, READ_OUT_OF_BOUNDS, READ_FEW_KMERS = range(4)

FLAG_UNMAPPED = 0x4
FLAG_REVERSE = 0x10
FLAG_MATE2 = 0x80
FLAG_SECONDARY = 0x100
FLAG_SUPPL = 0x800

CIGAR_M, CIGAR_I, CIGAR_D, CIGAR_S, CIGAR_H, CIGAR_EQ, CIGAR_X = 0, 1, 2, 4, 5, 7, 8


class Params(C.Structure):
    """model::Params (src/model/mod.rs:64-135)."""
    _fields_ = [
        ("boundary_size", C.c_uint32),
        ("tweak", C.c_int32),
        ("lik_skew", C.c_double),
        ("prob_diff", C.c_double),
        ("unmapped_penalty", C.c_double),
        ("poor_compl", C.c_double),
        ("poor_compl_edit", C.c_double),
        ("compl_weight_bp", C.c_double),
        ("compl_weight_pow", C.c_double),
        ("kmers_weight_bp", C.c_double),
        ("kmers_weight_pow", C.c_double),
        ("min_weight", C.c_double),
        ("filt_diff", C.c_double),
        ("prob_thresh", C.c_double),
        ("alt_cn", C.c_double * MAX_ALT_CN),
        ("n_alt_cn", C.c_uint32),
        ("kmer_soft_thresh", C.c_uint16),
        ("kmer_hard_thresh", C.c_uint16),
        ("complexity_k", C.c_uint8),
        ("dont_skip", C.c_uint8),
        ("strict_subset", C.c_uint8),
        ("_pad0", C.c_uint8),
        ("threads", C.c_uint32),
    ]


class Bg(C.Structure):
    """bg::BgDistr as loaded from distr.gz (src/bg/mod.rs:147-177)."""
    _fields_ = [
        ("op_lnprobs", C.c_double * 5),
        ("edit_alpha", C.c_double),
        ("edit_beta", C.c_double),
        ("ins_n", C.c_double),
        ("ins_p", C.c_double),
        ("depth_n", C.c_double * GC_BINS),
        ("depth_p", C.c_double * GC_BINS),
        ("edit_p1", C.c_double),
        ("edit_p2", C.c_double),
        ("window", C.c_uint32),
        ("neighb", C.c_uint32),
        ("is_paired", C.c_int32),
        ("technology", C.c_int32),
        ("edit_kind", C.c_int32),
        ("_pad0", C.c_uint32),
    ]


BG_REVERSE, BG_SECOND = 1, 2


class BgParams(C.Structure):
    """preproc's background parameters (src/command/preproc.rs:275-294, src/bg/mod.rs:39-46, src/bg/depth.rs:166-180)."""
    _fields_ = [
        ("technology", C.c_int32),
        ("explicit_technology", C.c_int32),
        ("min_mapq", C.c_uint32),
        ("ploidy", C.c_uint32),
        ("max_clipping", C.c_double),
        ("insert_pval", C.c_double),
        ("edit_pval", C.c_double),
        ("window_size", C.c_uint32),
        ("boundary_size", C.c_uint32),
        ("uniq_kmer_perc", C.c_double),
        ("frac_windows", C.c_double),
        ("min_tail_obs", C.c_uint32),
        ("_pad0", C.c_uint32),
        ("tail_var_mult", C.c_double),
        ("subsampling_rate", C.c_double),
    ]


DB_WARN_NEGATIVES_SEEN, DB_WARN_REF_MISMATCH = 1, 2


class DbParams(C.Structure):
    """`locityper target`'s parameters of process_alleles (src/command/add.rs:76-78, 606, 611)."""
    _fields_ = [("div_k", C.c_uint32), ("div_w", C.c_uint32), ("calc_div", C.c_int32), ("only_seqs", C.c_int32)]


class DbCheck(C.Structure):
    """check_divergencies (add.rs:521-543)."""
    _fields_ = [("n_high", C.c_uint64), ("highest", C.c_double), ("highest_i", C.c_uint32), ("highest_j", C.c_uint32)]


class DbStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_minimizers", "n_columns", "n_chunks", "n_fast", "n_walk", "n_sorted_host", "bytes_h2d",
                                          "bytes_d2h", "bitmat_bytes")] + \
               [(n, C.c_double) for n in ("minim_ms", "sort_ms", "sort_host_ms", "index_ms", "tiles_ms", "offt_ms", "host_ms", "total_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DbFiles(C.Structure):
    _fields_ = [("fasta", C.c_void_p), ("fasta_len", C.c_uint64), ("kmers", C.c_void_p), ("kmers_len", C.c_uint64),
                ("distances", C.c_void_p), ("distances_len", C.c_uint64), ("discarded", C.c_void_p), ("discarded_len", C.c_uint64),
                ("kept", C.c_void_p), ("n_kept", C.c_uint32), ("warn_bits", C.c_uint32), ("check", DbCheck), ("stats", DbStats)]


# ---- a locus from a pangenome VCF (lcty_panvcf.hip, the VCF reader of lcty_io.hip) ----
PANVCF_KEPT, PANVCF_UNKNOWN, PANVCF_HAS_N = 0, 1, 2
LOCUS_WARN_VERY_SHORT, LOCUS_WARN_SHORT, LOCUS_WARN_BOUNDARY_DIFFERS = 1, 2, 4


class _Dictable(C.Structure):
    def as_dict(self):
        return {n: (getattr(self, n).as_dict() if hasattr(getattr(self, n), "as_dict") else getattr(self, n)) for n, _ in self._fields_ if not n.startswith("_")}


class VcfView(C.Structure):
    _fields_ = [("n_samples", C.c_uint32), ("n_haps", C.c_uint32), ("n_records", C.c_uint64), ("samples", C.c_void_p), ("samples_len", C.c_uint64),
                ("ploidy", C.c_void_p), ("hap_off", C.c_void_p)]


class VcfRecords(C.Structure):
    _fields_ = [("n_recs", C.c_uint32), ("n_haps", C.c_uint32), ("n_samples", C.c_uint32), ("_pad0", C.c_uint32), ("n_alleles", C.c_uint64),
                ("pool_len", C.c_uint64), ("pos", C.c_void_p), ("ref_len", C.c_void_p), ("rec_allele", C.c_void_p), ("allele_off", C.c_void_p),
                ("allele_bytes", C.c_void_p), ("gt", C.c_void_p), ("phased", C.c_void_p)]


class VcfFetchStats(_Dictable):
    _fields_ = [(n, C.c_uint64) for n in ("n_chunks", "file_bytes", "bytes_read", "blocks_inflated", "bytes_inflated", "lines_walked", "records_kept")] + \
               [(n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_upload", "ms_lines", "ms_heads", "ms_alleles", "ms_gt", "ms_download", "ms_total")]


class PanvcfStats(_Dictable):
    _fields_ = [(n, C.c_uint64) for n in ("bytes_h2d", "bytes_d2h", "n_segments", "out_bytes")] + \
               [(n, C.c_double) for n in ("upload_ms", "rows_ms", "chain_ms", "scan_ms", "gather_ms", "compact_ms", "total_ms")]


class PanvcfOut(C.Structure):
    _fields_ = [("seqs", C.c_void_p), ("seq_off", C.c_void_p), ("names", C.c_void_p), ("names_len", C.c_uint64), ("kept_cols", C.c_void_p),
                ("col_unknown", C.c_void_p), ("col_len", C.c_void_p), ("col_reason", C.c_void_p), ("n_seqs", C.c_uint32), ("n_cols", C.c_uint32),
                ("n_unknown", C.c_uint32), ("n_with_n", C.c_uint32), ("total_overlaps", C.c_uint64), ("n_kept_records", C.c_uint64),
                ("stats", PanvcfStats)]


# ---- a locus's haplotypes as a VCF (lcty_pafvcf.hip) ----
PAFVCF_WARN_REF_SUFFIX, PAFVCF_WARN_PRUNED = 1, 2


class PafvcfStats(_Dictable):
    _fields_ = [(n, C.c_uint64) for n in ("n_variants", "n_unique", "n_merged", "n_shifted", "n_lines_merged", "n_lines_separate", "merged_bytes",
                                          "separate_bytes")] + \
               [(n, C.c_uint32) for n in ("n_missing", "n_bad_len", "warn_bits", "n_samples")] + \
               [(n, C.c_double) for n in ("upload_ms", "variants_ms", "ranges_ms", "table_ms", "text_ms", "total_ms")]


class PafvcfOut(C.Structure):
    _fields_ = [("n_seqs", C.c_uint32), ("_pad0", C.c_uint32)] + [(n, C.c_uint64) for n in ("n_variants", "n_unique", "n_merged", "n_ranges")] + \
               [(n, C.c_void_p) for n in ("var_off", "ref_start", "ref_end", "hap_start", "hap_end", "has_aln", "unique_start", "unique_end", "merged_start",
                                          "merged_end", "allele_ix", "n_alleles", "allele_off", "allele_hap", "allele_start", "allele_len")] + \
               [("merged", C.c_void_p), ("merged_len", C.c_uint64), ("separate", C.c_void_p), ("separate_len", C.c_uint64), ("stats", PafvcfStats)]


# ---- a cohort's genotypes as a phased VCF (lcty_gtvcf.hip) ----
GTVCF_REF = 0xFFFFFFFF
GTVCF_ABSENT = -(1 << 63)
GTVCF_QUAL, GTVCF_READS, GTVCF_UNEXPL, GTVCF_WDIST, GTVCF_WARN = 1, 2, 4, 8, 16
GTVCF_ALL, GTVCF_UPSTREAM = 31, 14


class GtvcfLocusIn(C.Structure):
    _fields_ = [("locus", C.c_char_p), ("chrom", C.c_char_p), ("contig_len", C.c_uint64), ("contig_ix", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32),
                ("_pad0", C.c_uint32), ("n_recs", C.c_uint32), ("n_haps", C.c_uint32)] + \
               [(n, C.c_void_p) for n in ("pos", "ref_len", "rec_allele", "allele_off", "allele_bytes", "gt", "id_off", "id_bytes", "pred_off", "pred_col", "qual10",
                                          "reads", "unexpl", "wdist5", "warn_off", "warn")] + \
               [("want_calls", C.c_int32), ("_pad1", C.c_int32)]


class GtvcfStats(_Dictable):
    _fields_ = [(n, C.c_uint64) for n in ("n_records", "n_samples", "n_slots", "n_predicted", "header_bytes", "text_bytes", "bytes_h2d", "bytes_d2h")] + \
               [(n, C.c_double) for n in ("upload_ms", "cells_ms", "merge_ms", "widths_ms", "write_ms", "download_ms", "total_ms")]


class GtvcfOut(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_uint64), ("line_off", C.c_void_p), ("n_lines", C.c_uint64), ("calls", C.c_void_p),
                ("n_slots", C.c_uint64), ("line_contig", C.c_void_p), ("line_pos", C.c_void_p), ("line_ref_len", C.c_void_p), ("n_joined", C.c_uint64),
                ("contigs", C.c_void_p), ("contigs_len", C.c_uint64), ("n_contigs", C.c_uint32), ("_pad0", C.c_uint32), ("contig_ix", C.c_void_p), ("stats", GtvcfStats)]


RES_CALLED, RES_NO_GENOTYPE, RES_MISSING, RES_UNKNOWN = 0, 1, 2, -1


class VcfContigs(C.Structure):
    _fields_ = [("n_contigs", C.c_uint32), ("_pad0", C.c_uint32), ("names", C.c_void_p), ("names_len", C.c_uint64), ("length", C.c_void_p)]


class ResSummary(C.Structure):
    _fields_ = [("genotype", C.c_void_p), ("warnings", C.c_void_p)] + [(n, C.c_int64) for n in ("qual10", "reads", "unexpl", "wdist5")] + \
               [("state", C.c_int32), ("_pad0", C.c_int32)]


class Predictions(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("text", C.c_void_p), ("text_len", C.c_uint64)] + \
               [(n, C.c_void_p) for n in ("sample_off", "locus_off", "genotype_off", "warn_off", "qual10", "reads", "unexpl", "wdist5", "samples_off")] + \
               [("n_samples", C.c_uint64)]


class ExpandOut(_Dictable):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("attempt", C.c_int32), ("allowed_expansion", C.c_uint32), ("n_attempts", C.c_uint32),
                ("crop_bits", C.c_uint32), ("total_ms", C.c_double)]


class LocusVcfIn(C.Structure):
    _fields_ = [("locus", C.c_char_p), ("contig", C.c_char_p), ("inner_start", C.c_uint32), ("inner_end", C.c_uint32), ("contig_len", C.c_uint32),
                ("win_start", C.c_uint32), ("win_seq", C.c_void_p), ("win_len", C.c_uint64), ("win_counts", C.c_void_p), ("n_win_counts", C.c_uint64),
                ("k", C.c_uint32), ("counter_bytes", C.c_uint32), ("n_recs", C.c_uint32), ("n_cols", C.c_uint32), ("pos", C.c_void_p),
                ("ref_len", C.c_void_p), ("rec_allele", C.c_void_p), ("allele_off", C.c_void_p), ("allele_bytes", C.c_void_p), ("gt", C.c_void_p),
                ("names", C.c_char_p), ("expansions", C.c_void_p), ("n_expansions", C.c_uint32), ("moving_window", C.c_uint32),
                ("unknown_frac", C.c_double), ("overlaps_allowed", C.c_int32), ("_pad0", C.c_int32), ("hap_counts", C.c_void_p),
                ("hap_cnt_off", C.c_void_p)]


class LocusVcfStats(_Dictable):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("attempt", C.c_int32), ("allowed_expansion", C.c_uint32), ("crop_bits", C.c_uint32),
                ("warn_bits", C.c_uint32)] + \
               [(n, C.c_uint32) for n in ("n_cols", "n_haplotypes", "n_unknown", "n_with_n", "n_identical", "n_records")] + \
               [(n, C.c_uint64) for n in ("n_kept_records", "total_overlaps", "shortest")] + \
               [(n, C.c_double) for n in ("filter_ms", "expand_ms", "reconstruct_ms", "build_ms", "total_ms")] + [("recon", PanvcfStats)]


class LocusVcfOut(C.Structure):
    _fields_ = [("files", DbFiles), ("ref_bed", C.c_void_p), ("ref_bed_len", C.c_uint64), ("hap_cols", C.c_void_p), ("n_hap_cols", C.c_uint32),
                ("_pad0", C.c_uint32), ("stats", LocusVcfStats)]


class BasisParams(C.Structure):
    """The basis step of `locityper augment` (src/command/augment.rs:59-61); window 2^32 - 1 = global, step 0 = max(window >> 1, 1)."""
    _fields_ = [("divergence", C.c_double), ("window", C.c_uint32), ("step", C.c_uint32), ("minimal", C.c_uint32), ("_pad0", C.c_uint32),
                ("node_limit", C.c_uint64)]


class BasisStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_entries", "n_walks", "n_batches", "n_rows_raw", "n_rows_unique", "n_rows_minimal", "n_forced",
                                          "n_nodes", "bytes_h2d", "bytes_d2h")] + \
               [(n, C.c_double) for n in ("windows_ms", "dedup_ms", "subsume_ms", "search_ms", "total_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AlignParams(C.Structure):
    """`locityper align`, the backbone strategy (src/seq/align.rs:48-64); penalties other than 4 / 6 / 1 are not offered."""
    _fields_ = [("div_k", C.c_uint32), ("div_w", C.c_uint32), ("skip_div", C.c_int32), ("n_backbone_ks", C.c_uint32),
                ("thresh_div", C.c_double), ("against_div", C.c_double), ("backbone_ks", C.c_uint32 * 8), ("max_gap", C.c_uint32),
                ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32)]


class AlignOut(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("aligned", C.c_void_p), ("n_matches", C.c_void_p), ("aln_len", C.c_void_p), ("nerrs", C.c_void_p),
                ("score", C.c_void_p), ("best_k", C.c_void_p), ("um", C.c_void_p), ("md", C.c_void_p), ("cigar_off", C.c_void_p),
                ("cigar", C.c_void_p)]


class AlignBackboneOut(C.Structure):
    _fields_ = [("n_matches", C.c_uint64), ("matches", C.c_void_p), ("chain_score", C.c_uint32), ("path_len", C.c_uint32), ("path", C.c_void_p),
                ("n_cigar", C.c_uint32), ("score", C.c_int32), ("cigar", C.c_void_p), ("n_dropped", C.c_uint32), ("_pad0", C.c_uint32)]


class AlignStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_aligned", "n_skipped", "n_dropped", "n_kmer_matches", "n_chain_points", "n_trivial", "n_simple",
                                          "n_small_dp", "n_general_dp", "dp_cells", "n_batches")] + [("n_level", C.c_uint64 * 3)] + \
               [(n, C.c_uint64) for n in ("bytes_h2d", "bytes_d2h")] + \
               [(n, C.c_double) for n in ("div_ms", "index_ms", "match_ms", "chain_ms", "fill_ms", "select_ms", "total_ms")]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "n_level" else getattr(self, n)) for n, _ in self._fields_}


class AlignTrParams(C.Structure):
    """`locityper align --tr-div / --tr-anchor` (src/seq/align.rs:59-60): 0.01, 101."""
    _fields_ = [("transitive_div", C.c_double), ("transitive_anchor", C.c_uint32), ("_pad0", C.c_uint32)]


class AlignTrOut(C.Structure):
    _fields_ = [("route", C.c_void_p), ("via", C.c_void_p)]


class AlignTrStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rounds", "n_accelerated", "n_shortcut", "n_tr_stretches", "tr_dp_cells", "store_bytes")] + \
               [(n, C.c_double) for n in ("plan_ms", "tr_fill_ms", "optimize_ms", "count_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


PRUNE_MAX_N = 16384
PRUNE_POWER_MIN, PRUNE_POWER_MAX = -(1 << 31), (1 << 31) - 1      # PowerMean::Min / ::Max
PRUNE_WARN_KMERS = 1


class PafDivStats(C.Structure):
    """What load_divergences (src/command/prune.rs:159-230) only logs."""
    _fields_ = [("n_missing", C.c_uint64), ("n_negative", C.c_uint64), ("n_conflicting", C.c_uint64), ("missing_i", C.c_uint32),
                ("missing_j", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PruneStep(C.Structure):
    _fields_ = [("cluster1", C.c_uint32), ("cluster2", C.c_uint32), ("dissimilarity", C.c_double), ("size", C.c_uint32), ("_pad0", C.c_uint32)]


PRUNE_STEP_DTYPE = np.dtype([("cluster1", "<u4"), ("cluster2", "<u4"), ("dissimilarity", "<f8"), ("size", "<u4"), ("_pad0", "<u4")])


class PruneParams(C.Structure):
    """`locityper prune` (src/command/prune.rs:39-55): threshold 0.0002, no n_clusters, power 2."""
    _fields_ = [("threshold", C.c_double), ("n_clusters", C.c_uint32), ("power", C.c_int32), ("only_tree", C.c_int32), ("skip_tree", C.c_int32)]


class PruneStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rescans", "n_rep_pairs", "bytes_h2d", "bytes_d2h", "matrix_bytes")] + \
               [(n, C.c_double) for n in ("build_ms", "merge_ms", "repr_ms", "host_ms", "total_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PruneOut(C.Structure):
    _fields_ = [("n", C.c_uint32), ("n_clusters", C.c_uint32), ("threshold", C.c_double), ("epsilon", C.c_double), ("steps", C.c_void_p),
                ("keep_ids", C.c_void_p), ("cluster_off", C.c_void_p), ("members", C.c_void_p), ("repr", C.c_void_p), ("acc", C.c_void_p),
                ("stats", PruneStats)]


class PruneFiles(C.Structure):
    _fields_ = [("newick", C.c_void_p), ("newick_len", C.c_uint64), ("discarded", C.c_void_p), ("discarded_len", C.c_uint64),
                ("fasta", C.c_void_p), ("fasta_len", C.c_uint64), ("kmers", C.c_void_p), ("kmers_len", C.c_uint64),
                ("distances", C.c_void_p), ("distances_len", C.c_uint64), ("paf", C.c_void_p), ("paf_len", C.c_uint64),
                ("keep", C.c_void_p), ("n_keep", C.c_uint32), ("unchanged", C.c_int32), ("warn_bits", C.c_uint32), ("_pad0", C.c_uint32),
                ("threshold", C.c_double), ("div", PafDivStats), ("stats", PruneStats)]


class BgReadsView(C.Structure):
    """The records of the background interval as load_alns keeps them (preproc.rs:988-1028)."""
    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_ignored", C.c_uint64),
        ("n_wo_cigar", C.c_uint64),
        ("paired", C.c_int32),
        ("_pad0", C.c_uint32),
        ("read_len", C.c_double),
        ("pos", C.c_void_p),
        ("end", C.c_void_p),
        ("qlen", C.c_void_p),
        ("flags", C.c_void_p),
        ("mate", C.c_void_p),
        ("cigar_off", C.c_void_p),
        ("cigar", C.c_void_p),
        ("seq_off", C.c_void_p),
        ("bases2", C.c_void_p),
        ("nmask", C.c_void_p),
    ]


class BgDiag(C.Structure):
    """The --debug intermediates of the background estimate (lcty_bg_diag)."""
    _fields_ = [
        ("n_windows", C.c_uint64), ("n_records", C.c_uint64), ("n_pairs", C.c_uint64), ("n_hist", C.c_uint64), ("n_edit", C.c_uint64),
        ("win_start", C.c_void_p), ("win_gc", C.c_void_p), ("win_kmer_frac", C.c_void_p), ("win_keep", C.c_void_p), ("win_depth", C.c_void_p),
        ("rec_counts", C.c_void_p), ("rec_edit", C.c_void_p), ("rec_read_len", C.c_void_p), ("rec_middle", C.c_void_p), ("rec_window", C.c_void_p),
        ("pair_first", C.c_void_p), ("pair_second", C.c_void_p), ("pair_insert", C.c_void_p), ("pair_same_strand", C.c_void_p),
        ("hist_size", C.c_void_p), ("hist_count", C.c_void_p),
        ("orient", C.c_uint64 * 2),
        ("ins_limit", C.c_double), ("ins_mean", C.c_double), ("ins_var", C.c_double),
        ("ci_low", C.c_uint32), ("ci_high", C.c_uint32),
        ("op_totals", C.c_uint64 * 5),
        ("edit_edit", C.c_void_p), ("edit_len", C.c_void_p), ("edit_count", C.c_void_p),
        ("unif_coef", C.c_double),
        ("n_stage", C.c_uint64 * 6),
        ("gc_nwin", C.c_uint32 * GC_BINS),
        ("loess_mean", C.c_double * GC_BINS), ("loess_var", C.c_double * GC_BINS),
        ("blur_mean", C.c_double * GC_BINS), ("blur_var", C.c_double * GC_BINS),
        ("nb_n", C.c_double * GC_BINS), ("nb_p", C.c_double * GC_BINS),
        ("depth_mean", C.c_double), ("depth_var", C.c_double),
        ("kernel_ms", C.c_double * 4), ("fit_ms", C.c_double), ("total_ms", C.c_double),
    ]


SOLVER_GREEDY, SOLVER_ANNEAL, SOLVER_EXACT = 0, 1, 2


class Solver(C.Structure):
    """One stage's solver (src/solvers/stoch.rs)."""
    _fields_ = [
        ("kind", C.c_int32),
        ("best_start", C.c_int32),
        ("sample_size", C.c_uint32),
        ("plato_size", C.c_uint32),
        ("anneal_steps", C.c_uint32),
        ("node_limit", C.c_uint32),
        ("init_prob", C.c_double),
    ]


class GtAlnsView(C.Structure):
    """lcty_gt_alns_view: a GenotypeAlignments after apply_tweak as plain arrays (model/assgn.rs:16-36)."""
    _fields_ = [
        ("n_reads", C.c_uint64),
        ("read_ixs", C.c_void_p),
        ("ln_prob", C.c_void_p),
        ("windows", C.c_void_p),
        ("n_windows", C.c_uint32),
        ("n_contigs", C.c_uint32),
        ("window_gc", C.c_void_p),
        ("window_weight", C.c_void_p),
        ("wshifts", C.c_void_p),
        ("depth_contrib", C.c_double),
        ("aln_contrib", C.c_double),
    ]


class DepthTables(C.Structure):
    """lcty_depth_tables: the caller's own window distributions as rows of ln-probabilities over the depth."""
    _fields_ = [("n_rows", C.c_uint32), ("width", C.c_uint32), ("values", C.c_void_p), ("id", C.c_uint64)]


class AlnRec(C.Structure):
    _fields_ = [
        ("pos", C.c_uint32),
        ("contig", C.c_uint16),
        ("flags", C.c_uint16),
        ("n_cigar", C.c_uint32),
        ("cigar_rel", C.c_uint32),
    ]


ALN_REC_DTYPE = np.dtype([("pos", "<u4"), ("contig", "<u2"), ("flags", "<u2"),
                          ("n_cigar", "<u4"), ("cigar_rel", "<u4")])
assert ALN_REC_DTYPE.itemsize == C.sizeof(AlnRec) == 16


class ReadsHost(C.Structure):
    _fields_ = [
        ("n_pairs", C.c_uint64),
        ("mate_len", C.POINTER(C.c_uint32)),
        ("mate_off", C.POINTER(C.c_uint64)),
        ("bases2", C.POINTER(C.c_uint32)),
        ("nmask", C.POINTER(C.c_uint32)),
        ("aln_off", C.POINTER(C.c_uint64)),
        ("recs", C.POINTER(AlnRec)),
        ("cigar_off", C.POINTER(C.c_uint64)),
        ("cigar", C.POINTER(C.c_uint32)),
    ]


class PairAln(C.Structure):
    _fields_ = [
        ("ln_prob", C.c_double),
        ("ix1", C.c_uint32),
        ("mid1", C.c_uint32),
        ("ix2", C.c_uint32),
        ("mid2", C.c_uint32),
        ("contig", C.c_uint16),
        ("_pad", C.c_uint16 * 3),
    ]


PAIR_ALN_DTYPE = np.dtype([("ln_prob", "<f8"), ("ix1", "<u4"), ("mid1", "<u4"), ("ix2", "<u4"),
                           ("mid2", "<u4"), ("contig", "<u2"), ("_pad", "<u2", (3,))])
assert PAIR_ALN_DTYPE.itemsize == C.sizeof(PairAln) == 32


def ptr(arr, ctype):
    """Pointer of `ctype` into a C-contiguous numpy array (kept alive by the caller)."""
    if arr is None:
        return C.cast(None, C.POINTER(ctype))
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(C.POINTER(ctype))


class ReadsChunk:
    """Numpy-backed lcty_reads_host: a chunk of read pairs with all their records."""

    def __init__(self, mate_len, mate_off, bases2, nmask, aln_off, recs, cigar_off, cigar):
        self.mate_len = np.ascontiguousarray(mate_len, dtype=np.uint32)
        self.mate_off = np.ascontiguousarray(mate_off, dtype=np.uint64)
        self.bases2 = np.ascontiguousarray(bases2, dtype=np.uint32)
        self.nmask = np.ascontiguousarray(nmask, dtype=np.uint32)
        self.aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
        self.recs = np.ascontiguousarray(recs, dtype=ALN_REC_DTYPE)
        self.cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64)
        self.cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        self.n_pairs = len(self.aln_off) - 1
        assert len(self.mate_len) == 2 * self.n_pairs
        assert len(self.mate_off) == 2 * self.n_pairs + 1
        assert len(self.cigar_off) == self.n_pairs + 1
        assert np.all(self.mate_off % 32 == 0)

    @property
    def n_bases(self):
        return int(self.mate_off[-1])

    def host_struct(self):
        h = ReadsHost()
        h.n_pairs = self.n_pairs
        h.mate_len = ptr(self.mate_len, C.c_uint32)
        h.mate_off = ptr(self.mate_off, C.c_uint64)
        h.bases2 = ptr(self.bases2, C.c_uint32)
        h.nmask = ptr(self.nmask, C.c_uint32)
        h.aln_off = ptr(self.aln_off, C.c_uint64)
        h.recs = C.cast(self.recs.ctypes.data, C.POINTER(AlnRec))
        h.cigar_off = ptr(self.cigar_off, C.c_uint64)
        h.cigar = ptr(self.cigar, C.c_uint32)
        return h

    # ---- construction from plain Python, for hand-written test cases ----
    @staticmethod
    def from_pairs(pairs):
        """pairs: list of dicts {"seq1": str, "seq2": str|None, "recs": [(contig, pos, flags, cigar_str)]}.

        Records must already be in the input-order contract (mate-1 group then mate-2 group);
        FLAG_MATE2 is added by the caller. cigar_str uses =XIDSHM letters.
        """
        opmap = {"M": 0, "I": 1, "D": 2, "S": 4, "H": 5, "=": 7, "X": 8, "N": 3, "P": 6}
        mate_len, mate_off, aln_off, cigar_off = [], [0], [0], [0]
        seqs, recs, cigar = [], [], []
        for p in pairs:
            for key in ("seq1", "seq2"):
                s = p.get(key) or ""
                mate_len.append(len(s))
                seqs.append(s)
                mate_off.append(mate_off[-1] + (len(s) + 31) // 32 * 32)
            rel = 0
            for contig, pos, flags, cig in p["recs"]:
                words = []
                num = ""
                for ch in cig:
                    if ch.isdigit():
                        num += ch
                    else:
                        words.append((int(num) << 4) | opmap[ch])
                        num = ""
                recs.append((pos, contig, flags, len(words), rel))
                cigar.extend(words)
                rel += len(words)
            aln_off.append(len(recs))
            cigar_off.append(len(cigar))
        nb = mate_off[-1]
        bases2 = np.zeros(max(nb // 16, 1), dtype=np.uint32)
        nmask = np.zeros(max(nb // 32, 1), dtype=np.uint32)
        code = {"A": 0, "C": 1, "G": 2, "T": 3}
        for m, s in enumerate(seqs):
            off = mate_off[m]
            for i, ch in enumerate(s):
                b = off + i
                if ch in code:
                    bases2[b >> 4] |= np.uint32(code[ch] << (2 * (b & 15)))
                else:
                    nmask[b >> 5] |= np.uint32(1 << (b & 31))
        rec_arr = np.array(recs, dtype=ALN_REC_DTYPE) if recs else np.zeros(0, dtype=ALN_REC_DTYPE)
        return ReadsChunk(mate_len, mate_off, bases2, nmask, aln_off, rec_arr, cigar_off,
                          np.array(cigar, dtype=np.uint32) if cigar else np.zeros(0, dtype=np.uint32))

    def slice(self, lo, hi):
        """Sub-chunk of pairs [lo, hi) with rebased offsets."""
        mo = self.mate_off[2 * lo:2 * hi + 1]
        ao = self.aln_off[lo:hi + 1]
        co = self.cigar_off[lo:hi + 1]
        return ReadsChunk(
            self.mate_len[2 * lo:2 * hi], mo - mo[0],
            self.bases2[int(mo[0]) // 16:max(int(mo[-1]) // 16, int(mo[0]) // 16 + 1)],
            self.nmask[int(mo[0]) // 32:max(int(mo[-1]) // 32, int(mo[0]) // 32 + 1)],
            ao - ao[0], self.recs[int(ao[0]):int(ao[-1])], co - co[0],
            self.cigar[int(co[0]):int(co[-1])])

    def counted(self, allele_len):
        """The chunk's records as lcty_aln_counted entries (uint32 x 4 per record): what count_region_operations_fast +
        limited_clipping (aln.rs:288-317) leave of every record, computed here as the caller of lcty_reads_append_counted would.
        Records with an empty CIGAR must not be in the chunk (the record path skips them; a counted batch has no way to say so)."""
        n = len(self.recs)
        try:                                                     # the C helper of the synthetic-data library does the same loop
            from . import synth
            out = np.zeros((n, 4), dtype=np.uint32)
            al = np.ascontiguousarray(allele_len, dtype=np.uint32)
            f = synth.lib().synth_count_records
            f.restype = C.c_uint64
            f.argtypes = [C.c_uint64] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
            bad = f(self.n_pairs, self.aln_off.ctypes.data, self.recs.ctypes.data, self.cigar_off.ctypes.data, self.cigar.ctypes.data,
                    al.ctypes.data, len(al), out.ctypes.data)
            assert bad == 0, f"record {bad - 1} cannot be counted (unsupported operation, empty CIGAR or a count above 65535)"
            return out
        except (ImportError, OSError, AttributeError):
            pass
        pair_of = np.repeat(np.arange(self.n_pairs, dtype=np.int64), np.diff(self.aln_off.astype(np.int64)))
        start = self.cigar_off[pair_of].astype(np.int64) + self.recs["cigar_rel"].astype(np.int64)
        ncig = self.recs["n_cigar"].astype(np.int64)
        unm = (self.recs["flags"].astype(np.int64) & FLAG_UNMAPPED) != 0
        assert np.all((ncig > 0) | unm), "a mapped record with an empty CIGAR in a chunk that is to be counted"
        rec_of = np.repeat(np.arange(n, dtype=np.int64), ncig)
        first = np.cumsum(ncig) - ncig
        word_ix = start[rec_of] + (np.arange(len(rec_of), dtype=np.int64) - first[rec_of])
        w = self.cigar[word_ix].astype(np.int64)
        op, ln = w & 15, w >> 4
        is_first = (np.arange(len(rec_of)) - first[rec_of]) == 0
        is_last = (np.arange(len(rec_of)) - first[rec_of]) == ncig[rec_of] - 1
        op = np.where((op == CIGAR_H) & (is_first | is_last), CIGAR_S, op)                       # hard_to_soft (cigar.rs:309-320)
        assert np.all(np.isin(op, (CIGAR_EQ, CIGAR_X, CIGAR_I, CIGAR_D, CIGAR_S))), "unsupported CIGAR operation"
        def total(mask):
            return np.bincount(rec_of[mask], weights=ln[mask], minlength=n).astype(np.int64)
        matches, mism, ins, dele = total(op == CIGAR_EQ), total(op == CIGAR_X), total(op == CIGAR_I), total(op == CIGAR_D)
        left = total((op == CIGAR_S) & is_first); right = total((op == CIGAR_S) & is_last & ~is_first)
        pos = self.recs["pos"].astype(np.int64)
        end = pos + matches + mism + dele
        clen = np.asarray(allele_len, dtype=np.int64)[np.minimum(self.recs["contig"].astype(np.int64), len(allele_len) - 1)]
        clip = np.minimum(left, pos) + np.minimum(right, np.maximum(clen - end, 0))               # limited_clipping (aln.rs:288-296)
        assert max(matches.max(initial=0), mism.max(initial=0), ins.max(initial=0), dele.max(initial=0), clip.max(initial=0)) < 65536
        fl = self.recs["flags"].astype(np.int64)
        pos_flags = pos | np.where(fl & FLAG_REVERSE, 1 << 28, 0) | np.where(fl & (FLAG_SECONDARY | FLAG_SUPPL), 1 << 29, 0) \
            | np.where(fl & FLAG_UNMAPPED, 1 << 30, 0)
        out = np.zeros((n, 4), dtype=np.uint32)
        out[:, 0] = pos_flags
        out[:, 1] = self.recs["contig"].astype(np.int64) | (matches << 16)
        out[:, 2] = mism | (ins << 16)
        out[:, 3] = dele | (clip << 16)
        return out

    def primaries(self):
        """The same pairs with only the primary record of each read end (no secondary / supplementary records)."""
        n = len(self.aln_off) - 1
        keep = (self.recs["flags"] & (FLAG_SECONDARY | FLAG_SUPPL)) == 0
        pair_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.aln_off.astype(np.int64)))
        recs = self.recs[keep].copy()
        pair_k = pair_of[keep]
        aln_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.bincount(pair_k, minlength=n), out=aln_off[1:], dtype=np.uint64)
        nc = recs["n_cigar"].astype(np.int64)
        src = self.cigar_off.astype(np.int64)[pair_k] + recs["cigar_rel"].astype(np.int64)
        ends = np.cumsum(nc)
        starts = ends - nc
        cigar_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.bincount(pair_k, weights=nc, minlength=n).astype(np.uint64), out=cigar_off[1:], dtype=np.uint64)
        recs["cigar_rel"] = (starts - cigar_off.astype(np.int64)[pair_k]).astype(np.uint32)
        total = int(ends[-1]) if len(ends) else 0
        gather = np.repeat(src - starts, nc) + np.arange(total, dtype=np.int64)
        cigar = self.cigar[gather] if total else np.zeros(0, dtype=np.uint32)
        return ReadsChunk(self.mate_len, self.mate_off, self.bases2, self.nmask, aln_off, recs, cigar_off, cigar)


class RecruitParams(C.Structure):      # lcty_recruit_params
    _fields_ = [("match_frac", C.c_double), ("match_length", C.c_uint32), ("thresh_kmer_count", C.c_uint16),
                ("minimizer_k", C.c_uint8), ("minimizer_w", C.c_uint8)]


class MapParams(C.Structure):          # lcty_map_params
    _fields_ = [("k", C.c_uint32), ("stride", C.c_uint32), ("min_votes", C.c_uint32), ("max_occ", C.c_uint32), ("match", C.c_int32), ("mismatch", C.c_int32),
                ("end_bonus", C.c_int32), ("min_score", C.c_int32), ("band", C.c_uint32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32),
                ("route", C.c_uint32), ("chain_gap", C.c_uint32), ("chain_skew", C.c_uint32), ("chain_back", C.c_uint32)]


MAP_ROUTE_AUTO, MAP_ROUTE_SHORT, MAP_ROUTE_LONG = 0, 1, 2


WARN_NO_PROBABLE_GENOTYPE, WARN_FEW_READS = 1, 2      # lcty_call_checks


class Stage(C.Structure):                # lcty_stage
    _fields_ = [("solver", Solver), ("in_size", C.c_uint64), ("attempts", C.c_uint32), ("_pad0", C.c_uint32)]


MAX_RESULT = 50


class Call(C.Structure):                 # lcty_call
    _fields_ = [("n_out", C.c_uint64), ("ixs", C.c_uint64 * MAX_RESULT), ("ln_probs", C.c_double * MAX_RESULT),
                ("quality", C.c_double), ("unexpl_reads", C.c_uint32), ("warnings", C.c_uint32), ("n_good", C.c_uint64),
                ("kept_after_filter", C.c_uint64)]


# ---- a resident genome (lcty_genome.hip) ----
GENOME_SCAN_RUN = 128            # LCTY_GENOME_SCAN_RUN: k-mer starts per thread of the scan kernel


class GenomeCountStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_query_kmers", "n_distinct", "table_slots", "n_scanned", "n_hits")] + \
               [("scan_run", C.c_uint32), ("_pad0", C.c_uint32)] + \
               [(n, C.c_double) for n in ("table_ms", "scan_ms", "gather_ms", "total_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("_")}


ROUTE_LEAN, ROUTE_TWO, ROUTE_GENERAL = 0, 1, 2                      # LCTY_ROUTE_*: the scoring kernel that took a pair
LEAN_FORM_NONE, LEAN_FORM_INDEX, LEAN_FORM_KEEP = 0, 1, 2           # LCTY_LEAN_FORM_*


class ScoreRoutes(C.Structure):        # lcty_score_routes
    _fields_ = [(n, C.c_uint64) for n in ("n_pairs", "n_lean", "n_two", "n_general")] + \
               [("lean_form", C.c_int32), ("two_ran", C.c_int32), ("route", C.c_void_p)]


class BgzfStats(C.Structure):          # lcty_bgzf_stats
    _fields_ = [(n, C.c_uint64) for n in ("n_blocks", "bytes_in", "bytes_out")] + \
               [(n, C.c_double) for n in ("ms_upload", "ms_kernel", "ms_download", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BgzfDeflateStats(C.Structure):   # lcty_bgzf_deflate_stats
    _fields_ = [(n, C.c_uint64) for n in ("n_blocks", "bytes_in", "bytes_out", "n_stored", "n_fixed", "n_dynamic")] + \
               [(n, C.c_double) for n in ("ms_upload", "ms_kernel", "ms_download", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AlnBamStats(C.Structure):        # lcty_aln_bam_stats
    _fields_ = [(n, C.c_uint64) for n in ("bytes_read", "bytes_inflated", "blocks", "records", "pairs", "bases", "cigar_words")] + \
               [(n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_walk", "ms_record", "ms_gather", "ms_unpack", "ms_download", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SampleBamStats(C.Structure):     # lcty_sample_bam_stats
    _fields_ = [(n, C.c_uint64) for n in ("n_regions", "n_chunks", "file_bytes", "bytes_read", "blocks_inflated", "bytes_inflated", "records_walked",
                                          "records_primary", "records_kept", "n_pairs", "n_discarded")] + \
               [(n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_walk", "ms_upload", "ms_record", "ms_pair", "ms_unpack", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BamStreamStats(C.Structure):     # lcty_bam_stream_stats
    _fields_ = [(n, C.c_uint64) for n in ("files", "file_bytes", "bytes_read", "blocks_inflated", "bytes_inflated", "windows", "windows_enlarged",
                                          "bytes_carried", "records_walked", "records_primary", "records_kept", "bases_kept", "reads", "first_kept")] + \
               [(n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_walk", "ms_upload", "ms_record", "ms_pair", "ms_unpack", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# lcty_recruited: the bytes knob "recruited_max_bytes" counts per 32-base unit (a 64-bit word of bases, a 32-bit word of mask) and per
# pair (two lengths, two offsets, an ordinal)
RECRUITED_UNIT_BYTES = 12
RECRUITED_PAIR_BYTES = 32


class FastxDeviceStats(C.Structure):   # lcty_fastx_device_stats
    _fields_ = [(n, C.c_uint64) for n in ("bytes_read", "bytes_inflated", "windows", "windows_enlarged", "records")] + \
               [(n, C.c_double) for n in ("ms_read", "ms_inflate", "ms_upload", "ms_lines", "ms_records", "ms_pack", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}
