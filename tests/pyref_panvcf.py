"""Restatement, in the reference's own serial form, of what `locityper target -v` does before process_alleles: the yardstick of the
pangenome-VCF tests. Written from the behaviour of the cited Rust lines — HaplotypeNames::new, filter_variants and
reconstruct_sequences (src/seq/panvcf.rs:65-321), find_best_boundary and expand_locus (src/command/add.rs:371-518), the retry loop and
the has_n filter of add_locus (733-780), check_sequences (655-690) — as loops over records, haplotypes and positions on Python lists
and floats (IEEE doubles, one rounding per operation as in Rust). It shares no closed form with the library: no transposed matrix, no
masks, no segment lists, no per-position view of the boundary weights."""
import struct


class PanvcfError(Exception):
    def __init__(self, kind, msg, record=None, column=None):
        super().__init__(msg)
        self.kind, self.record, self.column = kind, record, column


# ---- HaplotypeNames::new ------------------------------------------------------------------------------------------------------------------
def haplotype_names(samples, ploidy, ref_name, leave_out):
    """-> (names in column order, [(sample index or None, hap_ix)], haplotypes left out)"""
    leave_out = set(leave_out)
    seen, names, cols, left = set(), [], [], 0
    if ref_name in leave_out:
        left += 1
    else:
        seen.add(ref_name)
        names.append(ref_name)
        cols.append((None, 0))
    n_samples = 0
    for sid, sample in enumerate(samples):
        pl = int(ploidy[sid])
        if sample in leave_out:
            left += pl
            continue
        if pl == 0:
            raise PanvcfError("InvalidData", f"Sample {sample} has zero ploidy")
        if pl > 255:
            raise PanvcfError("InvalidData", f"Sample {sample} has extremely high ploidy")
        for hap_ix in range(pl):
            hap = sample if pl == 1 else f"{sample}.{hap_ix + 1}"
            if hap in leave_out:
                left += 1
                continue
            if hap in seen:
                raise PanvcfError("InvalidData", f"Duplicate haplotype name ({hap})")
            seen.add(hap)
            names.append(hap)
            cols.append((sid, hap_ix))
        n_samples += 1
    if n_samples == 0:
        raise PanvcfError("InvalidData", "Loaded zero haplotypes")
    return names, cols, left


# ---- fetch, filter_variants, reconstruct_sequences ----------------------------------------------------------------------------------------
def fetch(records, start, end):
    """Indices of the records htslib's fetch returns; records = [(pos, [REF, ALT, ...]), ...] in file order."""
    return [i for i, (pos, alleles) in enumerate(records) if pos < end and pos + len(alleles[0]) > start]


def has_variation(gt_row):
    for a in gt_row:
        if a >= 1:
            return True
    return False


def reconstruct(contig, ref_start, ref_end, ref_seq, records, gt, names, unknown_frac, overlaps_allowed):
    """records = [(pos, [REF, ALT, ...])] (bytes), gt[record][column] (-1 = missing) over the retained columns.
    -> dict: seqs (all columns), unknown, reason (0 kept, 1 unknown, 2 N), kept (columns), total_overlaps, n_kept_records"""
    assert len(ref_seq) == ref_end - ref_start
    n = len(names)
    recs = [i for i in range(len(records)) if has_variation(gt[i])]
    seqs = [bytearray() for _ in range(n)]
    unknown = [0] * n
    ref_pos = [ref_start] * n
    total_overlaps = 0
    for i in recs:
        var_start, alleles = records[i]
        ref_len = len(alleles[0])
        var_end = var_start + ref_len
        if var_end <= ref_start:
            continue
        elif ref_end <= var_start:
            break
        elif var_start < ref_start or ref_end < var_end:
            raise PanvcfError("Boundary", f"Variant {contig}:{var_start + 1} overlaps the boundary of the region {ref_start + 1}-{ref_end}", record=i)
        for col in range(n):
            allele_ix = gt[i][col]
            if allele_ix < 0:
                unknown[col] += ref_len
                allele_ix = 0
            if allele_ix == 0:
                continue
            prev_end = ref_pos[col]
            if var_start < prev_end:
                if not overlaps_allowed:
                    raise PanvcfError("Overlap", f"Overlapping variants forbidden ({contig}:{var_start + 1} for {names[col]})", record=i, column=col)
                total_overlaps += 1
                continue
            seqs[col] += ref_seq[prev_end - ref_start:var_start - ref_start]
            seqs[col] += alleles[allele_ix]
            ref_pos[col] = var_end
    for col in range(n):
        if ref_pos[col] < ref_end:
            seqs[col] += ref_seq[ref_pos[col] - ref_start:]
    reason = []
    for col in range(n):
        if float(unknown[col]) > unknown_frac * float(len(seqs[col])):
            reason.append(1)
        elif b"N" in seqs[col]:
            reason.append(2)
        else:
            reason.append(0)
    return {"seqs": [bytes(s) for s in seqs], "unknown": unknown, "reason": reason, "kept": [c for c in range(n) if reason[c] == 0],
            "total_overlaps": total_overlaps, "n_kept_records": len(recs)}


# ---- find_best_boundary -------------------------------------------------------------------------------------------------------------------
EFFECT_MARGIN = 9


def boundary_weights(start, end, variants, k, kmer_counts, allowed_expansion, moving_window, left):
    """The weights after the distance penalty (add.rs:389-425); variants = [(pos, ref_len)] in record order."""
    cumul = [0]
    for c in kmer_counts:
        cumul.append(cumul[-1] + (1 if c <= 1 else 0))
    per_window = moving_window + 1 - k
    divisor = float(per_window)
    weights = [float(s - lag) / divisor for lag, s in zip(cumul, cumul[per_window:])]
    assert len(weights) == end - start, (len(weights), end - start)
    effect_divisor = float(EFFECT_MARGIN + 1)
    for var_start, ref_len in variants:
        var_end = var_start + ref_len
        for i in range(max(var_start - start, 0), max(min(var_end, end) - start, 0)):
            weights[i] = 0.0
        for i in range(max(var_start - end, 0), min(max(var_start - start, 0), EFFECT_MARGIN)):
            weights[var_start - start - i - 1] *= float(EFFECT_MARGIN - i) / effect_divisor
        for i in range(max(start - var_end, 0), min(max(end - var_end, 0), EFFECT_MARGIN)):
            weights[var_end + i - start] *= float(i + 1) / effect_divisor
    per_bp_drop = 0.2 / float(allowed_expansion)
    n = len(weights)
    if left:
        for i in range(n):
            j = n - 1 - i
            weights[j] -= weights[j] * per_bp_drop * float(i)
    else:
        for i in range(n):
            weights[i] -= weights[i] * per_bp_drop * float(i)
    return weights


def find_best_boundary(start, end, variants, k, kmer_counts, allowed_expansion, moving_window, left):
    """-> (position or None, weights or None)"""
    if start == end:
        for pos, ref_len in variants:
            if pos <= start and end <= pos + ref_len:
                return None, None
        return start, None
    weights = boundary_weights(start, end, variants, k, kmer_counts, allowed_expansion, moving_window, left)
    best_i, best = 0, weights[0]
    for i in range(1, len(weights)):
        if (weights[i] >= best) if left else (weights[i] > best):      # the last / the first maximum
            best_i, best = i, weights[i]
    if best == 0.0:
        return None, weights
    return start + best_i, weights


def bits(weights):
    return [struct.unpack("<Q", struct.pack("<d", w))[0] for w in weights]


# ---- expand_locus and the retry loop ------------------------------------------------------------------------------------------------------
def expand_once(locus, inner_start, inner_end, contig_len, contig_seq, count_of, k, variants, allowed_expansion, moving_window):
    """contig_seq: bytes of the whole contig (or any object sliced by absolute position); count_of(start, end) -> the k-mer counts of
    contig[start:end]; variants = the kept records [(pos, ref_len)] in file order. -> (start, end) or None"""
    if inner_end - inner_start < moving_window:
        raise PanvcfError("Short", f"Locus {locus} is shorter ({inner_end - inner_start}) than the moving window ({moving_window})")
    left_start = max(inner_start - allowed_expansion, 0)
    left_end = inner_start + moving_window
    left_seq = contig_seq[left_start:left_end]
    right_start = inner_end - moving_window
    right_end = min(inner_end + allowed_expansion, contig_len)
    right_seq = contig_seq[right_start:right_end]
    shift = left_seq.rfind(b"N")
    if shift >= 0:
        left_start += shift + 1
        if left_start > inner_start:
            raise PanvcfError("UnknownSeq", f"Unknown sequence at the locus {locus}")
    shift = right_seq.find(b"N")
    if shift >= 0:
        right_end = right_start + shift
        if right_end < inner_end:
            raise PanvcfError("UnknownSeq", f"Unknown sequence at the locus {locus}")
    left_vars = [v for v in variants if v[0] < inner_start + 1 and v[0] + v[1] > left_start]
    right_vars = [v for v in variants if v[0] < right_end and v[0] + v[1] > inner_end - 1]
    new_start, _ = find_best_boundary(left_start, inner_start + 1, left_vars, k, count_of(left_start, left_end), allowed_expansion, moving_window, True)
    if new_start is None:
        return None
    new_end, _ = find_best_boundary(inner_end - 1, right_end, right_vars, k, count_of(right_start, right_end), allowed_expansion, moving_window, False)
    if new_end is None:
        return None
    return new_start, new_end + 1


def expand(locus, inner_start, inner_end, contig_len, contig_seq, count_of, k, variants, expansions, moving_window):
    """-> (start, end, index of the attempt)"""
    moving_window = max(k, moving_window)
    for attempt, allowed in enumerate(expansions):
        if allowed == 0:
            return inner_start, inner_end, attempt
        got = expand_once(locus, inner_start, inner_end, contig_len, contig_seq, count_of, k, variants, allowed, moving_window)
        if got is not None:
            return got[0], got[1], attempt
    raise PanvcfError("CannotExpand", f"Cannot expand locus {locus}")


# ---- check_sequences without a reference --------------------------------------------------------------------------------------------------
def check_sequences(seqs):
    """-> warn bits (1: shortest < 1000, 2: < 10000, 4: the haplotypes differ at the boundary)"""
    if len(seqs) < 2:
        raise PanvcfError("InvalidData", "Less than two haplotypes available")
    shortest = min(len(s) for s in seqs)
    warn = 1 if shortest < 1000 else 2 if shortest < 10000 else 0
    prefix, suffix = seqs[0][:5], seqs[0][-5:]
    if any(s[:5] != prefix or s[-5:] != suffix for s in seqs[1:]):
        warn |= 4
    return warn
