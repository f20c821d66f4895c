"""Serial restatement of `locityper paf-vcf` (src/command/paf_vcf.rs), written from the upstream source line by line and independent of
the C++: the parity reference of tests/test_pafvcf_host.py and tests/test_gpu_pafvcf.py. Positions are 0-based inside the reference
haplotype; sequences are bytes; a CIGAR is a list of (op, len) with op one of b"=XIDMHS"."""
import bisect
import re

HEADER = (b"##fileformat=VCFv4.2\n"
          b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
          b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT")          # paf_vcf.rs:349-352
NAME_RE = re.compile(rb"^([0-9A-Za-z][0-9A-Za-z+._|~=@^-]*?)([._][1-9])?$")  # paf_vcf.rs:577
WARN_REF_SUFFIX, WARN_PRUNED = 1, 2


class ParsingError(Exception):
    pass


class InvalidInput(Exception):
    pass


class InvalidData(Exception):
    pass


class RuntimeErr(Exception):
    pass


def load_discarded(text, names):
    """DiscardedHaplotypes::load (contigs.rs:488-528): ({contig index: [discarded names]}, all_identical). The lines of the text as BufRead::lines gives them: split at '\\n', no line behind a final newline; every line needs 3 columns."""
    ids = {n: i for i, n in enumerate(names)}
    by_contig, unknown, all_identical = {}, {}, True
    if not text:
        return by_contig, all_identical
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for line in lines:
        split = line.split()
        if len(split) < 3:
            raise InvalidInput("Each line in discarded haplotypes must have at least 3 columns")
        identical = split[1] == b"="
        all_identical &= identical
        rhs = []
        for contig in split[2:]:
            if contig.endswith(b","):
                contig = contig[:-1]
            if contig in ids:
                continue
            rhs.append(contig)
            if contig in unknown:
                rhs.extend(unknown.pop(contig))
        if split[0] in ids:
            by_contig[ids[split[0]]] = rhs
        else:
            unknown[split[0]] = rhs
    return by_contig, all_identical


def group_haplotypes(names, ref_hap, discarded_text=None):
    """group_haplotypes (569-621) with the warning of convert_to_vcf 633-635: ([(sample, [contig index or None])], ref_id, warning bits)."""
    by_contig, all_identical = load_discarded(discarded_text, names)
    warn = 0 if all_identical else WARN_PRUNED
    ref_id = None
    table = {}

    def add(i, name):
        nonlocal ref_id, warn
        m = NAME_RE.match(name)
        if not m or b"\n" in name:
            raise ParsingError("Cannot parse contig name `%s`" % name.decode(errors="replace"))
        sample, hap = m.group(1), m.group(2)
        if name == ref_hap:
            ref_id = i
            if hap is not None:
                warn |= WARN_REF_SUFFIX
            else:
                return
        slot = hap[1] - ord("1") if hap is not None else 0
        vec = table.setdefault(sample, [])
        new_len = max(len(vec), slot + 1, 1 if hap is None else 2)
        vec.extend([None] * (new_len - len(vec)))
        vec[slot] = i

    for i, contig in enumerate(names):
        add(i, contig)
        for hap in by_contig.get(i, []):
            add(i, hap)
    if ref_id is None:
        raise InvalidInput("Cannot find reference haplotype")
    return sorted(table.items()), ref_id, warn


def invert_cigar(cigar):
    return [({b"I": b"D", b"S": b"D", b"D": b"I"}.get(op, op), n) for op, n in cigar]


def cigar_lens(cigar):
    """(query_len, ref_len)"""
    q = sum(n for op, n in cigar if op in (b"=", b"X", b"M", b"I", b"S"))
    r = sum(n for op, n in cigar if op in (b"=", b"X", b"M", b"D"))
    return q, r


def gap_move_left(ref, gap_start, gap_seq, min_start):
    last = len(gap_seq) - 1
    k = last
    while gap_start > min_start and gap_seq[k] == ref[gap_start - 1]:
        gap_start -= 1
        k = k - 1 if k else last
    return gap_start


def move_all_left(vars_, ref, hap):
    """move_all_left (242-271), in place; returns the number of variants that moved."""
    last_end, moved = 0, 0
    for v in vars_:
        min_start, last_end = last_end, v[1]
        rl, al = v[1] - v[0], v[3] - v[2]
        if rl == al:
            continue
        vr, va = ref[v[0]:v[1]], hap[v[2]:v[3]]
        if any(a != b for a, b in zip(vr, va)):
            continue
        prefix = min(len(vr), len(va))
        gap_seq = va[prefix:] if prefix == len(vr) else vr[prefix:]
        gap_start = v[0] + prefix
        new_start = gap_move_left(ref, gap_start, gap_seq, min_start + prefix)
        shift = gap_start - new_start
        assert v[2] >= shift and v[0] - shift >= min_start
        if shift:
            moved += 1
        for k in range(4):
            v[k] -= shift
    return moved


def process_haplotype(ref, hap, cigar, stats=None):
    """process_haplotype (276-332): [[ref_start, ref_end, hap_start, hap_end]] after the left shift."""
    vars_ = []
    rpos = qpos = 0
    for op, n in cigar:
        if op == b"=":
            rpos += n
            qpos += n
            continue
        if op in (b"M", b"H"):
            raise RuntimeErr("Unexpected operation (M/H) in CIGAR")
        qd = n if op in (b"X", b"I", b"S") else 0
        rd = n if op in (b"X", b"D") else 0
        need_new = True
        if vars_:
            last = vars_[-1]
            if rpos <= last[1] and qpos <= last[3]:
                last[1] = max(last[1], rpos + rd)
                last[3] = max(last[3], qpos + qd)
                need_new = False
            else:
                assert rpos > last[1] and qpos > last[3]
        if need_new:
            if rd == qd:
                vars_.append([rpos, rpos + rd, qpos, qpos + qd])
            elif rpos == 0 or qpos == 0:
                vars_.append([rpos, rpos + rd + 1, qpos, qpos + qd + 1])
            else:
                vars_.append([rpos - 1, rpos + rd, qpos - 1, qpos + qd])
        rpos += rd
        qpos += qd
    if vars_ and (vars_[-1][1] > len(ref) or vars_[-1][3] > len(hap)):
        raise RuntimeErr("CIGAR operation out of range of the sequence")
    moved = move_all_left(vars_, ref, hap)
    if stats is not None:
        stats["moved"] = moved
    return vars_


def process_paf(seqs, ref_id, entries, stats=None):
    """process_paf (362-415). entries: [(query id, target id, cigar)] as lcty_paf_read keeps them. Per haplotype a variant list or None."""
    out = [None] * len(seqs)
    out[ref_id] = []
    bad = 0
    moved = {}
    for q, t, cigar in entries:
        if ref_id == q:
            hap_id, cigar = t, invert_cigar(cigar)
        elif ref_id == t:
            hap_id = q
        else:
            continue
        ql, rl = cigar_lens(cigar)
        if ql != len(seqs[hap_id]) or rl != len(seqs[ref_id]):
            bad += 1
            continue
        one = {}
        out[hap_id] = process_haplotype(seqs[ref_id], seqs[hap_id], cigar, one)
        moved[hap_id] = one["moved"]
    if stats is not None:
        stats["n_shifted"] = sum(moved.values())          # of the lists that stay (a later entry replaces an earlier one)
        stats["n_bad_len"] = bad
        stats["n_missing"] = sum(v is None for v in out)
    return out


def combine_ranges(vars_):
    """combine_variants (535-555): (unique ranges, merged ranges)."""
    unique = sorted({(v[0], v[1]) for hv in vars_ if hv is not None for v in hv})
    merged = []
    for start, end in unique:
        if merged and merged[-1][1] > start:
            merged[-1][1] = max(merged[-1][1], end)
        else:
            merged.append([start, end])
    return unique, [tuple(m) for m in merged]


def get_hap_ranges(ref_ranges, hv):
    """get_hap_ranges (420-460); the two bisections of bisect.rs (right_by on ref_end, left_by_at on ref_start from i) through `bisect`."""
    n = len(hv)
    if n == 0:
        return list(ref_ranges)
    ends = [v[1] for v in hv]
    starts = [v[0] for v in hv]
    out = []
    for start, end in ref_ranges:
        diff = end - start
        i = bisect.bisect_right(ends, start)            # the first variant with ref_end > start
        j = bisect.bisect_left(starts, end, i, n)       # the first at or behind i with ref_start >= end
        if i == n:
            last = hv[n - 1]
            s = start - last[1]
            out.append((last[3] + s, last[3] + s + diff))
            continue
        v1 = hv[i]
        if i == j:
            ls = v1[0] - start
            if v1[2] < ls:
                raise RuntimeErr("haplotype range starts before the haplotype")
            out.append((v1[2] - ls, v1[2] + diff - ls))
            continue
        v2 = hv[j - 1]
        if start <= v1[0] and v2[1] <= end:
            ls = v1[0] - start
            if v1[2] < ls:
                raise RuntimeErr("haplotype range starts before the haplotype")
            out.append((v1[2] - ls, v2[3] + (end - v2[1])))
        else:
            out.append(None)
    return out


def allele_table(ref_ranges, vars_, seqs, ref_id):
    """The allele part of write_vcf (473-494): (allele_ix[n_ranges][n_seqs] with -1 for None, alleles per range as bytes)."""
    hap_ranges = [get_hap_ranges(ref_ranges, hv) if hv is not None else [None] * len(ref_ranges) for hv in vars_]
    ref = seqs[ref_id]
    ix, all_alleles = [], []
    for r, (start, end) in enumerate(ref_ranges):
        alleles = [ref[start:end]]
        number = {alleles[0]: 0}                             # position() of 487 through a dictionary
        row = []
        for h, seq in enumerate(seqs):
            rng = hap_ranges[h][r]
            if rng is None:
                row.append(-1)
                continue
            if rng[1] > len(seq) or rng[0] > rng[1]:
                raise RuntimeErr("haplotype range outside the haplotype (upstream panics)")
            allele = seq[rng[0]:rng[1]]
            if b"N" in allele:
                row.append(-1)
                continue
            if allele not in number:
                number[allele] = len(alleles)
                alleles.append(allele)
            row.append(number[allele])
        ix.append(row)
        all_alleles.append(alleles)
    return ix, all_alleles


def vcf_body(chrom, shift, ref_ranges, ix, alleles, groups):
    """The record lines of write_vcf (495-517)."""
    out = []
    for r, (start, _end) in enumerate(ref_ranges):
        if len(alleles[r]) == 1:
            continue
        line = chrom + b"\t%d\t." % (start + shift + 1)
        for i, a in enumerate(alleles[r]):
            line += (b"\t" if i <= 1 else b",") + a
        line += b"\t60\t.\t.\tGT"
        for _, slots in groups:
            for i, j in enumerate(slots):
                line += b"\t" if i == 0 else b"|"
                line += b"%d" % ix[r][j] if j is not None and ix[r][j] >= 0 else b"."
        out.append(line + b"\n")
    return b"".join(out)


def vcf_header(groups):
    return HEADER + b"".join(b"\t" + name for name, _ in groups) + b"\n"


def paf_to_vcf(names, seqs, entries, ref_hap, discarded_text=None, region=None):
    """convert_to_vcf (623-657) on buffers: (merged text, separate text, stats)."""
    groups, ref_id, warn = group_haplotypes(names, ref_hap, discarded_text)
    if region is not None:
        chrom, start, end = region
        if end - start != len(seqs[ref_id]):
            raise InvalidData("region does not match reference haplotype")
        shift = start
    else:
        chrom, shift = ref_hap, 0
    stats = {"warn_bits": warn}
    vars_ = process_paf(seqs, ref_id, entries, stats)
    unique, merged = combine_ranges(vars_)
    texts = []
    for ranges in (merged, unique):
        ix, alleles = allele_table(ranges, vars_, seqs, ref_id)
        texts.append(vcf_header(groups) + vcf_body(chrom, shift, ranges, ix, alleles, groups))
    return texts[0], texts[1], stats
