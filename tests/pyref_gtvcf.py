"""A line-by-line Python restatement of the lcty_gtvcf_* section (extra/into_vcf.py, extra/into_csv.py): the column of a predicted allele,
fixed-point numbers, the header and the record lines of one locus. Plain Python over lists and bytes; the tests compare the library
with it byte for byte, and tests/test_gtvcf_host.py pins it to answers written out by hand."""

REF = 0xFFFFFFFF
ABSENT = -(1 << 63)
QUAL, READS, UNEXPL, WDIST, WARN = 1, 2, 4, 8, 16
ALL, UPSTREAM = 31, 14
KEYS = (("qual", "qual10", 1), ("reads", "reads", 0), ("unexpl", "unexpl", 0), ("wdist", "wdist5", 5))


class Refused(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


INVALID_INPUT, INVALID_DATA, UNSUPPORTED = 1, 2, 5


def column(samples, ploidy, genome_name, allele):
    """copy_genotype (into_vcf.py:99-114) for one allele name: the column of the GT matrix, or REF."""
    hap_off = [0]
    for p in ploidy:
        hap_off.append(hap_off[-1] + p)
    index = {s: i for i, s in enumerate(samples)}
    if len(allele) > 2 and allele[-2:-1] in (b".", b"_"):                  # 102
        sample, digit = allele[:-2], allele[-1:]
        if sample not in index:                                          # KeyError upstream
            raise Refused(INVALID_DATA, allele)
        if not digit.isdigit():                                          # int() raises upstream
            raise Refused(INVALID_DATA, allele)
        hap = int(digit)
        if hap == 0 or hap > ploidy[index[sample]]:                      # 0: Python would take the last haplotype; refused by the library
            raise Refused(INVALID_DATA, allele)
        return hap_off[index[sample]] + hap - 1                          # 106
    if allele == genome_name:                                            # 107-108
        return REF
    if allele not in index:
        raise Refused(INVALID_DATA, allele)
    if ploidy[index[allele]] != 1:                                       # 112
        raise Refused(INVALID_DATA, allele)
    return hap_off[index[allele]]                                        # 113


def fixed_print(v, decimals, pad=False):
    if v == ABSENT:
        return b"nan" if pad else b"."
    digits = str(abs(v)).rjust(decimals + 1, "0")
    ip, fp = (digits[:-decimals], digits[-decimals:]) if decimals else (digits, "")
    if not pad:
        fp = fp.rstrip("0")
    return (("-" if v < 0 else "") + ip + ("." + fp if fp else "")).encode()


def fixed_parse(text, decimals):
    if text == "NA" or text.lower() == "nan":
        return ABSENT
    body = text[1:] if text[:1] in ("+", "-") else text
    ip, _, fp = body.partition(".")
    if not ip + fp or any(c not in "0123456789" for c in ip + fp):        # a second point lands in fp
        raise Refused(INVALID_DATA, text)
    kept, dropped = fp[:decimals].ljust(decimals, "0"), fp[decimals:]
    v = int((ip or "0") + kept)
    if text[:1] == "-":
        v = -v - (1 if dropped.strip("0") else 0)
    return v


def format_key(mask):
    return b":".join([b"GT"] + [k.encode() for bit, (k, _, _) in enumerate(KEYS) if mask >> bit & 1] + ([b"warn"] if mask & WARN else []))


def header(contigs, samples):
    """create_vcf_header (into_vcf.py:76-96) as pysam writes it. contigs: [(name, length or None)]."""
    out = [b"##fileformat=VCFv4.2", b'##FILTER=<ID=PASS,Description="All filters passed">']
    for name, length in contigs:
        out.append(b"##contig=<ID=" + name + (b",length=%d" % length if length else b"") + b">")
    out += [b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            b'##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Converted genotype quality">',
            b'##FORMAT=<ID=qual,Number=1,Type=Float,Description="Raw genotype quality">',
            b'##FORMAT=<ID=reads,Number=1,Type=Integer,Description="Total number of reads used to predict locus genotype">',
            b'##FORMAT=<ID=unexpl,Number=1,Type=Integer,Description="Number of unexplained reads within the locus">',
            b'##FORMAT=<ID=wdist,Number=1,Type=Float,Description="Weighted distance between primary and non-primary genotype predictions">',
            b'##FORMAT=<ID=warn,Number=1,Type=String,Description="Genotype warnings">',
            b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"] + list(samples))]
    return b"\n".join(out) + b"\n"


def calls_of(gt_row, pred):
    return [0 if c == REF else (-1 if gt_row[c] < 0 else gt_row[c]) for c in pred]


def locus_records(case, mask=ALL):
    """The records of one locus as process_locus (into_vcf.py:117-144) fills them: [(chrom, pos, id, alleles, cells)], cells per sample
    (calls or None, the text of the features, quality in tenths or None)."""
    samples, n = case["samples"], len(case["samples"])
    feats, warns = case.get("feats") or {}, case.get("warns")
    for s in range(n):
        if case["preds"][s] and mask & WARN and warns is not None and any(c in b"\t \n:" for c in warns[s]):
            raise Refused(INVALID_DATA, samples[s])
    suffix, qual = [], []
    for s in range(n):                                                   # the features are the same in every record (140-141)
        parts = []
        for bit, (_, key, decimals) in enumerate(KEYS):
            if mask >> bit & 1:
                parts.append(fixed_print(feats[key][s] if feats.get(key) is not None and feats[key][s] is not None else ABSENT, decimals))
        if mask & WARN:
            parts.append((warns[s] if warns is not None else b"") or b".")
        suffix.append(b"".join(b":" + p for p in parts))
        qual.append(feats["qual10"][s] if feats.get("qual10") is not None else None)
    out, ids = [], case.get("ids")
    for r, rec in enumerate(case["recs"]):
        cells = []
        for s in range(n):
            pred = case["preds"][s]
            if not pred:                                                 # 135-136
                cells.append((None, b"", qual[s]))
                continue
            c = calls_of(case["gt"][r], pred)
            if any(v >= len(rec["alleles"]) for v in c):
                raise Refused(INVALID_DATA, "record %d" % r)
            cells.append((c, suffix[s], qual[s]))
        out.append((case["chrom"], rec["pos"], ids[r] if ids is not None and ids[r] else b".", rec["alleles"], cells))
    return out


def line_bytes(record, mask):
    chrom, pos, id_, alleles, cells = record
    fields = [chrom, b"%d" % (pos + 1), id_, alleles[0], b",".join(alleles[1:]) if len(alleles) > 1 else b".", b".", b".", b".", format_key(mask)]
    for calls, suffix, _ in cells:                                       # 138-141
        fields.append(b"." if calls is None else b"|".join(b"." if v < 0 else b"%d" % v for v in calls) + suffix)
    return b"\t".join(fields) + b"\n"


def locus_text(case, mask=ALL):
    """process_locus over a case of tests/gtvcf_cases.py: (text, line_off, calls [n_recs][n_slots])."""
    text = header([(case["chrom"], case.get("contig_len"))], case["samples"])
    line_off, calls = [], []
    for record in locus_records(case, mask):
        line_off.append(len(text))
        text += line_bytes(record, mask)
        calls.append([v for c, _, _ in record[4] if c is not None for v in c])
    line_off.append(len(text))
    return text, line_off, calls


def whole_units(tenths):
    return float("-inf") if tenths is None else tenths // 10             # an absent quality is the lowest


def merge_text(cases, mask=ALL):
    """merge_vcfs (into_vcf.py:167-196) over loci (cases with contig_ix, start, end) in the order they were added, with the library's own
    rule for two records of one key: (text, line_off, [(contig_ix, pos, len(REF))] per line, records joined)."""
    loci = sorted(cases, key=lambda c: (c["contig_ix"], c["start"], c["end"]))                 # 176; sorted() is stable
    contigs = {}
    for c in loci:
        contigs[c["contig_ix"]] = (c["chrom"], c.get("contig_len"))                              # 169-172
    records, joined = {}, 0
    for c in loci:
        for chrom, pos, id_, alleles, cells in locus_records(c, mask):
            key = (c["contig_ix"], pos, tuple(alleles))                                          # 181
            if key not in records:
                records[key] = (chrom, pos, id_, alleles, list(cells))
                continue
            joined += 1                                                                          # 184
            kept = records[key][4]
            for s, new in enumerate(cells):
                old = kept[s]
                if new[0] is not None and (old[0] is None or (old[0] != new[0] and whole_units(new[2]) > whole_units(old[2]))):
                    kept[s] = new
    text = header([contigs[k] for k in sorted(contigs)], cases[0]["samples"] if cases else [])
    line_off, info = [], []
    for key in sorted(records):                                                                  # 192
        line_off.append(len(text))
        text += line_bytes(records[key], mask)
        info.append((key[0], key[1], len(key[2][0])))
    line_off.append(len(text))
    return text, line_off, info, joined
