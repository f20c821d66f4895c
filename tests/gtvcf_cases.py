"""Designed inputs of the lcty_gtvcf_* section: a variants window (records, alleles, a GT matrix over samples of mixed ploidy), a cohort's
predictions as allele names, features and warning texts. A case is a dict of plain Python values (tests/pyref_gtvcf.py reads it);
arrays() gives what api.GenotypeVcf.add_locus takes. Not a test."""
import numpy as np

from tests import pyref_gtvcf as R

GENOME = b"GRCh38"


def variants_view(n_vsamples):
    """the samples of the variants file: ploidy 1, 2, 3 in turn (the first is haploid)"""
    names = [b"V%d" % i for i in range(n_vsamples)]
    ploidy = [(1, 2, 3)[i % 3] for i in range(n_vsamples)]
    return names, ploidy


def random_allele(rng, lo=1, hi=6):
    return bytes(rng.choice(list(b"ACGT"), int(rng.integers(lo, hi + 1))).astype(np.uint8))


def make_case(seed, n_samples, n_recs, n_vsamples=7, no_pred=(), allele_counts=None, missing_rate=0.1, with_ids=True, absent_rate=0.2,
              warn_texts=None, all_predicted=False):
    """n_samples output samples over n_recs records. no_pred: the samples without a prediction; allele_counts: the number of alleles of
    the first records (then 1 .. 5 at random); a GT takes every allele index of its record, the last one first."""
    rng = np.random.default_rng(seed)
    vnames, ploidy = variants_view(n_vsamples)
    hap_off = np.concatenate([[0], np.cumsum(ploidy)])
    n_haps = int(hap_off[-1])
    counts = list(allele_counts or []) + [int(rng.integers(1, 6)) for _ in range(n_recs)]
    recs, gt, pos = [], [], int(rng.integers(0, 1000))
    for r in range(n_recs):
        na = counts[r]
        alleles = [random_allele(rng, 1, 12 if na <= 8 else 3) for _ in range(na)]
        if na == 301:                                                    # mixed lengths for the allele copy: empty, one base, hundreds
            alleles = [random_allele(rng, (0, 1, 2, 300, 64, 65)[a % 6], (0, 1, 2, 300, 64, 65)[a % 6]) if a else b"ACGT" for a in range(na)]
        recs.append(dict(pos=pos, alleles=alleles, ref_len=len(alleles[0])))
        row = rng.integers(0, na, n_haps)
        row[rng.random(n_haps) < missing_rate] = -1
        row[: min(n_haps, 6)] = [na - 1, min(9, na - 1), min(10, na - 1), min(99, na - 1), min(100, na - 1), 0][: min(n_haps, 6)]
        gt.append([int(v) for v in row])
        pos += int(rng.integers(0, 40))                                  # records may share a position
    samples = sorted(b"S%04d" % i for i in range(n_samples))
    names, preds = [], []
    for s in range(n_samples):
        if s in no_pred:
            names.append(None)
            preds.append([])
            continue
        p = (2, 1, 3)[s % 3]
        mine = []
        for k in range(p):
            kind = (s + k) % 5
            v = int(rng.integers(0, n_vsamples))
            if kind == 0:
                mine.append(GENOME)                                      # the genome's own name
            elif kind == 1:
                mine.append(vnames[3 * int(rng.integers(0, (n_vsamples + 2) // 3))])   # a haploid sample without a suffix
            else:
                mine.append(vnames[v] + (b".", b"_")[kind % 2] + b"%d" % int(rng.integers(1, ploidy[v] + 1)))
        if s < 6 and not all_predicted:                                  # the first haplotype columns carry the designed allele indices
            mine[0] = (b"V0", b"V1.1", b"V1_2", b"V2.1", b"V2_2", b"V2.3")[s]
        names.append(mine)
        preds.append([R.column(vnames, ploidy, GENOME, a) for a in mine])

    def feature(scale):
        return [None if rng.random() < absent_rate else int(rng.integers(0, scale)) for _ in range(n_samples)]
    feats = dict(qual10=feature(3000), reads=feature(100000), unexpl=feature(5000), wdist5=feature(10 ** 7))
    if n_samples:
        feats["qual10"][0], feats["wdist5"][0] = 270, 123
    texts = warn_texts or [b"", b"*", b"GtQual;FewReads", b"x" * 300]
    warns = [texts[(s * 7 + seed) % len(texts)] for s in range(n_samples)]
    ids = [b"" if r % 3 == 1 else b"rs%d" % (r * 977) for r in range(n_recs)] if with_ids else None
    return dict(chrom=b"chr%d" % (seed % 22 + 1), contig_len=(None if seed % 4 == 0 else 10 ** 8 + seed), samples=samples, recs=recs, gt=gt, ids=ids, preds=preds,
                pred_names=names, feats=feats, warns=warns, vsamples=vnames, ploidy=ploidy, n_haps=n_haps)


def arrays(case):
    """the record arrays of an lcty_vcf_records"""
    recs = case["recs"]
    alleles = [a for r in recs for a in r["alleles"]]
    return dict(pos=np.array([r["pos"] for r in recs], dtype=np.uint32), ref_len=np.array([r["ref_len"] for r in recs], dtype=np.uint32),
                rec_allele=np.concatenate([[0], np.cumsum([len(r["alleles"]) for r in recs])]).astype(np.uint32),
                allele_off=np.concatenate([[0], np.cumsum([len(a) for a in alleles])]).astype(np.uint64),
                allele_bytes=np.frombuffer(b"".join(alleles), dtype=np.uint8))


def window(base, other, lo, hi, name, contig_ix=0, **over):
    """a locus over records lo .. hi of base's window with the predictions, features and warnings of `other` (same samples, same variants
    file), for lcty_gtvcf_merge: loci that overlap share records"""
    c = dict(other, recs=base["recs"][lo:hi], gt=base["gt"][lo:hi], ids=base["ids"][lo:hi] if base.get("ids") else None, chrom=base["chrom"],
             contig_len=base.get("contig_len"), n_haps=base["n_haps"], locus=name, contig_ix=contig_ix)
    c["start"] = c["recs"][0]["pos"] if c["recs"] else 0
    c["end"] = c["recs"][-1]["pos"] + 1 if c["recs"] else 0
    c.update(over)
    return c


def records_at(pos, tuples, n_haps, seed=0):
    """records with the given allele tuples at one position, and a GT row each"""
    rng = np.random.default_rng(seed)
    recs = [dict(pos=pos, alleles=list(t), ref_len=len(t[0])) for t in tuples]
    gt = [[int(v) for v in rng.integers(-1, len(t), n_haps)] for t in tuples]
    return recs, gt


def write_corpus(path, seed=1):
    """the corpus of scripts/gtvcf_probe_host.cpp (its head states the format): names, numbers and texts with the restatement's answers"""
    rng = np.random.default_rng(seed)

    def answer(f, *a):
        try:
            return 0, f(*a)
        except R.Refused as e:
            return e.code, 0
    vs, pl = [b"V0", b"V1", b"V2", b"a.b", b"GRCh38", b"x_y"], [1, 2, 3, 2, 1, 9]
    lines = ["view\t" + "\t".join("%s:%d" % (n.decode(), p) for n, p in zip(vs, pl))]
    alleles = [b"V0", b"V1", b"V2", b"GRCh38", b"a.b", b"x_y", b"", b"_", b"_1", b"V", b"V9", b"V9.1"]
    alleles += [n + sep + d for n in vs + [b"V9", b"", b"V"] for sep in (b".", b"_", b"-") for d in (b"0", b"1", b"2", b"3", b"9", b"x", b":", b"")]
    for genome in (b"GRCh38", b"V0", b"V1.1", b"none"):
        for a in alleles:
            st, col = answer(R.column, vs, pl, genome, a)
            lines.append("column\t%s\t%s\t%d\t%d" % (genome.decode(), a.decode() or "-", st, col))
    values = [0, 1, 9, 10, 99, 100, 99999, 100000, 100001, 10 ** 10, -1, -10, -100000, R.ABSENT, 10 ** 18 - 1, -(10 ** 18) + 1]
    values += [int(x) for x in rng.integers(-10 ** 13, 10 ** 13, 400)]
    for v in values:
        for d in (0, 1, 5, 18):
            for pad in (0, 1):
                lines.append("print\t%d\t%d\t%d\t%s" % (v, d, pad, R.fixed_print(v, d, bool(pad)).decode()))
    texts = ["", ".", "-", "+", "1e5", "inf", "nan", "NaN", "NAN", "NA", "na", "1.2.3", "1,5", " 1", "1 ", "27.", ".5", "-.5", "+0.25", "007", "-0", "-0.04",
             "0.0000000001", "-0.0000000001", "4611686018427387903", "4611686018427387904", "461168601842738790.3", "99999999999999999999", "1000000000.0", "0.00001"]
    texts += ["%s%d.%s" % (rng.choice(["", "-", "+"]), rng.integers(0, 10 ** 6), "".join(rng.choice(list("0123456789"), rng.integers(0, 9)))) for _ in range(300)]
    for t in texts:
        for d in (0, 1, 5):
            st, v = answer(R.fixed_parse, t, d)
            if st == 0 and v != R.ABSENT and abs(v) >= 10 ** 18:          # more than 18 digits: the library refuses, the restatement has no limit
                st, v = R.INVALID_DATA, 0
            lines.append("parse\t%s\t%d\t%d\t%d" % (t or "-", d, st, v))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines) - 1


def gt_matrix(case):
    return np.array(case["gt"], dtype=np.int16).reshape(len(case["recs"]), case["n_haps"])
