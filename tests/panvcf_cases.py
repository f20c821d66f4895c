"""Seeded cases of the pangenome-VCF tests: a reference, records with a chosen mix of variant kinds, a genotype matrix with a chosen
non-reference rate; the flat arrays the library takes, and the text of a VCF that holds them."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_seq(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def make_case(seed, ref_len, n_recs, n_cols, nonref_rate, missing_rate=0.0, ref_start=1000, max_alt=3, max_indel=30):
    """-> (ref_start, ref_end, ref_seq bytes, records [(pos, [REF, ALT...])] sorted by position and inside the interval, gt int16 [n_recs][n_cols])"""
    rng = np.random.default_rng(seed)
    ref = random_seq(rng, ref_len)
    ref_end = ref_start + ref_len
    pos = np.sort(rng.integers(ref_start, ref_end, n_recs))
    records = []
    for p in pos:
        p = int(p)
        kind = int(rng.integers(0, 5))
        rl = 1 if kind in (0, 2) else int(rng.integers(2, max_indel)) if kind in (1, 3) else int(rng.integers(1, 4))
        rl = min(rl, ref_end - p)
        alleles = [ref[p - ref_start:p - ref_start + rl]]
        for _ in range(int(rng.integers(1, max_alt + 1))):
            if kind == 0:
                alt = random_seq(rng, 1)                                    # SNP (may repeat the reference base: still an allele)
            elif kind == 1:
                alt = random_seq(rng, rl)                                   # MNP
            elif kind == 2:
                alt = alleles[0] + random_seq(rng, int(rng.integers(1, max_indel)))      # insertion
            elif kind == 3:
                alt = alleles[0][:1]                                        # deletion
            else:
                alt = random_seq(rng, int(rng.integers(1, max_indel)))      # replacement of another length
            alleles.append(alt)
        records.append((p, alleles))
    gt = np.zeros((n_recs, n_cols), dtype=np.int16)
    if n_recs:
        n_alt = np.array([len(a) - 1 for _, a in records])
        draw = rng.random((n_recs, n_cols))
        which = (rng.integers(0, 1 << 30, (n_recs, n_cols)) % n_alt[:, None]) + 1
        gt[draw < nonref_rate] = which[draw < nonref_rate].astype(np.int16)
        gt[(draw >= nonref_rate) & (draw < nonref_rate + missing_rate)] = -1
    return ref_start, ref_end, ref, records, gt


def flat(records):
    """The arrays of lcty_vcf_region for a list of records."""
    pos = np.array([p for p, _ in records], dtype=np.uint32)
    ref_len = np.array([len(a[0]) for _, a in records], dtype=np.uint32)
    rec_allele = np.zeros(len(records) + 1, dtype=np.uint32)
    lens, pool = [], bytearray()
    for i, (_, a) in enumerate(records):
        rec_allele[i + 1] = rec_allele[i] + len(a)
        for x in a:
            lens.append(len(x))
            pool += x
    allele_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    allele_off[1:] = np.cumsum(np.array(lens, dtype=np.uint64)) if lens else []
    return {"pos": pos, "ref_len": ref_len, "rec_allele": rec_allele, "allele_off": allele_off,
            "allele_bytes": np.frombuffer(bytes(pool), dtype=np.uint8) if pool else np.zeros(0, dtype=np.uint8)}


def vcf_text(contig, records, samples, ploidy, gt, sep="|", extra_format=False, gt_first=True):
    """A VCF of the records (0-based positions) for samples with the given ploidies; gt [n_recs][sum(ploidy)], -1 = '.'."""
    lines = ["##fileformat=VCFv4.2", f"##contig=<ID={contig}>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
             "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + list(samples))]
    for i, (pos, alleles) in enumerate(records):
        cols, c = [], 0
        for pl in ploidy:
            call = sep.join("." if gt[i][c + h] < 0 else str(int(gt[i][c + h])) for h in range(pl))
            cols.append(call if not extra_format else call + ":7" if gt_first else "7:" + call)
            c += pl
        alt = ",".join(a.decode() for a in alleles[1:]) or "."
        lines.append("\t".join([contig, str(pos + 1), ".", alleles[0].decode(), alt, ".", ".", ".", ("GT:DP" if gt_first else "DP:GT") if extra_format else "GT"] + cols))
    return ("\n".join(lines) + "\n").encode()


def bgzf(data, block=4096):
    """BGZF: gzip members with the BC extra field, and the empty end-of-file block."""
    import struct
    import zlib
    out = bytearray()
    chunks = [data[i:i + block] for i in range(0, len(data), block)] + [b""]
    for ch in chunks:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(ch) + co.flush()
        size = 12 + 6 + len(body) + 8
        out += b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, size - 1)
        out += body + struct.pack("<II", zlib.crc32(ch) & 0xFFFFFFFF, len(ch))
    return bytes(out)
