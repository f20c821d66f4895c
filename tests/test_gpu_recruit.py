"""Minimizer read recruitment on the device against the oracle, through the C ABI: bit-exact (sets of loci)."""
import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from locityper_amd.cdefs import ReadsChunk
from tests import oracle_ffi as O
from tests.helpers import noisy_read
from tests.test_oracle_recruit import _loci, _loci_with_other_bases, revcomp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ctx():
    return api.Context(0)


def _both(ctx, loci, base_k=25, **over):
    prm = api.recruit_params(**over)
    gt = api.Targets(ctx, prm)
    ot = O.OracleTargets(prm.minimizer_k, prm.minimizer_w, prm.match_frac, prm.match_length, prm.thresh_kmer_count)
    rng = np.random.default_rng(9)
    for alleles in loci:
        counts = [np.where(rng.random(len(a) - base_k + 1) < 0.1, 80, 0).astype(np.uint16) for a in alleles]
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64)
        cnt_off = np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64)
        gt.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, base_k)
        ot.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, base_k)
    n = gt.finalize(); ot.finalize()
    assert n == len({e[0] for e in ot.entries()})
    return gt, ot


def _reads(rng, loci, n, lens=(150, 150)):
    pairs = []
    for i in range(n):
        li = int(rng.integers(0, len(loci))); al = loci[li][int(rng.integers(0, len(loci[li])))]
        kind = i % 7
        l1 = int(rng.integers(lens[0], lens[1] + 1)); l2 = int(rng.integers(lens[0], lens[1] + 1))
        if kind == 6:
            r1 = bytes(rng.choice(list(b"ACGT"), l1).tolist()); r2 = bytes(rng.choice(list(b"ACGT"), l2).tolist())
        else:
            p = int(rng.integers(0, len(al) - 800))
            r1, _ = noisy_read(rng, al, p, l1, err=0.02 * (kind % 3)); r2, _ = noisy_read(rng, al, p + 300, l2, err=0.02 * (kind % 3))
            r2 = revcomp(r2)
            if kind == 4: r1 = r1[:30] + b"NN" + r1[32:]
            if kind == 5: r2 = r2[:10] + b"N" * 60 + r2[70:]
            if i % 2: r1, r2 = revcomp(r1), revcomp(r2)
        pairs.append({"seq1": r1.decode(), "seq2": r2.decode(), "recs": []})
    return pairs


@pytest.mark.parametrize("over", [dict(), dict(minimizer_k=27, minimizer_w=5, match_frac=0.7), dict(minimizer_k=11, minimizer_w=20, match_frac=0.3),
                                  dict(minimizer_k=31, minimizer_w=31, match_frac=0.5), dict(thresh_kmer_count=200),
                                  dict(minimizer_k=9, minimizer_w=45, match_frac=0.4), dict(minimizer_k=20, minimizer_w=2, match_frac=0.6)])
def test_read_pairs_and_single_reads_match_oracle(gpu_ctx, over):
    rng = np.random.default_rng(5)
    loci = _loci(rng, n_loci=4)
    gt, ot = _both(gpu_ctx, loci, **over)
    pairs = _reads(rng, loci, 700, lens=(60, 250))
    ch = ReadsChunk.from_pairs(pairs)
    cnt, out = gt.recruit(ch, paired=True)
    n_rec = n_multi = 0
    for i, pr in enumerate(pairs):
        exp = ot.recruit(pr["seq1"].encode(), pr["seq2"].encode())
        assert list(out[i, :cnt[i]]) == exp, (i, over)
        n_rec += bool(exp); n_multi += len(exp) > 1
    assert n_rec > 100 and n_multi > 5
    cnt, out = gt.recruit(ch, paired=False)
    for i, pr in enumerate(pairs):
        assert list(out[i, :cnt[i]]) == ot.recruit(pr["seq1"].encode()), (i, over)


def _pairs_of_other_bases(loci, seed):
    """200 read pairs of 150 bases copied from the alleles (every third with three substitutions); every tenth pair starts inside or
    just before the run of N of loci[1][1], so that a mate crosses it."""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(200):
        if i % 10 == 0: li, ai, p = 1, 1, int(rng.integers(560, 720))
        else: li, ai, p = int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 2000 - 450))
        al = loci[li][ai]
        r1, r2 = bytearray(al[p:p + 150]), bytearray(al[p + 300:p + 450])
        if i % 3 == 1:
            for r in (r1, r2):
                for q in rng.integers(0, 150, 3): r[int(q)] = b"ACGT"[int(rng.integers(0, 4))]
        r1, r2 = bytes(r1), revcomp(bytes(r2))
        if i % 2: r1, r2 = revcomp(r1), revcomp(r2)
        pairs.append({"seq1": r1.decode(), "seq2": r2.decode(), "recs": []})
    return pairs


@pytest.mark.parametrize("over", [dict(), dict(minimizer_k=11, minimizer_w=20, match_frac=0.3), dict(minimizer_k=27, minimizer_w=5, match_frac=0.7)])
def test_alleles_and_reads_with_other_bases_match_oracle(gpu_ctx, over):
    """Targets made from alleles that start with N, hold a run of N longer than w, a lower-case stretch and an R (the host walk of
    lcty_targets_add_locus), and reads drawn from them (the device walk as written): sets of loci as the oracle's, read by read."""
    loci = _loci_with_other_bases(np.random.default_rng(41))
    gt, ot = _both(gpu_ctx, loci, **over)                                    # asserts the number of distinct minimizers
    pairs = _pairs_of_other_bases(loci, 43)
    assert sum("N" in p["seq1"] or "N" in p["seq2"] for p in pairs) >= 10
    ch = ReadsChunk.from_pairs(pairs)
    for paired in (True, False):
        cnt, out = gt.recruit(ch, paired=paired)
        n_rec = 0
        for i, pr in enumerate(pairs):
            exp = ot.recruit(pr["seq1"].encode(), pr["seq2"].encode()) if paired else ot.recruit(pr["seq1"].encode())
            assert list(out[i, :cnt[i]]) == exp, (i, paired, over)
            n_rec += bool(exp)
        assert n_rec >= 1, (paired, over)
    gt.close()


def test_edges_and_misuse(gpu_ctx):
    rng = np.random.default_rng(7)
    loci = _loci(rng, n_loci=3)
    gt, ot = _both(gpu_ctx, loci)
    al = loci[0][0]
    # reads shorter than k + w - 1, empty mates, all-N reads, a read pair whose second mate is foreign
    pairs = [{"seq1": al[100:110].decode(), "seq2": al[400:420].decode(), "recs": []},
             {"seq1": "N" * 150, "seq2": al[400:550].decode(), "recs": []},
             {"seq1": al[100:250].decode(), "seq2": "ACGT" * 40, "recs": []},
             {"seq1": al[100:250].decode(), "seq2": revcomp(al[400:550]).decode(), "recs": []},
             {"seq1": al[100:124].decode(), "seq2": al[400:424].decode(), "recs": []}]
    ch = ReadsChunk.from_pairs(pairs)
    cnt, out = gt.recruit(ch, paired=True)
    for i, pr in enumerate(pairs):
        assert list(out[i, :cnt[i]]) == ot.recruit(pr["seq1"].encode(), pr["seq2"].encode()), i
    assert list(cnt) == [0, 0, 0, 1, 0] or cnt[3] == 1
    # mates of a pair beyond 256 bases are refused, never answered differently
    long_pair = ReadsChunk.from_pairs([{"seq1": al[:300].decode(), "seq2": al[400:700].decode(), "recs": []}])
    with pytest.raises(_lib.LocityperError) as ei:
        gt.recruit(long_pair, paired=True)
    assert ei.value.code == cdefs.ERR_UNSUPPORTED
    with pytest.raises(_lib.LocityperError):
        api.Targets(gpu_ctx, api.recruit_params(match_frac=0.1))
    with pytest.raises(_lib.LocityperError):
        api.Targets(gpu_ctx, api.recruit_params(minimizer_k=32))
    empty = api.Targets(gpu_ctx, api.recruit_params())
    with pytest.raises(_lib.LocityperError):
        empty.finalize()                                                      # "No minimizers for recruitment"


@pytest.mark.parametrize("over", [dict(technology=cdefs.TECH_NANOPORE, paired=False), dict(technology=cdefs.TECH_NANOPORE, paired=False, minimizer_k=19, minimizer_w=24, match_length=800),
                                  dict(technology=cdefs.TECH_ILLUMINA, paired=False)])
def test_single_reads_of_every_length_match_oracle(gpu_ctx, over):
    """recruit_short_read up to 500 bases, recruit_long_read (rare fraction, threshold, has_matching_stretch) beyond — one wavefront per read
    above 256 bases; reads with other bases than ACGT take the reference's procedure as written."""
    rng = np.random.default_rng(13)
    loci = _loci(rng, n_loci=3, length=9000)
    gt, ot = _both(gpu_ctx, loci, **over)
    reads = []
    for i in range(260):
        li = int(rng.integers(0, 3)); al = loci[li][int(rng.integers(0, 3))]
        kind = i % 8
        ln = int(rng.integers(100, 700)) if kind < 3 else int(rng.integers(700, 7000))
        p = int(rng.integers(0, len(al) - ln))
        r, _ = noisy_read(rng, al, p, ln, err=0.03 * (i % 4))
        if kind == 5: r = bytes(rng.choice(list(b"ACGT"), 2500).tolist()) + r[:900]          # mostly foreign: the stretch decides
        if kind == 6: r = r[:len(r) // 2] + b"N" * 3 + r[len(r) // 2 + 3:]
        if kind == 7: r = bytes(rng.choice(list(b"ACGT"), len(r)).tolist())
        if i % 2: r = revcomp(r)
        reads.append({"seq1": r.decode(), "seq2": None, "recs": []})
    ch = ReadsChunk.from_pairs(reads)
    cnt, out = gt.recruit(ch, paired=False, max_out=4)
    n_rec = n_long_rec = 0
    for i, rd in enumerate(reads):
        exp = ot.recruit(rd["seq1"].encode())
        assert list(out[i, :cnt[i]]) == exp, (i, len(rd["seq1"]), over)
        n_rec += bool(exp); n_long_rec += bool(exp) and len(rd["seq1"]) > 500
    assert n_rec > 60 and n_long_rec > 30, (n_rec, n_long_rec)


def test_fastq_files_through_the_readers_the_kernel_and_the_per_locus_writers(gpu_ctx, tmp_path):
    """recruit_single_thread's loop (src/seq/recruit.rs:1010-1024) with the library's own readers and writers (lcty_fastx.hip): two gzip
    FASTQ files -> chunks of 64 read pairs -> lcty_recruit -> `reads.fq` of every locus. Every locus' file must hold exactly the
    pairs the oracle's recruit_read_pair recruits to it, in input order, both mates one after the other, as write_fastq leaves them."""
    import gzip
    from locityper_amd import io as lio
    rng = np.random.default_rng(21)
    loci = _loci(rng, n_loci=3)
    gt, ot = _both(gpu_ctx, loci)
    pairs = _reads(rng, loci, 300)
    qual = lambda n: "".join(chr(33 + int(q)) for q in rng.integers(2, 40, n))
    recs = [(f"pair{i}/1 some description", p["seq1"], qual(len(p["seq1"])), f"pair{i}/2", p["seq2"], qual(len(p["seq2"]))) for i, p in enumerate(pairs)]
    with gzip.open(tmp_path / "r1.fq.gz", "wt") as a, gzip.open(tmp_path / "r2.fq.gz", "wt") as b:
        for n1, s1, q1, n2, s2, q2 in recs:
            a.write(f"@{n1}\n{s1}\n+\n{q1}\n")
            b.write(f"@{n2}\n{s2}\n+\n{q2}\n")
    want = [""] * len(loci)
    for n1, s1, q1, n2, s2, q2 in recs:
        for l in ot.recruit(s1.encode(), s2.encode()):
            want[l] += f"@{n1.split(' ')[0]}\n{s1}\n+\n{q1}\n@{n2}\n{s2}\n+\n{q2}\n"
    assert sum(1 for w in want if w) >= 2                                   # the sample recruits to several loci
    out = [tmp_path / f"locus{l}.fq" for l in range(len(loci))]
    writers = lio.FastxWriters(out)
    f = lio.Fastx(tmp_path / "r1.fq.gz", tmp_path / "r2.fq.gz")
    n_pairs = n_recruited = 0
    while True:
        ch = f.next(64)
        if ch is None:
            break
        cnt, lc = gt.recruit(ch, paired=True)
        n_recruited += f.write_recruited(writers, cnt, lc)
        n_pairs += ch.n_pairs
    writers.close()
    assert n_pairs == 300 and n_recruited == sum(1 for r in recs if ot.recruit(r[1].encode(), r[4].encode()))
    for l in range(len(loci)):
        assert out[l].read_text() == want[l]
    gt.close()
