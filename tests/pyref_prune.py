"""Transliteration of `locityper prune` for one locus (src/command/prune.rs, src/seq/paf.rs:237-267, src/ext/trimat.rs, src/math/mod.rs:267-295,
src/seq/contigs.rs:488-528), independent of the library: nothing here shares a closed form with lcty_prune.hip.

The clustering itself is NOT in the reference tree (kodama, a port of fastcluster that documents its output as SciPy's). `linkage` below is
the contract of DESIGN.md 5j written the naive way: the whole matrix is searched at every step."""
import math

import numpy as np

from tests import pyref_db as DB

POWER_MIN, POWER_MAX = "min", "max"


# ---- src/ext/trimat.rs ------------------------------------------------------------------------------------------------------------------
def triangle_indices(n):
    return [(i, j) for i in range(n - 1) for j in range(i + 1, n)] if n > 1 else []


def to_linear_index(n, i, j):
    assert i < j < n
    return (2 * n - 3 - i) * i // 2 + j - 1


def get_symmetric(tri, n, i, j):
    assert i != j
    return tri[to_linear_index(n, i, j)] if i < j else tri[to_linear_index(n, j, i)]


def thin_out_triangle(tri, n, ixs):
    return [get_symmetric(tri, n, ixs[i], ixs[j]) for i, j in triangle_indices(len(ixs))]


# ---- complete linkage: the contract ----------------------------------------------------------------------------------------------------
def linkage(tri, n):
    """[(cluster1, cluster2, dissimilarity, size)] * (n - 1). The active clusters are kept in ascending LABEL order (a new cluster has the
    largest label and goes last), values above the diagonal, NaN elsewhere; the first minimum of the row-major scan is therefore the
    pair of smallest a, then smallest b."""
    labels = list(range(n))
    sizes = [1] * n
    D = np.full((n, n), np.nan)
    for (i, j), v in zip(triangle_indices(n), tri):
        D[i, j] = v
    steps = []
    for s in range(n - 1):
        k = len(labels)
        if k == 2 or np.nanmin(D) == np.inf:
            i, j = 0, 1                                  # every value left is +inf: the first pair in label order
        else:
            i, j = divmod(int(np.nanargmin(D)), k)
        assert i < j
        d = D[i, j]
        ar = np.arange(k)
        full_i = np.where(ar < i, D[:, i], D[i, :])
        full_j = np.where(ar < j, D[:, j], D[j, :])
        v = np.maximum(full_i, full_j)
        steps.append((labels[i], labels[j], float(d), sizes[i] + sizes[j]))
        keep = [x for x in range(k) if x != i and x != j]
        E = np.full((k - 1, k - 1), np.nan)
        E[:k - 2, :k - 2] = D[np.ix_(keep, keep)]
        E[:k - 2, k - 2] = v[keep]
        D = E
        labels = [labels[x] for x in keep] + [n + s]
        sizes = [sizes[x] for x in keep] + [steps[-1][3]]
    return steps


# ---- src/math/mod.rs:267-295 ---------------------------------------------------------------------------------------------------------------
def powi(a, b):
    """compiler-rt's __powidf2, what f64::powi calls with a run-time exponent."""
    recip = b < 0
    r = 1.0
    while True:
        if b & 1:
            r *= a
        b = int(b / 2)                                   # C division: towards zero
        if b == 0:
            break
        a *= a
    return 1.0 / r if recip else r


def update_mult(power, acc, val, mult):
    if power == POWER_MIN:
        return min(acc, val)
    if power == POWER_MAX:
        return max(acc, val)
    if power == 0:
        return acc + mult * math.log(val)
    return acc + mult * powi(val, power)


# ---- src/command/prune.rs ---------------------------------------------------------------------------------------------------------------
def _rust_parse_f64(s):
    low = s.lower()
    body = low[1:] if low[:1] in "+-" else low
    if body in ("inf", "infinity", "nan"):
        return float(low)
    import re
    if not re.fullmatch(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", s):
        raise ValueError(s)
    return float(s)


class ParsingError(Exception):
    pass


class InvalidInput(Exception):
    pass


def _lines(text):
    ls = text.split("\n")
    if ls and ls[-1] == "":
        ls.pop()
    return [l[:-1] if l.endswith("\r") else l for l in ls]


def load_divergences(text, names, field="dv", repl_missing=0.002):
    """load_divergences (159-230): (triangle list, dict of the counts it logs)."""
    ids = {}
    for i, nm in enumerate(names):
        ids.setdefault(nm, i)
    n = len(names)
    prefix = field + ":"
    crop = len(prefix) + 2
    tri = [math.nan] * (n * (n - 1) // 2)
    stats = {"n_missing": 0, "n_negative": 0, "n_conflicting": 0, "missing_i": 0xFFFFFFFF, "missing_j": 0xFFFFFFFF}
    for line in _lines(text):
        split = line.rstrip(" \t\r\n\x0b\x0c").split("\t")
        if split[0] not in ids:
            continue
        if split[5] not in ids:
            continue
        id1, id2 = ids[split[0]], ids[split[5]]
        if id1 == id2:
            continue
        val = None
        for v in split[12:]:
            if v.startswith(prefix):
                try:
                    val = _rust_parse_f64(v[crop:])
                except ValueError:
                    raise ParsingError(v)
                break
        if val is None:
            continue
        if val < 0.0:
            stats["n_negative"] += 1
            continue
        k = to_linear_index(n, min(id1, id2), max(id1, id2))
        if not math.isnan(tri[k]) and tri[k] != val:
            stats["n_conflicting"] += 1
            continue
        tri[k] = val
    for k, (i, j) in enumerate(triangle_indices(n)):
        if math.isnan(tri[k]):
            stats["n_missing"] += 1
            stats["missing_i"], stats["missing_j"] = i, j
            tri[k] = repl_missing
    if stats["n_missing"] == len(tri):
        raise InvalidInput("Divergence missing for all haplotype pairs")
    return tri, stats


def load_discarded(text, names):
    """DiscardedHaplotypes::load: ({contig id: [names]}, all_identical)."""
    by_contig, unknown, all_identical = {}, {}, True
    known = set(names)
    for line in _lines(text):
        split = line.split()
        if len(split) < 3:
            raise InvalidInput("Each line in discarded haplotypes must have at least 3 columns")
        all_identical = all_identical and split[1] == "="
        rhs = []
        for c in split[2:]:
            c = c[:-1] if c.endswith(",") else c
            if c in known:
                continue
            rhs.append(c)
            if c in unknown:
                rhs.extend(unknown.pop(c))
        if split[0] in known:
            by_contig[names.index(split[0])] = rhs
        else:
            unknown[split[0]] = rhs
    return by_contig, all_identical


def fmt8(v):
    """Rust's {:.8}"""
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "-inf" if v < 0 else "inf"
    return "%.8f" % v


class Cluster:
    def __init__(self, i, name):
        self.haps = [(i, 1)]
        self.newick = name
        self.div = 0.0

    def add_identical(self, names):
        assert len(self.haps) == 1
        self.newick = "(" + self.newick + ":0"
        for h in names:
            self.newick += ",%s:0" % h
            self.haps[0] = (self.haps[0][0], self.haps[0][1] + 1)
        self.newick += ")"

    @staticmethod
    def merge_and_clear(first, second, div):
        c = Cluster.__new__(Cluster)
        c.haps = first.haps + second.haps
        first.haps, second.haps = [], []
        c.newick = "(%s:%s,%s:%s)" % (first.newick, fmt8(0.5 * (div - first.div)), second.newick, fmt8(0.5 * (div - second.div)))
        first.newick = second.newick = ""
        c.div = div
        return c

    def select_representative(self, tri, n, epsilon, power):
        """276-304: (representative id, the accumulators)."""
        buf = [0.0] * len(self.haps)
        for i, (id1, mult1) in enumerate(self.haps):
            if mult1 > 1:
                buf[i] = update_mult(power, buf[i], epsilon, float(mult1 - 1))
            for j in range(i + 1, len(self.haps)):
                id2, mult2 = self.haps[j]
                div = epsilon + get_symmetric(tri, n, id1, id2)
                buf[i] = update_mult(power, buf[i], div, float(mult2))
                buf[j] = update_mult(power, buf[j], div, float(mult1))
        k = 0
        want_max = power not in (POWER_MIN, POWER_MAX) and power < 0
        for i in range(1, len(buf)):
            if (buf[i] > buf[k]) if want_max else (buf[i] < buf[k]):
                k = i
        return self.haps[k][0], buf


def select_cut_threshold(steps, n, n_clusters):
    if n < n_clusters + 1:
        return 0.0
    return steps[n - n_clusters - 1][2]


def cluster_haplotypes(names, tri, thresh=0.0002, n_clusters=None, power=2, disc=None, steps=None):
    """cluster_haplotypes (350-427). disc: {contig id: [names]} of the old discarded_haplotypes.txt. Returns a dict: steps, threshold,
    epsilon, clusters [[ids]] in the order process_cluster meets them, acc [[accumulators]] ([] for clusters of one), repr, keep_ids,
    newick, new_lines (the text cluster_haplotypes appends to the old discarded_haplotypes.txt)."""
    n = len(names)
    tri = [float(x) for x in tri]
    min_val = min(tri) if tri else None
    epsilon = max(1e-6 * min_val, 1e-12) if tri else 1e-12
    if steps is None:
        steps = linkage(tri, n)
    if n_clusters is not None:
        thresh = select_cut_threshold(steps, n, n_clusters)
    clusters = [Cluster(i, names[i]) for i in range(n)]
    for i, hs in (disc or {}).items():
        clusters[i].add_identical(hs)
    out = {"steps": steps, "threshold": thresh, "epsilon": epsilon, "clusters": [], "acc": [], "repr": [], "new_lines": ""}

    def process_cluster(c):
        if len(c.haps) == 0:
            return False
        out["clusters"].append([h for h, _ in c.haps])
        if len(c.haps) == 1:
            out["repr"].append(c.haps[0][0])
            out["acc"].append([])
        else:
            rep, buf = c.select_representative(tri, n, epsilon, power)
            out["repr"].append(rep)
            out["acc"].append(buf)
            line = names[rep] + " "
            sep = "~"
            for h, _ in c.haps:
                if h != rep:
                    line += "%s %s" % (sep, names[h])
                    sep = ","
            out["new_lines"] += line + "\n"
        return True

    for c1, c2, d, _ in steps:
        if d > thresh:
            for c in (clusters[c1], clusters[c2]):
                if process_cluster(c):
                    c.haps = []
        clusters.append(Cluster.merge_and_clear(clusters[c1], clusters[c2], d))
    for c in clusters:
        process_cluster(c)
    assert len(clusters) == 2 * n - 1
    out["newick"] = clusters[-1].newick + ";\n"
    out["keep_ids"] = sorted(out["repr"])
    return out


# ---- src/seq/paf.rs:237-267 ---------------------------------------------------------------------------------------------------------------
def prune_paf(text, names, keep_ids):
    keep = set(names[i] for i in keep_ids)
    out = ""
    for line in _lines(text):
        if line.startswith("#"):
            out += line + "\n"
            continue
        split = line.split("\t", 6)
        if len(split) < 7:
            raise ParsingError(line)
        if split[0] in keep and split[5] in keep:
            out += line + "\n"
    return out


# ---- prune_files (471-518) ----------------------------------------------------------------------------------------------------------------
def read_varint(buf, p):
    v, shift = 0, 0
    while True:
        b = buf[p]
        p += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, p
        shift += 7


def kmer_counts_load(buf, p=0):
    """KmerCounts::load: (k, counter bytes as save would write them, [[counts]], next position)."""
    k, byte_len = buf[p], buf[p + 1]
    p += 2
    max_value = min(65535, (1 << (8 * byte_len)) - 1)
    n, p = read_varint(buf, p)
    counts = []
    for _ in range(n):
        m, p = read_varint(buf, p)
        cur = []
        for _ in range(m):
            v, p = read_varint(buf, p)
            cur.append(min(v, max_value))
        counts.append(cur)
    return k, bin(max_value).count("1") // 8, counts, p


def thin_kmers(buf, keep_ids):
    out = b""
    p = 0
    for _ in range(2):
        k, cb, counts, p = kmer_counts_load(buf, p)
        out += DB.kmer_counts_save(k, cb, [counts[i] for i in keep_ids])
    return out


def thin_distances(buf, n, keep_ids):
    k, w = buf[0], buf[1]
    m, p = read_varint(buf, 2)
    assert m == n
    tri = []
    for _ in range(n * (n - 1) // 2):
        v, p = read_varint(buf, p)
        tri.append(v)
    return DB.write_divergences(k, w, len(keep_ids), thin_out_triangle(tri, n, keep_ids))


def write_fasta(names, seqs, keep_ids):
    return b"".join(b">" + names[i].encode() + b"\n" + bytes(seqs[i]) + b"\n" for i in keep_ids)


def prune_locus(names, seqs, paf_text, kmers=None, distances=None, discarded=None, field="dv", thresh=0.0002, n_clusters=None, power=2,
                only_tree=False, skip_tree=False):
    """process_locus + prune_files on the decompressed contents of the locus directory; the dict of files (bytes; None = not written)."""
    repl = math.inf if n_clusters is not None else 10.0 * thresh
    tri, _ = load_divergences(paf_text, names, field, repl)
    old = b""
    disc = {}
    if not skip_tree and discarded is not None:
        old = bytes(discarded)
        disc, _ = load_discarded(old.decode(), names)
    res = cluster_haplotypes(names, tri, thresh, n_clusters, power, disc)
    files = {"newick": None if skip_tree else res["newick"].encode(), "keep": res["keep_ids"], "discarded": None, "fasta": None, "kmers": None,
             "distances": None, "paf": None, "unchanged": False}
    if only_tree:
        return files
    text = old + res["new_lines"].encode()
    files["discarded"] = text if text else None
    keep = res["keep_ids"]
    if len(keep) == len(names):
        files["unchanged"] = True
        return files
    files["fasta"] = write_fasta(names, seqs, keep)
    if kmers is not None:
        files["kmers"] = thin_kmers(kmers, keep)
    if distances is not None:
        files["distances"] = thin_distances(distances, len(names), keep)
    files["paf"] = prune_paf(paf_text, names, keep).encode()
    return files
