"""Independent numpy / scipy restatement of the background estimate of `locityper preproc -a` (lcty_bg.hip, lcty_bg_reads_load),
written from the reference's semantics (src/command/preproc.rs:988-1155, src/bg/*.rs, src/seq/cigar.rs, src/seq/aln.rs,
src/algo/loess.rs, src/math/distr/*.rs). The extended CIGAR is built here base by base; LOESS is solved with numpy.linalg.lstsq and
both Nelder–Mead fits run through scipy.optimize.minimize to a tight tolerance."""
import gzip
import struct

import numpy as np
from scipy import optimize, special

OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
CONSUMES_REF = set("MDN=X")
CONSUMES_QUERY = set("MIS=X")


class PyrefError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


INVALID_INPUT, INVALID_DATA, RUNTIME = 1, 2, 3


# ---- BAM -------------------------------------------------------------------------------------------------------------------------
def parse_bam(path):
    b = gzip.open(path, "rb").read()
    assert b[:4] == b"BAM\1"
    i = 4
    l_text, = struct.unpack_from("<I", b, i); i += 4 + l_text
    n_ref, = struct.unpack_from("<I", b, i); i += 4
    refs = []
    for _ in range(n_ref):
        ln, = struct.unpack_from("<I", b, i); i += 4
        refs.append(b[i:i + ln - 1].decode()); i += ln + 4
    recs = []
    while i < len(b):
        bs, = struct.unpack_from("<I", b, i); i += 4
        tid, pos, lrn, mapq, _bin, ncig, flag, lseq = struct.unpack_from("<iiBBHHHI", b, i)
        j = i + 32
        name = b[j:j + lrn - 1].decode(); j += lrn
        cig = [(OPS[w & 15], w >> 4) for w in struct.unpack_from("<%dI" % ncig, b, j)]; j += 4 * ncig
        seq = "".join(NT16[(b[j + (k >> 1)] >> (4 * (1 - (k & 1)))) & 15] for k in range(lseq))
        recs.append(dict(tid=tid, pos=pos, name=name, mapq=mapq, flag=flag, cigar=cig, seq=seq))
        i += bs
    return refs, recs


def ref_len(cigar):
    return sum(n for o, n in cigar if o in CONSUMES_REF)


def clipping_rate(rec):
    """raw_clipping / seq_len (seq/cigar.rs:944-966): first and last op that consume no reference (a one-op CIGAR twice)."""
    c = rec["cigar"]
    clip = (c[0][1] if c[0][0] not in CONSUMES_REF else 0) + (c[-1][1] if c[-1][0] not in CONSUMES_REF else 0)
    return 0.0 if clip == 0 else clip / len(rec["seq"])


def infer_ext_cigar(rec, padded_seq, padded_start):
    """Cigar::infer_ext_cigar (seq/cigar.rs:434-476): None when an M run leaves the padded sequence (end at or past its end)."""
    end = padded_start + len(padded_seq)
    rlen = qlen = 0
    out = []
    for o, n in rec["cigar"]:
        if o != "M":
            out.append((o, n))
        else:
            if rec["pos"] + rlen < padded_start or rec["pos"] + rlen + n >= end:
                return None
            r0 = rec["pos"] + rlen - padded_start
            eq = [padded_seq[r0 + t] == rec["seq"][qlen + t] for t in range(n)]
            t = 0
            while t < n:                                                # runs of = / X inside this M op
                u = t
                while u < n and eq[u] == eq[t]:
                    u += 1
                out.append(("=" if eq[t] else "X", u - t))
                t = u
        if o in CONSUMES_REF:
            rlen += n
        if o in CONSUMES_QUERY:
            qlen += n
    if len(rec["seq"]) and qlen != len(rec["seq"]):
        raise PyrefError(INVALID_DATA, "Failed to convert CIGAR")
    return out


def load_alns(path, contig, start, end, padded_seq, padded_start, min_mapq=30, max_clipping=0.02, technology=0):
    refs, recs = parse_bam(path)
    tid = refs.index(contig)
    if isinstance(padded_seq, (bytes, bytearray)):
        padded_seq = padded_seq.decode()
    kept, ignored, wo = [], 0, 0
    paired_counts = [0, 0]
    for r in recs:
        if r["tid"] != tid or r["pos"] < 0:
            continue
        rl = ref_len(r["cigar"])
        rend = r["pos"] + (1 if (r["flag"] & 4) or rl == 0 else rl)
        if not (r["pos"] < end and rend > start):
            continue
        if not (r["flag"] & 3844 == 0 and r["mapq"] >= min_mapq and clipping_rate(r) <= max_clipping):
            ignored += 1
            continue
        ext = infer_ext_cigar(r, padded_seq, padded_start)
        if ext is None:
            wo += 1
            continue
        if any(o not in "MIDS=X" for o, _ in r["cigar"]):
            raise PyrefError(INVALID_DATA, "unsupported op")
        r = dict(r, ext=ext, end=r["pos"] + rl, second=bool(r["flag"] & 0x80), reverse=bool(r["flag"] & 0x10))
        paired_counts[r["flag"] & 1] += 1
        kept.append(r)
    if paired_counts[0] and paired_counts[1]:
        raise PyrefError(INVALID_DATA, "BAM file contains both paired and unpaired reads")
    if not kept:
        raise PyrefError(INVALID_DATA, "BAM file contains no reads in the target region")
    paired = paired_counts[1] > 0
    mate = [None] * len(kept)
    if paired:
        by = {}
        for i, r in enumerate(kept):
            slot = by.setdefault(r["name"], [None, None])
            e = int(r["second"])
            if slot[e] is not None:
                raise PyrefError(INVALID_DATA, "several mates")
            slot[e] = i
        for a, b in by.values():
            if a is not None and b is not None:
                mate[a], mate[b] = b, a
    m = min(len(kept), 10000)
    read_len = sum(float(sum(n for o, n in r["cigar"] if o in CONSUMES_QUERY)) for r in kept[:m]) / m
    return dict(recs=kept, ignored=ignored, wo_cigar=wo, paired=paired, mate=mate, read_len=read_len)


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def window_layout(read_len, region_len, window_size=0, boundary=1000):
    w = window_size or int(min(max(int(np.floor(read_len * (2.0 / 3.0) + 0.5)), 20), 5000))
    neighb = max(w, 300)
    nw = (region_len - 2 * boundary) // w
    first = (region_len - nw * w) // 2
    return w, neighb, nw, first


def windows(region_seq, sub_counts, k, region_start, w, neighb, nw, first, uniq_perc=90.0):
    """filter_windows (bg/windows.rs:44-101) on the region's own sequence and k-mer counts."""
    seq = np.frombuffer(region_seq, dtype=np.uint8)
    isgc = (seq == ord("G")) | (seq == ord("C"))
    lp = (neighb - w) // 2
    rp = neighb - w - lp
    starts, gc, frac, keep = [], [], [], []
    for i in range(nw):
        ws = first + i * w
        s = max(ws - lp, 0)
        e = min(ws + w + rp, len(seq))
        e2 = e + 1 - k
        f = np.count_nonzero(sub_counts[s:e2] <= 1) / (e2 - s)
        starts.append(region_start + ws)
        gc.append(100.0 * int(isgc[s:e].sum()) / (e - s))
        frac.append(f)
        keep.append(f >= 0.01 * uniq_perc)
    return np.array(starts, dtype=np.uint32), np.array(gc), np.array(frac), np.array(keep, dtype=bool)


# ---- per-record counts -----------------------------------------------------------------------------------------------------------
def count_region_operations(pos, ext, rs, re):
    """seq/aln.rs:241-281 on an extended CIGAR."""
    m = x = i = d = s = 0
    rpos = pos
    for t, (o, n) in enumerate(ext):
        ov = max(min(rpos + n, re) - max(rpos, rs), 0)
        if o == "=":
            m += ov; rpos += n
        elif o == "X":
            x += ov; rpos += n
        elif o == "D":
            d += ov; rpos += n
        elif o == "I":
            i += n if rs <= rpos < re else 0
        elif o == "S":
            s += min(n, max(rpos - rs, 0)) if t == 0 else min(n, max(re - rpos, 0))
        else:
            raise PyrefError(INVALID_DATA, "Unsupported CIGAR operation " + o)
    return m, x, i, d, s


def record_stats(L, rs, re, win_start, win_end, w):
    out = []
    for r in L["recs"]:
        c = count_region_operations(r["pos"], r["ext"], rs, re)
        common = c[1] + c[2] + c[4]
        mid = (r["pos"] + r["end"]) // 2
        win = (mid - win_start) // w if win_start <= mid < win_end else 0xFFFFFFFF
        out.append(c + (common + c[3], common + c[0], mid, win))
    return np.array(out, dtype=np.int64)                # =, X, I, D, S, edit, read_len, middle, window


# ---- distributions ---------------------------------------------------------------------------------------------------------------
def nbinom_cdf(n, p, k):
    return special.betainc(n, k + 1.0, p)


def nbinom_quantile(n, p, q):
    """WithQuantile::quantile (math/distr/mod.rs:38-75)."""
    mean = n * (1 - p) / p
    low, high = 0, int(2.0 * mean)
    while nbinom_cdf(n, p, high) < q:
        low, high = high, high * 2
    while high >= low:
        mid = (low + high) // 2
        if nbinom_cdf(n, p, mid) >= q:
            high = mid - 1
        else:
            low = mid + 1
    c0, c1 = nbinom_cdf(n, p, high), nbinom_cdf(n, p, high + 1)
    if c1 - c0 == 0:
        return float(high)
    r = (q - c0) / (c1 - c0)
    return high * (1 - r) + (high + 1) * r


def nbinom_corrected(m, v):
    p = m / v
    if p > 0.99999:
        return 0.99999 * m / (1 - 0.99999), 0.99999
    return m * m / (v - m), p


def interpol_quantile(a, q):
    a = np.sort(a)
    f = (len(a) - 1) * q
    i = int(f)
    r = f - np.floor(f)
    return a[i] if r < 1e-6 else a[i] + (a[i + 1] - a[i]) * r


def mean_variance(a):
    a = np.asarray(a, dtype=np.float64)
    m = float(sum(a.tolist())) / len(a)
    return m, float(sum(((a - m) ** 2).tolist())) / (len(a) - 1)


def insert_fit(inserts, same, insert_pval=0.001):
    if len(inserts) < 1000:
        raise PyrefError(INVALID_DATA, "Not enough paired reads")
    keep = inserts < 500000
    ins = inserts[keep]
    orient = [int(np.count_nonzero(~same[keep])), int(np.count_nonzero(same[keep]))]
    tot = orient[0] + orient[1]
    if orient[0] / tot < 0.05 or orient[1] / tot >= 0.05:
        raise PyrefError(INVALID_DATA, "FF orientation is not supported")
    srt = np.sort(ins.astype(np.float64))
    limit = 3.0 * interpol_quantile(srt, 0.99)
    m = int(np.searchsorted(srt, limit, side="right"))
    mean, var = mean_variance(srt[:m])
    n, p = nbinom_corrected(mean, var)
    q = 0.5 * insert_pval
    lo = int(max(0.0, np.floor(nbinom_quantile(n, p, q) - 1e-8)))
    hi = int(np.ceil(nbinom_quantile(n, p, 1 - q) + 1e-8))
    sizes, counts = np.unique(ins, return_counts=True)
    return dict(hist_size=sizes, hist_count=counts, orient=orient, limit=limit, mean=mean, var=var, n=n, p=p, ci=(lo, hi))


def to_ln_probs(tot):
    s = float(tot[0] + tot[1] + tot[2] + tot[3])
    mi, ii, di = (max(tot[j] / s, 1e-5) for j in (1, 2, 3))
    ma = 1.0 - mi - ii - di
    if not ma > 0.5:
        raise PyrefError(INVALID_DATA, "Match probability must be over 50%")
    return np.log([ma, mi, ii, di, max(ii, mi)])


def bb_ln_pmf(k, n, a, b):
    return -special.betaln(n - k + 1.0, k + 1.0) + special.betaln(k + a, n - k + b) - np.log(n + 1.0) - special.betaln(a, b)


def bb_nll(params, triples, unif_coef):
    a, b = params
    if a <= 0 or b <= 0 or a >= 1e5 or b >= 1e5:
        return 1e30
    k, n, w = triples
    return -float(np.sum(w * np.logaddexp(np.log1p(-unif_coef) + bb_ln_pmf(k, n, a, b), np.log(unif_coef))))


def bb_fit(triples, unif_coef):
    best = None
    for x0 in ([0.7, 50.0], [0.3, 100.0], [0.5, 10.0]):
        r = optimize.minimize(bb_nll, x0, args=(triples, unif_coef), method="Nelder-Mead",
                              options=dict(xatol=1e-10, fatol=1e-12, maxiter=200000, maxfev=400000))
        if best is None or r.fun < best.fun:
            best = r
    return best.x, best.fun


def bb_inv_cdf(a, b, n, cdf):
    m = float(n)
    const = -np.log(m + 1.0) - special.betaln(a, b)
    ks = np.arange(0, n + 1, dtype=np.float64)
    lp = -special.betaln(m - ks + 1.0, ks + 1.0) + special.betaln(ks + a, m - ks + b) + const
    c = np.exp(np.logaddexp.accumulate(lp))
    over = np.nonzero(c[1:] > cdf)[0]
    return int(over[0]) if len(over) else n


def nb_reg_cost(x, mean, var, rate, lam):
    n, p = x
    if n <= 0 or p <= 0 or p >= 1:
        return 1e30
    me = rate * n * (1 - p) / p - mean
    ve = rate * n * (1 - p) * (p + rate - p * rate) / (p * p) - var
    return me * me + ve * ve + lam * n


def nb_regularized(mean, var, rate=1.0, lam=1e-5):
    simplex = np.array([[10.0, 0.3], [20.0, 0.7], [30.0, 0.3]])
    r = optimize.minimize(nb_reg_cost, simplex[0], args=(mean, var, rate, lam), method="Nelder-Mead",
                          options=dict(initial_simplex=simplex, xatol=1e-12, fatol=1e-14, maxiter=200000, maxfev=400000))
    return r.x


def nb_mean_var(n, p):
    return n * (1 - p) / p, n * (1 - p) / (p * p)


def tricube(v):
    return 70.0 / 81.0 * (1.0 - np.minimum(np.abs(v), 1.0) ** 3) ** 3


def loess(x, y, w, frac):
    """algo/loess.rs:79-160 with degree 1 at xout = 0..100; the weighted fit through numpy.linalg.lstsq."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    n_frac = max(int(np.floor(n * frac + 0.5)), 1)
    rng_ = x[-1] - x[0]
    out = []
    for xv in range(101):
        a = int(np.searchsorted(x, xv, side="left"))
        b = int(np.searchsorted(x, xv, side="right"))
        cur = b - a
        if cur >= n_frac:
            out.append(sum(y[a:b].tolist()) / cur)
            continue
        rem = n_frac - cur
        if a < n - b:
            left = min(a, rem // 2); right = min(n - b, rem - left)
        else:
            right = min(n - b, rem // 2); left = min(a, rem - right)
        a -= left; b += right
        wt = tricube((x[a:b] - xv) / rng_)
        if w is not None:
            wt = wt * np.asarray(w)[a:b]
        A = np.stack([wt, wt * x[a:b]], axis=1)
        coef = np.linalg.lstsq(A, y[a:b] * wt, rcond=None)[0]
        out.append(coef[0] + coef[1] * xv)
    return np.array(out)


def gc_bins(gc_sorted):
    bins, i = [], 0
    for g in range(101):
        j = int(np.searchsorted(gc_sorted, g + 0.5, side="right"))
        bins.append((i, j)); i = j
    return bins


def depth_model(depth1, gc, keep, frac_windows=0.5, min_tail_obs=100, tail_var_mult=0.02, gc_bias=True, rate=1.0, ploidy=2):
    d = depth1[keep].astype(np.float64)
    g = gc[keep]
    order = np.argsort(g, kind="stable")
    d, g = d[order], g[order]
    bins = gc_bins(g)
    res = dict(gc_nwin=np.array([j - i for i, j in bins]))
    if not gc_bias:
        m, v = mean_variance(d)
        n, p = nb_regularized(m, v, rate)
        res.update(mean=m, var=v, nb_n=np.full(101, n / ploidy), nb_p=np.full(101, p))
        return res
    lm = loess(g, d, None, frac_windows)
    vx, vy, vw = [], [], []
    for gcv, (i, j) in enumerate(bins):
        if j - i >= 10:
            vx.append(float(gcv)); vy.append(mean_variance(d[i:j])[1]); vw.append(np.sqrt((j - i) / len(d)))
    lv = loess(vx, vy, vw, 1.0)
    mtot = bins[-1][1]
    left = next((t for t, (_, e) in enumerate(bins) if e >= min_tail_obs), 101)
    right = 101 - next((p for p, (s, _) in enumerate(reversed(bins)) if mtot - s >= min_tail_obs), 101)
    bm, bv = lm.copy(), lv.copy()
    for t in range(left):
        bm[t] = lm[left]; bv[t] = max((1.0 + (left - t) * tail_var_mult) * lv[left], lv[t])
    for t in range(right + 1, 101):
        bm[t] = lm[right]; bv[t] = max((1.0 + (t - right) * tail_var_mult) * lv[right], lv[t])
    nb = np.array([nb_regularized(bm[t], bv[t], rate) for t in range(101)])
    res.update(loess_mean=lm, loess_var=lv, blur_mean=bm, blur_var=bv, nb_n=nb[:, 0] / ploidy, nb_p=nb[:, 1])
    return res
