"""Developer measurement: lcty_bg_estimate at the full size of `locityper preproc` — the default 4.5 Mb background region
(preproc.rs:599-603) at 30x 150 bp paired-end Illumina (~450 k pairs) and 30x 10 kb ONT (~13.5 k reads) — synthetic, from tests/bg_synth.
   python3 scripts/bg_probe.py --make DIR     write the two samples (BAM, padded sequence, k-mer counts) under DIR (CPU only)
   python3 scripts/bg_probe.py DIR            measure: one JSON line with the host BAM decode, the device time of each kernel (events
                                              around synchronised work), the host fits and the whole call, per sample"""
import json
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

REGION = 4_500_000


def make(d):
    from tests import bg_synth
    os.makedirs(d, exist_ok=True)
    for name, s in (("illumina", bg_synth.Sample(seed=21, region_len=REGION)),
                    ("ont", bg_synth.ont_sample(seed=22, region_len=REGION))):
        s.write(os.path.join(d, name + ".bam"))
        meta = dict(contig=s.contig, start=s.start, end=s.end, padded_start=s.padded_start, k=s.k, seq=s.padded_seq)
        with open(os.path.join(d, name + ".pkl"), "wb") as f:
            pickle.dump(meta, f)
        s.kmer_counts.tofile(os.path.join(d, name + ".u16"))


def measure(d):
    from locityper_amd import api, cdefs
    ctx = api.Context(0)
    out = {"region_bp": REGION}
    for name, tech in (("illumina", cdefs.TECH_ILLUMINA), ("ont", cdefs.TECH_NANOPORE)):
        with open(os.path.join(d, name + ".pkl"), "rb") as f:
            m = pickle.load(f)
        counts = np.fromfile(os.path.join(d, name + ".u16"), dtype=np.uint16)
        prm = api.bg_params(tech)
        t0 = time.perf_counter()
        reads = api.read_bg_bam(os.path.join(d, name + ".bam"), m["contig"], m["start"], m["end"], m["padded_start"], len(m["seq"]), prm)
        t_read = (time.perf_counter() - t0) * 1e3
        res = None
        for _ in range(2):                                   # the first call pays for module load and allocation
            t0 = time.perf_counter()
            bg, rl, dg = api.estimate_bg(ctx, reads, m["seq"], m["padded_start"], counts, m["k"], m["start"], m["end"], prm)
            res = (time.perf_counter() - t0) * 1e3, dg
        wall, dg = res
        out[name] = dict(records=reads.n_records, pairs=int(dg["n_stage"][1]), windows=int(len(dg["win_start"])),
                         bam_decode_ms=round(t_read, 1), kernel_ms=dict(zip(("windows", "counts", "pairs", "depth"),
                                                                            [round(float(x), 3) for x in dg["kernel_ms"]])),
                         fit_ms=round(float(dg["fit_ms"]), 1), call_ms=round(float(dg["total_ms"]), 1), call_wall_ms=round(wall, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--make":
        make(sys.argv[2])
    elif len(sys.argv) == 2:
        measure(sys.argv[1])
    else:
        sys.exit(__doc__)
