"""Developer measurement: lcty_bgzf_inflate on BAM-like data.
   python3 scripts/bgzf_inflate_probe.py MB [--calls 5]
MB megabytes of synthetic BAM records (100-base reads, names, qualities) are cut into blocks of 0xff00 bytes and deflated at level 6,
as BAM writers do. Measured on the same blocks in one process: zlib in one host thread (Python's zlib, block by block), the library's
pool of at most 16 zlib threads (the same call with every block's gzip FLG byte set to FEXTRA | FCOMMENT and an empty comment, which
sends it down the host route), and the device route with its upload / kernel / download split. The first call of each pays the
allocations; the medians of the calls after it are reported as one JSON line, in inflated GB/s. All three outputs must be equal."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def records(n_bytes, seed=7):
    """BAM records of 100-base reads: about n_bytes of them, distinct everywhere but in their fixed fields"""
    rng = np.random.default_rng(seed)
    per = 36 + 12 + 4 + 50 + 100
    n = n_bytes // per + 1
    rec = np.zeros((n, per), dtype=np.uint8)
    head = np.zeros(n, dtype=[("bs", "<u4"), ("tid", "<i4"), ("pos", "<i4"), ("ln", "u1"), ("mq", "u1"), ("bin", "<u2"), ("nc", "<u2"), ("fl", "<u2"),
                              ("ls", "<u4"), ("mt", "<i4"), ("mp", "<i4"), ("tl", "<i4")])
    head["bs"], head["ln"], head["mq"], head["nc"], head["ls"] = per - 4, 12, 60, 1, 100
    head["pos"] = np.sort(rng.integers(0, 200_000_000, n)); head["mp"] = head["pos"] + rng.integers(150, 350, n)
    head["fl"] = rng.choice([99, 147, 83, 163], n); head["bin"] = 4681 + (head["pos"] >> 14); head["tl"] = 350
    rec[:, :36] = head.view(np.uint8).reshape(n, 36)
    names = np.char.add("r", np.char.zfill(np.arange(n).astype(str), 10))
    rec[:, 36:47] = np.frombuffer("".join(names.tolist()).encode(), dtype=np.uint8).reshape(n, 11)
    rec[:, 48:52] = np.frombuffer(struct.pack("<I", 100 << 4), dtype=np.uint8)
    codes = np.array([1, 2, 4, 8], dtype=np.uint8)[rng.integers(0, 4, (n, 100))]
    rec[:, 52:102] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, 102:] = np.clip(rng.normal(32, 6, (n, 100)), 2, 41).astype(np.uint8)
    return rec.reshape(-1)[:n_bytes].tobytes()


def blocks(data, flg=4):
    out = []
    extra = b"\0" if flg & 16 else b""
    for i in range(0, len(data), 0xff00):
        chunk = data[i:i + 0xff00]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, flg, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25 + len(extra)) + extra + comp +
                   struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", type=int)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from locityper_amd import api, io as lio
    # a unit of 16 MB of records, deflated once and repeated: every block is still inflated on its own
    unit = records(min(a.mb, 16) << 20)
    reps = max(1, a.mb // 16)
    plain, named = blocks(unit), blocks(unit, flg=4 | 16)
    comp = np.frombuffer(b"".join(plain) * reps, dtype=np.uint8)
    comp_host = np.frombuffer(b"".join(named) * reps, dtype=np.uint8)
    n_out = len(unit) * reps
    ctx = api.Context(0)
    out = np.empty(n_out, dtype=np.uint8)
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    dev, host = [], []
    for c in range(a.calls + 1):
        _, st = lio.bgzf_inflate(ctx, comp, out=out)
        if c:
            dev.append(st)
    want = np.frombuffer(unit, dtype=np.uint8)
    equal = all(np.array_equal(out[r * len(unit):(r + 1) * len(unit)], want) for r in range(reps))
    out[:] = 0
    for c in range(a.calls + 1):
        _, st = lio.bgzf_inflate(ctx, comp_host, out=out)
        if c:
            host.append(st)
    equal = equal and all(np.array_equal(out[r * len(unit):(r + 1) * len(unit)], want) for r in range(reps)) and host[0]["ms_kernel"] == 0
    one = []
    for c in range(2):
        t0 = time.perf_counter()
        got = [zlib.decompress(b[18:-8], -15) for b in plain]
        one.append((time.perf_counter() - t0) * 1e3 * reps)
    equal = equal and b"".join(got) == unit
    gbs = lambda ms: round(n_out / ms / 1e6, 3)
    res = dict(mb=a.mb, calls=a.calls, blocks=int(dev[0]["n_blocks"]), bytes_in=int(dev[0]["bytes_in"]), bytes_out=n_out,
               host_threads=min(16, os.cpu_count() or 1), cpu=next((l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "?"),
               ms={"host_one_thread": round(min(one), 3), "host_pool": round(med(host, "ms_total"), 3), "device_total": round(med(dev, "ms_total"), 3),
                   "device_upload": round(med(dev, "ms_upload"), 3), "device_kernel": round(med(dev, "ms_kernel"), 3), "device_download": round(med(dev, "ms_download"), 3)},
               gb_per_s={"host_one_thread": gbs(min(one)), "host_pool": gbs(med(host, "ms_total")), "device_total": gbs(med(dev, "ms_total")),
                         "device_kernel": gbs(med(dev, "ms_kernel"))},
               outputs_equal=bool(equal))
    print(json.dumps(res))
    if not equal:
        raise SystemExit("the outputs differ")


if __name__ == "__main__":
    main()
