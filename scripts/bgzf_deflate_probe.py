"""Developer measurement: lcty_bgzf_deflate on BAM-like data.
   python3 scripts/bgzf_deflate_probe.py MB [--calls 5] [--out profiles/bgzf_deflate_probe.json]
MB megabytes of the synthetic BAM records of scripts/bgzf_inflate_probe.py (a unit of at most 16 MB, repeated) are deflated in blocks of
0xff00 bytes, in one process: by zlib in one host thread at levels 1 and 6 (Python's zlib, block by block, on the unit, times the
repeats), by the library's host route (lcty_io_write_bgzf to a file in memory: zlib level 6 in one thread; above 64 MB on the unit,
times the repeats: the route is one serial loop over blocks) and by the device with its upload / kernel / download split. The first
call of the device pays the allocations; the medians of the calls after it are reported, in input GB/s, with the output sizes, as one
JSON line on stdout and appended to --out. The device's output must inflate to the input (lcty_bgzf_inflate)."""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from bgzf_inflate_probe import records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", type=int)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bgzf_deflate_probe.json"))
    a = ap.parse_args()
    from locityper_amd import api, io as lio
    unit = records(min(a.mb, 16) << 20)
    reps = max(1, a.mb // 16)
    data = np.tile(np.frombuffer(unit, dtype=np.uint8), reps)
    n_in = len(data)
    ms, size = {}, {}
    for level in (1, 6):
        t0 = time.perf_counter()
        n = 0
        for i in range(0, len(unit), 0xff00):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            n += len(c.compress(unit[i:i + 0xff00]) + c.flush()) + 26
        ms[f"zlib_level_{level}_one_thread"] = (time.perf_counter() - t0) * 1e3 * reps
        size[f"zlib_level_{level}_one_thread"] = n * reps + 28
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=shm) as tmp:
        path = os.path.join(tmp, "probe.gz")
        whole = a.mb <= 64
        rows = []
        for c in range(2 if whole else 1):
            t0 = time.perf_counter()
            lio.write_bgzf(path, data if whole else unit)
            rows.append((time.perf_counter() - t0) * 1e3 * (1 if whole else reps))
        ms["library_host_route"] = min(rows)
        size["library_host_route"] = os.path.getsize(path) if whole else (os.path.getsize(path) - 28) * reps + 28
    ctx = api.Context(0)
    dev = []
    for c in range(a.calls + 1):
        out, off, st = lio.bgzf_deflate(ctx, data)
        if c:
            dev.append(st)
    back, _ = lio.bgzf_inflate(ctx, out)
    equal = bool(np.array_equal(back, data))
    med = lambda k: float(np.median([r[k] for r in dev]))
    for k in ("total", "upload", "kernel", "download"):
        ms[f"device_{k}"] = med(f"ms_{k}")
    size["device"] = int(dev[0]["bytes_out"])
    res = dict(mb=a.mb, calls=a.calls, blocks=int(dev[0]["n_blocks"]), bytes_in=n_in,
               forms={k: int(dev[0][f"n_{k}"]) for k in ("stored", "fixed", "dynamic")},
               host_route_measured_on_mb=a.mb if whole else len(unit) >> 20,
               cpu=next((l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "?"),
               bytes_out=size, ms={k: round(v, 3) for k, v in ms.items()}, gb_per_s={k: round(n_in / v / 1e6, 3) for k, v in ms.items()},
               device_output_inflates_to_the_input=equal)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    if not equal:
        raise SystemExit("the device's output does not inflate to the input")


if __name__ == "__main__":
    main()
