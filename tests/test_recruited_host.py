"""The host's half of a resident set of recruited reads (lcty_recruited), no device: the selection and rebasing rule of
tests/pyref_recruited.py on a hand-written case, the new entries against the header, and the bookkeeping of
locityper_amd/csrc/lcty_recruited_host.hpp (plan, byte cap, growth, names) as a stand-alone program under the address and
undefined-behaviour sanitizers (scripts/recruited_probe_host.cpp) held to the same restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from locityper_amd import _lib, cdefs
from tests import pyref_recruited as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["lcty_recruited_create", "lcty_recruited_destroy", "lcty_recruited_add", "lcty_recruited_add_fastx", "lcty_recruited_add_sample",
           "lcty_recruited_sizes", "lcty_recruited_view", "lcty_recruited_names", "lcty_reads_map_append_recruited"]


def test_pyref_on_five_pairs_and_three_loci():
    pairs = [("ACGT", "TTTT"), ("N" + "A" * 32, None), ("C" * 32, "G"), ("G" * 16, "ACGTN"), ("T", "AA")]
    view = PR.pack_reads(pairs)
    # the source, by hand: a mate owns ceil(len / 32) units of two words of bases and one of mask
    assert view[0].tolist() == [4, 4, 33, 0, 32, 1, 16, 5, 1, 2]
    assert view[1].tolist() == [0, 32, 64, 128, 128, 160, 192, 224, 256, 288, 320]
    assert view[2].tolist() == [0xE4, 0, 0xFF, 0, 0, 0, 0, 0, 0x55555555, 0x55555555, 2, 0, 0xAAAAAAAA, 0, 0xE4, 0, 3, 0, 0, 0]
    assert view[3].tolist() == [0, 0, 1, 0, 0, 0, 0, 16, 0, 0]
    cnt = np.array([2, 1, 0, 3, 1], dtype=np.uint32)
    loci = np.array([[0, 2, 9], [1, 9, 9], [9, 9, 9], [0, 1, 2], [2, 9, 9]], dtype=np.uint32)      # 9: never read
    E = PR.Expected(3)
    E.add(view, cnt, loci)
    l0, l1, l2 = (E.locus(l) for l in range(3))
    assert l0[0].tolist() == [4, 4, 16, 5] and l0[1].tolist() == [0, 32, 64, 96, 128]
    assert l0[2].tolist() == [0xE4, 0, 0xFF, 0, 0xAAAAAAAA, 0, 0xE4, 0] and l0[3].tolist() == [0, 0, 0, 16] and l0[4].tolist() == [0, 3]
    assert l1[0].tolist() == [33, 0, 16, 5] and l1[1].tolist() == [0, 64, 64, 96, 128]                    # the absent mate takes no unit
    assert l1[2].tolist() == [0, 0, 0, 0, 0xAAAAAAAA, 0, 0xE4, 0] and l1[3].tolist() == [1, 0, 0, 16] and l1[4].tolist() == [1, 3]
    assert l2[0].tolist() == [4, 4, 16, 5, 1, 2] and l2[1].tolist() == [0, 32, 64, 96, 128, 160, 192]
    assert l2[2].tolist() == [0xE4, 0, 0xFF, 0, 0xAAAAAAAA, 0, 0xE4, 0, 3, 0, 0, 0] and l2[3].tolist() == [0, 0, 0, 16, 0, 0] and l2[4].tolist() == [0, 3, 4]
    assert E.bytes() == 12 * (4 + 4 + 6) + 32 * (2 + 2 + 3)
    # a second chunk: its pairs go behind the first one's, the ordinals run on from 5 whether a pair was recruited or not
    E.add(PR.pack_reads([("C", None), ("GG", "T")]), [0, 1], [[9], [1]])
    l1 = E.locus(1)
    assert l1[0].tolist() == [33, 0, 16, 5, 2, 1] and l1[1].tolist() == [0, 64, 64, 96, 128, 160, 192]
    assert l1[2].tolist() == [0, 0, 0, 0, 0xAAAAAAAA, 0, 0xE4, 0, 10, 0, 3, 0] and l1[4].tolist() == [1, 3, 6]
    assert E.locus(0)[4].tolist() == [0, 3] and E.n_seen == 7


def test_entries_are_declared_bound_and_refuse_null_arguments():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locityper_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in the header"
        assert hasattr(L, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in m.group(1).split(",") if a.strip()]), name
    bad = cdefs.ERR_INVALID_INPUT
    assert L.lcty_recruited_create(None, 0, None) == bad
    out = _lib.VP()
    assert L.lcty_recruited_create(None, 1, out) == bad and not out.value
    cnt = np.zeros(1, dtype=np.uint32)
    assert L.lcty_recruited_add(None, None, 1, 1, cnt.ctypes.data, cnt.ctypes.data) == bad
    assert L.lcty_recruited_add_fastx(None, None, 1, cnt.ctypes.data, cnt.ctypes.data) == bad
    assert L.lcty_recruited_add_sample(None, None, 1, cnt.ctypes.data, cnt.ctypes.data) == bad
    assert L.lcty_recruited_sizes(None, 0, None, None) == bad
    assert L.lcty_recruited_view(None, 0, None, None) == bad
    assert L.lcty_recruited_names(None, 0, None, None) == bad
    p = cdefs.MapParams()
    assert L.lcty_reads_map_append_recruited(None, None, 0, 0, 0, C.byref(p)) == bad
    L.lcty_recruited_destroy(None)                                           # like free(NULL)


def test_knobs_are_in_the_list_and_in_the_header():
    """tests/test_host_api.py's rule for a knob: in the list lcty_ctx_set_knob accepts, with its words in the header's knob paragraph,
    and what the set asks its context for; the defaults are the header's"""
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    api_src, header = read("locityper_amd", "csrc", "lcty_api.hip"), read("include", "locityper_hip.h")
    src, host = read("locityper_amd", "csrc", "lcty_recruited.hip"), read("locityper_amd", "csrc", "lcty_recruited_host.hpp")
    known = api_src[api_src.index("known[] = {"):api_src.index("nullptr};")]
    paragraph = header[:header.index("int32_t lcty_ctx_set_knob(")]
    asked = set(re.findall(r'knob\("(recruited_[a-z_]+)"', src))
    assert asked == {"recruited_init_units", "recruited_max_bytes"}
    for name in asked:
        assert f'"{name}"' in known and f'"{name}"   ' in paragraph, name
    assert "INIT_UNITS_DEFAULT = 4096" in host and "default 4 096" in paragraph
    assert "MAX_BYTES_DEFAULT = 1ull << 36" in host and "default 2^36" in paragraph
    assert (cdefs.RECRUITED_UNIT_BYTES, cdefs.RECRUITED_PAIR_BYTES) == (PR.UNIT_BYTES, PR.PAIR_BYTES) == (12, 32)
    assert "UNIT_BYTES = 8 + 4, PAIR_BYTES = 2 * 4 + 2 * 8 + 8" in host


# ---------------------------------------------------------------- the bookkeeping under the sanitizers
def _grown(cap, need, init):
    if need <= cap:
        return cap
    c = cap if cap else max(init, 1)
    while c < need:
        c *= 2
    return c


def _corpus():
    """sets of adds: (name, n_loci, keep_names, init_units, max_bytes, [(max_out, named, [(len1, len2, [loci], name)], status)])"""
    rng = np.random.default_rng(17)
    lens = [0, 1, 31, 32, 33, 64, 150, 255, 256, 257, 5000]
    def chunk(n, n_loci, max_out, tag):
        rows = []
        for i in range(n):
            k = int(rng.integers(0, max_out + 1))
            rows.append((int(rng.choice(lens)), int(rng.choice(lens)), sorted(rng.choice(n_loci, size=min(k, n_loci), replace=False).tolist()), f"{tag}r{i}"))
        return rows
    sets = []
    sets.append(("grow", 4, 1, 1, 1 << 40, [(3, 1, chunk(40, 4, 3, "a"), 0), (3, 1, [(5, 5, [], "none")] * 3, 0), (3, 1, chunk(300, 4, 3, "c"), 0)]))
    sets.append(("default", 3, 1, 4096, 1 << 36, [(2, 1, chunk(500, 3, 2, "a"), 0), (8, 1, chunk(100, 3, 3, "b"), 0)]))
    sets.append(("unnamed", 2, 1, 7, 1 << 40, [(2, 1, chunk(10, 2, 2, "a"), 0), (2, 0, chunk(10, 2, 2, "b"), 0)]))
    sets.append(("no-names", 2, 0, 64, 1 << 40, [(2, 1, chunk(50, 2, 2, "a"), 0)]))
    # refused adds between accepted ones: the set stays what it was
    ok = chunk(30, 3, 3, "a")
    too_many = [(10, 10, [0, 1, 2], "x")]                                     # three loci with max_out 2
    beyond = [(10, 10, [3], "x")]                                             # locus 3 of 3
    sets.append(("refused", 3, 1, 2, 1 << 40, [(3, 1, ok, 0), (2, 1, too_many, cdefs.ERR_INVALID_INPUT), (3, 1, beyond, cdefs.ERR_INVALID_INPUT),
                                                (3, 1, chunk(30, 3, 3, "b"), 0)]))
    # the byte cap: one byte under the need is refused, the need itself fits
    first, second = chunk(20, 2, 2, "a"), chunk(20, 2, 2, "b")
    def need(rows):
        return sum(len(r[2]) * (PR.UNIT_BYTES * (PR.units_of(r[0]) + PR.units_of(r[1])) + PR.PAIR_BYTES) for r in rows)
    total = need(first) + need(second)
    sets.append(("cap-under", 2, 1, 16, total - 1, [(2, 1, first, 0), (2, 1, second, cdefs.ERR_UNSUPPORTED), (2, 1, [(1, 0, [], "z")], 0)]))
    sets.append(("cap-exact", 2, 1, 16, total, [(2, 1, first, 0), (2, 1, second, 0)]))
    return sets


def test_bookkeeping_is_clean_under_the_sanitizers_and_equals_the_restatement(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    exe = str(tmp_path / "recruited_probe_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "locityper_amd", "csrc"), os.path.join(ROOT, "scripts", "recruited_probe_host.cpp"), "-o", exe], check=True)
    sets = _corpus()
    want = []
    with open(tmp_path / "corpus.txt", "w") as f:
        for name, n_loci, keep, init, max_bytes, adds in sets:
            f.write(f"set {name} {n_loci} {keep} {init} {max_bytes}\n")
            books = [dict(pairs=0, units=0, cap_units=0, cap_pairs=0, names=[]) for _ in range(n_loci)]
            named_all = True
            for k, (max_out, named, rows, status) in enumerate(adds):
                f.write(f"add {len(rows)} {max_out} {named}\n")
                for l1, l2, loci, nm in rows:
                    f.write(f"{l1} {l2} {len(loci)} {' '.join(map(str, loci))} {nm}\n")
                want.append(f"{name} add {k} status {status}")
                if status:
                    continue
                gain = [[0, 0] for _ in range(n_loci)]
                for l1, l2, loci, nm in rows:
                    for l in loci:
                        gain[l][0] += 1; gain[l][1] += PR.units_of(l1) + PR.units_of(l2)
                        if keep and named:
                            books[l]["names"].append(nm)
                for l, (gp, gu) in enumerate(gain):
                    b = books[l]
                    if gp:
                        b["cap_units"] = _grown(b["cap_units"], b["units"] + gu, init)
                        b["cap_pairs"] = _grown(b["cap_pairs"], b["pairs"] + gp, max(init // 8, 1))
                    b["pairs"] += gp; b["units"] += gu
            f.write("end\n")
            for l, b in enumerate(books):
                want.append(f"{name} locus {l} {b['pairs']} {b['units']} {32 * b['units']} {b['cap_units']} {b['cap_pairs']} {','.join(b['names'])}")
    r = subprocess.run([exe, str(tmp_path / "corpus.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.strip().splitlines()
    assert got[-1] == f"recruited_probe_host: {len(sets)} sets"
    assert got[:-1] == want
    assert any(g.endswith(f" status {cdefs.ERR_UNSUPPORTED}") for g in got) and sum("grow locus" in g for g in got) == 4
