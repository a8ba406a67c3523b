"""CPU tests of the top-k surface: the host merge of per-GPU top-k runs (mrg_run.cpp merge_top_lines,
the multi-GPU half of top.txt) against a Python sort, and the MRG_FLAG_TOP flag / symbol plumbing.
Expected values never come from the library."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def top_of(lines, k):
    """First k of `lines` (b"key count", no newline) by (count descending, key bytes ascending)."""
    def order(ln):
        key, c = ln.rsplit(b" ", 1)
        return (-int(c), key)
    return sorted(lines, key=order)[:k]


def test_merge_top_lines_host():
    from mapreduce_rust_amd import native
    rng = random.Random(11)
    # keys that are prefixes of each other, and bytes >= 0x80 (they sort after every ASCII byte)
    alpha = [b"a", b"b", b"ab", b"abc", b"z", b"\xc3\xa9", b"\xc5\xbf", b"_", b"0", b"\xf0\x9f\x98\x80"]
    for trial in range(200):
        n_lines = rng.randint(0, 40)
        # few distinct counts (ties across runs), of 1..20 digits, no leading zero
        counts = [str(rng.randint(1, 9)) + "".join(rng.choice("0123456789") for _ in range(rng.randint(0, 19)))
                  for _ in range(rng.randint(1, 4))]
        lines = set()
        for _ in range(n_lines):
            key = b"".join(rng.choice(alpha) for _ in range(rng.randint(1, 4)))
            lines.add(key + b" " + rng.choice(counts).encode())
        lines = sorted(lines)
        n_runs = rng.randint(1, 9)
        runs = [[] for _ in range(n_runs)]
        for ln in lines:
            runs[rng.randrange(n_runs)].append(ln)
        blobs = []
        for r in runs:
            b = b"".join(x + b"\n" for x in top_of(r, len(r)))
            if b and rng.random() < 0.3:
                b = b[:-1]  # no final newline
            blobs.append(b)
        for k in {0, 1, rng.randint(0, len(lines) + 1), len(lines), len(lines) + 5, 10**9}:
            got = native.merge_top_lines(blobs, k)
            assert got == b"".join(x + b"\n" for x in top_of(lines, k)), (trial, k)
    assert native.merge_top_lines([], 5) == b"" and native.merge_top_lines([b"", b""], 5) == b""
    assert native.merge_top_lines([b"b 2\nab 1", b"a 10\nab 2\n", b""], 3) == b"a 10\nab 2\nb 2\n"
    # 20-digit counts beyond 2^64 still order as numbers
    assert native.merge_top_lines([b"x 99999999999999999999\n", b"y 100000000000000000000\n"], 2) == \
        b"y 100000000000000000000\nx 99999999999999999999\n"


def test_flag_top_and_symbols():
    from mapreduce_rust_amd import native
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    m = re.search(r"^#define MRG_FLAG_TOP\(k\) \(\(\(uint32_t\)\(k\) & (0x[0-9A-Fa-f]+)u\) << (\d+)\)", hdr, re.M)
    assert m, "include/mrgpu.h lacks #define MRG_FLAG_TOP(k)"
    mask, shift = int(m.group(1), 16), int(m.group(2))
    assert (mask, shift) == (0xFFFF, 16)
    for k in (0, 1, 65535):
        assert native.flag_top(k) == (k & mask) << shift
    assert native.flag_top(1) == 0x10000 and native.flag_top(65535) == 0xFFFF0000
    syms = native.exported_symbols()
    assert "mrg_job_topk" in syms and "mrg_job_copy_topk" in syms
