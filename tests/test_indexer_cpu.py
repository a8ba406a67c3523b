"""CPU tests: the two indexer references agree on the inputs of tests/indexer_util.py.

tests/test_gpu_indexer.py compares the device with oracle_lib.indexer (oracle/oracle.c), which test_oracle.py
checks at six files only.  Here it is compared, at every builder and R = 1, 5 and 64, with twin.indexer_job
(tests/golden/twin.py): a dict of words, sorted(values, key = UTF-8 bytes) and the drop-last reduce loop.  The
group sizes of digits() are checked a third way, from the builder's own bookkeeping."""
import collections

import pytest

import indexer_util as U
import oracle_lib as O

RS = (1, 5, 64)


def agree(docs, names):
    import twin
    texts = [d.decode() for d in docs]
    for R in RS:
        assert O.indexer(docs, names, R) == twin.indexer_job(texts, names, R), R


def test_sort_constants_match_the_source():
    """oversized() is built on MSD_LCAP and MSD_MAX_BIG: a change in k_sort.hip must be noticed here"""
    assert U.sort_constants() == (U.MSD_LCAP, U.MSD_MAX_BIG) == (2048, 16)


def test_builders_are_deterministic_and_small():
    for build in (U.digits, lambda: U.ranks(65537), U.name_order, lambda: U.oversized(17), U.long_runs,
                  lambda: U.pairs(300)):
        a, b = build(), build()
        assert a == b
        assert len(a[0]) == len(a[1])
        assert sum(len(d) for d in a[0]) < 2_000_000


def test_perm_names_shape():
    for n in U.RANKS_N:
        names = U.perm_names(n, 4242 + n)
        assert len(set(names)) == n and names.count("") == 1
        assert {len(s) for s in names} <= set(range(41))
        if n >= 255:
            assert {len(s.encode()) for s in names} == set(range(41))
            order = sorted(range(n), key=lambda i: names[i].encode())
            assert sum(1 for r, i in enumerate(order) if r == i) < n // 50      # rank != id nearly everywhere
    assert all(not set(s) & set(" ,\n") for s in U.NAME_ORDER_NAMES)


def test_digits_group_sizes_from_the_bookkeeping():
    """the lines of gN read "gN N " and then exactly N names: those of the builder's own member lists, sorted
    bytewise"""
    docs, names = U.digits()
    mem = U.digits_members()
    assert sorted(mem) == sorted(U.DIGITS_N) and all(len(ids) == n for n, ids in mem.items())
    (out,) = O.indexer(docs, names, 1)
    lines = {ln.split(b" ", 1)[0]: ln for ln in out.split(b"\n") if ln}
    for n, ids in mem.items():
        ln = lines[b"g%d" % n]
        head = b"g%d %d " % (n, n)
        assert ln.startswith(head), ln[:40]
        got = ln[len(head):].split(b",")
        assert len(got) == n
        assert got == sorted(names[d].encode() for d in ids)
    assert lines[b"g10"].startswith(b"g10 10 ") and lines[b"g1000"].startswith(b"g1000 1000 ")
    # x4 sorts last and is dropped at R = 1; kept, it is a 200-document group at the end of the partition
    assert b"x4" not in lines and b"x3" in lines
    agree(docs, names)


@pytest.mark.parametrize("n", U.RANKS_N)
def test_ranks_references_agree(n):
    docs, names = U.ranks(n)
    assert len(docs) == n
    agree(docs, names)


def test_name_order_references_agree():
    docs, names = U.name_order()
    agree(docs, names)
    # the order the names take is neither the id order nor a signed-char / UTF-16 order
    by_bytes = sorted(names, key=lambda s: s.encode())
    assert by_bytes != names
    assert by_bytes != sorted(names, key=lambda s: [b - 256 if b > 127 else b for b in s.encode()])
    assert by_bytes != sorted(names, key=lambda s: s.encode("utf-16-be"))
    (out,) = O.indexer(docs, names, 1)
    line = [ln for ln in out.split(b"\n") if ln.startswith(b"every 40 ")]
    assert line and line[0] == b"every 40 " + b",".join(s.encode() for s in by_bytes)


@pytest.mark.parametrize("k", U.OVERSIZED_K)
def test_oversized_references_agree_and_buckets(k):
    """k MSD buckets above MSD_LCAP records at R = 1, no other above 64: from the builder's words alone"""
    docs, names = U.oversized(k)
    agree(docs, names)
    per = collections.Counter(U.msd_bucket_r1(w) for d in docs for w in set(d.split()))
    big = [b for b, c in per.items() if c > U.MSD_LCAP]
    assert len(big) == k and all(per[b] == U.OVERSIZED_DOCS for b in big)
    assert max(c for b, c in per.items() if b not in big) <= 64
    assert (k > U.MSD_MAX_BIG) == (k == 17)
    # at R = 1 every 2049-document group is written (the dropped last group is a one-document word), in name order
    (out,) = O.indexer(docs, names, 1)
    big_lines = [ln for ln in out.split(b"\n") if b" %d " % U.OVERSIZED_DOCS in ln[:16]]
    assert len(big_lines) == k
    assert all(ln.split(b" ", 2)[2] == b",".join(sorted(s.encode() for s in names)) for ln in big_lines)


def test_long_runs_references_agree():
    docs, names = U.long_runs()
    agree(docs, names)
    (out,) = O.indexer(docs, names, 1)
    sizes = {ln.split(b" ")[0].decode(): int(ln.split(b" ")[1]) for ln in out.split(b"\n") if ln}
    for key, member in U.LONG_RUN_KEYS.items():
        assert sizes[key] == sum(1 for d in range(40) if member(d)), key
    assert sizes[U.K16] == 40 and sizes[U.K16 + "c" + "d" * 13] == 1


def test_pairs_references_agree():
    docs, names = U.pairs(300)
    assert sum(len(set(d.split())) for d in docs) == 300 * 200
    words = {w for d in docs for w in d.split()}
    assert sum(1 for w in words if 13 <= len(w) <= 16) > 50 and sum(1 for w in words if len(w) > 16) == 20
    agree(docs, names)
