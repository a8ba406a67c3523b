"""Inputs of the indexer tests (tests/test_indexer_cpu.py, tests/test_gpu_indexer.py): deterministic builders
with fixed seeds, standard library only.  Each returns (docs, names): docs[i] are the bytes of the document with
global id i and names[i] its name (str).  Every input stays below 2 MB.

What each builder is for is said at the builder; what the tests lean on in the library is said in DESIGN.md
("What the indexer tests cover")."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_sort.hip: an MSD bucket above MSD_LCAP records is sorted by the LSD radix sort on its own segment; more than
# MSD_MAX_BIG such buckets send the whole array through the LSD sort.  oversized() is built on these two values;
# sort_constants() reads them back from the source so that a change there is noticed (test_indexer_cpu.py).
MSD_LCAP = 2048
MSD_MAX_BIG = 16
# k_fix_runs regroups a run of equal (partition, 16-byte prefix) in ONE thread with an insertion sort: quadratic in
# the run length.  long_runs() keeps every run below this many records (DESIGN.md states the limit).
MAX_PREFIX_RUN = 200

RANKS_N = (1, 2, 255, 256, 257, 65536, 65537)
OVERSIZED_K = (1, 16, 17)


def sort_constants():
    """(MSD_LCAP, MSD_MAX_BIG) as k_sort.hip states them"""
    src = open(os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "k_sort.hip")).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))
                 for name in ("MSD_LCAP", "MSD_MAX_BIG"))


def perm_names(n, seed):
    """n distinct names in a fixed shuffled order, so that the rank of a name among the sorted names differs from
    its position (the document id) nearly everywhere; lengths 0 .. 40 bytes, exactly one empty name"""
    names = [""]
    for j in range(1, n):
        s = format(j, "x")                       # distinct: the hex digits end at the first '_' or at the end
        names.append(s + "_" * (max(len(s), (j * 7) % 41) - len(s)))
    random.Random(seed).shuffle(names)
    assert len(set(names)) == n and max(map(len, names)) <= 40
    return names


# ---------------------------------------------------------------- group sizes

DIGITS_N = (1, 2, 9, 10, 11, 99, 100, 101, 999, 1000, 1001)
DIGITS_DOCS = 1001


def digits_members():
    """{N: the sorted ids of the documents that hold the word gN}: exactly N of the 1001, drawn over the whole id
    range (a fixed sample, never the first N)"""
    rng = random.Random(1001)
    out = {}
    for n in DIGITS_N:
        ids = sorted(rng.sample(range(DIGITS_DOCS), n))
        assert n == DIGITS_DOCS or ids != list(range(n))
        out[n] = ids
    return out


def digit_name(d):
    return f"n{d * 37 % DIGITS_DOCS}.t"        # 37 and 1001 are coprime: distinct, 4 .. 7 bytes, rank != id


def digits():
    """group sizes of 1 .. 4 digits: gN occurs in exactly N documents; fillers f*, x* (x4 is the bytewise largest
    word and occurs in 200 documents: the last group of partition 0 at R = 1 is a many-document group)"""
    mem = digits_members()
    words = [[] for _ in range(DIGITS_DOCS)]
    for n, ids in mem.items():
        for d in ids:
            words[d].append(f"g{n}")
    docs = [" ".join([f"f{d % 37}"] + w + [f"x{d % 5}", f"f{d % 11}"]).encode() for d, w in enumerate(words)]
    return docs, [digit_name(d) for d in range(DIGITS_DOCS)]


# ---------------------------------------------------------------- document ranks

def ranks(n):
    """n documents: `the` in all of them, w{d % 50}, and q{d % 7} in every fourth; names permuted.  A word's
    documents are ordered by rank alone, so the second and third rank bytes decide from 257 and 65537 on"""
    docs = [(f"the w{d % 50}" + (f" q{d % 7}" if d % 4 == 0 else "")).encode() for d in range(n)]
    return docs, perm_names(n, 4242 + n)


# ---------------------------------------------------------------- bytewise name order

NAME_ORDER_NAMES = [
    "a.txt", "z", "a", "中", "a/", "0123456789abcdefY", "a-1", "é", "dup", "~",
    "0123456789abcdef0123456789abcdefQ", "", "0123456789abcdefX", "B", "dup", "0123456789abcdef0123456789abcdefP",
    "0123456789abcdef", "b", "_", "10", "9", "1", "zé", "\U00010400", "\ufffd", "Z", "a.txt.gz", "a0",
    "éa", "è", "中文", "~~", "zz", "0123456789abcdef0123456789abcdef", "A", "aa", "a-", "-",
    ".", "/",
]


def name_order():
    """40 documents whose names are prefixes of one another, differ only after 16 and after 32 bytes, hold bytes
    >= 0x80 next to '~' and 'z' (a signed-char comparison would put them first) and an astral codepoint next
    to U+FFFD (a UTF-16 comparison would swap them); two documents share a name and one has the empty name"""
    names = list(NAME_ORDER_NAMES)
    assert len(names) == 40 and names.count("dup") == 2 and names.count("") == 1
    docs = [(f"every w{d % 3} v{d % 7} " + ("half " if d % 2 else "") + f"own{d}").encode() for d in range(40)]
    return docs, names


# ---------------------------------------------------------------- natural oversized sort buckets

OVERSIZED_DOCS = MSD_LCAP + 1


def oversized(k):
    """2049 documents, each with the same k words and one word of its own; names permuted (two rank bytes).

    This follows from MSD_LCAP = 2048 and MSD_MAX_BIG = 16 of k_sort.hip: at R = 1 the MSD bucket of a record is
    the first three key bytes (7 bits each, the third without its lowest bit) and holds no document bits, so
    each shared word is one bucket of 2049 > MSD_LCAP records.  k = 1 and k = 16 are at most MSD_MAX_BIG such
    buckets (each sorted by the LSD radix sort on its segment), k = 17 is more (the whole array through the LSD
    sort) -- with no test knob.  The shared words differ in their first byte, a capital; the own words start with
    two small letters spread over 676 prefixes, a few records per bucket, and sort behind every shared word: the
    group a partition drops as its last is then a one-document group wherever it can be (at R = 1 always), and the
    order inside every 2049-document group is checked."""
    assert 1 <= k <= 26
    shared = " ".join(chr(65 + j) + "SH" + "X" * (j % 5) for j in range(k))
    docs = [f"{shared} {chr(97 + d % 26)}{chr(97 + d // 26 % 26)}{d}".encode() for d in range(OVERSIZED_DOCS)]
    return docs, perm_names(OVERSIZED_DOCS, 977 + k)


def msd_bucket_r1(key):
    """the MSD bucket of a key at R = 1 (k_sort.hip msd_bucket with pbits = 0), restated"""
    b = list(key[:3]) + [0, 0, 0]
    b0 = min(b[0], 127)
    b1 = 127 if b0 == 127 else min(b[1], 127)
    b2 = 127 if b1 == 127 else min(b[2], 127)
    return ((b0 << 14) | (b1 << 7) | b2) >> 1


# ---------------------------------------------------------------- long keys across documents

K16 = "sixteen_byte_key_"[:16]
LONG_RUN_KEYS = {                                # key -> the documents (of 40) that hold it
    K16: lambda d: True,                         # the short key, exactly 16 bytes, in all 40
    K16 + "a": lambda d: d % 2 == 0,             # 17 bytes, a prefix of the next
    K16 + "ab": lambda d: d % 3 == 0,            # 18 bytes
    K16 + "c" + "d" * 13: lambda d: d == 17,     # 30 bytes, one document
    "é" * 8: lambda d: d % 7 == 0,          # 16 bytes of 2-byte letters (short)
    "é" * 9: lambda d: d % 5 < 2,           # 18 bytes of 2-byte letters (long), same 16-byte prefix
}


def long_runs():
    """40 documents; long keys that extend one 16-byte short key, each in another subset of the documents, so
    that a run of equal 16-byte prefixes holds (key, document) pairs of several keys ordered by rank, which
    k_fix_runs must regroup by key.  The longest run is 40 + 20 + 14 + 1 = 75 records < MAX_PREFIX_RUN."""
    docs = []
    for d in range(40):
        ws = [k for k, f in LONG_RUN_KEYS.items() if f(d)]
        random.Random(d).shuffle(ws)
        docs.append((f"fill{d % 4} " + " ".join(ws) + " \u017flast").encode())   # (the bytewise largest word: dropped)
    assert len(K16) == 16
    run = sum(1 for d in range(40) for k, f in LONG_RUN_KEYS.items() if k.startswith(K16) and f(d))
    assert run == 75 and run < MAX_PREFIX_RUN
    return docs, perm_names(40, 31)


# ---------------------------------------------------------------- many (word, document) pairs

def pairs(n_docs):
    """n_docs documents of 200 distinct words each from a vocabulary of 2000 (60 of 13 .. 16 bytes, 20 longer
    than 16): 200 * n_docs distinct (word, document) pairs, enough to leave the per-bucket LDS tables of the
    aggregation once the internal hashes are truncated"""
    rng = random.Random(300)
    vocab = set()

    def fresh(lo, hi, count):
        out = []
        while len(out) < count:
            w = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(lo, hi)))
            if w not in vocab:
                vocab.add(w)
                out.append(w)
        return out
    words = fresh(3, 12, 1920) + fresh(13, 16, 60) + fresh(17, 30, 20)
    docs = [" ".join(rng.sample(words, 200)).encode() for _ in range(n_docs)]
    return docs, perm_names(n_docs, 300 + n_docs)

