"""Times the sharded search -- mrg_vocab_stats_add once, S x mrg_vocab_search_shard, mrg_search_merge -- against
mrg_vocab_search over the same index in one piece, in the same process and context.

Input, device-resident: the index tools/time_search.py builds (its build_index and time_terms.prepare are used):
the ids of 1 GiB of Zipf(1.1) text under a vocabulary of 65536 words, documents of 256 ids.  The CSR of
mrg_vocab_term_counts is indexed once in one piece and once per shard, S = 2, 4, 8 equal row ranges through
mrg_vocab_postings with doc_base.  64 queries of 4 positions from time_search.py's three ranges of word ranks, k =
10 and k = 1024.  Every path is run once as a warm-up and then --reps times, the one-piece search and the sharded
paths alternating inside a repetition; the figures are medians of a host clock around calls that end in a stream
synchronise (every call of the library returns with its outputs complete), and of the HIP-event phases of
mrg_search_info summed over the shards.

Per case: the one-piece search; per S the statistics, the S searches (wall, and their plan / accumulate / select /
order phases), the merge, the ratio of the whole sharded path to the one-piece search and the merge's share of it.
The merged rows are compared with the one-piece rows byte for byte (a check of the run, not a timing).  There is
no pass/fail threshold on the times.

    python tools/time_search_shards.py [--gib 1.0] [--reps 5] [--words 65536] [--queries 64]
                                       [--out profiles/search_shards_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mapreduce_rust_amd as M  # noqa: E402
from time_search import PHASES, SETS  # noqa: E402
from time_terms import layout, prepare  # noqa: E402

SHARDS = (2, 4, 8)


def med(xs):
    return round(statistics.median(xs), 3)


def build(ctx, v, ids, tok):
    """the CSR of the collection on the device, its index in one piece, and a function that indexes a row range"""
    toff = layout("d256", tok)
    n, n_words, n_docs = tok[-1], v.size()[0], len(toff) - 1
    terms = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    counts = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    row_off, _ = ctx.term_counts(v, ids.data_ptr(), toff, terms.data_ptr(), counts.data_ptr(), n)
    doc_len = torch.from_numpy(np.diff(np.asarray(toff, dtype=np.int64)).astype(np.int32)).to("cuda:0")

    def index(a, e):
        E = row_off[e] - row_off[a]
        post_off = torch.empty(n_words + 1, dtype=torch.int64, device="cuda:0")
        docs = torch.empty(max(E, 1), dtype=torch.int32, device="cuda:0")
        tf = torch.empty(max(E, 1), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.postings(v, terms.data_ptr(), counts.data_ptr(), row_off[a:e + 1], post_off.data_ptr(), docs.data_ptr(),
                     tf.data_ptr(), E, doc_base=a)
        return dict(post_off=post_off, docs=docs, tf=tf, E=E, a=a, n_docs=e - a)
    return index, doc_len, n_docs, n_words


def run_case(ctx, v, whole, shard_sets, doc_len, n_words, name, lo, hi, nq, k, reps, k1=1.2, b=0.75):
    rng = np.random.default_rng(lo + 1)                      # the queries of tools/time_search.py
    q = rng.integers(lo, hi, (nq, 4)).astype(np.int32)
    q_off = list(range(0, 4 * nq + 1, 4))
    d_q = torch.from_numpy(q.reshape(-1).copy()).to("cuda:0")
    one_d = torch.zeros(nq * k, dtype=torch.int32, device="cuda:0")
    one_s = torch.zeros(nq * k, dtype=torch.int32, device="cuda:0")
    mer_d, mer_s = torch.zeros_like(one_d), torch.zeros_like(one_s)
    df = torch.zeros(n_words, dtype=torch.int64, device="cuda:0")
    smax = max(SHARDS)
    in_d = torch.zeros(smax * nq * k, dtype=torch.int32, device="cuda:0")
    in_s = torch.zeros_like(in_d)
    torch.cuda.synchronize()
    dl = doc_len.data_ptr()

    def clock(fn):
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    def one_piece():
        ms, top = clock(lambda: ctx.search(v, whole["post_off"].data_ptr(), whole["docs"].data_ptr(), whole["tf"].data_ptr(),
                                           whole["E"], dl, whole["n_docs"], d_q.data_ptr(), q_off, k, one_d.data_ptr(),
                                           one_s.data_ptr(), k1=k1, b=b))
        return dict(ms=ms, top=top, info=ctx.search_info())

    def sharded(shards):
        r = dict(ms_search=0.0, phases={p: 0.0 for p in PHASES})
        df.zero_()
        torch.cuda.synchronize()
        coll = (0, 0)

        def stats():
            c = (0, 0)
            for s in shards:
                c = ctx.stats_add(v, s["post_off"].data_ptr(), dl + 4 * s["a"], s["n_docs"], df.data_ptr(), c)
            return c
        r["ms_stats"], coll = clock(stats)
        top = []
        for i, s in enumerate(shards):
            at = 4 * i * nq * k
            ms, n = clock(lambda: ctx.search_shard(v, s["post_off"].data_ptr(), s["docs"].data_ptr(), s["tf"].data_ptr(), s["E"],
                                                   dl + 4 * s["a"], s["n_docs"], d_q.data_ptr(), q_off, k, in_d.data_ptr() + at,
                                                   in_s.data_ptr() + at, df.data_ptr(), coll, k1=k1, b=b, doc_base=s["a"]))
            top += n
            r["ms_search"] += ms
            info = ctx.search_info()
            for p in PHASES:
                r["phases"][p] += info[p]
        r["ms_merge"], r["top"] = clock(lambda: ctx.search_merge(len(shards), nq, k, in_d.data_ptr(), in_s.data_ptr(), top, k,
                                                                 mer_d.data_ptr(), mer_s.data_ptr()))
        r["ms_total"] = r["ms_stats"] + r["ms_search"] + r["ms_merge"]
        return r

    ones, runs = [], {S: [] for S in SHARDS}
    same = {}
    for i in range(reps + 1):                                # (the first is the warm-up of every path)
        o = one_piece()
        torch.cuda.synchronize()
        want = (one_d.cpu().numpy().tobytes(), one_s.cpu().numpy().tobytes(), o["top"])
        if i:
            ones.append(o)
        for S in SHARDS:
            mer_d.zero_()
            mer_s.zero_()
            torch.cuda.synchronize()
            r = sharded(shard_sets[S])
            torch.cuda.synchronize()
            # (unwritten slots are 0 in both: the outputs were zeroed and top_n is compared)
            same[S] = (mer_d.cpu().numpy().tobytes(), mer_s.cpu().numpy().tobytes(), r["top"]) == want
            if not same[S]:
                raise SystemExit("the merged rows of %d shards differ from the one-piece search (%s, k = %d)" % (S, name, k))
            if i:
                runs[S].append(r)
    info = ones[-1]["info"]
    res = {"set": name, "ranks": [lo, hi], "k": k, "queries": nq, "positions": info["positions"], "postings": info["postings"],
           "one_piece": {"ms_wall": med([o["ms"] for o in ones]), **{p: med([o["info"][p] for o in ones]) for p in PHASES}},
           "sharded": []}
    one_ms = res["one_piece"]["ms_wall"]
    for S in SHARDS:
        rs = runs[S]
        total = med([r["ms_total"] for r in rs])
        entry = {"shards": S, "ms_stats_wall": med([r["ms_stats"] for r in rs]), "ms_search_wall": med([r["ms_search"] for r in rs]),
                 "ms_merge_wall": med([r["ms_merge"] for r in rs]), "ms_total_wall": total,
                 **{p + "_sum": med([r["phases"][p] for r in rs]) for p in PHASES},
                 "total_over_one_piece": round(total / one_ms, 2),
                 "merge_share": round(med([r["ms_merge"] for r in rs]) / total, 3),
                 "merge_over_one_shard_search": round(med([r["ms_merge"] for r in rs]) / (med([r["ms_search"] for r in rs]) / S), 2),
                 "bytes_equal_one_piece": same[S]}
        res["sharded"].append(entry)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_shards_timing.json"))
    a = ap.parse_args()
    total = int(a.gib * (1 << 30))
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": M.native.kernel_source_sha(), "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with M.Context(0) as ctx:
        v, ids, tok, base = prepare(ctx, total, a.words, a.reduce, 1)
        index, doc_len, n_docs, n_words = build(ctx, v, ids, tok)
        whole = index(0, n_docs)
        shard_sets = {}
        for S in SHARDS:
            cuts = [n_docs * i // S for i in range(S + 1)]
            shard_sets[S] = [index(x, y) for x, y in zip(cuts[:-1], cuts[1:])]
        res.update(base)
        res.update({"docs": n_docs, "entries": whole["E"], "shards": list(SHARDS)})
        for name, lo, hi in SETS:
            for k in (10, 1024):
                c = run_case(ctx, v, whole, shard_sets, doc_len, n_words, name, lo, min(hi, n_words), a.queries, k, a.reps)
                res["cases"].append(c)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
                print(json.dumps(c), flush=True)
        v.close()


if __name__ == "__main__":
    main()
