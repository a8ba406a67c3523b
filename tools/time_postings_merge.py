"""Times mrg_vocab_postings_merge against a device-to-device copy of the same postings and against rebuilding
the index from the CSR, and the search over the merged index against the sharded search, in one process and
context.

Input, device-resident: the index of tools/time_search_shards.py (time_terms.prepare, the CSR of
mrg_vocab_term_counts): the ids of 1 GiB of Zipf(1.1) text under a vocabulary of 65536 words, documents of 256
ids.  The CSR is indexed once in one piece and once per shard, S = 2, 4, 8 equal row ranges through
mrg_vocab_postings with doc_base.  Every path is run once as a warm-up and then --reps times, the paths alternating
inside a repetition: the merge of 2, 4 and 8 shards, the copy (the one-piece d_docs and d_tf, 8 bytes per posting,
with torch's copy_), the rebuild (mrg_vocab_postings over the whole CSR).  The figures are medians of a host clock
around calls that end in a stream synchronise, and of the HIP-event phases of mrg_postings_merge_info and
mrg_postings_info.  After every merge the three outputs are compared with the one-piece index on the device (a
check of the run, not a timing).

Then the searches: tools/time_search_shards.py's run_case with the merged index of 8 shards in the place of the
one-piece index, for its hot / middle / tail queries at k = 10: mrg_vocab_search over the merged index beside the
three-call path over 2, 4 and 8 shards, rows compared byte for byte.  There is no pass/fail threshold on the times.

    python tools/time_postings_merge.py [--gib 1.0] [--reps 9] [--search-reps 5] [--words 65536]
                                        [--out profiles/postings_merge_timing.json]
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
from time_search import SETS  # noqa: E402
from time_search_shards import SHARDS, run_case  # noqa: E402
from time_terms import layout, prepare  # noqa: E402

MERGE_PHASES = ("ms_sum", "ms_place", "ms_copy")
POST_PHASES = ("ms_count", "ms_scan", "ms_pack", "ms_sort", "ms_unpack")


def med(xs):
    return round(statistics.median(xs), 3)


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--search-reps", type=int, default=5)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postings_merge_timing.json"))
    a = ap.parse_args()
    total = int(a.gib * (1 << 30))
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": M.native.kernel_source_sha()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with M.Context(0) as ctx:
        ctx.set_timing(True)
        v, ids, tok, base = prepare(ctx, total, a.words, a.reduce, 1)
        toff = layout("d256", tok)
        n, n_words, n_docs = tok[-1], v.size()[0], len(toff) - 1
        terms = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
        counts = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
        row_off, _ = ctx.term_counts(v, ids.data_ptr(), toff, terms.data_ptr(), counts.data_ptr(), n)
        doc_len = torch.from_numpy(np.diff(np.asarray(toff, dtype=np.int64)).astype(np.int32)).to("cuda:0")

        def buffers(E):
            return dict(post_off=torch.empty(n_words + 1, dtype=torch.int64, device="cuda:0"),
                        docs=torch.empty(max(E, 1), dtype=torch.int32, device="cuda:0"),
                        tf=torch.empty(max(E, 1), dtype=torch.int32, device="cuda:0"), E=E)

        def index(x, y, into=None):
            E = row_off[y] - row_off[x]
            b = into or buffers(E)
            torch.cuda.synchronize()
            ctx.postings(v, terms.data_ptr(), counts.data_ptr(), row_off[x:y + 1], b["post_off"].data_ptr(), b["docs"].data_ptr(),
                         b["tf"].data_ptr(), E, doc_base=x)
            b.update(a=x, n_docs=y - x)
            return b

        whole = index(0, n_docs)
        E = whole["E"]
        shard_sets = {}
        for S in SHARDS:
            cuts = [n_docs * i // S for i in range(S + 1)]
            shard_sets[S] = [index(x, y) for x, y in zip(cuts[:-1], cuts[1:])]
        merged = {S: buffers(E) for S in SHARDS}
        rebuilt, copied = buffers(E), buffers(E)
        res.update(base)
        res.update({"docs": n_docs, "entries": E, "words": n_words, "shards": list(SHARDS), "reps": a.reps,
                    "posting_bytes": 8 * E})

        def merge(S):
            m = merged[S]
            args = [(s["post_off"].data_ptr(), s["docs"].data_ptr(), s["tf"].data_ptr(), s["E"]) for s in shard_sets[S]]
            ms, got = clock(lambda: ctx.postings_merge(v, args, m["post_off"].data_ptr(), m["docs"].data_ptr(),
                                                       m["tf"].data_ptr(), E))
            assert got == E
            return dict(ms=ms, info=ctx.postings_merge_info())

        def copy():
            def both():
                copied["docs"].copy_(whole["docs"])
                copied["tf"].copy_(whole["tf"])
            return clock(both)[0]

        def rebuild():
            ms, _ = clock(lambda: index(0, n_docs, rebuilt))
            return dict(ms=ms, info=ctx.postings_info())

        runs = {S: [] for S in SHARDS}
        copies, rebuilds = [], []
        same = {}
        for i in range(a.reps + 1):                          # (the first is the warm-up of every path)
            for S in SHARDS:
                for t in merged[S].values():
                    if torch.is_tensor(t):
                        t.zero_()
                r = merge(S)
                same[S] = all(torch.equal(merged[S][key], whole[key]) for key in ("post_off", "docs", "tf"))
                if not same[S]:
                    raise SystemExit("the merge of %d shards differs from the index in one piece" % S)
                if i:
                    runs[S].append(r)
            c, b = copy(), rebuild()
            if i:
                copies.append(c)
                rebuilds.append(b)
        res["copy_ms_wall"] = med(copies)
        res["copy_gb_per_s"] = round(2 * 8 * E / (med(copies) * 1e-3) / 1e9, 1)   # read + written
        # (the rebuild's wall time includes the binding's conversion of n_docs + 1 row offsets: compare the phases)
        res["rebuild"] = {"ms_wall": med([b["ms"] for b in rebuilds]),
                          **{p: med([b["info"][p] for b in rebuilds]) for p in POST_PHASES}}
        res["rebuild"]["ms_phases"] = round(sum(res["rebuild"][p] for p in POST_PHASES), 3)
        res["merge"] = []
        for S in SHARDS:
            rs = runs[S]
            info = rs[-1]["info"]
            wall = med([r["ms"] for r in rs])
            dev = {p: med([r["info"][p] for r in rs]) for p in MERGE_PHASES}
            res["merge"].append({"shards": S, "ms_wall": wall, **dev, "ms_phases": round(sum(dev.values()), 3),
                                 "tiles": info["tiles"], "single_word_tiles": info["single_word_tiles"],
                                 "scratch_bytes": info["scratch_bytes"],
                                 "copy_kernel_gb_per_s": round(2 * 8 * E / (dev["ms_copy"] * 1e-3) / 1e9, 1),
                                 "wall_over_copy": round(wall / res["copy_ms_wall"], 2),
                                 "phases_over_copy": round(sum(dev.values()) / res["copy_ms_wall"], 2),
                                 "wall_over_rebuild_phases": round(wall / res["rebuild"]["ms_phases"], 3),
                                 "phases_over_rebuild_phases": round(sum(dev.values()) / res["rebuild"]["ms_phases"], 3),
                                 "bytes_equal_one_piece": same[S]})
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: res[k] for k in ("entries", "copy_ms_wall", "copy_gb_per_s", "rebuild", "merge")}), flush=True)

        # the searches: the merged index of 8 shards in the place of the one-piece index
        ctx.set_timing(False)
        m8 = dict(merged[max(SHARDS)], n_docs=n_docs, a=0)
        res["search"] = []
        for name, lo, hi in SETS:
            c = run_case(ctx, v, m8, shard_sets, doc_len, n_words, name, lo, min(hi, n_words), a.queries, 10, a.search_reps)
            c["merged_index"] = c.pop("one_piece")
            res["search"].append(c)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            print(json.dumps(c), flush=True)
        v.close()


if __name__ == "__main__":
    main()
