"""Times mrg_vocab_search on the index of tools/time_postings.py's input, in the same run and context as two
yardsticks.

Input, device-resident: the ids of 1 GiB of Zipf(1.1) text under a vocabulary of 65536 words, exactly as
tools/time_terms.py prepares them (its prepare() is used), cut into documents of 256 ids; mrg_vocab_term_counts
and mrg_vocab_postings give the index.  64 queries of 4 positions, drawn (seeded) from three ranges of word ranks:
hot (0-15), middle (1000-2000) and tail (30000-60000); k = 10 and k = 1024.  Per set and k, --reps times after one
warm-up of each, medians:

    search    mrg_vocab_search                                  (HIP events per phase, mrg_search_info)
    floor     a device-to-device copy of 8 bytes per posting visited + a memset of the queries' score rows
    torch     the route a user has without the call: per query, the weights of every position computed in torch
              (gathers, float32 arithmetic), index_add_ into a dense row, torch.topk

The call's top-10 is checked against the torch route's scores by the rules of tests/search_util.py check_topk
(a check of the run, not a timing).  There is no pass/fail threshold on the times.

    python tools/time_search.py [--gib 1.0] [--reps 5] [--words 65536] [--queries 64] [--out profiles/search_timing.json]
"""
import argparse
import json
import math
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
from search_util import check_topk  # noqa: E402
from time_terms import layout, prepare  # noqa: E402

PHASES = ("ms_plan", "ms_accumulate", "ms_select", "ms_order")
SETS = (("hot", 0, 16), ("middle", 1000, 2000), ("tail", 30000, 60000))


def med(xs):
    return round(statistics.median(xs), 3)


def timed(fn, reps):
    """medians of torch-event ms of fn() on torch's stream, after one warm-up; returns (ms, last result)"""
    ms, out = [], None
    for i in range(reps + 1):
        out = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if i:
            ms.append(e0.elapsed_time(e1))
    return med(ms), out


def build_index(ctx, v, ids, tok):
    toff = layout("d256", tok)
    n, n_words, n_docs = tok[-1], v.size()[0], len(toff) - 1
    terms = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    counts = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    row_off, _ = ctx.term_counts(v, ids.data_ptr(), toff, terms.data_ptr(), counts.data_ptr(), n)
    E = row_off[-1]
    post_off = torch.empty(n_words + 1, dtype=torch.int64, device="cuda:0")
    docs = torch.empty(E, dtype=torch.int32, device="cuda:0")
    tf = torch.empty(E, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.postings(v, terms.data_ptr(), counts.data_ptr(), row_off, post_off.data_ptr(), docs.data_ptr(), tf.data_ptr(), E)
    doc_len = torch.from_numpy(np.diff(np.asarray(toff, dtype=np.int64)).astype(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return post_off, docs, tf, E, doc_len, n_docs


def run_set(ctx, v, ix, name, lo, hi, nq, k, reps, k1=1.2, b=0.75):
    post_off, docs, tf, E, doc_len, n_docs = ix
    rng = np.random.default_rng(lo + 1)
    q = rng.integers(lo, hi, (nq, 4)).astype(np.int32)
    q_off = list(range(0, 4 * nq + 1, 4))
    d_q = torch.from_numpy(q.reshape(-1).copy()).to("cuda:0")
    top_docs = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
    top_scores = torch.empty(nq * k, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rows, wall = [], []
    for i in range(reps + 1):                                # (the first is the warm-up)
        t = time.perf_counter()
        top_n = ctx.search(v, post_off.data_ptr(), docs.data_ptr(), tf.data_ptr(), E, doc_len.data_ptr(), n_docs,
                           d_q.data_ptr(), q_off, k, top_docs.data_ptr(), top_scores.data_ptr(), k1=k1, b=b)
        ms = (time.perf_counter() - t) * 1e3
        if i:
            wall.append(ms)
            rows.append(ctx.search_info())
    info = rows[-1]

    # the floor: the postings visited, copied once (8 bytes each), and the rows zeroed
    visited = info["postings"]
    src = torch.empty(2 * visited + 16, dtype=torch.int32, device="cuda:0")
    dst = torch.empty_like(src)
    acc = torch.empty((nq, n_docs), dtype=torch.float32, device="cuda:0")

    def floor():
        dst.copy_(src, non_blocking=True)
        acc.zero_()
    ms_floor, _ = timed(floor, reps)
    del src, dst, acc

    # the torch route
    h_po = post_off.cpu().numpy()
    avgdl = float(np.float32(float(doc_len.sum(dtype=torch.int64)) / n_docs))
    dlf = doc_len.to(torch.float32)
    docs_l = docs.to(torch.int64)

    def torch_route():
        scores = torch.zeros((nq, n_docs), dtype=torch.float32, device="cuda:0")
        for i in range(nq):
            for t in q[i]:
                a, e = int(h_po[t]), int(h_po[t + 1])
                if e == a:
                    continue
                idf = float(np.float32(math.log(1.0 + (n_docs - (e - a) + 0.5) / ((e - a) + 0.5))))
                d, f = docs_l[a:e], tf[a:e].to(torch.float32)
                w = idf * (f * (k1 + 1.0)) / (f + k1 * ((1.0 - b) + b * (dlf[d] / avgdl)))
                scores[i].index_add_(0, d, w)
        return scores, torch.topk(scores, min(k, n_docs), dim=1)
    ms_torch, (scores, _) = timed(torch_route, reps)
    ref = scores.cpu().numpy().astype(np.float64)
    del scores
    k10 = min(k, 10)
    got_d = top_docs.cpu().numpy().view(np.uint32).reshape(nq, k)[:, :k10]
    got_s = top_scores.cpu().numpy().reshape(nq, k)[:, :k10]
    check_topk(got_d, got_s, [min(n, k10) for n in top_n], ref, k10, 0)   # raises when the two routes disagree

    res = {"set": name, "ranks": [lo, hi], "k": k, "queries": nq, "positions": info["positions"], "postings": visited,
           "chunks": info["chunks"], "acc_launches": info["acc_launches"], "scratch_bytes": info["scratch_bytes"],
           "hits_min": int(min((ref > 0).sum(axis=1))), "top10_equals_torch_route": True}
    for p in PHASES:
        res[p] = med([r[p] for r in rows])
    res["ms_search"] = med([sum(r[p] for p in PHASES) for r in rows])
    res["ms_search_wall"] = med(wall)
    res["ms_floor"] = ms_floor
    res["ms_torch_route"] = ms_torch
    res["search_over_floor"] = round(res["ms_search"] / ms_floor, 2)
    res["torch_over_search"] = round(ms_torch / res["ms_search"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_timing.json"))
    a = ap.parse_args()
    total = int(a.gib * (1 << 30))
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": M.native.kernel_source_sha(), "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with M.Context(0) as ctx:
        v, ids, tok, base = prepare(ctx, total, a.words, a.reduce, 1)
        ix = build_index(ctx, v, ids, tok)
        res.update(base)
        res.update({"docs": ix[5], "entries": ix[3]})
        for name, lo, hi in SETS:
            for k in (10, 1024):
                c = run_set(ctx, v, ix, name, lo, min(hi, v.size()[0]), a.queries, k, a.reps)
                res["cases"].append(c)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
                print(json.dumps(c), flush=True)
        v.close()


if __name__ == "__main__":
    main()
