"""Times mrg_vocab_search_bool beside the plain mrg_vocab_search of the same positions, in one run and context
(DESIGN.md section 34).

Input, device-resident: the index of tools/time_search.py (its build_index is used): the ids of 1 GiB of Zipf(1.1)
text under a vocabulary of 65536 words, cut into documents of 256 ids.  64 queries of 4 positions, drawn (seeded)
exactly as tools/time_search.py draws them from three ranges of word ranks: hot (0-15), middle (1000-2000) and tail
(30000-60000); k = 10.  Per set the variants below are alternated, --reps rounds after one warm-up round, medians:

    search        mrg_vocab_search of the ids                         (the yardstick of every other row)
    all_should    mrg_vocab_search_bool, every role SHOULD: the same launches as `search`; the pair shows the spread
                  of the run and that the plain path did not move
    must2         positions 0, 1 MUST, positions 2, 3 SHOULD
    must4         every position MUST
    not1          positions 0 .. 2 SHOULD, position 3 MUST_NOT
    floor         per variant: a device-to-device copy of 8 bytes per scoring posting visited and of 4 bytes per
                  posting that touches the match state (a counted MUST posting: the read-modify-write; a MUST_NOT
                  posting: the document read and the store), + a memset of the score rows and, for a variant with
                  roles, of the match states

The top-10 of `must2` is checked per set against a torch evaluation (the weights of the scoring positions by gathers
and float32 arithmetic, index_add_ into a dense row, the predicate from index_fill_ masks) by the rules of
tests/search_util.py check_topk: a check of the run, not a timing.  There is no pass/fail threshold on the times.

    python tools/time_search_bool.py [--gib 1.0] [--reps 5] [--words 65536] [--queries 64]
                                     [--out profiles/search_bool_timing.json]
"""
import argparse
import json
import math
import os
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
from time_search import PHASES, SETS, build_index, med, timed  # noqa: E402
from time_terms import prepare  # noqa: E402

S, MU, NO = M.native.Q_SHOULD, M.native.Q_MUST, M.native.Q_MUST_NOT
VARIANTS = (("search", None), ("all_should", (S, S, S, S)), ("must2", (MU, MU, S, S)), ("must4", (MU, MU, MU, MU)),
            ("not1", (S, S, S, NO)))


def torch_reference(ix, q, roles, k1, b):
    """float64 scores (queries x n_docs) of the Boolean queries by torch: 0 where the predicate fails"""
    post_off, docs, tf, E, doc_len, n_docs = ix
    h_po = post_off.cpu().numpy()
    avgdl = float(np.float32(float(doc_len.sum(dtype=torch.int64)) / n_docs))
    dlf = doc_len.to(torch.float32)
    scores = torch.zeros((len(q), n_docs), dtype=torch.float32, device="cuda:0")
    for i in range(len(q)):
        ok = torch.ones(n_docs, dtype=torch.bool, device="cuda:0")
        for t, role in zip(q[i], roles):
            a, e = int(h_po[t]), int(h_po[t + 1])
            d = docs[a:e].to(torch.int64)
            if role != S:
                held = torch.zeros(n_docs, dtype=torch.bool, device="cuda:0").index_fill_(0, d, True)
                ok &= held if role == MU else ~held
            if role == NO or e == a:
                continue
            idf = float(np.float32(math.log(1.0 + (n_docs - (e - a) + 0.5) / ((e - a) + 0.5))))
            f = tf[a:e].to(torch.float32)
            scores[i].index_add_(0, d, idf * (f * (k1 + 1.0)) / (f + k1 * ((1.0 - b) + b * (dlf[d] / avgdl))))
        scores[i] *= ok
    return scores.cpu().numpy().astype(np.float64)


def run_set(ctx, v, ix, name, lo, hi, nq, k, reps, k1=1.2, b=0.75):
    post_off, docs, tf, E, doc_len, n_docs = ix
    rng = np.random.default_rng(lo + 1)
    q = rng.integers(lo, hi, (nq, 4)).astype(np.int32)
    q_off = list(range(0, 4 * nq + 1, 4))
    d_q = torch.from_numpy(q.reshape(-1).copy()).to("cuda:0")
    top_docs = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
    top_scores = torch.empty(nq * k, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    a = (v, post_off.data_ptr(), docs.data_ptr(), tf.data_ptr(), E, doc_len.data_ptr(), n_docs, d_q.data_ptr())
    o = (top_docs.data_ptr(), top_scores.data_ptr())
    rows = {n: [] for n, _ in VARIANTS}
    wall = {n: [] for n, _ in VARIANTS}
    top = {}
    for i in range(reps + 1):                                # (the first round is the warm-up)
        for vname, roles in VARIANTS:                        # alternated: a drift of the run meets every variant
            t = time.perf_counter()
            if roles is None:
                top[vname] = ctx.search(*a, q_off, k, *o, k1=k1, b=b)
            else:
                top[vname] = ctx.search_bool(*a, bytes(roles) * nq, q_off, k, *o, k1=k1, b=b)
            ms = (time.perf_counter() - t) * 1e3
            if i:
                wall[vname].append(ms)
                rows[vname].append(ctx.search_info())
            if i == reps and vname == "must2":               # the rows of the checked variant
                got_d = top_docs.cpu().numpy().view(np.uint32).reshape(nq, k)[:, :min(k, 10)].copy()
                got_s = top_scores.cpu().numpy().reshape(nq, k)[:, :min(k, 10)].copy()

    k10 = min(k, 10)
    ref = torch_reference(ix, q, dict(VARIANTS)["must2"], k1, b)
    check_topk(got_d, got_s, [min(n, k10) for n in top["must2"]], ref, k10, 0)   # raises when the two disagree

    h_po = post_off.cpu().numpy()
    df = lambda t: int(h_po[t + 1] - h_po[t])
    res = {"set": name, "ranks": [lo, hi], "k": k, "queries": nq, "must2_top10_equals_torch": True, "variants": {}}
    for vname, roles in VARIANTS:
        r = roles or (S, S, S, S)
        scoring = sum(df(t) for row in q for t, role in zip(row, r) if role != NO)
        state = sum(df(t) for row in q for j, (t, role) in enumerate(zip(row, r))
                    if role == NO or (role == MU and t not in [u for u, ru in zip(row[:j], r[:j]) if ru == MU]))
        with_state = any(role != S for role in r)
        src = torch.empty(2 * scoring + state + 16, dtype=torch.int32, device="cuda:0")
        dst = torch.empty_like(src)
        acc = torch.empty((nq * (2 if with_state else 1), n_docs), dtype=torch.float32, device="cuda:0")

        def floor():
            dst.copy_(src, non_blocking=True)
            acc.zero_()
        ms_floor, _ = timed(floor, reps)
        del src, dst, acc
        info = rows[vname][-1]
        c = {"postings": info["postings"], "scoring_postings": scoring, "match_state_postings": state,
             "chunks": info["chunks"], "acc_launches": info["acc_launches"], "scratch_bytes": info["scratch_bytes"],
             "hits_min": min(top[vname]), "hits_max": max(top[vname])}
        for p in PHASES:
            c[p] = med([x[p] for x in rows[vname]])
        c["ms_search"] = med([sum(x[p] for p in PHASES) for x in rows[vname]])
        c["ms_search_wall"] = med(wall[vname])
        c["ms_floor"] = ms_floor
        res["variants"][vname] = c
    plain = res["variants"]["search"]
    for vname, _ in VARIANTS[1:]:
        c = res["variants"][vname]
        c["over_search"] = round(c["ms_search"] / plain["ms_search"], 3)
        c["wall_over_search_wall"] = round(c["ms_search_wall"] / plain["ms_search_wall"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bool_timing.json"))
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
            c = run_set(ctx, v, ix, name, lo, min(hi, v.size()[0]), a.queries, 10, a.reps)
            res["cases"].append(c)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            print(json.dumps(c), flush=True)
        v.close()


if __name__ == "__main__":
    main()
