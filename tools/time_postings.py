"""Times mrg_vocab_postings on the document-term matrix of tools/time_terms.py's input, in the same run and
context as three yardsticks.

Input, device-resident: the ids of 1 GiB of Zipf(1.1) text under a vocabulary of 65536 words, exactly as
tools/time_terms.py prepares them (its prepare() is used), cut into documents of 256 ids (d256) or of
TERMS_WG_MAX ids (wg); mrg_vocab_term_counts gives the CSR.  Per layout, --reps times after one warm-up
of each, medians:

    df        mrg_vocab_postings, document frequencies only   (HIP events per phase, mrg_postings_info)
    full      mrg_vocab_postings with documents and term frequencies
    terms     mrg_vocab_term_counts of the same ids (the call that made the input)
    copy      a device-to-device copy of the three entry arrays (terms, counts, documents: 12 bytes per entry)
    torch     the route a user has without the call: torch.sort(terms, stable=True), a repeat_interleave for
              the rows, two gathers, torch.bincount and a cumsum

The torch route's result is compared with the call's (a check of the run, not a timing).  There is no
pass/fail threshold.  Each case merges its figures into the JSON file, so the cases run as one process each,
every one under its own time limit; the script starts no threads:

    timeout -k 10 300 python tools/time_postings.py --case d256 && \\
    timeout -k 10 300 python tools/time_postings.py --case wg

    python tools/time_postings.py [--case d256,wg] [--gib 1.0] [--reps 5] [--words 65536] [--out profiles/postings_timing.json]
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
import torch  # noqa: E402
import mapreduce_rust_amd as M  # noqa: E402
from time_terms import layout, prepare  # noqa: E402

PHASES = ("ms_count", "ms_scan", "ms_pack", "ms_sort", "ms_unpack")
TERMS_PHASES = ("ms_count_lds", "ms_count_large", "ms_emit_lds", "ms_emit_large")


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


def run_case(ctx, name, v, ids, tok, base, reps):
    n = tok[-1]
    n_words = v.size()[0]
    toff = layout(name, tok)
    terms = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    counts = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    t_ms = []
    for i in range(reps + 1):
        row_off, unk = ctx.term_counts(v, ids.data_ptr(), toff, terms.data_ptr(), counts.data_ptr(), n)
        if i:
            r = ctx.terms_info()
            t_ms.append(sum(r[p] for p in TERMS_PHASES))
    E = row_off[-1]
    terms, counts = terms[:E].clone(), counts[:E].clone()
    post_off = torch.empty(n_words + 1, dtype=torch.int64, device="cuda:0")
    docs = torch.empty(E, dtype=torch.int32, device="cuda:0")
    tf = torch.empty(E, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rows = {"df": [], "full": []}
    wall = {"df": [], "full": []}
    for i in range(reps + 1):                                # (the first of each is the warm-up)
        for kind in ("df", "full"):
            t = time.perf_counter()
            if kind == "df":
                ctx.postings(v, terms.data_ptr(), None, row_off, post_off.data_ptr())
            else:
                ctx.postings(v, terms.data_ptr(), counts.data_ptr(), row_off, post_off.data_ptr(), docs.data_ptr(),
                             tf.data_ptr(), E)
            ms = (time.perf_counter() - t) * 1e3
            if i:
                wall[kind].append(ms)
                rows[kind].append(ctx.postings_info())
    info = rows["full"][-1]

    # the copy of the three entry arrays
    dst = torch.empty((3, E), dtype=torch.int32, device="cuda:0")

    def copy3():
        dst[0].copy_(terms, non_blocking=True)
        dst[1].copy_(counts, non_blocking=True)
        dst[2].copy_(docs, non_blocking=True)
    ms_copy, _ = timed(copy3, reps)
    del dst

    # the torch route
    n_docs = len(toff) - 1
    d_row_off = torch.tensor(row_off, dtype=torch.int64, device="cuda:0")

    def torch_route():
        order = torch.sort(terms, stable=True).indices
        r = torch.repeat_interleave(torch.arange(n_docs, dtype=torch.int32, device="cuda:0"), torch.diff(d_row_off))
        df = torch.bincount(terms, minlength=n_words)
        return torch.cumsum(df, 0), r[order], counts[order]
    ms_torch, (t_off, t_docs, t_tf) = timed(torch_route, reps)
    ok = bool((t_off == post_off[1:]).all()) and bool((t_docs == docs).all()) and bool((t_tf == tf).all())
    ok = ok and int(post_off[0]) == 0 and int(post_off[-1]) == E
    del t_off, t_docs, t_tf

    res = dict(base)
    res.update({"case": name, "docs": n_docs, "reps": reps, "entries": E, "words": n_words, "max_df": info["max_df"],
                "passes": info["passes"], "lds_entries": info["lds_entries"], "global_entries": info["global_entries"],
                "scratch_bytes": info["scratch_bytes"], "equals_torch_route": ok})
    for kind in ("df", "full"):
        for p in PHASES:
            res["%s_%s" % (kind, p)] = med([r[p] for r in rows[kind]])
        res["ms_%s" % kind] = med([sum(r[p] for p in PHASES) for r in rows[kind]])
        res["ms_%s_wall" % kind] = med(wall[kind])
    res["ms_term_counts"] = med(t_ms)
    res["ms_copy_entries"] = ms_copy
    res["ms_torch_route"] = ms_torch
    res["full_over_term_counts"] = round(res["ms_full"] / res["ms_term_counts"], 2)
    res["full_over_copy"] = round(res["ms_full"] / ms_copy, 2)
    res["torch_over_full"] = round(ms_torch / res["ms_full"], 2)
    res["full_Mentries_per_s"] = round(E / res["ms_full"] / 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="d256,wg")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postings_timing.json"))
    a = ap.parse_args()
    total = int(a.gib * (1 << 30))
    sha = M.native.kernel_source_sha()
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": sha, "cases": []}
    if os.path.exists(a.out):  # merge into the figures of the same sources
        old = json.load(open(a.out))
        if old.get("kernel_source_sha") == sha:
            res["cases"] = old.get("cases", [])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with M.Context(0) as ctx:
        v, ids, tok, base = prepare(ctx, total, a.words, a.reduce, 1)
        for name in a.case.split(","):
            c = run_case(ctx, name, v, ids, tok, base, a.reps)
            res["cases"] = [x for x in res["cases"] if x["case"] != name] + [c]
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            print(json.dumps(c))
        v.close()


if __name__ == "__main__":
    main()
