"""Times mrg_vocab_term_counts against mrg_vocab_encode of the same text in the same run and context, and
against a device-to-device copy of the id buffer.

Input, device-resident: 1 GiB of Zipf(1.1) text over 2^20 words (gen_zipf) in four files, as
tools/time_decode.py makes it.  One word-count job gives mrg_job_vocab(65536); its text goes through
mrg_vocab_from_text and that vocabulary encodes the buffer (--reps times, the library's HIP events per
pass).  The ids are then cut into documents by four layouts, which change only tok_off:

    four   the four files (the large path: radix sort, in slices)
    wg     documents of TERMS_WG_MAX ids (the workgroup path at its largest)
    d256   documents of 256 ids (the wave path at its largest)
    mix    20, 256, 700, TERMS_WG_MAX and 50000 ids, drawn at random (all three paths in one call)

Per layout the sizes-only call and the full call (cap = the number of ids) are timed --reps times after one
warm-up of each: HIP events per phase from mrg_terms_info, and the wall clock.  A hipMemcpyAsync of the id
buffer's bytes is timed with HIP events as the floor.  Both yardsticks come from code that term counts do
not touch.  There is no pass/fail threshold.  Each case merges its figures into the JSON file, so the
cases run as one process each, every one under its own time limit; the script starts no threads:

    timeout -k 10 300 python tools/time_terms.py --case four && \\
    timeout -k 10 300 python tools/time_terms.py --case wg && \\
    timeout -k 10 300 python tools/time_terms.py --case d256 && \\
    timeout -k 10 300 python tools/time_terms.py --case mix

    python tools/time_terms.py [--case four,wg,d256,mix] [--gib 1.0] [--reps 5] [--words 65536] [--out profiles/terms_timing.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mapreduce_rust_amd as M  # noqa: E402

SEED = 0x5EED2026
PHASES = ("ms_count_lds", "ms_count_large", "ms_emit_lds", "ms_emit_large")


def med(xs):
    return round(statistics.median(xs), 3)


def cut(n, sizes, seed=1):
    rng = random.Random(seed)
    off = [0]
    while off[-1] < n:
        off.append(min(n, off[-1] + rng.choice(sizes)))
    return off


def layout(name, tok):
    n = tok[-1]
    if name == "four":
        return tok
    if name == "wg":
        return cut(n, [M.native.TERMS_WG_MAX])
    if name == "d256":
        return cut(n, [256])
    return cut(n, [20, 256, 700, M.native.TERMS_WG_MAX, 50000])


def prepare(ctx, total, words, R, reps):
    """the text, its vocabulary, its ids on the device; encode and copy timed"""
    nf = 4
    fb = (total // nf) & ~15
    buf = torch.empty(nf * fb + 64, dtype=torch.uint8, device="cuda:0")
    for i in range(nf):
        ctx.gen_zipf(buf.data_ptr() + i * fb, fb, SEED, i, 1 << 20, 1.1)
    torch.cuda.synchronize()
    off = [i * fb for i in range(nf + 1)]
    ctx.set_timing(True)
    ctx.job_begin(M.APP_WC, R, M.FLAG_NO_COMPAT_DROP_LAST)
    ctx.set_input(buf.data_ptr(), off)
    ctx.map()
    with ctx.vocab(words) as vj:
        text = vj.text()
    ctx.job_begin(M.APP_WC, R, 0)     # the job's memory goes back to the pool: term counts need no job
    v = ctx.vocab_from_text(text)
    n_tok = ctx.encode(v, buf.data_ptr(), off)[-1]
    ids = torch.empty(n_tok + 16, dtype=torch.int32, device="cuda:0")
    tok = ctx.encode(v, buf.data_ptr(), off, ids.data_ptr(), n_tok)      # (warm-up)
    enc = []
    for _ in range(reps):
        ctx.encode(v, buf.data_ptr(), off, ids.data_ptr(), n_tok)
        r = ctx.encode_info()
        enc.append(r["ms_count"] + r["ms_offsets"] + r["ms_emit"])
    unk = ctx.encode_info()["unk"]
    del buf
    dst = torch.empty(n_tok + 16, dtype=torch.int32, device="cuda:0")
    copy_ms = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst[:n_tok].copy_(ids[:n_tok], non_blocking=True)
        e1.record()
        e1.synchronize()
        if i:
            copy_ms.append(e0.elapsed_time(e1))
    del dst
    base = {"input_bytes": nf * fb, "vocab_words": v.size()[0], "ids": n_tok, "unk_ids": unk,
            "ms_encode": med(enc), "ms_copy_ids": med(copy_ms)}
    return v, ids, tok, base


def run_case(ctx, name, v, ids, tok, base, reps):
    n = tok[-1]
    toff = layout(name, tok)
    terms = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    counts = torch.empty(n + 16, dtype=torch.int32, device="cuda:0")
    rows = {"sizes": [], "full": []}
    wall = {"sizes": [], "full": []}
    for i in range(reps + 1):                                # (the first of each is the warm-up)
        for kind in ("sizes", "full"):
            t = time.perf_counter()
            if kind == "sizes":
                row_off, unk = ctx.term_counts(v, ids.data_ptr(), toff)
            else:
                row_off2, unk2 = ctx.term_counts(v, ids.data_ptr(), toff, terms.data_ptr(), counts.data_ptr(), n)
            ms = (time.perf_counter() - t) * 1e3
            if i:
                wall[kind].append(ms)
                rows[kind].append(ctx.terms_info())
    info = rows["full"][-1]
    # a check of the run, not a timing: the two calls agree, and every id is counted once
    entries = row_off[-1]
    ok = row_off2 == row_off and unk2 == unk and int(counts[:entries].sum(dtype=torch.int64)) + sum(unk) == n
    res = dict(base)
    res.update({"case": name, "docs": len(toff) - 1, "reps": reps, "entries": entries, "unk": info["unk"],
                "wave_docs": info["wave_docs"], "wg_docs": info["wg_docs"], "large_docs": info["large_docs"],
                "slices": info["slices"], "scratch_bytes": info["scratch_bytes"], "counts_ok": bool(ok)})
    for kind in ("sizes", "full"):
        for p in PHASES:
            res["%s_%s" % (kind, p)] = med([r[p] for r in rows[kind]])
        res["ms_%s" % kind] = med([sum(r[p] for p in PHASES) for r in rows[kind]])
        res["ms_%s_wall" % kind] = med(wall[kind])
    res["full_over_encode"] = round(res["ms_full"] / res["ms_encode"], 2)
    res["full_over_copy"] = round(res["ms_full"] / res["ms_copy_ids"], 2)
    res["sizes_over_copy"] = round(res["ms_sizes"] / res["ms_copy_ids"], 2)
    res["full_Gids_per_s"] = round(n / res["ms_full"] / 1e6, 2)
    del terms, counts
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="four,wg,d256,mix")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_timing.json"))
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
        v, ids, tok, base = prepare(ctx, total, a.words, a.reduce, a.reps)
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
