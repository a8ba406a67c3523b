"""Times the batched map (mrg_job_map_add, MRG_FLAG_STREAM) against the one-shot path.

resident   Device-resident input, job_begin .. reduce, host clock (every call ends in a stream sync
           inside the library): one mrg_job_map over the whole input (the yardstick) against the same
           input cut into batches for mrg_job_map_add.  4 GiB of Zipf(1.1) text in 4 x 1 GiB and
           16 x 256 MiB, and 1 GiB of near-unique keys in 4 batches, at nReduce 64.  After a warm-up of
           every variant the variants alternate; medians of --reps rounds.  Per batch: the map and
           aggregation kernels and the fold (HIP events), medians over batches and rounds.
files      mrg_run_job over page-cached files of the benchmark's end-to-end size (40 x 256 MiB of the
           same Zipf text, written just before), unstreamed against MRG_FLAG_STREAM with
           MRG_STREAM_BATCH_BYTES of 256 MiB, 1 GiB and 4 GiB, alternating; medians of --file-reps.

           Also both with MRG_READ_CHUNK_MIB of 8 and 32 (the readers' pinned staging chunks; the
           defaults are 32 unstreamed and 8 streamed).

    python tools/time_stream.py [--what resident,files] [--reps 7] [--file-reps 5] [--out profiles/stream_timing.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mapreduce_rust_amd as M  # noqa: E402

MIB = 1 << 20
SEED = 0x5EED2026


def med(xs):
    return round(statistics.median(xs), 3)


def gen(ctx, kind, dst, n, i):
    if kind == "zipf":
        ctx.gen_zipf(dst, n, SEED, i, 1 << 20, 1.1)
    else:
        ctx.gen_unique(dst, n, 0xC5, i)


def resident_case(ctx, name, kind, total, file_bytes, batchings, R, reps):
    nf = total // file_bytes
    buf = torch.empty(nf * file_bytes + 64, dtype=torch.uint8, device="cuda:0")
    for i in range(nf):
        gen(ctx, kind, buf.data_ptr() + i * file_bytes, file_bytes, i)
    torch.cuda.synchronize()
    ctx.set_timing(True)

    def one_shot():
        t = time.perf_counter()
        ctx.job_begin(M.APP_WC, R)
        ctx.set_input(buf.data_ptr(), [i * file_bytes for i in range(nf + 1)])
        ctx.map()
        st = ctx.stats()
        ctx.reduce()
        return (time.perf_counter() - t) * 1e3, [(st["ms_map"], st["ms_aggregate"], 0.0, 0.0)], ctx.stats()

    def batched(nb):
        per = nf // nb  # files per batch
        def run():
            t = time.perf_counter()
            ctx.job_begin(M.APP_WC, R)
            parts = []
            for b in range(nb):
                tb = time.perf_counter()
                base = buf.data_ptr() + b * per * file_bytes
                ctx.set_input(base, [i * file_bytes for i in range(per + 1)])
                ctx.map_add()
                wall = (time.perf_counter() - tb) * 1e3
                st = ctx.stats()
                parts.append((st["ms_map"], st["ms_aggregate"], ctx.acc_info()["ms_fold"], wall))
            te = time.perf_counter()
            ctx.reduce()
            end = time.perf_counter()
            st = ctx.stats()
            st["ms_emit_reduce"] = (end - te) * 1e3
            return (end - t) * 1e3, parts, st
        return run

    variants = [("one_shot", one_shot)] + [("map_add_%dx%dMiB" % (nb, total // nb // MIB), batched(nb)) for nb in batchings]
    for _ in range(2):  # warm-up of every variant: pool blocks, hints, code objects
        for _, f in variants:
            f()
    ms = {n: [] for n, _ in variants}
    parts = {n: [] for n, _ in variants}
    tail = {n: [] for n, _ in variants}
    last = {}
    for _ in range(reps):
        for n, f in variants:  # alternating
            w, p, st = f()
            ms[n].append(w)
            parts[n] += p
            tail[n].append(st.get("ms_emit_reduce", st["ms_sort"] + st["ms_format"]))
            last[n] = st
    out = {"case": name, "input_bytes": nf * file_bytes, "n_reduce": R, "reps": reps, "variants": {}}
    base = statistics.median(ms["one_shot"])
    for n, _ in variants:
        st = last[n]
        v = {"ms_median": med(ms[n]), "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
             "ratio_to_one_shot": round(statistics.median(ms[n]) / base, 3),
             "per_batch_ms": {"map_kernel": med([p[0] for p in parts[n]]), "aggregate_kernel": med([p[1] for p in parts[n]]),
                              "fold": med([p[2] for p in parts[n]]), "call_wall": med([p[3] for p in parts[n]])},
             "ms_emit_reduce" if n != "one_shot" else "ms_sort_format": med(tail[n]),
             "distinct_keys": st["distinct_keys"], "agg_path": st["agg_path"], "map_kind": st["map_kind"],
             "output_bytes": st["output_bytes"]}
        if n != "one_shot":
            v["accumulator"] = {k: x for k, x in ctx.acc_info().items() if k != "ms_fold"} if n == variants[-1][0] else None
        out["variants"][n] = v
    ob = {v["output_bytes"] for v in out["variants"].values()}
    assert len(ob) == 1, ("the variants' outputs differ in size", ob)
    del buf
    return out


def files_case(ctx, files, file_bytes, R, reps, chunks=()):
    d = tempfile.mkdtemp(prefix="mrg_stream_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        buf = torch.empty(file_bytes + 64, dtype=torch.uint8, device="cuda:0")
        host = torch.empty(file_bytes, dtype=torch.uint8, pin_memory=True)
        paths = []
        for i in range(files):
            gen(ctx, "zipf", buf.data_ptr(), file_bytes, i)
            torch.cuda.synchronize()
            host.copy_(buf[:file_bytes])
            p = os.path.join(d, f"gut-{i}.txt")
            with open(p, "wb") as f:
                f.write(host.numpy().tobytes())
            paths.append(p)
        del buf, host
        outd = os.path.join(d, "out")
        os.makedirs(outd)
        variants = [("unstreamed", 0, 0)] + [("stream_%dMiB" % (b // MIB), M.native.FLAG_STREAM, b)
                                             for b in (256 * MIB, 1 << 30, 4 << 30)]
        for chunk_mib in chunks:  # the same with another size of the pinned staging chunks (MRG_READ_CHUNK_MIB; defaults: 32 unstreamed, 8 streamed)
            variants += [("unstreamed_chunk%d" % chunk_mib, 0, -chunk_mib),
                         ("stream_1024MiB_chunk%d" % chunk_mib, M.native.FLAG_STREAM, -chunk_mib)]

        def run(flags, bb):
            if bb > 0:
                os.environ["MRG_STREAM_BATCH_BYTES"] = str(bb)
            elif bb < 0:
                os.environ["MRG_READ_CHUNK_MIB"] = str(-bb)
                os.environ["MRG_STREAM_BATCH_BYTES"] = str(1 << 30)
            t = time.perf_counter()
            st = M.native.run_job(paths, R, M.APP_WC, outd, flags)
            st["wall"] = (time.perf_counter() - t) * 1e3
            st["batches"], st["peak_input_bytes"] = M.native.run_stream_stats()
            os.environ.pop("MRG_STREAM_BATCH_BYTES", None)
            os.environ.pop("MRG_READ_CHUNK_MIB", None)
            return st

        for n, fl, bb in variants:  # warm-up: the library's host-side setup, the device block cache
            run(fl, bb)
        res = {n: [] for n, _, _ in variants}
        for _ in range(reps):
            for n, fl, bb in variants:  # alternating
                res[n].append(run(fl, bb))
        if os.environ.get("MRG_STREAM_TIMING_DEBUG"):  # one more streamed run with the library's own breakdown on stderr
            os.environ["MRG_DEBUG"] = "1"
            st = run(M.native.FLAG_STREAM, 1 << 30)
            os.environ.pop("MRG_DEBUG", None)
            print("debug run: ms_total %.2f ms_read %.2f ms_map %.2f" % (st["ms_total"], st["ms_read"], st["ms_map"]), file=sys.stderr)
        out = {"case": "files_zipf", "files": files, "file_bytes": file_bytes, "n_reduce": R, "reps": reps,
               "page_cache": "files written just before the runs", "variants": {}}
        base = statistics.median([r["ms_total"] for r in res["unstreamed"]])
        for n, _, _ in variants:
            rs = res[n]
            v = {k: med([r[k] for r in rs]) for k in ("ms_total", "ms_open", "ms_read", "ms_map", "ms_map_alloc", "ms_map_kernel",
                                                     "ms_aggregate_kernel", "ms_reduce", "ms_write", "wall")}
            v["ms_total_min"] = round(min(r["ms_total"] for r in rs), 3)
            v["ms_total_max"] = round(max(r["ms_total"] for r in rs), 3)
            v["ratio_to_unstreamed"] = round(statistics.median([r["ms_total"] for r in rs]) / base, 3)
            v["batches"], v["peak_input_bytes"] = rs[-1]["batches"], rs[-1]["peak_input_bytes"]
            v["output_bytes"] = rs[-1]["output_bytes"]
            out["variants"][n] = v
        assert len({v["output_bytes"] for v in out["variants"].values()}) == 1
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="resident,files")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--file-reps", type=int, default=5)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--zipf-gib", type=float, default=4.0)
    ap.add_argument("--unique-gib", type=float, default=1.0)
    ap.add_argument("--files", type=int, default=40)
    ap.add_argument("--file-mib", type=int, default=256)
    ap.add_argument("--chunk-mib", default="8,32", help="files: also time MRG_READ_CHUNK_MIB=<each of these> (empty: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_timing.json"))
    a = ap.parse_args()
    what = a.what.split(",")
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": M.native.kernel_source_sha(), "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def add(case):  # (written after every case: a later failure keeps the earlier figures)
        res["cases"].append(case)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    with M.Context(0) as ctx:
        if "resident" in what:
            add(resident_case(ctx, "resident_zipf_v2^20", "zipf", int(a.zipf_gib * (1 << 30)), 256 * MIB, (4, 16), a.reduce,
                              a.reps))
            add(resident_case(ctx, "resident_unique", "unique", int(a.unique_gib * (1 << 30)), 256 * MIB, (4,), a.reduce,
                              a.reps))
        if "files" in what:
            add(files_case(ctx, a.files, a.file_mib * MIB, a.reduce, a.file_reps,
                           [int(x) for x in a.chunk_mib.split(",") if x]))
    for c in res["cases"]:
        print(c["case"])
        for n, v in c["variants"].items():
            print("  %s: %s" % (n, json.dumps(v)))


if __name__ == "__main__":
    main()
