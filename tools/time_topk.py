"""Times mrg_job_topk against mrg_job_final on the same mapped job.

Two jobs, device-resident input: Zipf text (vocabulary 2^20) and near-unique keys, 1 GiB each by
default.  After a warm-up the three calls -- final, topk(100), topk(65535) -- alternate in one process;
each ends in a stream sync inside the library, so a host clock around the call times it.  Reports the
median of --reps rounds, and for each topk the keys, the candidates the select kept, the select
passes run and the bytes each pass read.  Writes the table as JSON (--out) and prints it.

    python tools/time_topk.py [--gib 1.0] [--reps 11] [--reduce 64] [--out profiles/topk_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mapreduce_rust_amd as M  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def run_case(ctx, name, gen, total, R, reps):
    L = M.load()
    fb = 256 << 20
    nf = max(1, total // fb)
    fb = (total // nf) & ~15  # (files start 16-byte aligned)
    buf = torch.empty(nf * fb + 64, dtype=torch.uint8, device="cuda:0")
    for i in range(nf):
        gen(buf.data_ptr() + i * fb, fb, i)
    torch.cuda.synchronize()
    ctx.job_begin(M.APP_WC, R)
    ctx.set_input(buf.data_ptr(), [i * fb for i in range(nf + 1)])
    ctx.map()
    nb, nl = C.c_uint64(), C.c_uint64()

    def final():
        rc = L.mrg_job_final(ctx.h, None, C.byref(nb))
        assert rc == 0, L.mrg_last_error()

    def topk(k):
        rc = L.mrg_job_topk(ctx.h, k, None, C.byref(nb), C.byref(nl))
        assert rc == 0, L.mrg_last_error()

    calls = [("final", final), ("topk_100", lambda: topk(100)), ("topk_65535", lambda: topk(65535))]
    for _ in range(2):  # warm-up: pool blocks allocated, the wide result made dense
        for _, f in calls:
            f()
    ms = {n: [] for n, _ in calls}
    info = {}
    for _ in range(reps):
        for n, f in calls:  # alternating
            ms[n].append(timed(f))
            if n != "final":
                info[n] = dict(ctx.topk_info(), lines=nl.value, bytes=nb.value)
    final()
    out = {"case": name, "input_bytes": nf * fb, "n_reduce": R, "reps": reps, "final_bytes": nb.value,
           "agg_path": ctx.stats()["agg_path"]}
    for n, _ in calls:
        out[n] = {"ms_median": round(statistics.median(ms[n]), 3), "ms_min": round(min(ms[n]), 3),
                  "ms_max": round(max(ms[n]), 3)}
        out[n].update(info.get(n, {}))
    del buf
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_timing.json"))
    a = ap.parse_args()
    total = int(a.gib * (1 << 30))
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": M.native.kernel_source_sha(), "cases": []}
    with M.Context(0) as ctx:
        res["cases"].append(run_case(ctx, "zipf_v2^20", lambda p, n, i: ctx.gen_zipf(p, n, 0x5EED2026, i, 1 << 20, 1.1),
                                     total, a.reduce, a.reps))
        res["cases"].append(run_case(ctx, "unique", lambda p, n, i: ctx.gen_unique(p, n, 0xC5, i), total, a.reduce,
                                     a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for c in res["cases"]:
        print(f"{c['case']}: {c['input_bytes'] >> 20} MiB, R {c['n_reduce']}, final {c['final']['ms_median']} ms")
        for k in ("topk_100", "topk_65535"):
            t = c[k]
            print(f"  {k}: {t['ms_median']} ms (min {t['ms_min']}), n {t['n']}, candidates {t['candidates']}, "
                  f"passes {t['passes']}, dropped {t['dropped']}, bytes/pass {t['pass_bytes']}")


if __name__ == "__main__":
    main()
