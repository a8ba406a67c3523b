"""Times mrg_vocab_encode against the map kernel on the same buffer and context.

Two inputs, device-resident, 1 GiB each by default: Zipf(1.1) text over 2^20 words (gen_zipf) and the
same in Gutenberg-like Unicode (gen_text style 1).  Per input: one word-count job over the buffer
(MRG_FLAG_NO_COMPAT_DROP_LAST, timing on) gives ms_map, the yardstick; mrg_job_vocab(65536) is timed
with HIP events and a host clock; then --reps encodes of the whole buffer with that vocabulary, each
pass timed by the library's HIP events (mrg_encode_info).  Medians.  Each case merges its figures into
the JSON file, so the two cases can run as two processes, each under its own time limit:

    timeout -k 10 300 python tools/time_encode.py --case zipf && \\
    timeout -k 10 300 python tools/time_encode.py --case gutenberg

    python tools/time_encode.py [--case zipf,gutenberg] [--gib 1.0] [--reps 7] [--words 65536] [--out profiles/encode_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mapreduce_rust_amd as M  # noqa: E402

SEED = 0x5EED2026


def med(xs):
    return round(statistics.median(xs), 3)


def run_case(ctx, name, style, total, words, R, reps):
    fb = 256 << 20
    nf = max(1, total // fb)
    fb = (total // nf) & ~15
    buf = torch.empty(nf * fb + 64, dtype=torch.uint8, device="cuda:0")
    for i in range(nf):
        ctx.gen_text(buf.data_ptr() + i * fb, fb, SEED, i, 1 << 20, 1.1, style)
    torch.cuda.synchronize()
    off = [i * fb for i in range(nf + 1)]
    ctx.set_timing(True)
    ms_map, ms_vocab, ms_vocab_wall = [], [], []
    v = None
    for _ in range(3):  # (the first is the warm-up of the pool and the map's hints)
        ctx.job_begin(M.APP_WC, R, M.FLAG_NO_COMPAT_DROP_LAST)
        ctx.set_input(buf.data_ptr(), off)
        ctx.map()
        st = ctx.stats()
        ms_map.append(st["ms_map"])
        if v is not None:
            v.close()
        t = time.perf_counter()
        v = ctx.vocab(words)
        ms_vocab_wall.append((time.perf_counter() - t) * 1e3)
        ms_vocab.append(ctx.encode_info()["ms_vocab"])
    n_tok = ctx.encode(v, buf.data_ptr(), off)[-1]   # count only (and the warm-up of the scratch blocks)
    out = torch.empty(n_tok + 16, dtype=torch.int32, device="cuda:0")
    ctx.encode(v, buf.data_ptr(), off, out.data_ptr(), n_tok)
    rows, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.encode(v, buf.data_ptr(), off, out.data_ptr(), n_tok)
        wall.append((time.perf_counter() - t) * 1e3)
        rows.append(ctx.encode_info())
    info = rows[-1]
    nbytes = nf * fb
    enc = [r["ms_count"] + r["ms_offsets"] + r["ms_emit"] for r in rows]
    k_map = statistics.median(ms_map[1:])
    res = {"case": name, "input_bytes": nbytes, "n_reduce": R, "reps": reps, "vocab_words": v.size()[0],
           "distinct_keys": st["distinct_keys"], "map_kind": st["map_kind"],
           "ms_map": round(k_map, 3), "map_GBps": round(nbytes / k_map / 1e6, 1),
           "ms_vocab": med(ms_vocab[1:]), "ms_vocab_wall": med(ms_vocab_wall[1:]),
           "ms_count": med([r["ms_count"] for r in rows]), "ms_offsets": med([r["ms_offsets"] for r in rows]),
           "ms_emit": med([r["ms_emit"] for r in rows]), "ms_encode": med(enc), "ms_encode_wall": med(wall),
           "encode_GBps": round(nbytes / statistics.median(enc) / 1e6, 1),
           "encode_over_map": round(statistics.median(enc) / k_map, 2),
           "tokens": info["tokens"], "unk": info["unk"], "long_tokens": info["long_tokens"],
           "nonascii_chunks": info["nonascii_chunks"], "chunks": (nbytes + 1023) // 1024, "probes": info["probes"],
           "scratch_bytes": info["scratch_bytes"]}
    v.close()
    del buf, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="zipf,gutenberg")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_timing.json"))
    a = ap.parse_args()
    total = int(a.gib * (1 << 30))
    sha = M.native.kernel_source_sha()
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_sha": sha, "cases": []}
    if os.path.exists(a.out):  # merge into the figures of the same sources
        old = json.load(open(a.out))
        if old.get("kernel_source_sha") == sha:
            res["cases"] = old.get("cases", [])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    styles = {"zipf": 0, "gutenberg": 1}
    with M.Context(0) as ctx:
        for name in a.case.split(","):
            c = run_case(ctx, name, styles[name], total, a.words, a.reduce, a.reps)
            res["cases"] = [x for x in res["cases"] if x["case"] != name] + [c]
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            print(json.dumps(c))


if __name__ == "__main__":
    main()
