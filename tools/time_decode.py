"""Times mrg_vocab_decode against mrg_vocab_encode of the same buffer in the same run, and against a
device-to-device copy of the output's bytes.

Two inputs, device-resident, 1 GiB in four documents each by default, as tools/time_encode.py makes them:
Zipf(1.1) text over 2^20 words (gen_zipf) and the same in Gutenberg-like Unicode (gen_text style 1).  Per
input: one word-count job gives mrg_job_vocab(65536); its text goes through mrg_vocab_from_text (timed:
ms_from_text, beside ms_vocab) and that vocabulary is the one used.  The buffer is encoded (--reps times,
the library's HIP events per pass), the ids are decoded (--reps times, HIP events per pass) with the UNK
bytes "UNK_", and a hipMemcpyAsync of the output's byte count is timed with HIP events as the floor.
Medians after one warm-up of each.  Each case merges its figures into the JSON file, so the two cases
can run as two processes, each under its own time limit:

    timeout -k 10 300 python tools/time_decode.py --case zipf && \\
    timeout -k 10 300 python tools/time_decode.py --case gutenberg

    python tools/time_decode.py [--case zipf,gutenberg] [--gib 1.0] [--reps 7] [--words 65536] [--out profiles/decode_timing.json]
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
UNK_BYTES = b"UNK_"


def med(xs):
    return round(statistics.median(xs), 3)


def run_case(ctx, name, style, total, words, R, reps):
    nf = 4
    fb = (total // nf) & ~15
    buf = torch.empty(nf * fb + 64, dtype=torch.uint8, device="cuda:0")
    for i in range(nf):
        ctx.gen_text(buf.data_ptr() + i * fb, fb, SEED, i, 1 << 20, 1.1, style)
    torch.cuda.synchronize()
    off = [i * fb for i in range(nf + 1)]
    ctx.set_timing(True)
    ctx.job_begin(M.APP_WC, R, M.FLAG_NO_COMPAT_DROP_LAST)
    ctx.set_input(buf.data_ptr(), off)
    ctx.map()
    ms_vocab = []
    for _ in range(3):
        with ctx.vocab(words) as vj:
            text = vj.text()
        ms_vocab.append(ctx.encode_info()["ms_vocab"])
    ctx.job_begin(M.APP_WC, R, 0)     # the job's memory goes back to the pool: from_text and decode need no job
    ms_from_text, ms_from_text_wall = [], []
    v = None
    for _ in range(3):
        if v is not None:
            v.close()
        t = time.perf_counter()
        v = ctx.vocab_from_text(text)
        ms_from_text_wall.append((time.perf_counter() - t) * 1e3)
        ms_from_text.append(ctx.decode_info()["ms_from_text"])
    n_tok = ctx.encode(v, buf.data_ptr(), off)[-1]
    ids = torch.empty(n_tok + 16, dtype=torch.int32, device="cuda:0")
    tok = ctx.encode(v, buf.data_ptr(), off, ids.data_ptr(), n_tok)      # (warm-up)
    enc_rows = []
    for _ in range(reps):
        ctx.encode(v, buf.data_ptr(), off, ids.data_ptr(), n_tok)
        enc_rows.append(ctx.encode_info())
    out_off = ctx.decode(v, ids.data_ptr(), tok, unk=UNK_BYTES)
    n_out = out_off[-1]
    out = torch.empty(n_out + 64, dtype=torch.uint8, device="cuda:0")
    ctx.decode(v, ids.data_ptr(), tok, out.data_ptr(), n_out, unk=UNK_BYTES)   # (warm-up)
    dec_rows, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.decode(v, ids.data_ptr(), tok, out.data_ptr(), n_out, unk=UNK_BYTES)
        wall.append((time.perf_counter() - t) * 1e3)
        dec_rows.append(ctx.decode_info())
    # the floor: a device-to-device copy of the output's bytes
    dst = torch.empty(n_out + 64, dtype=torch.uint8, device="cuda:0")
    copy_ms = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst[:n_out].copy_(out[:n_out], non_blocking=True)
        e1.record()
        e1.synchronize()
        if i:
            copy_ms.append(e0.elapsed_time(e1))
    # the decoded text re-encodes to the same ids (a check of the run, not a timing)
    back = torch.empty(n_tok + 16, dtype=torch.int32, device="cuda:0")
    tok2 = ctx.encode(v, out.data_ptr(), out_off, back.data_ptr(), n_tok)
    same = tok2 == tok and bool(torch.equal(back[:n_tok], ids[:n_tok]))
    info = dec_rows[-1]
    nbytes = nf * fb
    enc = [r["ms_count"] + r["ms_offsets"] + r["ms_emit"] for r in enc_rows]
    dec = [r["ms_count"] + r["ms_offsets"] + r["ms_emit"] for r in dec_rows]
    m_enc, m_dec, m_copy = statistics.median(enc), statistics.median(dec), statistics.median(copy_ms)
    res = {"case": name, "input_bytes": nbytes, "docs": nf, "reps": reps, "vocab_words": v.size()[0],
           "ids": info["ids"], "output_bytes": n_out, "unk": enc_rows[-1]["unk"], "chunks": info["chunks"],
           "scratch_bytes": info["scratch_bytes"], "round_trip_ok": same,
           "ms_count": med([r["ms_count"] for r in dec_rows]), "ms_offsets": med([r["ms_offsets"] for r in dec_rows]),
           "ms_emit": med([r["ms_emit"] for r in dec_rows]), "ms_decode": round(m_dec, 3), "ms_decode_wall": med(wall),
           "decode_GBps": round((4 * info["ids"] + n_out) / m_dec / 1e6, 1),
           "ms_encode": round(m_enc, 3), "decode_over_encode": round(m_dec / m_enc, 2),
           "ms_copy": round(m_copy, 3), "decode_over_copy": round(m_dec / m_copy, 2),
           "ms_vocab": med(ms_vocab[1:]), "ms_from_text": med(ms_from_text[1:]),
           "ms_from_text_wall": med(ms_from_text_wall[1:])}
    v.close()
    del buf, ids, out, dst, back
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="zipf,gutenberg")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--reduce", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_timing.json"))
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
