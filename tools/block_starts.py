"""Token starts per 1 KiB tile and per 2 KiB block of the C3 text.

Generates files of the bench's Zipf text on the device (the bench's seed, vocabulary and exponent), copies
them to the host and counts, with numpy, the bytes that start a token (a non-space byte after a space or at
the file's start) in every tile and block of the map's grid: the rounds of 128 tokens each takes when a wave
queues per tile, and when it queues per block with a queue of `--qcap` starts.

usage: python tools/block_starts.py [--files 2] [--out profiles/map_block_queue/block_starts.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mapreduce_rust_amd as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2)
    ap.add_argument("--file-mib", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0x5EED2026)
    ap.add_argument("--vocab", type=int, default=1 << 20)
    ap.add_argument("--zipf-s", type=float, default=1.1)
    ap.add_argument("--qcap", type=int, default=320)
    ap.add_argument("--out", default="profiles/map_block_queue/block_starts.json")
    a = ap.parse_args()
    fbytes = a.file_mib << 20
    tiles, blocks, tokens = [], [], 0
    with M.Context(0) as ctx:
        buf = torch.empty(fbytes + 64, dtype=torch.uint8, device="cuda:0")
        for fi in range(a.files):
            ctx.gen_zipf(buf.data_ptr(), fbytes, a.seed, fi, a.vocab, a.zipf_s)
            torch.cuda.synchronize()
            x = buf[:fbytes].cpu().numpy()
            sp = (x == 32) | ((x >= 9) & (x <= 13))
            st = ~sp
            st[1:] &= sp[:-1]
            tokens += int(st.sum())
            tiles.append(st.reshape(-1, 1024).sum(axis=1))
            blocks.append(st.reshape(-1, 2048).sum(axis=1))
    t, b = np.concatenate(tiles), np.concatenate(blocks)
    rounds_tile = int((-(-t // 128)).sum())
    rounds_block = int((-(-np.minimum(b, a.qcap) // 128)).sum())   # (a block past qcap is drained in ranges)
    res = {
        "files": a.files, "file_mib": a.file_mib, "bytes_per_token": round(a.files * fbytes / tokens, 4),
        "tile": {"mean": round(float(t.mean()), 2), "std": round(float(t.std()), 2), "max": int(t.max()),
                 "share_over_128": round(float((t > 128).mean()), 5),
                 "second_round_tokens_mean": round(float((t[t > 128] - 128).mean()), 2)},
        "block": {"mean": round(float(b.mean()), 2), "std": round(float(b.std()), 2), "max": int(b.max()),
                  "share_over_256": round(float((b > 256).mean()), 5),
                  "share_over_qcap": round(float((b > a.qcap).mean()), 7), "qcap": a.qcap},
        "rounds_per_block": {"per_tile_queues": round(rounds_tile / len(b), 4),
                             "block_queue": round(rounds_block / len(b), 4)},
    }
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
