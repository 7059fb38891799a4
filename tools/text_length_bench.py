#!/usr/bin/env python3
"""bench.py with every text sample at ONE length (GPU box): the headline run's masks are uniform in [16, L]; this replaces them with
`--length T` tokens per sample, so that the packed text pass sees exactly batch x lookahead x T live rows -- T = L is the
full-length batch, at which the 256x128 tile of the out-projection and FFN2 (BertTextEncoder.text_narrow_tile) runs a round and a
half of workgroups where 256x192 runs one.  Everything else is bench.py's own main(), its arguments passed through, its JSON line
printed; pair a run with `--text-tiles out=22,ffn2=22` (the library's choice) to read the crossover live fraction.
usage: text_length_bench.py --length 128 [bench.py arguments, e.g. --steps 40 --repeats 5 --no-cpu-baseline --no-lookahead-compare]"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import bench


def main():
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--length", type=int, required=True, help="live tokens of every sample (1 .. --seq-len)")
    args, rest = ap.parse_known_args()
    make = bench.make_batches

    def make_fixed_length(B, n, seed, dev):
        out = make(B, n, seed, dev)
        for bt in out:
            m = bt["attention_mask"]
            if not 1 <= args.length <= m.shape[1]:
                raise SystemExit(f"--length {args.length}: 1 .. {m.shape[1]}")
            m.zero_()
            m[:, :args.length] = 1
        return out

    bench.make_batches = make_fixed_length
    sys.argv = [sys.argv[0]] + rest
    bench.main()


if __name__ == "__main__":
    main()
