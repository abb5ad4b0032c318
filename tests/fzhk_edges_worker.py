"""Runs of tests/test_gpu_fzhk_edges.py under knobs the library reads once per process (FW_SEG_TARGET: `static const` in the host pool and
in the device rounds), started as a child process by that module -- one child at a time, the knobs in its environment.  The tables and
job lists are those of tests/fzhk_edges_tables.py, so parent and child hold the same bytes.  Prints one JSON line.

usage: FW_SEG_TARGET=1 python tests/fzhk_edges_worker.py --mode batches --which long
           {"<batch index>": [job result, ...]}   the batches of long_segment_batches() in segments of 8 192 ranks
       FW_SEG_TARGET=16384 python tests/fzhk_edges_worker.py --mode batches --which dir
           the batch "deep_size4" in segments of 512 ranks (the level-3 directory limit)
       FW_SEG_TARGET=64 FW_DH_LOG=<file> python tests/fzhk_edges_worker.py --mode rounds
           the max_k 5 network of the two-factor table under the device rounds, in plain lists"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FW_KNOBS", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batches", "rounds"), required=True)
    ap.add_argument("--which", choices=("long", "dir"), default="long")
    a = ap.parse_args()
    from tests import test_gpu_fzhk_edges as E
    if a.mode == "rounds":
        out = E.rounds_result()
    else:
        out = {str(i): E.engine_results(b) for i, b in enumerate(E.worker_batches(a.which))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
