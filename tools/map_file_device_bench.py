"""Times of the record split and the record functor map against the built-in
URL kernels, on the benchmark's synthetic HTML text already in HBM
(profiles/map_file_device.txt):

  1. C.split_records (count + scan + emit, the 9-byte separator `<a href="`)
     against C.url_starts (k_url_count + scan + k_url_emit, the same separator
     as compile-time constants), as GB/s of text;
  2. the InvertedIndex functor map of examples/python/inverted_index_device.py
     (split_records + devfn::map_records, no upload) against C.map_urls.

    python tools/map_file_device_bench.py [--mib 256] [--runs 7] [--warmup 2]

Every figure is wall time around one call with the device synchronised at both
ends; the minimum, the spread (max - min) and every run are printed."""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gpu_mapreduce_amd import C  # noqa: E402
from gpu_mapreduce_amd.utils import synth  # noqa: E402

TAG = b'<a href="'


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def report(name, ms, nbytes):
    lo = min(ms)
    print(f"{name}: min {lo:.3f} ms ({nbytes / lo / 1e6:.1f} GB/s), spread (max - min) {max(ms) - lo:.3f} ms, runs "
          + " ".join(f"{x:.3f}" for x in ms))
    return lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    n = a.mib << 20
    spec = importlib.util.spec_from_file_location("iid", os.path.join(ROOT, "examples", "python", "inverted_index_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    vocab = synth.url_vocab(1 << 20, seed=7, device="cuda")
    body = synth.html_file(n, a.seed * 1000003, device="cuda", vocab=vocab)
    text = torch.cat([body, torch.zeros(32, dtype=torch.uint8, device="cuda")])
    del body

    def bench(fn):
        for _ in range(a.warmup):
            fn()
        return [timed(fn)[1] for _ in range(a.runs)]

    print(f"text: {a.mib} MiB of synthetic HTML (seed {a.seed}) in HBM, {torch.cuda.get_device_name(0)}")
    (starts, nurl), _ = timed(lambda: C.url_starts(text, n))
    (off, nrec), _ = timed(lambda: C.split_records(text, n, n, TAG, False))
    head = nrec - nurl  # the text before the first link
    assert head in (0, 1) and torch.equal(off[head:nrec] + 9, starts), "split_records and url_starts disagree"
    print(f"{nurl} occurrences, {nrec} records")
    b = report("url_starts    (k_url_count + scan + k_url_emit)", bench(lambda: C.url_starts(text, n)), n)
    g = report("split_records (k_sep_count + scan + k_sep_emit)", bench(lambda: C.split_records(text, n, n, TAG, False)), n)
    print(f"ratio split_records / url_starts: {g / b:.3f}")

    def functor_map():
        o, r = C.split_records(text, n, n, TAG, False)
        return C.device_map_records(text, o, r, 0, 3, 0, ex.MAP)

    kv, _ = timed(functor_map)
    ref, _ = timed(lambda: C.map_urls(text, n, 3))
    assert kv.n == ref.n == nurl and torch.equal(kv.koff, ref.koff) and torch.equal(kv.kdata, ref.kdata), \
        "the functor map and map_urls disagree"
    del kv, ref
    b = report("map_urls                                        ", bench(lambda: C.map_urls(text, n, 3)), n)
    g = report("split_records + map_records (InvertedIndex map) ", bench(functor_map), n)
    report("map_records alone                               ",
           bench(lambda: C.device_map_records(text, off, nrec, 0, 3, 0, ex.MAP)), n)
    print(f"ratio functor map / map_urls: {g / b:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
