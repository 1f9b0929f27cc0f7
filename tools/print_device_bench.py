#!/usr/bin/env python3
"""Measurements of the print functor (print_device / text_device), on one GPU.

    python tools/print_device_bench.py [--keys 22] [--pairs 20] [--reps 9] [--out FILE]

Without --step this is a driver: it runs every step below as a child process
of its own under `timeout`, stops at the first one that fails, and appends
what they print to --out (default: standard output only).

  step a  text_device on an InvertedIndex-shaped KMV (2^keys URL keys of 20-80
          bytes, 1-8 int32 values each) with a functor that writes
          "url\\tid id ... \\n": the staged route (a tile's text formatted in LDS,
          copied out in 16-byte lines) against every tile forced direct
          (MRH_TEXT_STAGE=0), alternating, and (b) the built-in formatter of
          csrc/kernels/apps.hip (C.inverted_index_format) on the same KMV with
          the decimal ids as its names: the same bytes, checked.
  step c  MapReduce.print of 2^pairs (uint64, uint64) pairs to a file against
          print_device writing the same bytes, checked.

Every time is a host clock around a call that ends synchronised (text_device
reads the text's size back; the built-in call is followed by a device
synchronise), after one warm-up call per variant (compile, module load,
allocator). Reported: the median of --reps calls and their min - max."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# task t -> the pairs of URL t: a key of 20 .. 80 bytes (NUL included), 1 .. 8 values
GEN = r"""
__device__ unsigned long long mix(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  const unsigned long long h = mix((unsigned long long)t + 1);
  const int len = 20 + (int)(h % 61);  // with the NUL
  const int nv = 1 + (int)((h >> 20) % 8);
  unsigned char url[80];
  const char head[] = "http://h/";
  int n = 0;
  for (; n < 9; ++n) url[n] = (unsigned char)head[n];
  unsigned long long x = (unsigned long long)t;
  // 18 bytes that no other task has: every key is unique
  for (int i = 0; i < 9; ++i, x /= 36) url[n++] = (unsigned char)((x % 36) < 10 ? '0' + x % 36 : 'a' + x % 36 - 10);
  unsigned long long r = h;
  while (n < len - 1) {
    url[n++] = (unsigned char)('a' + r % 26);
    r = r / 26 + 0x9e3779b97f4a7c15ull * (unsigned long long)n;
  }
  url[len - 1] = 0;
  for (int j = 0; j < nv; ++j) {
    const int id = (int)(mix(h + j) % 100000);
    out.emit(url, len, &id, 4);
  }
}
"""
# the built-in formatter's line: the URL without its NUL, a tab, "id " per value, a newline
PRINT_KMV = r"""
__device__ void mr_print(mrd::Bytes url, mrd::Values ids, mrd::Text& out) {
  out.put(url.p, url.n - 1);
  out.chr('\t');
  for (long long i = 0; i < ids.n; ++i) {
    out.dec(ids.get<int>(i));
    out.chr(' ');
  }
  out.chr('\n');
}
"""
GEN_PAIRS = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out) {
  out.emit((unsigned long long)t * 2654435761ull, (unsigned long long)t);
}
"""
# MapReduce::print's line for kflag 2, vflag 2 on rank 0
PRINT_KV = r"""
__device__ void mr_print(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Text& out) {
  out.str("KV pair: proc 0, sizes 8 8, key ");
  out.udec(key.as<unsigned long long>());
  out.str(", value ");
  out.udec(value.as<unsigned long long>());
  out.chr('\n');
}
"""


def timed(call, sync):
    sync()
    t0 = time.perf_counter()
    r = call()
    sync()
    return (time.perf_counter() - t0) * 1e3, r


def report(name, ms, nbytes):
    med = statistics.median(ms)
    print(f"  {name:<34s} median {med:9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   "
          f"{nbytes / med / 1e6:8.2f} GB/s of text", flush=True)
    return med


def step_a(args):
    import numpy as np
    import torch
    import gpu_mapreduce_amd as g
    C = g.C
    mr = g.MapReduce(g.Comm(device="cuda:0"))
    sync = torch.cuda.synchronize
    nkey = 1 << args.keys
    npair = mr.map_device(nkey, GEN)
    assert mr.collate() == nkey
    kmv = mr.kmv
    print(f"step a: {nkey} keys, {npair} values, {kmv.keys.kdata.numel()} key bytes", flush=True)
    ids = [str(i).encode() for i in range(100000)]
    names = torch.from_numpy(np.frombuffer(b"".join(ids), dtype=np.uint8).copy()).cuda()
    noff = torch.from_numpy(np.cumsum([0] + [len(x) for x in ids], dtype=np.int64)).cuda()

    def staged():
        os.environ["MRH_TEXT_STAGE"] = "1"
        return mr.text_device(PRINT_KMV)

    def direct():
        os.environ["MRH_TEXT_STAGE"] = "0"
        return mr.text_device(PRINT_KMV)

    def builtin():
        return C.inverted_index_format(kmv, names, noff)

    variants = [("text_device, staged route", staged), ("text_device, every tile direct", direct),
                ("built-in formatter (apps.hip)", builtin)]
    texts = []
    for name, f in variants:  # warm-up, and the three texts are the same bytes
        t0 = C.device_text_tiles()
        texts.append(timed(f, sync)[1])
        t1 = C.device_text_tiles()
        print(f"  warm-up {name}: {texts[-1].numel()} bytes, tiles staged/direct +{t1[0] - t0[0]}/+{t1[1] - t0[1]}",
              flush=True)
    assert torch.equal(texts[0], texts[1]) and torch.equal(texts[0], texts[2]), "the three texts differ"
    nbytes = texts[0].numel()
    del texts
    ms = {name: [] for name, _ in variants}
    for _ in range(args.reps):  # alternating
        for name, f in variants:
            ms[name].append(timed(f, sync)[0])
    med = [report(name, ms[name], nbytes) for name, _ in variants]
    print(f"  staged / direct = {med[0] / med[1]:.3f}   staged / built-in = {med[0] / med[2]:.3f}", flush=True)
    os.environ.pop("MRH_TEXT_STAGE", None)


def step_c(args):
    import torch
    import gpu_mapreduce_amd as g
    mr = g.MapReduce(g.Comm(device="cuda:0"))
    sync = torch.cuda.synchronize
    n = 1 << args.pairs
    assert mr.map_device(n, GEN_PAIRS) == n
    print(f"step c: {n} pairs", flush=True)
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "print.txt"), os.path.join(d, "print_device.txt")
        variants = [("MapReduce.print to a file", lambda: mr.print(-1, 1, 2, 2, file=a, fflag=0)),
                    ("print_device to a file", lambda: mr.print_device(b, 0, -1, PRINT_KV))]
        for _, f in variants:
            f()
        with open(a, "rb") as fa, open(b, "rb") as fb:
            ta, tb = fa.read(), fb.read()
        assert ta == tb, "print and print_device wrote different bytes"
        ms = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, f in variants:
                ms[name].append(timed(f, sync)[0])
        med = [report(name, ms[name], len(ta)) for name, _ in variants]
        print(f"  print / print_device = {med[0] / med[1]:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["a", "c"])
    ap.add_argument("--keys", type=int, default=22, help="step a: log2 of the keys")
    ap.add_argument("--pairs", type=int, default=20, help="step c: log2 of the pairs")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--out", help="append the steps' output to this file")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, ROOT)
        {"a": step_a, "c": step_c}[args.step](args)
        return 0
    for step in ("a", "c"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--keys", str(args.keys), "--pairs", str(args.pairs), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        text = "$ " + " ".join(cmd[4:]) + "\n" + r.stdout
        sys.stdout.write(text)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text)
        if r.returncode != 0:  # nothing more on this GPU after a step that failed
            sys.stderr.write(r.stderr[-4000:])
            print(f"step {step} failed with status {r.returncode}; stopping")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
