"""The comparator merge sort (sort_keys_device with an mr_compare functor) on
one GPU, next to its two reference points: the radix route (mr_sortkey) on
keys that fit 64 bits, and the host comparator path sort_keys(compare_fn),
reached through OINK's named compare `compare_uint64` so the callback is C++.

Every figure is the op alone (device events around it, the KV rebuilt from the
same tensors before each run), after one warm-up run, median of 5. Results of
routes that sort the same data are compared before anything is printed.

    python tools/sort_compare_bench.py [--log2-fixed 24] [--log2-str 22] [--log2-host 22] [--out FILE]"""
import argparse
import io
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_mapreduce_amd.oink.interp import OINK  # noqa: E402
from gpu_mapreduce_amd.parallel.comm import Comm  # noqa: E402
from gpu_mapreduce_amd.runtime.mapreduce import MapReduce  # noqa: E402

CMP_U64X2 = """
// (u64 hi, u64 lo) ascending: a 128-bit key
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  const unsigned long long xh = x.as<unsigned long long>(0), yh = y.as<unsigned long long>(0);
  if (xh != yh) return xh < yh ? -1 : 1;
  const unsigned long long xl = x.as<unsigned long long>(8), yl = y.as<unsigned long long>(8);
  return xl < yl ? -1 : xl > yl ? 1 : 0;
}
"""
CMP_STR = """
// byte strings, lexicographic (a prefix first)
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  const long long n = x.n < y.n ? x.n : y.n;
  for (long long i = 0; i < n; ++i)
    if (x.p[i] != y.p[i]) return x.p[i] < y.p[i] ? -1 : 1;
  return x.n < y.n ? -1 : x.n > y.n ? 1 : 0;
}
"""
CMP_U64 = """
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  const unsigned long long a = x.as<unsigned long long>(), b = y.as<unsigned long long>();
  return a < b ? -1 : a > b ? 1 : 0;
}
"""
KEY_U64 = "__device__ unsigned long long mr_sortkey(mrd::Bytes x) { return x.as<unsigned long long>(); }\n"

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def check(ok, what):
    """a result check: said, counted, and the remaining measurements still run"""
    if not ok:
        say(f"CHECK FAILED: {what}")
        check.failed += 1


check.failed = 0


def timed(fill, op, reps=5):
    """median ms of op(mr) over reps runs after one warm-up; the last sorted KV"""
    ms, mr = [], None
    for rep in range(reps + 1):
        mr = fill()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        op(mr)
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), mr


def report(name, n, t):
    med, lo, hi, _ = t
    say(f"{name:58s} n=2^{n.bit_length() - 1}  median {med:10.2f} ms  (min {lo:.2f}, max {hi:.2f})  "
        f"{n / med / 1e3:8.2f} M pairs/s")


def same(a, b):
    ka, kb = a.kv, b.kv
    return ka.n == kb.n and torch.equal(ka.kdata, kb.kdata) and torch.equal(ka.vdata, kb.vdata)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-fixed", type=int, default=24)
    ap.add_argument("--log2-str", type=int, default=22)
    ap.add_argument("--log2-host", type=int, default=22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    comm = Comm(device="cuda")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    say(f"device {torch.cuda.get_device_name(0)}; events around the op, 1 warm-up, median of 5")

    def filler(keys, vals, koff=None):
        def fill():
            mr = MapReduce(comm)
            mr.map(1, lambda itask, kv: kv.add_tensors(keys, vals, koff=koff))
            return mr
        return fill

    # 1. 16-byte (u64, u64) keys, 8-byte values; few distinct high words so the low word decides often
    n = 1 << args.log2_fixed
    vals = torch.arange(n, dtype=torch.int64, device=dev)
    k16 = torch.stack([torch.randint(0, 1 << 12, (n,), generator=g, device=dev, dtype=torch.int64),
                       torch.randint(0, 1 << 62, (n,), generator=g, device=dev, dtype=torch.int64)], 1).contiguous()
    t = timed(filler(k16, vals), lambda mr: mr.sort_keys_device(CMP_U64X2))
    got = t[3].kv.kdata.view(torch.int64).view(-1, 2)
    order = torch.argsort(k16[:, 1], stable=True)
    order = order[torch.argsort(k16[:, 0][order], stable=True)]
    check(torch.equal(got, k16[order]) and torch.equal(t[3].kv.vdata.view(torch.int64), order),
          "16-byte keys: not the stable order of torch.argsort")
    report("mr_compare, 16-byte (u64,u64) keys, 8-byte values", n, t)
    del k16, got, order

    # 2. variable-width string keys (4..24 bytes over 4 letters), 8-byte values
    ns = 1 << args.log2_str
    lens = torch.randint(4, 25, (ns,), generator=g, device=dev, dtype=torch.int64)
    koff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    kbytes = torch.randint(97, 101, (int(koff[-1]),), generator=g, device=dev, dtype=torch.int64).to(torch.uint8)
    t = timed(filler(kbytes, vals[:ns].contiguous(), koff), lambda mr: mr.sort_keys_device(CMP_STR))
    report("mr_compare, string keys of 4..24 bytes, 8-byte values", ns, t)
    flag = timed(filler(kbytes, vals[:ns].contiguous(), koff), lambda mr: mr.sort_keys(5), reps=1)[3]
    ka, kb = t[3].kv, flag.kv  # against the built-in string sort (flag 5); equal keys only by key bytes
    check(torch.equal(ka.kdata, kb.kdata) and torch.equal(ka.koff, kb.koff), "string keys: differs from sort_keys(5)")
    del kbytes, koff, lens

    # 3. both device routes on the same 8-byte keys
    k8 = torch.randint(0, 1 << 62, (n,), generator=g, device=dev, dtype=torch.int64)
    tc = timed(filler(k8, vals), lambda mr: mr.sort_keys_device(CMP_U64))
    tr = timed(filler(k8, vals), lambda mr: mr.sort_keys_device(KEY_U64))
    check(same(tc[3], tr[3]), "u64 keys: mr_compare and mr_sortkey results differ")
    report("mr_compare, 8-byte u64 keys, 8-byte values", n, tc)
    report("mr_sortkey (radix), the same keys", n, tr)
    say(f"  merge sort / radix sort: {tc[0] / tr[0]:.2f}x the time")

    # 4. the host comparator path (OINK compare_uint64: C++ callback, std::stable_sort on the host) next to mr_compare
    nh = 1 << args.log2_host
    kh, vh = k8[:nh].contiguous(), vals[:nh].contiguous()
    o = OINK(comm, screen=io.StringIO(), logfile="none")
    o.file(text="mr hostsort\n")

    def fill_named():
        m = o.mr("hostsort")
        m.map(1, lambda itask, kv: kv.add_tensors(kh, vh))
        return m
    th = timed(fill_named, lambda mr: o.one("hostsort sort_keys compare_uint64"))
    td = timed(filler(kh, vh), lambda mr: mr.sort_keys_device(CMP_U64))
    check(same(th[3], td[3]), "u64 keys: the host comparator path and mr_compare results differ")
    report("host sort_keys(compare_fn) via OINK compare_uint64, u64 keys", nh, th)
    report("mr_compare, the same keys", nh, td)
    say(f"  host comparator path / merge sort: {th[0] / td[0]:.1f}x the time")
    o.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if check.failed else 0


if __name__ == "__main__":
    sys.exit(main())
