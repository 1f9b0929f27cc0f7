"""What the device functors' bound arguments cost and buy (docs/performance.md,
"Device functor arguments"). Prints plain text; the recorded run is
profiles/devfn_args.txt. Runs on a commit without the feature too: there it
measures item 1 and variant (a) of item 2, the counterparts to compare with.

  1. functors that do NOT use the argument: the README's map_device(1 << 27)
     and a fold reduce_device over one hot key of 2^27 values; every run's
     time, their minimum and their spread (max - min)
  2. an iteration whose parameter changes every step, a threshold filter over
     2^24 pairs: (a) the parameter pasted into the source, one hiprtc compile
     and module load per step; (b) the parameter in a bound buffer; and the
     compile on its own (device_functor_check of a fresh source)
  3. the K-means example's time per Lloyd iteration (examples/python/kmeans_device.py)

    python tools/functor_args_bench.py [runs=7]
"""
import importlib.util
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gpu_mapreduce_amd as g  # noqa: E402

MAP = """
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long t, mrd::Emit& out) {
  out.emit((long long)(t % 1000), (int)1);
}"""
HOT = """
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long t, mrd::Emit& out) { out.emit((long long)7, (int)1); }"""
FOLD = """
struct mr_acc { long long s; };
__device__ void mr_init(mrd::Bytes key, mr_acc& a) { a.s = 0; }
__device__ void mr_add(mr_acc& a, mrd::Bytes v) { a.s += v.as<int>(); }
__device__ void mr_merge(mr_acc& a, const mr_acc& b) { a.s += b.s; }
__device__ void mr_finish(mrd::Bytes key, const mr_acc& a, mrd::Emit& out) { out.emit(key.as<long long>(), a.s); }"""
GEN = """
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long t, mrd::Emit& out) {
  out.emit((long long)t, (double)((t * 2654435761ll >> 8) & 0xfffff));
}"""
PASTED = """
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long t, mrd::Emit& out) {
  if (v.as<double>() < %r) out.emit(k.as<long long>(), v.as<double>());
}"""
BOUND = """
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long t, mrd::Emit& out, const mrd::Args& args) {
  if (v.as<double>() < args[0].as<double>()[0]) out.emit(k.as<long long>(), v.as<double>());
}"""


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def report(name, ms):
    print(f"{name}: min {min(ms):.3f} ms, spread (max - min) {max(ms) - min(ms):.3f} ms, runs "
          + " ".join(f"{x:.3f}" for x in ms))


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    comm = g.Comm(device="cuda")
    has_args = hasattr(g.MapReduce, "device_args")
    print(f"device functor arguments: {'present' if has_args else 'absent (the counterpart commit)'}; {runs} runs each")

    print("\n1. functors that do not use the argument")
    mr = g.MapReduce(comm)
    mr.map_device(1 << 20, MAP)  # compile + warm
    report("map_device(1 << 27), t -> (t % 1000, 1)", [timed(lambda: mr.map_device(1 << 27, MAP)) for _ in range(runs)])
    mr.map_device(1 << 10, HOT)
    mr.collate()
    mr.reduce_device(FOLD)
    ms = []
    for _ in range(runs):
        mr.map_device(1 << 27, HOT)
        mr.collate()
        ms.append(timed(lambda: mr.reduce_device(FOLD)))
    report("reduce_device fold, one hot key of 2^27 values", ms)
    del mr

    print("\n2. a parameter that changes every step: threshold filter over 2^24 pairs")
    src = g.MapReduce(comm)
    src.map_device(1 << 24, GEN)
    out = g.MapReduce(comm)
    out.map_device(src, PASTED % 0.5)  # warm everything but the per-step compile
    report("(a) pasted into the source, per step (compile + load + run)",
           [timed(lambda i=i: out.map_device(src, PASTED % float(1000 * i + 1))) for i in range(runs)])
    t = []
    for i in range(runs):
        code = PASTED % float(1000 * i + 3)
        t0 = time.perf_counter()
        g.C.device_functor_check(code, False)
        t.append((time.perf_counter() - t0) * 1e3)
    report("    the hiprtc compile on its own", t)
    report("    the same source again (module cached)", [timed(lambda: out.map_device(src, PASTED % 0.5)) for _ in range(runs)])
    if has_args:
        thr = torch.zeros(1, dtype=torch.float64, device="cuda")
        out.device_args(thr)
        out.map_device(src, BOUND)
        before = g.C.device_functor_compiles()
        ms = []
        for i in range(runs):
            thr.fill_(float(1000 * i + 1))
            ms.append(timed(lambda: out.map_device(src, BOUND)))
        report("(b) in a bound buffer, per step", ms)
        print(f"    compiles during (b): {g.C.device_functor_compiles() - before}")

    if has_args:
        print("\n3. examples/python/kmeans_device.py, 4096 points, D = 2, K = 4")
        spec = importlib.util.spec_from_file_location("kmeans_device", os.path.join(ROOT, "examples", "python", "kmeans_device.py"))
        ex = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ex)
        points, init = ex.make_points()
        mrp = ex.load_points(g.MapReduce(comm), points)
        c = torch.from_numpy(init.copy()).cuda()
        ex.lloyd(mrp, c, 1)
        report("one Lloyd iteration (map, collate, fold reduce, scan)", [timed(lambda: ex.lloyd(mrp, c, 1)) for _ in range(runs)])
    return 0


if __name__ == "__main__":
    sys.exit(main())
