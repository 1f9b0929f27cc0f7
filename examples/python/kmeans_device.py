"""K-means (Lloyd iterations) written only with device functors: the points
are a KV in HBM, the current centroids live in ONE bound device buffer
(`args[0]`, the functors' user argument), and no functor is ever recompiled —
three sources, three run-time compiles for the whole run, whatever the
number of iterations.

    map      mr_map reads the centroids from args[0], emits (nearest, point)
    collate  groups the points of every cluster
    reduce   a fold functor emits (cluster, sum[D], count)
    scan     mr_scan writes sum / count into the SAME bound buffer

    python examples/python/kmeans_device.py [iterations=10] [seed=159]

It shows the argument and scan forms; models/kmeans.py (hand-written
kernels, in-mapper combining) is the fast K-means. Needs a GPU MapReduce and
runs on one rank (the scan writes this rank's buffer only)."""
import sys

import numpy as np

D, K = 2, 4

MAP = """
enum { D = %d };
// (id, point[D]) -> (nearest centroid, point[D]); centroids = args[0], K x D doubles
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long index, mrd::Emit& out, const mrd::Args& args) {
  const double* c = args[0].as<double>();
  const int K = (int)(args[0].count<double>() / D);
  double p[D];
  for (int d = 0; d < D; ++d) p[d] = value.as<double>(8 * d);
  int best = 0;
  double bd = 0;
  for (int k = 0; k < K; ++k) {
    double s = 0;
    for (int d = 0; d < D; ++d) s += (p[d] - c[k * D + d]) * (p[d] - c[k * D + d]);
    if (k == 0 || s < bd) {
      bd = s;
      best = k;
    }
  }
  out.emit(&best, 4, value.p, value.n);
}
""" % D

FOLD = """
enum { D = %d };
// (cluster, points) -> (cluster, sum[D], count)
struct mr_acc { double s[D]; double n; };
__device__ void mr_init(mrd::Bytes key, mr_acc& a) {
  for (int d = 0; d < D; ++d) a.s[d] = 0;
  a.n = 0;
}
__device__ void mr_add(mr_acc& a, mrd::Bytes v) {
  for (int d = 0; d < D; ++d) a.s[d] += v.as<double>(8 * d);
  a.n += 1;
}
__device__ void mr_merge(mr_acc& a, const mr_acc& b) {
  for (int d = 0; d < D; ++d) a.s[d] += b.s[d];
  a.n += b.n;
}
__device__ void mr_finish(mrd::Bytes key, const mr_acc& a, mrd::Emit& out) { out.emit(key.p, key.n, &a, sizeof(a)); }
""" % D

UPDATE = """
enum { D = %d };
// (cluster, sum[D], count) -> centroid `cluster` of args[0] = sum / count:
// one thread per cluster, distinct slots, plain stores; a cluster without
// points emits nothing and keeps its centroid
__device__ void mr_scan(mrd::Bytes key, mrd::Bytes value, long long index, const mrd::MutArgs& args) {
  double* c = args[0].as<double>();
  const int k = key.as<int>();
  const double n = value.as<double>(8 * D);
  for (int d = 0; d < D; ++d) c[k * D + d] = value.as<double>(8 * d) / n;
}
""" % D


def make_points(seed=159, nblob=8, per=512, grid=60, cells=16, spread=12):
    """nblob point-symmetric blobs of `per` integer-lattice points each, their
    centres on a coarse grid, and K initial centroids on the lattice (float64
    [n, D], [K, D]). The grid step is a multiple of every blob count a cluster
    can hold, so the mean of whole blobs is a lattice point itself."""
    rng = np.random.default_rng(seed)
    centres = grid * rng.integers(1, cells, size=(nblob, D))
    pts = []
    for c in centres:
        off = rng.integers(-spread, spread + 1, size=(per // 2, D))
        pts.append(c + off)
        pts.append(c - off)
    init = rng.integers(0, grid * cells, size=(K, D))
    return np.concatenate(pts).astype(np.float64), init.astype(np.float64)


def lloyd_step_numpy(points, centroids):
    """one Lloyd step on the host (the oracle): nearest centroid, lowest index
    on ties; an empty cluster keeps its centroid"""
    d2 = ((points[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2)
    near = d2.argmin(axis=1)
    out = centroids.copy()
    for k in range(len(centroids)):
        if (near == k).any():
            out[k] = points[near == k].sum(axis=0) / (near == k).sum()
    return out


def load_points(mr, points):
    """the points as a KV in HBM: (int64 id, D doubles)"""
    import torch
    p = torch.from_numpy(points).to(mr.device)
    ids = torch.arange(len(points), dtype=torch.int64, device=mr.device)
    mr.map(1, lambda itask, kv: kv.add_tensors(ids, p))
    return mr


def lloyd(mr_points, centroids, iterations, each=None):
    """`iterations` Lloyd steps over the points of mr_points; `centroids` (a
    float64 [K, D] device tensor) is bound once and updated in place by the
    scan functor. each(i, centroids), if given, runs after every step."""
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    mr = MapReduce(mr_points.comm)
    mr.device_args(centroids)
    for i in range(iterations):
        mr.map_device(mr_points, MAP)
        mr.collate()
        mr.reduce_device(FOLD)
        mr.scan_device(UPDATE)
        if each is not None:
            each(i, centroids)
    mr.device_args()
    return centroids


def main():
    import torch
    import gpu_mapreduce_amd as g
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    comm = g.init()
    if not comm.is_cuda or comm.size > 1:
        print("kmeans_device needs a GPU MapReduce on one rank; nothing to do")
        return 0
    points, init = make_points(seed)
    mrp = load_points(g.MapReduce(comm), points)
    c = torch.from_numpy(init).to(comm.device)
    before = g.C.device_functor_compiles()
    lloyd(mrp, c, iterations)
    print(f"{len(points)} points, {K} clusters, {iterations} iterations, "
          f"{g.C.device_functor_compiles() - before} functor compiles")
    for k, row in enumerate(c.cpu().tolist()):
        print(f"centroid {k}: " + " ".join(f"{x:.6f}" for x in row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
