"""K-means map (csrc/kernels/kmeans.hip, csrc/engine/kmeans.cpp) against an
exact integer oracle, over every route of the dispatcher.

Points and centroids with small integer coordinates make fp32 exact: the
direct (x-c)^2 score, the |c|^2 - 2 x.c score (VALU, matrix cores or library
GEMM), the fp32 LDS / register partial sums and the float counts are all
integers far below 2^24, and the two score forms differ by the per-point
constant |x|^2, so they order the centroids identically, ties included. The
map's output must therefore equal an int64 oracle bit for bit under the
first-minimum rule ("ties -> lower centroid index"); any difference is a bug
in a kernel, the dispatcher or the fallback, never rounding.

Which kernel a (D, K) pair reaches is decided by the dispatcher's LDS
arithmetic. `route()` below mirrors that arithmetic, and every case asserts
that the mirror predicts the route its id names, so an edit to the dispatcher
turns into "this case no longer covers route X" instead of a silent change
of what is tested.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_mapreduce_amd import C
from gpu_mapreduce_amd.models.kmeans import blobs

# ------------------------------------------------------------------ generator and oracle

FAR = 50  # the planted far centroid sits at (R + FAR, ...)


def lattice(n, D, K, seed, R=4):
    """int64 points [n, D] and centroids [K, D] in [-R, R]^D, with planted
    edge cases:
      * K >= 3: centroid K-1 is a copy of centroid 0 — it loses every tie to
        index 0, so its row must be exactly zero (tie rule + empty cluster);
      * K >= 4: centroid K//2 sits at (R+FAR, ...), farther from every point
        than any other centroid — its row must be zero as well;
      * the last min(ceil(n/4), 2K) points are copies of centroid rows
        (distance 0), cycling over all rows but the far one.
    The thresholds on K keep at least two distinct live centroids, so the
    argmin is never trivial because of the plants."""
    assert n * R < 2 ** 24, "an fp32 partial sum over all points must stay exact"
    assert D * (R + FAR) ** 2 + 2 * D * R * (R + FAR) < 2 ** 24, "every score must be an exact fp32 integer"
    rng = np.random.default_rng(seed)
    p = rng.integers(-R, R + 1, size=(n, D), dtype=np.int64)
    c = rng.integers(-R, R + 1, size=(K, D), dtype=np.int64)
    far = None
    if K >= 3:
        c[K - 1] = c[0]
    if K >= 4:
        far = K // 2
        c[far] = R + FAR
    rows = np.array([k for k in range(K) if k != far], dtype=np.int64)
    m = min((n + 3) // 4, 2 * K)
    if m:
        p[n - m:] = c[rows[np.arange(m) % len(rows)]]
    return p, c


def oracle(p, c):
    """[K, D+1] int64: per-cluster coordinate sums and count, each point going
    to the first minimum of |c|^2 - 2 x.c (all int64, chunked over points)"""
    n, D = p.shape
    K = c.shape[0]
    out = np.zeros((K, D + 1), dtype=np.int64)
    cc = (c * c).sum(1)
    ct = np.ascontiguousarray(c.T)
    step = max(1, (1 << 21) // K)
    for s in range(0, n, step):
        q = p[s:s + step]
        lab = (cc[None, :] - 2 * (q @ ct)).argmin(1)  # argmin: first minimum
        out[:, D] += np.bincount(lab, minlength=K)
        # sums: sort the chunk by cluster, add up each non-empty run
        order = np.argsort(lab, kind="stable")
        bounds = np.searchsorted(lab[order], np.arange(K + 1))
        live = np.flatnonzero(np.diff(bounds))
        out[live, :D] += np.add.reduceat(q[order], bounds[live], axis=0)
    return out


_cases = {}


def case(n, D, K, R=4):
    """(points, centroids, oracle) of one lattice case, computed once"""
    key = (n, D, K, R)
    if key not in _cases:
        p, c = lattice(n, D, K, seed=1000 * D + K + n, R=R)
        val = (p, c, oracle(p, c))
        if n > 100_000:  # the persistent-loop cases are used once: do not keep them
            return val
        _cases[key] = val
    return _cases[key]


def first_mismatch(kv, want):
    """None if the map's KV equals the oracle exactly, else a message naming
    the first differing (cluster, column, got, want)"""
    K, D1 = want.shape
    if kv.n != K * D1:
        return f"kv.n = {kv.n}, want {K * D1}"
    keys = kv.kdata.cpu().view(torch.int32).numpy()
    if not np.array_equal(keys, np.arange(K * D1, dtype=np.int32)):
        return "keys are not arange(K * (D + 1))"
    got = kv.vdata.cpu().view(torch.float64).numpy().reshape(K, D1)
    if np.array_equal(got, want.astype(np.float64)):
        return None
    k, j = np.argwhere(~(got == want))[0]
    return (f"{int((~(got == want)).sum())} of {got.size} values differ; first (cluster, column, got, want) = "
            f"({k}, {j}, {got[k, j]!r}, {int(want[k, j])})")


def check(n, D, K, device, R=4):
    p, c, want = case(n, D, K, R)
    pt = torch.from_numpy(p.astype(np.float32)).to(device)
    ct = torch.from_numpy(c.astype(np.float32)).to(device)
    kv = C.kmeans_map(pt, ct)
    bad = first_mismatch(kv, want)
    assert bad is None, f"n={n} D={D} K={K}: {bad}"
    assert int(want[:, D].sum()) == n
    if K >= 3:
        assert not want[K - 1].any()  # the planted duplicate of centroid 0 is empty
    if K >= 4:
        assert not want[K // 2].any()  # so is the far centroid


# ------------------------------------------------------------------ mirror of the dispatcher (kmeans.hip)

KB64 = 64 * 1024
MFMA_LDS_MAX = 120 * 1024  # kMfmaLds
TTILE, TKG, BCMAX = 2048, 8, 16
MFMA_GRID, MFMA_WG_POINTS = 2048, 64  # launch_mfma: nb <= 2048 workgroups x 4 waves x 16 points


def mfma_dp(D):
    return 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128 if D <= 128 else 0


def mfma_kp(K):
    return (K + 15) & ~15


def mfma_lds(D, K):
    return 4 * (mfma_kp(K) * mfma_dp(D) + mfma_kp(K) + K * (D + 1))


def tr_lds(D, K):
    return 4 * (4 * K + TTILE + max(D * TTILE, 8 * K * (D + 1)))


def batch_lds(D, K, bc):
    return 4 * (4 * K + bc * ((K * (D + 1)) | 1))


def batch_copies(D, K):
    bc = BCMAX
    while bc > 1 and batch_lds(D, K, bc) > KB64:
        bc >>= 1
    return bc


def small(D, K):
    return K * (2 * D + 1) * 4 <= KB64


def supported(D, K):
    if K < 1 or D < 1:
        return False
    if D in (1, 2, 3, 4, 8) and small(D, K):
        return True
    return bool(mfma_dp(D)) and mfma_lds(D, K) <= MFMA_LDS_MAX


def route(D, K, variant=0, gemm=False):
    """the kernel kmeans_map runs on the GPU for (D, K), as a string:
    tr/kg<KG>, batch/bc<copies>, reg, priv, generic, mfma/dp<DP>/<full|half>
    (half: KP is not a multiple of 32, so the last trip scores one 16-centroid
    tile), accum/lds or accum/global (library GEMM + argmin + k_kmeans_accum)"""
    if gemm or not supported(D, K):
        return "accum/lds" if K * (D + 1) * 4 <= KB64 else "accum/global"
    if D in (1, 2, 3, 4, 8) and small(D, K):
        if D <= 3:
            if variant == 4 and K <= 32:
                return "reg"
            if variant == 0 and K <= 32 * TKG and tr_lds(D, K) <= KB64:
                return "tr/kg%d" % (1 if K <= 32 else 2 if K <= 64 else 4 if K <= 128 else TKG)
            if variant != 1 and batch_lds(D, K, 1) <= KB64:
                return "batch/bc%d" % (1 if variant == 5 else batch_copies(D, K))
        if variant == 1 and K * (D + 1) <= 120:
            return "priv"
        return "generic"
    return "mfma/dp%d/%s" % (mfma_dp(D), "half" if mfma_kp(K) % 32 else "full")


def test_route_mirror_limits():
    """the LDS limits of the dispatcher that the route table below rests on"""
    assert tr_lds(3, 64) == 33 * 1024 and route(3, 64) == "tr/kg2"
    assert mfma_lds(16, 896) == 119 * 1024 and mfma_lds(16, 912) > MFMA_LDS_MAX
    assert mfma_lds(64, 128) > KB64  # more than 64 KiB of dynamic LDS in a default-dispatch launch
    assert small(8, 963) and not small(8, 964) and small(3, 2340) and not small(3, 2341)
    assert batch_lds(3, 2047, 1) <= KB64 < batch_lds(3, 2048, 1)
    # the matrix-core kernel is never reached with D < 5: past the `small`
    # bound of D in {1, 2, 3, 4} its own LDS need is beyond kMfmaLds
    for D in (1, 2, 3, 4):
        K = KB64 // (4 * (2 * D + 1)) + 1
        assert not small(D, K) and mfma_lds(D, K) > MFMA_LDS_MAX


# ------------------------------------------------------------------ CPU: matmul + argmin + index_add

@pytest.mark.parametrize("n", [0, 1, 2049])
@pytest.mark.parametrize("D,K", [(1, 1), (2, 5), (3, 33), (4, 7), (8, 64), (17, 31), (160, 8)])
def test_kmeans_lattice_cpu(D, K, n):
    check(n, D, K, "cpu")


# ------------------------------------------------------------------ GPU route table

N_GPU = 20_011
_TR_KG = {1: 1, 5: 1, 32: 1, 33: 2, 64: 2, 65: 4, 128: 4, 129: 8, 256: 8}
_MFMA_D = [5, 6, 7, 9, 16, 17, 33, 64, 65, 127, 128]
_MFMA_K = [1, 15, 16, 17, 33, 48]
_MFMA_HALF = {1: "half", 15: "half", 16: "half", 17: "full", 33: "half", 48: "half"}

ROUTES = [("tr/kg%d" % _TR_KG[K], D, K) for D in (1, 2, 3) for K in _TR_KG]
ROUTES += [("batch/bc8", 3, 257), ("batch/bc1", 3, 2047), ("batch/bc16", 1, 300)]
ROUTES += [("generic", D, K) for D, K in [(3, 2048), (3, 2340), (4, 1), (4, 7), (4, 64), (8, 7), (8, 64), (8, 963)]]
# covering subset of D x K: every D twice, every K three or four times, and
# K = 17 (the only full last trip) once per DP instantiation
_MFMA_PAIRS = {5: (1, 17), 6: (15, 33), 7: (16, 48), 9: (15, 48), 16: (33, 16), 17: (17, 48), 33: (1, 33),
               64: (15, 17), 65: (16, 33), 127: (48, 1), 128: (17, 15)}
ROUTES += [("mfma/dp%d/%s" % (mfma_dp(D), _MFMA_HALF[K]), D, K) for D in _MFMA_D for K in _MFMA_PAIRS[D]]
ROUTES += [("mfma/dp16/half", 8, 964),   # past the generic kernel's LDS bound
           ("mfma/dp16/full", 16, 896),  # 119 KiB of dynamic LDS
           ("mfma/dp64/full", 64, 128)]
ROUTES += [("accum/lds", 129, 8), ("accum/lds", 160, 8),
           ("accum/lds", 16, 912),       # mfma_lds > 120 KiB
           ("accum/lds", 3, 2341),       # not `small`, and too many centroids for the matrix-core kernel
           ("accum/global", 160, 128)]   # K * (D+1) floats > 64 KiB: fp64 global atomics


def _id(r, D, K):
    return f"{r}-D{D}-K{K}"


def test_route_table_covers_issue():
    """every D and K of the matrix-core grid appears at least twice, both
    shapes of its centroid loop and all four DP instantiations are there"""
    grid = [(D, K) for r, D, K in ROUTES if r.startswith("mfma") and D in _MFMA_D and K in _MFMA_K]
    for D in _MFMA_D:
        assert sum(d == D for d, _ in grid) >= 2
    for K in _MFMA_K:
        assert sum(k == K for _, k in grid) >= 2
    named = {r for r, _, _ in ROUTES}
    assert {"mfma/dp%d/%s" % (dp, h) for dp in (16, 32, 64, 128) for h in ("half", "full")} <= named
    assert {"tr/kg1", "tr/kg2", "tr/kg4", "tr/kg8", "batch/bc1", "batch/bc8", "generic", "accum/lds",
            "accum/global"} <= named


@pytest.mark.parametrize("r,D,K", ROUTES, ids=[_id(*x) for x in ROUTES])
def test_route_prediction(r, D, K):
    assert route(D, K) == r, f"(D={D}, K={K}) no longer covers route {r}: the dispatcher mirror says {route(D, K)}"


@pytest.mark.gpu
@pytest.mark.parametrize("r,D,K", ROUTES, ids=[_id(*x) for x in ROUTES])
def test_kmeans_lattice_gpu_routes(r, D, K):
    assert route(D, K) == r, f"(D={D}, K={K}) no longer covers route {r}: the dispatcher mirror says {route(D, K)}"
    check(N_GPU, D, K, "cuda")


# one case per kernel over the sizes around the MFMA row tile (16), a wave
# (64) and a tile of 2048 points
SWEEP = [("tr/kg1", 2, 5), ("batch/bc8", 3, 257), ("generic", 4, 7), ("mfma/dp16/half", 16, 10),
         ("mfma/dp128/half", 100, 40), ("accum/lds", 160, 8)]
SWEEP_N = [0, 1, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SWEEP_N)
@pytest.mark.parametrize("r,D,K", SWEEP, ids=[_id(*x) for x in SWEEP])
def test_kmeans_lattice_gpu_sizes(r, D, K, n):
    assert route(D, K) == r, f"(D={D}, K={K}) no longer covers route {r}: the dispatcher mirror says {route(D, K)}"
    check(n, D, K, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("D,K", [(1, 3), (2, 5)])
def test_kmeans_lattice_gpu_tr_persistent(D, K):
    """more tiles than the persistent grid of 8 workgroups per CU: some
    workgroups take a second trip, and the last tile is partial"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 8 * cus * TTILE + TTILE + 777
    assert route(D, K) == "tr/kg1"
    assert (n + TTILE - 1) // TTILE > 8 * cus
    check(n, D, K, "cuda", R=1)


@pytest.mark.gpu
def test_kmeans_lattice_gpu_mfma_persistent():
    """more than 2048 workgroups x 64 points: the wave loop takes a second trip"""
    n = 140_001
    assert route(16, 10) == "mfma/dp16/half"
    assert n > MFMA_GRID * MFMA_WG_POINTS
    check(n, 16, 10, "cuda")


# ------------------------------------------------------------------ env-selected variants, in child processes

# (environment, [(route under that environment, D, K)])
VARIANTS = [
    ({"MRH_KMEANS_KERNEL": "1"}, [("priv", 1, 8), ("priv", 2, 32), ("priv", 3, 30), ("priv", 4, 24), ("priv", 8, 13),
                                  ("generic", 8, 64)]),
    ({"MRH_KMEANS_KERNEL": "4"}, [("reg", 2, 32), ("reg", 3, 7), ("batch/bc16", 2, 33)]),
    ({"MRH_KMEANS_KERNEL": "5"}, [("batch/bc1", 2, 32), ("batch/bc1", 3, 257)]),
    ({"MRH_KMEANS_KERNEL": "6"}, [("batch/bc16", 2, 32), ("batch/bc8", 3, 257)]),
    ({"MRH_KMEANS_GEMM": "1"}, [("accum/lds", 2, 5), ("accum/lds", 16, 10)]),
]
VARIANT_N = [1, 2049, N_GPU]


def test_variant_route_prediction():
    for env, cases in VARIANTS:
        variant = int(env.get("MRH_KMEANS_KERNEL", "0"))
        gemm = env.get("MRH_KMEANS_GEMM") == "1"
        for r, D, K in cases:
            assert route(D, K, variant, gemm) == r, (env, D, K, route(D, K, variant, gemm))
            if r == "priv":
                assert K * (D + 1) <= 120


def _child(spec):
    """body of a variant child: spec is 'D:K,D:K,...'; exit status 1 and the
    first differing value on a mismatch"""
    for item in spec.split(","):
        D, K = (int(x) for x in item.split(":"))
        for n in VARIANT_N:
            p, c, want = case(n, D, K)
            kv = C.kmeans_map(torch.from_numpy(p.astype(np.float32)).cuda(), torch.from_numpy(c.astype(np.float32)).cuda())
            bad = first_mismatch(kv, want)
            if bad is not None:
                print(f"MISMATCH n={n} D={D} K={K}: {bad}", flush=True)
                return 1
            print(f"ok n={n} D={D} K={K}", flush=True)
    return 0


@pytest.mark.gpu
def test_kmeans_lattice_gpu_env_variants():
    """the kernel variant is read once per process, so each one runs in a
    fresh child; one child at a time, and none after a failed one"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_kmeans_exact as t; sys.exit(t._child(sys.argv[1]))"
            % (os.path.dirname(here), here))
    flags = ["-s"] if sys.flags.no_user_site else []
    for env, cases in VARIANTS:
        child_env = {k: v for k, v in os.environ.items() if k not in ("MRH_KMEANS_KERNEL", "MRH_KMEANS_GEMM")}
        child_env.update(env)
        spec = ",".join(f"{D}:{K}" for _, D, K in cases)
        r = subprocess.run([sys.executable, *flags, "-c", code, spec], env=child_env, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, f"{env}: child exit status {r.returncode}\n{r.stdout[-4000:]}"


# ------------------------------------------------------------------ random floats, near-ties removed

def float_margin_check(D, K, device):
    """blob points as in test_kmeans_map_gpu, without the points whose best
    and second-best float64 scores are closer than an fp32 error bound: each
    fp32 score is at most D+1 fused multiply-adds on partials bounded by
    S = max|c|^2 + 2 max|x| max|c| (Euclidean norms), two scores are
    compared, and a factor 2 is headroom: margin = 4 (D+2) 2^-24 S. On the
    remaining points every correct kernel makes the oracle's choice, so the
    counts are exact, and a sum differs from the float64 one by no more than
    the recursive-summation bound of its fp32 partials, count * 2^-24 * sum|x|."""
    n = 50_000
    p = blobs(n, D, K, seed=5, device=device)
    c = blobs(K, D, K, seed=6, device=device)
    p64, c64 = p.double().cpu().numpy(), c.double().cpu().numpy()
    cc = (c64 * c64).sum(1)
    score = cc[None, :] - 2.0 * (p64 @ c64.T)
    two = np.partition(score, 1, axis=1)[:, :2]
    S = cc.max() + 2.0 * np.sqrt((p64 * p64).sum(1).max() * cc.max())
    margin = 4 * (D + 2) * 2.0 ** -24 * S
    keep = (two[:, 1] - two[:, 0]) >= margin
    dropped = 1.0 - keep.mean()
    print(f"D={D} K={K}: margin {margin:.3e}, dropped {100 * dropped:.3f} % of {n} points")
    assert dropped <= 0.03
    pk, lab = p64[keep], score.argmin(1)[keep]
    ref = np.zeros((K, D + 1))
    sum_abs = np.zeros((K, D))
    np.add.at(ref[:, :D], lab, pk)
    np.add.at(sum_abs, lab, np.abs(pk))
    ref[:, D] = np.bincount(lab, minlength=K)
    kv = C.kmeans_map(p[torch.from_numpy(keep).to(device)].contiguous(), c)
    assert kv.n == K * (D + 1)
    assert np.array_equal(kv.kdata.cpu().view(torch.int32).numpy(), np.arange(K * (D + 1), dtype=np.int32))
    got = kv.vdata.cpu().view(torch.float64).numpy().reshape(K, D + 1)
    bound = ref[:, D:] * 2.0 ** -24 * sum_abs
    err = np.abs(got[:, :D] - ref[:, :D])
    print(f"D={D} K={K}: counts differ in {int((got[:, D] != ref[:, D]).sum())} clusters, "
          f"largest sum error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.array_equal(got[:, D], ref[:, D])
    assert np.all(err <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize("D,K", [(1, 8), (2, 32), (3, 256), (4, 7), (8, 64), (16, 10), (100, 40), (128, 16), (160, 8)])
def test_kmeans_map_gpu_float_margin(D, K):
    float_margin_check(D, K, "cuda")
