"""PageRankPlan (csrc/engine/graphplan.cpp) against an exact integer oracle,
over every iteration route, with float32 bit patterns compared.

Why float32 PageRank can be exact
---------------------------------
With alpha = 0.5, N = 2^k and every non-zero out-degree a power of two up to
2^m, the constants 1/N, 1/outdeg, base = (1 - alpha)/N and alpha are exact
float32 values, and every quantity an iteration forms is a non-negative
dyadic rational: c = r/outdeg, each partial sum of c, dmass/N, a + dterm,
base + alpha (a + dterm), the 2^62 fixed-point adds of k_pr_tile_step and
the fp64 partials of the L1 delta and the dangling mass. All terms are
non-negative, so any partial sum, in any order and in any kernel, is at most
the final value and a multiple of the unit u of its terms. If the final value
v satisfies v/u < 2^24 (2^53 for the fp64 sums), no operation on the way
rounds, with or without fma contraction, and every route must return the
bits of the integer oracle. A difference is a bug in a kernel, the plan build
or the dispatcher, never rounding.

`oracle()` computes the iterations in int64 units of 2^-U and checks that
budget itself, per destination: u_j is the finest unit among the c of j's
in-edges, dterm and base. It also requires every c to be a multiple of 2^-62
(the fixed-point scale of the tile step). T, the number of iterations
compared, is the largest count for which the budget holds; the oracle alone
decides it, and T < 2 fails the case (T >= 1 for the two named exceptions:
dangling vertices with in-edges, and the multi-slice blocking case).

Planted by `lattice_graph` (positions in the pull layout, where the edges are
sorted by the degree-descending new id of their destination; `pull_layout`
mirrors that order and `test_lattice_plants` asserts each plant):
  * out-degrees in {0} u {2^0..2^m}, every class populated;
  * exactly N / 2^j dangling vertices, without in-edges unless dangling_in;
  * new id 0 receives 1024 edges: its run starts on a wave-tile boundary
    (edge 0) and ends on one, and the next run starts on one (edge 1024);
  * one hub whose run starts off a boundary and spans several 1024-edge wave
    tiles; in the `big` graph more than 32 of them, at the end of an edge
    list of more than 2^17 edges, so that its carries cross a 64-entry wave
    of the tile kernel's level-1 carry fold (segred.h k_carry_fold). The wave
    gather's own two-level fold starts at 2^21 edges, outside the size limit
    of this file;
  * vertices with in-degree 0, a self-loop, multi-edges, and global ids in a
    random permutation (degree order differs from id order).

Routes, case ids and shapes (GPU unless noted)
----------------------------------------------
  host            build_host, CPU engine            g11, g13, degenerate; 2 and 3 gloo ranks
  pull/wave       MRH_PR_XCD=0: wave gather,        g11, g13, big, dang11, degenerate
                  scatter_f32, k_pr_update
  pull/tiles      + MRH_PLAN_KERNEL=tiles           g11, big
                  (pr_contrib)
  pull/variants   MRH_PR_DEGREES=partition | sort,  g13
                  MRH_PR_SRC_ORDER=1
  xcd             MRH_PR_L2_BYTES=4096 (cap 870     x11 (scalar tail of k_pr_tile_step),
                  ids), with and without            g13 (two full float4 tiles), dang13;
                  MRH_PR_XCD_LAYERS=1
  xcd/graph       HIP-graph replay of route xcd     g13, run(2) and run(3), twice
  blocking        MRH_PR_BLOCKING=1 (pbpr.hip)      blk (2 bins), slices (hub bin > 2^18 edges)
  rccl/...        forced one-rank RCCL plans, one   g13 with MRH_PR_L2_BYTES=4096
                  child process each: replicated,
                  pieces, pieces eager, partials
  tails           N = 2 * 4096 + 7, tolerance,      random graph, routes pull/wave and xcd
                  two steps
An empty edge list is not covered: PageRank.build() rejects it.
Graphs: g11 = lattice(11, 3), x11 = lattice(11, 5) with 1000 more sources of
out-degree 1 (several layers of ranges), g13 = lattice(13, 3), big = lattice(16, 2),
blk = lattice(15, 2), slices = lattice(15, 5), dang11/13 = dangling_in.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_mapreduce_amd as g
from gpu_mapreduce_amd.models.pagerank import PageRank, reference_pagerank

ALPHA = 0.5
WS_TILE = 1024        # wavesegred.h: edges per wave tile
SR_TILE = 4096        # segred.h: edges per block tile of the tiles kernel
PR_TILE = 4096        # graphops.hip: destinations per tile of k_pr_tile_step
PB_BIN = 1 << 14      # pbpr.hip: destinations per bin
PB_SLICE = 1 << 18    # graphplan.cpp build_blocking: edges per work unit
L2_SMALL = "4096"     # MRH_PR_L2_BYTES: cap = 4096 / 4 * 85 / 100 = 870 ids
XCD_CAP = 870

# ------------------------------------------------------------------ generator


def lattice_graph(k, m, seed, j=3, dangling_in=False, hub=None, hub_back=False, bin0=None, ones=0):
    """int64 edges [ne, 2] over N = 2^k vertices; see the module docstring for
    the plants. j: N / 2^j dangling vertices (None: none). hub: in-edges of the
    hub (default: three wave tiles and a bit). hub_back: the hub is the last
    receiving new id, so its run ends the edge list. bin0: fraction of the
    other edges whose destination has a new id below 2^14 (blocking bins).
    ones: that many more vertices of out-degree 1 (a long cold tail of sources:
    the XCD ranges then need several layers even at a small N)."""
    N = 1 << k
    rng = np.random.default_rng(seed)
    nd = (N >> j) if j is not None else 0
    na = N - nd
    ex = np.concatenate([np.arange(m + 1), np.zeros(ones, dtype=np.int64), rng.integers(0, m + 1, na - (m + 1) - ones)])
    ex = np.sort(ex)[::-1]  # new ids: by out-degree, descending
    deg = np.concatenate([np.int64(1) << ex, np.zeros(nd, dtype=np.int64)]).astype(np.int64)
    # global id of every new id: a random permutation, ascending inside each
    # degree class (the relabel is a stable sort by degree)
    p = rng.permutation(N).astype(np.int64)
    gid = p[np.lexsort((p, -deg))]
    ne = int(deg.sum())
    src = rng.permutation(np.repeat(np.arange(N, dtype=np.int64), deg))
    H = int(hub) if hub is not None else 3 * WS_TILE + 100
    hub_id = na - 1 if hub_back else 2
    lo, hi = (2, na - 1) if hub_back else (3, na)
    recv = np.arange(lo, hi, dtype=np.int64)
    recv = recv[recv % 16 != 5]  # planted in-degree 0 among the active vertices
    if dangling_in:
        recv = np.concatenate([recv, np.arange(na, N, dtype=np.int64)])
    rest = ne - WS_TILE - 7 - H
    assert rest > 0, "not enough edges for the plants"
    if bin0 is None:
        other = rng.choice(recv, rest)
    else:
        n0 = int(rest * bin0)
        other = np.concatenate([rng.choice(recv[recv < PB_BIN], n0), rng.choice(recv[recv >= PB_BIN], rest - n0)])
    indeg = np.bincount(other, minlength=N).astype(np.int64)
    indeg[0], indeg[1], indeg[hub_id] = WS_TILE, 7, H
    dst = np.repeat(np.arange(N, dtype=np.int64), indeg)
    i = int(np.flatnonzero(src == 0)[0])  # self-loop at new id 0 (slot 0 is one of its in-edges)
    src[[0, i]] = src[[i, 0]]
    e = np.stack([gid[src], gid[dst]], axis=1)
    return np.ascontiguousarray(e[rng.permutation(ne)])


def pull_layout(edges, N):
    """mirror of the pull layout: (new id of every global id, in-degree per
    new id, first edge of every new id's run)"""
    outdeg = np.bincount(edges[:, 0], minlength=N)
    order = np.argsort(-outdeg, kind="stable")
    new_of = np.empty(N, dtype=np.int64)
    new_of[order] = np.arange(N)
    indeg = np.bincount(new_of[edges[:, 1]], minlength=N)
    start = np.concatenate([[0], np.cumsum(indeg)[:-1]])
    return new_of, indeg, start


GRAPHS = {
    "g11": dict(k=11, m=3, seed=11),
    "x11": dict(k=11, m=5, seed=111, ones=1000),
    "g13": dict(k=13, m=3, seed=13, hub=5 * WS_TILE + 100),
    "big": dict(k=16, m=2, seed=16, hub=34 * WS_TILE + 333, hub_back=True),
    "blk": dict(k=15, m=2, seed=15, hub=6 * WS_TILE + 9, bin0=0.5),
    "slices": dict(k=15, m=5, seed=155, hub=40 * WS_TILE + 77, bin0=0.97),
    "dang11": dict(k=11, m=3, seed=211, dangling_in=True),
    "dang13": dict(k=13, m=2, seed=213, dangling_in=True, hub=4 * WS_TILE + 50),
    "nodangling": dict(k=11, m=3, seed=311, j=None),
}
# iterations the oracle must allow at least
TMIN = {name: 2 for name in GRAPHS}
TMIN.update(slices=1, dang11=1, dang13=1)

DEGENERATE = {
    # N = 2: vertex 0 has a self-loop and an edge to the dangling vertex 1
    "n2": (1, [[0, 0], [0, 1]]),
    # N = 4: out-degrees 2, 1, 1, 0; a self-loop; vertex 3 dangling with an in-edge
    "n4": (2, [[0, 1], [0, 2], [1, 1], [2, 3]]),
    # all but two vertices dangling
    "twolive": (11, [[5, 9], [5, 5], [9, 5]]),
}
TMIN.update({name: 2 for name in DEGENERATE})

_graphs = {}


def graph(name):
    """(k, edges, oracle) of a named graph, computed once and left unchanged"""
    if name not in _graphs:
        if name in DEGENERATE:
            k, e = DEGENERATE[name]
            edges = np.array(e, dtype=np.int64).reshape(-1, 2)
        else:
            k = GRAPHS[name]["k"]
            edges = lattice_graph(**GRAPHS[name])
        edges.setflags(write=False)
        _graphs[name] = (k, edges, oracle(edges, k))
    return _graphs[name]


# ------------------------------------------------------------------ oracle


def _tz(v):
    """trailing zero bits of every int64 in v (63 for 0)"""
    v = np.asarray(v, dtype=np.int64)
    low = v & -v
    out = np.full(v.shape, 63, dtype=np.int64)
    nz = low > 0
    out[nz] = np.frexp(low[nz].astype(np.float64))[1] - 1  # a power of two: exact
    return out


class Oracle:
    """steps[t - 1] = (U, r, delta, dmass): after iteration t the rank of
    global id v is r[v] * 2^-U, the L1 delta is delta * 2^-U and the dangling
    mass dmass * 2^-U. T = len(steps); why = the budget check that ended it."""

    def __init__(self, edges, k):
        self.k, self.N, self.ne = k, 1 << k, len(edges)
        self.outdeg = np.bincount(edges[:, 0], minlength=self.N).astype(np.int64)
        self.indeg = np.bincount(edges[:, 1], minlength=self.N).astype(np.int64)
        self.ndangling = int((self.outdeg == 0).sum())
        self.steps, self.why = [], None

    @property
    def T(self):
        return len(self.steps)

    def want(self, t):
        """float32 ranks after iteration t"""
        U, r, _, _ = self.steps[t - 1]
        return np.ldexp(r.astype(np.float64), -U).astype(np.float32)

    def delta(self, t):
        U, _, d, _ = self.steps[t - 1]
        return math.ldexp(d, -U)


def oracle(edges, k, tmax=4):
    o = Oracle(edges, k)
    N = o.N
    live = o.outdeg > 0
    assert not (o.outdeg[live] & (o.outdeg[live] - 1)).any(), "out-degrees must be powers of two"
    lg = np.zeros(N, dtype=np.int64)
    lg[live] = _tz(o.outdeg[live])
    m = int(lg.max()) if N else 0
    by_dst = np.argsort(edges[:, 1], kind="stable")
    src = edges[by_dst, 0]
    has = o.indeg > 0
    first = (np.cumsum(o.indeg) - o.indeg)[has]
    U, r = k, np.ones(N, dtype=np.int64)
    for _ in range(tmax):
        # c = r / outdeg in units of 2^-(U + m); the tile step adds c in units of 2^-62
        Uc = U + m
        if Uc > 62:
            o.why = "c is finer than the 2^-62 fixed point"
            break
        c = np.where(live, r << (m - lg), 0)
        a = np.zeros(N, dtype=np.int64)
        fine = np.full(N, 63, dtype=np.int64)  # trailing zeros of the finest in-edge term
        if o.ne:
            a[has] = np.add.reduceat(c[src], first)
            fine[has] = np.minimum.reduceat(_tz(c)[src], first)
        # dterm = dmass / N, formed in fp64 and converted to float32
        dm = int(r[~live].astype(object).sum()) if o.ndangling else 0
        Ud, dmi = k, 0
        if dm:
            z = (dm & -dm).bit_length() - 1
            dmi, Ud = dm >> z, U + k - z
            if dmi.bit_length() > 24:
                o.why = "dterm needs %d bits" % dmi.bit_length()
                break
        Ux = max(Uc, Ud, k) + 1
        if Ux > 62:
            o.why = "ranks finer than 2^-62"
            break
        x = (np.int64(1) << (Ux - k - 1)) + (a << (Ux - 1 - Uc)) + (np.int64(dmi) << (Ux - 1 - Ud))
        # unit of everything formed on the way to x_j: the finest of j's terms
        W = np.maximum(np.maximum(Uc - fine, Ud), k) + 1
        over = (x >> (Ux - W)) >= (1 << 24)
        if over.any():
            o.why = "%d ranks need more than 24 bits" % int(over.sum())
            break
        rs = r << (Ux - U)
        d = int(np.abs(x - rs).astype(object).sum())
        z = int(min(_tz(x).min(), _tz(rs).min()))
        dmn = int(x[~live].astype(object).sum()) if o.ndangling else 0
        if (d >> z) >= (1 << 53) or (dmn >> int(_tz(x).min())) >= (1 << 53):
            o.why = "fp64 delta / dangling mass need more than 53 bits"
            break
        o.steps.append((Ux, x, d, dmn))
        U, r = Ux, x
    return o


# ------------------------------------------------------------------ comparison


def first_mismatch(o, t, ids, ranks):
    """None if the plan's (ids, ranks) are the oracle's float32 ranks of
    iteration t bit for bit, else a message naming the first differing vertex"""
    ids = np.asarray(ids, dtype=np.int64)
    got32 = np.asarray(ranks, dtype=np.float32)
    if ids.shape != (o.N,) or not np.array_equal(np.sort(ids), np.arange(o.N)):
        return "ids() is not a permutation of the %d vertices" % o.N
    got = np.empty(o.N, dtype=np.float32)
    got[ids] = got32
    want = o.want(t)
    if np.array_equal(got, want) and np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return None
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    v = int(bad[0])
    U = o.steps[t - 1][0]
    new = int(np.flatnonzero(ids == v)[0])
    return ("iteration %d: %d of %d ranks differ; first: global id %d, new id %d, in-degree %d, "
            "got %r, want %d (units of 2^-%d)" % (t, len(bad), o.N, v, new, int(o.indeg[v]),
                                                   float(np.ldexp(np.float64(got[v]), U)), int(o.steps[t - 1][1][v]), U))


def check_step(o, t, pr, what):
    ids, r = pr.ranks()
    bad = first_mismatch(o, t, ids.cpu().numpy(), r.cpu().numpy())
    assert bad is None, f"{what}: {bad}"
    got, want = pr.delta(), o.delta(t)
    assert got == want, f"{what}: iteration {t}: delta() = {got!r}, want {want!r}"


def check_counts(o, pr, what):
    assert pr.nedge == o.ne, f"{what}: nedge = {pr.nedge}, want {o.ne}"
    assert pr.ndangling == o.ndangling, f"{what}: ndangling = {pr.ndangling}, want {o.ndangling}"


class env_set:
    """the plan reads its switches when it is built: set, build, restore"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


PLAN_ENV = ("MRH_PR_XCD", "MRH_PR_L2_BYTES", "MRH_PR_XCD_LAYERS", "MRH_PR_BLOCKING", "MRH_PLAN_KERNEL",
            "MRH_PR_DEGREES", "MRH_PR_SRC_ORDER", "MRH_PR_GRAPH", "MRH_PR_DIST", "MRH_PR_OVERLAP", "MRH_PR_DIST_GRAPH")


def build_plan(edges, N, device, env, comm=None, alpha=ALPHA):
    """a PageRank plan of the edges (rank r of a several-rank communicator
    contributes every size-th edge) built under exactly the switches in env"""
    comm = comm or g.Comm(device=device)
    mr = g.MapReduce(comm)
    P = comm.size
    mr.map(P, lambda itask, kv: kv.add_tensors(torch.from_numpy(np.array(edges[itask::P])).to(comm.device)))
    full = {k: "" for k in PLAN_ENV if k in os.environ}  # an inherited switch must not change the route
    full.update(env)
    with env_set(full):
        for k in [k for k, v in full.items() if v == ""]:
            os.environ.pop(k, None)
        pr = PageRank(mr, N, alpha).build()
    return comm, pr


# ------------------------------------------------------------------ mirror of the dispatcher (graphplan.cpp)


def route(pr, comm, env):
    """the route a built plan takes, from its own attributes and the switches
    it was built under (PageRankPlan's constructor, build_device, step, run)"""
    if not comm.is_cuda:
        return "host"
    if pr.layout == "partials":
        return "rccl/partials"
    if pr.layout == "replicated":
        if not pr.overlapped:
            return "rccl/replicated"
        return "rccl/pieces/eager" if env.get("MRH_PR_DIST_GRAPH") == "0" else "rccl/pieces"
    if pr.blocking:
        return "blocking"
    if pr.xcd_ranges > 0:
        return "xcd"
    return "pull/tiles" if env.get("MRH_PLAN_KERNEL") == "tiles" else "pull/wave"


def expect_ranges(o, env):
    """xcd_ranges(): ranges exist iff the active vertices outnumber the cap"""
    if env.get("MRH_PR_XCD") == "0" or env.get("MRH_PR_BLOCKING") == "1":
        return False
    cap = max(4096, int(env.get("MRH_PR_L2_BYTES", 3 << 20))) // 4 * 85 // 100
    return o.N - o.ndangling > cap


def run_exact(name, device, env, want_route):
    """build the plan of a named graph, assert its route, and compare every
    iteration the oracle allows"""
    k, edges, o = graph(name)
    assert o.T >= TMIN[name], f"{name}: the exact budget ends after {o.T} iterations ({o.why})"
    comm, pr = build_plan(edges, o.N, device, env)
    what = f"{name} {want_route} {env}"
    got_route = route(pr, comm, env)
    assert got_route == want_route, f"{what}: this case no longer covers route {want_route}: the plan took {got_route}"
    if comm.is_cuda and pr.layout == "local":
        assert (pr.xcd_ranges > 0) == expect_ranges(o, env), f"{what}: xcd_ranges = {pr.xcd_ranges}"
        assert comm.native.transport == "local", what
    check_counts(o, pr, what)
    for t in range(1, o.T + 1):
        pr.step()
        check_step(o, t, pr, what)
    assert pr.graph_iterations == 0, what
    return o, pr


# ------------------------------------------------------------------ the generator and the budget (no GPU)


@pytest.mark.parametrize("name", list(GRAPHS) + list(DEGENERATE))
def test_budget(name):
    """the oracle's own budget assertions give every graph its iterations"""
    k, edges, o = graph(name)
    print(f"{name}: N = 2^{k}, {o.ne} edges, T = {o.T} ({o.why})")
    assert o.T >= TMIN[name], o.why
    assert edges.shape == (o.ne, 2) and (o.ne == 0 or (edges.min() >= 0 and edges.max() < o.N))
    for t in range(1, o.T + 1):
        U, r, d, dm = o.steps[t - 1]
        assert int(r.astype(object).sum()) <= 1 << U  # ranks never gain mass
        assert np.array_equal(np.ldexp(o.want(t).astype(np.float64), U), r.astype(np.float64))


def test_oracle_matches_float64_reference():
    """the integer iteration is the documented one: equal to the float64
    reference to its rounding"""
    for name in ("g11", "dang11", "n4", "twolive"):
        k, edges, o = graph(name)
        ref = reference_pagerank(np.asarray(edges), o.N, alpha=ALPHA, iters=o.T)
        np.testing.assert_allclose(o.want(o.T).astype(np.float64), ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_lattice_plants(name):
    spec = GRAPHS[name]
    k, edges, o = graph(name)
    N, m, j = o.N, spec["m"], spec.get("j", 3)
    new_of, indeg, start = pull_layout(edges, N)
    assert set(np.unique(o.outdeg)) == ({0} if j is not None else set()) | {1 << i for i in range(m + 1)}
    assert o.ndangling == (N >> j if j is not None else 0)
    dang_in = int(o.indeg[o.outdeg == 0].sum())
    assert (dang_in > 0) == bool(spec.get("dangling_in"))
    assert ((o.indeg == 0) & (o.outdeg > 0)).sum() >= N // 32
    assert (edges[:, 0] == edges[:, 1]).any()
    assert len(np.unique(edges, axis=0)) < o.ne  # multi-edges
    assert not np.array_equal(new_of, np.arange(N))
    end = start + indeg
    run = indeg > 0
    assert ((start[run] % WS_TILE == 0) & (start[run] > 0)).any()   # a run starting on a wave-tile boundary
    assert ((end[run] % WS_TILE == 0) & (end[run] < o.ne)).any()    # and one ending on one
    h = int(indeg.argmax())
    assert indeg[h] == spec.get("hub", 3 * WS_TILE + 100) and start[h] % WS_TILE != 0
    tiles = (end[h] - 1) // WS_TILE - start[h] // WS_TILE + 1
    assert tiles >= 4
    if name == "big":
        # > 32 wave tiles; the tiles kernel folds its carries in levels (more
        # than 64 entries) and the hub's cross a 64-entry wave of level 1
        assert tiles > 32 and 2 * -(-o.ne // SR_TILE) > 64
        assert start[h] // SR_TILE < 32 <= (end[h] - 1) // SR_TILE
    if name in ("blk", "slices"):
        per_bin = np.bincount(new_of[edges[:, 1]] // PB_BIN, minlength=2)
        assert N == 2 * PB_BIN and per_bin.min() > 0
        assert (per_bin.max() > PB_SLICE) == (name == "slices")


# ------------------------------------------------------------------ case 1: the CPU engine


@pytest.mark.parametrize("name", ["g11", "g13", "dang11", "nodangling", "n2", "n4", "twolive"])
def test_exact_host(name):
    run_exact(name, "cpu", {}, "host")


def case_exact(comm):
    """one rank of a gloo world (tests/test_distributed_cpu.py run_world)"""
    out = {}
    for name in ("g11", "g13"):
        k, edges, o = graph(name)
        _, pr = build_plan(edges, o.N, "cpu", {}, comm=comm)
        steps = []
        for t in range(1, o.T + 1):
            pr.step()
            ids, r = pr.ranks()
            steps.append((ids.cpu().numpy().copy(), r.cpu().numpy().copy(), pr.delta()))
        out[name] = (pr.layout, pr.nedge, pr.ndangling, pr.nlocal, steps)
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_exact_host_ranks(world):
    """2 and 3 gloo ranks (source-owned edges, all-to-all of partial sums,
    allreduced stats); with 3 ranks nlocal is no multiple of 4"""
    from test_distributed_cpu import run_world
    out = run_world("test_pagerank_exact:case_exact", world)
    for name in ("g11", "g13"):
        k, edges, o = graph(name)
        assert o.T >= TMIN[name], o.why
        res = [out[r][name] for r in range(world)]
        assert all(x[0] == "partials" for x in res)
        assert sum(x[1] for x in res) == o.ne and all(x[2] == o.ndangling for x in res)
        assert [x[3] for x in res] == [(o.N - r + world - 1) // world for r in range(world)]
        if world == 3:
            assert any(x[3] % 4 for x in res)
        for t in range(1, o.T + 1):
            ids = np.concatenate([x[4][t - 1][0] for x in res])
            ranks = np.concatenate([x[4][t - 1][1] for x in res])
            bad = first_mismatch(o, t, ids, ranks)
            assert bad is None, f"{name} world {world}: {bad}"
            for x in res:
                assert x[4][t - 1][2] == o.delta(t), f"{name} world {world}: iteration {t}: delta {x[4][t - 1][2]!r}"


# ------------------------------------------------------------------ cases 2, 7, 8: the pull routes

PULL = {"MRH_PR_XCD": "0"}
TILES = {"MRH_PR_XCD": "0", "MRH_PLAN_KERNEL": "tiles"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g11", "g13", "big", "dang11", "nodangling", "n2", "n4", "twolive"])
def test_exact_pull_wave(name):
    run_exact(name, "cuda", PULL, "pull/wave")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g11", "big", "n4"])
def test_exact_pull_tiles(name):
    run_exact(name, "cuda", TILES, "pull/tiles")


@pytest.mark.gpu
@pytest.mark.parametrize("var", [{"MRH_PR_DEGREES": "partition"}, {"MRH_PR_DEGREES": "sort"}, {"MRH_PR_SRC_ORDER": "1"}],
                         ids=["partition", "sort", "src_order"])
def test_exact_pull_build_variants(var):
    run_exact("g13", "cuda", dict(PULL, **var), "pull/wave")


# ------------------------------------------------------------------ cases 3, 7: XCD ranges and the fused tile step

XCD = {"MRH_PR_L2_BYTES": L2_SMALL}
XCD1 = {"MRH_PR_L2_BYTES": L2_SMALL, "MRH_PR_XCD_LAYERS": "1"}


@pytest.mark.gpu
@pytest.mark.parametrize("layers", ["layer1", "layers"])
@pytest.mark.parametrize("name", ["x11", "g13", "dang13"])
def test_exact_xcd(name, layers):
    k, edges, o = graph(name)
    if name == "x11":
        assert o.N < PR_TILE                                 # the scalar tail path of k_pr_tile_step (nd < TILE)
    else:
        assert o.N == 2 * PR_TILE                            # two full tiles: the float4 path
    o, pr = run_exact(name, "cuda", XCD1 if layers == "layer1" else XCD, "xcd")
    assert o.N - o.ndangling > XCD_CAP
    if layers == "layer1":
        assert pr.xcd_ranges == 9                            # 8 hot ranges and the cold one
    else:
        assert pr.xcd_ranges > 9 and (pr.xcd_ranges - 1) % 8 == 0, pr.xcd_ranges


# ------------------------------------------------------------------ case 4: HIP-graph replay


@pytest.mark.gpu
def test_exact_xcd_graph_replay():
    """run(T) by graph replay and by plain launches, even and odd T, and again
    after reset(): each equals the oracle, not merely the other"""
    k, edges, o = graph("g13")
    assert o.T >= 3, o.why
    comm, pr = build_plan(edges, o.N, "cuda", XCD)
    assert route(pr, comm, XCD) == "xcd" and pr.xcd_ranges > 0
    check_counts(o, pr, "graph replay")
    for iters in (2, 3):
        pr.use_graph = False
        before = pr.graph_iterations
        pr.reset()
        assert pr.run(iters) == iters
        check_step(o, iters, pr, f"plain run({iters})")
        assert pr.graph_iterations == before
        pr.use_graph = True
        for again in range(2):
            pr.reset()
            assert pr.run(iters) == iters
            check_step(o, iters, pr, f"graph run({iters}) #{again}")
        assert pr.graph_iterations - before == 2 * 2 * (iters // 2)


# ------------------------------------------------------------------ case 5: propagation blocking

BLOCKING = {"MRH_PR_BLOCKING": "1"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blk", "slices"])
def test_exact_blocking(name):
    """two destination bins of 2^14 with destinations in both; in `slices` the
    hub bin holds more than 2^18 edges and is cut into several work units
    (test_lattice_plants asserts both from the mirrored layout)"""
    run_exact(name, "cuda", BLOCKING, "blocking")


# ------------------------------------------------------------------ case 6: forced one-rank RCCL plans

FORCED = [
    ("rccl/replicated", {"MRH_FORCE_RCCL": "1"}),
    ("rccl/pieces", {"MRH_FORCE_RCCL": "1", "MRH_PR_OVERLAP": "2"}),
    ("rccl/pieces/eager", {"MRH_FORCE_RCCL": "1", "MRH_PR_OVERLAP": "2", "MRH_PR_DIST_GRAPH": "0"}),
    ("rccl/partials", {"MRH_FORCE_RCCL": "1", "MRH_PR_DIST": "partials"}),
]


def _forced_child(out_path):
    """body of a forced-RCCL child: every iteration's ranks by step(), then
    twice reset() and run(T) (the pieces plan replays a graph from its second run)"""
    k, edges, o = graph("g13")
    env = {name: os.environ[name] for name in PLAN_ENV if name in os.environ}
    comm, pr = build_plan(edges, o.N, "cuda", env)
    res = {"route": route(pr, comm, env), "layout": pr.layout, "xcd_ranges": int(pr.xcd_ranges),
           "transport": comm.native.transport, "nedge": int(pr.nedge), "ndangling": int(pr.ndangling), "delta": []}
    arrays = {}
    for t in range(1, o.T + 1):
        pr.step()
        ids, r = pr.ranks()
        arrays[f"ids{t}"], arrays[f"r{t}"] = ids.cpu().numpy(), r.cpu().numpy()
        res["delta"].append(pr.delta())
    res["graph"] = [int(pr.graph_iterations)]
    res["delta_run"] = []
    for n in (1, 2):
        pr.reset()
        pr.run(o.T)
        ids, r = pr.ranks()
        arrays[f"ids_run{n}"], arrays[f"r_run{n}"] = ids.cpu().numpy(), r.cpu().numpy()
        res["delta_run"].append(pr.delta())
        res["graph"].append(int(pr.graph_iterations))
    np.savez(out_path, **arrays)
    print(json.dumps(res), flush=True)
    return 0


@pytest.mark.gpu
def test_exact_forced_rccl(tmp_path):
    """MRH_FORCE_RCCL and the communicator are fixed at start-up: one fresh
    child per plan, one at a time, none after a failed one"""
    k, edges, o = graph("g13")
    assert o.T >= TMIN["g13"], o.why
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_pagerank_exact as t; sys.exit(t._forced_child(sys.argv[1]))"
            % (os.path.dirname(here), here))
    flags = ["-s"] if sys.flags.no_user_site else []
    for want_route, extra in FORCED:
        env = {k: v for k, v in os.environ.items()
               if k not in PLAN_ENV and k not in ("MRH_FORCE_RCCL", "WORLD_SIZE", "RANK", "LOCAL_RANK")}
        env.update(extra, MRH_PR_L2_BYTES=L2_SMALL)
        path = str(tmp_path / (want_route.replace("/", "_") + ".npz"))
        p = subprocess.run([sys.executable, *flags, "-c", code, path], env=env, timeout=120, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, f"{want_route}: child exit status {p.returncode}\n{p.stderr[-3000:]}"
        res = json.loads(p.stdout.strip().splitlines()[-1])
        z = np.load(path)
        assert res["route"] == want_route, f"this case no longer covers route {want_route}: {res}"
        assert res["transport"] == "rccl", res
        assert (res["xcd_ranges"] > 0) == (want_route != "rccl/partials"), res
        assert (res["nedge"], res["ndangling"]) == (o.ne, o.ndangling), res
        for t in range(1, o.T + 1):
            bad = first_mismatch(o, t, z[f"ids{t}"], z[f"r{t}"])
            assert bad is None, f"{want_route}: {bad}"
            assert res["delta"][t - 1] == o.delta(t), f"{want_route}: iteration {t}: delta {res['delta'][t - 1]!r}"
        for n in (1, 2):
            bad = first_mismatch(o, o.T, z[f"ids_run{n}"], z[f"r_run{n}"])
            assert bad is None, f"{want_route} run({o.T}) #{n} after reset(): {bad}"
            assert res["delta_run"][n - 1] == o.delta(o.T), (want_route, res["delta_run"])
        # run() of the pieces plan: the first one stays eager (two iterations
        # to make RCCL's connections, fewer than two left); later ones step once
        # on the fresh c, then replay pairs
        replayed = 2 * ((o.T - 1) // 2) if want_route == "rccl/pieces" else 0
        assert res["graph"] == [0, 0, replayed], (want_route, res)


# ------------------------------------------------------------------ the tails the exact regime cannot reach

TAIL_N = 2 * PR_TILE + 7


def tail_graph():
    """random out-degrees 0..8 (an eighth of the vertices dangling), uniform
    destinations and one hub"""
    rng = np.random.default_rng(77)
    deg = rng.integers(1, 9, TAIL_N)
    deg[rng.permutation(TAIL_N)[:TAIL_N // 8]] = 0
    vi = np.repeat(np.arange(TAIL_N, dtype=np.int64), deg)
    vj = rng.integers(0, TAIL_N, len(vi))
    vj[rng.permutation(len(vi))[:3000]] = 4242
    return np.stack([vi, vj], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("want_route,env", [("pull/wave", PULL), ("xcd", XCD)], ids=["pull", "xcd"])
def test_tails_one_step(want_route, env):
    """N = 2 * 4096 + 7: the scalar tail of k_pr_update (n % 4 = 3) and a
    partial last tile of k_pr_tile_step after two full ones; one step() from
    reset() against the float64 reference, alpha = 0.85, then a second one.

    Bound: |got_j - ref_j| <= (indeg_j + 16) 2^-24 ref_j. All terms are
    non-negative, so to first order the relative error of r'_j is at most the
    number of float32 roundings on the way to it, each at most 2^-24: 1/N,
    1/outdeg, their product c (3), indeg_j - 1 additions of the gather (the
    fixed-point adds of the tile step are exact), dterm, a + dterm, the
    multiplication by alpha and the final addition of base (4): indeg_j + 6,
    plus one for the float32 alpha and base constants. 16 leaves room for the
    second-order terms.

    A second step checks what one step cannot show: the dangling mass the
    first step accumulated (the dangling flags are bytes unpacked from one
    uint32 per four vertices, and here, unlike with N = 2^k, the first
    dangling new id is no multiple of 4). Its terms c_i and dterm carry the
    first step's relative errors, at most E_j = max(indeg_i + 16) 2^-24 over
    j's in-neighbours i and the dangling vertices; a sum of non-negative terms
    keeps the largest relative error of its terms, and the second step adds
    its own indeg_j + 6 roundings (1/outdeg and the product for c, the
    additions, dterm, a + dterm, alpha, base):
    |got_j - ref_j| <= (E_j + indeg_j + 16) 2^-24 ref_j."""
    edges = tail_graph()
    comm, pr = build_plan(edges, TAIL_N, "cuda", env, alpha=0.85)
    assert route(pr, comm, env) == want_route
    assert TAIL_N % 4 == 3 and TAIL_N % PR_TILE == 7 and TAIL_N // PR_TILE == 2
    pr.reset()
    pr.step()
    ids, r = pr.ranks()
    got = np.empty(TAIL_N)
    got[ids.cpu().numpy()] = r.cpu().numpy().astype(np.float64)
    ref = reference_pagerank(edges, TAIL_N, alpha=0.85, iters=1)
    indeg = np.bincount(edges[:, 1], minlength=TAIL_N)
    bound = (indeg + 16) * 2.0 ** -24 * ref
    err = np.abs(got - ref)
    worst = int(np.argmax(err / bound))
    print(f"{want_route}: worst error / bound = {err[worst] / bound[worst]:.3f} at vertex {worst} (in-degree {indeg[worst]})")
    assert np.all(err <= bound), f"{int((err > bound).sum())} vertices past the bound; worst {worst}"
    assert abs(pr.delta() - np.abs(ref - 1.0 / TAIL_N).sum()) <= 1e-5
    outdeg = np.bincount(edges[:, 0], minlength=TAIL_N)
    first_dangling = int((outdeg > 0).sum())
    assert first_dangling % 4 == 3 and first_dangling > PR_TILE
    pr.step()
    ids, r = pr.ranks()
    got[ids.cpu().numpy()] = r.cpu().numpy().astype(np.float64)
    ref2 = reference_pagerank(edges, TAIL_N, alpha=0.85, iters=2)
    e1 = (indeg + 16).astype(np.float64)
    E = np.full(TAIL_N, e1[outdeg == 0].max())
    np.maximum.at(E, edges[:, 1], e1[edges[:, 0]])
    bound2 = (E + indeg + 16) * 2.0 ** -24 * ref2
    err2 = np.abs(got - ref2)
    worst = int(np.argmax(err2 / bound2))
    print(f"{want_route}: second step: worst error / bound = {err2[worst] / bound2[worst]:.3f} at vertex {worst}")
    assert np.all(err2 <= bound2), f"second step: {int((err2 > bound2).sum())} vertices past the bound; worst {worst}"
