"""pagerank_mr: PageRank as an iterated MapReduce on the generic engine
(csrc/oink/commands.cpp PageRankMR), its scatter / update compress callbacks
as device kernels (csrc/kernels/prmr.hip) on cuda and host twins on cpu.

Oracle: the float64 numpy iteration of models/pagerank.py. Tolerances:
  * files are printed with "%g" (6 significant digits), so a printed rank is
    within 5e-6 relative of the computed one: rtol 1e-5, atol 0 (every rank is
    >= (1 - alpha) / N > 0);
  * against the float32 `pagerank` plan: tests/test_pagerank.py's rtol 2e-4,
    atol 1e-9;
  * op level, float64: sums of m positive terms in any order differ by at most
    m * 2^-53 relative (under 2e-12 for groups of <= 2^14 values): rtol 1e-11
    between device, host twin and numpy; two runs of the device op on the same
    input are bitwise equal."""
import io
import os
import re

import numpy as np
import pytest

from gpu_mapreduce_amd.models.pagerank import reference_pagerank
from gpu_mapreduce_amd.oink.interp import OINK

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
FILE_TOL = dict(rtol=1e-5, atol=0.0)
PLAN_TOL = dict(rtol=2e-4, atol=1e-9)
OP_TOL = dict(rtol=1e-11, atol=0.0)
MSG = r"PageRank_MR: (\d+) vertices, (\d+) iterations, L1 delta (\S+)"


def run(script, tmp_path, monkeypatch, comm=None):
    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    o = OINK(comm, screen=out, logfile="log.oink")
    o.file(text=script)
    return out.getvalue()


def comm_for(dev):
    if dev == "cpu":
        return None
    from gpu_mapreduce_amd.parallel.comm import Comm
    return Comm(device=dev)


def rmat_script(scale, seed=12345, tol="0.0", maxiter=15, plan=True):
    s = (f"rmat {scale} 8 0.57 0.19 0.19 0.05 0.0 {seed} -o tmp.rmat mre\n"
         f"pagerank_mr {tol} {maxiter} 0.85 -i mre -o tmp.prmr NULL\n")
    return s + (f"pagerank {tol} {maxiter} 0.85 -i mre -o tmp.pr NULL\n" if plan else "")


def load_ranks(path, n):
    """ranks of a (vertex, rank) file: exactly n lines, every id in [0, n) once"""
    rows = np.loadtxt(path, ndmin=2)
    ids = rows[:, 0].astype(np.int64)
    assert len(ids) == n and np.array_equal(np.sort(ids), np.arange(n))
    r = np.zeros(n)
    r[ids] = rows[:, 1]
    return r


def check_command(tmp_path, text, edges, iters):
    n = int(edges.max()) + 1
    ref = reference_pagerank(edges, n, 0.85, iters)
    got = load_ranks(tmp_path / "tmp.prmr.0", n)
    plan = load_ranks(tmp_path / "tmp.pr.0", n)
    rel = np.abs(got / ref - 1).max()
    print(f"pagerank_mr vs oracle: max rel {rel:.3e}; vs plan: max rel {np.abs(got / plan - 1).max():.3e}; "
          f"sum {got.sum():.9f}")
    np.testing.assert_allclose(got, ref, **FILE_TOL)
    np.testing.assert_allclose(got, plan, **PLAN_TOL)
    m = re.search(MSG, text)
    assert m and int(m.group(1)) == n and int(m.group(2)) == iters
    assert abs(got.sum() - 1.0) < 1e-4


@pytest.mark.parametrize("dev", DEVS)
def test_pagerank_mr_matches_oracle(tmp_path, monkeypatch, dev):
    scale = 8 if dev == "cpu" else 12
    text = run(rmat_script(scale), tmp_path, monkeypatch, comm_for(dev))
    e = np.loadtxt(tmp_path / "tmp.rmat.0", dtype=np.int64, ndmin=2)
    check_command(tmp_path, text, e, 15)


def kernel_breaker_edges():
    """the shapes that break kernels, in one graph (ids below 30 000):
      * vertex 1: 9 001 in-edges from distinct sources 10 000.. (its update
        segment spans three 4 096-value segred tiles);
      * vertex 2: 9 001 out-edges to 20 000.. (its scatter group spans several
        256-thread blocks);
      * 3 -> 4 three times (duplicates count in the out-degree);
      * a self loop 5 -> 5; a chain 6 -> 7 -> 8 -> 9;
      * vertex 9 (and 20 000..29 000): in-edges only;
      * ids 0, 11..9 999 and 19 001..19 999 appear in no edge: lone RANKs in
        both joins;
      * 18 011 edges + 29 001 ranks = 47 012 scatter values, 18 011
        contributions + 29 001 ranks in update: neither a multiple of 64."""
    e = [(10000 + i, 1) for i in range(9001)] + [(2, 20000 + i) for i in range(9001)]
    e += [(3, 4)] * 3 + [(5, 5)] + [(6, 7), (7, 8), (8, 9)] + [(1, 2), (4, 6)]
    e = np.array(e, dtype=np.int64)
    assert (len(e) + int(e.max()) + 1) % 64 != 0
    return e


@pytest.mark.parametrize("dev", DEVS)
def test_pagerank_mr_kernel_breaking_shapes(tmp_path, monkeypatch, dev):
    e = kernel_breaker_edges()
    rng = np.random.default_rng(3)
    with open(tmp_path / "graph.e", "w") as f:
        for x, y in e[rng.permutation(len(e))]:
            f.write(f"{x} {y}\n")
    s = ("pagerank_mr 0.0 15 0.85 -i graph.e -o tmp.prmr NULL\n"
         "pagerank 0.0 15 0.85 -i graph.e -o tmp.pr NULL\n")
    text = run(s, tmp_path, monkeypatch, comm_for(dev))
    check_command(tmp_path, text, e, 15)


def test_pagerank_mr_stopping_rule(tmp_path, monkeypatch):
    """tol 1e-3: the reported count is the first k at which the oracle's L1 step
    is below tol. With rmat seed 12345 the oracle's steps around that k are
    1.32e-3 (k - 1) and 3.35e-4 (k): both more than 1 % away from tol, so
    float64 rounding cannot move the stop (asserted below)."""
    tol, maxiter = 1e-3, 100
    text = run(rmat_script(8, tol="1.0e-3", maxiter=maxiter, plan=False), tmp_path, monkeypatch)
    e = np.loadtxt(tmp_path / "tmp.rmat.0", dtype=np.int64, ndmin=2)
    n = int(e.max()) + 1
    prev, steps = reference_pagerank(e, n, 0.85, 0), []
    for k in range(1, maxiter + 1):
        cur = reference_pagerank(e, n, 0.85, k)
        steps.append(np.abs(cur - prev).sum())
        prev = cur
        if steps[-1] < tol:
            break
    k = len(steps)
    print(f"oracle L1 steps around the stop: k-1 {steps[-2]:.6e}, k {steps[-1]:.6e}")
    assert 1 < k < maxiter and steps[-1] < tol * 0.99 and steps[-2] > tol * 1.01
    m = re.search(MSG, text)
    assert m and int(m.group(2)) == k
    assert float(m.group(3)) == pytest.approx(steps[-1], rel=1e-4)
    np.testing.assert_allclose(load_ranks(tmp_path / "tmp.prmr.0", n), prev, **FILE_TOL)


# ---------------------------------------------------------------- ops on hand-built groups

def f2i(x):
    return int(np.float64(x).view(np.int64))


def edgew(vj, w):
    return np.array([vj, f2i(w)], dtype=np.int64).tobytes()


def contrib(x):
    return np.array([f2i(x)], dtype=np.int64).tobytes()


def rank(r):
    return np.array([f2i(r), 0, 0], dtype=np.int64).tobytes()


def groups_kmv(dev, recs, fn):
    """the local groups of (key, value bytes) records as a KMV handed to fn"""
    import torch
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    mr = MapReduce(comm_for(dev))

    def m(itask, kv):
        if not recs:
            return
        keys = torch.tensor([k for k, _ in recs], dtype=torch.int64)
        lens = [len(v) for _, v in recs]
        voff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
        vals = torch.frombuffer(bytearray(b"".join(v for _, v in recs)), dtype=torch.uint8)
        if len(set(lens)) == 1:
            kv.add_tensors(keys.to(kv.device), vals.view(len(recs), lens[0]).to(kv.device))
        else:
            kv.add_tensors(keys.to(kv.device), vals.to(kv.device), voff=voff.to(kv.device))
    mr.map(1, m)
    out = []
    mr.compress_batch(lambda kmv, kv: out.append(fn(kmv)))
    if not recs and not out:  # no groups, no piece, no call: the op on a KMV that holds nothing
        from gpu_mapreduce_amd import C
        out.append(fn(C.KMV()))
    assert len(out) == 1
    return out[0]


def scatter_case():
    """key 10: lone RANK (dangling); 11: RANK + 1 edge; 12: RANK first + 70
    edges (crosses the 64-lane boundary); 13: RANK last; 14: RANK in the
    middle; 15: lone RANK"""
    rng = np.random.default_rng(11)
    r = {k: float(rng.uniform(0.01, 1.0)) for k in range(10, 16)}
    recs, edges = [(10, rank(r[10]))], []

    def add_edges(key, n):
        for _ in range(n):
            vj, w = int(rng.integers(0, 1000)), float(rng.uniform(0.001, 1.0))
            recs.append((key, edgew(vj, w)))
            edges.append((key, vj, w))
    recs.append((11, rank(r[11])))
    add_edges(11, 1)
    recs.append((12, rank(r[12])))
    add_edges(12, 70)
    add_edges(13, 5)
    recs.append((13, rank(r[13])))
    add_edges(14, 3)
    recs.append((14, rank(r[14])))
    add_edges(14, 4)
    recs.append((15, rank(r[15])))
    return recs, edges, r, r[10] + r[15]


def scatter_np(out):
    import torch
    ek, ed, ck, cc, dang = out
    return (ek.cpu().numpy(), ed.cpu().numpy(), ck.cpu().numpy(),
            cc.cpu().contiguous().view(torch.float64).numpy(), float(dang))


@pytest.mark.parametrize("dev", DEVS)
def test_prmr_scatter_groups(dev):
    from gpu_mapreduce_amd import C
    recs, edges, r, dang = scatter_case()
    ek, ed, ck, cc, got_dang = scatter_np(groups_kmv(dev, recs, C.prmr_scatter))
    want = sorted((k, vj, f2i(w), f2i(w * r[k])) for k, vj, w in edges)
    # contrib = w * r is one float64 product: exact on both devices
    assert sorted(zip(ek.tolist(), ed[:, 0].tolist(), ed[:, 1].tolist(), cc.view(np.int64).tolist())) == want
    assert np.array_equal(ck, ed[:, 0])
    np.testing.assert_allclose(got_dang, dang, **OP_TOL)
    if dev == "cuda":
        host = scatter_np(groups_kmv("cpu", recs, C.prmr_scatter))
        for a, b in zip((ek, ed, ck), host[:3]):  # both emit in value order
            assert np.array_equal(a, b)
        np.testing.assert_allclose(cc, host[3], **OP_TOL)
        np.testing.assert_allclose(got_dang, host[4], **OP_TOL)
        again = scatter_np(groups_kmv(dev, recs, C.prmr_scatter))
        assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip((ek, ed, ck, cc), again[:4]))
        assert np.float64(got_dang).tobytes() == np.float64(again[4]).tobytes()


def update_case():
    """key 20: lone RANK; 21: RANK + 1 contribution; 22: RANK in the middle of
    5 000 contributions (two segred tiles)"""
    rng = np.random.default_rng(12)
    r = {k: float(rng.uniform(0.01, 1.0)) for k in (20, 21, 22)}
    c = {20: np.zeros(0), 21: rng.uniform(0.0, 1.0, 1), 22: rng.uniform(0.0, 1e-3, 5000)}
    recs = [(20, rank(r[20])), (21, contrib(c[21][0])), (21, rank(r[21]))]
    recs += [(22, contrib(x)) for x in c[22][:2500]] + [(22, rank(r[22]))] + [(22, contrib(x)) for x in c[22][2500:]]
    return recs, r, c


def update_np(out):
    import torch
    ranks, delta = out
    t = ranks.cpu().contiguous()
    assert tuple(t.shape[1:]) == (3,) and not t[:, 1:].any()
    return t[:, 0].contiguous().view(torch.float64).numpy(), float(delta)


@pytest.mark.parametrize("dev", DEVS)
def test_prmr_update_groups(dev):
    from gpu_mapreduce_amd import C
    recs, r, c = update_case()
    base, alpha, dterm = 0.15 / 3, 0.85, 0.0123
    keys = []

    def op(kmv):
        import torch
        keys[:] = kmv.keys.kdata.view(torch.int64).tolist()
        return C.prmr_update(kmv, base, alpha, dterm)
    got, delta = update_np(groups_kmv(dev, recs, op))
    want = np.array([base + alpha * (c[k].sum() + dterm) for k in keys])
    np.testing.assert_allclose(got, want, **OP_TOL)
    np.testing.assert_allclose(delta, sum(abs(w - r[k]) for w, k in zip(want, keys)), **OP_TOL)
    if dev == "cuda":
        host, hdelta = update_np(groups_kmv("cpu", recs, op))
        np.testing.assert_allclose(got, host, **OP_TOL)
        np.testing.assert_allclose(delta, hdelta, **OP_TOL)
        again, adelta = update_np(groups_kmv(dev, recs, op))
        assert np.array_equal(got.view(np.int64), again.view(np.int64))
        assert np.float64(delta).tobytes() == np.float64(adelta).tobytes()


@pytest.mark.parametrize("dev", DEVS)
def test_prmr_ops_contract(dev):
    """no RANK / two RANKs raise on both ops; an empty KMV returns empties"""
    from gpu_mapreduce_amd import C
    upd = lambda kmv: C.prmr_update(kmv, 0.05, 0.85, 0.0)  # noqa: E731
    ok = [(1, rank(0.5)), (1, edgew(2, 0.5))]
    for bad in ([(3, edgew(4, 1.0))], [(3, rank(0.1)), (3, rank(0.2))],
                ok + [(3, edgew(4, 0.5)), (3, edgew(5, 0.5))], ok + [(3, rank(0.1)), (3, edgew(1, 1.0)), (3, rank(0.2))]):
        with pytest.raises(Exception, match="one RANK per vertex"):
            groups_kmv(dev, bad, C.prmr_scatter)
    oku = [(1, rank(0.5)), (1, contrib(0.25))]
    for bad in ([(3, contrib(0.5))], [(3, rank(0.1)), (3, rank(0.2))],
                oku + [(3, contrib(0.5)), (3, contrib(0.25))], oku + [(3, rank(0.1)), (3, contrib(1.0)), (3, rank(0.2))]):
        with pytest.raises(Exception, match="one RANK per vertex"):
            groups_kmv(dev, bad, upd)
    ek, ed, ck, cc, dang = groups_kmv(dev, [], C.prmr_scatter)
    assert ek.numel() == ed.numel() == ck.numel() == cc.numel() == 0 and dang == 0.0
    ranks, delta = groups_kmv(dev, [], upd)
    assert ranks.numel() == 0 and delta == 0.0


# ---------------------------------------------------------------- two ranks

def case_prmr(comm):
    os.chdir(os.environ["OINK_TEST_DIR"])
    out = io.StringIO()
    OINK(comm, screen=out, logfile="none").file(text=rmat_script(8))
    return out.getvalue()


def test_pagerank_mr_two_ranks(tmp_path, monkeypatch):
    """1 rank against 2 (gloo): the combiner, the all-rank dangling mass and
    the all-rank delta"""
    from test_distributed_cpu import _oink_files, run_world
    d1, d2 = tmp_path / "p1", tmp_path / "p2"
    d1.mkdir()
    d2.mkdir()
    text1 = run(rmat_script(8), d1, monkeypatch)
    monkeypatch.setenv("OINK_TEST_DIR", str(d2))
    text2 = run_world("test_pagerank_mr:case_prmr", 2)[0]
    assert _oink_files(d1, "tmp.rmat") == _oink_files(d2, "tmp.rmat")
    p1 = dict(ln.split() for ln in _oink_files(d1, "tmp.prmr"))
    p2 = dict(ln.split() for ln in _oink_files(d2, "tmp.prmr"))
    assert p1.keys() == p2.keys() and len(p1) == len(_oink_files(d2, "tmp.prmr"))
    ids = sorted(p1)
    np.testing.assert_allclose([float(p2[i]) for i in ids], [float(p1[i]) for i in ids], **FILE_TOL)
    m1, m2 = re.search(MSG, text1), re.search(MSG, text2)
    assert m1 and m2 and m1.group(1, 2) == m2.group(1, 2) and int(m1.group(2)) == 15


# ---------------------------------------------------------------- out of core

@pytest.mark.gpu
def test_pagerank_mr_out_of_core(tmp_path, monkeypatch):
    """under a 128 KiB HBM budget (8 pages of 16 KiB) the appends, both joins
    and the aggregates go through the out-of-core paths and the callbacks run
    once per piece (the dangling mass and the delta accumulate); a hub-free
    graph, so no group exceeds a page"""
    n, m = 3000, 12000
    rng = np.random.default_rng(7)
    e = np.unique(rng.integers(0, n, size=(4 * m, 2)), axis=0)
    e = e[rng.permutation(len(e))[:m]]
    assert len(e) == m
    with open(tmp_path / "graph.e", "w") as f:
        for x, y in e:
            f.write(f"{x} {y}\n")
    s = ("set memsize -16384 maxpage 8\n"
         "pagerank_mr 0.0 10 0.85 -i graph.e -o tmp.prmr NULL\n")
    text = run(s, tmp_path, monkeypatch, comm_for("cuda"))
    nv = int(e.max()) + 1
    got = load_ranks(tmp_path / "tmp.prmr.0", nv)
    np.testing.assert_allclose(got, reference_pagerank(e, nv, 0.85, 10), **FILE_TOL)
    m_ = re.search(MSG, text)
    assert m_ and int(m_.group(1)) == nv and int(m_.group(2)) == 10
