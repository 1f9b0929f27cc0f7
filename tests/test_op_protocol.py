"""The protocol every MapReduce op follows (csrc/engine/mapreduce.cpp, the op
frame): the name it reports to MRH_TRACE and to the fault points, its screen
lines, and the global count it returns. MRH_TRACE and MRH_FAULT are read once
per process, so every job runs in a child process (as test_faults.py does)."""
import json
import re

import pytest

from test_distributed_cpu import run_world
from test_faults import _py

# ~200 pairs over 17 keys, every public op that runs on the CPU engine once.
# call(name, count) records the returned counts in call order.
CPU_JOB = """
import json, os, struct, sys
import torch
import gpu_mapreduce_amd as g
tmp = os.environ["OP_PROTOCOL_TMP"]
comm = g.Comm(device="cpu")
counts = []
def call(name, n):
    counts.append([name, None if n is None else int(n)])
def fresh():
    mr = g.MapReduce(comm)
    mr.verbosity = 1
    mr.timer = 1
    return mr
PAIRS = [(struct.pack("<i", i % 17), struct.pack("<i", i)) for i in range(200)]
def fill(i, kv):
    for k, v in PAIRS[i::2]:
        kv.add(k, v)
def count_values(k, vals, kv):
    kv.add(k, struct.pack("<i", len(vals)))
def first_of_each(kmv, kv):
    kv.add_tensors(kmv.keys.kdata.view(torch.int32), kmv.seg[:-1].clone())
def compare(a, b):
    return (a > b) - (a < b)
with open(os.path.join(tmp, "two_lines.txt"), "w") as f:
    f.write("alpha\\nbeta\\n")
def lines(i, name, kv):
    for ln in open(name).read().split():
        kv.add(ln.encode(), None)

a, b, c = fresh(), fresh(), fresh()
call("map", a.map(2, fill))
call("map_mr", b.map_mr(a, lambda i, k, v, kv: kv.add(k, v)))
call("map_mr_batch", c.map_mr_batch(a, lambda src, kv: kv.add_kv(src)))
call("map_file", c.map_file([os.path.join(tmp, "two_lines.txt")], 0, 0, 0, lines))
call("add", b.add(a))
c.open()
c.kv_open.add(struct.pack("<i", 99), struct.pack("<i", 99))
call("close", c.close())
call("aggregate", a.aggregate())
call("aggregate_dest", a.aggregate_dest(torch.zeros(200, dtype=torch.int32)))
call("broadcast", a.broadcast(0))
call("gather", a.gather(1))
call("convert", a.convert())
call("scan_kmv", a.scan_kmv(lambda k, vals: None))
call("kmv_stats", a.kmv_stats(1))
call("sort_multivalues", a.sort_multivalues(1))
call("sort_multivalues_fn", a.sort_multivalues(compare))
call("reduce", a.reduce(count_values))
call("collate", b.collate())
call("reduce_sum", b.reduce("sum"))
call("map_addflag", c.map(2, fill, addflag=1))
call("clone", c.clone())
call("reduce_batch", c.reduce_batch(first_of_each))
call("collapse", c.collapse(b"all"))
call("reduce_count", c.reduce("count"))
call("map_again", c.map(2, fill))
call("scrunch", c.scrunch(1, b"all"))
call("map_b", b.map(2, fill))
call("compress", b.compress(count_values))
call("map_b2", b.map(2, fill))
call("compress_builtin", b.compress("sum"))
call("map_b3", b.map(2, fill))
call("compress_batch", b.compress_batch(first_of_each))
call("scan_kv", b.scan_kv(lambda k, v: None))
call("sort_keys", b.sort_keys(-1))
call("sort_keys_fn", b.sort_keys(compare))
call("sort_values", b.sort_values(1))
call("sort_values_fn", b.sort_values(compare))
call("kv_stats", b.kv_stats(1))
b.save(os.path.join(tmp, "b.ckpt"))
call("load", c.load(os.path.join(tmp, "b.ckpt")))
c.spill()
c.unspill()
call("sort_keys_after_unspill", c.sort_keys(1))
json.dump(counts, open(os.path.join(tmp, "counts.json"), "w"))
"""

CPU_TRACE = [("map", 0), ("map_mr", 0), ("map_mr_batch", 0), ("map_file", 0), ("add", 0), ("aggregate", 0), ("aggregate_dest", 0),
 ("broadcast", 0), ("gather", 0), ("convert", 0), ("scan_kmv", 0), ("sort_multivalues", 0), ("sort_multivalues", 0),
 ("reduce", 0), ("aggregate", 1), ("convert", 1), ("collate", 0), ("reduce_builtin", 0), ("map", 0), ("clone", 0),
 ("reduce_batch", 0), ("collapse", 0), ("reduce_builtin", 0), ("map", 0), ("gather", 1), ("collapse", 1),
 ("scrunch", 0), ("map", 0), ("compress", 0), ("map", 0), ("compress_builtin", 0), ("map", 0), ("compress_batch", 0),
 ("scan_kv", 0), ("sort_keys", 0), ("sort_keys", 0), ("sort_values", 0), ("sort_values", 0), ("sort_keys", 0)]

CPU_SCREEN = ["Map time (secs) = #", "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Add time (secs) = #",
 "Add KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Close time (secs) = #",
 "Close KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Aggregate time (secs) = #",
 "Aggregate KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Aggregate time (secs) = #",
 "Aggregate KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Broadcast time (secs) = #",
 "Broadcast KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Gather time (secs) = #",
 "Gather KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Convert time (secs) = #",
 "Convert KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Scan time (secs) = #",
 "Scan KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "# pairs, # Mb keys, # Mb values, # Mb, # pages",
 "Sort_multivalues time (secs) = #", "Sort_multivalues KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages",
 "Sort_multivalues time (secs) = #", "Sort_multivalues KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages",
 "Reduce time (secs) = #", "Reduce KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Collate time (secs) = #",
 "Collate KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Reduce time (secs) = #",
 "Reduce KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Clone time (secs) = #",
 "Clone KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Reduce time (secs) = #",
 "Reduce KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Collapse time (secs) = #",
 "Collapse KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Reduce time (secs) = #",
 "Reduce KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Scrunch time (secs) = #",
 "Scrunch KMV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Compress time (secs) = #",
 "Compress KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Compress time (secs) = #",
 "Compress KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Map time (secs) = #",
 "Map KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Compress time (secs) = #",
 "Compress KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Scan time (secs) = #",
 "Scan KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Sort_keys time (secs) = #",
 "Sort_keys KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Sort_keys time (secs) = #",
 "Sort_keys KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Sort_values time (secs) = #",
 "Sort_values KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "Sort_values time (secs) = #",
 "Sort_values KV = # pairs, # Mb keys, # Mb values, # Mb, # pages", "# pairs, # Mb keys, # Mb values, # Mb, # pages",
 "Sort_keys time (secs) = #", "Sort_keys KV = # pairs, # Mb keys, # Mb values, # Mb, # pages"]

CPU_COUNTS = [("map", 200), ("map_mr", 200), ("map_mr_batch", 200), ("map_file", 2), ("add", 400), ("close", 1),
 ("aggregate", 200), ("aggregate_dest", 200), ("broadcast", 200), ("gather", 200), ("convert", 17), ("scan_kmv", 17),
 ("kmv_stats", 17), ("sort_multivalues", 17), ("sort_multivalues_fn", 17), ("reduce", 17), ("collate", 17),
 ("reduce_sum", 17), ("map_addflag", 201), ("clone", 201), ("reduce_batch", 201), ("collapse", 1),
 ("reduce_count", 1), ("map_again", 200), ("scrunch", 1), ("map_b", 200), ("compress", 17), ("map_b2", 200),
 ("compress_builtin", 17), ("map_b3", 200), ("compress_batch", 17), ("scan_kv", 17), ("sort_keys", 17),
 ("sort_keys_fn", 17), ("sort_values", 17), ("sort_values_fn", 17), ("kv_stats", 17), ("load", 17),
 ("sort_keys_after_unspill", 17)]


def _trace(path):
    return [(r["op"], r["depth"]) for r in map(json.loads, open(path).read().splitlines())]


def _masked(text):
    return [re.sub(r"[-+]?\d+(\.\d+)?(e[-+]?\d+)?", "#", ln) for ln in text.splitlines()]


def test_every_op_keeps_its_names(tmp_path):
    """Every CPU-engine op once, on one rank with verbosity 1 and timer 1: the
    (op, depth) records of the trace in order, the screen lines in order (every
    number masked as #) and every returned count. The three literals were
    recorded by running this job on the commit before the op frame was
    introduced, so they pin the names, headings and counts the faces and
    tools/trace_summary.py rely on."""
    r = _py(CPU_JOB, {"OP_PROTOCOL_TMP": str(tmp_path), "MRH_TRACE": str(tmp_path / "trace")})
    assert r.returncode == 0, r.stderr
    assert _trace(tmp_path / "trace.0") == CPU_TRACE
    assert _masked(r.stdout) == CPU_SCREEN
    assert [tuple(c) for c in json.load(open(tmp_path / "counts.json"))] == CPU_COUNTS


def case_nested_comm(comm):
    """pipeline=0 collate and scrunch on two ranks with keys owned by both"""
    import io
    import struct
    import sys
    import gpu_mapreduce_amd as g
    out = io.StringIO()
    sys.stdout = out  # the native screen output follows sys.stdout
    try:
        mr = g.MapReduce(comm)
        mr.verbosity = 1
        mr.pipeline = 0
        mr.map(comm.size, lambda i, kv: [kv.add(struct.pack("<i", j % 61), struct.pack("<i", j)) for j in range(300)])
        nkey = mr.collate()
        owned = mr.kmv.nkey
        mr.map(comm.size, lambda i, kv: [kv.add(struct.pack("<i", j), None) for j in range(300)])
        mr.scrunch(1, b"all")
    finally:
        sys.stdout = sys.__stdout__
    return nkey, owned, out.getvalue()


def test_nested_ops_report_their_own_comm():
    """collate without the pipeline runs aggregate then convert, scrunch runs
    gather then collapse: the outer op's Comm line reports the bytes its inner
    ops moved (their start must not overwrite the outer op's)."""
    out = run_world("test_op_protocol:case_nested_comm", 2)
    assert out[0][0] == 61 and all(0 < out[r][1] < 61 for r in out), "keys must hash to both ranks"
    text = out[0][2]
    m = re.search(r"^Collate Comm = (\S+) Mb send, (\S+) Mb recv$", text, re.M)
    assert m and float(m.group(1)) > 0, text
    m = re.search(r"^Scrunch Comm = (\S+) Mb send, (\S+) Mb recv$", text, re.M)
    assert m and float(m.group(1)) > 0, text
    assert text.index("Collate Comm") < text.index("Scrunch Comm")


def test_quiet_scope_survives_a_throw():
    """collate silences its inner ops; when one of them throws (here convert,
    by fault injection) the object keeps the caller's verbosity and timer."""
    code = """
    import gpu_mapreduce_amd as g
    mr = g.MapReduce(g.Comm(device="cpu"))
    mr.verbosity = 1
    mr.timer = 1
    mr.pipeline = 0
    mr.map(1, lambda i, kv: kv.add(b"k", b"v"))
    try:
        mr.collate()
        print("NO ERROR")
    except RuntimeError as e:
        print("CAUGHT", "injected failure in convert" in str(e))
    print("SETTINGS", mr.verbosity, mr.timer)
    """
    r = _py(code, {"MRH_FAULT": "throw:convert:-1"})
    assert r.returncode == 0, r.stderr
    assert "CAUGHT True" in r.stdout
    assert "SETTINGS 1 1" in r.stdout


# 4096 pairs over 17 keys through every device functor op, then convert +
# reduce("sum") + sort_keys(1) under a 64 KiB HBM budget (the out-of-core
# branches and the per-op HBM cap). Every result is checked against NumPy.
GPU_JOB = r"""
import os, struct
import numpy as np
import torch
import gpu_mapreduce_amd as g
comm = g.Comm(device="cuda:0")
N, K = 4096, 17
t = np.arange(N)
key, val = t % K, (t * 7919) % 1009 - 500
GEN = '''
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long t, mrd::Emit& out) {
  out.emit((long long)(t % 17), (int)((t * 7919) % 1009 - 500));
}'''
GEN32 = GEN.replace("(long long)(t % 17)", "(int)(t % 17)")
DOUBLE = '''
__device__ void mr_map(mrd::Bytes k, mrd::Bytes v, long long i, mrd::Emit& out) {
  out.emit(k.as<long long>(), (int)(2 * v.as<int>()));
}'''
SUM = '''
__device__ void mr_reduce(mrd::Bytes k, mrd::Values vals, mrd::Emit& out) {
  long long s = 0;
  for (long long i = 0; i < vals.n; ++i) s += vals.get<int>(i);
  out.emit(k.as<long long>(), s);
}'''
ASC_I32 = '''
__device__ unsigned long long mr_sortkey(mrd::Bytes v) { return (unsigned int)v.as<int>() ^ 0x80000000u; }'''
DESC_I32 = '''
__device__ int mr_compare(mrd::Bytes a, mrd::Bytes b) {
  const int x = a.as<int>(), y = b.as<int>();
  return x > y ? -1 : x < y ? 1 : 0;
}'''
DESC_I64 = '''
__device__ unsigned long long mr_sortkey(mrd::Bytes k) { return ~(unsigned long long)k.as<long long>(); }'''
ASC_I64 = '''
__device__ int mr_compare(mrd::Bytes a, mrd::Bytes b) {
  const long long x = a.as<long long>(), y = b.as<long long>();
  return x < y ? -1 : x > y ? 1 : 0;
}'''
SCAN_KMV = '''
__device__ void mr_scan(mrd::Bytes k, mrd::Values vals, const mrd::MutArgs& args) {
  atomicAdd(args[0].as<unsigned long long>(), (unsigned long long)vals.n);
  int m = vals.get<int>(0);
  for (long long i = 1; i < vals.n; ++i) m = vals.get<int>(i) > m ? vals.get<int>(i) : m;
  args[1].as<long long>()[k.as<long long>()] = m;
}'''
SCAN_KV = '''
__device__ void mr_scan(mrd::Bytes k, mrd::Bytes v, long long index, const mrd::MutArgs& args) {
  unsigned long long* acc = args[0].as<unsigned long long>();
  atomicAdd(acc + 0, 1ull);
  atomicAdd(acc + 1, (unsigned long long)index);
}'''
def kv(mr, kf="<q", vf="<i"):
    return [(struct.unpack(kf, k)[0], struct.unpack(vf, v)[0]) for k, v in mr.kv_pairs()]
def kmv(mr):
    return {struct.unpack("<q", k)[0]: [struct.unpack("<i", v)[0] for v in vals] for k, vals in mr.kmv_pairs()}
sums = {k: int(val[key == k].sum()) for k in range(K)}

src = g.MapReduce(comm)
assert src.map_device(N, GEN) == N
assert sorted(kv(src)) == sorted(zip(key.tolist(), val.tolist()))
mr = g.MapReduce(comm)
assert mr.map_device(src, DOUBLE) == N
assert sorted(kv(mr)) == sorted(zip(key.tolist(), (2 * val).tolist()))
assert mr.collate() == K
assert mr.sort_multivalues_device(ASC_I32) == K
assert kmv(mr) == {k: np.sort(2 * val[key == k]).tolist() for k in range(K)}
assert mr.sort_multivalues_device(DESC_I32) == K
assert kmv(mr) == {k: np.sort(2 * val[key == k])[::-1].tolist() for k in range(K)}
total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
best = torch.zeros(K, dtype=torch.int64, device="cuda:0")
assert mr.scan_device(SCAN_KMV, args=[total, best]) == K
assert total.item() == N and best.cpu().tolist() == [int(2 * val[key == k].max()) for k in range(K)]
assert mr.reduce_device(SUM) == K
assert dict(kv(mr, vf="<q")) == {k: 2 * s for k, s in sums.items()}
assert mr.sort_keys_device(DESC_I64) == K
assert [k for k, _ in kv(mr, vf="<q")] == list(range(K))[::-1]
assert mr.sort_values_device(ASC_I64) == K
assert [v for _, v in kv(mr, vf="<q")] == sorted(2 * s for s in sums.values())
acc = torch.zeros(2, dtype=torch.int64, device="cuda:0")
assert mr.scan_device(SCAN_KV, args=[acc]) == K
assert acc.cpu().tolist() == [K, K * (K - 1) // 2]
mr = g.MapReduce(comm)
assert mr.map_device(N, GEN) == N
assert mr.compress_device(SUM) == K
assert dict(kv(mr, vf="<q")) == sums

mr = g.MapReduce(comm)
mr.hbm_budget = 64 << 10
mr.fpath = os.environ["OP_PROTOCOL_TMP"]
assert mr.map_device(N, GEN32) == N
assert mr.convert() == K
assert mr.reduce("sum") == K
assert mr.sort_keys(1) == K
got = []
assert mr.scan_kv(lambda k, v: got.append((struct.unpack("<i", k)[0], struct.unpack("<i", v)[0]))) == K
assert got == sorted(sums.items())
print("GPU-JOB-OK")
"""

GPU_TRACE = [("map", 0), ("map_mr_batch", 0), ("aggregate", 1), ("convert", 1), ("collate", 0),
             ("sort_multivalues", 0), ("sort_multivalues", 0), ("scan_device", 0), ("reduce_batch", 0),
             ("sort_keys_device", 0), ("sort_values_device", 0), ("scan_device", 0), ("map", 0),
             ("compress_batch", 0), ("map", 0), ("convert", 0), ("reduce_builtin", 0), ("sort_keys", 0),
             ("scan_kv", 0)]


@pytest.mark.gpu
def test_device_ops_keep_their_names_gpu(tmp_path):
    """The device functor ops, and convert / reduce / sort_keys past an HBM
    budget, under MRH_TRACE and MRH_CHECK=1: the job checks every result
    against NumPy, and the (op, depth) records are those recorded by running
    this job on the commit before the op frame was introduced."""
    r = _py(GPU_JOB, {"OP_PROTOCOL_TMP": str(tmp_path), "MRH_TRACE": str(tmp_path / "trace"), "MRH_CHECK": "1"},
            gpu=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GPU-JOB-OK" in r.stdout
    assert _trace(tmp_path / "trace.0") == GPU_TRACE
