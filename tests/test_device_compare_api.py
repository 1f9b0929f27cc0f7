"""The comparator form of the device sort functors through the C API
(MR_sort_keys_device with mr_compare code, MR_sort_multivalues_device: a C
program, compiled the way test_capi.py compiles its own) and through OINK
(`<mr> sort_multivalues/device file [bits]`, checked through print output).
The functor sources are the ones of test_device_compare.py (tests/functors)."""
import io
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu_mapreduce_amd")
FUNCTORS = os.path.join(ROOT, "tests", "functors")


@pytest.mark.gpu
def test_capi_device_compare(tmp_path):
    exe = str(tmp_path / "device_compare_test")
    subprocess.run(["gcc", "-O1", "-Wall", os.path.join(ROOT, "tests", "capi", "device_compare_test.c"), "-I",
                    os.path.join(ROOT, "csrc", "capi"), "-L", PKG, "-lmrhip", f"-Wl,-rpath,{PKG}", "-o", exe],
                   check=True)
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([exe, os.path.join(FUNCTORS, "cmp16.hip"), os.path.join(FUNCTORS, "cmp12.hip")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def _oink(comm, tmp_path, monkeypatch):
    from gpu_mapreduce_amd.oink.interp import OINK
    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    return OINK(comm, screen=out, logfile="log.oink"), out


def test_oink_sort_multivalues_device_missing_file(tmp_path, monkeypatch):
    o, _ = _oink(None, tmp_path, monkeypatch)
    from gpu_mapreduce_amd.oink.interp import OinkError
    with pytest.raises(OinkError, match="Cannot open device functor file"):
        o.file(text="mr m\nm sort_multivalues/device no_such_file.hip\n")


@pytest.mark.gpu
def test_oink_sort_multivalues_device(tmp_path, monkeypatch):
    from gpu_mapreduce_amd.parallel.comm import Comm
    o, _ = _oink(Comm(device="cuda"), tmp_path, monkeypatch)
    o.file(text="mr m\n")
    n, nkey = 3000, 4
    vals = [(i * 31 % 7 - 3, i * 17 % 9 - 4, i) for i in range(n)]
    o.mr("m").map(1, lambda itask, kv: kv.add_multi_static([struct.pack("<q", i % nkey) for i in range(n)],
                                                           [struct.pack("<iiI", *v) for v in vals]))
    # print kflag 2 = the key as uint64, vflag 6 = the first two ints (a, b) of each 12-byte value
    o.file(text="m collate NULL\n"
                "m print tmp.before 0 0 1 2 6\n"
                f"m sort_multivalues/device {os.path.join(FUNCTORS, 'cmp12.hip')}\n"
                "m print tmp.after 0 0 1 2 6\n")

    def parse(path):
        rows = []
        for ln in (tmp_path / path).read_text().splitlines():
            if ln.startswith("KMV pair"):
                x = [int(t) for t in ln.split(", values ")[1].split()]
                rows.append((int(ln.split("key ")[1].split(",")[0]), list(zip(x[0::2], x[1::2]))))
        return rows

    before, after = parse("tmp.before"), parse("tmp.after")
    assert [k for k, _ in after] == [k for k, _ in before] and sorted(k for k, _ in after) == list(range(nkey))
    for (k, got), (_, had) in zip(after, before):
        assert sorted(had) == sorted((a, b) for i, (a, b, _) in enumerate(vals) if i % nkey == k)
        assert got == sorted(had, key=lambda r: (-r[0], r[1])), k  # a descending, then b ascending
