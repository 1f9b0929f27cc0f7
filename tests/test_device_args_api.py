"""Device functor arguments through the other faces of the engine: the C API
(MR_set_device_args with hipMalloc'd buffers, MR_map_device_tasks,
MR_scan_device: a C program built the way test_device_compare_api.py builds
its own, plus the HIP runtime for the buffers), OINK (`<mr> device_args v...`,
`<mr> scan/device file`) and the worked example examples/python/
kmeans_device.py, whose centroids after every Lloyd step must equal a NumPy
step exactly and whose whole run costs one compile per functor source."""
import importlib.util
import io
import os
import subprocess

import numpy as np
import pytest
import torch

from test_device_args import MAP_TABLE, SCAN_KV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu_mapreduce_amd")


def _example():
    spec = importlib.util.spec_from_file_location("kmeans_device", os.path.join(ROOT, "examples", "python", "kmeans_device.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rocm():
    from torch.utils.cpp_extension import ROCM_HOME
    return ROCM_HOME or os.environ.get("ROCM_PATH") or "/opt/rocm"


@pytest.mark.gpu
def test_capi_device_args(tmp_path):
    exe = str(tmp_path / "device_args_test")
    rocm = _rocm()
    subprocess.run(["gcc", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "capi", "device_args_test.c"),
                    "-I", os.path.join(ROOT, "csrc", "capi"), "-I", os.path.join(rocm, "include"), "-L", PKG, "-lmrhip",
                    "-L", os.path.join(rocm, "lib"), "-lamdhip64", f"-Wl,-rpath,{PKG}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}",
                    "-o", exe], check=True)
    (tmp_path / "map.hip").write_text(MAP_TABLE)
    (tmp_path / "scan.hip").write_text(SCAN_KV)
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([exe, str(tmp_path / "map.hip"), str(tmp_path / "scan.hip")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def _oink(comm, tmp_path, monkeypatch):
    from gpu_mapreduce_amd.oink.interp import OINK
    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    return OINK(comm, screen=out, logfile="log.oink"), out


# every task whose number is a multiple of the bound parameter (args[0], float64)
EVERY = r"""
__device__ void mr_map(mrd::Bytes key, mrd::Bytes value, long long t, mrd::Emit& out, const mrd::Args& args) {
  const long long step = (long long)args[0].as<double>()[0];
  if (t % step == 0) out.emit((long long)t, (long long)args[0].count<double>());
}
"""
# the pair count, added into the last bound value
COUNT = r"""
__device__ void mr_scan(mrd::Bytes key, mrd::Bytes value, long long index, const mrd::MutArgs& args) {
  atomicAdd(args[0].as<double>() + args[0].count<double>() - 1, 1.0);
}
"""


def test_oink_device_args_binds_one_float64_buffer(tmp_path, monkeypatch):
    from gpu_mapreduce_amd.oink.interp import OinkError
    o, _ = _oink(None, tmp_path, monkeypatch)
    o.file(text="mr m\nm device_args 3 0.5 -2e3\n")
    (b,) = o.mr("m").bound_device_args
    assert b.dtype.is_floating_point and b.element_size() == 8 and b.tolist() == [3.0, 0.5, -2000.0]
    o.file(text="m device_args\n")
    assert o.mr("m").bound_device_args == []
    with pytest.raises(OinkError, match="device_args value x7"):
        o.file(text="m device_args 1 x7\n")
    with pytest.raises(OinkError, match="Cannot open device functor file"):
        o.file(text="m scan/device no_such_file.hip\n")


@pytest.mark.gpu
def test_oink_device_args_and_scan_device(tmp_path, monkeypatch):
    from gpu_mapreduce_amd import C
    from gpu_mapreduce_amd.parallel.comm import Comm
    o, _ = _oink(Comm(device="cuda"), tmp_path, monkeypatch)
    (tmp_path / "every.hip").write_text(EVERY)
    (tmp_path / "count.hip").write_text(COUNT)
    o.file(text="mr m\nm device_args 3\nm map/device 1000 every.hip\n")
    mr = o.mr("m")
    assert mr.kv.n == 334 and mr.kv.vdata.view(torch.int64).unique().tolist() == [1]
    compiles = C.device_functor_compiles()
    o.file(text="m device_args 5 0\nm map/device 1000 every.hip\n")
    assert mr.kv.n == 200 and mr.kv.vdata.view(torch.int64).unique().tolist() == [2]
    assert C.device_functor_compiles() == compiles  # the parameter changed, the module did not
    o.file(text="m scan/device count.hip\n")
    assert mr.kv.n == 200  # the pairs stay
    assert mr.bound_device_args[0].tolist() == [5.0, 200.0]  # one visit per pair


@pytest.mark.gpu
def test_kmeans_example_matches_numpy_lloyd_exactly():
    from gpu_mapreduce_amd import C
    from gpu_mapreduce_amd.parallel.comm import Comm
    from gpu_mapreduce_amd.runtime.mapreduce import MapReduce
    ex = _example()
    points, init = ex.make_points()
    assert points.shape == (4096, 2) and init.shape == (4, 2)
    want, c = [], init
    for _ in range(3):
        c = ex.lloyd_step_numpy(points, c)
        want.append(c)
    assert not (want[0] == want[1]).all() and not (want[1] == want[2]).all()  # three steps that each move
    mrp = ex.load_points(MapReduce(Comm(device="cuda")), points)
    cent = torch.from_numpy(init.copy()).cuda()
    got = []
    before = C.device_functor_compiles()
    out = ex.lloyd(mrp, cent, 3, each=lambda i, t: got.append(t.cpu().numpy().copy()))
    assert C.device_functor_compiles() - before == len({ex.MAP, ex.FOLD, ex.UPDATE}) == 3
    assert out.data_ptr() == cent.data_ptr()  # updated in the bound buffer itself
    for i in range(3):
        assert (got[i] == want[i]).all(), (i, got[i], want[i])


def test_kmeans_example_points_are_exact_for_float64():
    """the oracle alone: over the three steps no point is equidistant from two
    centroids and every centroid stays on the integer lattice (whole blobs
    move between clusters), so distances, sums and means are exact in float64
    whatever the order of the additions"""
    ex = _example()
    points, c = ex.make_points()
    assert (points == np.round(points)).all() and np.abs(points).max() < 1024
    for _ in range(3):
        d2 = np.sort(((points[:, None, :] - c[None, :, :]) ** 2).sum(axis=2), axis=1)
        assert (d2[:, 0] < d2[:, 1]).all()
        c = ex.lloyd_step_numpy(points, c)
        assert (c == np.round(c)).all()
