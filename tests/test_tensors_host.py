"""run_tensors and the device-cloud ABI without a GPU: arguments refused before any device work, torch kept out of
`import simpleicp_amd`, the companion header (C99, versioned, every entry exported, NULL probe), and the positions the device
selection picks, against numpy.  (The GPU side: tests/test_gpu_tensors.py.)"""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from simpleicp_amd import PointCloud, SimpleICPException, _lib, backend, run_batch, run_tensors
from simpleicp_amd.pointcloud import _ALL

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture
def no_device(monkeypatch):
    """Any context (the process-wide one, the batch pool) is device work: the refusals must come first."""
    def touched(*_a, **_k):
        raise AssertionError("a context was asked for before the arguments were checked")
    monkeypatch.setattr(backend, "get_context", touched)
    monkeypatch.setattr(backend, "get_batch_contexts", touched)


def cpu(n=16, dtype=torch.float64, cols=3):
    return torch.zeros((n, cols), dtype=dtype)


def test_cpu_tensor_refused_and_pointed_to_host_road(no_device):
    with pytest.raises(ValueError) as ei:
        run_tensors(cpu(), cpu())
    msg = str(ei.value)
    assert "X_fix" in msg and "run()" in msg and "run_batch" in msg


def test_int_dtype_refused(no_device):
    with pytest.raises(TypeError, match="float32 or float64"):
        run_tensors(cpu(dtype=torch.int64), cpu())
    with pytest.raises(TypeError, match="float32 or float64"):
        run_tensors(cpu(dtype=torch.int32), cpu(dtype=torch.int32))


@pytest.mark.parametrize("shape", [(16, 2), (16,), (2, 16, 3), (16, 4)])
def test_wrong_shape_refused(no_device, shape):
    with pytest.raises(ValueError, match=r"shape \(n, 3\)"):
        run_tensors(torch.zeros(shape, dtype=torch.float64), cpu())


def test_not_a_tensor_refused(no_device):
    with pytest.raises(TypeError, match="torch.Tensor"):
        run_tensors(np.zeros((16, 3)), cpu())


def test_unknown_keyword_refused(no_device):
    with pytest.raises(TypeError, match="unexpected keyword"):
        run_tensors(cpu(), cpu(), corespondences=10)


def test_debug_dirpath_refused(no_device, tmp_path):
    with pytest.raises(SimpleICPException, match="debug_dirpath"):
        run_tensors(cpu(), cpu(), debug_dirpath=str(tmp_path))
    assert not any(tmp_path.iterdir())


def test_run_argument_checks_apply(no_device):
    """SimpleICP._check_arguments, same messages as run()."""
    with pytest.raises(SimpleICPException, match=r"^distance_weights must be > 0\.$"):
        run_tensors(cpu(), cpu(), distance_weights=0)
    with pytest.raises(SimpleICPException, match="exactly 6 elements"):
        run_tensors(cpu(), cpu(), rbp_observed_values=(0.0,) * 5)
    with pytest.raises(SimpleICPException, match="must be >= 0"):
        run_tensors(cpu(), cpu(), rbp_observation_weights=(-1.0,) + (0.0,) * 5)


def test_run_batch_refuses_half_device_pair(no_device):
    class Cuda:                            # (a stand-in, there is no GPU here: what the pair check looks at)
        __module__ = "torch"
        is_cuda = True
    with pytest.raises(ValueError, match="one CUDA tensor and one host cloud"):
        run_batch([(Cuda(), np.zeros((4, 3)))])


def test_import_does_not_import_torch():
    r = subprocess.run([sys.executable, "-c", "import sys, simpleicp_amd; simpleicp_amd.run_tensors; print('torch' in sys.modules)"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False"


def device_header_functions():
    txt = (ROOT / "include" / "simpleicp_hip_device.h").read_text()
    return sorted(set(re.findall(r"^int\s+(sicp_\w+)\s*\(", txt, flags=re.M)))


def test_device_header_symbols_exported_and_versioned():
    assert device_header_functions() == sorted(_lib.DEVICE_EXPORTS)
    L = _lib.load()
    for name in _lib.DEVICE_EXPORTS:
        assert hasattr(L, name), name
    assert L.sicp_device_version() == _lib.DEVICE_VERSION == 1
    assert _lib.device_version() == 1
    assert not set(_lib.DEVICE_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS))   # the other lists stay as they are
    txt = (ROOT / "include" / "simpleicp_hip_device.h").read_text()
    assert "#define SICP_DEVICE_VERSION 1" in txt and '#include "simpleicp_hip.h"' in txt


def test_device_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (oracle/)"
    src = tmp_path / "probe.c"
    src.write_text('#include "simpleicp_hip_device.h"\n'
                   "int probe(sicp_ctx *c, void *p) {\n"
                   "    int64_t q = 0, pos[4];\n"
                   "    return sicp_device_version() + sicp_cloud_upload_strided(c, SICP_FIX, p, SICP_DT_F32, 1, 3, 1, 0)\n"
                   "         + sicp_select_n_device(c, (const uint8_t *)p, 1, 1, (int64_t *)p, &q) + sicp_select_positions(4, 2, pos, &q)\n"
                   "         + sicp_cloud_write_strided(c, SICP_MOV, (const double *)p, p, SICP_DT_F64, 3, 1);\n"
                   "}\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_device_null_probe_in_child():
    code = (
        "import ctypes as C\n"
        "from simpleicp_amd import _lib\n"
        "L = _lib.load()\n"
        "q = C.c_int64(7)\n"
        "print(L.sicp_cloud_upload_strided(None, 0, None, 2, 1, 3, 1, 0), L.sicp_last_error().decode())\n"
        "print(L.sicp_select_n_device(None, None, 1, 1, None, C.byref(q)), q.value, L.sicp_last_error().decode())\n"
        "print(L.sicp_cloud_write_strided(None, 1, None, None, 2, 3, 1), L.sicp_last_error().decode())\n"
        "print(L.sicp_select_positions(5, 0, None, None), L.sicp_last_error().decode())\n"
    )
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith(f"{_lib.ERR_INVALID} ") and "null ctx" in lines[0]
    assert lines[1].startswith(f"{_lib.ERR_INVALID} 7 ") and "null ctx" in lines[1]
    assert lines[2].startswith(f"{_lib.ERR_INVALID} ") and "null ctx" in lines[2]
    assert lines[3].startswith(f"{_lib.ERR_INVALID} ")


def numpy_positions(m, Q):
    """What PointCloud.select_n_points does with m kept rows (pointcloud.py:196-212)."""
    if m <= Q:
        return np.arange(m, dtype=np.int64)
    return np.round(np.linspace(0, m - 1, Q)).astype(np.int64)


def position_cases():
    rng = np.random.default_rng(7)
    cases = [(1, 1), (2, 1), (5, 1), (1, 5), (7, 7), (7, 8), (8, 7), (4, 3), (6, 3), (8, 5), (10, 4), (22, 8), (2**20 + 1, 3),
             (10_000_000, 1000), (10_000_000, 10_000), (1_300_000, 10_000), (9_999_999, 999), (2**31 + 5, 1000)]
    # exact halves: (m - 1) * j / (Q - 1) = k + 0.5 in binary, e.g. Q - 1 a power of two and m - 1 odd
    cases += [(int(2 ** e * o + 1), 2 ** e + 1) for e in range(1, 8) for o in (1, 3, 5, 101)]
    cases += [(int(m), int(q)) for m, q in zip(rng.integers(1, 3_000_000, 300), rng.integers(1, 20_000, 300))]
    cases += [(int(q) + int(d), int(q)) for q, d in zip(rng.integers(1, 5000, 200), rng.integers(1, 40, 200))]
    return cases


def test_select_positions_match_numpy():
    halves = 0
    for m, Q in position_cases():
        ref = numpy_positions(m, Q)
        got = _lib.select_positions(m, Q)
        assert np.array_equal(got, ref), (m, Q)
        if m > Q > 1:
            y = np.linspace(0, m - 1, Q)
            halves += int(np.count_nonzero(y - np.floor(y) == 0.5))
    assert halves > 100                     # the half-to-even rule was exercised


def test_select_positions_are_select_n_points():
    """... and picking those positions among the kept rows is select_n_points itself (np.unique drops nothing)."""
    rng = np.random.default_rng(3)
    for n, Q, p in [(1000, 10, 0.5), (5000, 999, 0.2), (300, 300, 0.9), (64, 1, 0.5), (10_000, 1000, 0.01), (777, 50, 1.0)]:
        pc = PointCloud(np.zeros((n, 3)), columns=["x", "y", "z"])
        if p == 1.0:
            ref = pc.select_n_points(Q, _cur=_ALL)
            kept = np.arange(n)
        else:
            kept = np.flatnonzero(rng.random(n) < p)
            ref = pc.select_n_points(Q, _cur=kept)
        assert np.array_equal(kept[_lib.select_positions(len(kept), Q)], ref), (n, Q, p)
