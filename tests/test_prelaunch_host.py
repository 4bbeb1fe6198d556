"""Host side of the tail -> match hand-over (no GPU): the bookkeeping header under the sanitizers, the companion header and the
binding."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_handover_bookkeeping_under_sanitizers(tmp_path):
    """tests/native/handover_check.cpp: a stand-alone program (its own main, the launchers stubbed) compiled with
    -fsanitize=address,undefined and run as it is."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "handover_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(ROOT / "tests" / "native" / "handover_check.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "handover_check OK" in r.stdout


def test_chain_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "simpleicp_hip_chain.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.CHAIN_EXPORTS)
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.CHAIN_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS) | set(_lib.OUTLIER_EXPORTS))
    assert not set(_lib.CHAIN_EXPORTS) & others
    L = _lib.load()
    assert L.sicp_chain_version() == _lib.CHAIN_VERSION == 1
    assert L.sicp_chain_info(None, None) == _lib.ERR_INVALID
