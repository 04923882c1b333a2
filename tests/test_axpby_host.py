"""Host-side checks of Y = alpha*A*X + beta*Y (smfv_plan_execute_axpby): the
C ABI exports it, SMFV_PLAN_STATS did not grow, and the epilogue instances of
the row kernels fit the register budgets of the plain ones (read from the
code object's metadata, as test_host.py::test_ws_kernels_register_budget
does for the plain k_rows_ws instances).  No GPU.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparsematrixmultiplicationmpi_amd")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_axpby_symbols_exported():
    lib = ctypes.CDLL(os.path.join(PKG, "libsmfv.so"))
    for name in ("smfv_plan_execute_axpby", "smfv_plan_epilogue_mode"):
        assert hasattr(lib, name), name


def test_plan_stats_did_not_grow():
    """The epilogue mode has its own accessor: out[] of smfv_plan_stats keeps
    its 18 entries (callers size their arrays by the header's constant)."""
    with open(os.path.join(ROOT, "include", "smfv.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+SMFV_PLAN_STATS\s+(\d+)", src).group(1) == "18"
    assert re.search(r"#define\s+SMFV_PLAN_AXPBY\s+65536\b", src)
    assert re.search(r"#define\s+SMFV_PLAN_AXPBY_TWO_PASS\s+131072\b", src)
    from sparsematrixmultiplicationmpi_amd import engine
    assert engine.PLAN_STATS == 18 and engine.PLAN_AXPBY == 65536 and engine.PLAN_AXPBY_TWO_PASS == 131072


def _kernel_notes(tmp_path):
    """mangled kernel name -> (vgprs, vgpr spills, sgpr spills) of libsmfv.so's gfx950 code object"""
    so = tmp_path / "libsmfv.so"
    shutil.copy(os.path.join(PKG, "libsmfv.so"), so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(so)], cwd=tmp_path, capture_output=True,
                   check=True)
    co = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert co, os.listdir(tmp_path)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / co[0])],
                           capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = tuple(int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                          for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count"))
    return out


def test_axpby_kernels_register_budget(tmp_path):
    """Every epilogue instance of the tiled kernel (k_ws_axpby, k_ws_axpby_live)
    fits the waves per SIMD its geometry runs -- geometries 1 (8 + 8 waves)
    and 2 (4 + 4, two blocks per CU): 4 waves per SIMD, <= 128 VGPRs; geometry
    3 (8 + 4): 3 waves, <= 168 -- with no spills: y0 is loaded at the store,
    where the row's read-ahead registers are dead, so the epilogue does not
    raise the peak.  The epilogue instances of k_rows_mh, k_rows (their Axpby
    argument pack) and k_rows_list do not spill."""
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no ROCm llvm tools")
    notes = _kernel_notes(tmp_path)
    per_geom = {1: 0, 2: 0, 3: 0}
    others = {"k_rows_mh": 0, "k_rows": 0, "k_rows_list_axpby": 0, "k_axpby": 0}
    for name, (vgpr, vspill, sspill) in notes.items():
        geo = re.search(r"\d+k_ws_axpby(?:_live)?ILi(\d+)ELi(\d+)E", name)
        if geo:
            cw, lw = map(int, geo.groups())
            g = {(8, 8): 1, (4, 4): 2, (8, 4): 3}[(cw, lw)]
            assert vgpr <= (168 if g == 3 else 128) and vspill == 0 and sspill == 0, (name, vgpr, vspill, sspill)
            per_geom[g] += 1
            continue
        m = re.match(r"_ZN4smfv\d+(k_rows_mh|k_rows)I.*5AxpbyE", name) or \
            re.match(r"_ZN4smfv\d+(k_rows_list_axpby|k_axpby)[EI]", name)
        if m:
            assert vspill == 0 and sspill == 0, (name, vspill, sspill)
            others[m.group(1)] += 1
    # per geometry: snapshot (SADDR x NARROW) and live (NARROW) instances
    assert all(n >= 6 for n in per_geom.values()), per_geom
    assert all(n >= 1 for n in others.values()), others
    # the plain instances are still there under their own names
    assert sum("k_rows_ws" in n for n in notes) >= 24
