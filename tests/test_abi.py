"""CPU: the C-ABI library loads and exports every symbol include/ultrafnd_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def _declared():
    text = (REPO / "include" / "ultrafnd_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ufnd_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import torch  # noqa: F401  (its HIP runtime must be resident before ours is resolved)
    from ultrafnd_git_amd.build import build
    lib = ctypes.CDLL(str(build()))
    names = _declared()
    assert len(names) >= 10
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    from ultrafnd_git_amd import _lib as L
    assert lib.ufnd_abi_version() == L.ABI_VERSION == 6


def test_struct_mirrors_match_header_sizes():
    from ultrafnd_git_amd import _lib as L
    assert ctypes.sizeof(L.StepState) == 80
    assert ctypes.sizeof(L.Dims) == 13 * 4
    assert ctypes.sizeof(L.FusionParams) == 8 * (12 + 12 + 6)
    assert ctypes.sizeof(L.ClfParams) == 8 * 11


def test_argument_checks_reject_bad_calls_without_touching_a_gpu():
    from ultrafnd_git_amd import _lib as L
    lib = L.lib()
    d = L.Dims()
    d.hidden = 500
    assert lib.ufnd_fusion_workspace_floats(ctypes.byref(d), 4) > 0
    rc = lib.ufnd_fusion_forward(ctypes.byref(d), None, None, None, None, None, None, 4, 0, None, None, 512, None, None,
                                 None, None)
    assert rc == 1 and b"hidden" in lib.ufnd_last_error()
    assert lib.ufnd_grad_norm(None, 0, None, None, None) == 1


def test_product_never_imports_the_oracle():
    """The oracle is the checker: the package and the tools never import it (tests/, __graft_entry__.smoke() and bench.py's
    cpu_baseline leg do)."""
    for d in ("ultrafnd_git_amd", "tools"):
        for f in (REPO / d).rglob("*.py"):
            src = f.read_text()
            assert "import oracle" not in src and "from oracle" not in src, f


def test_product_reads_no_environment_override():
    """No test seam or experiment switch hides behind an environment variable: the package's Python reads none (build.py's
    HIPCC -- which compiler binary to run -- is the one exception), and the library's strings name no UFND_* variable."""
    import torch  # noqa: F401
    from ultrafnd_git_amd.build import build
    for f in (REPO / "ultrafnd_git_amd").rglob("*.py"):
        src = f.read_text()
        for m in re.finditer(r"environ(?:\.get)?\s*[\[(]\s*[\"']([A-Za-z0-9_]+)", src):
            assert f.name == "build.py" and m.group(1) == "HIPCC", (f.name, m.group(1))
        assert "getenv" not in src, f
    assert not re.search(rb"UFND_[A-Z_]{3,}", Path(build()).read_bytes())


def test_diagnostics_are_not_reachable_through_the_product_library():
    """Timing ablations, in-kernel stamps and experimental tiles live in libultrafnd_hip_diag.so (csrc/diag/): the
    product library exports none of them, has no environment override of the tile choice, and the package never
    loads the diagnostics library."""
    import torch  # noqa: F401
    from ultrafnd_git_amd.build import build
    lib = ctypes.CDLL(str(build()))
    for name in ("ufnd_gemm_bf16_stamps", "ufnd_diag_gemm_bf16_stamps", "ufnd_diag_gemm_bf16_ex", "ufnd_diag_where"):
        assert not hasattr(lib, name), name
    blob = Path(build()).read_bytes()
    assert b"UFND_GEMM_FORCE_CFG" not in blob
    for f in (REPO / "ultrafnd_git_amd").rglob("*.py"):
        if f.name != "build.py":
            assert "hip_diag" not in f.read_text(), f
    # the tile table query is host-only: ids built into the library answer 1, others 0
    n = lib.ufnd_gemm_bf16_tile_count()
    built = [t for t in range(n) if lib.ufnd_gemm_bf16_tile_info(t, None, None, None)]
    assert 4 <= len(built) < n and lib.ufnd_gemm_bf16_tile_info(n, None, None, None) == 0 and lib.ufnd_gemm_bf16_tile_info(-1, None, None, None) == 0


def test_no_device_kernel_of_the_product_library_uses_scratch(tmp_path):
    """Register spills are silent HBM traffic (round 3: 56 spilled VGPRs in the 256x256 LayerNorm-aware GEMM cost 44 MB
    read + 44 MB written per FFN1 launch and 5 % of the step; only the PMC WRITE_SIZE pass showed it).  The code
    objects' own metadata says what each kernel reserves: every kernel of the product library must reserve none."""
    import shutil
    import subprocess
    from ultrafnd_git_amd.build import build
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "llvm-objdump").exists() or not (llvm / "llvm-readelf").exists():
        pytest.skip("ROCm LLVM binutils not present")
    so = tmp_path / "lib.so"
    shutil.copy(build(), so)
    subprocess.run([str(llvm / "llvm-objdump"), "--offloading", so.name], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(tmp_path.glob("lib.so.*gfx950"))
    assert objs, "no gfx950 code object in the library"
    kernels, bad = 0, []
    for o in objs:
        notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            kernels += 1
            if int(m.group(2)) != 0:
                bad.append((m.group(1), int(m.group(2))))
    assert kernels >= 40, kernels
    assert not bad, bad
