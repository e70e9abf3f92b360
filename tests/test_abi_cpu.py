"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/dct.h declares, and the ctypes binding table covers exactly that set."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "dct.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dct_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from dct_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) > 40
    for n in names:
        assert hasattr(lib, n), f"libdct_hip.so does not export {n}"


def test_binding_table_matches_header():
    from dct_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_status_strings_and_version():
    from dct_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dct.h")).read()
    assert lib.dct_version() == _lib.ABI_VERSION == int(re.search(r"#define DCT_VERSION (\d+)", header).group(1)) == 101
    assert lib.dct_status_string(0) == b"ok"
    assert b"workspace" in lib.dct_status_string(-4)


def test_load_refuses_a_library_of_another_abi_version(monkeypatch):
    """A stale libdct_hip.so beside newer Python would be handed structs of another layout: load() must refuse it."""
    import pytest
    from dct_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(ImportError, match="ABI version"):
        _lib.load()


def test_product_path_rejects_cpu_tensors():
    import pytest
    import torch
    from dct_amd import _lib
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.view(torch.zeros(1, 2, 2, 8))
    with pytest.raises(RuntimeError):
        _lib.check(-2, "x")


def test_library_holds_no_packed_fp32_arithmetic(tmp_path):
    """csrc/Makefile builds every device file with -packed-fp32-ops: a packed-FP32 instruction that reads a source pair with swapped
    halves gives wrong results in waves that run beside the shared-halo conv / filter-row weight-gradient kernels (DESIGN 4.3,
    tools/probe_packed_fp32), and the compiler forms such instructions from ordinary float code.  The gfx950 code object of the built
    library must therefore hold no v_pk_{add,mul,fma}_f32 at all (a new file compiled without the flag, or inline asm, would)."""
    import shutil
    import subprocess
    import pytest
    from dct_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{llvm}/llvm-objdump") and shutil.which("objcopy")):
        pytest.skip("no ROCm binutils here")
    so = _lib.LIB_PATH
    fat, co = str(tmp_path / "fatbin.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    subprocess.check_call([f"{llvm}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    asm = subprocess.run([f"{llvm}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    assert asm.count("v_mfma_f32_") > 100                      # (the right code object: the MFMA tiles are in it)
    packed = re.findall(r"v_pk_(?:add|mul|fma)_f32[^\n]*", asm)
    assert not packed, packed[:5]
