"""The C-ABI library loads and exports every symbol include/e3gnn.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import subprocess
import sys

import pytest

from sevennet_finetuning_amd import _lib


def test_library_exports_header_symbols():
    lib = _lib.load()
    declared = _lib.header_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), name
    assert set(declared) == set(_lib.SIGNATURES), set(declared) ^ set(_lib.SIGNATURES)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    assert set(declared) <= exported


def test_build_lib_refuses_variants_as_the_product(tmp_path):
    """defines without a path of their own would rebuild the product library as
    a variant, and an unknown switch name would build the default kernels under
    a variant's name: both are refused before anything is compiled"""
    from sevennet_finetuning_amd import build_lib
    with pytest.raises(ValueError, match='out'):
        build_lib.build(defines=['E3GNN_DH2_X3=0'])
    with pytest.raises(ValueError, match='E3GNN_LS_DMA.*E3GNN_STAMPS_FWD'):
        build_lib.build(out=str(tmp_path / 'v.so'), defines=['E3GNN_DH2_X3=0', 'E3GNN_LS_DMA=1'])
    assert not (tmp_path / 'v.so').exists()
    # the command line goes through the same check
    r = subprocess.run([sys.executable, '-m', 'sevennet_finetuning_amd.build_lib', '-DE3GNN_STAMPS'],
                       capture_output=True, text=True)
    assert r.returncode != 0 and '--out' in r.stderr


def test_environment_switches_are_the_documented_ones():
    """the run-time switches of the product: every E3GNN_* name the library
    reads with getenv or the package reads through os.environ (DESIGN.md,
    "Switches", says why each remains)"""
    import glob
    import os
    import re
    pkg = os.path.dirname(_lib.__file__)
    names = set()
    for ext in ('cpp', 'hip', 'h'):
        for path in glob.glob(os.path.join(pkg, 'csrc', '*.' + ext)):
            with open(path) as f:
                names |= set(re.findall(r'getenv\(\s*"(E3GNN_[A-Z0-9_]+)"', f.read()))
    for path in glob.glob(os.path.join(pkg, '*.py')):
        with open(path) as f:
            for line in f:
                if 'os.environ' in line:
                    names |= set(re.findall(r'''['"](E3GNN_[A-Z0-9_]+)['"]''', line))
    assert names == {'E3GNN_LIB', 'E3GNN_GENERIC', 'E3GNN_NODELIN', 'E3GNN_D3_BIN', 'E3GNN_D3_NO_C6TAB',
                     'E3GNN_TRACE_ERRORS', 'E3GNN_SYNC', 'E3GNN_TRAIN_IRREPS'}


def test_abi_version_and_errors():
    lib = _lib.load()
    assert lib.e3gnn_abi_version() == 1
    # bad arguments are reported, not crashed on (no device needed for these)
    out = (ctypes.c_float * 27)()
    assert lib.e3gnn_cg_table(3, 3, 3, out) != 0
    assert b'coupling' in lib.e3gnn_last_error()
    assert lib.e3gnn_layer_forward(None, 0, None) != 0
    assert lib.e3gnn_ctx_create(None) is None
    # one refused call per translation unit behind the ABI (csrc/api_train.cpp,
    # api_nlist.cpp, api_d3.cpp): each sets the library's one last-error string
    ERR_ARG = 1
    assert lib.e3gnn_conv_dims(7, None, None, None) == ERR_ARG
    assert b'conv kind' in lib.e3gnn_last_error()
    assert lib.e3gnn_nlist_build(None, 0, None, None, None, 5.0, None, None) == ERR_ARG
    assert b'null neighbour-list handle' in lib.e3gnn_last_error()
    assert lib.e3gnn_d3_compute(None, 0, None, None, None, None, None, None, None, None) == ERR_ARG
    assert b'null d3 handle' in lib.e3gnn_last_error()


def test_library_is_gfx950_code_object(tmp_path):
    import shutil
    lib = tmp_path / 'lib.so'   # --offloading extracts bundles next to its input
    shutil.copy(_lib.LIB_PATH, lib)
    out = subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-objdump', '--offloading', str(lib)],
                         capture_output=True, text=True, cwd=tmp_path)
    text = out.stdout + out.stderr
    assert 'gfx950' in text


def test_grouped_gemm_refuses_operands_beyond_32bit_offsets():
    """e3gnn_gemm_grouped addresses each operand through one buffer
    descriptor (32-bit byte offsets, csrc/tgemm.hip TG_RECORDS): a problem
    whose operand spans more is refused with E3GNN_ERR_ARG before anything
    is launched (no device is touched, so this runs on the CPU)"""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: the check comes first
    d = _lib.GemmDesc()
    d.a = d.b = d.c = fake
    d.m, d.n, d.ldc = 64, 64, 64
    # op(A) = A^T of a (K x 64) row-major matrix: K = 2^23 rows x 64 floats = 2 GB
    d.k, d.lda, d.trans_a, d.ldb, d.trans_b = 1 << 23, 64, 1, 64, 0
    rc = lib.e3gnn_gemm_grouped(1, ctypes.byref(d), None, 0, None)
    assert rc == 1   # E3GNN_ERR_ARG
    assert b'2 GB' in lib.e3gnn_last_error()
    # an int32-overflowing leading dimension is refused as well
    d.k, d.lda = 16, 1 << 33
    assert lib.e3gnn_gemm_grouped(1, ctypes.byref(d), None, 0, None) != 0
    # general layouts: K summed over segments whose stride walks past 2 GB
    lay = _lib.GemmLayouts()
    d2 = _lib.GemmDesc()
    d2.a = d2.b = d2.c = fake
    d2.m, d2.n, d2.k = 16, 16, 4 * 1000
    for g in (lay.a, lay.b):
        g.ld, g.rep, g.rs, g.kst, g.ks, g.sst = 16, 1, 0, 1 << 20, 1000, 1
    lay.ldc, lay.crep, lay.crs, lay.cns = 16, 1, 0, 1
    d2.layout = ctypes.addressof(lay)
    assert lib.e3gnn_gemm_grouped(1, ctypes.byref(d2), None, 0, None) != 0
    assert b'2 GB' in lib.e3gnn_last_error()
