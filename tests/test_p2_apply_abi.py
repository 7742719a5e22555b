"""tfem_p2_apply_rows (csrc/tfem_p2apply.hip) as far as a machine without a GPU can tell: the
declaration, the export, the refusals decided on the host before any launch, and the engine's
may_apply_p2_matrix_free()."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID, UNSUPPORTED = 1, 2  # TFEM_ERR_INVALID_ARGUMENT, TFEM_ERR_UNSUPPORTED


def test_header_declares_and_library_exports_the_p2_apply_entry_point():
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    header = open(os.path.join(REPO, "include", "tfem_assembly.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*(tfem_[a-z0-9_]+)\(", header, re.M))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    listing = subprocess.run([nm, "-D", "--defined-only", _native.LIB_PATH], check=True,
                             capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    name = "tfem_p2_apply_rows"
    assert name in declared, f"{name} is not declared in tfem_assembly.h"
    assert name in exported and hasattr(lib, name), f"{name} is not exported"
    # coords, real_bytes, quad_order, alpha, beta, plan, layout, colind, nnz, u, y, n_dofs, stream
    assert len(_native.SIGNATURES[name][1]) == 13
    assert lib.tfem_abi_version() == 2


def test_p2_apply_refuses_bad_arguments_without_a_device():
    """real_bytes, a NULL layout, negative sizes, an n_dofs that is not the plan's, overlapping
    vectors, an unknown quadrature order, NULL arrays: all decided on the host before any launch."""
    from pytorch_fem_solver_amd import _native

    lib = _native.load()
    layout = np.zeros(24, dtype=np.int64)
    layout[0], layout[1], layout[2], layout[3] = 1, 1, 25, 56  # a launch would follow the checks
    z = ctypes.c_void_p(layout.ctypes.data)
    call = lib.tfem_p2_apply_rows

    def refused(status, word, *args):
        assert call(*args) == status
        assert word in lib.tfem_last_error(), lib.tfem_last_error()

    refused(INVALID, b"real_bytes", None, 3, 2, 1.0, 0.0, None, z, None, 10, None, None, 81, None)
    refused(INVALID, b"plan_layout_host", None, 8, 2, 1.0, 0.0, None, None, None, 10, None, None, 81, None)
    refused(INVALID, b"negative", None, 8, 2, 1.0, 0.0, None, z, None, 10, None, None, -1, None)
    refused(INVALID, b"negative", None, 8, 2, 1.0, 0.0, None, z, None, -10, None, None, 81, None)
    refused(INVALID, b"81 DoFs, not 80", None, 8, 2, 1.0, 0.0, None, z, None, 10, None, None, 80, None)
    # u inside [y, y + 81 * 8): addresses only, nothing is dereferenced
    y = ctypes.c_void_p(1 << 20)
    refused(INVALID, b"overlap", None, 8, 2, 1.0, 0.0, None, z, None, 10, ctypes.c_void_p((1 << 20) + 8 * 80), y, 81, None)
    refused(INVALID, b"overlap", None, 8, 2, 1.0, 0.0, None, z, None, 10, y, y, 81, None)
    refused(UNSUPPORTED, b"order", None, 8, 9, 1.0, 0.0, None, z, None, 10, None, y, 81, None)
    refused(INVALID, b"NULL", None, 8, 2, 1.0, 0.0, None, z, None, 10, None, y, 81, None)
    # an empty plan: nothing to do
    empty = np.zeros(24, dtype=np.int64)
    assert call(None, 8, 2, 1.0, 0.0, None, ctypes.c_void_p(empty.ctypes.data), None, 0, None, None, 0, None) == 0


def test_may_apply_p2_matrix_free_is_known_without_a_device(monkeypatch):
    import pytorch_fem_solver_amd as tf
    from pytorch_fem_solver_amd import meshgen

    mesh_np = meshgen.unit_square(4, 0.25, 0)
    p1 = tf.Basis(tf.MeshTri(triangulation=mesh_np), tf.ElementTri(1, 3))._engine
    p2 = tf.Basis(tf.MeshTri(triangulation=mesh_np), tf.ElementTri(2, 2))._engine
    assert p1.may_apply_p2_matrix_free() is False and p1.may_apply_matrix_free() is True
    assert p2.may_apply_p2_matrix_free() is True and p2.may_apply_matrix_free() is False
    assert p2._p2rows is None and p2._csr is None  # nothing was built to answer
    monkeypatch.setenv("TFEM_KERNEL", "gather")
    forced = tf.Basis(tf.MeshTri(triangulation=mesh_np), tf.ElementTri(2, 2))._engine
    assert forced.may_apply_p2_matrix_free() is False
