"""The persistent re-solve with a new objective vector through the interfaces (no GPU needed): cuoptamd_solver_reset_objective /
cuoptamd_batch_reset_objectives / cuoptamd_batch_reset_stats in the solver's header and in the library, pdlpdev_set_objective /
pdlpdev_small_batch_reset_objectives / pdlpdev_small_batch_reset_stats in the device layer's, the prototypes and methods of
cuopt_amd.capi, the answers to a null solver and a null batch, and the settings struct, which did not grow."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cuopt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cuoptamd_solver_reset_objective", "cuoptamd_batch_reset_objectives", "cuoptamd_batch_reset_stats")
DEVICE_SYMBOLS = ("pdlpdev_set_objective", "pdlpdev_small_batch_reset_objectives", "pdlpdev_small_batch_reset_stats")


def test_the_symbols_are_in_both_headers_and_in_the_library():
    header = open(os.path.join(ROOT, "include", "cuopt_amd", "pdlp_solver.h")).read()
    assert re.search(r"int cuoptamd_solver_reset_objective\(cuoptamd_solver\* \w+, const double\* c, double objective_offset,", header)
    assert re.search(r"int cuoptamd_batch_reset_objectives\(cuoptamd_batch\* \w+, const double\* const\* c, const double\* objective_offset,", header)
    assert re.search(r"int cuoptamd_batch_reset_stats\(cuoptamd_batch\* \w+, int64_t out\[2\]\);", header)
    for name in SYMBOLS:
        assert hasattr(capi.lib, name), name
    device = open(os.path.join(ROOT, "include", "cuopt_amd", "pdlp_device.h")).read()
    assert re.search(r"int pdlpdev_set_objective\(pdlpdev_ctx\* ctx, const double\* c, double sums\[2\]\);", device)
    for name in DEVICE_SYMBOLS:
        assert re.search(r"int %s\(" % name, device), name
        assert hasattr(capi.lib, name), name
    # what the call does not do is said where a caller reads it
    for text in (header, device):
        assert "Out of scope" in text and "lockstep" in text and "sense" in text and "auxiliary" in text
    # pdlpdev_small_batch_reset keeps its signature
    assert re.search(r"int pdlpdev_small_batch_reset\(pdlpdev_small_batch\* batch, const int32_t\* take, const double\* const\* lb,", device)


def test_the_headers_still_compile_as_c_and_the_settings_did_not_grow(tmp_path):
    cc = next((c for c in ("cc", "gcc", "g++", "clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler on this machine (the library's own build needs one)"
    src = tmp_path / "objective_resolve.c"
    src.write_text('#include <stdio.h>\n#include "cuopt_amd/pdlp_solver.h"\n#include "cuopt_amd/pdlp_device.h"\n'
                   'int main(void) {\n'
                   '  int (*one)(cuoptamd_solver*, const double*, double, const double*, const double*, const double*, const double*,\n'
                   '             const cuoptamd_settings*, const double*, const double*) = cuoptamd_solver_reset_objective;\n'
                   '  int (*many)(cuoptamd_batch*, const double* const*, const double*, const double* const*, const double* const*,\n'
                   '              const double* const*, const double* const*, int) = cuoptamd_batch_reset_objectives;\n'
                   '  int (*stats)(cuoptamd_batch*, int64_t*) = cuoptamd_batch_reset_stats;\n'
                   '  int (*dev)(pdlpdev_ctx*, const double*, double*) = pdlpdev_set_objective;\n'
                   '  printf("%zu %d\\n", sizeof(cuoptamd_settings), one && many && stats && dev); return 0; }\n')
    exe = tmp_path / "objective_resolve.o"
    subprocess.check_call([cc, "-x", "c", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    # sizeof(cuoptamd_settings) as the C compiler sees it is the size of the mirror the solvers are created with: printed by a program
    # that needs no library
    size_src = tmp_path / "size.c"
    size_src.write_text('#include <stdio.h>\n#include "cuopt_amd/pdlp_solver.h"\nint main(void) { printf("%zu\\n", sizeof(cuoptamd_settings)); return 0; }\n')
    size_exe = tmp_path / "size"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(size_src), "-o", str(size_exe)])
    assert int(subprocess.check_output([str(size_exe)]).decode()) == ctypes.sizeof(capi.SolverSettingsWithDeviceMajor)
    assert ctypes.sizeof(capi.SolverSettingsWithDeviceMajor) == ctypes.sizeof(capi.SolverSettingsWithSharded)


def test_capi_has_the_prototypes_and_the_methods():
    vp, dbl, i = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    for name in SYMBOLS + DEVICE_SYMBOLS[:1]:
        fn = getattr(capi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and fn.argtypes[0] is vp, name
    assert capi.lib.cuoptamd_solver_reset_objective.argtypes == [vp, vp, dbl, vp, vp, vp, vp, ctypes.POINTER(capi.SolverSettings), vp, vp]
    assert capi.lib.cuoptamd_batch_reset_objectives.argtypes == [vp] * 7 + [i]
    assert capi.lib.cuoptamd_batch_reset_stats.argtypes == [vp, vp]
    assert capi.lib.pdlpdev_set_objective.argtypes == [vp, vp, vp]
    assert callable(capi.Solver.reset_objective)
    for method in ("reset_objectives", "reset_stats"):
        assert callable(getattr(capi.SharedMatrixBatch, method)), method
    assert callable(capi.Device.set_objective)


def test_a_null_solver_or_batch_fails_with_minus_one():
    c = np.zeros(3)
    assert capi.lib.cuoptamd_solver_reset_objective(None, c.ctypes.data, 0.0, None, None, None, None, None, None, None) == -1
    msg = capi.lib.cuoptamd_last_error().decode()
    assert "null" in msg and "cuoptamd_solver_reset_objective" in msg
    assert capi.lib.cuoptamd_batch_reset_objectives(None, None, None, None, None, None, None, 0) == -1
    msg = capi.lib.cuoptamd_last_error().decode()
    assert "null" in msg and "cuoptamd_batch_reset_objectives" in msg
    out = (ctypes.c_int64 * 2)()
    assert capi.lib.cuoptamd_batch_reset_stats(None, out) == -1
    assert "null" in capi.lib.cuoptamd_last_error().decode()
    assert capi.lib.pdlpdev_set_objective(None, c.ctypes.data, None) == -1
    assert "null" in capi.lib.pdlpdev_last_error().decode()


def test_a_wrong_length_is_a_value_error_before_the_call():
    class Handle:  # (never reaches the library: the length is checked first)
        n, m = 4, 2
    solver = capi.Solver.__new__(capi.Solver)
    solver.n, solver.m, solver.handle = 4, 2, None
    with pytest.raises(ValueError):
        solver.reset_objective(np.zeros(5))
    batch = capi.SharedMatrixBatch.__new__(capi.SharedMatrixBatch)
    batch.solvers, batch.handle = [Handle(), Handle()], None
    with pytest.raises(ValueError):
        batch.reset_objectives([np.zeros(4)])
    with pytest.raises(ValueError):
        batch.reset_objectives([np.zeros(4), np.zeros(3)])
    with pytest.raises(ValueError):
        batch.reset_objectives([np.zeros(4), None], objective_offset=[0.0])
    dev = capi.Device(handle=ctypes.c_void_p(), owner=False)
    dev.n = 4
    with pytest.raises(ValueError):
        dev.set_objective(np.zeros(3))
