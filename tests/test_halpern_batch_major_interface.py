"""The batch-level opt-in of device-decided major iterations for a K-workgroup Halpern batch through the interfaces (no GPU needed):
cuoptamd_batch_set_halpern_device_major / cuoptamd_batch_halpern_device_major / cuoptamd_batch_halpern_burst_stats in the header and
in the library, the prototypes and methods of cuopt_amd.capi, and the setter's answer to a null batch."""
import ctypes
import os
import re
import shutil
import subprocess

from cuopt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cuoptamd_batch_set_halpern_device_major", "cuoptamd_batch_halpern_device_major", "cuoptamd_batch_halpern_burst_stats")
DEVICE_SYMBOLS = ("pdlpdev_small_batch_set_halpern_device_major", "pdlpdev_small_batch_run_halpern_burst", "pdlpdev_small_batch_halpern_burst_stats",
                  "pdlpdev_debug_halpern_major_decide_batch")


def test_the_three_symbols_are_in_the_header_and_in_the_library():
    header = open(os.path.join(ROOT, "include", "cuopt_amd", "pdlp_solver.h")).read()
    assert re.search(r"int cuoptamd_batch_set_halpern_device_major\(cuoptamd_batch\* \w+, int32_t P\);", header)
    assert re.search(r"int cuoptamd_batch_halpern_device_major\(cuoptamd_batch\* \w+\);", header)
    assert re.search(r"int cuoptamd_batch_halpern_burst_stats\(cuoptamd_batch\* \w+, int64_t out\[4\]\);", header)
    for name in SYMBOLS:
        assert hasattr(capi.lib, name), name
    device = open(os.path.join(ROOT, "include", "cuopt_amd", "pdlp_device.h")).read()
    for name in DEVICE_SYMBOLS:
        assert re.search(r"int %s\(" % name, device), name
        assert hasattr(capi.lib, name), name


def test_the_headers_still_compile_as_c_and_the_settings_did_not_grow(tmp_path):
    cc = next((c for c in ("cc", "gcc", "g++", "clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler on this machine (the library's own build needs one)"
    src = tmp_path / "batch_major.c"
    src.write_text('#include <stdio.h>\n#include "cuopt_amd/pdlp_solver.h"\n#include "cuopt_amd/pdlp_device.h"\n'
                   'int main(void) { int (*set)(cuoptamd_batch*, int32_t) = cuoptamd_batch_set_halpern_device_major;\n'
                   '  int (*get)(cuoptamd_batch*) = cuoptamd_batch_halpern_device_major;\n'
                   '  int (*stats)(cuoptamd_batch*, int64_t*) = cuoptamd_batch_halpern_burst_stats;\n'
                   '  printf("%zu %d\\n", sizeof(cuoptamd_settings), set && get && stats); return 0; }\n')
    obj = tmp_path / "batch_major.o"
    subprocess.check_call([cc, "-x", "c", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)])
    # (the option is the batch object's: the struct the solvers are created with has the size its own mirror has)
    assert ctypes.sizeof(capi.SolverSettingsWithDeviceMajor) == ctypes.sizeof(capi.SolverSettingsWithSharded)


def test_capi_has_the_prototypes_and_the_methods():
    for name in SYMBOLS:
        fn = getattr(capi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and fn.argtypes[0] is ctypes.c_void_p, name
    assert capi.lib.cuoptamd_batch_set_halpern_device_major.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert capi.lib.cuoptamd_batch_halpern_burst_stats.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    for method in ("set_halpern_device_major", "halpern_device_major", "burst_stats"):
        assert callable(getattr(capi.SharedMatrixBatch, method)), method
    assert capi.SmallBatch is capi.SharedMatrixBatch
    assert callable(capi.debug_halpern_major_decide_batch)


def test_the_setter_on_a_null_batch_fails_with_minus_one():
    for P in (0, 4, 17):
        assert capi.lib.cuoptamd_batch_set_halpern_device_major(None, P) == -1
        assert "null batch" in capi.lib.cuoptamd_last_error().decode()
    assert capi.lib.cuoptamd_batch_halpern_device_major(None) == 0
    out = (ctypes.c_int64 * 4)()
    assert capi.lib.cuoptamd_batch_halpern_burst_stats(None, out) == -1
