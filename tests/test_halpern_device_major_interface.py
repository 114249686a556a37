"""The opt-in of device-decided major iterations in reflected-Halpern mode through the interfaces (no GPU needed):
cuoptamd_settings::halpern_device_major, the string parameter CUOPT_AMD_HALPERN_DEVICE_MAJOR of the C API's registry and the Python
mirror's constant and pass-through."""
import ctypes
import os
import shutil
import subprocess

import pytest

from cuopt_amd import capi
from cuopt_amd import linear_programming as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_layout(tmp_path):
    """(offsetof(halpern_sharded), offsetof(halpern_device_major), sizeof(cuoptamd_settings)) as the C compiler lays the struct out"""
    cc = next((c for c in ("cc", "gcc", "g++", "clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler on this machine (the library's own build needs one)"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cuopt_amd/pdlp_solver.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", offsetof(cuoptamd_settings, halpern_sharded), '
                   'offsetof(cuoptamd_settings, halpern_device_major), sizeof(cuoptamd_settings)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return tuple(int(v) for v in subprocess.check_output([str(exe)]).split())


def test_the_settings_field_is_appended_behind_halpern_sharded_where_the_c_compiler_puts_it(tmp_path):
    sharded, major, size = _c_layout(tmp_path)
    assert major == sharded + 4  # appended, with nothing in between
    assert issubclass(capi.SolverSettingsWithDeviceMajor, capi.SolverSettingsWithSharded)
    # (halpern_sharded ends four bytes short of the doubles' alignment: the new member lies in what ctypes counts as tail padding, so it
    # is a view of those bytes and no entry of _fields_; the classes in front keep the ends their own tests pin)
    assert capi.SolverSettingsWithDeviceMajor._fields_ == []
    assert [f for f, _ in capi.SolverSettingsWithSharded._fields_] == ["halpern_sharded"]
    assert capi.SolverSettingsWithSharded.halpern_sharded.offset == sharded
    assert capi.SolverSettingsWithDeviceMajor._DEVICE_MAJOR_OFFSET == major
    assert ctypes.sizeof(capi.SolverSettingsWithDeviceMajor) == size == ctypes.sizeof(capi.SolverSettingsWithSharded)
    s = capi.default_settings()
    assert isinstance(s, capi.SolverSettingsWithDeviceMajor) and s.halpern_device_major == 0
    s = capi.default_settings(halpern_device_major=5)
    assert s.halpern_device_major == 5 and s.halpern_sharded == 0 and s.halpern_lockstep_rays == 0 and s.halpern_infeasibility == 0
    assert ctypes.c_int.from_buffer(s, major).value == 5
    s.halpern_sharded = 1  # (neighbours: neither write reaches the other)
    s.halpern_device_major = 0
    assert s.halpern_sharded == 1 and s.halpern_device_major == 0
    s.halpern_device_major = 16
    s.halpern_sharded = 0
    assert s.halpern_sharded == 0 and s.halpern_device_major == 16


def test_the_library_writes_the_default_where_the_mirror_reads_it():
    s = capi.SolverSettingsWithDeviceMajor()
    s.halpern_device_major = 7  # (cuoptamd_default_settings must put its 0 at this offset)
    s.halpern_sharded = 7
    capi.lib.cuoptamd_default_settings(ctypes.byref(s))
    assert s.halpern_device_major == 0 and s.halpern_sharded == 0


def test_the_string_parameter_takes_zero_to_sixteen():
    assert lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR == "amd_halpern_device_major"
    st = capi.Settings()
    try:
        assert int(st.get(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR)) == 0
        for good in range(0, 17):
            st.set(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR, str(good))
            assert int(st.get(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR)) == good
        assert int(st.get(lp.CUOPT_AMD_HALPERN_SHARDED)) == 0 and int(st.get(lp.CUOPT_AMD_HALPERN_RESIDENT)) == 0
        for bad in ("-1", "17"):
            with pytest.raises(capi.CuOptError):
                st.set(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR, bad)
        assert int(st.get(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR)) == 16  # (a refused value changes nothing)
    finally:
        st.close()


def test_the_python_mirror_validates_and_keeps_the_parameter():
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR) == 0
    for bad in (17, -1):
        with pytest.raises(ValueError):
            settings.set_parameter(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR, bad)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR) == 0
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR, 4)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR) == 4
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_DEVICE_MAJOR] == 4
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_SHARDED] == 0


def test_the_record_and_parameter_mirrors_have_the_c_sizes(tmp_path):
    cc = next((c for c in ("cc", "gcc", "g++", "clang") if shutil.which(c)), None)
    assert cc is not None
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cuopt_amd/pdlp_device.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(pdlpdev_halpern_major_params), sizeof(pdlpdev_halpern_major_record), '
                   'offsetof(pdlpdev_halpern_major_params, per_constraint_residual), offsetof(pdlpdev_halpern_major_record, steps_taken)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    params, record, pc, steps = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert ctypes.sizeof(capi.HalpernMajorParams) == params and capi.HalpernMajorParams.per_constraint_residual.offset == pc
    assert ctypes.sizeof(capi.HalpernMajorRecord) == record and capi.HalpernMajorRecord.steps_taken.offset == steps
