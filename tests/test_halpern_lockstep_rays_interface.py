"""The opt-in of infeasibility detection in Halpern lockstep batches through the interfaces (no GPU needed):
cuoptamd_settings::halpern_lockstep_rays, the string parameter CUOPT_AMD_HALPERN_LOCKSTEP_RAYS of the C API's registry, the Python
mirror's pass-through and the entry points of the K-wide pass."""
import ctypes

import pytest

from cuopt_amd import capi
from cuopt_amd import linear_programming as lp


def test_the_settings_field_is_appended_behind_halpern_infeasibility_and_defaults_to_zero():
    # (the two classes in front keep the ends their own tests pin; the struct every call passes appends to them.  The C compiler puts
    # the new int32_t straight behind halpern_infeasibility -- inside what ctypes counts as that class's tail padding --, so the mirror
    # reads it there, as a view of the structure's own buffer)
    assert issubclass(capi.SolverSettingsWithLockstepRays, capi.SolverSettingsWithRays)
    assert [f for f, _ in capi.SolverSettingsWithRays._fields_] == ["halpern_infeasibility"]
    assert [f for f, _ in capi.SolverSettings._fields_][-1] == "halpern_lockstep"
    last, offset = capi.SolverSettingsWithRays.halpern_infeasibility, capi.SolverSettingsWithLockstepRays._LOCKSTEP_RAYS_OFFSET
    assert offset == last.offset + last.size and offset + 4 <= ctypes.sizeof(capi.SolverSettingsWithLockstepRays)
    s = capi.default_settings()
    assert isinstance(s, capi.SolverSettingsWithLockstepRays) and s.halpern_lockstep_rays == 0
    s = capi.default_settings(halpern_lockstep_rays=1)
    assert s.halpern_lockstep_rays == 1 and s.halpern_infeasibility == 0 and s.halpern_lockstep == 0 and s.detect_infeasibility == 0
    assert ctypes.c_int.from_buffer(s, offset).value == 1
    s.halpern_infeasibility = 1  # (neighbours: neither write reaches the other)
    s.halpern_lockstep_rays = 0
    assert s.halpern_infeasibility == 1 and s.halpern_lockstep_rays == 0


def test_the_library_writes_the_default_where_the_mirror_reads_it():
    s = capi.SolverSettingsWithLockstepRays()
    s.halpern_lockstep_rays = 7  # (cuoptamd_default_settings must put its 0 at this offset)
    s.halpern_infeasibility = 7
    capi.lib.cuoptamd_default_settings(ctypes.byref(s))
    assert s.halpern_lockstep_rays == 0 and s.halpern_infeasibility == 0


def test_the_string_parameter_accepts_zero_and_one_only():
    assert lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS == "amd_halpern_lockstep_rays"
    st = capi.Settings()
    try:
        assert int(st.get(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS)) == 0
        st.set(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS, "1")
        assert int(st.get(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS)) == 1
        assert int(st.get(lp.CUOPT_AMD_HALPERN_INFEASIBILITY)) == 0 and int(st.get(lp.CUOPT_AMD_HALPERN_LOCKSTEP)) == 0
        st.set(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS, 0)
        for bad in ("2", "-1"):
            with pytest.raises(capi.CuOptError):
                st.set(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS, bad)
    finally:
        st.close()


def test_the_python_mirror_validates_and_keeps_the_parameter():
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS) == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            settings.set_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS, bad)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS, 1)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS) == 1
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS] == 1
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_INFEASIBILITY] == 0


def test_the_entry_points_are_exported():
    for name in ("pdlpdev_batch_halpern_rays", "pdlpdev_batch_ray_stats", "pdlpdev_batch_spmv"):
        assert hasattr(capi.lib, name), name
    assert callable(capi.SharedMatrixBatch.spmv) and callable(capi.SharedMatrixBatch.ray_stats)


def test_null_arguments_are_refused_without_a_device():
    assert capi.lib.pdlpdev_batch_halpern_rays(None, None) == -1
    assert capi.lib.pdlpdev_batch_ray_stats(None, None) == -1
    assert capi.lib.pdlpdev_batch_spmv(None, 0, None, None, None) == -1
