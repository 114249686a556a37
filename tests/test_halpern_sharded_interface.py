"""The opt-in of row-block sharded solves in reflected-Halpern mode through the interfaces (no GPU needed):
cuoptamd_settings::halpern_sharded, the string parameter CUOPT_AMD_HALPERN_SHARDED of the C API's registry and the Python mirror's
constant and pass-through."""
import ctypes

import pytest

from cuopt_amd import capi
from cuopt_amd import linear_programming as lp


def test_the_settings_field_is_appended_behind_halpern_lockstep_rays_and_defaults_to_zero():
    # (halpern_lockstep_rays filled the four bytes of tail padding, so the subclass's field starts exactly where the C compiler puts
    # the new member; the classes in front keep the ends their own tests pin)
    assert issubclass(capi.SolverSettingsWithSharded, capi.SolverSettingsWithLockstepRays)
    assert [f for f, _ in capi.SolverSettingsWithSharded._fields_] == ["halpern_sharded"]
    assert [f for f, _ in capi.SolverSettingsWithRays._fields_] == ["halpern_infeasibility"]
    assert [f for f, _ in capi.SolverSettings._fields_][-1] == "halpern_lockstep"
    field = capi.SolverSettingsWithSharded.halpern_sharded
    assert field.offset == capi.SolverSettingsWithLockstepRays._LOCKSTEP_RAYS_OFFSET + 4 and field.size == 4
    assert field.offset + 4 <= ctypes.sizeof(capi.SolverSettingsWithSharded)
    s = capi.default_settings()
    assert isinstance(s, capi.SolverSettingsWithSharded) and s.halpern_sharded == 0
    s = capi.default_settings(halpern_sharded=1)
    assert s.halpern_sharded == 1 and s.halpern_lockstep_rays == 0 and s.halpern_infeasibility == 0 and s.halpern_lockstep == 0
    assert ctypes.c_int.from_buffer(s, field.offset).value == 1
    s.halpern_lockstep_rays = 1  # (neighbours: neither write reaches the other)
    s.halpern_sharded = 0
    assert s.halpern_lockstep_rays == 1 and s.halpern_sharded == 0


def test_the_library_writes_the_default_where_the_mirror_reads_it():
    s = capi.SolverSettingsWithSharded()
    s.halpern_sharded = 7  # (cuoptamd_default_settings must put its 0 at this offset)
    s.halpern_lockstep_rays = 7
    capi.lib.cuoptamd_default_settings(ctypes.byref(s))
    assert s.halpern_sharded == 0 and s.halpern_lockstep_rays == 0


def test_the_string_parameter_accepts_zero_and_one_only():
    assert lp.CUOPT_AMD_HALPERN_SHARDED == "amd_halpern_sharded"
    st = capi.Settings()
    try:
        assert int(st.get(lp.CUOPT_AMD_HALPERN_SHARDED)) == 0
        st.set(lp.CUOPT_AMD_HALPERN_SHARDED, "1")
        assert int(st.get(lp.CUOPT_AMD_HALPERN_SHARDED)) == 1
        assert int(st.get(lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS)) == 0 and int(st.get(lp.CUOPT_AMD_HALPERN_INFEASIBILITY)) == 0
        st.set(lp.CUOPT_AMD_HALPERN_SHARDED, 0)
        for bad in ("2", "-1"):
            with pytest.raises(capi.CuOptError):
                st.set(lp.CUOPT_AMD_HALPERN_SHARDED, bad)
    finally:
        st.close()


def test_the_python_mirror_validates_and_keeps_the_parameter():
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_SHARDED) == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            settings.set_parameter(lp.CUOPT_AMD_HALPERN_SHARDED, bad)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_SHARDED, 1)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_SHARDED) == 1
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_SHARDED] == 1
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_LOCKSTEP_RAYS] == 0
