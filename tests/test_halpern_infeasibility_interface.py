"""The opt-in of infeasibility detection in reflected Halpern mode through the interfaces (no GPU needed):
cuoptamd_settings::halpern_infeasibility, the string parameter CUOPT_AMD_HALPERN_INFEASIBILITY of the C API's registry, and the Python
mirror's pass-through."""
import pytest

from cuopt_amd import capi
from cuopt_amd import linear_programming as lp


def test_the_settings_field_is_appended_behind_halpern_lockstep_and_defaults_to_zero():
    # (capi.SolverSettings ends at halpern_lockstep, as its own test pins it; the struct every call passes appends to it)
    assert issubclass(capi.SolverSettingsWithRays, capi.SolverSettings)
    assert [f for f, _ in capi.SolverSettingsWithRays._fields_] == ["halpern_infeasibility"]
    last, new = capi.SolverSettings.halpern_lockstep, capi.SolverSettingsWithRays.halpern_infeasibility
    assert new.offset == last.offset + last.size and isinstance(capi.default_settings(), capi.SolverSettingsWithRays)
    assert capi.default_settings().halpern_infeasibility == 0
    s = capi.default_settings(halpern_infeasibility=1)
    assert s.halpern_infeasibility == 1 and s.halpern_lockstep == 0 and s.detect_infeasibility == 0
    assert (s.primal_infeasible_tolerance, s.dual_infeasible_tolerance) == (1e-8, 1e-8)


def test_the_string_parameter_accepts_zero_and_one_only():
    assert lp.CUOPT_AMD_HALPERN_INFEASIBILITY == "amd_halpern_infeasibility"
    st = capi.Settings()
    try:
        assert int(st.get(lp.CUOPT_AMD_HALPERN_INFEASIBILITY)) == 0
        st.set(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, "1")
        assert int(st.get(lp.CUOPT_AMD_HALPERN_INFEASIBILITY)) == 1
        st.set(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, 0)
        for bad in ("2", "-1"):
            with pytest.raises(capi.CuOptError):
                st.set(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, bad)
    finally:
        st.close()


def test_the_python_mirror_validates_and_keeps_the_parameter():
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_INFEASIBILITY) == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            settings.set_parameter(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, bad)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_INFEASIBILITY, 1)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_INFEASIBILITY) == 1
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_INFEASIBILITY] == 1


def test_the_entry_points_are_exported():
    for name in ("cuoptamd_solver_get_ray", "pdlpdev_halpern_eval_infeasibility", "pdlpdev_halpern_get_ray", "pdlpdev_set_halpern_rays"):
        assert hasattr(capi.lib, name), name
