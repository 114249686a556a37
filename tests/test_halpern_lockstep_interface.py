"""The opt-in of the Halpern lockstep batch through the interfaces (no GPU needed): cuoptamd_settings::halpern_lockstep, the string
parameter CUOPT_AMD_HALPERN_LOCKSTEP of the C API's registry, and the Python mirror's pass-through."""
import pytest

from cuopt_amd import capi
from cuopt_amd import linear_programming as lp


def test_the_settings_field_is_appended_and_defaults_to_zero():
    fields = [f for f, _ in capi.SolverSettings._fields_]
    assert fields[-2:] == ["halpern_batch", "halpern_lockstep"]
    s = capi.default_settings()
    assert s.halpern_lockstep == 0 and s.halpern_batch == 0
    assert capi.default_settings(halpern_lockstep=1).halpern_lockstep == 1


def test_the_string_parameter_accepts_zero_and_one_only():
    assert lp.CUOPT_AMD_HALPERN_LOCKSTEP == "amd_halpern_lockstep"
    st = capi.Settings()
    try:
        st.set(lp.CUOPT_AMD_HALPERN_LOCKSTEP, "1")
        st.set(lp.CUOPT_AMD_HALPERN_LOCKSTEP, "0")
        for bad in ("2", "-1"):
            with pytest.raises(capi.CuOptError):
                st.set(lp.CUOPT_AMD_HALPERN_LOCKSTEP, bad)
    finally:
        st.close()


def test_the_python_mirror_validates_and_keeps_the_parameter():
    settings = lp.SolverSettings()
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP) == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            settings.set_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP, bad)
    settings.set_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP, 1)
    assert settings.get_parameter(lp.CUOPT_AMD_HALPERN_LOCKSTEP) == 1
    assert settings.toDict()[lp.CUOPT_AMD_HALPERN_LOCKSTEP] == 1
