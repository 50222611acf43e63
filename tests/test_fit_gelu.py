"""tools/fit_gelu.py on the CPU: the coefficients pasted into csrc/device_utils.h are the ones the script records, the fit
reproduces them, and their float32-emulated error against float64 GELU is within 3e-7."""
import importlib.util
import os
import re

from conftest import ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("fit_gelu", os.path.join(ROOT, "tools", "fit_gelu.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_committed_coefficients_error_and_source():
    t = _tool()
    assert len(t.COMMITTED) == 7
    assert t.max_error(t.from_bits(t.COMMITTED)) <= 3e-7
    src = open(os.path.join(ROOT, "state_policy_diffusionmodel_amd", "csrc", "device_utils.h")).read()
    body = src[src.index("float gelu_erf(float v)"):]
    body = body[:body.index("\n}\n")]
    pasted = tuple(int(h, 16) for h in re.findall(r"0x([0-9a-f]{8})u", body))
    assert pasted == tuple(t.COMMITTED), (pasted, t.COMMITTED)


def test_fit_regenerates_coefficients_of_the_same_quality():
    t = _tool()
    coef = t.fit()
    assert t.max_error(coef) <= 3e-7
    # (the least-squares solve may differ in the last bits between LAPACK builds; a flipped float32 rounding of one coefficient moves E by up to 1e-6 on [0, 6])
    import numpy as np
    x = np.linspace(0.0, 6.0, 601)
    assert np.max(np.abs(np.polyval(coef.astype(np.float64), x) - np.polyval(t.from_bits(t.COMMITTED).astype(np.float64), x))) <= 1e-5
