"""planet_heightmap_generation_amd/js/precipitation.js under Node: the reference module's export names and result keys (recorded in
the golden's metadata), the argument checks before any device work, computePrecipitation through the addon against the config-1
golden by both routes (GPU), and, without a device, the same error as the other modules throw."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import precip_common as PC
from conftest import REPO

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
DRIVER = REPO / "tests" / "node" / "run_precip.mjs"
pytestmark = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")


def run_precip(tmp, case):
    for k in ("off", "adj", "xyz", "e", "plate", "ocean"):
        case[k].tofile(tmp / f"{k}.bin")
    for k in PC.WIND_INPUTS:
        np.ascontiguousarray(case["wind"][k]).tofile(tmp / f"wind_{k}.bin")
    for k in PC.OCEAN_INPUTS:
        np.ascontiguousarray(case["warm"][k]).tofile(tmp / f"warm_{k}.bin")
    (tmp / "precip_job.json").write_text(json.dumps(dict(numRegions=case["N"], seed=case["seed"], wind={k: f"wind_{k}.bin" for k in PC.WIND_INPUTS},
                                                         warm={k: f"warm_{k}.bin" for k in PC.OCEAN_INPUTS},
                                                         **{k: f"{k}.bin" for k in ("off", "adj", "xyz", "e", "plate", "ocean")})))
    r = subprocess.run([NODE, "--no-warnings", str(DRIVER), str(tmp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads((tmp / "precip_result.json").read_text())


def check_surface(res, meta):
    assert res["exports"] == meta["exports"] == ["computePrecipitation"]
    assert res["arity"] == 5                                # five parameters before the two with defaults, as in the reference
    assert res["badWind"]["name"] == "RangeError" and "r_pressure_winter" in res["badWind"]["message"]
    assert res["badCoast"]["name"] == "RangeError" and "r_coastDistLand" in res["badCoast"]["message"]
    assert res["badOcean"]["name"] == "RangeError" and "r_ocean_warmth_winter" in res["badOcean"]["message"]
    assert res["badElevation"]["name"] == "RangeError" and "r_elevation" in res["badElevation"]["message"]


def test_surface_and_no_device_error(tmp_path):
    """The argument checks come before any device work; without a device computePrecipitation throws the Error every device call of
    the other modules throws (tests/test_node_host.py: 'no usable HIP device')."""
    case = PC.golden_case("precip_N2000_ocean_s1")
    res = run_precip(tmp_path, case)
    check_surface(res, case["meta"])
    if res["deviceCount"] == 0:
        assert res["threw"] and res["threw"]["name"] == "Error" and "no usable HIP device" in res["threw"]["message"]
    else:
        assert res["threw"] is None


@pytest.mark.gpu
def test_compute_precipitation_through_the_addon(tmp_path):
    case = PC.golden_case("precip_config1_N10000_s1")
    meta = case["meta"]
    res = run_precip(tmp_path, case)
    check_surface(res, meta)
    assert res["threw"] is None, res["threw"]
    assert res["noWind"] is not None and "no wind result" in res["noWind"]["message"]
    assert res["noOcean"] is not None and "no ocean result" in res["noOcean"]["message"]
    for tag in ("resident", "passed"):
        assert res[tag]["keys"] == [k for k in meta["keys"] if k != "_precipTiming"]
        assert res[tag]["arrays"] == meta["arrays"]
        got = {k: np.fromfile(tmp_path / f"precip_{tag}_{k}.bin", np.float32) for k in PC.RESULT_KEYS}
        PC.assert_golden(f"js/precipitation.js computePrecipitation ({tag} wind and ocean results)", got, case)
