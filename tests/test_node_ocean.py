"""planet_heightmap_generation_amd/js/ocean.js under Node: the reference module's export names and result keys (recorded in the
golden's metadata), computeOceanCurrents through the addon against the config-1 golden by both routes (GPU), and, without a
device, the same error as the other modules throw."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import ocean_common as OC
from conftest import REPO

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
DRIVER = REPO / "tests" / "node" / "run_ocean.mjs"
pytestmark = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")


def run_ocean(tmp, case):
    for k in ("off", "adj", "xyz", "e", "plate", "ocean"):
        case[k].tofile(tmp / f"{k}.bin")
    for k in OC.WIND_INPUTS:
        np.ascontiguousarray(case["wind"][k]).tofile(tmp / f"wind_{k}.bin")
    (tmp / "ocean_job.json").write_text(json.dumps(dict(numRegions=case["N"], seed=case["seed"], wind={k: f"wind_{k}.bin" for k in OC.WIND_INPUTS},
                                                        **{k: f"{k}.bin" for k in ("off", "adj", "xyz", "e", "plate", "ocean")})))
    r = subprocess.run([NODE, "--no-warnings", str(DRIVER), str(tmp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads((tmp / "ocean_result.json").read_text())


def check_surface(res, meta):
    assert res["exports"] == meta["exports"] == ["computeOceanCurrents"]
    assert res["badWind"]["name"] == "RangeError" and "r_lon" in res["badWind"]["message"]
    assert res["badLand"]["name"] == "RangeError" and "r_isLand" in res["badLand"]["message"]


def test_surface_and_no_device_error(tmp_path):
    """The argument checks come before any device work; without a device computeOceanCurrents throws the Error every device call of
    the other modules throws (tests/test_node_host.py: 'no usable HIP device')."""
    case = OC.golden_case("ocean_N2000_ocean_s1")
    res = run_ocean(tmp_path, case)
    check_surface(res, case["meta"])
    if res["deviceCount"] == 0:
        assert res["threw"] and res["threw"]["name"] == "Error" and "no usable HIP device" in res["threw"]["message"]
    else:
        assert res["threw"] is None


@pytest.mark.gpu
def test_compute_ocean_currents_through_the_addon(tmp_path):
    case = OC.golden_case("ocean_config1_N10000_s1")
    meta = case["meta"]
    res = run_ocean(tmp_path, case)
    check_surface(res, meta)
    assert res["threw"] is None, res["threw"]
    assert res["noWind"] is not None and "no wind result" in res["noWind"]["message"]
    for tag in ("resident", "passed"):
        assert res[tag]["keys"] == [k for k in meta["keys"] if k != "_oceanTiming"]
        assert res[tag]["arrays"] == meta["arrays"]
        got = {k: np.fromfile(tmp_path / f"ocean_{tag}_{k}.bin", ty) for k, ty in OC.result_fields()}
        OC.assert_golden(f"js/ocean.js computeOceanCurrents ({tag} wind)", got, case)
