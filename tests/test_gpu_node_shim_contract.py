"""The contract of the N-API shim (planet_heightmap_generation_amd/napi/worogen_napi.cc) behind the planet handle, on one context
and one planet built from tests/golden/mesh_N2000_s1.npz: every throw site behind the planet check, each case wrong in exactly one
thing (region arrays too short, of another class or missing, with their `what` texts; the plate tables; result keys; the integer
ranges; the communicator and flood-exchange checks), the successes of the bodies that the entry points share (the five rasters, the
three mapColor* calls, the relief read-backs, both mesh-device calls, the ocean-mask passes and erodeComposite, the copied-out
results), and the dead handle after planetDestroy.

tests/node/run_shim_contract.mjs gives for each case [errorClass, message] or the shape of what was returned, and for the successes
the FNV-1a hash of every returned buffer and the value of every number, so that two arguments swapped in a shared body cannot pass.
tests/node/shim_contract_expected.json holds what the addon built from the commit BEFORE the shim was rewritten gave for the same
cases; two consecutive runs of that addon agreed on every case, hashes included."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import map_common as MC
from conftest import REPO, load_golden
from test_node_shim_contract import differences

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
DRIVER = REPO / "tests" / "node" / "run_shim_contract.mjs"
EXPECTED = REPO / "tests" / "node" / "shim_contract_expected.json"
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("shim_contract")
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    for name, a, ty in (("off", mesh.adjOffset, np.int32), ("adj", mesh.adjList, np.int32), ("tri", mesh.triangles, np.int32), ("he", mesh.halfedges, np.int32),
                        ("xyz", xyz, np.float32), ("nd", load_golden("mesh_N2000_s1")["ref_neighborDist"], np.float32)):
        np.ascontiguousarray(a, ty).tofile(tmp / f"{name}.bin")
    r = subprocess.run([NODE, "--no-warnings", str(DRIVER), "gpu", str(tmp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout), json.loads(EXPECTED.read_text())["gpu"]


def test_outcomes_behind_the_planet_handle_are_the_parents(table):
    got, want = table
    bad = differences(got, want)
    assert not bad, "\n".join(bad[:40])


def test_the_table_covers_what_it_is_there_for(table):
    got, want = table
    thrown = [v["thrown"] for v in want.values() if "thrown" in v]
    dead = [k for k in want if k.startswith("dead planet: ")]
    assert len(dead) == 65 + 9 and all(want[k] == {"thrown": ["TypeError", "expected a planet handle"]} for k in dead)   # the 65 of the null sweep and the 9 that check arrays first
    assert want["planetDestroy, again"] == {"ret": "undefined"}
    assert sum(1 for v in want.values() if "#" in json.dumps(v.get("ret", ""))) >= 50                                         # hashed successes
    for text in ("r_elevation length must equal mesh.numRegions", "r_isOcean length mismatch", "r_hotspot length must equal mesh.numRegions",
                 "computeWind: r_plate must be an Int32Array", "computeGradients: nine Float32Arrays of numRegions entries", "r_superPlate length mismatch",
                 "plate table: expected typed arrays", "plate table: wrong array type or length", "noise tables must have 512 entries",
                 "expected a result key (string)", "windUpload: expected a Float32Array, Int32Array or Uint8Array", "coarse mesh arrays do not match",
                 "planetExchangeNeighbors: expected a communicator handle", "planetSetFloodExchange: r_isOcean length must equal mesh.numRegions"):
        assert any(t[1] == text for t in thrown), text
