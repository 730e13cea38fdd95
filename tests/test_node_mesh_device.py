"""The device mesh builder under Node (planet_heightmap_generation_amd/js): js/sphere-mesh.js's buildSphere with a context against
without at N = 2 000, with and without the reference's pole-fan numbering; the shim's refusals; and the worker's `generate` with
deviceMesh: true against without on generate_N5000_s3_P6's message: the same `done` fields, the same stage names."""
import json
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")]
N, JITTER, SEED = 2000, 0.75, 3
MESH = ("triangles", "halfedges", "adjOffset", "adjList", "_adjTriList")
GEN = ("triangles", "halfedges", "r_xyz", "t_xyz", "r_plate", "prePostElev", "r_elevation", "t_elevation", "r_stress", "plateSeeds", "plateIsOcean",
       "mountain_r", "coastline_r", "ocean_r")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mesh_device_node")
    message = json.loads(bytes(load_golden("generate_N5000_s3_P6")["meta_json"]).decode())["message"]
    (tmp / "mesh_job.json").write_text(json.dumps(dict(N=N, jitter=JITTER, seed=SEED, message=message)))
    r = subprocess.run([NODE, "--no-warnings", str(REPO / "tests" / "node" / "run_mesh_device.mjs"), str(tmp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return tmp, json.loads((tmp / "mesh_result.json").read_text())


@pytest.mark.parametrize("tag", ["plain", "closure"])
def test_build_sphere_with_a_context(run, tag):
    from planet_heightmap_generation_amd import sphere_mesh as SM
    tmp, out = run
    m = out["module"][tag]
    assert m["hostKeys"] == ["mesh", "r_xyz"] and m["deviceKeys"] == ["mesh", "r_xyz", "neighborDist"]
    assert m["meshType"] == "SphereMesh" and m["numRegions"] == N + 1 and m["numSides"] == 3 * (2 * (N + 1) - 4) and m["numTriangles"] == 2 * (N + 1) - 4
    assert m["types"] == {k: "Int32Array" for k in MESH} and m["distType"] == "Float32Array"
    assert m["circulate"][0] == m["circulate"][1] and len(m["circulate"][0]) >= 3
    for k in MESH + ("xyz", "dist"):
        assert (tmp / f"dev_{tag}_{k}.bin").read_bytes() == (tmp / f"host_{tag}_{k}.bin").read_bytes(), k
    # and both are the Python binding's host route
    mesh, xyz, nd = SM.build_sphere(N, JITTER, SEED, reference_closure=(tag == "closure"))
    for k, a in (("triangles", mesh.triangles), ("halfedges", mesh.halfedges), ("adjOffset", mesh.adjOffset), ("adjList", mesh.adjList), ("_adjTriList", mesh.adjTriList),
                 ("xyz", xyz), ("dist", nd)):
        assert (tmp / f"dev_{tag}_{k}.bin").read_bytes() == np.ascontiguousarray(a).tobytes(), k


def test_shim_refusals(run):
    e = run[1]["errors"]
    assert e["noContext"].startswith("TypeError") and "context" in e["noContext"]
    assert e["xyzType"].startswith("TypeError") and e["xyzLength"].startswith("RangeError") and e["tooFew"].startswith("RangeError")
    assert e["duplicate"].startswith("Error: sphereMeshDevice: sphere_delaunay: star construction failed")


def test_worker_generate_with_device_mesh(run):
    tmp, out = run
    w = out["worker"]
    assert all(w[t]["type"] == "done" for t in ("host", "device", "off")), [w[t].get("message") for t in w]
    assert w["device"]["keys"] == w["host"]["keys"] and w["device"]["stages"] == w["host"]["stages"] and w["device"]["params"] == w["host"]["params"]
    assert w["device"]["stages"][:3] == ["Sphere mesh (Fibonacci + Delaunay + pole)", "Neighbor distances", "Triangle centers"]
    for k in GEN:
        want = (tmp / f"gen_host_{k}.bin").read_bytes()
        assert (tmp / f"gen_device_{k}.bin").read_bytes() == want and (tmp / f"gen_off_{k}.bin").read_bytes() == want, k
    print("worker _pipelineTiming (ms), host mesh:", [(s["stage"], round(s["ms"], 2)) for s in w["host"]["pipeline"][:3]],
          "device mesh:", [(s["stage"], round(s["ms"], 2)) for s in w["device"]["pipeline"][:3]])
    assert out["disposed"] == "disposed"
