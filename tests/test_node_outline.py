"""The outlines under Node: the shim's four entries (napi/worogen_napi.cc: outlineBuild, outlineDownload, outlinePositions,
outlineLonLat) are callable properties of the addon that are not enumerable, so the recorded export list of
tests/test_node_shim_contract.py stands, and their checks before the planet handle throw; and, on the device, the worker's
exportOutlines command (js/planet-worker.js, js/outline-export.js) answers in every format with the rings of the Python host on the
same planet, and exportGlobe with `outlines` gives one more LINES primitive whose floats are wo_outline_positions'."""
import json
import shutil
import struct
import subprocess

import numpy as np
import pytest

import outline_common as OC
from conftest import REPO

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
needs_node = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")
DRIVER = str(REPO / "tests" / "node" / "run_outlines.mjs")
WIDTH, CENTER, LEVELS = 512, 1.25, [-0.2, 0.0, 0.3]
INFO = ["boundarySides", "rings", "longestRing", "rounds", "launches"]

TYPED, ELEMENT, PLANET = ["TypeError", "expected a typed array"], ["TypeError", "typed array has the wrong element type"], ["TypeError", "expected a planet handle"]
EXPORT = dict(type="function", enumerable=False, writable=True, configurable=True, listed=False)
SHIM = {
    **{f"export {k}": EXPORT for k in ("outlineBuild", "outlineDownload", "outlinePositions", "outlineLonLat")},
    "outlineBuild()": {"thrown": TYPED}, "outlineBuild: halfedges of another type": {"thrown": ELEMENT},
    "outlineBuild: halfedges of another length": {"thrown": ["RangeError", "outlineBuild: triangles and halfedges must have the same length, numSides"]},
    "outlineBuild: no planet": {"thrown": PLANET}, "outlineDownload()": {"thrown": PLANET}, "outlinePositions({})": {"thrown": PLANET}, "outlineLonLat(null)": {"thrown": PLANET},
}


@needs_node
def test_outline_calls_of_the_shim_without_a_device():
    r = subprocess.run([NODE, "--no-warnings", DRIVER, "shim"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout)
    bad = [f"{k}: expected {json.dumps(SHIM.get(k))}, got {json.dumps(got.get(k))}" for k in list(SHIM) + [k for k in got if k not in SHIM] if got.get(k) != SHIM.get(k)]
    assert not bad, "\n".join(bad)


def glb_doc(data):
    """the JSON chunk of a binary glTF file"""
    magic, version, total = struct.unpack_from("<4sII", data, 0)
    n, kind = struct.unpack_from("<I4s", data, 12)
    assert magic == b"glTF" and version == 2 and total == len(data) and kind == b"JSON"
    return json.loads(bytes(data[20:20 + n]).decode("utf-8"))


def _arrays(tmp_path, tag):
    res = {f: np.fromfile(tmp_path / f"{tag}_{f}.bin", np.int32) for f in OC.FIELDS}
    res["lonlat"] = np.fromfile(tmp_path / f"{tag}_lonlat.bin", np.float64).reshape(-1, 2)
    return res


@needs_node
@pytest.mark.gpu
def test_worker_export_outlines_and_globe(tmp_path):
    import import_common as IC
    from planet_heightmap_generation_amd import globe_export as GE, heightmap_import as HI, outline_export as OE, sphere_mesh as SM
    g = IC.golden()
    imp = IC.meta(g)["import"]
    img = g["img_512x256"]
    img.tofile(tmp_path / "img.bin")
    (tmp_path / "outline_job.json").write_text(json.dumps(dict(
        N=imp["N"], jitter=imp["jitter"], seed=imp["seed"], W=int(img.shape[1]), H=int(img.shape[0]), image="img.bin", params=imp["params"], width=WIDTH, centerLon=CENTER,
        levels=LEVELS)))
    r = subprocess.run([NODE, "--no-warnings", DRIVER, "worker", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads((tmp_path / "outline_result.json").read_text())

    for tag in ("nothingRetained", "afterDispose"):
        assert out[tag]["type"] == "error" and out[tag]["message"] == "No retained state for exportOutlines", out[tag]
    assert out["imported"]["type"] == "done" and out["disposed"] == "disposed"
    E = out["errors"]
    assert all(v["type"] == "error" for k, v in E.items() if k != "noSuperPlates"), E
    assert "unknown outline source 'shore'" in E["badSource"]["message"] and "unknown format 'kml'" in E["badFormat"]["message"]
    assert "no Koppen result" in E["noKoppen"]["message"] and "no rivers result" in E["noRivers"]["message"]
    assert "levels[1] = 0.1" in E["descending"]["message"] and "onlyClass is -2" in E["onlyClass"]["message"]
    assert E["noSuperPlates"]["type"] in ("error", "outlinesDone") and "outlines take { source" in E["globeNoSource"]["message"]
    c = out["coast"]
    assert c["type"] == "outlinesDone" and c["keys"] == ["type", "source", "format"] + INFO + ["filename"] + list(OC.FIELDS) + ["lonlat", "_outlineTiming"]
    assert c["fields"] == {**{f: "Int32Array" for f in OC.FIELDS}, "lonlat": "Float64Array"} and c["progress"] == [[0, "Tracing outlines..."], [90, "Done"]]
    assert c["filename"] == f"orogen-outline-coast-{imp['seed']}.geojson" and out["coastSvg"]["filename"].endswith(".svg")
    assert all(out["afterErrors"][k] == c[k] for k in INFO)        # a refused request leaves the worker serving

    # the same planet through the Python host
    keep = []
    d = HI.import_heightmap(imp["N"], imp["jitter"], img, img.shape[1], img.shape[0], imp["params"], seed=imp["seed"], planet_out=keep)
    pl = keep[0]
    try:
        mesh = SM.sphere_mesh_from_triangles(d["triangles"], d["halfedges"], d["numRegions"])
        plain_py = GE.export_globe(pl, mesh, "color", imp["seed"], wireframe=True)["glb"]
        want = OE.build_outline(pl, mesh, "coast", want_lonlat=True)
        got = _arrays(tmp_path, "coast")
        OC.same_result(got, want)
        assert np.array_equal(got["lonlat"].view(np.uint64), want["lonlat"].view(np.uint64)) and all(c[k] == want["info"][k] for k in INFO)
        assert c["boundarySides"] > 100 and c["rings"] > 1
        assert json.loads((tmp_path / "coastGeojson.txt").read_text()) == json.loads(OE.to_geojson(want, {"source": "coast"}))
        assert (tmp_path / "coastSvg.txt").read_text() == OE.to_svg(want, WIDTH, CENTER)
        OC.same_result(_arrays(tmp_path, "plates"), OE.build_outline(pl, mesh, "values", values=d["r_plate"]))
        OC.same_result(_arrays(tmp_path, "levels"), OE.build_outline(pl, mesh, "levels", levels=LEVELS, only_class=1))
        assert out["plates"]["source"] == "plates" and out["levels"]["rings"] > 0
        # exportGlobe: without `outlines` the file it always gave, with it one more LINES primitive of the positions' floats
        plain = (tmp_path / "globePlain_glb.bin").read_bytes()
        assert plain == plain_py
        with_outlines = (tmp_path / "globeOutlines_glb.bin").read_bytes()
        py = GE.export_globe(pl, mesh, "color", imp["seed"], wireframe=True, outlines=dict(source="coast"))
        assert with_outlines == py["glb"]
        a, b = glb_doc(plain), glb_doc(with_outlines)
        pa, pb = a["meshes"][0]["primitives"], b["meshes"][0]["primitives"]
        assert len(pb) == len(pa) + 1 and pb[:-1] == pa and pb[-1]["mode"] == 1 and pb[-1]["extras"] == {"name": "outlines"}
        M = want["sides"].size
        assert b["accessors"][pb[-1]["attributes"]["POSITION"]]["count"] == 2 * M
        rings = OE.build_outline(pl, mesh, "coast", base=OE.GLOBE_BASE)
        segments = py["outlines"].reshape(M, 2, 3)
        follower = np.arange(M) + 1
        follower[rings["ring_start"][1:] - 1] = rings["ring_start"][:-1]
        assert np.array_equal(segments[:, 0].view(np.uint32), rings["xyz"].view(np.uint32)) and np.array_equal(segments[:, 1].view(np.uint32), rings["xyz"][follower].view(np.uint32))
        view = b["bufferViews"][b["accessors"][pb[-1]["attributes"]["POSITION"]]["bufferView"]]
        n_json = int.from_bytes(with_outlines[12:16], "little")
        floats = np.frombuffer(with_outlines, "<f4", 6 * M, 20 + n_json + 8 + view["byteOffset"])
        assert np.array_equal(floats.view(np.uint32), py["outlines"].view(np.uint32))
        only = OE.build_outline(pl, mesh, "coast", only_class=1, base=OE.GLOBE_BASE)
        assert out["globeArrays"]["outlines"] == "Float32Array" and "glb" not in out["globeArrays"]
        assert np.array_equal(np.fromfile(tmp_path / "globeArrays_outlines.bin", np.float32).view(np.uint32), OE.ring_segments(only).view(np.uint32))
    finally:
        pl.close()
