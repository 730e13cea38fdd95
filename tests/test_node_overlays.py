"""The worker's overlay requests (planet_heightmap_generation_amd/js/planet-worker.js, js/overlay-export.js) under Node:
importHeightmap -> computeClimate -> exportGlobe with arrows, ITCZ line and grid as GLB bytes against the Python path's bytes on the
same planet; exportOverlays against the Python arrays; the error answers before computeClimate; and old exportGlobe and exportMap
messages, which answer as before."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import globe_common as GC
import map_common as MC
from conftest import REPO

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")]
LAYER, WIDTH, GRID, GRID2, CENTER = "windSpeedSummer", 256, 30, 22.5, 0.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_worker_overlays(tmp_path):
    import import_common as IC
    from planet_heightmap_generation_amd import globe_export as GE, heightmap_import as HI, map_export as ME, overlay_export as OE, sphere_mesh as SM
    g = IC.golden()
    imp = IC.meta(g)["import"]
    img = g["img_512x256"]
    img.tofile(tmp_path / "img.bin")
    keep = []
    d = HI.import_heightmap(imp["N"], imp["jitter"], img, img.shape[1], img.shape[0], imp["params"], seed=imp["seed"], planet_out=keep)
    pl = keep[0]
    try:
        mesh = SM.sphere_mesh_from_triangles(d["triangles"], d["halfedges"], d["numRegions"])
        MC.climate_chain(pl, d["r_plate"], d["plateIsOcean"], d["seed"])
        want = GE.export_globe(pl, mesh, LAYER, imp["seed"], wireframe=True, wind_arrows="summer", ocean_current_arrows="winter", itcz="summer", grid=GRID)
        old = GE.export_globe(pl, mesh, "color", imp["seed"], wireframe=True)
        overlays = dict(windArrows=OE.wind_arrows(pl, "summer", CENTER), oceanCurrentArrows=OE.ocean_current_arrows(pl, "winter", CENTER), itcz=OE.itcz(pl, "winter"),
                        grid=OE.grids(GRID2, CENTER))
        plain = ME.export_map(pl, mesh, ["color"], WIDTH)
    finally:
        pl.close()
    (tmp_path / "overlays_job.json").write_text(json.dumps(dict(N=imp["N"], jitter=imp["jitter"], seed=imp["seed"], W=int(img.shape[1]), H=int(img.shape[0]), image="img.bin",
                                                                params=imp["params"], width=WIDTH, layer=LAYER, grid=GRID, grid2=GRID2, centerLon=CENTER)))
    r = subprocess.run([NODE, "--no-warnings", str(REPO / "tests" / "node" / "run_overlays.mjs"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads((tmp_path / "overlays_result.json").read_text())
    rd = lambda name, ty=np.uint32: np.fromfile(tmp_path / name, ty)  # noqa: E731
    assert out["imported"]["type"] == "done" and out["climate"]["type"] == "climateDone", (out["imported"], out["climate"])

    # before computeClimate: the arrows and the ITCZ line have nothing to read, the grid needs nothing
    assert out["noWind"]["type"] == "error" and "no wind result" in out["noWind"]["message"] and "wo_compute_wind first" in out["noWind"]["message"], out["noWind"]
    assert out["noOcean"]["type"] == "error" and "no ocean result" in out["noOcean"]["message"], out["noOcean"]
    assert out["noWindGlobe"]["type"] == "error" and "no wind result" in out["noWindGlobe"]["message"], out["noWindGlobe"]
    assert out["noItcz"]["type"] == "error" and "no wind result" in out["noItcz"]["message"], out["noItcz"]
    assert out["gridOnly"]["type"] == "overlaysDone" and out["gridOnly"]["keys"] == ["type", "centerLon", "grid", "_overlayTiming"]
    assert np.array_equal(rd("gridonly.grid.globe"), bits(OE.globe_grid(GRID))) and np.array_equal(rd("gridonly.grid.map"), bits(OE.map_grid(GRID, 0)))

    # exportGlobe with every overlay: the Python path's GLB bytes, and they parse back to the arrays
    o = out["glb"]
    assert o["type"] == "globeDone" and o["keys"] == ["type", "view", "filename", "numSides", "bounds", "glb", "_globeTiming"] and o["kinds"] == {"bounds": "Float32Array", "glb": "Uint8Array"}
    data = (tmp_path / "glb.glb").read_bytes()
    assert data == want["glb"]
    parsed = GC.parse_glb(data)
    names = [p.get("extras", {}).get("name") for p in parsed["json"]["meshes"][0]["primitives"]]
    assert names == [None, "wireframe", "windArrows", "oceanCurrentArrows", "itcz", "grid"] and len(parsed["arrays"]) == 9
    assert want["windArrows"]["position"].size > 18 * 500 and want["oceanCurrentArrows"]["position"].size > 18 * 500
    a = out["arrays"]
    assert a["keys"] == ["type", "view", "filename", "numSides", "bounds", "position", "color", "wireframe", "itcz", "grid", "windArrows", "oceanCurrentArrows", "_globeTiming"]
    for k in ("position", "color", "wireframe", "itcz", "grid"):
        assert np.array_equal(rd(f"arrays.{k}"), bits(want[k])), k
    for k in ("windArrows", "oceanCurrentArrows"):
        for part in ("position", "color"):
            assert np.array_equal(rd(f"arrays.{k}.{part}"), bits(want[k][part])), (k, part)

    # exportOverlays: both forms of everything, the Python arrays
    o = out["overlays"]
    assert o["type"] == "overlaysDone" and o["keys"] == ["type", "centerLon", "windArrows", "oceanCurrentArrows", "itcz", "grid", "_overlayTiming"] and o["centerLon"] == CENTER
    assert o["counts"] == {k: overlays[k]["count"] for k in ("windArrows", "oceanCurrentArrows")}
    assert set(o["kinds"].values()) == {"Float32Array"} and len(o["kinds"]) == 12
    for k in ("windArrows", "oceanCurrentArrows"):
        for form in ("globe", "map"):
            for part in ("position", "color"):
                assert np.array_equal(rd(f"overlays.{k}.{form}.{part}"), bits(overlays[k][form][part])), (k, form, part)
    for k in ("itcz", "grid"):
        for form in ("globe", "map"):
            assert np.array_equal(rd(f"overlays.{k}.{form}"), bits(overlays[k][form])), (k, form)
    assert out["badSeason"]["type"] == "error" and "'spring'" in out["badSeason"]["message"]
    assert out["badGrid"]["type"] == "error" and "grid spacing" in out["badGrid"]["message"]

    # old messages answer as before
    assert out["oldGlobe"]["keys"] == ["type", "view", "filename", "numSides", "bounds", "glb", "_globeTiming"] and (tmp_path / "oldglobe.glb").read_bytes() == old["glb"]
    assert out["oldGlobe"]["progress"] == [[0, "Building globe..."], [90, "Done"]]
    assert out["oldGlobeArrays"]["keys"] == ["type", "view", "filename", "numSides", "bounds", "position", "color", "wireframe", "_globeTiming"]
    assert out["oldMap"]["type"] == "exportDone" and out["oldMap"]["keys"] == ["type", "width", "height", "maps", "_exportTiming"]
    assert np.array_equal(rd("oldmap_color.rgba", np.uint8).reshape(WIDTH // 2, WIDTH, 4), plain["maps"]["color"])
    assert out["disposed"] == "disposed" and (out["afterDispose"]["type"], out["afterDispose"]["message"]) == ("error", "No retained state for exportOverlays")
