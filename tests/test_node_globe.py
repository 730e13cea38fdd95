"""The worker's exportGlobe command (planet_heightmap_generation_amd/js/planet-worker.js) and js/globe-export.js under Node:
importHeightmap -> computeClimate -> exportGlobe of the default view, one layer, koppen and `plates`, each with both line sets, as GLB
bytes against the Python path's bytes on the same planet, each parsed back to its arrays; the error answers; an old exportMap
command, which answers as before; and the module's own functions against the emulator."""
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
LAYER, WIDTH = "tempSummer", 256


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_worker_export_globe(tmp_path):
    import import_common as IC
    from planet_heightmap_generation_amd import globe_export as GE, heightmap_import as HI, map_export as ME, sphere_mesh as SM
    g = IC.golden()
    imp = IC.meta(g)["import"]
    img = g["img_512x256"]
    img.tofile(tmp_path / "img.bin")
    small, sxyz = MC.golden_mesh("mesh_N2000_s1")
    se, ssp = GC.rough_elevation(sxyz, 4), GC.sector_plates(sxyz)
    se[~np.isfinite(se)] = 0.25                               # finite bounds: the module's mesh goes into a GLB
    splate = (np.arange(small.numRegions) % 5 * 11).astype(np.int32)
    sseeds, socean = [0, 11, 22, 33], [11, 33]                # plate 44 has no colour
    for k, a in (("off", small.adjOffset), ("adj", small.adjList), ("xyz", sxyz), ("tri", small.triangles), ("he", small.halfedges), ("e", se), ("sp", ssp), ("plate", splate)):
        np.ascontiguousarray(a).tofile(tmp_path / f"small_{k}.bin")

    # the same planet through the Python path first: its super-plate field goes to the worker
    keep = []
    d = HI.import_heightmap(imp["N"], imp["jitter"], img, img.shape[1], img.shape[0], imp["params"], seed=imp["seed"], planet_out=keep)
    pl = keep[0]
    try:
        mesh = SM.sphere_mesh_from_triangles(d["triangles"], d["halfedges"], d["numRegions"])
        sp = GC.sector_plates(d["r_xyz"], 7)
        sp[11] = np.nan
        sp.tofile(tmp_path / "sp.bin")
        MC.climate_chain(pl, d["r_plate"], d["plateIsOcean"], d["seed"])
        seeds = [int(s) for s in d["plateSeeds"]]
        plates = dict(r_plate=d["r_plate"], plateSeeds=seeds, plateColors=GE.compute_plate_colors(seeds, d["plateIsOcean"]))
        want = {"default": GE.export_globe(pl, mesh, "color", imp["seed"], wireframe=True, super_plates=sp),
                "layer": GE.export_globe(pl, mesh, LAYER, imp["seed"], wireframe=True, super_plates=sp),
                "koppen": GE.export_globe(pl, mesh, "koppen", imp["seed"], wireframe=True, super_plates=sp),
                "plates": GE.export_globe(pl, mesh, "plates", imp["seed"], plates=plates, wireframe=True, super_plates=sp)}
        plain = ME.export_map(pl, mesh, ["color", "koppen"], WIDTH)
    finally:
        pl.close()

    (tmp_path / "globe_job.json").write_text(json.dumps(dict(
        N=imp["N"], jitter=imp["jitter"], seed=imp["seed"], W=int(img.shape[1]), H=int(img.shape[0]), image="img.bin", params=imp["params"], width=WIDTH, layer=LAYER,
        superPlates="sp.bin", small=dict(numRegions=small.numRegions, seeds=sseeds, ocean=socean, **{k: f"small_{k}.bin" for k in ("off", "adj", "xyz", "tri", "he", "e", "sp", "plate")}))))
    r = subprocess.run([NODE, "--no-warnings", str(REPO / "tests" / "node" / "run_globe.mjs"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads((tmp_path / "globe_result.json").read_text())

    assert out["filename"] == GE.globe_filename("koppen", 7)
    assert out["imported"]["type"] == "done" and out["climate"]["type"] == "climateDone", (out["imported"], out["climate"])
    # a climate layer before computeClimate
    assert out["noWind"]["type"] == "error" and "no wind result" in out["noWind"]["message"] and "wo_compute_wind first" in out["noWind"]["message"], out["noWind"]
    # the GLB bytes of the four views are the Python path's, and each parses back to its arrays
    names = {"default": "color", "layer": LAYER, "koppen": "koppen", "plates": "plates"}
    for tag, view in names.items():
        o = out[tag + "Glb"]
        assert o["type"] == "globeDone" and o["keys"] == ["type", "view", "filename", "numSides", "bounds", "glb", "_globeTiming"], o
        assert o["view"] == view and o["filename"] == GE.globe_filename(view, imp["seed"]) == want[tag]["filename"] and o["kinds"] == {"glb": "Uint8Array"}
        assert o["progress"] == [[0, "Building globe..."], [90, "Done"]] and o["numSides"] == mesh.triangles.size
        data = (tmp_path / f"{tag}_glb.glb").read_bytes()
        assert data == want[tag]["glb"], tag
        arrays = GC.parse_glb(data)["arrays"]
        assert len(arrays) == 4
        for a, k in zip(arrays, ("position", "color", "wireframe", "superPlateBorders")):
            assert np.array_equal(bits(a), bits(want[tag][k])), (tag, k)
    assert len({want[t]["color"].tobytes() for t in want}) == 4 and len({want[t]["position"].tobytes() for t in want}) == 1
    # the arrays instead of the file
    a = out["arrays"]
    assert a["keys"] == ["type", "view", "filename", "numSides", "bounds", "position", "color", "wireframe", "superPlateBorders", "_globeTiming"]
    assert a["kinds"] == {k: "Float32Array" for k in ("position", "color", "wireframe", "superPlateBorders")}
    for k in ("position", "color", "wireframe", "superPlateBorders"):
        assert np.array_equal(np.fromfile(tmp_path / f"arrays.{k}", np.uint32), bits(want["layer"][k])), k
    assert np.array_equal(np.array(a["bounds"], np.float32), want["layer"]["bounds"])
    assert out["bare"]["keys"] == ["type", "view", "filename", "numSides", "bounds", "position", "color", "_globeTiming"] and out["bare"]["view"] == "color"
    assert np.array_equal(np.fromfile(tmp_path / "bare.color", np.uint32), bits(want["default"]["color"]))
    assert out["generic"]["type"] == "globeDone" and out["generic"]["view"] == "erosionDelta"
    # the error answers
    assert out["unknownLayer"]["type"] == "error" and out["unknownLayer"]["message"].startswith("exportGlobe: unknown map layer 'stress' (one of continentality, ")
    assert out["landmask"]["type"] == "error" and "unknown globe view 'landmask'" in out["landmask"]["message"]
    assert out["noSuperPlates"]["type"] == "error" and "no superPlates" in out["noSuperPlates"]["message"]
    assert out["disposed"] == "disposed" and (out["afterDispose"]["type"], out["afterDispose"]["message"]) == ("error", "No retained state for exportGlobe")
    # an old exportMap command returns what it returned before
    assert out["oldMap"]["type"] == "exportDone" and out["oldMap"]["keys"] == ["type", "width", "height", "maps", "_exportTiming"]
    assert out["oldMap"]["maps"] == [[t, ME.export_filename(t, imp["seed"])] for t in ("color", "koppen")]
    assert out["oldMap"]["progress"] == [[0, "Rendering..."], [40, "Rendering..."], [80, "Rendering..."]]
    for t in ("color", "koppen"):
        assert np.array_equal(np.fromfile(tmp_path / f"oldmap_{t}.rgba", np.uint8).reshape(WIDTH // 2, WIDTH, 4), plain["maps"][t]), t

    # the module's own functions on the 2 000-cell mesh against the emulator
    tri, he = small.triangles, small.halfedges
    rd = lambda name: np.fromfile(tmp_path / f"module.{name}", np.float32)  # noqa: E731
    pos, _ = GC.emu_positions(sxyz, se, tri, he)
    assert MC.same_bits(rd("position"), pos) and MC.same_bits(rd("bounds"), GC.emu_bounds(pos))
    assert MC.same_bits(rd("color"), GC.emu_view_colors("heightmap", se, tri, small.adjOffset, small.adjList))
    assert MC.same_bits(rd("layer"), GC.emu_view_colors("precipWinter", se, tri, small.adjOffset, small.adjList, a=ssp))
    assert MC.same_bits(rd("wireframe"), GC.emu_lines(GC.WIREFRAME, sxyz, se, tri, he)[0])
    assert MC.same_bits(rd("borders"), GC.emu_lines(GC.BORDERS, sxyz, se, tri, he, ssp)[0])
    table = GE.compute_plate_colors(sseeds, socean)
    assert MC.same_bits(rd("plates"), GC.emu_colors(tri, GC.emu_plate_colors(splate, sseeds, table)))
    assert (tmp_path / "module.glb").read_bytes() == GE.encode_glb(dict(position=pos, color=rd("color"), bounds=GC.emu_bounds(pos)))
    t = out["threw"]
    assert "landmask" in t["landmask"] and "no wind result" in t["noWind"] and "colour table" in t["noTable"], t
