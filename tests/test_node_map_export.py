"""The worker's exportMap command (planet_heightmap_generation_amd/js/planet-worker.js) under Node: importHeightmap ->
computeClimate -> exportMap of all six kinds with PNG files, against the Python path on the same planet; progress, timing keys
and the error answers; a reapply followed by exportMap shows the re-eroded field."""
import json
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import map_common as MC
from conftest import REPO

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")]
WIDTH = 512
PARAMS2 = dict(terrainWarp=0.25, smoothing=0.30, glacialErosion=0.0, hydraulicErosion=0.20, thermalErosion=0.0, ridgeSharpening=0.10)


def png_pixels(data):
    """(width, height, RGBA bytes) of an 8-bit RGBA PNG whose rows all use filter 0"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(data):
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body)
        if kind == b"IHDR":
            size = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            idat += body
        at += 12 + n
    w, h = size[:2]
    assert size[2:] == (8, 6, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert np.all(rows[:, 0] == 0)
    return w, h, rows[:, 1:].reshape(h, w, 4)


def test_worker_export_map(tmp_path):
    import import_common as IC
    from planet_heightmap_generation_amd import heightmap_import as HI, map_export as ME, sphere_mesh as SM
    g = IC.golden()
    imp = IC.meta(g)["import"]
    img = g["img_512x256"]
    img.tofile(tmp_path / "img.bin")
    small, sxyz = MC.golden_mesh("mesh_N2000_s1")
    se = MC.fbm_like(sxyz, 4)
    for k, a in (("off", small.adjOffset), ("adj", small.adjList), ("xyz", sxyz), ("tri", small.triangles), ("he", small.halfedges), ("e", se)):
        np.ascontiguousarray(a).tofile(tmp_path / f"small_{k}.bin")
    (tmp_path / "map_job.json").write_text(json.dumps(dict(
        N=imp["N"], jitter=imp["jitter"], seed=imp["seed"], W=int(img.shape[1]), H=int(img.shape[0]), image="img.bin", params=imp["params"], params2=PARAMS2,
        width=WIDTH, types=list(MC.TYPES), small=dict(numRegions=small.numRegions, **{k: f"small_{k}.bin" for k in ("off", "adj", "xyz", "tri", "he", "e")}))))
    r = subprocess.run([NODE, "--no-warnings", str(REPO / "tests" / "node" / "run_map_export.mjs"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads((tmp_path / "map_result.json").read_text())

    # the four error answers, and the ones of the arguments
    for tag in ("nothingRetained", "afterDispose"):
        assert out[tag]["type"] == "error" and out[tag]["message"] == "No retained state for exportMap", out[tag]
    assert out["retained"] == out["retained2"] == "retained" and out["disposed"] == "disposed"
    assert out["noMesh"]["type"] == "error" and "mesh.triangles and mesh.halfedges" in out["noMesh"]["message"], out["noMesh"]
    assert out["noHalfedges"]["type"] == "error" and "mesh.halfedges" in out["noHalfedges"]["message"] and "triangles" not in out["noHalfedges"]["message"]
    assert out["imported"]["type"] == "done" and out["climate"]["type"] == "climateDone", (out["imported"], out["climate"])
    for tag in ("noKoppen", "noBiome"):
        assert out[tag]["type"] == "error" and "no Koppen result" in out[tag]["message"], out[tag]
    assert out["unknown"]["type"] == "error" and "plates" in out["unknown"]["message"] and "unknown map type" in out["unknown"]["message"]
    assert out["oddWidth"]["type"] == "error" and "width" in out["oddWidth"]["message"]

    # the answer's shape, progress and timing
    a = out["all"]
    assert a["type"] == "exportDone" and a["keys"] == ["type", "width", "height", "maps", "_exportTiming"] and (a["width"], a["height"]) == (WIDTH, WIDTH // 2)
    assert a["timingKeys"] == ["raster", "color", "encode", "workerTotal"] and all(isinstance(v, (int, float)) and v >= 0 for v in a["timing"].values())
    assert a["timing"]["encode"] > 0 and out["one"]["timing"]["encode"] == 0
    n = len(MC.TYPES)
    assert a["progress"] == [[0, "Rendering..."]] + [[80 * (k + 1) / n, "Rendering..."] for k in range(n)] + [[85, "Encoding PNG..."]]
    assert out["one"]["progress"] == [[0, "Rendering..."], [80, "Rendering..."]]
    assert [m["type"] for m in a["maps"]] == list(MC.TYPES)
    assert [m["filename"] for m in a["maps"]] == [ME.export_filename(t, imp["seed"]) for t in MC.TYPES]
    assert all(m["keys"] == ["type", "filename", "rgba", "png"] and m["rgba"] == "Uint8ClampedArray" and m["png"] == "Uint8Array" for m in a["maps"])
    assert out["one"]["maps"] == [dict(type="landmask", filename=ME.export_filename("landmask", imp["seed"]), keys=["type", "filename", "rgba"], rgba="Uint8ClampedArray", png=None)]
    print("worker _exportTiming (10 k cells, 512 x 256, six types, png):", a["timing"])

    # js/map-export.js's own exportMap / exportMapBatch on the 2 000-cell mesh against the emulator
    assert out["module"]["one"] == [128, 64, "Uint8ClampedArray"] and out["module"]["batch"] == [128, 64, ["color", "landmask"]]
    assert "no Koppen result" in out["module"]["noKoppen"]
    rm, _, _ = MC.emu_raster(sxyz, small.triangles, small.halfedges, 128)
    for t in ("heightmap", "color", "landmask"):
        got = np.fromfile(tmp_path / f"module_{t}.rgba", np.uint8).reshape(64, 128, 4)
        assert np.array_equal(got, MC.emu_rgba(t, se, np.zeros(se.size, np.uint8), small.adjOffset, small.adjList, rm)), t

    # the same planet through the Python path
    keep = []
    d = HI.import_heightmap(imp["N"], imp["jitter"], img, img.shape[1], img.shape[0], imp["params"], seed=imp["seed"], planet_out=keep)
    pl = keep[0]
    try:
        mesh = SM.sphere_mesh_from_triangles(d["triangles"], d["halfedges"], d["numRegions"])
        koppen = MC.climate_chain(pl, d["r_plate"], d["plateIsOcean"], d["seed"])
        assert np.array_equal(koppen, np.fromfile(tmp_path / "koppen.bin", np.uint8))
        want = ME.export_map(pl, mesh, MC.TYPES, WIDTH)
        for t in MC.TYPES:
            rgba = np.fromfile(tmp_path / f"all_{t}.rgba", np.uint8).reshape(WIDTH // 2, WIDTH, 4)
            assert np.array_equal(rgba, want["maps"][t]), t
            w, h, px = png_pixels((tmp_path / f"all_{t}.png").read_bytes())
            assert (w, h) == (WIDTH, WIDTH // 2) and np.array_equal(px, rgba), t
        # after a reapply with other sliders the export shows the re-eroded field
        re_e = np.fromfile(tmp_path / "re_elevation.bin", np.float32)
        assert out["reapply"] == "reapplyDone" and not np.array_equal(re_e, d["r_elevation"])
        assert out["afterReapply"]["type"] == "exportDone"
        for t in ("heightmap", "color"):
            rgba = np.fromfile(tmp_path / f"after_{t}.rgba", np.uint8).reshape(WIDTH // 2, WIDTH, 4)
            assert np.array_equal(rgba, ME.color(pl, t, re_e)), t
            assert not np.array_equal(rgba, want["maps"][t]), t
    finally:
        pl.close()
