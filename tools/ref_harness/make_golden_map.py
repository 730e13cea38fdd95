#!/usr/bin/env python3
"""Generate tests/golden/map_N2000_s1.npz by running the REFERENCE's own exportMapBatch and colour functions
(js/planet-mesh.js:30-80, :1965-2180, js/color-map.js) under Node 12.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never
enter this repository.  The reference draws with three.js on a page; in the scratch copy only, stubs of our own stand in for both:
  * node_modules/three: Plane, Vector3, Scene, Color, Mesh, MeshBasicMaterial, OrthographicCamera, WebGLRenderTarget, DoubleSide,
    BufferAttribute, and a BufferGeometry whose setAttribute records the arrays it is given;
  * scene.js: a renderer with capabilities.maxTextureSize and no-op render / setRenderTarget / readRenderTargetPixels;
  * planet-mesh.js gets one appended line exporting its module-private colour functions;
run_map.mjs supplies window, navigator, location and a document whose canvas does nothing.  So nothing is drawn: the golden
holds what the reference hands to the renderer (the position array and, per type, the colour array) and what its functions
return, not pixels.  state.curData is the reference's own SphereMesh of tests/golden/mesh_N2000_s1.npz with an fbm elevation of
both signs and Koppen ids 0..30 by hash, made here from fixed seeds.  Running this again reproduces every array exactly.

Usage:  python tools/ref_harness/make_golden_map.py --ref <checkout of the reference>
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402
from planet_heightmap_generation_amd import capi  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_map.mjs"
N, SEED, WIDTH = 2000, 1, 64
TYPES = ("color", "heightmap", "landheightmap", "landmask", "biome", "koppen")

THREE_STUB = """// stub of three (golden generation only): nothing is drawn; BufferGeometry records what it is given
export const DoubleSide = 2;
export class Vector3 { constructor(x = 0, y = 0, z = 0) { this.x = x; this.y = y; this.z = z; } set(x, y, z) { this.x = x; this.y = y; this.z = z; return this; } }
export class Plane { constructor(normal, constant) { this.normal = normal; this.constant = constant; } }
export class Color { constructor(hex) { this.hex = hex; } }
export class Scene { constructor() { this.children = []; this.background = null; } add(o) { this.children.push(o); } remove(o) { this.children = this.children.filter((c) => c !== o); } }
export class BufferAttribute { constructor(array, itemSize) { this.array = array; this.itemSize = itemSize; } }
export class BufferGeometry {
    constructor() { this.attributes = {}; }
    setAttribute(name, attr) { this.attributes[name] = attr; globalThis.__woRecorded.push({ name, array: attr.array }); return this; }
    dispose() {}
}
export class MeshBasicMaterial { constructor(opts) { Object.assign(this, opts); } dispose() {} }
export class Mesh { constructor(geometry, material) { this.geometry = geometry; this.material = material; } }
export class OrthographicCamera { constructor(...a) { this.frustum = a; this.position = new Vector3(); } lookAt() {} }
export class WebGLRenderTarget { constructor(w, h) { this.width = w; this.height = h; } dispose() {} }
"""
SCENE_STUB = """// stub of scene.js (golden generation only): a renderer that draws nothing
export const renderer = { capabilities: { maxTextureSize: 16384 }, localClippingEnabled: false, render() {}, setRenderTarget() {}, readRenderTargetPixels() {} };
export const scene = { add() {}, remove() {} };
export const waterMesh = {}, atmosMesh = {}, starsMesh = {};
"""


def elevation(xyz: np.ndarray) -> np.ndarray:
    """fbm on the unit sphere scaled to reach both signs, the deep ocean and the peaks (our SimplexNoise on the host)."""
    L = capi.lib()
    perm, pm12 = np.empty(512, np.uint8), np.empty(512, np.uint8)
    capi.check(L.wo_noise_tables(11.0, capi.ptr(perm), capi.ptr(pm12)), "wo_noise_tables")
    out = np.empty(1, np.float64)
    e = np.empty(xyz.size // 3, np.float32)
    for r, (x, y, z) in enumerate(xyz.reshape(-1, 3).astype(np.float64)):
        capi.check(L.wo_noise_point(capi.ptr(perm), capi.ptr(pm12), 1, 5, 0.5, 0.0, 0.0, 1.3 * x, 1.3 * y, 1.3 * z, capi.ptr(out)), "wo_noise_point")
        e[r] = np.float32(out[0] * 1.6 + 0.05)
    return e


def koppen_ids(n: int) -> np.ndarray:
    r = np.arange(n, dtype=np.uint64)
    return (((r * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(31)).astype(np.uint8)


def height_km(e):
    t = np.minimum(e, 1.0)
    return np.where(e <= 0, e * 10, 6 * t ** 4 * (5 - 4 * t))


def sweep_elevations() -> np.ndarray:
    """Every branch boundary of the colour functions and f32 neighbours on both sides, +-0, NaN, infinities, elevations above 1."""
    f = np.float32
    marks = [-0.50, -0.10, 0.0, 0.03, 0.25, 0.50, 0.75, 0.95, 1.0]
    # elevations at which elevToHeightKm crosses the altitude lines of biomeColor (0.2 km, alpine and snow lines, snow line + 2.5)
    for h in (0.2, 0.4, 0.5, 0.8, 1.5, 2.0, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0):
        lo, hi = 0.0, 1.0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if height_km(np.float64(mid)) < h else (lo, mid)
        marks.append(hi)
    vals = []
    for m in marks:
        v = f(m)
        around = [v]
        up = down = v
        for _ in range(2):
            up, down = np.nextafter(up, f(np.inf)), np.nextafter(down, f(-np.inf))
            around += [up, down]
        vals += around
    vals += [f(0.0), f(-0.0), f(np.nan), f(np.inf), f(-np.inf), f(1.5), f(2.0), f(100.0), f(-1.0), f(-5.0), f(1e-30), f(-1e-30), f(0.1), f(0.6), f(0.85)]
    return np.array(vals, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (the directory that holds its js/)")
    args = ap.parse_args()
    gm = np.load(GOLD / f"mesh_N{N}_s{SEED}.npz")
    xyz, tri, he, nreg = gm["xyz"], gm["triangles"], gm["halfedges"], int(gm["numRegions"])
    e, k = elevation(xyz), koppen_ids(nreg)
    assert (e > 0).any() and (e < -0.5).any() and (e > 0.75).any()
    se, sk = sweep_elevations(), np.array(list(range(32)) + [255], np.uint8)
    with tempfile.TemporaryDirectory(prefix="wo_golden_map_") as td:
        work = Path(td)
        ref_js = prepare_reference(Path(args.ref), work)
        three = ref_js.parent / "node_modules" / "three"
        three.mkdir(parents=True)
        (three / "package.json").write_text('{"name":"three","type":"module","main":"three.js","exports":"./three.js"}')
        (three / "three.js").write_text(THREE_STUB)
        (ref_js / "scene.js").write_text(SCENE_STUB)
        pm = ref_js / "planet-mesh.js"
        pm.write_text(pm.read_text() + "\nexport { heightmapColor, landHeightmapColor, landMaskColor, koppenColor, smoothBiomeColors };\n")
        put = lambda name, a: (np.ascontiguousarray(a).tofile(work / name), str(work / name))[1]  # noqa: E731
        job = dict(numRegions=nreg, seed=SEED, width=WIDTH, triangles=put("tri.bin", tri), halfedges=put("he.bin", he), xyz=put("xyz.bin", xyz),
                   elevation=put("e.bin", e), koppen=put("k.bin", k), sweep_e=put("se.bin", se), sweep_k=put("sk.bin", sk), out=str(work / "o_"))
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", str(HARNESS), str(ref_js), str(work / "job.json")], check=True)
        rd = lambda name, ty: np.fromfile(work / f"o_{name}.bin", ty)  # noqa: E731
        data = dict(r_elevation=e, r_koppen=k, sweep_e=se, sweep_k=sk, position_xy=rd("position_xy", np.float32), triRegions=rd("triRegions", np.int32),
                    lut=rd("lut", np.uint8), background_linear=rd("background_linear", np.float32), smooth_small=rd("smooth_small", np.float32))
        for t in TYPES:
            data[f"regionColor_{t}"] = rd(f"regionColor_{t}", np.float32)
            data[f"sweep_{t}"] = rd(f"sweep_{t}", np.float32)
        data["meta_json"] = np.frombuffer((work / "o_meta.json").read_bytes(), np.uint8)
    out = GOLD / f"map_N{N}_s{SEED}.npz"
    np.savez_compressed(out, **data)
    print(f"wrote {out.relative_to(REPO)} ({out.stat().st_size / 1024:.0f} KiB), {data['triRegions'].size} triangles, sweep {se.size} x {sk.size}")


if __name__ == "__main__":
    main()
