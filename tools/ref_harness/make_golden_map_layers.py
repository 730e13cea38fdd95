#!/usr/bin/env python3
"""Generate tests/golden/map_layers_N2000_s1.npz by running the REFERENCE's own buildMapMesh (the map view, js/planet-mesh.js:200-382)
and its six layer colour functions (:83-172, :506-529) under Node 12.

As in make_golden_map.py the reference's sources are copied to a scratch directory (oracle/ref_harness/make_golden.py:
prepare_reference) and never enter this repository; in the scratch copy only, stubs of our own stand in for three and scene.js
(here with what buildMapMesh, buildMapGrid and updateSuperPlateBorders touch as well: LineSegments, LineBasicMaterial,
Float32BufferAttribute, Group, Mesh.add / .position), planet-mesh.js gets one appended line exporting its six module-private colour
functions, and run_map_layers.mjs supplies a document whose getElementById returns { checked: false }.  Nothing is drawn: the golden
holds what buildMapMesh hands to the renderer and what the functions return.

Recorded, on tests/golden/mesh_N2000_s1.npz with state.mapMode = true:
  * position_c<k>: the position array (x, y per vertex) at state.mapCenterLon = CENTERS[k]; centre 0 is asserted to reproduce
    map_N2000_s1.npz's position_xy bit for bit, and triRegions is asserted to be that file's;
  * field_<layer> / regionColor_<layer>: synthetic fields from fixed seeds that span every branch, and the one colour buildMapMesh
    gives every region for them at centre 0 (recovered through state.mapFaceToSide after checking that a region has one colour);
  * range_<case> / regionColor_range_<case>: the same for five arrays of a generic debug layer, and rangeMinMax_<case>, the range
    restated in the harness with the reference's `<` / `>` loop;
  * sweep_*: every colour function called directly over its branch boundaries and their f32 neighbours, +-0, NaN, infinities.
Running this again reproduces every array exactly.

Usage:  python tools/ref_harness/make_golden_map_layers.py --ref <checkout of the reference>
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

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_map_layers.mjs"
N, SEED = 2000, 1
CENTERS = (1.0, -2.5, float(np.pi))
# the reference's debugLayer names of the climate layers, in the order of WO_MAP_LAYER_CONTINENTALITY .. (include/worogen.h)
LAYERS = ("continentality", "tempSummer", "tempWinter", "precipSummer", "precipWinter", "rainShadowSummer", "rainShadowWinter", "oceanCurrentSummer",
          "oceanCurrentWinter", "pressureSummer", "pressureWinter", "windSpeedSummer", "windSpeedWinter")
RANGE_CASES = ("positive", "negative", "zero", "nan", "inf")
f32 = np.float32

THREE_STUB = """// stub of three (golden generation only): nothing is drawn; geometries keep the arrays they are given
export const DoubleSide = 2;
export class Vector3 { constructor(x = 0, y = 0, z = 0) { this.x = x; this.y = y; this.z = z; } set(x, y, z) { this.x = x; this.y = y; this.z = z; return this; } }
export class Plane { constructor(normal, constant) { this.normal = normal; this.constant = constant; } }
export class Color { constructor(r, g, b) { this.r = r; this.g = g; this.b = b; } }
class Node3 { constructor() { this.children = []; this.position = new Vector3(); this.visible = true; } add(...o) { this.children.push(...o); return this; } remove(o) { this.children = this.children.filter((c) => c !== o); } }
export class Group extends Node3 {}
export class Scene extends Node3 { constructor() { super(); this.background = null; } }
export class BufferAttribute { constructor(array, itemSize) { this.array = array; this.itemSize = itemSize; this.needsUpdate = false; } }
export class Float32BufferAttribute extends BufferAttribute { constructor(array, itemSize) { super(new Float32Array(array), itemSize); } }
export class BufferGeometry {
    constructor() { this.attributes = {}; }
    setAttribute(name, attr) { this.attributes[name] = attr; return this; }
    getAttribute(name) { return this.attributes[name]; }
    dispose() {}
}
export class MeshBasicMaterial { constructor(opts) { Object.assign(this, opts); } dispose() {} }
export class LineBasicMaterial { constructor(opts) { Object.assign(this, opts); } dispose() {} }
export class Mesh extends Node3 { constructor(geometry, material) { super(); this.geometry = geometry; this.material = material; } }
export class LineSegments extends Node3 { constructor(geometry, material) { super(); this.geometry = geometry; this.material = material; } }
export class OrthographicCamera { constructor(...a) { this.frustum = a; this.position = new Vector3(); } lookAt() {} }
export class WebGLRenderTarget { constructor(w, h) { this.width = w; this.height = h; } dispose() {} }
"""
SCENE_STUB = """// stub of scene.js (golden generation only): a renderer that draws nothing
export const renderer = { capabilities: { maxTextureSize: 16384 }, localClippingEnabled: false, render() {}, setRenderTarget() {}, readRenderTargetPixels() {} };
export const scene = { add() {}, remove() {} };
export const waterMesh = {}, atmosMesh = {}, starsMesh = {};
"""


def around(marks, steps=2):
    """every mark as f32 and its `steps` f32 neighbours on both sides"""
    out = []
    for m in marks:
        v = f32(m)
        up = down = v
        out.append(v)
        for _ in range(steps):
            up, down = np.nextafter(up, f32(np.inf)), np.nextafter(down, f32(-np.inf))
            out += [up, down]
    return out


SPECIAL = [f32(0.0), f32(-0.0), f32(np.nan), f32(np.inf), f32(-np.inf), f32(-1.0), f32(1.5), f32(2.0), f32(100.0), f32(-100.0), f32(1e-30), f32(-1e-30), f32(0.1), f32(0.33), f32(0.6), f32(0.85)]


def sweeps() -> dict:
    s = {}
    s["sweep_in_precipitation"] = np.array(around([0.0, 0.25, 0.5, 0.75, 1.0]) + SPECIAL, f32)
    s["sweep_in_rainShadow"] = np.array(around([0.0, 0.01, -0.01, 0.5, -0.5]) + SPECIAL, f32)
    s["sweep_in_continentality"] = np.array(around([0.0, 0.15, 0.4, 0.7, 0.9, 1.0]) + SPECIAL, f32)
    # temperature: the f32 neighbours of (T + 45) / 90 for every threshold T
    s["sweep_in_temperature"] = np.array(around([0.0, 1.0] + [(T + 45.0) / 90.0 for T in (-38, 0, 10, 18, 22, 32, 40)]) + SPECIAL, f32)
    # debugValueToColor(v, min, max) called directly: every pair of bounds with values around 0, +-range and beyond
    v, lo, hi = [], [], []
    for mn, mx in ((-1.0, 1.0), (0.0, 0.0), (-0.0, 0.0), (-2.0, 0.5), (-0.25, 3.0), (0.0, 3.0), (-7.5, 0.0), (-np.inf, 1.0), (0.0, np.inf), (-1e-30, 1e-30), (-3e38, 3e38)):
        r = max(abs(mn), abs(mx)) or 1.0
        vals = around([0.0]) + SPECIAL
        if np.isfinite(r):
            with np.errstate(over="ignore"):               # 2 * 3e38 is +inf as an f32, on purpose
                vals += around([r, -r, r / 2, -r / 2]) + [f32(2 * r), f32(-2 * r)]
        for x in vals:
            v.append(x); lo.append(f32(mn)); hi.append(f32(mx))
    s["sweep_debug_v"], s["sweep_debug_min"], s["sweep_debug_max"] = np.array(v, f32), np.array(lo, f32), np.array(hi, f32)
    # debugValueToColor over the array's own range (finite values and NaN, so that the range stays finite): +-range and neighbours inside
    own = around([0.0, 0.5, -0.5, 1.0, -1.0, 2.5, -2.5]) + [f32(-3.0), f32(np.nextafter(f32(-3.0), f32(0))), f32(2.75), f32(np.nan), f32(-0.0), f32(1e-30), f32(-1e-30), f32(0.75), f32(-1.5)]
    s["sweep_in_debugSelf"] = np.array(own, f32)
    # oceanCurrentColor(warmth, speed, elevation <= 0): warmth x speed x elevation
    w = around([0.05, -0.05, 2.0 / 3.0, -2.0 / 3.0]) + [f32(0.0), f32(-0.0), f32(np.nan), f32(1.0), f32(-1.0), f32(np.inf), f32(-np.inf), f32(0.3), f32(-0.3)]
    sp = around([0.0, 1.0 / 3.0]) + [f32(0.1), f32(0.02), f32(0.5), f32(1.0), f32(np.nan), f32(np.inf), f32(-0.2)]
    el = [f32(-0.0), f32(0.0), f32(1e-30), f32(-1e-30), f32(np.nan), f32(0.4), f32(-0.4)]
    W, S, E = np.meshgrid(np.array(w, f32), np.array(sp, f32), np.array(el, f32), indexing="ij")
    s["sweep_ocean_warmth"], s["sweep_ocean_speed"], s["sweep_ocean_elevation"] = W.reshape(-1).copy(), S.reshape(-1).copy(), E.reshape(-1).copy()
    return s


def fields(n: int, elevation: np.ndarray) -> dict:
    """synthetic per-region fields from fixed seeds; every branch of the layer's colour function is taken by many regions"""
    rng = np.random.default_rng(20241)
    u = lambda lo, hi: rng.uniform(lo, hi, n).astype(f32)  # noqa: E731
    F = {}
    F["continentality"] = u(-0.1, 1.1)
    for k in ("tempSummer", "tempWinter", "precipSummer", "precipWinter"):
        F[k] = u(-0.1, 1.1)
    for k in ("rainShadowSummer", "rainShadowWinter"):
        a = u(-0.8, 0.8)
        a[::7] = u(-0.02, 0.02)[::7]
        F[k] = a
    for season in ("summer", "winter"):
        w = u(-1.0, 1.0)
        w[::5] = u(-0.1, 0.1)[::5]
        sp = u(0.0, 0.6)
        sp[::11] = 0.0
        F[f"r_ocean_warmth_{season}"], F[f"r_ocean_speed_{season}"] = w, sp
    for k in ("pressureSummer", "pressureWinter"):
        F[k] = (rng.normal(size=n) * 8.0 + 1.5).astype(f32)
    for k in ("windSpeedSummer", "windSpeedWinter"):
        F[k] = u(0.0, 1.0)
    for a in F.values():                                     # a few non-finite cells in every field
        a[3], a[17], a[29] = np.nan, np.inf, -np.inf
    assert (elevation > 0).any() and (elevation <= 0).any()
    return F


def range_cases(n: int) -> dict:
    rng = np.random.default_rng(777)
    base = (rng.normal(size=n) * 3.0).astype(f32)
    R = {"positive": np.abs(base) + f32(0.5), "negative": -np.abs(base) - f32(0.25), "zero": np.zeros(n, f32), "nan": base.copy(), "inf": base.copy()}
    R["zero"][5] = -0.0
    R["nan"][::3] = np.nan
    R["inf"][n // 2] = np.inf
    return R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (the directory that holds its js/)")
    args = ap.parse_args()
    gm = np.load(GOLD / f"mesh_N{N}_s{SEED}.npz")
    g0 = np.load(GOLD / f"map_N{N}_s{SEED}.npz")
    xyz, tri, he, nreg = gm["xyz"], gm["triangles"], gm["halfedges"], int(gm["numRegions"])
    e = np.ascontiguousarray(g0["r_elevation"], f32)
    F, R, S = fields(nreg, e), range_cases(nreg), sweeps()
    with tempfile.TemporaryDirectory(prefix="wo_golden_map_layers_") as td:
        work = Path(td)
        ref_js = prepare_reference(Path(args.ref), work)
        three = ref_js.parent / "node_modules" / "three"
        three.mkdir(parents=True)
        (three / "package.json").write_text('{"name":"three","type":"module","main":"three.js","exports":"./three.js"}')
        (three / "three.js").write_text(THREE_STUB)
        (ref_js / "scene.js").write_text(SCENE_STUB)
        pm = ref_js / "planet-mesh.js"
        pm.write_text(pm.read_text() + "\nexport { debugValueToColor, precipitationColor, rainShadowColor, continentalityColor, temperatureColor, oceanCurrentColor };\n")
        put = lambda name, a: (np.ascontiguousarray(a).tofile(work / name), str(work / name))[1]  # noqa: E731
        job = dict(numRegions=nreg, seed=SEED, centers=list(CENTERS), layers=list(LAYERS), rangeCases=list(RANGE_CASES), triangles=put("tri.bin", tri),
                   halfedges=put("he.bin", he), xyz=put("xyz.bin", xyz), elevation=put("e.bin", e), out=str(work / "o_"),
                   fields={k: put(f"f_{k}.bin", a) for k, a in F.items()}, ranges={k: put(f"r_{k}.bin", a) for k, a in R.items()},
                   sweeps={k: put(f"s_{k}.bin", a) for k, a in S.items()})
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", str(HARNESS), str(ref_js), str(work / "job.json")], check=True)
        rd = lambda name, ty=np.float32: np.fromfile(work / f"o_{name}.bin", ty)  # noqa: E731
        data = dict(r_elevation=e, centers=np.array(CENTERS, np.float64), triRegions=rd("triRegions", np.int32))
        assert np.array_equal(rd("position_c0").view(np.uint32), g0["position_xy"].view(np.uint32)), "centre 0 does not reproduce map_N2000_s1.npz"
        assert np.array_equal(data["triRegions"], g0["triRegions"])
        for k in range(len(CENTERS)):
            data[f"position_c{k + 1}"] = rd(f"position_c{k + 1}")
            data[f"triRegions_c{k + 1}"] = rd(f"triRegions_c{k + 1}", np.int32)
        for name, a in F.items():
            data[f"field_{name}"] = a
        for name in LAYERS:
            data[f"regionColor_{name}"] = rd(f"regionColor_{name}")
        for name, a in R.items():
            data[f"range_{name}"] = a
            data[f"regionColor_range_{name}"] = rd(f"regionColor_range_{name}")
            data[f"rangeMinMax_{name}"] = rd(f"rangeMinMax_{name}")
        for name, a in S.items():
            data[name] = a
        for name in ("precipitation", "rainShadow", "continentality", "temperature", "debug", "debugSelf", "ocean"):
            data[f"sweep_{name}"] = rd(f"sweep_{name}")
        data["sweep_debugSelf_minmax"] = rd("sweep_debugSelf_minmax")
        data["meta_json"] = np.frombuffer((work / "o_meta.json").read_bytes(), np.uint8)
    out = GOLD / f"map_layers_N{N}_s{SEED}.npz"
    np.savez_compressed(out, **data)
    print(f"wrote {out.relative_to(REPO)} ({out.stat().st_size / 1024:.0f} KiB), {data['triRegions'].size} triangles at centre 0, "
          + ", ".join(f"{data[f'triRegions_c{k + 1}'].size} at {c:.4f}" for k, c in enumerate(CENTERS)))


if __name__ == "__main__":
    main()
