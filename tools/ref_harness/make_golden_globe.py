#!/usr/bin/env python3
"""Generate tests/golden/globe_N2000_s1.npz by running the REFERENCE's own buildMesh, updateMeshColors and updateSuperPlateBorders
(the globe view, js/planet-mesh.js:620-836, :840-957, :533-576) under Node 12.

As in make_golden_map_layers.py the reference's sources are copied to a scratch directory (oracle/ref_harness/make_golden.py:
prepare_reference) and never enter this repository; in the scratch copy only, that script's stubs of our own stand in for three and
scene.js, here with MeshLambertMaterial added, and run_globe.mjs supplies a document whose chkPlates / chkWire boxes it sets per
run.  Nothing is drawn: the golden holds the arrays buildMesh hands to the renderer.

Recorded, on tests/golden/mesh_N2000_s1.npz with state.mapMode = false:
  * r_elevation: map_N2000_s1.npz's field of both signs with cells at +0, -0, NaN, +inf, -inf and above 1 and two triangles whose
    corners are all +0 / all -0, so that a triangle elevation of each kind occurs; t_elevation as the reference's worker makes it;
  * position: buildMesh's position array (numSides x 9); swapped / swappedSides: the sides whose winding it swapped, told from
    which vertex it stored second (swappedSides 2, not counted: both candidates have the same bits, NaN or infinite ones, and
    the arrays cannot tell);
  * wireframe: the wire mesh's positions; superPlates / borders: a super-plate field with NaN and -0 cells and the border mesh's
    positions for it;
  * color_default: buildMesh's colour array of the default view; layer_field / color_layer: updateMeshColors' for one climate layer;
  * lineOpacity and plateFallback in meta_json.
Running this again reproduces every array exactly.

Usage:  python tools/ref_harness/make_golden_globe.py --ref <checkout of the reference>
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
sys.path.insert(0, str(Path(__file__).resolve().parent))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402
from make_golden_map_layers import SCENE_STUB, THREE_STUB  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_globe.mjs"
N, SEED = 2000, 1
LAYER = "tempSummer"
f32 = np.float32
THREE_GLOBE = THREE_STUB + ("export class MeshLambertMaterial { constructor(opts) { Object.assign(this, opts); } dispose() {} }\n"
                            "export class ShaderMaterial { constructor(opts) { Object.assign(this, opts); } dispose() {} }\n")      # buildGlobeGrid's


def elevation(base: np.ndarray, tri: np.ndarray) -> np.ndarray:
    e = np.ascontiguousarray(base, f32).copy()
    e[5], e[6], e[40], e[80], e[120], e[160] = 0.0, -0.0, np.nan, np.inf, -np.inf, 1.7
    e[tri[3 * 100: 3 * 100 + 3]] = 0.0                      # a triangle elevation of +0 ...
    e[tri[3 * 2000: 3 * 2000 + 3]] = -0.0                   # ... and of -0
    return e


def super_plates(n: int, xyz: np.ndarray) -> np.ndarray:
    """six super plates by octant-like sectors, with NaN cells and a plate 0 that is -0 in places"""
    p = np.asarray(xyz, f32).reshape(-1, 3)
    sp = (np.floor((np.arctan2(p[:, 0], p[:, 2]) + np.pi) / (2 * np.pi) * 3).clip(0, 2) + 3 * (p[:, 1] > 0)).astype(f32)
    sp[::97] = np.nan
    zero = np.flatnonzero(sp == 0)
    sp[zero[::2]] = -0.0
    return sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (the directory that holds its js/)")
    args = ap.parse_args()
    gm = np.load(GOLD / f"mesh_N{N}_s{SEED}.npz")
    g0 = np.load(GOLD / f"map_N{N}_s{SEED}.npz")
    gl = np.load(GOLD / f"map_layers_N{N}_s{SEED}.npz")
    xyz, tri, he, nreg = gm["xyz"], gm["triangles"], gm["halfedges"], int(gm["numRegions"])
    e = elevation(g0["r_elevation"], tri)
    sp = super_plates(nreg, xyz)
    field = np.ascontiguousarray(gl[f"field_{LAYER}"], f32)
    with tempfile.TemporaryDirectory(prefix="wo_golden_globe_") as td:
        work = Path(td)
        ref_js = prepare_reference(Path(args.ref), work)
        three = ref_js.parent / "node_modules" / "three"
        three.mkdir(parents=True)
        (three / "package.json").write_text('{"name":"three","type":"module","main":"three.js","exports":"./three.js"}')
        (three / "three.js").write_text(THREE_GLOBE)
        (ref_js / "scene.js").write_text(SCENE_STUB)
        put = lambda name, a: (np.ascontiguousarray(a).tofile(work / name), str(work / name))[1]  # noqa: E731
        job = dict(numRegions=nreg, seed=SEED, layer=LAYER, triangles=put("tri.bin", tri), halfedges=put("he.bin", he), xyz=put("xyz.bin", xyz),
                   elevation=put("e.bin", e), superPlates=put("sp.bin", sp), layerField=put("field.bin", field), out=str(work / "o_"))
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", str(HARNESS), str(ref_js), str(work / "job.json")], check=True)
        rd = lambda name, ty=np.float32: np.fromfile(work / f"o_{name}.bin", ty)  # noqa: E731
        meta = json.loads((work / "o_meta.json").read_text())
        data = dict(r_elevation=e, t_elevation=rd("t_elevation"), position=rd("position"), swapped=np.int64(meta["swapped"]), swappedSides=rd("swappedSides", np.uint8),
                    wireframe=rd("wireframe"), superPlates=sp, borders=rd("borders"), color_default=rd("color_default"), layer_field=field, color_layer=rd("color_layer"),
                    meta_json=np.frombuffer((work / "o_meta.json").read_bytes(), np.uint8))
    t_e = data["t_elevation"]
    kinds = dict(pos=(t_e > 0).any(), neg=(t_e < 0).any(), pzero=((t_e == 0) & ~np.signbit(t_e)).any(), nzero=((t_e == 0) & np.signbit(t_e)).any(), nan=np.isnan(t_e).any(),
                 pinf=np.isposinf(t_e).any(), ninf=np.isneginf(t_e).any(), above1=(t_e[np.isfinite(t_e)] > 1 / 3).any())
    assert all(kinds.values()), kinds
    assert data["position"].size == tri.size * 9 and data["wireframe"].size == tri.size // 2 * 6 and 0 < data["borders"].size < data["wireframe"].size
    out = GOLD / f"globe_N{N}_s{SEED}.npz"
    np.savez_compressed(out, **data)
    print(f"wrote {out.relative_to(REPO)} ({out.stat().st_size / 1024:.0f} KiB): {tri.size} sides, {meta['swapped']} swapped, {data['borders'].size // 6} border segments")
    assert out.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
