"""Heightmap import, CPU side: the fdlibm ports and the sampler body against the reference's own outputs (tests/golden,
tools/ref_harness/make_golden_import.py), the component contract on the reference's output, the union-find bodies under
several thread orders, and argument checks that refuse before any device work."""
import json
import shutil
import subprocess

import numpy as np
import pytest

import import_common as IC
from conftest import GOLDEN, REPO, load_golden


def test_fdlibm_ports_equal_v8_math():
    m = np.load(GOLDEN / "math_v8.npz")
    x = np.ascontiguousarray(m["asin_x"])
    out = np.empty_like(x)
    IC.emu().emu_asin(IC.C.c_int64(x.size), IC.ptr(x), IC.ptr(out))
    assert x.size > 20000 and IC.same_bits(out, m["asin_v8"]), int((out.view(np.uint64) != m["asin_v8"].view(np.uint64)).sum())
    y, xx = np.ascontiguousarray(m["atan2_y"]), np.ascontiguousarray(m["atan2_x"])
    out = np.empty_like(y)
    IC.emu().emu_atan2(IC.C.c_int64(y.size), IC.ptr(y), IC.ptr(xx), IC.ptr(out))
    assert y.size > 20000 and IC.same_bits(out, m["atan2_v8"])


@pytest.mark.parametrize("name", IC.IMAGES)
def test_emulated_sampler_equals_reference(name):
    g, mesh = IC.golden(), load_golden("mesh_N10000_s1")
    img = g[f"img_{name}"]
    assert IC.same_bits(IC.emu_sample(mesh["xyz"], img), g[f"ref_sample_{name}_mesh"])
    assert IC.same_bits(IC.emu_sample(g["edge_xyz"], img), g[f"ref_sample_{name}_edge"])


def test_contract_holds_on_reference_output():
    """The reference's deriveSyntheticPlates is 'smallest id of the same-class component' and its lists are ascending restatements."""
    g, mesh = IC.golden(), load_golden("mesh_N10000_s1")
    off, adj = mesh["ref_adjOffset"], mesh["ref_adjList"]
    e = g["done_r_elevation"]
    assert np.array_equal(g["done_r_plate"], IC.host_components(off, adj, e))
    seeds, ocean_seeds = IC.seeds_of(g["done_r_plate"], e)
    assert np.array_equal(g["done_plateSeeds"], seeds) and np.array_equal(g["done_plateIsOcean"], ocean_seeds)
    assert len(seeds) > 10 and 0 < len(ocean_seeds) < len(seeds)
    for got, want in zip(IC.numpy_regions(off, adj, e), (g["done_mountain_r"], g["done_coastline_r"], g["done_ocean_r"])):
        assert np.array_equal(got, want)
    for k, v in (("land", 0.25), ("ocean", -0.5)):
        field = np.full(off.size - 1, v, np.float32)
        assert np.array_equal(g[f"plates_{k}_r_plate"], IC.host_components(off, adj, field))
        assert g[f"plates_{k}_seeds"].tolist() == [0] and g[f"plates_{k}_isOcean"].tolist() == ([0] if k == "ocean" else [])


def test_emulated_union_find_any_order_equals_host():
    import irregular_mesh as IM
    g, mesh = IC.golden(), load_golden("mesh_N10000_s1")
    off, adj, e = mesh["ref_adjOffset"], mesh["ref_adjList"], g["done_r_elevation"]
    want = IC.host_components(off, adj, e)
    for seed in (0, 1, 2, 3):
        assert np.array_equal(IC.emu_components(off, adj, e, seed), want), seed
    hp = IM.hub_mesh(4000, 3, 24)
    rng = np.random.default_rng(5)
    meshes = [hp.mesh, IM.permute_vertices(hp.mesh, hp.xyz, rng.permutation(hp.mesh.adjOffset.size - 1))[0], IM.shuffle_rows(hp.mesh, 7)]
    for m in meshes:
        n = m.adjOffset.size - 1
        for field in (rng.uniform(-1, 1, n).astype(np.float32), np.where(rng.random(n) < 0.7, 0.3, -0.2).astype(np.float32)):
            want = IC.host_components(m.adjOffset, m.adjList, field)
            for seed in (0, 11, 12):
                assert np.array_equal(IC.emu_components(m.adjOffset, m.adjList, field, seed), want)


def test_triangle_centers_equal_reference():
    from planet_heightmap_generation_amd import heightmap_import as HI
    from planet_heightmap_generation_amd import sphere_mesh as SM
    g, mesh = IC.golden(), load_golden("mesh_N10000_s1")
    m = SM.sphere_mesh_from_triangles(g["done_triangles"], g["done_halfedges"], int(mesh["numRegions"]))
    assert IC.same_bits(HI.triangle_centers(m, mesh["xyz"]), g["done_t_xyz"])
    assert IC.same_bits(SM.triangle_elevations(m, g["done_r_elevation"]), g["done_t_elevation"])


def test_python_refuses_bad_images_before_device_work():
    from planet_heightmap_generation_amd import capi
    from planet_heightmap_generation_amd import heightmap_import as HI
    img = np.zeros(8, np.uint8)
    with pytest.raises(ValueError, match="pixels"):
        HI.check_image(img, 3, 2)
    with pytest.raises(ValueError, match="positive"):
        HI.check_image(img, 0, 8)
    with pytest.raises(ValueError, match="2\\^31"):
        HI.check_image(img, 65536, 65536)
    with pytest.raises(TypeError):
        HI.check_image(img.astype(np.float32), 4, 2)
    with pytest.raises(ValueError):
        HI.import_heightmap(100, 0.75, img, 3, 3, {}, seed=1)      # refused before the mesh is built
    L = capi.lib()
    assert L.wo_sample_heightmap(None, capi.ptr(img), 4, 2, None) != 0 and "wo_sample_heightmap" in capi.last_error()
    out = np.zeros(8, np.int32)
    assert L.wo_synthetic_plates(None, capi.ptr(out), capi.ptr(out), None, capi.ptr(out)) != 0
    assert L.wo_classify_regions(None, capi.ptr(out), capi.ptr(out), capi.ptr(out), capi.ptr(out)) != 0
    assert L.wo_triangle_centers(1, None, None, None) != 0 and "wo_triangle_centers" in capi.last_error()


NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"


@pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")
def test_addon_refuses_bad_images(tmp_path):
    """Type and length of the image are checked before the planet handle is looked at (no device needed)."""
    script = tmp_path / "bad.mjs"
    script.write_text(f"""
import addon from '{(REPO / "planet_heightmap_generation_amd" / "js" / "native.js").as_posix()}';
import {{ sampleHeightmap }} from '{(REPO / "planet_heightmap_generation_amd" / "js" / "heightmap-import.js").as_posix()}';
const out = {{}};
const tryit = (k, f) => {{ try {{ f(); out[k] = 'no error'; }} catch (e) {{ out[k] = e.constructor.name + ': ' + e.message; }} }};
tryit('float', () => addon.sampleHeightmap(null, new Float32Array(8), 4, 2, false));
tryit('short', () => addon.sampleHeightmap(null, new Uint8Array(7), 4, 2, false));
tryit('clampedShort', () => addon.sampleHeightmap(null, new Uint8ClampedArray(9), 4, 2, false));
tryit('size', () => addon.sampleHeightmap(null, new Uint8Array(0), 0, 2, false));
tryit('jsType', () => sampleHeightmap({{ numRegions: 4, adjOffset: new Int32Array(5), adjList: new Int32Array(0) }}, new Float32Array(12), [1, 2], 2, 1));
console.log(JSON.stringify(out));
""")
    r = subprocess.run([NODE, "--no-warnings", str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["float"].startswith("TypeError") and out["jsType"].startswith("TypeError"), out
    assert out["short"].startswith("RangeError") and out["clampedShort"].startswith("RangeError") and out["size"].startswith("RangeError"), out
