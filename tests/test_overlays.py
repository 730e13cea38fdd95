"""The line overlays against the reference's own arrays (tests/golden/overlays_N2000_s1.npz, overlays_crafted.npz; generator:
tools/ref_harness/make_golden_overlays.py): the host emulator of csrc/overlay_ops.h in both forms of the bin winners (the reference's
sequential loop, the minimum of the 64-bit keys) in every word, the two forms against each other on random clusterings, the ITCZ
line and the grids of overlay_export, and the LINES primitives of the binary glTF.  No GPU."""
import json

import numpy as np
import pytest

import globe_common as GC
import map_common as MC
import overlay_common as OC


def same(a, b):
    return MC.same_bits(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32))


def _golden_xyz():
    _, xyz = MC.golden_mesh("mesh_N2000_s1")
    return np.ascontiguousarray(xyz, np.float32)


# ---- 1. the emulator equals the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["loop", "keys"])
def test_emulator_equals_the_references_arrays(form):
    g, xyz = OC.golden(), _golden_xyz()
    meta = g["meta"]
    for pre, kind, season, center in (("wind", OC.WIND, meta["windSeason"], meta["windCenterLon"]), ("ocean", OC.OCEAN, meta["oceanSeason"], meta["oceanCenterLon"])):
        winners, n, arrays = OC.emu_call(kind, xyz, g["r_elevation"], OC.golden_fields(kind, season), center, form)
        assert np.array_equal(winners, g[pre + "_gridRegions"]), pre
        assert n == meta["calls"][pre]["count"] and 0 < n < int((winners >= 0).sum())
        for a, k in zip(arrays, ("globe_position", "globe_color", "map_position", "map_color")):
            bad = np.flatnonzero(~((a.view(np.uint32) == g[f"{pre}_{k}"].view(np.uint32)) | (np.isnan(a) & np.isnan(g[f"{pre}_{k}"]))))
            assert a.size == n * 18 and bad.size == 0, (pre, k, bad.size, (bad[:8] // 18).tolist())
    # the other centre meridian moves the map form alone
    winners, n, arrays = OC.emu_call(OC.WIND, xyz, None, OC.golden_fields(OC.WIND, meta["windSeason"]), meta["windCCenterLon"], form)
    assert same(arrays[2], g["wind_c_map_position"]) and same(arrays[0], g["wind_globe_position"]) and not same(arrays[2], g["wind_map_position"])
    # the ocean form left the land out, the wind form did not
    land = g["r_elevation"] > 0
    assert land[g["wind_gridRegions"][g["wind_gridRegions"] >= 0]].any() and not land[g["ocean_gridRegions"][g["ocean_gridRegions"] >= 0]].any()


def test_golden_holds_the_cases_it_was_made_for():
    g = OC.golden()
    w, o = g["meta"]["planted"]["wind"], g["meta"]["planted"]["ocean"]
    E, Nn = g["field_r_wind_east_summer"].astype(np.float64), g["field_r_wind_north_summer"].astype(np.float64)
    sp = np.sqrt(E * E + Nn * Nn)
    assert (sp[w[:5]] < 0.001).any() and (sp[w[:5]] >= 0.001).any() and np.isnan(sp[w[5]]) and sp[w[6]] == 0 and sp[w[7]] * 3 > 1
    S, Wm = g["field_r_ocean_speed_winter"].astype(np.float64), g["field_r_ocean_warmth_winter"].astype(np.float64)
    assert (S[o[:5]] < 0.01).any() and (S[o[:5]] >= 0.01).any() and np.isnan(S[o[5]])
    assert g["field_r_ocean_current_east_winter"][o[6]] == 0 and g["field_r_ocean_current_north_winter"][o[6]] == 0 and S[o[6]] > 0.01
    assert (Wm[o[8:14]] > 0.1).any() and (Wm[o[8:14]] < -0.1).any() and ((Wm[o[8:14]] <= 0.1) & (Wm[o[8:14]] >= -0.1)).any() and np.isnan(Wm[o[14]])
    for r in w:
        assert r in g["wind_gridRegions"]
    for r in o:
        assert r in g["ocean_gridRegions"]


@pytest.mark.parametrize("form", ["loop", "keys"])
def test_crafted_positions(form):
    c = OC.crafted()
    xyz = c["xyz"]
    winners = OC.emu_winners(xyz, form=form)
    assert np.array_equal(winners, c["gridRegions"])
    idx, d2 = OC.emu_candidates(xyz)
    up = OC.round_kinds(d2)
    copies = lambda r: np.flatnonzero((xyz.view(np.uint32) == xyz[r].view(np.uint32)).all(axis=1))  # noqa: E731
    (a, b) = [li * 120 + lo for li, lo in c["cells"][:2]]
    ra, rb = winners[a], winners[b]
    assert up[ra] and copies(ra).size == 5 and ra == copies(ra)[-1]          # a d2 that rounds up: the last copy wins
    assert not up[rb] and copies(rb).size == 5 and rb == copies(rb)[0]       # one that does not: the first
    assert int((idx < 0).sum()) == 2 and np.isnan(xyz[idx < 0]).any(axis=1).all()
    # the poles, the antimeridian and y above 1 fall into the outermost bands of the reference's floor
    for p, cell in (((0, 1, 0), (59, 59)), ((0, -1, 0), (0, 59)), ((-0.0, 1, -0.0), (59, 0)), ((0.0, 0, -1), (29, 119)), ((-0.0, 0, -1), (29, 0))):
        i, _ = OC.emu_candidates(np.array(p, np.float32))
        assert i[0] == cell[0] * 120 + cell[1], (p, i)
    # (0, 1, 0), (-0, 1, 0) and (0, 1.0000001, 0) have one d2: y is clamped, and -0 changes the sign of dlon alone
    pole = np.flatnonzero((idx == 59 * 120 + 59))
    assert pole.size == 3 and np.unique(d2[pole]).size == 1 and xyz[pole[-1], 1] > 1
    assert winners[59 * 120 + 59] == (pole[-1] if up[pole[0]] else pole[0])


# ---- 2. the key form equals the loop ---------------------------------------------------------------------------------------------------
def test_keys_equal_the_loop_on_the_goldens():
    g, xyz = OC.golden(), _golden_xyz()
    for e, skip in ((None, False), (g["r_elevation"], True)):
        assert np.array_equal(OC.emu_winners(xyz, e, skip, "keys"), OC.emu_winners(xyz, e, skip, "loop"))
    assert np.array_equal(OC.emu_winners(OC.crafted()["xyz"], form="keys"), OC.emu_winners(OC.crafted()["xyz"], form="loop"))


def test_keys_equal_the_loop_on_random_clusterings():
    """200 clusterings of 10 000 points in 1 to 50 bins, a tenth of them copies of other points at random indices.  Points of one bin
    lie close together, so that many share fround(d2); the test counts the bins that the last copy of a position won."""
    rng = np.random.default_rng(7)
    last_copy_won = first_copy_won = 0
    for trial in range(200):
        bins = int(rng.integers(1, 51))
        n = 10000
        idx = rng.integers(0, bins, n).astype(np.int32)
        # d2 as the pass makes it: a sum of two squares of offsets within a 3 degree cell; a coarse lattice of offsets gives equal d2 among strangers too
        step = np.radians(1.5) / rng.choice([8, 64, 4096, 1 << 20])
        off = rng.integers(-int(np.radians(1.5) / step), int(np.radians(1.5) / step) + 1, (n, 2)).astype(np.float64) * step
        d2 = off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]
        dup = rng.choice(n, n // 10, replace=False)
        src = rng.integers(0, n, dup.size)
        idx[dup], d2[dup] = idx[src], d2[src]
        if trial % 10 == 0:
            d2[rng.integers(0, n, 5)] = np.nan                # never a winner
            idx[rng.integers(0, n, 5)] = -1
        loop, keys = OC.emu_pick(idx, d2, bins, "loop"), OC.emu_pick(idx, d2, bins, "keys")
        assert np.array_equal(loop, keys), trial
        up = OC.round_kinds(d2)
        for b in range(bins):
            r = loop[b]
            if r < 0:
                continue
            twins = np.flatnonzero((idx == b) & (d2 == d2[r]))
            if twins.size > 1:
                assert r == (twins[-1] if up[r] else twins[0]), (trial, b)
                last_copy_won += bool(up[r])
                first_copy_won += not up[r]
    print(f"bins decided among identical d2: the last copy won {last_copy_won}, the first {first_copy_won}")
    assert last_copy_won > 0 and first_copy_won > 0


def test_key_rule_on_a_hand_made_bin():
    """fround(d2) equal among different d2: a d2 that rounded up beats every d2 that did not, wherever it stands"""
    m = np.float32(0.001)
    below, above = np.nextafter(np.float64(m), 0.0), np.nextafter(np.float64(m), 1.0)      # both round to m
    assert np.float32(below) == m == np.float32(above)
    for d2, want in (([above, float(m), above], 0), ([above, below, above], 1), ([below, above, below], 2), ([float(m), below, below, above], 2), ([0.5, below], 1)):
        idx = np.zeros(len(d2), np.int32)
        for form in ("loop", "keys"):
            assert OC.emu_pick(idx, np.array(d2), 1, form)[0] == want, (d2, form)


# ---- 3. the host parts -----------------------------------------------------------------------------------------------------------------
def test_itcz_line_and_grids_equal_the_reference():
    from planet_heightmap_generation_amd import overlay_export as OE
    g = OC.golden()
    line = OE.itcz_line(g["field_itczLons"], g["field_itczLatsSummer"])
    assert same(line["globe"], g["itcz_globe"]) and same(line["map"], g["itcz_map"])
    assert line["globe"].size == 360 * 6 and line["map"].size == 359 * 6                # the antimeridian segment is left out of the map form
    for name, spec in g["meta"]["grids"].items():
        got = OE.grids(spec["spacing"], spec["centerLon"])
        assert same(got["globe"], g[name + "_globe"]) and same(got["map"], g[name + "_map"]), name
    assert g["meta"]["opacity"] == {"arrows": OE.ARROW_OPACITY, "mapGrid": OE.GRID_OPACITY, "globeGrid": OE.GRID_OPACITY}
    assert g["meta"]["itczColor"] == 0x00ff88 and OE.ITCZ_COLOR == (0.0, 1.0, 0x88 / 255)
    for bad in (0, -5, float("nan"), float("inf"), 1e-9):
        with pytest.raises(ValueError):
            OE.globe_grid(bad)


def _mesh_dict():
    mesh, xyz, e = GC.golden_case()
    pos, _ = GC.emu_positions(xyz, np.where(np.isfinite(e), e, np.float32(0.2)).astype(np.float32), mesh.triangles, mesh.halfedges)
    wire, _ = GC.emu_lines(GC.WIREFRAME, xyz, np.zeros(e.size, np.float32), mesh.triangles, mesh.halfedges)
    return dict(position=pos, color=GC.golden()["color_default"], bounds=GC.emu_bounds(pos)), wire


def _finite_arrows(pre):
    """the golden's globe arrows without those that hold a NaN (glTF's JSON cannot hold their bounds)"""
    g = OC.golden()
    ok = np.isfinite(g[pre + "_globe_position"].reshape(-1, 18)).all(axis=1)
    return dict(position=g[pre + "_globe_position"].reshape(-1, 18)[ok].reshape(-1), color=g[pre + "_globe_color"].reshape(-1, 18)[ok].reshape(-1))


def test_glb_with_the_overlays():
    from planet_heightmap_generation_amd import globe_export as GE
    from planet_heightmap_generation_amd import overlay_export as OE
    g = OC.golden()
    m, wire = _mesh_dict()
    wind, ocean = _finite_arrows("wind"), _finite_arrows("ocean")
    data = GE.encode_glb(m, wire, wind_arrows=dict(globe=wind, map=None, count=wind["position"].size // 18), ocean_current_arrows=ocean, itcz=g["itcz_globe"], grid=g["grid30_globe"])
    parsed = GC.parse_glb(data)
    doc, arrays = parsed["json"], parsed["arrays"]
    want = [m["position"], m["color"], wire, wind["position"], wind["color"], ocean["position"], ocean["color"], g["itcz_globe"], g["grid30_globe"]]
    assert len(arrays) == len(want) and all(same(a, b) for a, b in zip(arrays, want))
    prims = doc["meshes"][0]["primitives"]
    assert prims[0] == {"attributes": {"POSITION": 0, "COLOR_0": 1}, "mode": 4, "material": 0}
    assert [p["extras"]["name"] for p in prims[1:]] == ["wireframe", "windArrows", "oceanCurrentArrows", "itcz", "grid"] and all(p["mode"] == 1 for p in prims[1:])
    assert [p["attributes"] for p in prims[2:]] == [{"POSITION": 3, "COLOR_0": 4}, {"POSITION": 5, "COLOR_0": 6}, {"POSITION": 7}, {"POSITION": 8}]
    acc = doc["accessors"]
    for p in prims[1:]:
        a = acc[p["attributes"]["POSITION"]]
        assert np.array_equal(np.array(a["min"] + a["max"], np.float32), GC.numpy_bounds(arrays[p["attributes"]["POSITION"]]))
        if "COLOR_0" in p["attributes"]:
            assert "min" not in acc[p["attributes"]["COLOR_0"]] and acc[p["attributes"]["COLOR_0"]]["count"] == a["count"]
    mats = [doc["materials"][p["material"]] for p in prims[2:]]
    assert [x["pbrMetallicRoughness"]["baseColorFactor"] for x in mats] == [[1, 1, 1, 0.6], [1, 1, 1, 0.6], [0, 1, 0x88 / 255, 1], [1, 1, 1, 0.12]]
    assert [x.get("alphaMode") for x in mats] == ["BLEND", "BLEND", None, "BLEND"] and all(x["extensions"] == {"KHR_materials_unlit": {}} for x in mats)
    assert doc["extensionsUsed"] == ["KHR_materials_unlit"] and "extensions" not in doc["materials"][1]
    # an overlay without a segment adds nothing; arrows need their colours, the lines take none
    empty = dict(position=np.empty(0, np.float32), color=np.empty(0, np.float32))
    assert GE.encode_glb(m, wire, wind_arrows=empty, grid=np.empty(0, np.float32)) == GE.encode_glb(m, wire)
    with pytest.raises(ValueError):
        GE.encode_glb(m, wind_arrows=wind["position"])
    with pytest.raises(ValueError):
        GE.encode_glb(m, itcz=wind)
    with pytest.raises(ValueError, match="not finite"):
        GE.encode_glb(m, wind_arrows=dict(position=g["wind_globe_position"], color=g["wind_globe_color"]))
    assert OE.BINS == OC.BINS


def test_glb_without_the_overlays_is_what_it_was():
    """the document of a call without the new arguments, key by key, as tests/test_globe.py expects it of the exporter before the
    overlays existed (its comparison with js/globe-glb.js, which this change does not touch, holds the bytes)"""
    from planet_heightmap_generation_amd import globe_export as GE
    m, wire = _mesh_dict()
    for lines in ((None, None), (wire, None), (wire, wire[: 6 * 37])):
        data = GE.encode_glb(m, *lines)
        assert data == GE.encode_glb(m, *lines, wind_arrows=None, ocean_current_arrows=None, itcz=None, grid=None)
        doc = GC.parse_glb(data)["json"]
        given = [a for a in lines if a is not None]
        assert list(doc) == ["asset", "scene", "scenes", "nodes", "meshes", "materials", "buffers", "bufferViews", "accessors"]
        assert len(doc["accessors"]) == 2 + len(given) == len(doc["bufferViews"]) and len(doc["materials"]) == 1 + len(given)
        assert doc["materials"][0] == {"name": "globe", "pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 1}}
        for j, k in enumerate(GE.LINE_KINDS[: len(given)]):
            assert doc["materials"][1 + j] == {"name": k, "pbrMetallicRoughness": {"baseColorFactor": [0, 0, 0, GE.LINE_OPACITY[k]], "metallicFactor": 0, "roughnessFactor": 1},
                                               "alphaMode": "BLEND"}
            assert doc["meshes"][0]["primitives"][1 + j] == {"attributes": {"POSITION": 2 + j}, "mode": 1, "material": 1 + j, "extras": {"name": k}}
        assert json.dumps(doc).count("KHR_") == 0


# ---- 4. Python and JavaScript give the same bytes --------------------------------------------------------------------------------------
NODE = __import__("shutil").which("node")


@pytest.mark.skipif(NODE is None, reason="node not available")
def test_host_parts_python_equal_js(tmp_path):
    """the ITCZ line, the grids and the GLB with every new primitive: js/overlay-lines.js and js/globe-glb.js (no native code) against
    overlay_export.py and globe_export.py, byte for byte"""
    import subprocess

    from conftest import REPO
    from planet_heightmap_generation_amd import globe_export as GE
    from planet_heightmap_generation_amd import overlay_export as OE
    g = OC.golden()
    m, wire = _mesh_dict()
    wind, ocean = _finite_arrows("wind"), _finite_arrows("ocean")
    for k, a in (("position", m["position"]), ("color", m["color"]), ("bounds", m["bounds"]), ("wire", wire), ("wind_p", wind["position"]), ("wind_c", wind["color"]),
                 ("ocean_p", ocean["position"]), ("ocean_c", ocean["color"]), ("lons", g["field_itczLons"]), ("lats", g["field_itczLatsWinter"])):
        np.ascontiguousarray(a, np.float32).tofile(tmp_path / f"{k}.bin")
    js = (REPO / "planet_heightmap_generation_amd" / "js").as_posix()
    script = tmp_path / "overlays.mjs"
    script.write_text(f"import fs from 'fs';\nimport {{ encodeGlb }} from '{js}/globe-glb.js';\nimport {{ itczLine, globeGrid, mapGrid }} from '{js}/overlay-lines.js';\n"
                      "const dir = process.argv[2];\n"
                      "const rd = (k) => { const b = fs.readFileSync(dir + '/' + k + '.bin'); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };\n"
                      "const wr = (k, a) => fs.writeFileSync(dir + '/' + k, Buffer.from(a.buffer, a.byteOffset, a.byteLength));\n"
                      "const line = itczLine(rd('lons'), rd('lats'));\n"
                      "wr('itcz_globe.out', line.globe); wr('itcz_map.out', line.map);\n"
                      "for (const [tag, s, c] of [['a', 30, 0], ['b', 22.5, 2.5], ['c', 7, -1.25], ['d', 0.7, NaN]]) { wr('grid_' + tag + '_globe.out', globeGrid(s)); wr('grid_' + tag + '_map.out', mapGrid(s, c)); }\n"
                      "const m = { position: rd('position'), color: rd('color'), bounds: rd('bounds') };\n"
                      "const wind = { position: rd('wind_p'), color: rd('wind_c') }, ocean = { position: rd('ocean_p'), color: rd('ocean_c') };\n"
                      "wr('all.glb', encodeGlb(m, { wireframe: rd('wire'), windArrows: { globe: wind, map: null, count: 0 }, oceanCurrentArrows: ocean, itcz: line.globe, grid: globeGrid(30) }));\n"
                      "wr('some.glb', encodeGlb(m, { itcz: line, windArrows: wind }));\n"
                      "wr('plain.glb', encodeGlb(m, { wireframe: rd('wire') }));\n")
    r = subprocess.run([NODE, "--no-warnings", str(script), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = OE.itcz_line(g["field_itczLons"], g["field_itczLatsWinter"])
    rd = lambda k: np.fromfile(tmp_path / k, np.float32)  # noqa: E731
    assert same(rd("itcz_globe.out"), line["globe"]) and same(rd("itcz_map.out"), line["map"]) and line["map"].size == 359 * 6
    for tag, s, c in (("a", 30, 0), ("b", 22.5, 2.5), ("c", 7, -1.25), ("d", 0.7, float("nan"))):
        assert same(rd(f"grid_{tag}_globe.out"), OE.globe_grid(s)) and same(rd(f"grid_{tag}_map.out"), OE.map_grid(s, c)), tag
    assert (tmp_path / "all.glb").read_bytes() == GE.encode_glb(m, wire, wind_arrows=wind, ocean_current_arrows=ocean, itcz=line["globe"], grid=OE.globe_grid(30))
    assert (tmp_path / "some.glb").read_bytes() == GE.encode_glb(m, itcz=line, wind_arrows=wind)
    assert (tmp_path / "plain.glb").read_bytes() == GE.encode_glb(m, wire)
