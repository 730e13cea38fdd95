"""The contract of the shim's globe-view calls (napi/worogen_napi.cc: viewRaster, viewDepth) that reaches no device: they are callable
properties of the addon that are not enumerable, so the recorded export list of tests/test_node_shim_contract.py stands, and every
check that comes before the planet handle throws the class and the message written down here from the shim's source."""
import json
import shutil
import subprocess

import pytest

from conftest import REPO

NODE = shutil.which("node")
ADDON = REPO / "planet_heightmap_generation_amd" / "worogen.node"
DRIVER = REPO / "tests" / "node" / "run_view_shim_contract.mjs"
pytestmark = pytest.mark.skipif(NODE is None or not ADDON.exists(), reason="node or worogen.node not available")

TYPED, ELEMENT, PLANET = ["TypeError", "expected a typed array"], ["TypeError", "typed array has the wrong element type"], ["TypeError", "expected a planet handle"]
WIDTH, HEIGHT = ["RangeError", "viewRaster: width must be an integer from 1 to 16384"], ["RangeError", "viewRaster: height must be an integer from 1 to 16384"]
EXPORT = dict(type="function", enumerable=False, writable=True, configurable=True, listed=False)
EXPECTED = {
    "export viewRaster": EXPORT, "export viewDepth": EXPORT,
    "viewRaster()": {"thrown": TYPED}, "viewRaster(null)": {"thrown": TYPED}, "viewRaster: triangles no typed array": {"thrown": TYPED},
    "viewRaster: halfedges of another type": {"thrown": ELEMENT},
    "viewRaster: halfedges of another length": {"thrown": ["RangeError", "viewRaster: triangles and halfedges must have the same length, numSides"]},
    **{f"viewRaster: width {w}": {"thrown": WIDTH} for w in ("0", "16385", "2.5", "x")},
    **{f"viewRaster: height {h}": {"thrown": HEIGHT} for h in ("0", "16385", "2.5", "undefined")},
    "viewRaster: odd sizes pass the size checks": {"thrown": PLANET}, "viewRaster: no planet": {"thrown": PLANET},
    "viewDepth()": {"thrown": PLANET}, "viewDepth(null)": {"thrown": PLANET}, "viewDepth({})": {"thrown": PLANET},
}


def test_view_calls_of_the_shim_without_a_device():
    r = subprocess.run([NODE, "--no-warnings", str(DRIVER)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout)
    bad = [f"{k}: expected {json.dumps(EXPECTED.get(k))}, got {json.dumps(got.get(k))}" for k in list(EXPECTED) + [k for k in got if k not in EXPECTED] if got.get(k) != EXPECTED.get(k)]
    assert not bad, "\n".join(bad)
