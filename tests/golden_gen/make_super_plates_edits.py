#!/usr/bin/env python3
"""tests/golden/super_plates_edits_N10000_s1.npz: the outputs of the REFERENCE's buildSuperPlates (js/super-plates.js, run under
Node by run_super_plates.mjs from a scratch copy of that one file) on edits of the inputs of elev_config1_N10000_s1.

Cases (every rule is deterministic; slots are positions in plateSeeds):
  unchanged, all_land, all_ocean                  the plate kinds as they are / all one kind;
  ocean6_to_land, land6_to_ocean                  the first six ocean (land) plates in plateSeeds order change kind;
  random_half                                     the plates picked by default_rng(20240).random(P) < 0.5 change kind;
  P10, P8                                         the first P seeds kept: r_plate relabelled by Jacobi sweeps in which every cell
                                                  of a dropped plate takes the plate of its first neighbour (row order) that has a
                                                  kept plate, until no such cell is left;
  missing_vec_density                             slot 3 has no plateVec entry, slot 5 no density; slots 40.. have no plateVec
                                                  either, so some super plates fall back to [0, 1, 0].
A plate that changes kind takes the density 3.0 + slot / 1024 (now ocean) or 2.7 + slot / 1024 (now land).

Per case the file holds <case>__plateIsOcean, __plateDensity (NaN: undefined), the reference's __r_superPlate, __superPlateVec
(pole + omega per super plate), __superPlateDensity, __superPlateIsOcean, and __r_plate / __plateSeeds / __hasVec where they differ
from config 1's.  The archive is written with fixed member dates: a second run reproduces it byte for byte.

Usage: python tests/golden_gen/make_super_plates_edits.py --ref <reference checkout> [--check]
"""
from __future__ import annotations

import argparse
import io
import json
import shutil
import subprocess
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
GOLD = REPO / "tests" / "golden"
NAME = "super_plates_edits_N10000_s1"
HARNESS = Path(__file__).resolve().parent / "run_super_plates.mjs"


def truncate_plates(off, adj, r_plate, seeds, P):
    keep = np.zeros(int(seeds.max()) + 1, bool)
    keep[seeds[:P]] = True
    rp = r_plate.copy()
    ok = keep[rp]
    while not ok.all():
        nxt, nok = rp.copy(), ok.copy()
        for r in np.flatnonzero(~ok):
            for ni in range(off[r], off[r + 1]):
                if ok[adj[ni]]:
                    nxt[r] = rp[adj[ni]]; nok[r] = True
                    break
        assert nok.sum() > ok.sum()
        rp, ok = nxt, nok
    return rp


def toggled(isoc, dens, pick):
    oc, de = isoc.copy(), dens.copy()
    for s in np.flatnonzero(pick):
        oc[s] = 1 - oc[s]
        de[s] = (3.0 if oc[s] else 2.7) + s / 1024.0
    return oc, de


def cases():
    g = np.load(GOLD / "elev_config1_N10000_s1.npz")
    off, adj, rp, seeds = g["adjOffset"], g["adjList"], g["r_plate"], g["plateSeeds"]
    isoc, dens = g["plateIsOcean"].astype(np.uint8), g["plateDensity"].astype(np.float64)
    P = seeds.size
    slots = np.arange(P)
    out = []

    def add(name, oc, de, r_plate=None, sd=None, has=None):
        out.append(dict(name=name, plateIsOcean=oc, plateDensity=de, r_plate=r_plate, plateSeeds=sd, hasVec=has))
    add("unchanged", isoc, dens)
    add("all_land", *toggled(isoc, dens, isoc == 1))
    add("all_ocean", *toggled(isoc, dens, isoc == 0))
    add("ocean6_to_land", *toggled(isoc, dens, np.isin(slots, np.flatnonzero(isoc == 1)[:6])))
    add("land6_to_ocean", *toggled(isoc, dens, np.isin(slots, np.flatnonzero(isoc == 0)[:6])))
    add("random_half", *toggled(isoc, dens, np.random.default_rng(20240).random(P) < 0.5))
    for k in (10, 8):
        add(f"P{k}", isoc[:k], dens[:k], truncate_plates(off, adj, rp, seeds, k), seeds[:k])
    has = np.ones(P, np.uint8); has[3] = 0; has[40:] = 0
    de = dens.copy(); de[5] = np.nan
    add("missing_vec_density", isoc, de, has=has)
    return g, out


def write_npz(path, arrays):
    """An .npz whose bytes depend on its contents only (fixed member dates, fixed order)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference project (its js/super-plates.js is copied to a scratch directory)")
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    g, cs = cases()
    with tempfile.TemporaryDirectory(prefix="wo_super_") as td:
        work = Path(td)
        (work / "ref").mkdir()
        shutil.copy(Path(args.ref) / "js" / "super-plates.js", work / "ref" / "super-plates.js")
        (work / "ref" / "package.json").write_text('{"type":"module"}')
        P = g["plateSeeds"].size
        g["adjOffset"].astype(np.int32).tofile(work / "adjOffset.bin"); g["adjList"].astype(np.int32).tofile(work / "adjList.bin")
        job = dict(adjOffset=str(work / "adjOffset.bin"), adjList=str(work / "adjList.bin"), cases=[])
        for c in cs:
            pre = str(work / c["name"]) + "_"
            sd = c["plateSeeds"] if c["plateSeeds"] is not None else g["plateSeeds"]
            n = sd.size
            files = dict(r_plate=(c["r_plate"] if c["r_plate"] is not None else g["r_plate"]).astype(np.int32), plateSeeds=sd.astype(np.int32),
                         plateVec=g["plateVec"].astype(np.float64)[:4 * n], hasVec=(c["hasVec"] if c["hasVec"] is not None else np.ones(P, np.uint8))[:n],
                         plateIsOcean=c["plateIsOcean"], plateDensity=c["plateDensity"])
            entry = dict(name=c["name"], out=pre + "o_")
            for k, a in files.items():
                a.tofile(pre + k + ".bin"); entry[k] = pre + k + ".bin"
            job["cases"].append(entry)
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", str(HARNESS), str(work / "ref"), str(work / "job.json")], check=True)
        data = {"cases_json": np.frombuffer(json.dumps([c["name"] for c in cs]).encode(), np.uint8)}
        for c in cs:
            k, pre = c["name"] + "__", str(work / c["name"]) + "_o_"
            data[k + "plateIsOcean"] = c["plateIsOcean"].astype(np.uint8); data[k + "plateDensity"] = c["plateDensity"].astype(np.float64)
            for opt in ("r_plate", "plateSeeds"):
                if c[opt] is not None:
                    data[k + opt] = c[opt].astype(np.int32)
            if c["hasVec"] is not None:
                data[k + "hasVec"] = c["hasVec"].astype(np.uint8)
            for name, dt in (("r_superPlate", np.int32), ("superPlateVec", np.float64), ("superPlateDensity", np.float64), ("superPlateIsOcean", np.uint8)):
                data[k + name] = np.fromfile(pre + name + ".bin", dtype=dt)
        target = work / (NAME + ".npz") if args.check else GOLD / (NAME + ".npz")
        write_npz(target, data)
        if args.check:
            same = target.read_bytes() == (GOLD / (NAME + ".npz")).read_bytes()
            print("reproduces the committed fixture byte for byte" if same else "DIFFERS from the committed fixture")
            sys.exit(0 if same else 1)
        print(f"wrote tests/golden/{NAME}.npz ({target.stat().st_size / 1024:.0f} KiB), super plates per case:",
              {c["name"]: int(data[c["name"] + "__superPlateDensity"].size) for c in cs})


if __name__ == "__main__":
    main()
